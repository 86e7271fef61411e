// Host side of the label visualisation (kernels_visualize.hip): the plan of a binary PLY file -- where its vertex block sits and which
// three bytes of a vertex record are the colour -- and the reference's optional label dilation over an adjacency list (util.py:445-454).
// A PLY file is untrusted input: every size is formed in 64-bit arithmetic and held against the file's length, as sgl.cpp does.
#include "sg_common.h"

#include <cerrno>
#include <fcntl.h>
#include <string>
#include <sys/stat.h>
#include <unistd.h>

namespace {

constexpr long long kMaxHeader = 1 << 20;        // bytes of header looked at (ScanNet's are ~350)
constexpr int kMaxProps = 4096;                  // properties of one element

int ply_type_size(const std::string& t) {
    if (t == "char" || t == "uchar" || t == "int8" || t == "uint8") return 1;
    if (t == "short" || t == "ushort" || t == "int16" || t == "uint16") return 2;
    if (t == "int" || t == "uint" || t == "float" || t == "int32" || t == "uint32" || t == "float32") return 4;
    if (t == "double" || t == "float64") return 8;
    return 0;
}

std::vector<std::string> split(const std::string& line) {
    std::vector<std::string> tok;
    size_t i = 0;
    while (i < line.size()) {
        while (i < line.size() && (line[i] == ' ' || line[i] == '\t' || line[i] == '\r')) ++i;
        size_t j = i;
        while (j < line.size() && line[j] != ' ' && line[j] != '\t' && line[j] != '\r') ++j;
        if (j > i) tok.emplace_back(line, i, j - i);
        i = j;
    }
    return tok;
}

bool parse_count(const std::string& s, long long* out) {
    if (s.empty() || s.size() > 18) return false;
    long long v = 0;
    for (char c : s) {
        if (c < '0' || c > '9') return false;
        v = v * 10 + (c - '0');
    }
    *out = v;
    return true;
}

}  // namespace

extern "C" {

int sg_ply_plan(const char* path, long long* h_plan) {
    if (!path || !h_plan) return sg::fail(SG_EINVAL, "sg_ply_plan: null argument");
    for (int i = 0; i < SG_PLY_PLAN_WORDS; ++i) h_plan[i] = 0;
    const int fd = open(path, O_RDONLY | O_CLOEXEC);
    if (fd < 0) return sg::fail(SG_EINVAL, "sg_ply_plan: cannot open %s: %s", path, strerror(errno));
    struct stat sb;
    if (fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode)) { close(fd); return sg::fail(SG_EINVAL, "sg_ply_plan: %s is not a regular file", path); }
    const long long file_len = (long long)sb.st_size;
    std::string head((size_t)std::min(file_len, kMaxHeader), '\0');
    size_t got = 0;
    while (got < head.size()) {
        const ssize_t r = read(fd, &head[got], head.size() - got);
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) break;
        got += (size_t)r;
    }
    close(fd);
    head.resize(got);

    enum { kNone, kVertex, kOther } cur = kNone;  // the element whose properties are being read
    bool first = true, format_ok = false, ended = false, seen_vertex = false, list_before = false;
    long long pos = 0, before_vertex = 0, V = -1, stride = 0, cur_count = 0, cur_stride = 0;
    long long off[3] = {-1, -1, -1};
    int nprops = 0;
    while ((size_t)pos < head.size()) {
        const size_t nl = head.find('\n', (size_t)pos);
        if (nl == std::string::npos) break;      // no complete line left: the header is truncated
        const std::vector<std::string> tok = split(head.substr((size_t)pos, nl - (size_t)pos));
        pos = (long long)nl + 1;
        if (first) {
            if (tok.size() != 1 || tok[0] != "ply") return sg::fail(SG_EINVAL, "sg_ply_plan: %s is not a PLY file", path);
            first = false;
            continue;
        }
        if (tok.empty() || tok[0] == "comment" || tok[0] == "obj_info") continue;
        if (tok[0] == "format") {
            if (tok.size() < 2 || tok[1] != "binary_little_endian")
                return sg::fail(SG_EINVAL, "sg_ply_plan: %s: only binary_little_endian PLY is supported, got %s", path, tok.size() > 1 ? tok[1].c_str() : "nothing");
            format_ok = true;
        } else if (tok[0] == "element") {
            long long count = 0;
            if (tok.size() != 3 || !parse_count(tok[2], &count)) return sg::fail(SG_EINVAL, "sg_ply_plan: %s: malformed element line", path);
            // an element in front of the vertex element shifts the vertex block by its bytes
            if (cur == kOther && !seen_vertex) before_vertex += cur_count * cur_stride;
            if (before_vertex > file_len) break;  // (each term is below 2^55: checked before the next one is added)
            cur_count = cur_stride = 0;
            nprops = 0;
            if (tok[1] == "vertex") {
                if (seen_vertex) return sg::fail(SG_EINVAL, "sg_ply_plan: %s: two vertex elements", path);
                if (list_before) return sg::fail(SG_EINVAL, "sg_ply_plan: %s: an element with a list property in front of the vertex element", path);
                if (count > SG_MAX_POINTS) return sg::fail(SG_EINVAL, "sg_ply_plan: %s: %lld vertices, at most %d are supported", path, count, SG_MAX_POINTS);
                seen_vertex = true;
                cur = kVertex;
                V = count;
            } else {
                if (count > (1ll << 40)) return sg::fail(SG_EINVAL, "sg_ply_plan: %s: element count %lld", path, count);
                cur = kOther;
                cur_count = count;
            }
        } else if (tok[0] == "property") {
            if (cur == kNone) return sg::fail(SG_EINVAL, "sg_ply_plan: %s: a property in front of the first element", path);
            if (++nprops > kMaxProps) return sg::fail(SG_EINVAL, "sg_ply_plan: %s: more than %d properties in one element", path, kMaxProps);
            if (tok.size() >= 2 && tok[1] == "list") {
                if (tok.size() != 5 || !ply_type_size(tok[2]) || !ply_type_size(tok[3])) return sg::fail(SG_EINVAL, "sg_ply_plan: %s: malformed list property", path);
                if (cur == kVertex) return sg::fail(SG_EINVAL, "sg_ply_plan: %s: the vertex element has a list property (%s)", path, tok[4].c_str());
                if (!seen_vertex) list_before = true;
                continue;
            }
            const int size = tok.size() == 3 ? ply_type_size(tok[1]) : 0;
            if (!size) return sg::fail(SG_EINVAL, "sg_ply_plan: %s: malformed property line", path);
            if (cur == kVertex) {
                const int ch = tok[2] == "red" ? 0 : tok[2] == "green" ? 1 : tok[2] == "blue" ? 2 : -1;
                if (ch >= 0) {
                    if (tok[1] != "uchar" && tok[1] != "uint8")
                        return sg::fail(SG_EINVAL, "sg_ply_plan: %s: vertex property %s is %s, not uchar", path, tok[2].c_str(), tok[1].c_str());
                    if (off[ch] >= 0) return sg::fail(SG_EINVAL, "sg_ply_plan: %s: vertex property %s appears twice", path, tok[2].c_str());
                    off[ch] = stride;
                }
                stride += size;
            } else {
                cur_stride += size;
            }
        } else if (tok[0] == "end_header") {
            if (cur == kOther && !seen_vertex) before_vertex += cur_count * cur_stride;
            ended = true;
            break;
        } else {
            return sg::fail(SG_EINVAL, "sg_ply_plan: %s: unknown header line '%s'", path, tok[0].c_str());
        }
    }
    if (first) return sg::fail(SG_EINVAL, "sg_ply_plan: %s is not a PLY file", path);
    if (before_vertex > file_len) return sg::fail(SG_EINVAL, "sg_ply_plan: %s: the elements in front of the vertices exceed the file", path);
    if (!ended) return sg::fail(SG_EINVAL, "sg_ply_plan: %s: truncated PLY header", path);
    if (!format_ok) return sg::fail(SG_EINVAL, "sg_ply_plan: %s: no format line", path);
    if (!seen_vertex) return sg::fail(SG_EINVAL, "sg_ply_plan: %s: no vertex element", path);
    if (off[0] < 0 || off[1] < 0 || off[2] < 0) return sg::fail(SG_EINVAL, "sg_ply_plan: %s: the vertex element lacks red / green / blue", path);
    // V <= 2^20 and stride <= 8 * kMaxProps: the block's size cannot overflow
    const long long vertex_off = pos + before_vertex;
    const long long block = V * stride;
    if (vertex_off > file_len || block > file_len - vertex_off)
        return sg::fail(SG_EINVAL, "sg_ply_plan: %s: %lld vertices of %lld bytes do not fit the file (%lld bytes, vertex block at %lld)", path, V, stride,
                        file_len, vertex_off);
    h_plan[0] = vertex_off;                      // everything in front of the vertex block: header text (+ earlier elements)
    h_plan[1] = V;
    h_plan[2] = stride;
    h_plan[3] = off[0];
    h_plan[4] = off[1];
    h_plan[5] = off[2];
    h_plan[6] = vertex_off + block;              // where the rest of the file starts ...
    h_plan[7] = file_len - (vertex_off + block); // ... and its length
    h_plan[8] = file_len;
    h_plan[9] = pos;                             // length of the header text alone
    return SG_OK;
}

int sg_dilate_labels(int32_t* h_labels, int V, const long long* h_indptr, const int32_t* h_indices) {
    if (V < 0 || (V > 0 && (!h_labels || !h_indptr)) ) return sg::fail(SG_EINVAL, "sg_dilate_labels: bad arguments");
    if (V == 0) return SG_OK;
    const long long E = h_indptr[V];
    if (h_indptr[0] != 0 || E < 0 || (E > 0 && !h_indices)) return sg::fail(SG_EINVAL, "sg_dilate_labels: bad CSR");
    for (int i = 0; i < V; ++i)
        if (h_indptr[i + 1] < h_indptr[i] || h_indptr[i + 1] > E) return sg::fail(SG_EINVAL, "sg_dilate_labels: row pointers not ascending at %d", i);
    for (long long e = 0; e < E; ++e)
        if (h_indices[e] < 0 || h_indices[e] >= V) return sg::fail(SG_EINVAL, "sg_dilate_labels: neighbour %d outside [0, %d)", h_indices[e], V);
    // the sources are fixed before the first propagation (util.py:451), each one then hands on the value it holds at ITS turn (453-454)
    std::vector<uint8_t> source((size_t)V);
    for (int i = 0; i < V; ++i) source[i] = h_labels[i] != -1;
    for (int i = 0; i < V; ++i) {
        if (!source[i]) continue;
        const int32_t l = h_labels[i];
        for (long long e = h_indptr[i]; e < h_indptr[i + 1]; ++e) h_labels[h_indices[e]] = l;
    }
    return SG_OK;
}

}  // extern "C"
