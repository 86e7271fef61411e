// The compact pseudo-label file (`pseudo_labels.sgl`, include/seggroup_hip.h): every label vector of an export directory is a table
// look-up, vec[t][v] = tables[t][seg_of_vertex[v]] (-1 where seg_of_vertex[v] < 0), so the file holds the [nvec,S] tables and the one
// seg_of_vertex array the vectors share -- ~0.38 MB per 150k-vertex / 1.5k-segment scene instead of 8.4 MB of `.npy`.  Host only; also
// built under ASan/UBSan (`make asan`).  The reader treats the file as untrusted: every size is checked in 64-bit arithmetic against
// the file's length before anything is read, and the payload's CRC-32 before anything is handed out.
#include <atomic>
#include <cerrno>
#include <fcntl.h>
#include <string>
#include <sys/stat.h>
#include <sys/uio.h>
#include <unistd.h>

#include "sg_common.h"

namespace {

// header: 48 bytes, little-endian (the only byte order this library runs on)
struct SglHeader {
    char magic[8];            // "SGLABEL\0"
    uint32_t version;         // SG_SGL_VERSION
    uint32_t nvec;            // label vectors (hip.LABEL_NAMES order): 14 ins_infer / train, 6 sem_infer
    uint32_t S;               // over-segments (table columns)
    uint32_t V;               // raw mesh vertices
    uint32_t sov_width;       // bytes per seg_of_vertex entry: 2 when S < 65535 (0xFFFF = -1), else 4 (int32)
    uint32_t reserved0;       // 0
    uint64_t payload_bytes;   // nvec * S * 4 + V * sov_width
    uint32_t crc32;           // CRC-32 (IEEE 802.3, zlib's) of the payload
    uint32_t reserved1;       // 0
};
static_assert(sizeof(SglHeader) == SG_SGL_HEADER_BYTES, "the .sgl header is 48 bytes");
const char kMagic[8] = {'S', 'G', 'L', 'A', 'B', 'E', 'L', 0};

// CRC-32, slicing by 8 (a byte-wise table runs at ~0.5 GB/s: too slow beside the writer pool's other work)
struct CrcTables {
    uint32_t t[8][256];
    CrcTables() {
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
            t[0][i] = c;
        }
        for (uint32_t i = 0; i < 256; ++i)
            for (int s = 1; s < 8; ++s) t[s][i] = (t[s - 1][i] >> 8) ^ t[0][t[s - 1][i] & 0xff];
    }
};
const CrcTables kCrc;

uint32_t crc_update(uint32_t crc, const void* data, size_t n) {
    const uint8_t* p = static_cast<const uint8_t*>(data);
    uint32_t c = ~crc;
    while (n >= 8) {
        uint32_t lo, hi;
        memcpy(&lo, p, 4);
        memcpy(&hi, p + 4, 4);
        lo ^= c;
        c = kCrc.t[7][lo & 0xff] ^ kCrc.t[6][(lo >> 8) & 0xff] ^ kCrc.t[5][(lo >> 16) & 0xff] ^ kCrc.t[4][lo >> 24] ^
            kCrc.t[3][hi & 0xff] ^ kCrc.t[2][(hi >> 8) & 0xff] ^ kCrc.t[1][(hi >> 16) & 0xff] ^ kCrc.t[0][hi >> 24];
        p += 8;
        n -= 8;
    }
    while (n--) c = kCrc.t[0][(c ^ *p++) & 0xff] ^ (c >> 8);
    return ~c;
}

int sov_width_for(int64_t S) { return S < 65535 ? 2 : 4; }

// every size of a header, overflow-checked; SG_OK or SG_EINVAL with the reason
int check_header(const SglHeader& h, const char* path, uint64_t* payload_out) {
    if (memcmp(h.magic, kMagic, 8) != 0) return sg::fail(SG_EINVAL, "%s: not a .sgl pseudo-label file (bad magic)", path);
    if (h.version != SG_SGL_VERSION) return sg::fail(SG_EINVAL, "%s: .sgl version %u (this build reads %d)", path, h.version, SG_SGL_VERSION);
    if (h.nvec < 1 || h.nvec > SG_NUM_LABEL_VECTORS) return sg::fail(SG_EINVAL, "%s: nvec %u outside [1, %d]", path, h.nvec, SG_NUM_LABEL_VECTORS);
    if (h.S < 1 || h.S > (uint32_t)INT32_MAX) return sg::fail(SG_EINVAL, "%s: S %u outside [1, 2^31)", path, h.S);
    if (h.V > (uint32_t)INT32_MAX) return sg::fail(SG_EINVAL, "%s: V %u outside [0, 2^31)", path, h.V);
    if (h.sov_width != (uint32_t)sov_width_for(h.S)) return sg::fail(SG_EINVAL, "%s: seg_of_vertex width %u does not match S %u", path, h.sov_width, h.S);
    if (h.reserved0 || h.reserved1) return sg::fail(SG_EINVAL, "%s: reserved header fields are not zero", path);
    uint64_t tab = 0, sov = 0, total = 0;
    if (__builtin_mul_overflow((uint64_t)h.nvec, (uint64_t)h.S, &tab) || __builtin_mul_overflow(tab, (uint64_t)4, &tab) ||
        __builtin_mul_overflow((uint64_t)h.V, (uint64_t)h.sov_width, &sov) || __builtin_add_overflow(tab, sov, &total))
        return sg::fail(SG_EINVAL, "%s: header sizes overflow", path);
    if (total != h.payload_bytes) return sg::fail(SG_EINVAL, "%s: payload length %llu does not match nvec, S, V (%llu)", path,
                                                  (unsigned long long)h.payload_bytes, (unsigned long long)total);
    *payload_out = total;
    return SG_OK;
}

int read_header(int fd, const char* path, SglHeader* h, uint64_t* payload) {
    struct stat st;
    if (fstat(fd, &st) != 0) return sg::fail(SG_EINVAL, "%s: cannot stat: %s", path, strerror(errno));
    if (!S_ISREG(st.st_mode)) return sg::fail(SG_EINVAL, "%s: not a regular file", path);
    if ((uint64_t)st.st_size < sizeof(SglHeader)) return sg::fail(SG_EINVAL, "%s: truncated .sgl file (%lld bytes)", path, (long long)st.st_size);
    size_t got = 0;
    while (got < sizeof(SglHeader)) {
        const ssize_t r = pread(fd, reinterpret_cast<char*>(h) + got, sizeof(SglHeader) - got, (off_t)got);
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) return sg::fail(SG_EINVAL, "%s: short read of the header", path);
        got += (size_t)r;
    }
    const int rc = check_header(*h, path, payload);
    if (rc < 0) return rc;
    if ((uint64_t)st.st_size - sizeof(SglHeader) != *payload)
        return sg::fail(SG_EINVAL, "%s: file holds %lld payload bytes, the header says %llu (truncated or trailing bytes)", path,
                        (long long)st.st_size - (long long)sizeof(SglHeader), (unsigned long long)*payload);
    return SG_OK;
}

int read_exact(int fd, void* dst, size_t n, off_t off) {
    size_t got = 0;
    while (got < n) {
        const ssize_t r = pread(fd, static_cast<char*>(dst) + got, n - got, off + (off_t)got);
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) return -1;
        got += (size_t)r;
    }
    return 0;
}

std::atomic<unsigned long long> g_tmp_counter{0};

}  // namespace

extern "C" {

int sg_write_sgl(const char* path, const int32_t* h_tables, int nvec, int S, const int32_t* h_seg_of_vertex, int V) {
    if (!path || !h_tables || nvec < 1 || nvec > SG_NUM_LABEL_VECTORS || S < 1 || V < 0 || (V > 0 && !h_seg_of_vertex))
        return sg::fail(SG_EINVAL, "sg_write_sgl: bad arguments");
    const int width = sov_width_for(S);
    std::vector<uint8_t> sov((size_t)V * width);
    if (width == 2) {
        uint16_t* o = reinterpret_cast<uint16_t*>(sov.data());
        for (int v = 0; v < V; ++v) {
            const int32_t s = h_seg_of_vertex[v];
            if (s < -1 || s >= S) return sg::fail(SG_EINVAL, "sg_write_sgl: seg_of_vertex[%d] = %d outside [-1, %d)", v, s, S);
            o[v] = s < 0 ? (uint16_t)0xFFFF : (uint16_t)s;
        }
    } else {
        for (int v = 0; v < V; ++v) {
            const int32_t s = h_seg_of_vertex[v];
            if (s < -1 || s >= S) return sg::fail(SG_EINVAL, "sg_write_sgl: seg_of_vertex[%d] = %d outside [-1, %d)", v, s, S);
        }
        if (V) memcpy(sov.data(), h_seg_of_vertex, (size_t)V * 4);
    }
    const size_t tab_bytes = (size_t)nvec * S * 4;
    SglHeader h;
    memset(&h, 0, sizeof h);
    memcpy(h.magic, kMagic, 8);
    h.version = SG_SGL_VERSION;
    h.nvec = (uint32_t)nvec;
    h.S = (uint32_t)S;
    h.V = (uint32_t)V;
    h.sov_width = (uint32_t)width;
    h.payload_bytes = tab_bytes + sov.size();
    h.crc32 = crc_update(crc_update(0, h_tables, tab_bytes), sov.data(), sov.size());

    // atomically: a temporary name in the same directory, then rename over the final name -- a crashed run leaves a stray temporary,
    // never a truncated file under the name a reader looks for
    const std::string tmp = std::string(path) + ".tmp." + std::to_string((long long)getpid()) + "." + std::to_string(g_tmp_counter++);
    const int fd = open(tmp.c_str(), O_WRONLY | O_CREAT | O_EXCL | O_CLOEXEC, 0666);
    if (fd < 0) return sg::fail(SG_EINVAL, "sg_write_sgl: cannot create %s: %s", tmp.c_str(), strerror(errno));
    struct iovec iov[3] = {{&h, sizeof h}, {(void*)h_tables, tab_bytes}, {sov.data(), sov.size()}};
    int first = 0;
    bool ok = true;
    while (first < 3) {
        const ssize_t w = writev(fd, iov + first, 3 - first);
        if (w < 0) { if (errno == EINTR) continue; ok = false; break; }
        size_t left = (size_t)w;
        while (first < 3 && left >= iov[first].iov_len) { left -= iov[first].iov_len; ++first; }
        if (first < 3) { iov[first].iov_base = (char*)iov[first].iov_base + left; iov[first].iov_len -= left; }
    }
    if (close(fd) != 0) ok = false;
    if (!ok) {
        unlink(tmp.c_str());
        return sg::fail(SG_EINVAL, "sg_write_sgl: short write to %s", tmp.c_str());
    }
    if (renameat(AT_FDCWD, tmp.c_str(), AT_FDCWD, path) != 0) {
        const int e = errno;
        unlink(tmp.c_str());
        return sg::fail(SG_EINVAL, "sg_write_sgl: cannot rename to %s: %s", path, strerror(e));
    }
    return SG_OK;
}

int sg_read_sgl_header(const char* path, int* h_info) {
    if (!path || !h_info) return sg::fail(SG_EINVAL, "sg_read_sgl_header: bad arguments");
    const int fd = open(path, O_RDONLY | O_CLOEXEC);
    if (fd < 0) return sg::fail(SG_EINVAL, "sg_read_sgl_header: cannot open %s: %s", path, strerror(errno));
    SglHeader h;
    uint64_t payload = 0;
    const int rc = read_header(fd, path, &h, &payload);
    close(fd);
    if (rc < 0) return rc;
    h_info[0] = (int)h.version; h_info[1] = (int)h.nvec; h_info[2] = (int)h.S; h_info[3] = (int)h.V; h_info[4] = (int)h.sov_width;
    return SG_OK;
}

int sg_read_sgl(const char* path, int32_t* h_tables, long long tables_capacity, int32_t* h_seg_of_vertex, long long V_capacity) {
    if (!path || !h_tables || tables_capacity < 0 || V_capacity < 0 || (V_capacity > 0 && !h_seg_of_vertex))
        return sg::fail(SG_EINVAL, "sg_read_sgl: bad arguments");
    const int fd = open(path, O_RDONLY | O_CLOEXEC);
    if (fd < 0) return sg::fail(SG_EINVAL, "sg_read_sgl: cannot open %s: %s", path, strerror(errno));
    SglHeader h;
    uint64_t payload = 0;
    int rc = read_header(fd, path, &h, &payload);
    if (rc < 0) { close(fd); return rc; }
    const uint64_t ntab = (uint64_t)h.nvec * h.S;       // <= 14 * 2^31: no overflow (check_header bounded both)
    if (ntab > (uint64_t)tables_capacity || (uint64_t)h.V > (uint64_t)V_capacity) {
        close(fd);
        return sg::fail(SG_EINVAL, "sg_read_sgl: %s needs %llu table and %u vertex entries (capacity %lld / %lld)", path,
                        (unsigned long long)ntab, h.V, tables_capacity, V_capacity);
    }
    std::vector<uint8_t> sov((size_t)h.V * h.sov_width);
    if (read_exact(fd, h_tables, (size_t)ntab * 4, (off_t)sizeof(SglHeader)) != 0 ||
        read_exact(fd, sov.data(), sov.size(), (off_t)(sizeof(SglHeader) + ntab * 4)) != 0) {
        close(fd);
        return sg::fail(SG_EINVAL, "sg_read_sgl: short read of %s", path);
    }
    close(fd);
    const uint32_t crc = crc_update(crc_update(0, h_tables, (size_t)ntab * 4), sov.data(), sov.size());
    if (crc != h.crc32) return sg::fail(SG_EINVAL, "sg_read_sgl: %s: payload CRC-32 %08x, header says %08x (corrupt file)", path, crc, h.crc32);
    const int32_t S = (int32_t)h.S;
    if (h.sov_width == 2) {
        const uint16_t* p = reinterpret_cast<const uint16_t*>(sov.data());
        for (uint32_t v = 0; v < h.V; ++v) {
            const int32_t s = p[v] == 0xFFFF ? -1 : (int32_t)p[v];
            if (s >= S) return sg::fail(SG_EINVAL, "sg_read_sgl: %s: seg_of_vertex[%u] = %d outside [-1, %d)", path, v, s, S);
            h_seg_of_vertex[v] = s;
        }
    } else {
        if (h.V) memcpy(h_seg_of_vertex, sov.data(), (size_t)h.V * 4);
        for (uint32_t v = 0; v < h.V; ++v)
            if (h_seg_of_vertex[v] < -1 || h_seg_of_vertex[v] >= S)
                return sg::fail(SG_EINVAL, "sg_read_sgl: %s: seg_of_vertex[%u] = %d outside [-1, %d)", path, v, h_seg_of_vertex[v], S);
    }
    return SG_OK;
}

}  // extern "C"
