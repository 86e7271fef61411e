"""Per-operator parity on the GPU: every device entry point of include/seggroup_hip.h against its
oracle twin (oracle/cpu_ref.py) on seeded inputs, including the edge cases the reference's own
behaviour defines (tiny clusters, duplicated points, the n<=k kNN rows, trailing-zero FPS fix-up).
Integer outputs bit-exact; floats within 1e-4 (north_star) -- observed ~1e-6."""
import ctypes as C

import numpy as np
import pytest

from conftest import make_fixture_scene

pytestmark = pytest.mark.gpu
TOL = 1e-4


@pytest.fixture(scope="module")
def env(sg_lib):
    import torch
    from seggroup_amd import hip
    hip.require_device()
    return sg_lib, torch, hip


_KEEP = []


def _up(torch, a):
    """Upload and keep alive: a temporary freed right after `.data_ptr()` would be recycled by the
    caching allocator for the very next upload while the kernel still reads it."""
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    _KEEP.append(t)
    if len(_KEEP) > 256:
        torch.cuda.synchronize()
        del _KEEP[:128]
    return t


def _ws(torch, nbytes):
    return torch.zeros(max(int(nbytes), 256), dtype=torch.uint8, device="cuda:0")


def _morton_sort_oracle(data, seg_points, seg_off):
    """NumPy statement of what sg_segment_sort_boxes defines (include/seggroup_hip.h): per over-segment its box [min xyz | max xyz |
    max |p|^2 | 0], the order of its points by (30-bit Morton code inside that box, CSR index) and the boxes of every run of 32
    sorted points.  Every axis is quantised to 10 bits by its own extent unless that is < 1/4 of the largest (then by the largest);
    all arithmetic in float32 like the kernel."""
    f = np.float32
    xyz = data[seg_points, :3].astype(f)
    S = len(seg_off) - 1
    n = np.diff(seg_off)
    seg = np.repeat(np.arange(S), n)
    xx = (xyz[:, 0] * xyz[:, 0] + xyz[:, 1] * xyz[:, 1]) + xyz[:, 2] * xyz[:, 2]
    box = np.zeros((S, 8), f)
    nz = n > 0
    st = seg_off[:-1][nz]
    box[nz, 0:3] = np.minimum.reduceat(xyz, st, axis=0)
    box[nz, 3:6] = np.maximum.reduceat(xyz, st, axis=0)
    box[nz, 6] = np.maximum.reduceat(xx, st)
    e = box[:, 3:6] - box[:, 0:3]
    emax = e.max(axis=1, keepdims=True)
    ext = np.where(e >= f(0.25) * emax, e, emax)[seg]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(ext > 0, (xyz - box[seg, 0:3]) / ext, f(0)).astype(f)
    q = np.minimum(np.maximum(t * f(1023.0), f(0)), f(1023.0)).astype(np.uint32)

    def spread(v):
        v = v & 0x3ff
        v = (v | (v << 16)) & 0x030000ff
        v = (v | (v << 8)) & 0x0300f00f
        v = (v | (v << 4)) & 0x030c30c3
        return (v | (v << 2)) & 0x09249249
    m = spread(q[:, 0]) | (spread(q[:, 1]) << 1) | (spread(q[:, 2]) << 2)
    idx = np.arange(len(seg))
    sperm = np.lexsort((idx, m, seg)).astype(np.int32)
    sx, sxx = xyz[sperm], xx[sperm]
    chunk_off = np.concatenate([[0], np.cumsum((n + 31) // 32)])
    cstart = np.concatenate([seg_off[s] + 32 * np.arange((n[s] + 31) // 32) for s in range(S)]).astype(np.int64) if S else np.zeros(0, np.int64)
    cbox = np.zeros((int(chunk_off[-1]), 8), f)
    if len(cstart):
        cbox[:, 0:3] = np.minimum.reduceat(sx, cstart, axis=0)
        cbox[:, 3:6] = np.maximum.reduceat(sx, cstart, axis=0)
        cbox[:, 6] = np.maximum.reduceat(sxx, cstart)
    return box, sperm, cbox



def _layer_arrays(layer):
    """member CSR of an oracle Layer"""
    members = np.concatenate(layer.members).astype(np.int32)
    off = np.zeros(layer.count + 1, np.int32)
    np.cumsum([len(m) for m in layer.members], out=off[1:])
    return members, off


def _tiles(off, width=256):
    tc, lo, hi, cto = [], [], [], [0]
    for c in range(len(off) - 1):
        for s in range(off[c], off[c + 1], width):
            tc.append(c); lo.append(s); hi.append(min(s + width, off[c + 1]))
        cto.append(len(tc))
    return (np.array(tc, np.int32), np.array(lo, np.int32), np.array(hi, np.int32), np.array(cto, np.int32))


def test_contract_point_edges_matches_update_adj(env, golden_index):
    lib, torch, hip = env
    from oracle import cpu_ref as O
    sc = make_fixture_scene(golden_index, "small_20k")
    part = O.Partition(sc.weak_label[:, 1], sc.weak_label[:, 0], sc.seg)
    ref = O.contract_edges(sc.adj, part, np.arange(sc.num_points), O.Layer(part))
    S = sc.num_segments
    d_adj, d_seg = _up(torch, sc.adj), _up(torch, sc.seg)
    out = torch.zeros(sc.adj.shape[0], 2, dtype=torch.int32, device="cuda:0")
    cnt = torch.zeros(4, dtype=torch.int32, device="cuda:0")
    ws = _ws(torch, lib.sg_contract_ws_bytes(S))
    hip.check(lib.sg_contract_point_edges(d_adj.data_ptr(), sc.adj.shape[0], d_seg.data_ptr(), sc.num_points, S, out.data_ptr(),
                                          out.shape[0], cnt.data_ptr(), ws.data_ptr(), ws.numel(), None))
    n = int(cnt[0].item())
    assert n == ref.shape[0]
    assert np.array_equal(out[:n].cpu().numpy(), ref.astype(np.int32))
    # empty edge list -> zero rows (the reference returns a 1-D empty tensor)
    hip.check(lib.sg_contract_point_edges(d_adj.data_ptr(), 0, d_seg.data_ptr(), sc.num_points, S, out.data_ptr(), out.shape[0],
                                          cnt.data_ptr(), ws.data_ptr(), ws.numel(), None))
    assert int(cnt[0].item()) == 0


def _fps_case(env, data, layer, P, ch_out, transform):
    lib, torch, hip = env
    members, off = _layer_arrays(layer)
    N = data.shape[0]
    d_data, d_m, d_o = _up(torch, data), _up(torch, members), _up(torch, off)
    out = torch.zeros(layer.count, P, ch_out, device="cuda:0")
    sel = torch.zeros(layer.count, P, dtype=torch.int32, device="cuda:0")
    ws = _ws(torch, lib.sg_fps_ws_bytes(N))
    hip.check(lib.sg_fps_sample(d_data.data_ptr(), N, data.shape[1], d_m.data_ptr(), d_o.data_ptr(), layer.count, P, ch_out, transform,
                                out.data_ptr(), sel.data_ptr(), ws.data_ptr(), ws.numel(), None))
    torch.cuda.synchronize()
    return out.cpu().numpy(), sel.cpu().numpy()


def test_fps_sample_layer1_exact_picks(env, golden_index):
    from oracle import cpu_ref as O
    for name in ("tiny_4k", "tiny_dup_4k"):
        sc = make_fixture_scene(golden_index, name)
        part = O.Partition(sc.weak_label[:, 1], sc.weak_label[:, 0], sc.seg)
        L = O.Layer(part)
        ref, ref_sel = O.sample_clusters(sc.data, L, 64, transform=True)
        out, sel = _fps_case(env, sc.data, L, 64, 6, 1)
        assert np.array_equal(sel, ref_sel.astype(np.int32)), name        # integer picks: bit-exact
        assert np.abs(out - ref).max() < 1e-5


def test_fps_sample_edge_cases(env):
    """tiny clusters (n < P: tiling + remainder), n == P, exact duplicates forcing the trailing-zero
    fix-up (probe fixture of SURVEY 8c: picks [4,0,1,0] -> [4,0,1,4]), a cluster larger than the LDS carve."""
    from oracle import cpu_ref as O
    rng = np.random.default_rng(5)
    blocks = [np.array([[0, 0, 0], [1, 0, 0], [1, 0, 0], [0, 0, 0], [2, 0, 0]], np.float32),      # SURVEY quirk fixture
              rng.uniform(0, 1, (3, 3)).astype(np.float32),
              rng.uniform(0, 1, (64, 3)).astype(np.float32),
              np.repeat(rng.uniform(0, 1, (4, 3)).astype(np.float32), 5, axis=0),                   # heavy duplicates
              rng.uniform(0, 3, (9000, 3)).astype(np.float32),                                      # > kLdsCap, global path
              rng.uniform(0, 3, (2500, 3)).astype(np.float32)]                                      # 16-wave class in LDS
    xyz = np.concatenate(blocks)
    data = np.concatenate([xyz, rng.uniform(-1, 1, (xyz.shape[0], 3)).astype(np.float32)], axis=1)
    seg = np.concatenate([np.full(len(b), i) for i, b in enumerate(blocks)])

    class L:  # minimal Layer
        pass
    layer = L()
    layer.members = [np.nonzero(seg == i)[0] for i in range(len(blocks))]
    layer.count = len(blocks)
    # the quirk fixture asks for k=4 picks out of 5 points: P = 9 -> rep 1, rem 4
    assert O.fps_with_fixup(blocks[0], 4).tolist() == [4, 0, 1, 4]
    for P, ch, tr in ((9, 6, 0), (64, 6, 1), (1024, 3, 0)):
        ref, ref_sel = O.sample_clusters(data[:, :max(ch, 3)] if ch == 3 else data, layer, P, transform=bool(tr))
        out, sel = _fps_case(env, data, layer, P, ch, tr)
        for c in range(layer.count):
            assert np.array_equal(sel[c], ref_sel[c].astype(np.int32)), (P, ch, tr, c, len(layer.members[c]),
                                                                          np.nonzero(sel[c] != ref_sel[c])[0][:8])
        ok = np.isfinite(ref)
        assert np.abs(out[ok] - ref[ok]).max() < 1e-5


def test_mlp1_forward(env, golden_index, weight_sets):
    lib, torch, hip = env
    from oracle import cpu_ref as O
    sc = make_fixture_scene(golden_index, "tiny_dup_4k")
    W = weight_sets["ins_infer"]
    part = O.Partition(sc.weak_label[:, 1], sc.weak_label[:, 0], sc.seg)
    samples, _ = O.sample_clusters(sc.data, O.Layer(part), 64, transform=True)
    ref = O.mlp1_forward(samples, W)
    C_ = samples.shape[0]
    d_s = _up(torch, samples)
    out = torch.zeros(C_, 128, device="cuda:0")
    ws = _ws(torch, lib.sg_mlp1_ws_bytes(C_))
    w, g, b = (_up(torch, W[k]) for k in ("mlp_1.conv1.0.weight", "mlp_1.bn1.weight", "mlp_1.bn1.bias"))
    hip.check(lib.sg_mlp1_forward(d_s.data_ptr(), C_, w.data_ptr(), g.data_ptr(), b.data_ptr(), out.data_ptr(), 128, ws.data_ptr(),
                                  ws.numel(), None))
    assert np.abs(out.cpu().numpy() - ref).max() < TOL


def test_edge_distance_and_group_max(env):
    lib, torch, hip = env
    from oracle import cpu_ref as O
    rng = np.random.default_rng(3)
    for D in (4, 128, 192, 256):
        S, E = 300, 1500
        f = rng.normal(size=(S, D)).astype(np.float32)
        adj = rng.integers(0, S, (E, 2)).astype(np.int32)
        adj[0] = (5, 5)                                   # pairwise_distance(x, x) = sqrt(D) * 1e-6
        ref = O.edge_distance(f, adj)
        d_f, d_a = _up(torch, f), _up(torch, adj)
        out = torch.zeros(E, device="cuda:0")
        hip.check(lib.sg_edge_distance(d_f.data_ptr(), D, D, d_a.data_ptr(), E, out.data_ptr(), None))
        got = out.cpu().numpy()
        assert np.abs(got - ref).max() < 1e-5
        assert abs(got[0] - np.sqrt(D) * 1e-6) < 1e-9
    # aggregate_cluster_feature
    groups = [list(rng.choice(300, size=rng.integers(1, 9), replace=False)) for _ in range(40)]
    goff = np.zeros(41, np.int32)
    np.cumsum([len(g) for g in groups], out=goff[1:])
    gidx = np.concatenate(groups).astype(np.int32)
    ref = O.group_max(f, groups)
    out = torch.zeros(40, 300, device="cuda:0")
    hip.check(lib.sg_group_max_rows(d_f.data_ptr(), 256, 256, _up(torch, goff).data_ptr(), _up(torch, gidx).data_ptr(), 40,
                                    out.data_ptr(), 300, None))
    assert np.array_equal(out.cpu().numpy()[:, :256], ref)


def _semantic_inputs(sc, nclusters_target):
    """A layer with merged clusters (random unions in oracle Partition) incl. tiny clusters."""
    from oracle import cpu_ref as O
    part = O.Partition(sc.weak_label[:, 1], sc.weak_label[:, 0], sc.seg)
    roots = part.roots()
    rng = np.random.default_rng(9)
    while len(part.roots()) > nclusters_target:
        r = part.roots()
        a, b = rng.choice(len(r), 2, replace=False)
        part.ins[r[a]] = -1                                 # bypass the label veto for this synthetic merge
        part.union(r[a], r[b])
    return part, O.Layer(part)


def test_center_knn_segmax_pipeline_ops(env, golden_index):
    """sg_center_clusters + sg_cluster_knn + sg_segment_max on a layer with clusters of 1..>1024 points."""
    lib, torch, hip = env
    from oracle import cpu_ref as O
    sc = make_fixture_scene(golden_index, "tiny_dup_4k")
    part, L = _semantic_inputs(sc, 5)
    # add tiny clusters: split three single points / a 7-point and a 20-point group off as their own clusters
    members, off = _layer_arrays(L)
    sizes = np.diff(off).tolist()
    big = int(np.argmax(sizes))
    cut = [1, 1, 7, 20, 21]
    new_members, new_sizes = [], []
    for c, m in enumerate(L.members):
        if c == big:
            pos = 0
            for k in cut:
                new_members.append(m[pos:pos + k]); pos += k
            new_members.append(m[pos:])
        else:
            new_members.append(m)

    class L2:
        pass
    layer = L2()
    layer.members = new_members
    layer.count = len(new_members)
    members, off = _layer_arrays(layer)
    N = sc.num_points
    tc, lo, hi, cto = _tiles(off)
    d = {k: _up(torch, v) for k, v in dict(data=sc.data, members=members, off=off, tc=tc, lo=lo, hi=hi, cto=cto).items()}
    x9m = torch.zeros(N, 12, device="cuda:0")
    xyzw = torch.zeros(N, 4, device="cuda:0")
    ws = _ws(torch, lib.sg_center_ws_bytes(len(tc), layer.count))
    hip.check(lib.sg_center_clusters(d["data"].data_ptr(), N, d["members"].data_ptr(), d["off"].data_ptr(), layer.count,
                                     d["tc"].data_ptr(), d["lo"].data_ptr(), d["hi"].data_ptr(), len(tc), d["cto"].data_ptr(),
                                     x9m.data_ptr(), xyzw.data_ptr(), ws.data_ptr(), ws.numel(), None))
    ref9 = O.centre_per_cluster(sc.data, layer)
    got9 = x9m.cpu().numpy()
    assert np.array_equal(got9[:, :6], sc.data[members])
    assert np.abs(got9[:, 6:9] - ref9[members, 6:9]).max() < 2e-6
    assert np.all(got9[:, 9:] == 0)

    pos_of_point = np.empty(N, np.int64)
    pos_of_point[members] = np.arange(N)
    knn = torch.zeros(N, 20, dtype=torch.int32, device="cuda:0")
    hip.check(lib.sg_cluster_knn(xyzw.data_ptr(), N, d["off"].data_ptr(), d["tc"].data_ptr(), d["lo"].data_ptr(), d["hi"].data_ptr(),
                                 len(tc), 20, int(pos_of_point[0]), knn.data_ptr(), None))
    got = members[knn.cpu().numpy()]                       # positions -> point ids, rows in member order
    ref = O.cluster_knn(sc.data[:, :3], layer, 20)[members]
    # clusters with n <= 20: exact rows including the "column stays 0 = global point 0" quirk
    small = np.concatenate([np.arange(off[c], off[c + 1]) for c in range(layer.count) if off[c + 1] - off[c] <= 20])
    assert small.size > 0 and np.array_equal(got[small], ref[small])
    # big clusters: neighbour SETS equal except for exact-tie rows (duplicated points): compare the scores instead
    diff = np.nonzero(np.any(np.sort(got, 1) != np.sort(ref, 1), axis=1))[0]
    xyz = sc.data[:, :3]
    for r in diff:
        q = xyz[members[r]][None]
        sg_, sr_ = np.sort(O.knn_scores(q, xyz[got[r]])[0]), np.sort(O.knn_scores(q, xyz[ref[r]])[0])
        assert np.array_equal(sg_, sr_), f"row {r}: different neighbour scores"
    # first neighbour is the query itself or an exact duplicate of it
    big_rows = np.setdiff1d(np.arange(N), small)
    assert np.all(xyz[got[big_rows, 0]] == xyz[members[big_rows]])

    # segment max
    rng = np.random.default_rng(2)
    rows = rng.normal(size=(N, 64)).astype(np.float32)
    cl_of_pos = np.repeat(np.arange(layer.count), np.diff(off)).astype(np.int32)
    out = torch.zeros(layer.count, 192, device="cuda:0")
    hip.check(lib.sg_segment_max(_up(torch, rows).data_ptr(), N, 64, _up(torch, cl_of_pos).data_ptr(), out[:, 128:].data_ptr(), 192,
                                 layer.count, None))
    ref = np.stack([rows[off[c]:off[c + 1]].max(0) for c in range(layer.count)])
    assert np.array_equal(out.cpu().numpy()[:, 128:], ref)


@pytest.mark.parametrize("N", [4000, 4001, 37])
def test_edgeconv_forward(env, N):
    lib, torch, hip = env
    from oracle import cpu_ref as O
    from seggroup_amd import weights
    rng = np.random.default_rng(N)
    K = 20
    x9 = rng.uniform(-1, 1, (N, 9)).astype(np.float32)
    x9[:, :3] *= 4
    knn = rng.integers(0, N, (N, K)).astype(np.int32)
    W = weights.make_weights(1, 2.0, affine_jitter=0.3)
    W["mlp_3.bn2.weight"][::7] *= -1.0                      # negative gamma: the kernel keeps max_k of sgn(gamma)*y
    W["mlp_2.bn1.weight"][::5] *= -1.0
    W["mlp_3.bn1.weight"][::3] *= -1.0                      # inner BN (folded into conv1's weights)
    W["mlp_3.bn2.weight"][9] = 0.0                          # gamma == 0: the channel is LReLU(beta) everywhere
    W["mlp_2.bn1.weight"][11] = 0.0
    x12 = np.zeros((N, 12), np.float32)
    x12[:, :9] = x9
    d_x, d_k = _up(torch, x12), _up(torch, knn)
    for layers, which in ((1, "mlp_2"), (2, "mlp_3")):
        ws = _ws(torch, lib.sg_edgeconv_ws_bytes(N))
        out = torch.zeros(N, 64, device="cuda:0")
        t = {k: _up(torch, W[k]) for k in W}
        p2 = (t["mlp_3.conv2.0.weight"].data_ptr(), t["mlp_3.bn2.weight"].data_ptr(), t["mlp_3.bn2.bias"].data_ptr()) if layers == 2 \
            else (None, None, None)
        hip.check(lib.sg_edgeconv_forward(d_x.data_ptr(), d_k.data_ptr(), N, K, layers, t[f"{which}.conv1.0.weight"].data_ptr(),
                                          t[f"{which}.bn1.weight"].data_ptr(), t[f"{which}.bn1.bias"].data_ptr(), *p2, out.data_ptr(),
                                          ws.data_ptr(), ws.numel(), None))
        ref = O.edgeconv_forward(x9, knn.astype(np.int64), W, which)
        assert np.abs(out.cpu().numpy() - ref).max() < 2e-5, which
        # the ranged entry: conv1's operand on fp16 pieces scaled by the range word (MLP2), the word cleared afterwards
        rng_bits = torch.zeros(256, dtype=torch.int32, device="cuda:0")
        hip.check(lib.sg_edge_range(d_x.data_ptr(), N, rng_bits.data_ptr(), None))
        assert rng_bits.cpu().numpy().view(np.float32).max() == np.abs(x9 - x9[0]).max()
        out2 = torch.zeros(N, 64, device="cuda:0")
        hip.check(lib.sg_edgeconv_forward_r(d_x.data_ptr(), d_k.data_ptr(), N, K, layers, t[f"{which}.conv1.0.weight"].data_ptr(),
                                            t[f"{which}.bn1.weight"].data_ptr(), t[f"{which}.bn1.bias"].data_ptr(), *p2, out2.data_ptr(),
                                            ws.data_ptr(), ws.numel(), rng_bits.data_ptr(), None))
        assert np.abs(out2.cpu().numpy() - ref).max() < 2e-5, which
        assert int(rng_bits.cpu().abs().sum()) == 0


@pytest.mark.parametrize("spread,offset", [(1e-3, 0.0), (50.0, 0.0), (4.0, 900.0), (1e-6, 3.0)])
def test_edgeconv_fp16_conv1_ranges(env, spread, offset):
    """MLP2's conv1 on fp16 pieces (sg_edgeconv_forward_r): clouds of 1 mm, 50 m and 4 m extent -- the last 900 m from the origin -- and one
    that is constant up to 1e-6: the power-of-two scale keeps the pieces inside fp16 whatever the data's magnitude (a difference can be
    1e-6 of the range: it lands on fp16 subnormals, which the matrix pipe keeps), the result stays within 2e-5 of the float64 oracle (3e-5 for the near-constant cloud)."""
    lib, torch, hip = env
    from oracle import cpu_ref as O
    from seggroup_amd import weights
    N, K = 3000, 20
    rng = np.random.default_rng(7)
    x9 = (rng.uniform(-1, 1, (N, 9)) * spread).astype(np.float32)
    x9[:, :3] += np.float32(offset)
    x9[:, 6:9] = x9[:, :3] - x9[:, :3].mean(0)                       # centred copy, like the layout kernel writes it
    x9[1, 3] += np.float32(spread * 1e-6)                            # a tiny difference beside the large ones
    knn = rng.integers(0, N, (N, K)).astype(np.int32)
    W = weights.make_weights(1, 2.0, affine_jitter=0.3)
    x12 = np.zeros((N, 12), np.float32)
    x12[:, :9] = x9
    d_x, d_k = _up(torch, x12), _up(torch, knn)
    t = {k: _up(torch, W[k]) for k in W}
    ws = _ws(torch, lib.sg_edgeconv_ws_bytes(N))
    out = torch.zeros(N, 64, device="cuda:0")
    rng_bits = torch.zeros(256, dtype=torch.int32, device="cuda:0")
    hip.check(lib.sg_edge_range(d_x.data_ptr(), N, rng_bits.data_ptr(), None))
    hip.check(lib.sg_edgeconv_forward_r(d_x.data_ptr(), d_k.data_ptr(), N, K, 1, t["mlp_2.conv1.0.weight"].data_ptr(), t["mlp_2.bn1.weight"].data_ptr(),
                                        t["mlp_2.bn1.bias"].data_ptr(), None, None, None, out.data_ptr(), ws.data_ptr(), ws.numel(), rng_bits.data_ptr(), None))
    ref = O.edgeconv_forward(x9, knn.astype(np.int64), W, "mlp_2")
    assert np.isfinite(out.cpu().numpy()).all()
    assert np.abs(out.cpu().numpy() - ref).max() < 2e-5
    # MLP3's conv1' the same way (the fp16 image and its scale come out of k_bn_fold_moments)
    hip.check(lib.sg_edge_range(d_x.data_ptr(), N, rng_bits.data_ptr(), None))
    hip.check(lib.sg_edgeconv_forward_r(d_x.data_ptr(), d_k.data_ptr(), N, K, 2, t["mlp_3.conv1.0.weight"].data_ptr(), t["mlp_3.bn1.weight"].data_ptr(),
                                        t["mlp_3.bn1.bias"].data_ptr(), t["mlp_3.conv2.0.weight"].data_ptr(), t["mlp_3.bn2.weight"].data_ptr(),
                                        t["mlp_3.bn2.bias"].data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(), rng_bits.data_ptr(), None))
    ref = O.edgeconv_forward(x9, knn.astype(np.int64), W, "mlp_3")
    assert np.isfinite(out.cpu().numpy()).all()
    # the cloud that is constant up to 1e-6 normalises by a standard deviation of ~1e-6 of the values: how a tile's fp32 partial sums are
    # associated shows there first (2.2e-5 with the halving cross-lane reduction of round 4, 1.9e-5 with the chains before it)
    assert np.abs(out.cpu().numpy() - ref).max() < (3e-5 if spread < 1e-5 else 2e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [31, 4096 + 17, 50_000])
def test_edgeconv_hand_scheduled_slot_loop_equals_compiler_loop(env, N):
    """The K = 20 neighbour-slot loop runs as a hand-scheduled instruction stream (csrc/edgeconv_slots_gen.h, tools/gen_edgeconv_asm.py);
    the compiler-scheduled C++ loop it replaces stays in the library (other K, SG_EDGECONV_COMPILER_LOOP).  Both issue the same
    operations on the same values in the same order per accumulator: outputs and therefore every label must be BIT-identical, for
    MLP2 and MLP3, tail tiles, duplicate neighbours and a far-away cloud included."""
    lib, torch, hip = env
    from seggroup_amd import weights
    rng = np.random.default_rng(1000 + N)
    K = 20
    x9 = rng.uniform(-1, 1, (N, 9)).astype(np.float32)
    x9[:, :3] = x9[:, :3] * 4 + np.float32(37.5)
    x9[:, 6:9] = x9[:, :3] - x9[:, :3].mean(0)
    knn = rng.integers(0, N, (N, K)).astype(np.int32)
    knn[::3, 5:] = knn[::3, 4:5]                              # short clusters: repeated neighbours
    W = weights.make_weights(1, 2.0, affine_jitter=0.3)
    W["mlp_3.bn2.weight"][::7] *= -1.0
    W["mlp_2.bn1.weight"][::5] *= -1.0
    x12 = np.zeros((N, 12), np.float32)
    x12[:, :9] = x9
    d_x, d_k = _up(torch, x12), _up(torch, knn)
    t = {k: _up(torch, W[k]) for k in W}
    ws = _ws(torch, lib.sg_edgeconv_ws_bytes(N))
    for layers, which in ((1, "mlp_2"), (2, "mlp_3")):
        p2 = (t["mlp_3.conv2.0.weight"].data_ptr(), t["mlp_3.bn2.weight"].data_ptr(), t["mlp_3.bn2.bias"].data_ptr()) if layers == 2 \
            else (None, None, None)
        outs = []
        for flags in (0, 1, 0):
            rng_bits = torch.zeros(256, dtype=torch.int32, device="cuda:0")
            hip.check(lib.sg_edge_range(d_x.data_ptr(), N, rng_bits.data_ptr(), None))
            out = torch.full((N, 64), float("nan"), device="cuda:0")
            hip.check(lib.sg_edgeconv_forward_x(d_x.data_ptr(), d_k.data_ptr(), N, K, layers, t[f"{which}.conv1.0.weight"].data_ptr(),
                                                t[f"{which}.bn1.weight"].data_ptr(), t[f"{which}.bn1.bias"].data_ptr(), *p2, out.data_ptr(),
                                                ws.data_ptr(), ws.numel(), rng_bits.data_ptr(), flags, None))
            outs.append(out.cpu().numpy())
        assert np.isfinite(outs[0]).all(), which
        assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32)), (which, float(np.abs(outs[0] - outs[1]).max()))
        assert np.array_equal(outs[0].view(np.uint32), outs[2].view(np.uint32)), which      # and the same bits run to run


@pytest.mark.gpu
@pytest.mark.parametrize("g1_scale,w2_scale", [(1e3, 1e-3), (1e-3, 1e3), (3e4, 1e-4), (1.0, 1e-6)])
def test_edgeconv_fp16_operand_scaling(env, g1_scale, w2_scale):
    """MLP3's conv2 runs on fp16 pieces; the kernel moves both operands into fp16's exponent range by powers of two derived from
    the weights (kernels_edgeconv.hip, k_bn_fold_moments).  Activations 1000x larger / smaller than usual and conv2 weights far
    from O(0.1) must come out as accurate as the ordinary case (no overflow to inf, no fp16 subnormal loss)."""
    lib, torch, hip = env
    from oracle import cpu_ref as O
    from seggroup_amd import weights
    N, K = 3000, 20
    rng = np.random.default_rng(77)
    x9 = rng.uniform(-1, 1, (N, 9)).astype(np.float32)
    knn = rng.integers(0, N, (N, K)).astype(np.int32)
    W = weights.make_weights(1, 2.0, affine_jitter=0.3)
    W["mlp_3.bn1.weight"] = (W["mlp_3.bn1.weight"] * g1_scale).astype(np.float32)
    W["mlp_3.bn1.bias"] = (W["mlp_3.bn1.bias"] * g1_scale).astype(np.float32)
    W["mlp_3.conv2.0.weight"] = (W["mlp_3.conv2.0.weight"] * w2_scale).astype(np.float32)
    x12 = np.zeros((N, 12), np.float32)
    x12[:, :9] = x9
    d_x, d_k = _up(torch, x12), _up(torch, knn)
    ws = _ws(torch, lib.sg_edgeconv_ws_bytes(N))
    out = torch.zeros(N, 64, device="cuda:0")
    t = {k: _up(torch, W[k]) for k in W}
    hip.check(lib.sg_edgeconv_forward(d_x.data_ptr(), d_k.data_ptr(), N, K, 2, t["mlp_3.conv1.0.weight"].data_ptr(),
                                      t["mlp_3.bn1.weight"].data_ptr(), t["mlp_3.bn1.bias"].data_ptr(), t["mlp_3.conv2.0.weight"].data_ptr(),
                                      t["mlp_3.bn2.weight"].data_ptr(), t["mlp_3.bn2.bias"].data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(), None))
    ref = O.edgeconv_forward(x9, knn.astype(np.int64), W, "mlp_3")
    got = out.cpu().numpy()
    assert np.isfinite(got).all()
    assert np.abs(got - ref).max() < 2e-5 * max(1.0, float(np.abs(ref).max()))
    # ... and with conv1' on fp16 pieces too (the ranged entry: its weights a w T / Sd have to stay inside fp16 for every one of these scales)
    rng_bits = torch.zeros(256, dtype=torch.int32, device="cuda:0")
    hip.check(lib.sg_edge_range(d_x.data_ptr(), N, rng_bits.data_ptr(), None))
    out.zero_()
    hip.check(lib.sg_edgeconv_forward_r(d_x.data_ptr(), d_k.data_ptr(), N, K, 2, t["mlp_3.conv1.0.weight"].data_ptr(),
                                        t["mlp_3.bn1.weight"].data_ptr(), t["mlp_3.bn1.bias"].data_ptr(), t["mlp_3.conv2.0.weight"].data_ptr(),
                                        t["mlp_3.bn2.weight"].data_ptr(), t["mlp_3.bn2.bias"].data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(),
                                        rng_bits.data_ptr(), None))
    got = out.cpu().numpy()
    assert np.isfinite(got).all()
    assert np.abs(got - ref).max() < 2e-5 * max(1.0, float(np.abs(ref).max()))


def test_gcn_forward(env):
    lib, torch, hip = env
    from oracle import cpu_ref as O
    rng = np.random.default_rng(4)
    for D in (192, 256):
        S = 333
        x = rng.normal(size=(S, D)).astype(np.float32)
        pairs = np.unique(np.sort(rng.integers(0, S, (1200, 2)), axis=1), axis=0)
        adj = pairs[pairs[:, 0] != pairs[:, 1]].astype(np.int32)
        E = adj.shape[0]
        Wfc = (rng.uniform(-1, 1, (D, D)) / np.sqrt(D)).astype(np.float32)
        ref = O.gcn_forward(x, adj, Wfc)
        rowptr = np.zeros(S + 1, np.int32)
        for a, b in adj:
            rowptr[a + 1] += 1; rowptr[b + 1] += 1
        np.cumsum(rowptr, out=rowptr)
        fill = rowptr[:-1].copy()
        col = np.zeros(2 * E, np.int32); eid = np.zeros(2 * E, np.int32)
        for e, (a, b) in enumerate(adj):
            col[fill[a]] = b; eid[fill[a]] = e; fill[a] += 1
            col[fill[b]] = a; eid[fill[b]] = e; fill[b] += 1
        out = torch.zeros(S, D, device="cuda:0")
        ws = _ws(torch, lib.sg_gcn_ws_bytes(S, D, E))
        hip.check(lib.sg_gcn_forward(_up(torch, x).data_ptr(), S, D, _up(torch, adj).data_ptr(), E, _up(torch, rowptr).data_ptr(),
                                     _up(torch, col).data_ptr(), _up(torch, eid).data_ptr(), _up(torch, Wfc).data_ptr(),
                                     C.c_float(0.125), out.data_ptr(), ws.data_ptr(), ws.numel(), None))
        assert np.abs(out.cpu().numpy() - ref).max() < 1e-5


def _gcn_graph(S, hubs, seed):
    """Random sparse cluster graph (~3 edges per row) on the first four fifths of the S rows, plus every hub row joined to exactly
    `degree` distinct non-hub rows; the last fifth has no edges but those of the hubs."""
    rng = np.random.default_rng(seed)
    hub_rows = [r for r, _ in hubs]
    other = np.setdiff1d(np.arange(S), hub_rows)
    live = other[other < S - S // 5]
    pairs = [rng.choice(live, (3 * live.size, 2))] if live.size > 1 else []
    for row, deg in hubs:
        pairs.append(np.stack([np.full(deg, row), rng.choice(other, size=deg, replace=False)], 1))
    if not pairs:
        return np.zeros((0, 2), np.int32)
    p = np.unique(np.sort(np.concatenate(pairs), axis=1), axis=0)
    return p[p[:, 0] != p[:, 1]].astype(np.int32)


GCN_EDGE_CASES = [  # (S, D, hub rows (row, degree), seed)
    (600, 192, [(3, 300), (9, 256), (17, 257)], 11),          # unstaged rows (> kDegCap = 256), the staged path at its cap, one past it
    (600, 256, [(5, 300), (8, 256), (13, 257)], 12),
    (17, 192, [], 14),
    (1, 256, [], 15),                                          # S = 1: E = 0
    (40, 192, [], 16),                                         # E forced to 0 below
    (4000, 192, [(1234, 300)], 17),
    (4000, 256, [], 18),
    (333, 64, [(2, 280)], 19),                                 # D outside {192, 256}: the VALU k_gcn_fc
    (333, 100, [(7, 257), (8, 256)], 20),
    (129, 100, [], 21),
]


@pytest.mark.parametrize("S,D,hubs,seed", GCN_EDGE_CASES, ids=[f"S{c[0]}-D{c[1]}-hub{max([h[1] for h in c[2]], default=0)}-{c[3]}" for c in GCN_EDGE_CASES])
def test_gcn_forward_edge_cases(env, S, D, hubs, seed):
    """sg_gcn_forward against the float64 oracle where test_gcn_forward does not go: rows of more than kDegCap = 256 edges (the
    aggregate's unstaged path), exactly 256 and 257, rows without edges, E = 0, S = 1 / 17 / 4,000 and D outside {192, 256}."""
    lib, torch, hip = env
    from oracle import cpu_ref as O
    rng = np.random.default_rng(seed)
    adj = _gcn_graph(S, hubs, seed) if seed != 16 else np.zeros((0, 2), np.int32)
    E = adj.shape[0]
    deg = np.bincount(adj.reshape(-1), minlength=S)
    for row, d in hubs:
        assert deg[row] == d, (row, deg[row], d)
    if S >= 5:
        assert (deg == 0).any()                                   # rows without edges take part
    x = rng.normal(size=(S, D)).astype(np.float32)
    Wfc = (rng.uniform(-1, 1, (D, D)) / np.sqrt(D)).astype(np.float32)
    ref = O.gcn_forward(x, adj, Wfc, alpha=0.125)
    rowptr = np.zeros(S + 1, np.int32)
    np.add.at(rowptr, adj[:, 0] + 1, 1)
    np.add.at(rowptr, adj[:, 1] + 1, 1)
    np.cumsum(rowptr, out=rowptr)
    fill = rowptr[:-1].copy()
    col = np.zeros(max(2 * E, 1), np.int32)
    eid = np.zeros(max(2 * E, 1), np.int32)
    for e, (a, b) in enumerate(adj):
        col[fill[a]] = b; eid[fill[a]] = e; fill[a] += 1
        col[fill[b]] = a; eid[fill[b]] = e; fill[b] += 1
    out = torch.full((S, D), float("nan"), device="cuda:0")
    ws = _ws(torch, lib.sg_gcn_ws_bytes(S, D, E))
    adj_d = _up(torch, adj if E else np.zeros((1, 2), np.int32))
    hip.check(lib.sg_gcn_forward(_up(torch, x).data_ptr(), S, D, adj_d.data_ptr(), E, _up(torch, rowptr).data_ptr(),
                                 _up(torch, col).data_ptr(), _up(torch, eid).data_ptr(), _up(torch, Wfc).data_ptr(),
                                 C.c_float(0.125), out.data_ptr(), ws.data_ptr(), ws.numel(), None))
    got = out.cpu().numpy()
    assert np.isfinite(got).all()
    err = np.abs(got - ref).max()
    assert err < 1e-5, f"max |HIP - oracle| = {err:.3g}"


def test_export_and_evaluate(env, golden_index):
    lib, torch, hip = env
    from oracle import cpu_ref as O
    sc = make_fixture_scene(golden_index, "tiny_dup_4k")          # V != N, non-identity unmap
    rng = np.random.default_rng(8)
    S, V, N = sc.num_segments, sc.unmap.shape[0], sc.num_points
    tables = rng.integers(-1, 50, (14, S)).astype(np.int32)
    out = torch.zeros(14, V, dtype=torch.int32, device="cuda:0")
    hip.check(lib.sg_export_labels(_up(torch, sc.unmap.astype(np.int32)).data_ptr(), V, _up(torch, sc.seg).data_ptr(), N,
                                   _up(torch, tables).data_ptr(), 14, S, out.data_ptr(), None))
    assert np.array_equal(out.cpu().numpy(), tables[:, sc.seg[sc.unmap]])
    # evaluate: predictions with unlabeled (-1) vertices and an instance whose first vertex has sem == -1
    sem_pred = rng.integers(-1, 41, V).astype(np.int32)
    sem_pred[sem_pred == 0] = -1
    ins_pred = rng.integers(-1, 6, V).astype(np.int32)
    ins_pred[ins_pred == 0] = -1
    first5 = np.nonzero((ins_pred == 5) & (sc.gt[:, 0] != 0))[0][0]
    sem_pred[first5] = -1                                         # slot -2 wraps to class 38 (model.py:636-639)
    ref = O.evaluate(sc.gt, sem_pred, ins_pred)
    iou_s, iou_i, acc = np.zeros(80, np.float32), np.zeros(80, np.float32), np.zeros(4, np.float32)
    ws = _ws(torch, lib.sg_eval_ws_bytes(8))
    hip.check(lib.sg_evaluate(_up(torch, sc.gt.astype(np.int32)).data_ptr(), _up(torch, sem_pred).data_ptr(),
                              _up(torch, ins_pred).data_ptr(), V, 8, iou_s.ctypes.data, iou_i.ctypes.data, acc.ctypes.data,
                              ws.data_ptr(), ws.numel(), None))
    assert np.array_equal(iou_s.reshape(1, 2, 40), ref[0])
    assert np.array_equal(iou_i.reshape(1, 2, 40), ref[1])
    assert np.allclose(acc, ref[2], rtol=0, atol=1e-7, equal_nan=True)


def test_pruned_knn_equals_bruteforce_and_oracle(env, golden_index):
    """sg_cluster_knn_pruned (segment-box pruning) must give the same table as the brute-force kernel,
    bit for bit, and both must equal the oracle (same defined tie rule) -- including duplicated points."""
    lib, torch, hip = env
    from oracle import cpu_ref as O
    for name, target in (("tiny_dup_4k", 4), ("small_20k", 12), ("small_20k", 3)):
        sc = make_fixture_scene(golden_index, name)
        part, L = _semantic_inputs(sc, target)
        members, off = _layer_arrays(L)
        N, S = sc.num_points, sc.num_segments
        # ordered segment list of every cluster, recovered from the member arrays
        order, dst, cso = [], [], [0]
        for c, m in enumerate(L.members):
            segs = sc.seg[m]
            starts = np.concatenate([[0], np.nonzero(np.diff(segs))[0] + 1])
            order += segs[starts].tolist()
            dst += (off[c] + starts).tolist()
            cso.append(len(order))
        assert sorted(order) == list(range(S))
        segorder = np.argsort(sc.seg, kind="stable").astype(np.int32)
        seg_off = np.concatenate([[0], np.cumsum(np.bincount(sc.seg, minlength=S))]).astype(np.int32)
        tc, lo, hi, cto = _tiles(off)
        d = {k: _up(torch, np.asarray(v, np.int32)) for k, v in dict(members=members, off=off, tc=tc, lo=lo, hi=hi, cto=cto, order=order,
                                                                      dst=dst, cso=cso, segpts=segorder, segoff=seg_off).items()}
        d_data = _up(torch, sc.data)
        x9m = torch.zeros(N, 12, device="cuda:0"); xyzw = torch.zeros(N, 4, device="cuda:0")
        ws = _ws(torch, lib.sg_center_ws_bytes(len(tc), L.count))
        hip.check(lib.sg_center_clusters(d_data.data_ptr(), N, d["members"].data_ptr(), d["off"].data_ptr(), L.count, d["tc"].data_ptr(),
                                         d["lo"].data_ptr(), d["hi"].data_ptr(), len(tc), d["cto"].data_ptr(), x9m.data_ptr(),
                                         xyzw.data_ptr(), ws.data_ptr(), ws.numel(), None))
        box = torch.zeros(S, 8, device="cuda:0")
        hip.check(lib.sg_segment_boxes(d_data.data_ptr(), d["segpts"].data_ptr(), d["segoff"].data_ptr(), S, box.data_ptr(), None))
        b = box.cpu().numpy()
        for s_ in (0, S // 2, S - 1):
            pts = sc.data[sc.seg == s_, :3]
            assert np.array_equal(b[s_, :3], pts.min(0)) and np.array_equal(b[s_, 3:6], pts.max(0))
        pos_of_point = np.empty(N, np.int64); pos_of_point[members] = np.arange(N)
        k_brute = torch.zeros(N, 20, dtype=torch.int32, device="cuda:0")
        k_prune = torch.full((N, 20), -7, dtype=torch.int32, device="cuda:0")
        hip.check(lib.sg_cluster_knn(xyzw.data_ptr(), N, d["off"].data_ptr(), d["tc"].data_ptr(), d["lo"].data_ptr(), d["hi"].data_ptr(),
                                     len(tc), 20, int(pos_of_point[0]), k_brute.data_ptr(), None))
        slot_of_pos = np.repeat(np.arange(S), np.diff(np.concatenate([dst, [N]])) if False else
                                np.diff(np.concatenate([np.asarray(dst), [N]]))).astype(np.int32)
        d_slot = _up(torch, slot_of_pos)
        tc4, lo4, hi4, _ = _tiles(off, 64)
        d4 = [_up(torch, x) for x in (tc4, lo4, hi4)]
        hip.check(lib.sg_cluster_knn_pruned(xyzw.data_ptr(), N, d["off"].data_ptr(), d4[0].data_ptr(), d4[1].data_ptr(),
                                            d4[2].data_ptr(), len(tc4), d["cso"].data_ptr(), d["order"].data_ptr(), d["dst"].data_ptr(),
                                            d["segoff"].data_ptr(), box.data_ptr(), d_slot.data_ptr(), 20, int(pos_of_point[0]),
                                            k_prune.data_ptr(), None))
        a, b_ = k_brute.cpu().numpy(), k_prune.cpu().numpy()
        assert np.array_equal(a, b_), f"{name}/{target}: {int(np.any(a != b_, axis=1).sum())} rows differ between brute force and pruned"
        # spatially sorted variant: Morton order inside every segment + 32-point chunk boxes
        chunk_off = np.concatenate([[0], np.cumsum((np.diff(seg_off) + 31) // 32)]).astype(np.int32)
        d_co = _up(torch, chunk_off)
        sperm = torch.zeros(N, dtype=torch.int32, device="cuda:0")
        cbox = torch.zeros(int(chunk_off[-1]) + 1, 8, device="cuda:0")
        wss = _ws(torch, lib.sg_segment_sort_ws_bytes(N))
        d_sop = _up(torch, sc.seg)
        obox, osperm, ocbox = _morton_sort_oracle(sc.data, segorder, seg_off)
        assert np.array_equal(obox, box.cpu().numpy())                 # sg_segment_boxes: the same boxes
        sperm.copy_(torch.from_numpy(osperm)); cbox[:len(ocbox)].copy_(torch.from_numpy(ocbox))
        # the single-launch kernel (segment box + Morton sort in LDS + chunk boxes) against the NumPy statement, bit for bit
        box2 = torch.full((S, 8), 7.0, device="cuda:0"); sperm2 = torch.full((N,), -1, dtype=torch.int32, device="cuda:0")
        cbox2 = torch.zeros_like(cbox)
        for max_seg in (int(np.diff(seg_off).max()), 1 << 20):      # fits a block / also launches the big-segment kernel (nothing for it to do)
            box2.fill_(7.0); sperm2.fill_(-1); cbox2.zero_()
            sums = torch.zeros(S, 3, dtype=torch.float64, device="cuda:0")
            hip.check(lib.sg_segment_sort_boxes(d_data.data_ptr(), N, d["segpts"].data_ptr(), d["segoff"].data_ptr(), d_sop.data_ptr(), S,
                                                d_co.data_ptr(), max_seg, box2.data_ptr(), sperm2.data_ptr(), cbox2.data_ptr(), sums.data_ptr(),
                                                wss.data_ptr(), wss.numel(), None))
            assert torch.equal(box2, box) and torch.equal(sperm2, sperm) and torch.equal(cbox2, cbox), max_seg
            want_sums = np.stack([np.bincount(sc.seg, weights=sc.data[:, k_].astype(np.float64), minlength=S) for k_ in range(3)], 1)
            assert np.allclose(sums.cpu().numpy(), want_sums, rtol=1e-13, atol=1e-9)
        sp = sperm.cpu().numpy()
        for s_ in (0, S - 1):      # a permutation of the segment's CSR range
            assert sorted(sp[seg_off[s_]:seg_off[s_ + 1]].tolist()) == list(range(seg_off[s_], seg_off[s_ + 1]))
        sxyzw = torch.zeros(N, 4, device="cuda:0")
        smpos = torch.zeros(N, dtype=torch.int32, device="cuda:0")
        hip.check(lib.sg_knn_operands(d_data.data_ptr(), d["segpts"].data_ptr(), d["segoff"].data_ptr(), sperm.data_ptr(), S,
                                      d["order"].data_ptr(), d["dst"].data_ptr(), sxyzw.data_ptr(), smpos.data_ptr(), None))
        assert sorted(smpos.cpu().numpy().tolist()) == list(range(N))
        # sg_layer_layout = gather_members + center_clusters + knn_operands in one launch: the same arrays, bit for bit,
        # with the cluster centroids formed on the host from the per-segment coordinate sums
        hs = sums.cpu().numpy()
        cl_of_slot = np.repeat(np.arange(L.count), np.diff(cso)).astype(np.int32)
        mean = np.zeros((L.count, 3), np.float32)
        for c_ in range(L.count):
            mean[c_] = (hs[np.asarray(order)[cso[c_]:cso[c_ + 1]]].sum(0) / float(off[c_ + 1] - off[c_])).astype(np.float32)
        lay = dict(members=torch.full((N,), -1, dtype=torch.int32, device="cuda:0"), pop=torch.full((N,), -1, dtype=torch.int32, device="cuda:0"),
                   cop=torch.full((N,), -1, dtype=torch.int32, device="cuda:0"), sop=torch.full((N,), -1, dtype=torch.int32, device="cuda:0"),
                   x9m=torch.full((N, 12), 7.0, device="cuda:0"), sx=torch.zeros(N, 4, device="cuda:0"),
                   sm=torch.full((N,), -1, dtype=torch.int32, device="cuda:0"), rec=torch.zeros(N, 4, device="cuda:0"))
        d_cls, d_mean = _up(torch, cl_of_slot), _up(torch, mean)
        hip.check(lib.sg_layer_layout(d_data.data_ptr(), N, d["segpts"].data_ptr(), d["segoff"].data_ptr(), sperm.data_ptr(), S,
                                      d["order"].data_ptr(), d["dst"].data_ptr(), d_cls.data_ptr(), d_mean.data_ptr(), lay["members"].data_ptr(),
                                      lay["pop"].data_ptr(), lay["cop"].data_ptr(), lay["sop"].data_ptr(), lay["x9m"].data_ptr(),
                                      lay["sx"].data_ptr(), lay["sm"].data_ptr(), lay["rec"].data_ptr(), None, None, None))
        assert np.array_equal(lay["members"].cpu().numpy(), members) and np.array_equal(lay["pop"].cpu().numpy(), pos_of_point)
        rec = lay["rec"].cpu().numpy()                          # by point id: xyz + the bits of the point's member position
        assert np.array_equal(rec[:, :3], d_data.cpu().numpy()[:, :3]) and np.array_equal(rec[:, 3].copy().view(np.int32), pos_of_point.astype(np.int32))
        # with seed ids: id of a point = its place in the Morton-sorted CSR of the over-segmentation (the same in every layer);
        # the records are indexed by it
        sid = torch.full((N,), -1, dtype=torch.int32, device="cuda:0")
        rec2 = torch.zeros(N, 4, device="cuda:0")
        rng_bits = torch.zeros(256, dtype=torch.int32, device="cuda:0")
        hip.check(lib.sg_layer_layout(d_data.data_ptr(), N, d["segpts"].data_ptr(), d["segoff"].data_ptr(), sperm.data_ptr(), S,
                                      d["order"].data_ptr(), d["dst"].data_ptr(), d_cls.data_ptr(), d_mean.data_ptr(), lay["members"].data_ptr(),
                                      lay["pop"].data_ptr(), lay["cop"].data_ptr(), lay["sop"].data_ptr(), lay["x9m"].data_ptr(),
                                      lay["sx"].data_ptr(), lay["sm"].data_ptr(), rec2.data_ptr(), sid.data_ptr(), rng_bits.data_ptr(), None))
        # ... and the layer's range word: bits of the largest |centred xyz| / |feature|
        xc = lay["x9m"].cpu().numpy()
        want_range = np.float32(max(np.abs(xc[:, 6:9]).max(), np.abs(xc[:, 3:6]).max()))
        assert rng_bits.cpu().numpy().view(np.float32).max() == want_range
        sid_np, rec2_np = sid.cpu().numpy(), rec2.cpu().numpy()
        sorted_pts = segorder[sperm.cpu().numpy()]                # seed id -> point id
        assert sorted(sid_np.tolist()) == list(range(N)) and np.array_equal(sorted_pts[sid_np], members)
        assert np.array_equal(rec2_np[:, :3], sc.data[sorted_pts, :3]) and np.array_equal(rec2_np[:, 3].copy().view(np.int32), pos_of_point[sorted_pts].astype(np.int32))
        assert np.array_equal(lay["cop"].cpu().numpy(), np.repeat(np.arange(L.count), np.diff(off)))
        assert np.array_equal(lay["sop"].cpu().numpy(), slot_of_pos)
        assert torch.equal(lay["x9m"], x9m) and torch.equal(lay["sx"], sxyzw) and torch.equal(lay["sm"], smpos)
        for variant in (1, 2, 4, 0):        # one-pass with 1 / 2 / 4 waves per tile | 0: chosen by tile count
            k_sorted = torch.full((N, 20), -7, dtype=torch.int32, device="cuda:0")
            hip.check(lib.sg_cluster_knn_sorted_w(sxyzw.data_ptr(), smpos.data_ptr(), N, d["off"].data_ptr(), d4[0].data_ptr(), d4[1].data_ptr(),
                                                  d4[2].data_ptr(), len(tc4), d["cso"].data_ptr(), d["order"].data_ptr(), d["dst"].data_ptr(),
                                                  d["segoff"].data_ptr(), d_co.data_ptr(), box.data_ptr(), cbox.data_ptr(), d_slot.data_ptr(), 20,
                                                  int(pos_of_point[0]), variant, k_sorted.data_ptr(), None))
            c_ = k_sorted.cpu().numpy()
            assert np.array_equal(a, c_), f"{name}/{target}/variant {variant}: {int(np.any(a != c_, axis=1).sum())} rows differ between brute force and sorted"
        # two-pass kernel over the cluster-ordered chunk table (host side of the table as in pipeline.cpp)
        nch_slot = (np.diff(seg_off)[np.asarray(order)] + 31) // 32
        slot_chunk0 = np.concatenate([[0], np.cumsum(nch_slot)]).astype(np.int32)
        cl_chunk_off = slot_chunk0[np.asarray(cso)].astype(np.int32)
        dst_a = np.asarray(dst)
        tile_chunk0 = np.zeros(len(tc4), np.int32)
        for t_, (c__, lo_) in enumerate(zip(tc4, lo4)):
            slot = cso[c__] + int(np.searchsorted(dst_a[cso[c__]:cso[c__ + 1]], lo_, side="right")) - 1
            tile_chunk0[t_] = slot_chunk0[slot] + (lo_ - dst_a[slot]) // 32 - cl_chunk_off[c__]
        d_sc0, d_cco, d_tc0 = _up(torch, slot_chunk0), _up(torch, cl_chunk_off), _up(torch, tile_chunk0)
        cc = torch.zeros(int(slot_chunk0[-1]) + 1, 8, device="cuda:0")
        hip.check(lib.sg_knn_chunk_table(d["order"].data_ptr(), d["dst"].data_ptr(), d["segoff"].data_ptr(), d_co.data_ptr(), cbox.data_ptr(),
                                         S, d_sc0.data_ptr(), cc.data_ptr(), None))
        cch = cc.cpu().numpy()[:-1]
        packed = cch[:, 7].copy().view(np.int32)
        assert np.array_equal(np.sort(packed >> 6), np.sort(np.concatenate([dst_a[i] + 32 * np.arange(nch_slot[i]) for i in range(S)])))
        assert int(((packed & 63) + 1).sum()) == N
        k_two = torch.full((N, 20), -7, dtype=torch.int32, device="cuda:0")
        hip.check(lib.sg_cluster_knn_2pass(sxyzw.data_ptr(), smpos.data_ptr(), N, d["off"].data_ptr(), d4[0].data_ptr(), d4[1].data_ptr(),
                                           d4[2].data_ptr(), d_tc0.data_ptr(), len(tc4), d_cco.data_ptr(), cc.data_ptr(), 20,
                                           int(pos_of_point[0]), k_two.data_ptr(), None))
        e_ = k_two.cpu().numpy()
        assert np.array_equal(a, e_), f"{name}/{target}: {int(np.any(a != e_, axis=1).sum())} rows differ between brute force and two-pass"
        ref = O.cluster_knn(sc.data[:, :3], L, 20)[members]
        assert np.array_equal(members[a], ref)


def _knn_layer_setup(lib, torch, hip, sc, L):
    """Device arrays of one layer for the sorted kNN kernels + the brute-force table (member-position entries)."""
    members, off = _layer_arrays(L)
    N, S = sc.num_points, sc.num_segments
    order, dst, cso = [], [], [0]
    for c, m in enumerate(L.members):
        segs = sc.seg[m]
        starts = np.concatenate([[0], np.nonzero(np.diff(segs))[0] + 1])
        order += segs[starts].tolist()
        dst += (off[c] + starts).tolist()
        cso.append(len(order))
    segorder = np.argsort(sc.seg, kind="stable").astype(np.int32)
    seg_off = np.concatenate([[0], np.cumsum(np.bincount(sc.seg, minlength=S))]).astype(np.int32)
    tc, lo, hi, cto = _tiles(off)
    tc4, lo4, hi4, _ = _tiles(off, 64)
    pos_of_point = np.empty(N, np.int32); pos_of_point[members] = np.arange(N, dtype=np.int32)
    slot_of_pos = np.repeat(np.arange(S), np.diff(np.concatenate([np.asarray(dst), [N]]))).astype(np.int32)
    chunk_off = np.concatenate([[0], np.cumsum((np.diff(seg_off) + 31) // 32)]).astype(np.int32)
    d = {k: _up(torch, np.asarray(v, np.int32)) for k, v in dict(members=members, off=off, tc=tc, lo=lo, hi=hi, cto=cto, order=order, dst=dst,
                                                                  cso=cso, segpts=segorder, segoff=seg_off, tc4=tc4, lo4=lo4, hi4=hi4,
                                                                  pos_of_point=pos_of_point, slot=slot_of_pos, co=chunk_off, sop=sc.seg).items()}
    d["data"] = _up(torch, sc.data)
    x9m = torch.zeros(N, 12, device="cuda:0"); xyzw = torch.zeros(N, 4, device="cuda:0")
    ws = _ws(torch, lib.sg_center_ws_bytes(len(tc), L.count))
    hip.check(lib.sg_center_clusters(d["data"].data_ptr(), N, d["members"].data_ptr(), d["off"].data_ptr(), L.count, d["tc"].data_ptr(),
                                     d["lo"].data_ptr(), d["hi"].data_ptr(), len(tc), d["cto"].data_ptr(), x9m.data_ptr(), xyzw.data_ptr(),
                                     ws.data_ptr(), ws.numel(), None))
    brute = torch.zeros(N, 20, dtype=torch.int32, device="cuda:0")
    hip.check(lib.sg_cluster_knn(xyzw.data_ptr(), N, d["off"].data_ptr(), d["tc"].data_ptr(), d["lo"].data_ptr(), d["hi"].data_ptr(), len(tc), 20,
                                 int(pos_of_point[0]), brute.data_ptr(), None))
    box = torch.zeros(S, 8, device="cuda:0")
    hip.check(lib.sg_segment_boxes(d["data"].data_ptr(), d["segpts"].data_ptr(), d["segoff"].data_ptr(), S, box.data_ptr(), None))
    sperm = torch.zeros(N, dtype=torch.int32, device="cuda:0")
    cbox = torch.zeros(int(chunk_off[-1]) + 1, 8, device="cuda:0")
    wss = _ws(torch, lib.sg_segment_sort_ws_bytes(N))
    box_s = torch.zeros_like(box)
    hip.check(lib.sg_segment_sort_boxes(d["data"].data_ptr(), N, d["segpts"].data_ptr(), d["segoff"].data_ptr(), d["sop"].data_ptr(), S,
                                        d["co"].data_ptr(), int(np.diff(seg_off).max()), box_s.data_ptr(), sperm.data_ptr(), cbox.data_ptr(), None,
                                        wss.data_ptr(), wss.numel(), None))
    assert torch.equal(box_s, box)
    sxyzw = torch.zeros(N, 4, device="cuda:0"); smpos = torch.zeros(N, dtype=torch.int32, device="cuda:0")
    hip.check(lib.sg_knn_operands(d["data"].data_ptr(), d["segpts"].data_ptr(), d["segoff"].data_ptr(), sperm.data_ptr(), S, d["order"].data_ptr(),
                                  d["dst"].data_ptr(), sxyzw.data_ptr(), smpos.data_ptr(), None))
    d.update(box=box, cbox=cbox, sxyzw=sxyzw, smpos=smpos, brute=brute, pos0=int(pos_of_point[0]), nt4=len(tc4), members_np=members, off_np=off)
    return d


@pytest.mark.parametrize("name,fine,coarse", [("small_20k", 40, 6), ("tiny_dup_4k", 12, 3), ("small_20k", 150, 40)])
def test_seeded_knn_equals_bruteforce(env, golden_index, name, fine, coarse):
    """sg_knn_seed_points + sg_cluster_knn_seeded: the coarse layer's clusters are unions of the fine layer's (more unions
    on the SAME partition), every query starts from its fine-layer list and skips its former cluster's chunks; the table
    must equal the coarse layer's brute-force table, duplicates and former clusters of <= 20 points included."""
    lib, torch, hip = env
    sc = make_fixture_scene(golden_index, name)
    part, Lf = _semantic_inputs(sc, fine)
    f = _knn_layer_setup(lib, torch, hip, sc, Lf)
    N, S = sc.num_points, sc.num_segments
    seed = torch.full((N, 20), -1, dtype=torch.int32, device="cuda:0")
    hip.check(lib.sg_knn_seed_points(f["brute"].data_ptr(), f["members"].data_ptr(), N, 20, seed.data_ptr(), None))
    sd = seed.cpu().numpy()
    fb = f["brute"].cpu().numpy()
    assert np.array_equal(sd[f["members_np"]], f["members_np"][fb])           # rows and entries are point ids now
    # the fine layer's cluster of every segment, -1 where it has no kNN list
    fine_sizes = np.diff(f["off_np"])
    cl_of_seg = np.empty(S, np.int64)
    for c, m in enumerate(Lf.members):
        cl_of_seg[np.unique(sc.seg[m])] = c
    seg_prevcl = np.where(fine_sizes[cl_of_seg] > 20, cl_of_seg, -1).astype(np.int32)
    assert (seg_prevcl >= 0).any()
    # coarser layer: keep merging the same partition
    import oracle.cpu_ref as O
    rng = np.random.default_rng(10)
    while len(part.roots()) > coarse:
        r = part.roots()
        a, b = rng.choice(len(r), 2, replace=False)
        part.ins[r[a]] = -1
        part.union(r[a], r[b])
    Lc = O.Layer(part)
    c = _knn_layer_setup(lib, torch, hip, sc, Lc)
    d_prev = _up(torch, seg_prevcl)
    # sg_layer_layout's per-point records of THIS layer: xyz + the bits of the member position
    rec_np = np.zeros((N, 4), np.float32)
    rec_np[:, :3] = c["data"].cpu().numpy()[:, :3]
    rec_np[:, 3] = c["pos_of_point"].cpu().numpy().astype(np.int32).view(np.float32)
    rec = _up(torch, rec_np)
    out = torch.full((N, 20), -7, dtype=torch.int32, device="cuda:0")
    hip.check(lib.sg_cluster_knn_seeded(c["sxyzw"].data_ptr(), c["smpos"].data_ptr(), N, c["off"].data_ptr(), c["tc4"].data_ptr(),
                                        c["lo4"].data_ptr(), c["hi4"].data_ptr(), c["nt4"], c["cso"].data_ptr(), c["order"].data_ptr(),
                                        c["dst"].data_ptr(), c["segoff"].data_ptr(), c["co"].data_ptr(), c["box"].data_ptr(), c["cbox"].data_ptr(),
                                        c["slot"].data_ptr(), seed.data_ptr(), d_prev.data_ptr(), c["members"].data_ptr(),
                                        rec.data_ptr(), 20, c["pos0"], out.data_ptr(), None))
    a_, b_ = c["brute"].cpu().numpy(), out.cpu().numpy()
    assert np.array_equal(a_, b_), f"{int(np.any(a_ != b_, axis=1).sum())} rows differ between brute force and seeded"


@pytest.mark.parametrize("n,s,seed,target,kw", [(3000, 30, 40000, 30, {}), (3000, 30, 40007, 9, {}), (2400, 400, 91, 60, dict(min_seg=1)),
                                                (2400, 400, 91, 25, dict(min_seg=1)), (2400, 200, 92, 40, dict(min_seg=1, dup_frac=0.2)),
                                                (2000, 250, 94, 80, dict(min_seg=1)), (2000, 250, 94, 120, dict(min_seg=1)), (1500, 60, 93, 60, dict(min_seg=2))],
                         ids=["3000pts-30clusters", "3000pts-9clusters", "6pt-segments-40pt-clusters", "6pt-segments-96pt-clusters", "12pt-segments-dups",
                              "8pt-segments-25pt-clusters", "8pt-segments-17pt-clusters", "25pt-clusters"])
def test_multi_wave_knn_with_slices_short_of_candidates(env, n, s, seed, target, kw):
    """Gate for kNN changes.  With two or four waves per tile the cluster's chunks are dealt round-robin to the
    waves and every wave publishes bounds from its OWN list; in small clusters a wave's slice holds fewer than 20 (or fewer than 20 / waves)
    real candidates, its list ends in padding entries (key 0: score -inf) and the bound it publishes is the padding's.  Round 5's list-form
    thresholds decoded such a bound to a NaN -- only scenes of ~3,000 points take these kernels inside the engine, and no operator test fed
    them small clusters.  Every variant, clusters of 21 .. ~300 points (and <= 20: the padded rows), against the brute-force kernel; the
    brute-force table against the oracle."""
    lib, torch, hip = env
    from oracle import cpu_ref as O
    from seggroup_amd import synthetic
    sc = synthetic.make_scene(n, s, seed, **kw)
    part, L = _semantic_inputs(sc, target)
    sizes = np.array([len(m) for m in L.members])
    assert ((sizes > 20) & (sizes < 80)).any() or n == 3000, sizes          # clusters whose slices run short
    d = _knn_layer_setup(lib, torch, hip, sc, L)
    N = sc.num_points
    a = d["brute"].cpu().numpy()
    ref = O.cluster_knn(sc.data[:, :3], L, 20)[d["members_np"]]
    assert np.array_equal(d["members_np"][a], ref)
    for variant in (4, 2, 1, 0):
        out = torch.full((N, 20), -7, dtype=torch.int32, device="cuda:0")
        hip.check(lib.sg_cluster_knn_sorted_w(d["sxyzw"].data_ptr(), d["smpos"].data_ptr(), N, d["off"].data_ptr(), d["tc4"].data_ptr(), d["lo4"].data_ptr(),
                                              d["hi4"].data_ptr(), d["nt4"], d["cso"].data_ptr(), d["order"].data_ptr(), d["dst"].data_ptr(),
                                              d["segoff"].data_ptr(), d["co"].data_ptr(), d["box"].data_ptr(), d["cbox"].data_ptr(), d["slot"].data_ptr(), 20,
                                              d["pos0"], variant, out.data_ptr(), None))
        b = out.cpu().numpy()
        assert b.min() >= 0 and b.max() < N, f"variant {variant}: entries outside the scene ({b.min()} .. {b.max()}): a padding entry reached the table"
        assert np.array_equal(a, b), f"variant {variant}: {int(np.any(a != b, axis=1).sum())} rows differ between brute force and sorted"


@pytest.mark.parametrize("cfg", [(30000, 6, 140, dict(min_seg=4)), (60000, 600, 70000, dict(seg_profile="scannet")),
                                 (60000, 600, 70001, dict(seg_profile="scannet")), (20000, 3, 142, dict(min_seg=4, dup_frac=0.3))],
                         ids=["5k-point-segments", "scannet-subsampled", "scannet-tiled", "7k-segments-30pct-duplicates"])
def test_segments_beyond_the_lds_sort_cap(env, cfg):
    """Over-segments of more than 2,048 points (floors and walls of a real scan: 10k-30k points) are Morton-sorted by
    k_bigseg_sort_boxes (cells of the top 12 Morton bits, every run of cells sorted in LDS): segment boxes, sorted order, chunk
    boxes and coordinate sums must equal the NumPy statement of the order (`_morton_sort_oracle`) bit for bit."""
    lib, torch, hip = env
    from seggroup_amd import synthetic
    n, s, seed, kw = cfg
    sc = synthetic.make_scene(n, s, seed, **kw)
    N, S = sc.num_points, sc.num_segments
    counts = np.bincount(sc.seg, minlength=S)
    assert counts.max() > 2048
    order = np.argsort(sc.seg, kind="stable").astype(np.int32)
    seg_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    chunk_off = np.concatenate([[0], np.cumsum((counts + 31) // 32)]).astype(np.int32)
    d_data, d_pts, d_off, d_sop, d_co = (_up(torch, x) for x in (sc.data, order, seg_off, sc.seg, chunk_off))
    nchunk = int(chunk_off[-1])
    # the order the header defines, evaluated in NumPy: boxes, (segment, morton30, CSR index) order, chunk boxes
    obox, osperm, ocbox = _morton_sort_oracle(sc.data, order, seg_off)
    box, sperm = _up(torch, obox), _up(torch, osperm)
    cbox = torch.zeros(nchunk + 1, 8, device="cuda:0"); cbox[:nchunk].copy_(torch.from_numpy(ocbox))
    # the pipeline's path
    box2 = torch.full((S, 8), 7.0, device="cuda:0"); sperm2 = torch.full((N,), -1, dtype=torch.int32, device="cuda:0")
    cbox2 = torch.zeros_like(cbox); sums = torch.zeros(S, 3, dtype=torch.float64, device="cuda:0")
    ws2 = _ws(torch, lib.sg_segment_sort_ws_bytes(N))
    for rep in range(2):                                        # twice: the scratch keeps stale keys from the first run
        hip.check(lib.sg_segment_sort_boxes(d_data.data_ptr(), N, d_pts.data_ptr(), d_off.data_ptr(), d_sop.data_ptr(), S, d_co.data_ptr(),
                                            int(counts.max()), box2.data_ptr(), sperm2.data_ptr(), cbox2.data_ptr(), sums.data_ptr(),
                                            ws2.data_ptr(), ws2.numel(), None))
        torch.cuda.synchronize()
        assert torch.equal(box2, box)
        bad = torch.nonzero(sperm2 != sperm).flatten()
        assert bad.numel() == 0, f"{bad.numel()} sorted positions differ, first at {int(bad[0])} (segment {int(sc.seg[order[int(bad[0])]])})"
        assert torch.equal(cbox2[:nchunk], cbox[:nchunk])
    want = np.stack([np.bincount(sc.seg, weights=sc.data[:, k_].astype(np.float64), minlength=S) for k_ in range(3)], 1)
    assert np.allclose(sums.cpu().numpy(), want, rtol=1e-13, atol=1e-9)
    with pytest.raises(hip.SgError):                            # the scratch is checked, not trusted
        hip.check(lib.sg_segment_sort_boxes(d_data.data_ptr(), N, d_pts.data_ptr(), d_off.data_ptr(), d_sop.data_ptr(), S, d_co.data_ptr(),
                                            int(counts.max()), box2.data_ptr(), sperm2.data_ptr(), cbox2.data_ptr(), sums.data_ptr(),
                                            ws2.data_ptr(), 1024, None))


def test_dpp_wave_reductions_selftest(env):
    """csrc/wave_ops.h: sums (float, double), max / min, integer max, argmax with the lowest-index tie rule and the readlane
    broadcasts equal the ds_bpermute butterflies on 512 waves x 64 rounds of pseudo-random values (ties included)."""
    lib, torch, hip = env
    bad = C.c_int(-1)
    hip.check(lib.sg_selftest_wave_ops(C.byref(bad), None))
    assert bad.value == 0


def test_list_form_insertion_selftest(env):
    """csrc/knn_device.h: the top-20 list as doubles of one exponent (two v_min_f64 / v_max_f64 per slot) holds the same keys in the same
    order as the 64-bit integer list it replaced -- 32k lanes x 300 keys with exact score ties, signed zeros, tiny positive scores, the
    empty key, indices up to 2^20 - 1."""
    lib, torch, hip = env
    bad = C.c_int(-1)
    hip.check(lib.sg_selftest_list_insert(C.byref(bad), None))
    assert bad.value == 0


def test_knn_refuses_scenes_beyond_the_list_index_bits(env):
    """The list keys carry 20 index bits: a table for more than 2^20 points must be refused loudly, not computed wrongly."""
    lib, torch, hip = env
    z = torch.zeros(64, dtype=torch.int32, device="cuda:0")
    f = torch.zeros(64, 4, device="cuda:0")
    with pytest.raises(hip.SgError):
        hip.check(lib.sg_cluster_knn_sorted(f.data_ptr(), z.data_ptr(), (1 << 20) + 1, z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), 1, z.data_ptr(),
                                            z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), f.data_ptr(), f.data_ptr(), z.data_ptr(), 20, 0, z.data_ptr(), None))
