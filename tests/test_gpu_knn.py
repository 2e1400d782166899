"""k nearest neighbours on the GPU (include/rrl.h rrl_knn; rrl_hip/neighbors.py knn, knn_group, estimate_normals_knn;
rrl_hip/callsites.py dcp_knn, dcp_graph_feature) against the numpy twin of tests/knn_refs.py.

Everything is bit for bit unless said otherwise: idx and found equal the twin's, dist2 is float32(the twin's float64 d), the
features are float32 gathers and float32 subtractions, and the tree equals brute force.  The two bounds that are not equality:
- the DCP call sites against the recorded reference and against its float32 matmul formulation on the same GPU: exact on the
  rows the twin does not mark borderline (two consecutive keys within 2^-20 (|x_i|^2 + |x_j|^2)), at most 2 % of rows per case;
- estimate_normals_knn against the float64 normals twin on the twin's groups: a zero row is a zero row, every row whose
  twin quality is >= 1e-2 within 2^-22 per component (DESIGN.md section 19's bound for estimate_normals)."""
import ctypes

import numpy as np
import pytest
import torch

import knn_refs as KR
import plane_refs as PR
import prep_refs
from conftest import load_golden

pytestmark = pytest.mark.gpu

KS = [1, 3, 20, 32]
METHODS = ("brute", "tree")


@pytest.fixture(scope="module")
def mods():
    from rrl_hip import _lib, callsites, neighbors, ops
    return _lib, callsites, neighbors, ops


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.int32 if a.dtype.itemsize == 4 else np.int64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def cloud(kind, B, n, seed=0):
    """(B, n, 3) float32 of one of the test's cloud kinds."""
    g = np.random.default_rng(1000 * seed + n)
    if kind == "cube":
        x = g.uniform(-1, 1, (B, n, 3))
    elif kind == "sphere":
        x = g.standard_normal((B, n, 3))
        x /= np.linalg.norm(x, axis=-1, keepdims=True)
    elif kind == "identical":
        x = np.broadcast_to(g.uniform(-1, 1, (B, 1, 3)), (B, n, 3))
    elif kind == "lattice":  # many equal distances
        side = int(np.ceil(n ** (1 / 3)))
        a = np.arange(side)
        grid = np.stack(np.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3)
        x = np.stack([grid[g.permutation(len(grid))[:n]] for _ in range(B)])
    elif kind == "collinear":
        x = g.uniform(-1, 1, (B, n, 1)) * np.array([[[1.0, 2.0, -0.5]]])
    elif kind == "clusters":  # two far clusters
        x = g.uniform(-1, 1, (B, n, 3)) * 0.01
        x[:, n // 2:] += 500.0
    elif kind in ("nan", "huge"):  # the brute branch inside the tree launch, in one sample of the batch
        x = g.uniform(-1, 1, (B, n, 3))
        x[B - 1, n // 3, 1] = np.nan if kind == "nan" else 1e20
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(x, np.float32)


def check(nb, x, k, twin=None, what="", **kw):
    """Both methods against the twin: idx, found, dist2; returns the twin."""
    if twin is None:
        twin = KR.knn(x, k, **{a: (None if v is None else (v.cpu().numpy() if isinstance(v, torch.Tensor) else v)) for a, v in kw.items()})
    with np.errstate(over="ignore"):
        want_d = twin["d"].astype(np.float32)
    args = {a: (cuda(v) if isinstance(v, np.ndarray) else v) for a, v in kw.items()}
    outs = []
    for method in METHODS:
        idx, found, d2 = nb.knn(cuda(x), k, return_dist=True, method=method, **args)
        assert idx.dtype == torch.int32 and found.dtype == torch.int32 and d2.dtype == torch.float32
        assert np.array_equal(found.cpu().numpy(), twin["found"]), (what, method, "found")
        bad = (idx.cpu().numpy() != twin["idx"]).any(-1)
        assert not bad.any(), (what, method, "idx", int(bad.sum()), np.argwhere(bad)[:3].tolist())
        assert same_bits(d2, want_d), (what, method, "dist2")
        outs.append((idx, found, d2))
    for a, b in zip(*outs):
        assert same_bits(a, b), (what, "tree != brute")
    return twin


@pytest.mark.parametrize("k", KS)
def test_shapes_against_the_twin(mods, k):
    """n around 1, k, the supergroup of 64 and several supergroups; one and three clouds."""
    nb = mods[2]
    for n in sorted({1, 2, k - 1, k, k + 1, 63, 64, 65, 130, 257, 1025} - {0}):
        for B in (1, 3):
            twin = check(nb, cloud("cube", B, n, seed=k), k, what=(n, k, B))
            assert (twin["found"] == min(k, n)).all()


def test_the_other_sort_path(mods):
    """n = 4097: the records launch and the wide sort."""
    check(mods[2], cloud("sphere", 1, 4097), 20, what="4097")


@pytest.mark.parametrize("kind", ["cube", "sphere", "identical", "lattice", "collinear", "clusters", "nan", "huge"])
def test_cloud_kinds(mods, kind):
    nb = mods[2]
    for k in (3, 20):
        x = cloud(kind, 3, 257)
        twin = check(nb, x, k, what=(kind, k))
        if kind == "identical":  # ties by index only
            assert (twin["idx"] == np.arange(k)).all()
        if kind == "nan":
            assert twin["found"][2, 257 // 3] == 0 and not (twin["idx"][2] == 257 // 3).any()
        if kind == "huge":  # 1e20 squared is finite in double: the point is a neighbour like any other, far away
            assert twin["found"][2, 257 // 3] == k
    if kind in ("nan", "huge"):  # ... and the same branch with a query cloud
        x, q = cloud(kind, 2, 130), cloud("cube", 2, 70, seed=3)
        check(nb, x, 5, query=q, what=(kind, "cross"))
        check(nb, q, 5, query=x, what=(kind, "cross, the queries"))


def test_k3_is_knn3_self(mods):
    nb = mods[2]
    for x in (prep_refs.gaussian_cloud(7, 2, 300), prep_refs.lattice_cloud(3)[None, :1500]):
        tx = cuda(x)
        want = nb.knn3_self(tx, method="brute")
        for method in METHODS:
            idx, found = nb.knn(tx, 3, method=method)
            assert torch.equal(idx, want) and (found == 3).all()
    # n = 4225 = 66 supergroups + 1 record: the walk of rrl_knn_walk.h in both tree kernels, its flat loop in a second round,
    # on the records launch and the wide sort -- against the twin as well as against each other
    x = cloud("cube", 1, 4225, seed=6)
    tx = cuda(x)
    twin = KR.knn(x, 3)
    for method in METHODS:
        nn3 = nb.knn3_self(tx, method=method)
        idx, found = nb.knn(tx, 3, method=method)
        assert np.array_equal(nn3.cpu().numpy(), twin["idx"]), (method, "knn3_self against the twin")
        assert torch.equal(idx, nn3) and (found == 3).all(), method


def test_exclude_self_with_duplicates(mods):
    nb = mods[2]
    x = cloud("cube", 2, 130)
    x[:, 40:80] = x[:, :40]  # every one of these rows has a twin at another index
    for k in (1, 5, 32):
        twin = check(nb, x, k, exclude_self=True, what=("exclude_self", k))
        assert not (twin["idx"] == np.arange(130)[None, :, None]).any()
        assert (twin["idx"][:, :40, 0] == np.arange(40, 80)).all() and (twin["d"][:, :80, 0] == 0).all()
    x1 = cloud("cube", 1, 1)
    twin = check(nb, x1, 3, exclude_self=True, what="a lone point")
    assert not twin["found"].any()


@pytest.mark.parametrize("n", [130, 1025, 4225])
def test_cross_form(mods, n):
    nb = mods[2]
    if n == 4225:  # 66 full supergroups and one record: the walk's flat loop runs a second round; the queries shifted by +3 on
        x = cloud("sphere", 2, n)  # every axis, so that the seed is not the query supergroup's own index
        q = cloud("cube", 2, 130, seed=5) + np.float32(3.0)
        for k in (1, 3, 20):
            check(nb, x, k, query=q, what=("cross", n, 130, k, "shifted"))
        return
    x = cloud("sphere", 3, n)
    for S in (1, 70, n):
        q = cloud("cube", 3, S, seed=5)
        for k in (1, 20):
            check(nb, x, k, query=q, what=("cross", n, S, k))
    check(nb, x, 4, query=x.copy(), what="the cloud as its own query cloud")


def test_ragged_batches(mods):
    nb = mods[2]
    B, n, S, k = 5, 130, 70, 8
    x, q = cloud("cube", B, n), cloud("sphere", B, S, seed=2)
    counts, qcounts = [130, 0, 5, 64, 100], [70, 9, 0, 3, 65]
    for c in range(B):  # what lies beyond a count is never read
        x[c, counts[c]:] = np.nan
        q[c, qcounts[c]:] = np.nan
    twin = check(nb, x, k, counts=counts, what="ragged self")
    assert twin["found"][2, :5].tolist() == [5] * 5 and not twin["idx"][1].any() and not twin["idx"][2, 5:].any()
    twin = check(nb, x, k, query=q, counts=counts, qcounts=qcounts, what="ragged cross")
    assert not twin["found"][1].any() and not twin["found"][2].any() and twin["found"][3, :3].tolist() == [8] * 3
    # device-resident counts: the same, and out of range ones are clamped
    dc, dq = torch.tensor(counts, dtype=torch.int32, device="cuda"), torch.tensor(qcounts, dtype=torch.int32, device="cuda")
    for method in METHODS:
        a = nb.knn(cuda(x), k, query=cuda(q), counts=counts, qcounts=qcounts, return_dist=True, method=method)
        d = nb.knn(cuda(x), k, query=cuda(q), counts=dc, qcounts=dq, return_dist=True, method=method)
        assert all(same_bits(u, v) for u, v in zip(a, d))
        for c in range(B):  # sample b of a ragged batch == its own call
            if counts[c] and qcounts[c]:
                own = nb.knn(cuda(x[c:c + 1, :counts[c]]), k, query=cuda(q[c:c + 1, :qcounts[c]]), return_dist=True, method=method)
                assert all(same_bits(u[c, :qcounts[c]], v[0]) for u, v in zip(a, own))
                assert all(not u[c, qcounts[c]:].any() for u in a)
        fx, fq = cloud("cube", 2, n), cloud("sphere", 2, S)
        wild = torch.tensor([-7, 10 ** 6], dtype=torch.int32, device="cuda")
        i, f = nb.knn(cuda(fx), k, query=cuda(fq), counts=wild, qcounts=wild.flip(0), method=method)
        j, g = nb.knn(cuda(fx), k, query=cuda(fq), counts=[0, n], qcounts=[S, 0], method=method)
        assert torch.equal(i, j) and torch.equal(f, g) and not f.any()
        i, f = nb.knn(cuda(fx), k, counts=wild.flip(0), method=method)
        j, g = nb.knn(cuda(fx), k, counts=[n, 0], method=method)
        assert torch.equal(i, j) and torch.equal(f, g) and (f[0] == k).all()
    # the walk's rounds in one ragged batch of capacity 4225: 4225 = 66 supergroups + 1 record; 4161 = 65 + 1 record, where
    # supergroup 0 has kmax = 130 and a third round of two candidates; 65 = one full supergroup and one record; 64 = a single
    # supergroup, kmax = 0; 2 = found < k
    big, qbig = [4225, 4161, 65, 64, 2], [130, 64, 65, 2, 0]
    x, q = cloud("cube", B, 4225, seed=9), cloud("sphere", B, 130, seed=9)
    for c in range(B):
        x[c, big[c]:] = np.nan
        q[c, qbig[c]:] = np.nan
    twin = check(nb, x, k, counts=big, what="ragged self, 4225")
    assert twin["found"][4, :2].tolist() == [2, 2] and (twin["found"][3, :64] == k).all() and not twin["idx"][3, 64:].any()
    twin = check(nb, x, k, query=q, counts=big, qcounts=qbig, what="ragged cross, 4225")
    assert (twin["found"][0] == k).all() and twin["found"][3, :2].tolist() == [k, k] and not twin["found"][4].any()


def test_features(mods):
    """Every channel subset in both layouts: exact gathers and float32 subtractions, pads repeat slot 0, zero rows are zero."""
    nb = mods[2]
    B, n, k = 2, 70, 6
    x = cloud("cube", B, n)
    x[0, 7, 0] = np.nan  # a zero row inside a sample
    counts = [70, 4]     # found < k in sample 1, rows beyond its count
    twin = KR.knn(x, k, counts=counts)
    assert twin["found"][1, :4].tolist() == [4] * 4
    q = cloud("sphere", B, 9, seed=4)
    twin_q = KR.knn(x, k, query=q, counts=counts)
    names = KR.FEATURES
    for mask in range(1, 8):
        sub = tuple(f for i, f in enumerate(names) if mask >> i & 1)
        for cf in (False, True):
            for method in METHODS:
                feat, idx, found = nb.knn_group(cuda(x), k, features=sub[::-1], channel_first=cf, counts=counts, method=method)
                assert np.array_equal(idx.cpu().numpy(), twin["idx"]) and np.array_equal(found.cpu().numpy(), twin["found"])
                want = KR.features(x, twin, sub, channel_first=cf)
                assert tuple(feat.shape) == want.shape and same_bits(feat, want), (sub, cf, method)
                feat, idx, found = nb.knn_group(cuda(x), k, features=sub, channel_first=cf, query=cuda(q), counts=counts, method=method)
                assert same_bits(feat, KR.features(x, twin_q, sub, query=q, channel_first=cf)), (sub, cf, method, "cross")
    feat = nb.knn_group(cuda(x), k, features=names, counts=counts)[0].cpu().numpy()
    assert (feat[1, :4, 4:] == feat[1, :4, :1]).all() and not feat[1, 4:].any() and not np.isnan(feat).any()
    assert np.array_equal(feat[0, :, :, 3:6], feat[0, :, :, 0:3] - feat[0, :, :, 6:9])


def dcp_formulation(x, k):
    """dcp/model.py:46-52 restated: x (B, 3, N) -> (B, N, k) indices by topk of -|xi|^2 + 2 xi.xj - |xj|^2 in float32."""
    inner = -2 * torch.matmul(x.transpose(2, 1).contiguous(), x)
    xx = torch.sum(x ** 2, dim=1, keepdim=True)
    return (-xx - inner - xx.transpose(2, 1).contiguous()).topk(k=k, dim=-1)[1]


@pytest.mark.parametrize("name", list(KR.DCP_CASES))
def test_dcp_call_sites(mods, name):
    cs = mods[1]
    g = load_golden("knn_dcp.npz")
    x = g[f"{name}_xyz"]
    tx = cuda(x).transpose(2, 1).contiguous()  # channel-first, as DCP holds its clouds
    for k in KR.DCP_KS:
        twin = KR.knn(x, k)
        keep = ~twin["border"]
        assert twin["border"].mean() <= KR.BORDER_SHARE_MAX
        idx = cs.dcp_knn(tx, k)
        assert idx.dtype == torch.int64 and np.array_equal(idx.cpu().numpy(), twin["idx"])
        assert np.array_equal(idx.cpu().numpy()[keep], g[f"{name}_k{k}_idx"].astype(np.int64)[keep]), (name, k, "the recorded reference")
        there = dcp_formulation(tx, k).cpu().numpy()
        print(f"{name} k={k}: borderline {100 * twin['border'].mean():.2f} %, rows differing from the matmul form {int((there != twin['idx']).any(-1).sum())}")
        assert np.array_equal(idx.cpu().numpy()[keep], there[keep]), (name, k, "the matmul formulation on this GPU")
        feat = cs.dcp_graph_feature(tx, k)
        assert tuple(feat.shape) == (x.shape[0], 6, x.shape[1], k)
        assert same_bits(feat, KR.features(x, twin, ("nbr", "ctr"), channel_first=True))
    with pytest.raises(ValueError):
        cs.dcp_knn(tx[:, :, :10], 11)


@pytest.mark.parametrize("n, k", [(65, 8), (257, 20), (1025, 20)])
def test_estimate_normals_knn(mods, n, k):
    from rrl_hip import synth
    nb = mods[2]
    x = np.stack([synth.surface_cloud(300 + n + 1000 * b, n) for b in range(2)])
    counts = [n, n - 7]
    g = KR.knn(x, k, counts=counts)
    twin = PR.idx_normals(x, g["idx"], g["found"], counts)
    normals, quality = nb.estimate_normals_knn(cuda(x), k, counts=counts, return_quality=True)
    got, tn, tq = normals.cpu().numpy(), twin["normals"], twin["quality"]
    zero = ~tn.any(-1)
    assert not got[zero].any() and not got[1, n - 7:].any()
    live = (~zero) & (tq >= 1e-2)
    err = np.abs(got[live].astype(np.float64) - tn[live]).max()
    print(f"n={n} k={k}: {int(live.sum())} rows of {2 * n}, worst normal error {err / 2.0 ** -22:.3f} of 2^-22")
    assert live.sum() >= n and err <= 2.0 ** -22
    assert same_bits(nb.estimate_normals_knn(cuda(x), k, counts=counts), normals)


def test_repeats_and_graph_replay(mods):
    nb = mods[2]
    tx, tq = cuda(cloud("sphere", 2, 1025)), cuda(cloud("cube", 2, 300, seed=8))
    for method in METHODS:
        for kw in (dict(), dict(query=tq)):
            def call():
                return nb.knn_group(tx, 20, features=("nbr", "dxyz", "ctr"), channel_first=True, method=method, **kw) + \
                    (nb.knn(tx, 20, return_dist=True, method=method, **kw)[2],)
            first = call()
            assert all(same_bits(u, v) for u, v in zip(first, call()))
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                call()
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                outs = call()
            for _ in range(2):
                for o in outs:
                    o.zero_()
                graph.replay()
                torch.cuda.synchronize()
                assert all(same_bits(u, v) for u, v in zip(first, outs)), (method, sorted(kw))


@pytest.mark.parametrize("n", [65, 4097])
def test_scratch_guard_band(mods, n):
    """The three entries that build the sorted layout in a scratch of their own (PairLayout, rrl_tree.h) stay inside the bytes their
    size functions return: each runs in the first workspace_bytes bytes of a buffer with 4096 more bytes of 0xA5 behind them, which
    stay 0xA5, and gives the bits of a call on a plain buffer.  n = 65: the sort from the points; n = 4097: records launch + wide sort."""
    ops = mods[3]
    B, S, k = 2, 70, 5
    x, y, q = cuda(cloud("cube", B, n, seed=11)), cuda(cloud("sphere", B, n - 1, seed=12)), cuda(cloud("cube", B, S, seed=13))
    dev, P = x.device, ops._p

    def chamfer(ws, nb):
        bx, by = torch.zeros(B, n, dtype=torch.int64, device=dev), torch.zeros(B, n - 1, dtype=torch.int64, device=dev)
        value = torch.zeros(1, device=dev)
        ops._run(dev, "rrl_chamfer_tree_fwd_ex", P(x), P(y), P(ws), nb, P(bx), P(by), P(value), B, n, n - 1, None, None, None, 0)
        return bx, by, value

    def knn3(ws, nb):
        nn, tri = torch.zeros(B, n, 3, dtype=torch.int32, device=dev), torch.zeros(B, n, 9, device=dev)
        ops._run(dev, "rrl_knn3_self", P(x), None, P(ws), nb, P(nn), P(tri), None, B, n)
        return nn, tri

    def knn(query):
        def call(ws, nb):
            Sq = n if query is None else S
            idx, found = torch.zeros(B, Sq, k, dtype=torch.int32, device=dev), torch.zeros(B, Sq, dtype=torch.int32, device=dev)
            d2 = torch.zeros(B, Sq, k, device=dev)
            ops._run(dev, "rrl_knn", P(x), None, P(query), None, k, 0, 0, P(ws), nb, P(idx), P(found), P(d2), None, B, n, Sq)
            return idx, found, d2
        return call

    for what, call, size in (("chamfer", chamfer, ("rrl_chamfer_workspace_bytes", B, n, n - 1)),
                             ("knn3_self", knn3, ("rrl_knn3_self_workspace_bytes", B, n)),
                             ("knn self", knn(None), ("rrl_knn_workspace_bytes", B, n, n)),
                             ("knn cross", knn(q), ("rrl_knn_workspace_bytes", B, n, S))):
        nb = ops._scratch_size(*size)
        assert nb > 0
        guarded = torch.full((nb + 4096,), 0xA5, dtype=torch.uint8, device=dev)
        got = call(guarded, nb)
        want = call(torch.full((nb,), 0x5A, dtype=torch.uint8, device=dev), nb)
        torch.cuda.synchronize()
        assert (guarded[nb:] == 0xA5).all(), (what, n, "bytes behind the scratch were written")
        assert all(same_bits(u, v) for u, v in zip(got, want)), (what, n)


def test_c_level_refusals(mods):
    _lib, _, _, ops = mods
    lib = _lib.load()
    B, n, S, k = 2, 10, 4, 3
    ref, qry = torch.zeros(B, n, 3, device="cuda"), torch.zeros(B, S, 3, device="cuda")
    idx = torch.full((B, n, k), -5, dtype=torch.int32, device="cuda")
    feat = torch.full((B, n, k, 3), -5.0, device="cuda")
    nbytes = lib.rrl_knn_workspace_bytes(B, n, n)
    assert nbytes > 0 and lib.rrl_knn_workspace_bytes(-1, n, n) == 0
    ws = torch.empty(lib.rrl_knn_workspace_bytes(B, n, S), dtype=torch.uint8, device="cuda")
    P, E_ARG, E_WS = ops._p, _lib.CONSTANTS["RRL_E_ARG"], _lib.CONSTANTS["RRL_E_WS"]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(ref_=ref, qry_=None, k_=k, flags=0, ch=0, ws_=ws, wsb=None, idx_=idx, feat_=None, B_=B, n_=n, S_=n):
        return lib.rrl_knn(P(ref_), None, P(qry_), None, k_, flags, ch, P(ws_), ws_.numel() if wsb is None and ws_ is not None else (wsb or 0),
                           P(idx_), None, None, P(feat_), B_, n_, S_, stream)
    for kw in (dict(ref_=None), dict(idx_=None), dict(ws_=None), dict(B_=-1), dict(B_=32768), dict(n_=0, S_=0), dict(S_=-1), dict(k_=0),
               dict(k_=33), dict(S_=S), dict(flags=8), dict(ch=8), dict(ch=1), dict(feat_=feat), dict(qry_=qry, S_=-1)):
        assert call(**kw) == E_ARG, kw
    assert call(wsb=nbytes - 1) == E_WS and call(qry_=qry, S_=S, wsb=16) == E_WS
    assert call(B_=0) == 0 and call(qry_=qry, S_=0) == 0
    torch.cuda.synchronize()
    assert (idx == -5).all() and (feat == -5).all()  # nothing ran
    assert call(ch=1, feat_=feat) == 0 and call(flags=4, k_=32, n_=n, idx_=torch.empty(B, n, 32, dtype=torch.int32, device="cuda")) == 0  # k > n is legal
    torch.cuda.synchronize()
    assert (idx == torch.arange(k, device="cuda", dtype=torch.int32)).all() and not feat.any()  # ten points at the origin: index order, their coordinates
