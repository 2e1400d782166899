"""The device-side pseudo-triangle builder on the GPU (include/rrl.h rrl_fps_counted, rrl_knn3_counted, rrl_knn3_self;
rrl_hip.neighbors.pseudo_triangles / knn3_self), all by EQUALITY: the tree walk against prep_refs.knn3_ref
(float64 distances, ties to the lower index) on every cloud kind that can break a pruning bound or a tie, against the
brute-force kernel where the twin is too large, and the counted entries against tests/neigh_refs.py -- sample b of a ragged
call gives what the B = 1 call on its truncated cloud gives, rows beyond a count (filled with NaN) are never read."""
import numpy as np
import pytest
import torch

import neigh_refs as NR
import prep_refs as PF
from conftest import load_golden

pytestmark = pytest.mark.gpu


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def NB():
    from rrl_hip import _lib, neighbors
    _lib.load()
    assert torch.cuda.is_available()
    return neighbors


def tree_nn(NB, pts, counts=None):
    return NB.knn3_self(cu(pts), counts=counts, method="tree").cpu().numpy()


def ref_nn(pts):
    """(B, n, 3): knn3_ref of every point, per cloud."""
    return np.stack([NR.knn3_chunked(p, np.arange(len(p))) for p in pts])


# ----------------------------------------------------------------------------------------------------------------- the tree
@pytest.mark.parametrize("B, n", [(3, 3), (3, 4), (3, 63), (3, 64), (3, 65), (3, 255), (3, 256), (3, 257), (3, 1025),
                                  (1, 4096), (1, 4097)])
def test_tree_equals_the_twin_on_gaussian_clouds(NB, B, n):
    """Supergroup edges (64), group edges, several supergroups, and both sides of the small / large build switch (4096)."""
    pts = PF.gaussian_cloud(1000 + n, B, n)
    got = tree_nn(NB, pts)
    assert got.shape == (B, n, 3) and got.dtype == np.int32
    np.testing.assert_array_equal(got, ref_nn(pts))
    np.testing.assert_array_equal(NB.knn3_self(cu(pts), method="brute").cpu().numpy(), got)


def _collinear():
    t = np.random.default_rng(7).uniform(-3.0, 3.0, 200).astype(np.float32)
    return (t[:, None] * np.array([0.5, -1.25, 2.0], np.float32)[None, :] + np.float32(0.75)).astype(np.float32)


def _clusters():
    c = PF.gaussian_cloud(9, 2, 512)
    c[1] += np.float32(1.0e5)
    return c.reshape(-1, 3)[np.random.default_rng(10).permutation(1024)]


DEGENERATE = {
    "lattice": lambda: PF.lattice_cloud(43),            # ties everywhere, copies with a twin at a lower index
    "far": lambda: PF.far_cloud(41),                    # coordinates of 2e5
    "identical": lambda: np.full((130, 3), 0.375, np.float32),
    "collinear": _collinear,
    "clusters": _clusters,                              # two 512-point clusters 1e5 apart
}


@pytest.mark.parametrize("kind", list(DEGENERATE))
def test_tree_equals_the_twin_on_degenerate_clouds(NB, kind):
    pts = DEGENERATE[kind]()[None]
    got = tree_nn(NB, pts)
    np.testing.assert_array_equal(got, ref_nn(pts))
    if kind == "identical":
        np.testing.assert_array_equal(got[0], np.tile(np.arange(3), (130, 1)))
    if kind == "lattice":  # a copy finds its twin at the lower index first
        k = PF.LATTICE_SIDE ** 3
        assert np.all(got[0, k:, 0] < k)


def test_tree_equals_the_brute_force_kernel_beyond_65536(NB):
    """n = 65537: the numpy twin is too large there; the brute-force kernel is itself pinned to it (test_gpu_prep_kernels)."""
    n = 65537
    pts = cu(PF.gaussian_cloud(65537, 1, n))
    want = NB.knn3(pts, torch.arange(n, dtype=torch.int32)[None])
    got = NB.knn3_self(pts, method="tree")
    assert torch.equal(got, want)


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_non_finite_coordinates_take_the_brute_force_loop(NB, bad):
    pts = PF.gaussian_cloud(300, 2, 300)
    pts[1, 123, 1] = bad
    t = cu(pts)
    want = NB.knn3(t, torch.arange(300, dtype=torch.int32)[None].expand(2, -1).contiguous())
    assert torch.equal(NB.knn3_self(t, method="tree"), want)
    np.testing.assert_array_equal(want[0].cpu().numpy(), ref_nn(pts[:1])[0])  # the finite sample beside it: the tree, the twin


# ----------------------------------------------------------------------------------------------------------------- ragged
RAG_CAP, RAG_COUNTS = 1100, [1100, 700, 3, 2]


@pytest.fixture(scope="module")
def ragged():
    pts = PF.gaussian_cloud(21, 4, RAG_CAP)
    for b, c in enumerate(RAG_COUNTS):
        pts[b, c:] = np.nan
    start = [17, 699, 2, 1]
    return dict(pts=pts, start=start, full=NR.pseudo_triangles_ref(pts, counts=RAG_COUNTS),
                sub=NR.pseudo_triangles_ref(pts, counts=RAG_COUNTS, num_sample=500, start=start))


@pytest.mark.parametrize("method", ["tree", "brute"])
@pytest.mark.parametrize("device_counts", [True, False])
def test_ragged_all_points(NB, ragged, method, device_counts):
    """Every sample equals the call on its truncated cloud (the twin, and the B = 1 call itself), rows beyond a count are
    zero, tri_counts = (1100, 700, 3, 0)."""
    t = cu(ragged["pts"])
    counts = cu(np.array(RAG_COUNTS, np.int32)) if device_counts else RAG_COUNTS
    tri, tc, idx, nn = NB.pseudo_triangles(t, counts=counts, method=method, return_index=True)
    want = ragged["full"]
    assert tc.dtype == torch.int32 and tc.tolist() == [1100, 700, 3, 0] == want["tri_counts"].tolist()
    np.testing.assert_array_equal(nn.cpu().numpy(), want["nn"])
    np.testing.assert_array_equal(tri.cpu().numpy().view(np.uint32), want["tri"].view(np.uint32))
    assert tri.grad_fn is None and idx[1].tolist() == list(range(RAG_CAP))
    np.testing.assert_array_equal(NB.knn3_self(t, counts=counts, method=method).cpu().numpy(), want["nn"])
    for b, c in enumerate(RAG_COUNTS[:3]):
        t1, none, _, nn1 = NB.pseudo_triangles(t[b:b + 1, :c].contiguous(), method=method, return_index=True)
        assert none is None and torch.equal(nn1[0], nn[b, :c]) and torch.equal(t1[0].view(torch.int32), tri[b, :c].view(torch.int32))


@pytest.mark.parametrize("device_counts", [True, False])
def test_ragged_sampled(NB, ragged, device_counts):
    """num_sample = 500: S_b = (500, 500, 3, 0) triangles; the sampler's indices are those of the B = 1 call."""
    t = cu(ragged["pts"])
    counts = cu(np.array(RAG_COUNTS, np.int32)) if device_counts else RAG_COUNTS
    start = cu(np.array(ragged["start"], np.int32)) if device_counts else torch.tensor(ragged["start"])
    tri, tc, idx, nn = NB.pseudo_triangles(t, 500, counts=counts, start=start, return_index=True)
    want = ragged["sub"]
    assert tc.tolist() == [500, 500, 3, 0] == want["tri_counts"].tolist() and tuple(tri.shape) == (4, 500, 9)
    np.testing.assert_array_equal(idx.cpu().numpy(), want["idx"])
    np.testing.assert_array_equal(nn.cpu().numpy(), want["nn"])
    np.testing.assert_array_equal(tri.cpu().numpy().view(np.uint32), want["tri"].view(np.uint32))
    for b, c in enumerate(RAG_COUNTS[:3]):
        t1, _, i1, nn1 = NB.pseudo_triangles(t[b:b + 1, :c].contiguous(), 500, start=torch.tensor(ragged["start"][b:b + 1]),
                                             return_index=True)
        s = min(500, c)
        assert tuple(i1.shape) == (1, s) and torch.equal(i1[0], idx[b, :s]) and torch.equal(nn1[0], nn[b, :s])
        assert torch.equal(t1[0].view(torch.int32), tri[b, :s].view(torch.int32))
        assert torch.equal(NB.fps(t[b:b + 1, :c].contiguous(), 500, start=torch.tensor(ragged["start"][b:b + 1]))[0], idx[b, :s])


def test_counts_at_the_capacity_give_the_uniform_calls_bits(NB):
    pts = cu(PF.gaussian_cloud(23, 3, 700))
    full = cu(np.full(3, 700, np.int32))
    start = torch.tensor([5, 699, 0])
    for method in ("tree", "brute"):
        a = NB.pseudo_triangles(pts, method=method, return_index=True)
        b = NB.pseudo_triangles(pts, counts=full, method=method, return_index=True)
        assert a[1] is None and b[1].tolist() == [700] * 3
        assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[3], b[3])
    a = NB.pseudo_triangles(pts, 200, start=start, return_index=True)
    b = NB.pseudo_triangles(pts, 200, counts=full, start=start, return_index=True)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    assert torch.equal(a[2], NB.fps(pts, 200, start=start)) and torch.equal(a[3], NB.knn3(pts, a[2]))


BIG_CAP = 5000  # beyond 4096: the records launch + the histogram / scatter / sphere kernels build the tree


def _brute_rows(NB, t, b, c):
    """The brute-force kernel (pinned to the twin by test_gpu_prep_kernels) on sample b's truncated cloud: (c, 3)."""
    return NB.knn3(t[b:b + 1, :c].contiguous(), torch.arange(c, dtype=torch.int32)[None])[0]


@pytest.mark.parametrize("device_counts", [True, False])
def test_ragged_on_the_large_build(NB, device_counts):
    """Capacity 5000 with counts at it, between 4096 and it, below 4096 and below three, NaN beyond every count: each sample
    equals the brute-force kernel on its truncated cloud, rows beyond are zero, tri_counts = (5000, 4100, 700, 0)."""
    counts = [BIG_CAP, 4100, 700, 2]
    pts = PF.gaussian_cloud(71, 4, BIG_CAP)
    for b, c in enumerate(counts):
        pts[b, c:] = np.nan
    t = cu(pts)
    cnt = cu(np.array(counts, np.int32)) if device_counts else counts
    tri, tc, _, nn = NB.pseudo_triangles(t, counts=cnt, method="tree", return_index=True)
    assert tc.tolist() == [BIG_CAP, 4100, 700, 0]
    for b, c in enumerate(counts):
        live = c if c >= 3 else 0
        assert not nn[b, live:].any() and not tri[b, live:].any()
        if live:
            want = _brute_rows(NB, t, b, c)
            assert torch.equal(nn[b, :c], want)
            assert torch.equal(tri[b, :c].view(torch.int32), t[b][want.long().reshape(-1)].reshape(c, 9).view(torch.int32))
    assert torch.equal(NB.knn3_self(t, counts=cnt, method="brute"), nn)


@pytest.mark.parametrize("bad", [np.nan, -np.inf])
def test_non_finite_coordinates_on_the_large_build(NB, bad):
    """One bad coordinate inside the count of one sample of three at capacity 5000 (and one beyond another sample's count,
    which must not matter): the flagged sample takes the brute-force loop, the others the tree; all equal rrl_knn3."""
    counts = [BIG_CAP, 4500, 4200]
    pts = PF.gaussian_cloud(73, 3, BIG_CAP)
    pts[1, 4321, 2] = bad   # inside sample 1's count
    pts[2, 4300, 0] = bad   # beyond sample 2's count: never read
    t = cu(pts)
    got = NB.knn3_self(t, counts=cu(np.array(counts, np.int32)), method="tree")
    for b, c in enumerate(counts):
        assert torch.equal(got[b, :c], _brute_rows(NB, t, b, c)) and not got[b, c:].any()
    np.testing.assert_array_equal(got[2, :4200].cpu().numpy(), NR.knn3_chunked(pts[2, :4200], np.arange(4200)))


# ----------------------------------------------------------------------------------------------------------------- counted FPS
def _fps_counted(NB, pts, counts, start, S):
    from rrl_hip.ops import _p, _run
    t = cu(pts)
    B, n, _ = pts.shape
    out = torch.full((B, S), -7, dtype=torch.int32, device="cuda")
    oc = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    scratch = torch.empty(B, n, dtype=torch.float32, device="cuda")
    cnt = cu(np.asarray(counts, np.int32)) if counts is not None else None
    _run(t.device, "rrl_fps_counted", _p(t), _p(cnt), _p(cu(np.asarray(start, np.int32))), _p(out), _p(oc), _p(scratch), B, n, S)
    return out.cpu().numpy(), oc.cpu().numpy()


def test_counted_fps_at_the_lane_and_trip_edges(NB):
    """prep_refs.FPS_N as COUNTS inside a capacity of 2100, NaN beyond them: S_b = n_b indices, fps_ref's, zeros beyond."""
    cap, counts = 2100, PF.FPS_N
    pts = PF.gaussian_cloud(31, len(counts), cap)
    for b, c in enumerate(counts):
        pts[b, c:] = np.nan
    start = [0 if c < 3 else c - 2 for c in counts]
    want, sb = NR.fps_counted_ref(pts, counts, cap, start)
    got, oc = _fps_counted(NB, pts, counts, start, cap)
    assert oc.tolist() == sb.tolist() == counts
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("cap", [PF.FPS_LDS_MAX, PF.FPS_LDS_MAX + 1])
def test_counted_fps_on_both_sides_of_the_lds_switch(NB, cap):
    """Capacities 8192 (points in LDS) and 8193 (global memory), a count below and one at the capacity; NULL counts give
    rrl_fps's bits."""
    pts = PF.gaussian_cloud(33, 2, cap)
    counts, start, S = [cap, 5000], [cap - 1, 4999], 48
    pts[1, 5000:] = np.nan
    want, sb = NR.fps_counted_ref(pts, counts, S, start)
    got, oc = _fps_counted(NB, pts, counts, start, S)
    assert oc.tolist() == [S, S]
    np.testing.assert_array_equal(got, want)
    clean = PF.gaussian_cloud(33, 2, cap)
    got0, _ = _fps_counted(NB, clean, None, start, S)
    np.testing.assert_array_equal(got0, NB.fps(cu(clean), S, start=torch.tensor(start)).cpu().numpy())


# ----------------------------------------------------------------------------------------------------------------- given queries
def test_counted_knn3_for_given_queries(NB):
    """prep_refs.KNN_SHAPES as (n_b, S_b) inside a capacity of (2100, 800), NaN points and out-of-count queries beyond."""
    shapes = PF.KNN_SHAPES
    B, cap, S = len(shapes), 2100, 800
    g = np.random.default_rng(35)
    pts = PF.gaussian_cloud(35, B, cap)
    q = np.full((B, S), cap - 1, np.int64)
    for b, (n, s) in enumerate(shapes):
        pts[b, n:] = np.nan
        q[b, :s] = g.integers(0, n, s)
    counts, qcounts = [n for n, _ in shapes], [s for _, s in shapes]
    want = np.zeros((B, S, 3), np.int64)
    for b, (n, s) in enumerate(shapes):
        want[b, :s] = NR.knn3_chunked(pts[b, :n], q[b, :s])
    for dev in (True, False):
        c, qc = (cu(np.array(x, np.int32)) if dev else x for x in (counts, qcounts))
        qi = cu(q.astype(np.int32)) if dev else torch.from_numpy(np.where(np.arange(S)[None] < np.array(qcounts)[:, None], q, 0))
        np.testing.assert_array_equal(NB.knn3_counted(cu(pts), qi, counts=c, qcounts=qc).cpu().numpy(), want)


# ----------------------------------------------------------------------------------------------------------------- end to end
def test_golden_sample_neighs(NB):
    """The reference's recorded rows (tests/golden/sample_neighs.npz), as test_sample_neighs_vs_reference reads them."""
    g = load_golden("sample_neighs.npz")
    pts = torch.from_numpy(g["points"])[None]
    torch.manual_seed(78)
    tri, tc = NB.pseudo_triangles(pts, num_sample=300)
    assert tc is None and tri.is_cuda and tuple(tri.shape) == (1, 300, 9)
    np.testing.assert_array_equal(tri.cpu().numpy().reshape(-1, 3), g["sub"])
    torch.manual_seed(77)
    tri, _ = NB.pseudo_triangles(pts, num_sample=5000)  # Sample_neighs's default sample count
    np.testing.assert_array_equal(tri.cpu().numpy().reshape(-1, 3), g["full"])


def test_ragged_batches_feed_the_loss_without_a_read_back(NB):
    """A ragged pair of batches built on the device, handed with tri_counts and orders to the loss: the same loss and info
    bits as the same call on triangles built by the host twin."""
    import loss as L
    from rrl_hip import ops
    g = np.random.default_rng(51)
    p1, p2 = PF.gaussian_cloud(52, 3, 600), PF.gaussian_cloud(53, 3, 500)
    c1, c2 = [600, 333, 64], [257, 500, 100]
    for b in range(3):
        p1[b, c1[b]:] = np.nan
        p2[b, c2[b]:] = np.nan
    d = g.standard_normal((3, 1500, 3)).astype(np.float32)
    d /= np.linalg.norm(d.astype(np.float64), axis=-1, keepdims=True).astype(np.float32)
    lines = cu(np.concatenate([d, (0.3 * g.standard_normal((3, 1500, 3))).astype(np.float32)], -1))
    dc1, dc2 = cu(np.array(c1, np.int32)), cu(np.array(c2, np.int32))
    t1, tc1, o1 = NB.pseudo_triangles(cu(p1), counts=dc1, method="tree", order=True)
    t2, tc2, o2 = NB.pseudo_triangles(cu(p2), counts=dc2, method="brute", order=True)
    loss, info, status = ops.intersection_loss(t1, t2, lines, mode="cull", counts1=tc1, counts2=tc2, order1=o1, order2=o2)
    la, valid = L.batched_intersection_loss(t1, t2, lines, counts1=tc1, counts2=tc2)
    r1, r2 = NR.pseudo_triangles_ref(p1, counts=c1), NR.pseudo_triangles_ref(p2, counts=c2)
    h1, h2 = cu(r1["tri"]), cu(r2["tri"])
    hc1, hc2 = cu(r1["tri_counts"].astype(np.int32)), cu(r2["tri_counts"].astype(np.int32))
    wl, wi, _ = ops.intersection_loss(h1, h2, lines, mode="cull", counts1=hc1, counts2=hc2,
                                      order1=ops.cloud_order(h1, counts=hc1), order2=ops.cloud_order(h2, counts=hc2))
    wa, wv = L.batched_intersection_loss(h1, h2, lines, counts1=hc1, counts2=hc2)
    assert torch.equal(loss.view(torch.int32), wl.view(torch.int32)) and torch.equal(info, wi)
    assert torch.equal(la.view(torch.int32), wa.view(torch.int32)) and torch.equal(valid, wv)
    assert torch.equal(la.view(torch.int32), loss.detach().view(torch.int32))
    assert int(info[:, 0].sum()) > 0, "no line selected in any sample: the comparison would be vacuous"


# ----------------------------------------------------------------------------------------------------------------- capture
@pytest.mark.parametrize("num_sample, method", [(None, "tree"), (None, "brute"), (200, "auto")])
def test_capture_and_replay(NB, num_sample, method):
    """Device counts and a given start: nothing synchronises, so the call is captured once and replayed after the points and
    counts were rewritten in place; the replay equals a fresh call on the new data."""
    a, b = PF.gaussian_cloud(61, 2, 900), PF.gaussian_cloud(62, 2, 900)
    pts, cnt = cu(a), cu(np.array([900, 411], np.int32))
    start = cu(np.array([3, 400], np.int32)) if num_sample else None
    NB.pseudo_triangles(pts, num_sample, counts=cnt, start=start, method=method, order=True, return_index=True)  # warm-up
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = NB.pseudo_triangles(pts, num_sample, counts=cnt, start=start, method=method, order=True, return_index=True)
    pts.copy_(cu(b))
    cnt.copy_(cu(np.array([77, 900], np.int32)))
    if num_sample:
        start.copy_(cu(np.array([76, 5], np.int32)))
    graph.replay()
    torch.cuda.synchronize()
    fresh = NB.pseudo_triangles(pts, num_sample, counts=cnt, start=start, method=method, order=True, return_index=True)
    assert fresh[1].tolist() == ([77, 900] if num_sample is None else [77, 200])
    for got, want in zip(out, fresh):
        assert torch.equal(got.view(torch.int32) if got.dtype == torch.float32 else got, want.view(torch.int32) if want.dtype == torch.float32 else want)
