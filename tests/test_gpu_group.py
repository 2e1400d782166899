"""rrl_ball_group on the GPU (neighbors.ball_query / ball_group, callsites.rpm_raw_features / rpm_sample_and_group_multi)
against the host twin tests/group_refs.py: indices, found and dxyz bit for bit, the xyz channel bit for bit, an angle within
2^-20 rad, |d| within 3 * 2^-24 of itself, pad slots exactly 0.  The bounds come from the rule, none is
measured; each test prints the worst observed ratio to its bound."""
import numpy as np
import pytest
import torch

import group_refs as GR
from conftest import load_golden

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 130, 257, 1025]  # both sides of the 64-candidate tile, several tiles, more than one workgroup
NSAMPLES = [1, 8, 64]


@pytest.fixture(scope="module")
def nb():
    from rrl_hip import neighbors
    return neighbors


def cloud(seed, B, n):
    rs = np.random.default_rng(seed)
    x = rs.uniform(-1.0, 1.0, (B, n, 3)).astype(np.float32)
    nr = rs.standard_normal((B, n, 3))
    return x, (nr / np.linalg.norm(nr, axis=-1, keepdims=True)).astype(np.float32)


def radii(n, nsample):
    """Three radii for n uniform points in [-1, 1]^3: (almost) every row empty, about nsample / 2 expected members -- rows
    partly filled, some empty, some truncated --, and every other point a member (truncated wherever n - 1 >= nsample)."""
    mid = (min(max(nsample / 2.0, 1.5), n / 4.0 + 1.0) * 8.0 / (n * 4.18879)) ** (1.0 / 3.0)
    return (0.01, float(min(mid, 1.5)), 4.0)


def bits(a):
    """float32 -> its bit patterns, every NaN as one pattern (which NaN a subtraction of NaNs returns is the machine's choice)."""
    a = np.ascontiguousarray(a)
    if a.dtype != np.float32:
        return a
    return np.where(np.isnan(a), np.uint32(0x7fc00000), a.view(np.uint32))


def compare(got, want, features, exclude_self, what):
    """got: (feat, idx, found) tensors; want: the twin's dict.  Returns (angle error / bound, |d| error / bound)."""
    feat, idx, found = got
    assert idx.dtype == torch.int32 and found.dtype == torch.int32
    assert np.array_equal(idx.cpu().numpy(), want["idx"]), what
    assert np.array_equal(found.cpu().numpy(), want["found"]), what
    if feat is None:
        return 0.0, 0.0
    f = feat.cpu().numpy()
    assert f.dtype == np.float32 and f.shape == want["feat"].shape, what
    at = 0
    ratios = (0.0, 0.0)
    for name in GR.FEATURES:
        if name not in features:
            continue
        if name == "xyz":
            assert np.array_equal(bits(f[..., at:at + 3]), bits(want["feat"][..., at:at + 3].astype(np.float32))), what
        elif name == "dxyz":
            assert np.array_equal(bits(f[..., at:at + 3]), bits(want["dxyz"])), what
        else:
            finite = np.isfinite(want["feat"][..., at:at + 4]).all(-1)
            assert np.array_equal(np.isfinite(f[..., at:at + 4]).all(-1), finite), what
            ang, rel = GR.ppf_errors(f[finite], want["feat"][finite], at)
            assert ang <= GR.ANGLE_TOL and rel <= GR.NORM_RTOL, (what, ang, rel)
            if exclude_self:
                pad = (np.arange(f.shape[2])[None, None, :] >= want["found"][..., None]) & finite
                assert not f[pad][:, at - 3 if "dxyz" in features else at:].any(), what  # d = 0: dxyz and ppf exactly 0
            ratios = (ang / GR.ANGLE_TOL, rel / GR.NORM_RTOL)
        at += GR.SIZES[name]
    return ratios


def run(nb, x, nr, radius, nsample, features=GR.FEATURES, **kw):
    tk = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
    if not features:
        return (None,) + tuple(nb.ball_query(torch.from_numpy(x).cuda(), radius, nsample, **tk))
    return nb.ball_group(torch.from_numpy(x).cuda(), None if nr is None else torch.from_numpy(nr).cuda(), radius, nsample,
                         features=features, **tk)


@pytest.mark.parametrize("n", SIZES)
def test_grouping_and_features_equal_the_twin(nb, n):
    """B = 3 and, from the same twin (a sample is its own call), B = 1; every nsample at three radii; both pad rules."""
    x, nr = cloud(100 + n, 3, n)
    worst = [0.0, 0.0]
    kinds = set()
    for nsample in NSAMPLES:
        for radius in radii(n, nsample):
            for excl in ((True, False) if nsample == 8 else (True,)):
                want = GR.ball_group(x, nr, radius, nsample, GR.FEATURES, exclude_self=excl)
                r = compare(run(nb, x, nr, radius, nsample, exclude_self=excl), want, GR.FEATURES, excl, (n, nsample, radius, excl, 3))
                one = {k: v[:1] for k, v in want.items()}
                compare(run(nb, x[:1], nr[:1], radius, nsample, exclude_self=excl), one, GR.FEATURES, excl, (n, nsample, radius, excl, 1))
                worst = [max(a, b) for a, b in zip(worst, r)]
                if excl and nsample == 8:
                    kinds |= {"empty"} if (want["found"] == 0).any() else set()
                    kinds |= {"partly"} if ((want["found"] > 0) & (want["found"] < nsample)).any() else set()
                    kinds |= {"truncated"} if (want["found"] == nsample).any() else set()
    print(f"ball_group n = {n}: worst angle error {worst[0]:.3f} of 2^-20 rad, worst |d| error {worst[1]:.3f} of 3 * 2^-24")
    assert kinds == ({"empty"} if n == 1 else {"empty", "partly"} if n == 2 else {"empty", "partly", "truncated"}), kinds


def test_index_only_form_and_single_channels(nb):
    x, nr = cloud(7, 2, 130)
    for excl in (True, False):
        want = GR.ball_group(x, nr, 0.4, 8, GR.FEATURES, exclude_self=excl)
        compare(run(nb, x, None, 0.4, 8, features=(), exclude_self=excl), want, (), excl, "query")
        for feats in (("xyz",), ("dxyz",), ("ppf",), ("ppf", "xyz"), ("dxyz", "xyz")):
            w = GR.ball_group(x, nr, 0.4, 8, feats, exclude_self=excl)
            compare(run(nb, x, nr if "ppf" in feats else None, 0.4, 8, features=feats, exclude_self=excl), w, feats, excl, feats)


def test_lattice_pairs_at_exactly_the_radius_are_members(nb):
    """Coordinates in multiples of 0.25, radius 0.5: every squared distance is exact, r2 = 0.25 too."""
    g = np.arange(-2, 3) * 0.25
    x = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(1, -1, 3).astype(np.float32)
    x = x[:, np.random.default_rng(3).permutation(x.shape[1])]
    nr = cloud(3, 1, x.shape[1])[1]
    want = GR.ball_group(x, nr, 0.5, 64, GR.FEATURES)
    d2 = GR.dist2(x[0], x[0])
    on_sphere = (d2 == 0.25)
    assert on_sphere.sum() > 0
    for i in range(x.shape[1]):
        assert set(np.flatnonzero(on_sphere[i])) <= set(want["idx"][0, i, :want["found"][0, i]])
    assert (want["found"][0] == ((d2 <= 0.25).sum(1) - 1)).all()
    compare(run(nb, x, nr, 0.5, 64), want, GR.FEATURES, True, "lattice")
    compare(run(nb, x, nr, 0.5, 8, exclude_self=False), GR.ball_group(x, nr, 0.5, 8, GR.FEATURES, exclude_self=False), GR.FEATURES, False,
            "lattice, first-member pad")


def test_duplicates_and_a_nan_point(nb):
    x, nr = cloud(11, 2, 130)
    x[0, 70], x[0, 100], x[0, 129] = x[0, 5], x[0, 5], x[0, 5]  # a duplicate of the query at another index is a member
    x[1, 64, 2] = np.nan                                         # inside the count: a member of no row, its own row all pad
    for excl in (True, False):
        for radius, nsample in ((0.0, 4), (0.5, 8), (4.0, 64)):
            want = GR.ball_group(x, nr, radius, nsample, GR.FEATURES, exclude_self=excl)
            got = run(nb, x, nr, radius, nsample, exclude_self=excl)
            compare(got, want, GR.FEATURES, excl, ("dup / nan", radius, nsample, excl))
            idx, found = got[1].cpu().numpy(), got[2].cpu().numpy()
            assert found[1, 64] == 0 and (idx[1, 64] == 64).all() and not (np.delete(idx[1], 64, 0) == 64).any()
            if radius == 0.0:
                assert list(idx[0, 5, :found[0, 5]]) == ([70, 100, 129] if excl else [5, 70, 100, 129])


def test_query_index_form(nb):
    x, nr = cloud(13, 3, 257)
    q = torch.tensor([[256, 0, 64, 63, 200], [1, 1, 255, 128, 65], [5, 4, 3, 2, 1]])
    for excl in (True, False):
        for radius, nsample in ((0.3, 8), (0.5, 64)):
            want = GR.ball_group(x, nr, radius, nsample, GR.FEATURES, query_idx=q.numpy(), exclude_self=excl)
            assert want["idx"].shape == (3, 5, nsample)
            compare(run(nb, x, nr, radius, nsample, query_idx=q, exclude_self=excl), want, GR.FEATURES, excl, ("query_idx", radius, nsample))
            compare(run(nb, x, nr, radius, nsample, query_idx=q.cuda().int(), exclude_self=excl), want, GR.FEATURES, excl, "device query_idx")


def test_ragged_counts(nb):
    """Zero and one among the counts; rows beyond the counts are zero; sample b equals its own B = 1 call; NaN beyond a count
    changes nothing; device counts are clamped, not validated."""
    B, n = 5, 130
    x, nr = cloud(17, B, n)
    counts, qcounts = [130, 0, 1, 77, 64], [130, 0, 1, 50, 0]
    want = GR.ball_group(x, nr, 0.45, 8, GR.FEATURES, counts=counts, qcounts=qcounts)
    got = run(nb, x, nr, 0.45, 8, counts=counts, qcounts=qcounts)
    compare(got, want, GR.FEATURES, True, "ragged")
    feat, idx, found = (t.cpu().numpy() for t in got)
    for b in range(B):
        assert not idx[b, qcounts[b]:].any() and not found[b, qcounts[b]:].any() and not feat[b, qcounts[b]:].any()
        if counts[b]:
            own = run(nb, x[b:b + 1, :counts[b]], nr[b:b + 1, :counts[b]], 0.45, 8)
            for mine, theirs in zip((feat, idx, found), own):
                assert np.array_equal(bits(mine[b, :qcounts[b]]), bits(theirs.cpu().numpy()[0, :qcounts[b]])), b
    assert found[2, 0] == 0 and (idx[2, 0] == 0).all()  # one point: nothing but itself
    xn, nn = x.copy(), nr.copy()
    for b in range(B):
        xn[b, counts[b]:], nn[b, counts[b]:] = np.nan, np.nan
    dc, dq = torch.tensor(counts, dtype=torch.int32), torch.tensor(qcounts, dtype=torch.int32)
    again = run(nb, xn, nn, 0.45, 8, counts=dc, qcounts=dq)
    for a, b_ in zip(got, again):
        assert torch.equal(a, b_)
    wild = run(nb, xn, nn, 0.45, 8, counts=torch.tensor([1000, -5, 1, 77, 64], dtype=torch.int32),
               qcounts=torch.tensor([999, -1, 1, 50, 0], dtype=torch.int32))  # clamped into [0, n] by the kernel
    for a, b_ in zip(got[1:], wild[1:]):
        assert torch.equal(a[1:], b_[1:])
    # counts without qcounts in the every-point form: a sample has as many queries as points
    w2 = GR.ball_group(x, nr, 0.45, 8, GR.FEATURES, counts=counts)
    compare(run(nb, xn, nn, 0.45, 8, counts=counts), w2, GR.FEATURES, True, "counts only")
    assert not w2["idx"][3, 77:].any() and w2["found"][3, :77].any()


def test_fused_tensor_two_calls_and_a_captured_graph(nb):
    from rrl_hip import callsites
    x, nr = cloud(19, 3, 257)
    tx, tn = torch.from_numpy(x).cuda(), torch.from_numpy(nr).cuda()
    fused = callsites.rpm_raw_features(tx, tn, ("ppf", "xyz", "dxyz"), radius=0.3, nsample=16)
    parts = [nb.ball_group(tx, tn, 0.3, 16, features=(f,))[0] for f in GR.FEATURES]
    assert fused.shape == (3, 257, 16, 10) and fused.is_contiguous() and torch.equal(fused, torch.cat(parts, -1))
    assert torch.equal(parts[0], tx[:, :, None, :].expand(-1, -1, 16, -1))
    first, second = nb.ball_group(tx, tn, 0.3, 16), nb.ball_group(tx, tn, 0.3, 16)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    assert torch.equal(first[0], fused)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        nb.ball_group(tx, tn, 0.3, 16)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = nb.ball_group(tx, tn, 0.3, 16)
    for _ in range(2):
        for o in outs:
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for o, want in zip(outs, first):
            assert torch.equal(o, want)


def test_no_stray_writes(nb):
    """Every output inside a buffer with a sentinel border, through the C entry: the borders are untouched."""
    from rrl_hip import _lib, ops
    B, n, S, ns, C, pad = 2, 65, 65, 7, 10, 64
    x, nr = cloud(23, B, n)
    tx, tn = torch.from_numpy(x).cuda(), torch.from_numpy(nr).cuda()
    bufs = [torch.full((B * S * ns + 2 * pad,), -7, dtype=torch.int32, device="cuda"),
            torch.full((B * S + 2 * pad,), -7, dtype=torch.int32, device="cuda"),
            torch.full((B * S * ns * C + 2 * pad,), -7.0, dtype=torch.float32, device="cuda")]
    inner = [b[pad:-pad] for b in bufs]
    ops._run(tx.device, "rrl_ball_group", ops._p(tx), ops._p(tn), None, None, None, float(GR.r2_of(0.6)), ns, 1, 7, ops._p(inner[0]),
             ops._p(inner[1]), ops._p(inner[2]), B, n, S)
    torch.cuda.synchronize()
    for b in bufs:
        assert (b[:pad] == -7).all() and (b[-pad:] == -7).all()
    feat, idx, found = nb.ball_group(tx, tn, 0.6, ns)
    assert torch.equal(inner[0].view(B, S, ns), idx) and torch.equal(inner[1].view(B, S), found) and torch.equal(inner[2].view(B, S, ns, C), feat)
    assert _lib.GROUP_MAX_SAMPLE == 64


def test_call_site_reproduces_the_reference_run(nb):
    """callsites.rpm_sample_and_group_multi against tests/golden/ball_query_rpm.npz (the reference's float32 run on the CPU):
    indices on rows without a borderline pair, dxyz bit for bit there, the angles and |d| within the bounds."""
    from rrl_hip import callsites
    golden = load_golden("ball_query_rpm.npz")
    name = "sphere_b2_130"
    x, nr = golden[f"{name}_xyz"], golden[f"{name}_normals"]
    tx, tn = torch.from_numpy(x).cuda(), torch.from_numpy(nr).cuda()
    for radius, nsample in ((float(r), int(k)) for r, k in golden[f"{name}_settings"]):
        tag = f"r{int(round(radius * 100)):03d}_k{nsample}"
        out, grouped, fps_idx = callsites.rpm_sample_and_group_multi(tx, tn, radius, nsample, returnfps=True)
        assert set(out) == {"xyz", "dxyz", "ppf"} and torch.equal(out["xyz"], tx)
        assert out["dxyz"].shape == (2, 130, nsample, 3) and out["ppf"].shape == (2, 130, nsample, 4)
        assert torch.equal(fps_idx, torch.arange(130, device="cuda")[None].repeat(2, 1))
        clear = ~GR.ball_group(x, None, radius, nsample)["border"]
        widx = golden[f"{name}_{tag}_idx"].astype(np.int64)
        assert np.array_equal(grouped.cpu().numpy()[clear], x[np.arange(2)[:, None, None], widx][clear])
        assert np.array_equal(bits(out["dxyz"].cpu().numpy()[clear]), bits(golden[f"{name}_{tag}_dxyz"][clear]))
        ang, rel = GR.ppf_errors(out["ppf"].cpu().numpy()[clear], golden[f"{name}_{tag}_ppf"][clear], 0)
        print(f"rpm_sample_and_group_multi {tag}: angles within {ang / GR.ANGLE_TOL:.3f} x 2^-20 of the reference's float32, |d| within "
              f"{rel / GR.NORM_RTOL:.3f} x 3 * 2^-24")
        assert ang <= GR.ANGLE_TOL and rel <= GR.NORM_RTOL
    # the sampled form: npoint > 0 goes through the farthest-point sampler and the query_idx form
    torch.manual_seed(3)
    out, grouped, fps_idx = callsites.rpm_sample_and_group_multi(tx, tn, 0.3, 16, npoint=20, returnfps=True)
    want = GR.ball_group(x, nr, 0.3, 16, ("dxyz", "ppf"), query_idx=fps_idx.cpu().numpy())
    assert fps_idx.shape == (2, 20) and fps_idx.dtype == torch.int64
    assert torch.equal(out["xyz"], torch.gather(tx, 1, fps_idx.unsqueeze(-1).expand(-1, -1, 3)))
    assert np.array_equal(bits(out["dxyz"].cpu().numpy()), bits(want["dxyz"]))
    assert np.array_equal(grouped.cpu().numpy(), x[np.arange(2)[:, None, None], want["idx"]])
