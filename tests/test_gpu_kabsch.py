"""The closed-form rigid fit on the GPU (include/rrl.h rrl_kabsch_fwd, rrl_kabsch_bwd; rrl_hip/kabsch.py)
against the float64 twins of tests/kabsch_refs.py.

Bounds, from the arithmetic rule (fixed-order double sums of float32 inputs, double SVD, one rounding to float32), none
measured: the moments W, abar, bbar, S within (n + 2) 2^-52 sum|terms| of the twin; wherever the twin's gap
(s1 + delta s2) / s0 >= 1e-3, every entry of R within 2^-23 and T within 2^-23 max(1, |abar|_inf + |bbar|_inf); under the same
condition every entry of ga, gb, gw within 2^-22 of the sample's largest |entry| of the twin's float64 autograd.  Two calls
give the same bits."""
import ctypes

import numpy as np
import pytest
import torch

import kabsch_refs as KR
from test_kabsch_refs_host import E_ARG, E_WS, FAKE, KABSCH_REFUSALS, kabsch_args

pytestmark = pytest.mark.gpu

U23, U22, U52 = 2.0 ** -23, 2.0 ** -22, 2.0 ** -52
SIZES = [1, 2, 3, 63, 64, 65, 257, 1023, 4097]
GAP_MIN = 1e-3


@pytest.fixture(scope="module")
def kb():
    from rrl_hip import _lib, kabsch
    _lib.load()
    assert torch.cuda.is_available()
    return kabsch


def rot(rs, deg):
    ax = rs.standard_normal(3)
    ax /= np.linalg.norm(ax)
    a = np.deg2rad(deg)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


def rigid_pairs(seed, B, n, stride=3, noise=0.02, offset=0.0, mirror=False, counts=None):
    """a, b (B, n, stride) float32: b = a R + t + noise per sample (row convention), unit extent about `offset`; columns
    3.. (pseudo-triangle neighbours) random; rows beyond a count NaN; w (B, n) in (0.1, 1)."""
    rs = np.random.default_rng(seed)
    a = np.full((B, n, stride), np.nan, np.float32)
    b = np.full((B, n, stride), np.nan, np.float32)
    for s in range(B):
        c = n if counts is None else counts[s]
        p = rs.uniform(-0.5, 0.5, (c, 3)) + offset
        q = (p - offset) @ rot(rs, rs.uniform(5, 170)) + offset + rs.uniform(-0.3, 0.3, 3) + noise * rs.standard_normal((c, 3))
        if mirror:
            q[:, 2] = 2 * offset - q[:, 2]
        a[s, :c, :3], b[s, :c, :3] = p, q
        a[s, :c, 3:], b[s, :c, 3:] = rs.standard_normal((c, stride - 3)), rs.standard_normal((c, stride - 3))
    w = rs.uniform(0.1, 1.0, (B, n)).astype(np.float32)
    return a, b, w


def cuda(*xs):
    return tuple(torch.from_numpy(np.ascontiguousarray(x)).cuda() if x is not None else None for x in xs)


def check_fit(got, twin, n, what):
    """One sample's outputs (R, T, info, fit as numpy) against the twin's dict, with the bounds of the file header."""
    R, T, info, fit = got
    assert info.tolist() == twin["info"], (what, info.tolist(), twin["info"])
    k = twin["info"][0]
    if twin["info"][1] == KR.FIT_FEW:
        assert np.array_equal(R, np.eye(3, dtype=np.float32)) and not T.any() and not fit[1:].any(), what
        assert abs(fit[0] - twin["W"]) <= (n + 2) * U52 * abs(twin["W"]), what
        return
    t, c = twin["terms"], (k + 2) * U52
    assert abs(fit[0] - twin["W"]) <= c * t["W"], (what, "W")
    assert (np.abs(fit[1:4] - twin["abar"]) <= c * t["abar"]).all(), (what, "abar", fit[1:4] - twin["abar"], c * t["abar"])
    assert (np.abs(fit[4:7] - twin["bbar"]) <= c * t["bbar"]).all(), (what, "bbar")
    assert (np.abs(fit[16:19] - twin["S"]) <= c * np.linalg.norm(t["H"])).all(), (what, "S", fit[16:19] - twin["S"], c * np.linalg.norm(t["H"]))
    assert fit[28] == twin["delta"] or twin["gap"] < GAP_MIN * twin["S"][0], (what, "delta")
    assert abs(fit[29] - twin["res_after"]) <= c * t["res"], (what, "res_after", fit[29], twin["res_after"])
    assert abs(fit[30] - twin["key_mean"]) <= c * t["key"], (what, "key_mean")
    U, V = fit[7:16].reshape(3, 3), fit[19:28].reshape(3, 3)
    for M in (U, V, R.astype(np.float64)):
        assert np.abs(M.T @ M - np.eye(3)).max() <= 4 * U23, (what, "orthonormal")
    assert np.abs(U @ np.diag(fit[16:19]) @ V.T - twin["H"]).max() <= 2 * c * np.linalg.norm(t["H"]), (what, "U S V^T")  # (the moments' bound, once more for the decomposition)
    if twin["gap"] >= GAP_MIN * twin["S"][0]:
        assert np.abs(R - twin["R"]).max() <= U23, (what, "R", np.abs(R - twin["R"]).max() / U23)
        lim = U23 * max(1.0, np.abs(twin["abar"]).max() + np.abs(twin["bbar"]).max())
        assert np.abs(T - twin["T"]).max() <= lim, (what, "T", np.abs(T - twin["T"]).max() / lim)


def counts_for(B, n):
    return None if B == 1 else [0, n, max(n // 2, min(n, 3))][:B]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", SIZES)
def test_fit_against_the_twin(kb, n, B):
    """Random rigid pairs with noise and weights; strides 3 and 9, both values of transpose_r, counts 0 / full / half with NaN
    beyond them; n < 3 gives status 1 with (I, 0).  The second call repeats the first bit for bit."""
    stride, tr, eps = (9 if n % 2 else 3), bool((n + B) % 2), (1e-5 if n % 3 == 0 else 0.0)
    counts = counts_for(B, n)
    a, b, w = rigid_pairs(1000 + n + B, B, n, stride, counts=counts)
    ta, tb, tw = cuda(a, b, w)
    outs = [kb.kabsch(ta, tb, tw, counts=counts, eps=eps, transpose_r=tr, with_info=True) for _ in range(2)]
    torch.cuda.synchronize()
    for x, y in zip(*outs):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    R, T, info, fit = (x.cpu().numpy() for x in outs[0])
    for s in range(B):
        twin = KR.fit(a[s], b[s], w[s], None, None if counts is None else counts[s], None if counts is None else counts[s],
                      eps=eps, transpose_r=tr)
        check_fit((R[s], T[s], info[s], fit[s]), twin, n, (n, B, s))
        if n >= 3 and (counts is None or counts[s] >= 3):
            assert info[s, 1] == KR.FIT_OK and info[s, 0] == (n if counts is None else counts[s])


SPECIAL = {
    "mirrored-257": dict(n=257, mirror=True),
    "mirrored-4097-offset": dict(n=4097, mirror=True, offset=1000.0),
    "offset1000-257": dict(n=257, offset=1000.0),
    "offset1000-1023-stride9": dict(n=1023, offset=1000.0, stride=9),
    "offset1000-4097": dict(n=4097, offset=1000.0),
}


@pytest.mark.parametrize("name", list(SPECIAL))
def test_reflections_and_clouds_far_from_the_origin(kb, name):
    """A mirrored b: delta = -1, the reflection is fixed and reported, R is still a rotation and the twin's.  Unit clouds 1000
    from the origin: the case a float32 accumulator (or a float32 centroid) fails -- R and T keep their bounds."""
    spec = dict(SPECIAL[name])
    n, mirror = spec.pop("n"), spec.get("mirror", False)
    a, b, w = rigid_pairs(77, 3, n, **spec)
    ta, tb, tw = cuda(a, b, w)
    R, T, info, fit = (x.cpu().numpy() for x in kb.kabsch(ta, tb, tw, with_info=True))
    for s in range(3):
        twin = KR.fit(a[s], b[s], w[s])
        assert twin["gap"] >= GAP_MIN * twin["S"][0] and twin["delta"] == (-1.0 if mirror else 1.0)
        check_fit((R[s], T[s], info[s], fit[s]), twin, n, (name, s))
        assert info[s, 2] == int(mirror) and abs(np.linalg.det(R[s].astype(np.float64)) - 1.0) <= 8 * U23


def test_degenerate_inputs_have_their_status(kb):
    """Collinear points: status 2, R and T still written (a rotation that maps the line), zero gradient.  All-zero weights and
    n < 3: status 1, (I, 0), zero gradient.  The third sample is regular and keeps its gradient."""
    rs = np.random.default_rng(9)
    n = 65
    a, b, w = rigid_pairs(10, 3, n)
    tline = np.linspace(-1, 1, n)[:, None]
    a[0] = (tline * np.array([[1.0, 2.0, -0.5]]) + 0.3).astype(np.float32)
    b[0] = (a[0].astype(np.float64) @ rot(rs, 40.0) + 0.1).astype(np.float32)
    w[1] = 0.0
    ta, tb, tw = cuda(a, b, w)
    ta.requires_grad_(True); tb.requires_grad_(True); tw.requires_grad_(True)
    R, T, info, fit = kb.kabsch(ta, tb, tw, with_info=True)
    (R.sum() + (T * T).sum()).backward()
    info, Rn, Tn = info.cpu().numpy(), R.detach().cpu().numpy().astype(np.float64), T.detach().cpu().numpy().astype(np.float64)
    assert info[:, 1].tolist() == [KR.FIT_DEGENERATE, KR.FIT_FEW, KR.FIT_OK] and info[:, 0].tolist() == [n, n, n]
    assert np.abs(Rn[0].T @ Rn[0] - np.eye(3)).max() <= 4 * U23 and abs(np.linalg.det(Rn[0]) - 1.0) <= 8 * U23
    assert np.abs(a[0].astype(np.float64) @ Rn[0] + Tn[0] - b[0]).max() <= 1e-5  # the line is mapped onto its image
    assert np.array_equal(Rn[1], np.eye(3)) and not Tn[1].any()
    for g in (ta.grad, tb.grad, tw.grad):
        assert not g[:2].any() and torch.isfinite(g).all() and g[2].abs().max() > 0
    R2, T2, info2, _ = kb.kabsch(ta[:, :2].detach(), tb[:, :2].detach(), with_info=True)
    assert info2[:, 1].tolist() == [KR.FIT_FEW] * 3 and torch.equal(R2.cpu(), torch.eye(3).expand(3, 3, 3)) and not T2.any()


def make_keys(rs, B, n, m):
    idx = rs.integers(0, m, (B, n)).astype(np.uint64)
    dist = rs.uniform(0.0, 1.0, (B, n)).astype(np.float32)
    return (dist.view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx, dist


def test_keys_counts_gate_and_filler(kb):
    """Partners through keys: all-ones rows, indices >= m and >= count_b and rows >= count_a are skipped and counted; a gate
    removes the pairs whose distance word exceeds it; NaN filler beyond the counts (and at the skipped targets) is invisible."""
    rs = np.random.default_rng(21)
    B, n, m = 3, 300, 260
    ca, cb = [300, 150, 0], [260, 100, 260]
    a = np.full((B, n, 3), np.nan, np.float32)
    b = np.full((B, m, 9), np.nan, np.float32)
    for s in range(B):
        a[s, :ca[s]] = rs.uniform(-1, 1, (ca[s], 3))
        b[s, :cb[s], :3] = rs.uniform(-1, 1, (cb[s], 3)) + 0.2
    w = rs.uniform(0.1, 1.0, (B, n)).astype(np.float32)
    keys, dist = make_keys(rs, B, n, m)
    keys[:, 5::17] = np.uint64(KR.ALL_ONES)
    keys[:, 3::29] = (keys[:, 3::29] & ~np.uint64(0xFFFFFFFF)) | np.uint64(m + 5)
    keys[:, 7::31] = (keys[:, 7::31] & ~np.uint64(0xFFFFFFFF)) | np.uint64(0xFFFFFFFE)
    gate = np.array([0.5, 0.25, 0.5], np.float32)
    ta, tb, tw = cuda(a, b, w)
    tk = torch.from_numpy(keys.view(np.int64)).cuda()
    for gated in (False, True):
        R, T, info, fit = (x.cpu().numpy() for x in kb.kabsch_from_keys(
            ta, tk, tb, w=tw, counts_a=ca, counts_b=cb, max_sqdist=torch.from_numpy(gate) if gated else None))
        for s in range(B):
            twin = KR.fit(a[s], b[s], w[s], keys[s], ca[s], cb[s], gate[s] if gated else None)
            check_fit((R[s], T[s], info[s], fit[s]), twin, n, ("keys", gated, s))
        assert info[2].tolist() == [0, KR.FIT_FEW, 0, n] and info[0, 3] > 0 and info[1, 3] > info[0, 3]
        if gated:
            live = [i for i in range(n) if keys[0, i] != KR.ALL_ONES and int(keys[0, i]) & 0xFFFFFFFF < m]
            assert info[0, 0] == sum(1 for i in live if dist[0, i] <= gate[0]) < len(live)
    # unit weights, no counts: the uniform walk's own keys (every partner in range) give key_mean = the mean distance word
    full_a, full_b = np.nan_to_num(a, nan=0.5), np.nan_to_num(b, nan=0.25)
    keys2, dist2 = make_keys(rs, B, n, m)
    R, T, info, fit = kb.kabsch_from_keys(*cuda(full_a), torch.from_numpy(keys2.view(np.int64)).cuda(), *cuda(full_b))
    assert info[:, 0].tolist() == [n] * B and not info[:, 3].any()
    assert np.abs(fit[:, 30].cpu().numpy() - dist2.astype(np.float64).mean(1)).max() <= (n + 2) * U52


BWD_CASES = [(3, 3), (63, 9), (65, 3), (257, 9), (1023, 3), (4097, 3)]


@pytest.mark.parametrize("n,stride", BWD_CASES)
def test_backward_against_float64_autograd(kb, n, stride):
    """ga, gb, gw of <gR, R> + <gT, T> per sample against the twin's float64 autograd on the sample's own rows: each entry
    within 2^-22 of the sample's largest |entry|; rows beyond a count (and a (B, n, 9) input's other columns) get zeros; the
    second backward repeats the first bit for bit.  Sample 0 has eps and R^T, sample-wide flags alternate with n."""
    B = 3
    tr, eps = bool(n % 2), (1e-5 if stride == 9 else 0.0)
    counts = [n, max(n // 2, 3), 0] if n > 3 else [3, 3, 0]
    offset = 1000.0 if n == 1023 else 0.0
    a, b, w = rigid_pairs(500 + n, B, n, stride, noise=0.05, offset=offset, counts=counts)
    rs = np.random.default_rng(n)
    gR, gT = rs.standard_normal((B, 3, 3)).astype(np.float32), rs.standard_normal((B, 3)).astype(np.float32)
    grads = []
    for _ in range(2):
        ta, tb, tw = cuda(a, b, w)
        ta.requires_grad_(True); tb.requires_grad_(True); tw.requires_grad_(True)
        R, T, info, fit = kb.kabsch(ta, tb, tw, counts=counts, eps=eps, transpose_r=tr, with_info=True)
        ((R * torch.from_numpy(gR).cuda()).sum() + (T * torch.from_numpy(gT).cuda()).sum()).backward()
        grads.append([g.cpu().numpy() for g in (ta.grad, tb.grad, tw.grad)])
    for x, y in zip(*grads):
        assert np.array_equal(x.view(np.int32), y.view(np.int32))
    ga, gb, gw = grads[0]
    assert ga.shape == a.shape and gb.shape == b.shape and not ga[:, :, 3:].any() and not gb[:, :, 3:].any()
    for s in range(B):
        c = counts[s]
        assert not ga[s, c:].any() and not gb[s, c:].any() and not gw[s, c:].any()
        if c == 0:
            continue
        twin = KR.fit(a[s, :c], b[s, :c], w[s, :c], eps=eps)
        assert twin["gap"] >= GAP_MIN * twin["S"][0]
        wa, wb, ww = KR.grads_torch(a[s:s + 1, :c, :3], b[s:s + 1, :c, :3], w[s:s + 1, :c], gR[s:s + 1], gT[s:s + 1], eps, tr)
        for got, want, what in ((ga[s, :c, :3], wa[0], "ga"), (gb[s, :c, :3], wb[0], "gb"), (gw[s, :c], ww[0], "gw")):
            lim = U22 * np.abs(want).max()
            assert np.abs(got - want).max() <= lim, (n, s, what, np.abs(got - want).max() / lim)


def test_trainer_heads_match_the_reference_recording(kb):
    """callsites.rpm_compute_rigid_transform against the reference's own output and gradients (tests/golden/kabsch_rpm.npz),
    and callsites.dcp_svd_head_pose against the restated head: the forward bounds of this file; the gradients within 2^-22 of
    the sample's largest entry."""
    from conftest import load_golden
    from rrl_hip import callsites
    g = load_golden("kabsch_rpm.npz")
    for name in [str(c) for c in g["cases"]]:
        a, b, w, C = (g[f"{name}_{k}"] for k in ("a", "b", "w", "C"))
        ta, tb, tw = (torch.tensor(x, dtype=torch.float32, device="cuda", requires_grad=True) for x in (a, b, w))
        out = callsites.rpm_compute_rigid_transform(ta, tb, tw)
        (out * torch.tensor(C, dtype=torch.float32, device="cuda")).sum().backward()
        got, want = out.detach().cpu().numpy(), g[f"{name}_transform"]
        for s in range(a.shape[0]):
            twin = KR.fit(a[s].astype(np.float32), b[s].astype(np.float32), w[s].astype(np.float32), eps=1e-5)
            lim = U23 * max(1.0, np.abs(twin["abar"]).max() + np.abs(twin["bbar"]).max())
            assert twin["gap"] >= GAP_MIN * twin["S"][0]
            assert np.abs(got[s, :, :3] - want[s, :, :3]).max() <= U23 and np.abs(got[s, :, 3] - want[s, :, 3]).max() <= lim, name
        C32 = C.astype(np.float32).astype(np.float64)  # the upstream gradient as the node received it
        for s in range(a.shape[0]):
            wa, wb, ww = KR.grads_torch(a[s:s + 1], b[s:s + 1], w[s:s + 1], C32[s:s + 1, :, :3], C32[s:s + 1, :, 3], 1e-5, True)
            for t, want_g in ((ta, wa), (tb, wb), (tw, ww)):
                assert np.abs(t.grad[s].cpu().numpy() - want_g[0]).max() <= U22 * np.abs(want_g).max(), name
        Rd, td = callsites.dcp_svd_head_pose(ta.detach().transpose(2, 1).contiguous(), tb.detach().transpose(2, 1).contiguous())
        Rw, tw_ = KR.dcp_head(torch.tensor(a).transpose(1, 2), torch.tensor(b).transpose(1, 2))
        lim = U23 * max(1.0, np.abs(a.mean(1)).max() + np.abs(b.mean(1)).max())
        assert np.abs(Rd.cpu().numpy() - Rw.numpy()).max() <= U23 and np.abs(td.cpu().numpy() - tw_.numpy()).max() <= lim


def test_c_refusals_leave_the_outputs_untouched(kb):
    """Every refusal returns its code before a launch: real buffers, prefilled, keep their bits."""
    from rrl_hip import _lib, ops
    lib = _lib.load()
    B, n = 2, 1000
    a, b = torch.randn(B, n, 3, device="cuda"), torch.randn(B, n, 3, device="cuda")
    R, T = torch.full((B, 9), 7.0, device="cuda"), torch.full((B, 3), 7.0, device="cuda")
    fit = torch.full((B, 32), 7.0, dtype=torch.float64, device="cuda")
    info = torch.full((B, 4), 7, dtype=torch.int32, device="cuda")
    part = torch.empty(int(lib.rrl_kabsch_part_bytes(B, n)) // 8, dtype=torch.float64, device="cuda")
    real = dict(a=a.data_ptr(), b=b.data_ptr(), R=R.data_ptr(), T=T.data_ptr(), fit=fit.data_ptr(), info=info.data_ptr(), part=part.data_ptr())
    stream = ops._stream(a.device)
    def realise(k, v):  # the host test's overrides on real buffers: NULL stays NULL, a misaligned fake becomes a misaligned real
        if v is None or k in ("B", "n", "m", "a_stride", "b_stride", "struct_bytes"):
            return v
        return a.data_ptr() if k == "gate_sq" else real[k] + (v - FAKE)
    for over in KABSCH_REFUSALS:
        fix = {k: realise(k, v) for k, v in over.items()}
        assert lib.rrl_kabsch_fwd(ctypes.byref(kabsch_args(lib, **{**real, **fix})), stream) == E_ARG, over
    assert lib.rrl_kabsch_fwd(ctypes.byref(kabsch_args(lib, **real, part_bytes=part.numel() * 8 - 1)), stream) == E_WS
    torch.cuda.synchronize()
    assert (R == 7).all() and (T == 7).all() and (fit == 7).all() and (info == 7).all()
    assert lib.rrl_kabsch_fwd(ctypes.byref(kabsch_args(lib, **real)), stream) == 0
    torch.cuda.synchronize()
    assert info[:, 1].tolist() == [0, 0] and info[:, 0].tolist() == [n, n]
