"""The Sinkhorn soft assignment on the GPU (include/rrl.h rrl_sinkhorn_fwd, rrl_sinkhorn_bwd; rrl_hip/sinkhorn.py; DESIGN.md
section 17) against the float64 twin of tests/sinkhorn_refs.py.

Bounds, from the arithmetic rule, none measured.  A matrix term is the exponential of a double argument, evaluated in double
by a degree-9 polynomial after an exact reduction: its Taylor remainder on |r| <= ln 2 / 2 is at most 0.3466^10 / 10! e^0.35 = 1.0e-11 of
the value, the dozen double roundings and those of a sum of at most 1025 terms (2^-43) lie far below: every term, and every
per-lane partial sum, is good to d = 2^-36.  A logsumexp adds such terms under a running maximum whose rescaling factor is one
more such exponential, at most once per round of four terms: at most 8 rounds per lane at these shapes, so the sum is good to
9 d and a potential moves by 9 d plus what the potential under it moved (softmax weights sum to at most 1):
|du^n|, |dv^n| <= 18 n d.  Hence, with e = (36 n + 1) d for an exponential of the final or any intermediate matrix, and 2^-24
for the one rounding of a result to float32 (2^-126 where that underflows):
  log_perm within 36 n d + 2^-24 |log_perm|;  s, c within (e + 2^-24) of themselves + 2^-126;  W within (2 e + 2^-24) max|x| + 2^-126;
  dA[j][k], gx[k] within (2 n + 4) e of the sum of |terms| of that entry (the twin's dA_abs / gx_abs, which carry the
  cancellation inside the adjoint vectors: each of the at most 2 n + 2 stages behind an entry, and the row scalars, adds e of
  it), plus 2^-24 of the entry and 2^-126.
The ceiling no derivation may exceed: per case and per quantity the largest deviation from the twin is at most 2 x that of the
reference's padded formulation evaluated in float32 by torch on the CPU (sinkhorn_refs.padded_torch); for the gradients both
deviations are taken relative to the entry's sum |terms|, floored at 2^-102: below it a float32 result's underflow step, 2^-126,
exceeds its relative rounding, and an entry that both evaluations flush to zero would otherwise set both deviations to 1.  The worst ratios are printed per case (run with -s).
Two calls give the same bits, forward and backward; sample b of a ragged batch has the bits of its own B = 1 call."""
import ctypes

import numpy as np
import pytest
import torch

import sinkhorn_refs as SR
from test_sinkhorn_refs_host import ITERS, SHAPES, SIGMAS, make_inputs

pytestmark = pytest.mark.gpu

U23, U24, TINY = 2.0 ** -23, 2.0 ** -24, 2.0 ** -126
D = 2.0 ** -36
FLOOR = 2.0 ** -102  # below it a float32 result's underflow step (2^-126) exceeds its relative rounding (2^-24)


@pytest.fixture(scope="module")
def sk():
    from rrl_hip import _lib, sinkhorn
    _lib.load()
    assert torch.cuda.is_available()
    return sinkhorn


def cuda(*xs):
    return tuple(torch.from_numpy(np.ascontiguousarray(x)).cuda() if x is not None else None for x in xs)


def run(sk, A, x, g, n, slack, counts_src=None, counts_ref=None):
    """forward + backward on the GPU -> dict of float64 numpy arrays (and the raw float32 tensors under 'raw')."""
    ta, tx = (t.requires_grad_(True) for t in cuda(A, x))
    W, s, c, info, lp = sk.soft_assign(ta, tx, n_iters=n, slack=slack, counts_src=counts_src, counts_ref=counts_ref,
                                       with_info=True, return_log_perm=True)
    assert not lp.requires_grad and not info.requires_grad
    gW, gs, gc = cuda(*g)
    ((W * gW).sum() + (s * gs).sum() + (c * gc).sum()).backward()
    raw = (W.detach(), s.detach(), c.detach(), lp, ta.grad, tx.grad)
    out = {k: v.double().cpu().numpy() for k, v in zip(("W", "s", "c", "log_perm", "dA", "gx"), raw)}
    out["info"], out["raw"] = info.cpu().numpy(), raw
    return out


def check_case(sk, seed, B, J, K, n, slack, sigma):
    """One case against the twin: the derived bounds and the ceiling; returns the worst ratio to the float32 yardstick."""
    A, x, g = make_inputs(seed, B, J, K, sigma, n)
    f = SR.forward(A, x, n, slack)
    bw = SR.backward(A, x, *g, n, slack, fwd=f)
    r32 = dict(zip(("log_perm", "W", "s", "c", "dA", "gx"), SR.padded_torch_grads(A, x, *g, n, slack, dtype=torch.float32)))
    got = run(sk, A, x, g, n, slack)
    what = (B, J, K, n, slack, sigma)
    assert not got["info"].any(), what
    e = (36 * n + 1) * D
    xmax = np.abs(x.astype(np.float64)).max()
    bounds = {"log_perm": 36 * n * D + U24 * np.abs(f["log_perm"]), "s": (e + U24) * f["s"] + TINY, "c": (e + U24) * f["c"] + TINY,
              "W": (2 * e + U24) * xmax + TINY}
    worst = 0.0
    for key, lim in bounds.items():
        dev, ref = np.abs(got[key] - f[key]), np.abs(r32[key] - f[key])
        print(f"sinkhorn {what} {key}: deviation {dev.max():.3e}, float32 torch {ref.max():.3e}, bound (at the worst entry) "
              f"{np.max(lim * np.ones_like(dev)):.3e}")
        assert (dev <= lim).all(), (what, key, dev.max())
        assert dev.max() <= 2 * ref.max(), (what, key, dev.max(), ref.max())
        worst = max(worst, dev.max() / ref.max() if ref.max() > 0 else 0.0)
    for key, mag in (("dA", bw["dA_abs"]), ("gx", bw["gx_abs"])):
        lim = (2 * n + 4) * e * mag + U24 * np.abs(bw[key]) + TINY
        dev, ref = np.abs(got[key] - bw[key]), np.abs(r32[key] - bw[key])
        assert (dev <= lim).all(), (what, key, (dev / lim).max())
        scale = np.maximum(mag, FLOOR)
        rel, rel32 = (dev / scale).max(), (ref / scale).max()
        print(f"sinkhorn {what} {key}: deviation / sum|terms| {rel:.3e}, float32 torch {rel32:.3e}")
        assert rel <= 2 * rel32, (what, key, rel, rel32)
        worst = max(worst, rel / rel32 if rel32 > 0 else 0.0)
    return worst


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("J,K", SHAPES)
def test_against_the_twin(sk, J, K, B):
    worst = 0.0
    for slack in (True, False):
        for n in ITERS:
            for sigma in SIGMAS:
                worst = max(worst, check_case(sk, 1000 * J + 10 * K + B + n, B, J, K, n, slack, sigma))
    print(f"sinkhorn ({B}, {J}, {K}): worst ratio to the float32 yardstick {worst:.3f}")


def test_the_largest_case(sk):
    w1 = check_case(sk, 5, 1, 1025, 1025, 5, True, 30.0)
    w2 = check_case(sk, 6, 1, 1025, 1025, 1, False, 3.0)
    print(f"sinkhorn (1, 1025, 1025): worst ratio to the float32 yardstick {max(w1, w2):.3f}")


def test_fixture_cases_through_rpm_match_head(sk):
    """callsites.rpm_match_head against the reference's own run (tests/golden/sinkhorn_rpm.npz): the transform within the
    bounds of tests/test_gpu_kabsch.py (R within 2^-23, T within 2^-23 max(1, |abar| + |bbar|)) wherever the recorded Kabsch gap
    is >= 1e-3 (every case with a rotation to determine: all but the single-point one); W, s, c within this file's bounds."""
    import kabsch_refs as KR
    from conftest import load_golden
    from rrl_hip import callsites
    g = load_golden("sinkhorn_rpm.npz")
    checked = 0
    for name in [str(c) for c in g["cases"]]:
        A, src, xr = (g[f"{name}_{k}"] for k in ("log_alpha", "xyz_src", "xyz_ref"))
        slack, n = (int(v) for v in g[f"{name}_spec"])
        ta, ts, tx = cuda(A, src, xr)
        ta.requires_grad_(True)
        tx.requires_grad_(True)
        tr, W, s, c = callsites.rpm_match_head(ta, ts, tx, n_iters=n, slack=bool(slack))
        CW, Cs, Cc = cuda(g[f"{name}_CW"], g[f"{name}_Cs"], g[f"{name}_Cc"])
        ga, gx = torch.autograd.grad((W * CW).sum() + (s * Cs).sum() + (c * Cc).sum(), (ta, tx))
        e = (36 * n + 1) * D
        for got, key, lim in ((s, "s", (e + U24) * g[f"{name}_s"]), (c, "c", (e + U24) * g[f"{name}_c"]),
                              (W, "W", (2 * e + U24) * np.abs(xr).max() + TINY)):
            assert (np.abs(got.detach().double().cpu().numpy() - g[f"{name}_{key}"]) <= lim).all(), (name, key)
        bw = SR.backward(A, xr, g[f"{name}_CW"], g[f"{name}_Cs"], g[f"{name}_Cc"], n, bool(slack))
        for got, key, mag in ((ga, "gA", bw["dA_abs"]), (gx, "gx", bw["gx_abs"])):
            want = g[f"{name}_{key}"]
            assert (np.abs(got.double().cpu().numpy() - want) <= (2 * n + 4) * e * mag + U24 * np.abs(want) + TINY).all(), (name, key)
        for b in range(A.shape[0]):
            if g[f"{name}_gap"][b] < 1e-3:
                continue
            twin = KR.fit(src[b], g[f"{name}_W"][b].astype(np.float32), g[f"{name}_s"][b].astype(np.float32), eps=1e-5)
            lim = U23 * max(1.0, np.abs(twin["abar"]).max() + np.abs(twin["bbar"]).max())
            got, want = tr[b].detach().cpu().numpy().astype(np.float64), g[f"{name}_transform"][b]
            print(f"sinkhorn fixture {name}[{b}]: R off by {np.abs(got[:, :3] - want[:, :3]).max() / U23:.2f} x 2^-23, "
                  f"T by {np.abs(got[:, 3] - want[:, 3]).max() / lim:.2f} x its bound")
            assert np.abs(got[:, :3] - want[:, :3]).max() <= U23 and np.abs(got[:, 3] - want[:, 3]).max() <= lim, (name, b)
            checked += 1
    assert checked == 6  # 2 + 1 + 2 + 1 samples; the single-point case has no rotation


@pytest.mark.parametrize("slack", [True, False])
def test_ragged_samples_equal_their_own_calls_bit_for_bit(sk, slack):
    J, K, n = 257, 130, 5
    cs, cr = [0, 1, J // 2, J], [K, K // 2, K, 1]
    A, x, g = make_inputs(11, 4, J, K, 30.0, n)
    filled = [a.copy() for a in (A, x, *g)]
    for b in range(4):  # NaN beyond the counts: never read (an upstream gradient there multiplies nothing)
        A[b, cs[b]:, :] = np.nan
        A[b, :, cr[b]:] = np.nan
        x[b, cr[b]:] = np.nan
    got = run(sk, A, x, g, n, slack, cs, cr)
    again = run(sk, A, x, g, n, slack, torch.tensor(cs, dtype=torch.int32).cuda(), torch.tensor(cr, dtype=torch.int32).cuda())
    assert not got["info"].any()
    for a, b_ in zip(got["raw"], again["raw"]):
        assert torch.equal(a, b_)
    W, s, c, lp, dA, gx = got["raw"]
    for b in range(4):
        j, k = cs[b], cr[b]
        assert not s[b, j:].any() and not W[b, j:].any() and not c[b, k:].any() and not gx[b, k:].any()
        assert not dA[b, j:, :].any() and not dA[b, :, k:].any()
        assert torch.isinf(lp[b, j:, :]).all() and torch.isinf(lp[b, :, k:]).all()
        if j == 0:
            assert not c[b].any() and not gx[b].any()
            continue
        one = run(sk, filled[0][b:b + 1, :j, :k], filled[1][b:b + 1, :k], [filled[2][b:b + 1, :j], filled[3][b:b + 1, :j], filled[4][b:b + 1, :k]],
                  n, slack)
        W1, s1, c1, lp1, dA1, gx1 = one["raw"]
        assert torch.equal(W[b, :j], W1[0]) and torch.equal(s[b, :j], s1[0]) and torch.equal(c[b, :k], c1[0]), b
        assert torch.equal(lp[b, :j, :k], lp1[0]) and torch.equal(dA[b, :j, :k], dA1[0]) and torch.equal(gx[b, :k], gx1[0]), b


def test_minus_infinity_entries_with_slack(sk):
    A, x, g = make_inputs(12, 2, 65, 63, 3.0, 5)
    A[0, 2, :] = -np.inf
    A[0, 5, 7] = A[1, 64, 62] = A[1, 0, 0] = -np.inf
    hole = np.isinf(A)
    got = run(sk, A, x, g, 5, True)
    f = SR.forward(A, x, 5, True)
    assert not got["info"].any()
    assert np.isinf(got["log_perm"][hole]).all() and not got["dA"][hole].any()
    assert got["s"][0, 2] == 0.0 and not got["W"][0, 2].any()
    for key in ("W", "s", "c", "dA", "gx"):
        assert np.isfinite(got[key]).all(), key
    e = 181 * D
    assert (np.abs(got["s"] - f["s"]) <= (e + U24) * f["s"]).all() and (np.abs(got["c"] - f["c"]) <= (e + U24) * f["c"]).all()


def test_a_nan_inside_the_counts_sets_the_flag(sk):
    for n in (0, 5):
        A, x, g = make_inputs(13, 3, 70, 130, 3.0, n)
        A[1, 40, 100] = np.nan
        A[2, 69, 129] = np.inf
        got = run(sk, A, x, g, n, True, [70, 70, 70], [130, 130, 129])
        assert got["info"].tolist() == [0, 1, 0], n  # (sample 2's +inf lies beyond its count)
        got = run(sk, A, x, g, n, True)
        assert got["info"].tolist() == [0, 1, 1], n


def test_two_calls_and_a_captured_graph_give_the_same_bits(sk):
    A, x, g = make_inputs(14, 3, 257, 130, 30.0, 5)
    first, second = run(sk, A, x, g, 5, True), run(sk, A, x, g, 5, True)
    for a, b in zip(first["raw"], second["raw"]):
        assert torch.equal(a, b)
    ta, tx = (t.requires_grad_(True) for t in cuda(A, x))
    gW, gs, gc = cuda(*g)

    def step():
        W, s, c = sk.soft_assign(ta, tx, n_iters=5, slack=True)
        return (W, s, c) + torch.autograd.grad((W * gW).sum() + (s * gs).sum() + (c * gc).sum(), (ta, tx))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for _ in range(2):
        for o in outs:
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for o, want in zip(outs, (first["raw"][i] for i in (0, 1, 2, 4, 5))):
            assert torch.equal(o, want)


def test_no_stray_writes(sk):
    """Every output inside a buffer with a sentinel border, through the C entries: the borders are untouched."""
    from rrl_hip import _lib, ops
    B, J, K, n, pad = 2, 65, 63, 5, 64
    A, x, g = make_inputs(15, B, J, K, 3.0, n)
    ta, tx, gW, gs, gc = cuda(A, x, *g)
    dev = ta.device
    lib = _lib.load()

    def bordered(numel, dtype=torch.float32, fill=-7.0):
        return torch.full((numel + 2 * pad,), fill, dtype=dtype, device=dev)
    wsn = int(lib.rrl_sinkhorn_workspace_bytes(B, J, K, n)) // 8
    bufs = dict(ws=bordered(wsn, torch.float64), W=bordered(B * J * 3), s=bordered(B * J), c=bordered(B * K), log_perm=bordered(B * J * K),
                info=bordered(B, torch.int32, -7), gA=bordered(B * J * K), gx=bordered(B * K * 3))
    P = lambda t: ctypes.c_void_p(t.data_ptr() + pad * t.element_size())  # noqa: E731
    k = _lib.SinkhornArgs()
    k.struct_bytes = ctypes.sizeof(k)
    k.B, k.J, k.K, k.n_iters, k.slack = B, J, K, n, 1
    k.log_alpha, k.xyz_ref, k.eps = ops._p(ta), ops._p(tx), 1e-5
    k.ws, k.ws_bytes = P(bufs["ws"]), wsn * 8
    k.W, k.s, k.c, k.log_perm, k.info = (P(bufs[q]) for q in ("W", "s", "c", "log_perm", "info"))
    ops._run(dev, "rrl_sinkhorn_fwd", ctypes.byref(k))
    ops._run(dev, "rrl_sinkhorn_bwd", ctypes.byref(k), ops._p(gW), ops._p(gs), ops._p(gc), P(bufs["gA"]), P(bufs["gx"]))
    torch.cuda.synchronize()
    for name, t in bufs.items():
        assert (t[:pad] == -7).all() and (t[-pad:] == -7).all(), name
    want = run(sk, A, x, g, n, True)["raw"]
    for name, w in zip(("W", "s", "c", "log_perm", "gA", "gx"), want):
        assert torch.equal(bufs[name][pad:-pad], w.reshape(-1)), name
