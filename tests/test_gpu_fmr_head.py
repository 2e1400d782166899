"""FMR's inverse-compositional head on the GPU (include/rrl.h rrl_ic_*; rrl_hip/fmr.py) against the host
twin of tests/fmr_refs.py.

Bounds, from the arithmetic rule, none measured (fmr_refs.bound):
    |device - twin| <= 2^-24 |value| + (n + 64) 2^-53 (1 + kappa) sum|terms|
n the number of terms of the value's double sum (K for the sums over the features, N for the perturbation's, the small algebra's
operations are the 64), sum|terms| the twin's sum with every term replaced by its magnitude, kappa = cond_2(H) for pinv and
3 cond_2(H) for its gradients (H^-1 enters S twice and dJ once), 0 elsewhere.  No float32-sized slack beyond the one final
rounding: g_new and the update's backward are compared on the device's own dx (the rule says "on the dx the forward kept").
perturb's forward is bit for bit the twin's float32 chain.  The worst ratio to each bound is printed per test (pytest -s)."""
import numpy as np
import pytest
import torch

import fmr_refs as FR
from conftest import load_golden

pytestmark = pytest.mark.gpu

KS = [1, 5, 6, 7, 63, 64, 65, 256, 1024, 1025, 4096, 16384]
MIXED_DT = [1e-3, 0.5, 2e-2, 0.3, 1e-3, 5e-2]


@pytest.fixture(scope="module")
def fm():
    from rrl_hip import _lib, fmr
    _lib.load()
    assert torch.cuda.is_available()
    return fmr


def cuda(*xs):
    return tuple(torch.from_numpy(np.ascontiguousarray(x)).cuda() if x is not None else None for x in xs)


def bits(t):
    return t.detach().cpu().numpy().tobytes()


def ratio(err, bound, worst, key):
    assert (err <= bound).all(), (key, float((err / np.maximum(bound, 1e-300)).max()))
    live = bound > FR.TINY
    if live.any():
        worst[key] = max(worst.get(key, 0.0), float((err[live] / bound[live]).max()))


# ---- pinv ------------------------------------------------------------------------------------------------------------------
def run_pinv(fm, f0, fp, dt, G):
    a, p, d = (t.requires_grad_(True) for t in cuda(f0, fp, dt))
    (tG,) = cuda(G)
    pinv, info = fm.ic_pinv(a, p, d, with_info=True)
    assert not info.requires_grad and pinv.shape == fp.shape
    grads = torch.autograd.grad((pinv * tG).sum(), (a, p, d))
    torch.cuda.synchronize()
    raw = (pinv.detach(), info) + grads
    return dict(raw=raw, **{n: t.cpu().numpy() for n, t in zip(("pinv", "info", "d_f0", "d_fp", "d_dt"), raw)})


def check_pinv_sample(got, b, f0, fp, dt, G, worst):
    K = f0.shape[1]
    tw = FR.pinv_fwd(f0[b], fp[b], dt[b])
    bw = FR.pinv_bwd(tw, dt[b], G[b])
    assert got["info"][b] == tw["flag"], (b, got["info"][b], tw["flag"], tw["kappa"])
    if tw["flag"]:
        assert not got["pinv"][b].any() and not got["d_f0"][b].any() and not got["d_fp"][b].any() and not got["d_dt"][b].any()
        return tw
    ratio(np.abs(got["pinv"][b] - tw["pinv"]), FR.bound(tw["pinv"], tw["mag"], K, tw["kappa"]), worst, "pinv")
    for name in ("f0", "fp", "dt"):
        ratio(np.abs(got["d_" + name][b] - bw["d_" + name]), FR.bound(bw["d_" + name], bw["mag_" + name], K, 3 * tw["kappa"]), worst, "d_" + name)
    return tw


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("K", KS)
def test_pinv_and_both_backwards(fm, K, B):
    f0, fp, dt, _, G = FR.make_features(K, B=B, seed=1, dt=MIXED_DT if B == 3 else 1e-2)
    got, again = run_pinv(fm, f0, fp, dt, G), run_pinv(fm, f0, fp, dt, G)
    for x, y in zip(got["raw"], again["raw"]):
        assert bits(x) == bits(y), "two calls"
    worst = {}
    for b in range(B):
        tw = check_pinv_sample(got, b, f0, fp, dt, G, worst)
        assert tw["flag"] == (1 if K < 6 else 0)   # K < 6 must flag, and give exact zeros (checked above)
    if B == 3:  # sample b of a batch equals its own B = 1 call
        for b in range(B):
            one = run_pinv(fm, f0[b:b + 1], fp[b:b + 1], dt[b:b + 1], G[b:b + 1])
            for x, y in zip(got["raw"], one["raw"]):
                assert bits(x[b:b + 1]) == bits(y), ("batch against single", b)
    print(f"pinv K={K} B={B} worst ratio to the bound:", {k: round(v, 3) for k, v in worst.items()})


def test_pinv_flags(fm):
    f0, fp, dt, _, G = FR.make_features(64, B=3, seed=2)
    clean = run_pinv(fm, f0, fp, dt, G)
    assert clean["info"].tolist() == [0, 0, 0]
    singles = [run_pinv(fm, f0[b:b + 1], fp[b:b + 1], dt[b:b + 1], G[b:b + 1]) for b in range(3)]

    def spoiled(f0=f0, fp=fp, dt=dt, which=1):
        got = run_pinv(fm, f0, fp, dt, G)
        assert got["info"].tolist() == [1 if b == which else 0 for b in range(3)], got["info"]
        assert not got["pinv"][which].any() and not got["d_f0"][which].any() and not got["d_fp"][which].any() and not got["d_dt"][which].any()
        for b in range(3):  # the others keep the bits of their B = 1 call
            if b != which:
                for x, y in zip(got["raw"], singles[b]["raw"]):
                    assert bits(x[b:b + 1]) == bits(y), ("flagged neighbour", b)
    rank = fp.copy()
    rank[1, 4] = rank[1, 1]                  # two equal perturbation rows: a rank-deficient J
    spoiled(fp=rank)
    zero = dt.copy()
    zero[1, 2] = 0.0
    spoiled(dt=zero)
    for bad in (np.nan, np.inf, -np.inf):
        for name in ("f0", "fp", "dt"):
            arr = dict(f0=f0, fp=fp, dt=dt)[name].copy()
            arr.reshape(3, -1)[1, 3] = bad
            spoiled(**{name: arr})


# ---- perturb ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["uniform", "mixed"])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_perturb(fm, N, kind):
    rs = np.random.default_rng([7, N])
    B = 2
    p0 = FR.ellipsoid_cloud(rs, B, N) if N > 1 else rs.standard_normal((B, 1, 3)).astype(np.float32)
    dt = np.full((B, 6), 1e-2, np.float32) if kind == "uniform" else np.stack([MIXED_DT, MIXED_DT[::-1]]).astype(np.float32)
    g_out = rs.standard_normal((B, 6, N, 3)).astype(np.float32)

    def run(p0, dt, g_out):
        tp, td, tg = cuda(p0, dt, g_out)
        td.requires_grad_(True)
        out = fm.ic_perturb(tp, td)
        g_dt, = torch.autograd.grad((out * tg).sum(), td)
        torch.cuda.synchronize()
        return out.detach(), g_dt
    out, g_dt = run(p0, dt, g_out)
    out2, g_dt2 = run(p0, dt, g_out)
    assert bits(out) == bits(out2) and bits(g_dt) == bits(g_dt2), "two calls"
    assert np.array_equal(out.cpu().numpy(), FR.perturb_fwd(p0, dt)), "the float32 chain, bit for bit"
    mine, mag = FR.perturb_bwd(p0, dt, g_out)
    worst = {}
    got = g_dt.cpu().numpy().astype(np.float64)
    ratio(np.abs(got - mine), FR.bound(mine, mag, N), worst, "g_dt")
    h = 1e-6  # central differences of the twin's plain float64 function: 1e-6 relative, plus the differences' own rounding
    for b in range(B):
        for i in range(6):
            e = np.zeros((B, 6))
            e[b, i] = h
            fd = ((FR.perturb_exact(p0, dt.astype(np.float64) + e) * g_out).sum() - (FR.perturb_exact(p0, dt.astype(np.float64) - e) * g_out).sum()) / (2 * h)
            noise = 4 * 2.0 ** -53 / h * np.abs(g_out).sum() * (1.0 + np.abs(p0).max())  # (each term g out is rounded at its own scale)
            assert abs(fd - got[b, i]) <= 1e-6 * abs(fd) + noise, (b, i, fd, got[b, i])
    for b in range(B):  # sample b of the batch equals its own B = 1 call
        o1, g1 = run(p0[b:b + 1], dt[b:b + 1], g_out[b:b + 1])
        assert bits(out[b:b + 1]) == bits(o1) and bits(g_dt[b:b + 1]) == bits(g1)
    print(f"perturb N={N} {kind} worst ratio to the bound:", {k: round(v, 3) for k, v in worst.items()})


# ---- update ----------------------------------------------------------------------------------------------------------------
def update_case(K, B, seed=3):
    f0, fp, dt, f1, _ = FR.make_features(K, B=B, seed=seed)
    pinv, _, _ = FR.head_pinv(f0, fp, dt)
    if K < 6:  # (a flagged pinv is zero: give the sums something to add)
        pinv = (0.01 * np.random.default_rng(K).standard_normal((B, 6, K))).astype(np.float32)
    rs = np.random.default_rng([seed, K, B, 1])
    g = np.stack([FR.exp6(0.3 * rs.standard_normal(6)) for _ in range(B)]).astype(np.float32)
    Gg, Gr, Gdx = (rs.standard_normal(s).astype(np.float32) for s in ((B, 4, 4), (B, K), (B, 6)))
    return pinv, f0, f1, g, Gg, Gr, Gdx


def run_update(fm, pinv, f0, f1, g, Gg, Gr, Gdx, xtol, stop_in=0):
    tp, t0, t1, tg = (t.requires_grad_(True) for t in cuda(pinv, f0, f1, g))
    stop = fm.new_stop()
    stop.fill_(stop_in)
    r, dx, g_new, stop_out = fm.ic_update(tp, t0, t1, tg, stop, xtol)
    assert stop_out is stop
    loss = sum((a * b).sum() for a, b in zip((g_new, r, dx), cuda(Gg, Gr, Gdx)) if b is not None)
    grads = torch.autograd.grad(loss, (tp, t0, t1, tg), allow_unused=True)
    grads = tuple(torch.zeros_like(t) if gr is None else gr for gr, t in zip(grads, (tp, t0, t1, tg)))
    torch.cuda.synchronize()
    raw = (r.detach(), dx.detach(), g_new.detach(), stop.clone()) + grads
    return dict(raw=raw, **{n: t.cpu().numpy() for n, t in zip(("r", "dx", "g_new", "stop", "d_pinv", "d_f0", "d_f1", "d_g"), raw)})


def check_update(got, pinv, f0, f1, g, Gg, Gr, Gdx, xtol, stop_in, worst):
    """A whole result against the twin: r bit for bit, dx within its sum bound, the decision, g_new and the gradients on the
    device's own dx."""
    K = pinv.shape[2]
    r, dx, mag = FR.update_sums(pinv, f0, f1)
    assert got["r"].tobytes() == r.tobytes()
    ratio(np.abs(got["dx"] - dx), FR.bound(dx, mag, K), worst, "dx")
    g_new, gmag, stopped = FR.update_pose(got["dx"], g, xtol, stop_in)
    assert got["stop"].tolist() == [stopped]
    if stopped:
        assert got["g_new"].tobytes() == g.tobytes()
    else:
        ratio(np.abs(got["g_new"] - g_new), FR.bound(g_new, gmag, 4), worst, "g_new")
    bw = FR.update_bwd(pinv, got["r"], got["dx"], g, stopped, Gg, Gr, Gdx)
    if stopped:
        want = (np.zeros_like(g) if Gg is None else Gg, np.zeros_like(f0) if Gr is None else Gr)
        assert got["d_g"].tobytes() == want[0].tobytes() and got["d_f1"].tobytes() == want[1].tobytes()
        assert np.array_equal(got["d_f0"], -want[1]) and not got["d_pinv"].any()
        return stopped
    ratio(np.abs(got["d_g"] - bw["d_g"]), FR.bound(bw["d_g"], bw["mag_g"], 4), worst, "d_g")
    ratio(np.abs(got["d_pinv"] - bw["d_pinv"]), FR.bound(bw["d_pinv"], bw["mag_pinv"], 1), worst, "d_pinv")
    ratio(np.abs(got["d_f1"] - bw["d_f1"]), FR.bound(bw["d_f1"], bw["mag_f1"], 7), worst, "d_f1")
    assert np.array_equal(got["d_f0"], -got["d_f1"])
    return stopped


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("K", KS)
def test_update_and_backward(fm, K, B):
    case = update_case(K, B)
    got, again = run_update(fm, *case, xtol=0.0), run_update(fm, *case, xtol=0.0)
    for x, y in zip(got["raw"], again["raw"]):
        assert bits(x) == bits(y), "two calls"
    worst = {}
    assert check_update(got, *case, 0.0, 0, worst) == 0     # xtol = 0 never stops
    if B == 3:
        for b in range(B):  # sample b of the batch equals its own B = 1 call (xtol = 0: the decision is the same)
            one = run_update(fm, *(None if v is None else v[b:b + 1] for v in case), xtol=0.0)
            for i, (x, y) in enumerate(zip(got["raw"], one["raw"])):
                if i != 3:
                    assert bits(x[b:b + 1]) == bits(y), ("batch against single", b, i)
    print(f"update K={K} B={B} worst ratio to the bound:", {k: round(v, 3) for k, v in worst.items()})


def test_update_stop_rule(fm):
    pinv, f0, f1, g, Gg, Gr, Gdx = update_case(65, 3)
    worst = {}
    # f1 = f0: g_new = g bits, stop = 1
    got = run_update(fm, pinv, f0, f0, g, Gg, Gr, Gdx, xtol=1e-7)
    assert check_update(got, pinv, f0, f0, g, Gg, Gr, Gdx, 1e-7, 0, worst) == 1 and got["g_new"].tobytes() == g.tobytes()
    # a later call with r != 0 still leaves g and passes G' through unchanged
    got = run_update(fm, pinv, f0, f1, g, Gg, Gr, Gdx, xtol=1e-7, stop_in=1)
    assert check_update(got, pinv, f0, f1, g, Gg, Gr, Gdx, 1e-7, 1, worst) == 1
    assert got["dx"].any() and got["g_new"].tobytes() == g.tobytes() and got["d_g"].tobytes() == Gg.tobytes()
    # one moving sample keeps the whole batch going
    f1_one = f0.copy()
    f1_one[1] = f1[1]
    got = run_update(fm, pinv, f0, f1_one, g, Gg, Gr, Gdx, xtol=1e-7)
    assert check_update(got, pinv, f0, f1_one, g, Gg, Gr, Gdx, 1e-7, 0, worst) == 0
    assert not got["dx"][0].any() and np.array_equal(got["g_new"][0], g[0]) and not np.array_equal(got["g_new"][1], g[1])
    # xtol = 0 never stops, not even at r = 0
    got = run_update(fm, pinv, f0, f0, g, Gg, Gr, Gdx, xtol=0.0)
    assert check_update(got, pinv, f0, f0, g, Gg, Gr, Gdx, 0.0, 0, worst) == 0 and np.array_equal(got["g_new"], g)
    # a NaN dx does not stop the batch: that sample's pose is NaN, the others move
    f1_nan = f1.copy()
    f1_nan[2, 0] = np.nan
    got = run_update(fm, pinv, f0, f1_nan, g, None, Gr, None, xtol=1e-7)
    assert got["stop"].tolist() == [0] and np.isnan(got["g_new"][2, :3]).all() and np.isfinite(got["g_new"][:2]).all()
    # each optional gradient input NULL in turn
    for drop in range(3):
        grads = [None if i == drop else v for i, v in enumerate((Gg, Gr, Gdx))]
        got = run_update(fm, pinv, f0, f1, g, *grads, xtol=1e-7)
        assert check_update(got, pinv, f0, f1, g, *grads, 1e-7, 0, worst) == 0
    print("update stop rule worst ratio to the bound:", {k: round(v, 3) for k, v in worst.items()})


def test_batch_boundary_is_refused_not_run(fm):
    """B = 65535 is the largest batch (K = 1 here): only the refusal boundary is checked, nothing that large is launched."""
    from rrl_hip import _lib
    lib = _lib.load()
    fm.check_request("update", (65535, 6, 1), (65535, 1), (65535, 1), (65535, 4, 4))
    with pytest.raises(ValueError, match="65535"):
        fm.check_request("update", (65536, 6, 1), (65536, 1), (65536, 1), (65536, 4, 4))
    small = torch.zeros(64, device="cuda")
    P = small.data_ptr()
    assert lib.rrl_ic_update_workspace_bytes(65535) == 65535 * 4 + 4 and lib.rrl_ic_update_workspace_bytes(65536) == 0
    assert lib.rrl_ic_update_fwd(P, P, P, P, 0.0, P, P, 8, P, P, P, P, 65536, 1, None) == -1
    assert lib.rrl_ic_update_fwd(P, P, P, P, 0.0, P, P, 8, P, P, P, P, 65535, 1, None) == -3   # past the shape check: a short ws


# ---- all three entries: raw calls, NaN-filled outputs, workspace refusals, graph replay ----------------------------------------
def test_raw_entries_prefilled_with_nan_and_replayed(fm):
    from rrl_hip import _lib, ops
    lib = _lib.load()
    B, N, K = 3, 65, 257
    rs = np.random.default_rng(21)
    p0 = FR.ellipsoid_cloud(rs, B, N)
    f0, fp, dt, f1, G = FR.make_features(K, B=B, seed=5, dt=MIXED_DT)
    pinv_h, f0_, f1_, g, Gg, Gr, Gdx = update_case(K, B)
    g_out = rs.standard_normal((B, 6, N, 3)).astype(np.float32)
    tp0, tdt, tgo, tf0, tfp, tf1, tG, tg, tGg, tGr, tGdx = cuda(p0, dt, g_out, f0, fp, f1, G, g, Gg, Gr, Gdx)
    dev, P = tp0.device, ops._p
    nan = lambda *s: torch.full(s, float("nan"), device=dev)  # noqa: E731
    out = dict(pert=nan(B, 6, N, 3), g_dt=nan(B, 6), ws=torch.full((B * FR.WS_DOUBLES,), float("nan"), dtype=torch.float64, device=dev),
               pinv=nan(B, 6, K), info=torch.full((B,), -7, dtype=torch.int32, device=dev), d_f0=nan(B, K), d_fp=nan(B, 6, K), d_dt=nan(B, 6),
               uws=torch.full(((B + 1) // 2,), float("nan"), dtype=torch.float64, device=dev), r=nan(B, K), dx=nan(B, 6), g_new=nan(B, 4, 4),
               stopped=torch.full((1,), -7, dtype=torch.int32, device=dev), stop=torch.zeros(1, dtype=torch.int32, device=dev),
               e_g=nan(B, 4, 4), e_pinv=nan(B, 6, K), e_f0=nan(B, K), e_f1=nan(B, K))

    def calls():
        o = out
        o["stop"].zero_()
        ops._run(dev, "rrl_ic_perturb_fwd", P(tp0), P(tdt), P(o["pert"]), B, N)
        ops._run(dev, "rrl_ic_perturb_bwd", P(tp0), P(tdt), P(tgo), P(o["g_dt"]), B, N)
        ops._run(dev, "rrl_ic_pinv_fwd", P(tf0), P(tfp), P(tdt), P(o["ws"]), o["ws"].numel() * 8, P(o["pinv"]), P(o["info"]), B, K)
        ops._run(dev, "rrl_ic_pinv_bwd", P(tf0), P(tfp), P(tdt), P(o["ws"]), o["ws"].numel() * 8, P(tG), P(o["d_f0"]), P(o["d_fp"]), P(o["d_dt"]), B, K)
        ops._run(dev, "rrl_ic_update_fwd", P(o["pinv"]), P(tf0), P(tf1), P(tg), 1e-7, P(o["stop"]), P(o["uws"]), o["uws"].numel() * 8,
                 P(o["r"]), P(o["dx"]), P(o["g_new"]), P(o["stopped"]), B, K)
        ops._run(dev, "rrl_ic_update_bwd", P(o["pinv"]), P(o["r"]), P(o["dx"]), P(tg), P(o["stopped"]), P(tGg), P(tGr), P(tGdx),
                 P(o["e_g"]), P(o["e_pinv"]), P(o["e_f0"]), P(o["e_f1"]), B, K)
    calls()
    torch.cuda.synchronize()
    first = {k: bits(v) for k, v in out.items()}
    for k, v in out.items():  # every element of every output is written (the workspaces' padding included)
        assert not torch.isnan(v.double()).any() and not (v == -7).any(), k
    # the same numbers as the nodes give
    td = tdt.clone().requires_grad_(True)
    assert bits(fm.ic_perturb(tp0, td)) == first["pert"]
    pinv_node, info_node = fm.ic_pinv(tf0, tfp, tdt, with_info=True)
    assert bits(pinv_node) == first["pinv"] and bits(info_node) == first["info"] and info_node.tolist() == [0] * B
    # refilled with NaN and replayed from a captured graph: the same bits
    for k, v in out.items():
        if k != "stop":
            v.fill_(float("nan") if v.is_floating_point() else -7)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        calls()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        calls()
    for k, v in out.items():
        if k != "stop":
            v.fill_(float("nan") if v.is_floating_point() else -7)
    graph.replay()
    torch.cuda.synchronize()
    for k, v in out.items():
        assert bits(v) == first[k], ("graph replay", k)
    # a short or misaligned workspace is refused (real device pointers: nothing is launched)
    wsb = out["ws"].numel() * 8
    a = lambda t: t.data_ptr()  # noqa: E731
    for ws, nbytes in ((a(out["ws"]), wsb - 1), (a(out["ws"]) + 4, wsb)):
        assert lib.rrl_ic_pinv_fwd(a(tf0), a(tfp), a(tdt), ws, nbytes, a(out["pinv"]), a(out["info"]), B, K, None) == -3
        assert lib.rrl_ic_pinv_bwd(a(tf0), a(tfp), a(tdt), ws, nbytes, a(tG), a(out["d_f0"]), None, None, B, K, None) == -3
    for ws, nbytes in ((a(out["uws"]), 4 * B - 1), (a(out["uws"]) + 4, 16)):
        assert lib.rrl_ic_update_fwd(a(out["pinv"]), a(tf0), a(tf1), a(tg), 1e-7, a(out["stop"]), ws, nbytes, a(out["r"]), a(out["dx"]),
                                     a(out["g_new"]), a(out["stopped"]), B, K, None) == -3
    torch.cuda.synchronize()
    for k, v in out.items():
        assert bits(v) == first[k], ("after the refusals", k)


def test_null_gradients_and_null_outputs_through_the_c_entries(fm):
    """rrl_ic_update_bwd with each of g_g_new / g_r / g_dx NULL in turn, and with all but one NULL: against the twin under the
    file's bounds, and the bits of the call that passes a zero tensor in its place.  Then every gradient OUTPUT of
    rrl_ic_update_bwd and rrl_ic_pinv_bwd NULL in turn: the others keep their bits.  (The node reaches the same NULLs: it does
    not materialise absent gradients -- test_update_stop_rule's last block.)"""
    from rrl_hip import ops
    B, K = 3, 65
    pinv, f0, f1, g, Gg, Gr, Gdx = update_case(K, B)
    tp, t0, t1, tg, tGg, tGr, tGdx = cuda(pinv, f0, f1, g, Gg, Gr, Gdx)
    dev, P = tp.device, ops._p
    r, dx, g_new = torch.empty(B, K, device=dev), torch.empty(B, 6, device=dev), torch.empty(B, 4, 4, device=dev)
    stop, stopped = fm.new_stop(dev), torch.empty(1, dtype=torch.int32, device=dev)
    ws = torch.empty((B + 1) // 2, dtype=torch.float64, device=dev)
    ops._run(dev, "rrl_ic_update_fwd", P(tp), P(t0), P(t1), P(tg), 1e-7, P(stop), P(ws), ws.numel() * 8, P(r), P(dx), P(g_new), P(stopped), B, K)
    assert stopped.tolist() == [0]

    def bwd(gg, gr, gdx, outs=(True, True, True, True)):
        o = [torch.full(s, float("nan"), device=dev) if use else None for s, use in zip(((B, 4, 4), (B, 6, K), (B, K), (B, K)), outs)]
        ops._run(dev, "rrl_ic_update_bwd", P(tp), P(r), P(dx), P(tg), P(stopped), P(gg), P(gr), P(gdx), P(o[0]), P(o[1]), P(o[2]), P(o[3]), B, K)
        torch.cuda.synchronize()
        return o
    names = ("d_g", "d_pinv", "d_f0", "d_f1")
    worst = {}
    for use in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)):
        null = bwd(*(t if u else None for u, t in zip(use, (tGg, tGr, tGdx))))
        zero = bwd(*(t if u else torch.zeros_like(t) for u, t in zip(use, (tGg, tGr, tGdx))))
        for n, a, b in zip(names, null, zero):
            assert not torch.isnan(a).any() and bits(a) == bits(b), (use, n)
        bw = FR.update_bwd(pinv, r.cpu().numpy(), dx.cpu().numpy(), g, 0, *(v if u else None for u, v in zip(use, (Gg, Gr, Gdx))))
        got = {n: t.cpu().numpy() for n, t in zip(names, null)}
        ratio(np.abs(got["d_g"] - bw["d_g"]), FR.bound(bw["d_g"], bw["mag_g"], 4), worst, "d_g")
        ratio(np.abs(got["d_pinv"] - bw["d_pinv"]), FR.bound(bw["d_pinv"], bw["mag_pinv"], 1), worst, "d_pinv")
        ratio(np.abs(got["d_f1"] - bw["d_f1"]), FR.bound(bw["d_f1"], bw["mag_f1"], 7), worst, "d_f1")
        assert np.array_equal(got["d_f0"], -got["d_f1"])
    full = bwd(tGg, tGr, tGdx)
    for drop in range(4):
        part = bwd(tGg, tGr, tGdx, outs=tuple(i != drop for i in range(4)))
        for i, (a, b) in enumerate(zip(part, full)):
            assert (a is None) if i == drop else bits(a) == bits(b), ("update_bwd output", drop, i)
    # pinv's backward: each of d_f0 / d_fp / d_dt NULL in turn
    f0p, fp, dt, _, G = FR.make_features(K, B=B, seed=9, dt=MIXED_DT)
    tf0, tfp, tdt, tG = cuda(f0p, fp, dt, G)
    pws = torch.empty(B * FR.WS_DOUBLES, dtype=torch.float64, device=dev)
    pv, info = torch.empty(B, 6, K, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
    ops._run(dev, "rrl_ic_pinv_fwd", P(tf0), P(tfp), P(tdt), P(pws), pws.numel() * 8, P(pv), None, B, K)   # (info is optional too)
    ops._run(dev, "rrl_ic_pinv_fwd", P(tf0), P(tfp), P(tdt), P(pws), pws.numel() * 8, P(pv), P(info), B, K)
    assert info.tolist() == [0] * B

    def pbwd(outs=(True, True, True)):
        o = [torch.full(s, float("nan"), device=dev) if use else None for s, use in zip(((B, K), (B, 6, K), (B, 6)), outs)]
        ops._run(dev, "rrl_ic_pinv_bwd", P(tf0), P(tfp), P(tdt), P(pws), pws.numel() * 8, P(tG), P(o[0]), P(o[1]), P(o[2]), B, K)
        torch.cuda.synchronize()
        return o
    full = pbwd()
    assert not any(torch.isnan(t).any() for t in full)
    for drop in range(3):
        part = pbwd(tuple(i != drop for i in range(3)))
        for i, (a, b) in enumerate(zip(part, full)):
            assert (a is None) if i == drop else bits(a) == bits(b), ("pinv_bwd output", drop, i)
    print("NULL gradients through the C entries, worst ratio to the bound:", {k: round(v, 3) for k, v in worst.items()})


# ---- the closed loop -------------------------------------------------------------------------------------------------------
class PointNet(torch.nn.Module):
    """The reference's encoder (fmr/model.py:57-126) restated: five shared 1 x 1 convolutions with GroupNorm(8) and ReLU,
    3 -> 64 -> 64 | 64 -> 64 -> 128 -> K, then a max over the points.  The names match the fixture's state_dict."""

    def __init__(self, K):
        super().__init__()
        def mlp(widths):
            layers = []
            for a, b in zip(widths[:-1], widths[1:]):
                layers += [torch.nn.Conv1d(a, b, 1), torch.nn.GroupNorm(8, b), torch.nn.ReLU()]
            return torch.nn.Sequential(*layers)
        self.h1, self.h2 = mlp([3, 64, 64]), mlp([64, 64, 128, K])

    def forward(self, points):
        x = self.h2(self.h1(points.transpose(1, 2)))
        return torch.nn.functional.max_pool1d(x, x.size(-1)).flatten(1)


def ref_exp(x):
    """se_math/se3.py:57-80 exp with sinc.py's branches, batched, any device and dtype."""
    w, v = x[:, :3], x[:, 3:]
    t = w.norm(dim=1).view(-1, 1, 1)
    O = torch.zeros_like(w[:, 0])
    W = torch.stack((torch.stack((O, -w[:, 2], w[:, 1]), 1), torch.stack((w[:, 2], O, -w[:, 0]), 1), torch.stack((-w[:, 1], w[:, 0], O), 1)), 1)
    S = W.bmm(W)
    small = t.abs() < 0.01
    ts = torch.where(small, torch.ones_like(t), t)
    t2 = t * t
    s1 = torch.where(small, 1 - t2 / 6 * (1 - t2 / 20 * (1 - t2 / 42)), torch.sin(ts) / ts)
    s2 = torch.where(small, 0.5 * (1 - t2 / 12 * (1 - t2 / 30 * (1 - t2 / 56))), (1 - torch.cos(ts)) / (ts * ts))
    s3 = torch.where(small, 1 / 6 * (1 - t2 / 20 * (1 - t2 / 42 * (1 - t2 / 72))), (ts - torch.sin(ts)) / (ts ** 3))
    eye = torch.eye(3).to(x)
    R = eye + s1 * W + s2 * S
    p = (eye + s2 * W + s3 * S).bmm(v.reshape(-1, 3, 1))
    bottom = torch.tensor([0.0, 0.0, 0.0, 1.0]).to(x).view(1, 1, 4).repeat(x.shape[0], 1, 1)
    return torch.cat((torch.cat((R, p), 2), bottom), 1)


class RefExp(torch.autograd.Function):
    """se_math/se3.py:133-165 ExpMap restated."""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return ref_exp(x)

    @staticmethod
    def backward(ctx, go):
        x, = ctx.saved_tensors
        dg = torch.from_numpy(FR.GEN).to(x)[None] @ ref_exp(x)[:, None]
        return (go[:, None] * dg).sum((-1, -2))


class RefInv(torch.autograd.Function):
    """se_math/invmat.py:83-112 InvMatrix restated."""

    @staticmethod
    def forward(ctx, x):
        y = torch.stack([m.inverse() for m in x])
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, go):
        y, = ctx.saved_tensors
        return -(y.transpose(1, 2) @ go @ y.transpose(1, 2))


def eager_ic_algo(enc, p0, p1, dt, maxiter, xtol):
    """fmr/model.py:318-439 restated in eager torch on the inputs' device: (r, g_series)."""
    B, N = p0.shape[:2]
    f0 = enc(p0)
    D = RefExp.apply(-torch.diag_embed(dt).reshape(B * 6, 6)).reshape(B, 6, 1, 4, 4)
    p = (D[..., :3, :3] @ p0[:, None, :, :, None]).squeeze(-1) + D[..., :3, 3]
    fp = enc(p.reshape(6 * B, N, 3)).view(B, 6, -1).transpose(1, 2)
    J = (f0.unsqueeze(-1) - fp) / dt.unsqueeze(1)
    Jt = J.transpose(1, 2)
    pinv = RefInv.apply(Jt.bmm(J)).bmm(Jt)
    g = torch.eye(4).to(p0).expand(B, 4, 4).contiguous()
    series, r = [], None
    for _ in range(maxiter):
        p = (g[:, None, :3, :3] @ p1[..., None]).squeeze(-1) + g[:, None, :3, 3]
        r = enc(p) - f0
        dx = -pinv.bmm(r.unsqueeze(-1)).view(B, 6)
        if float(dx.detach().norm(p=2, dim=1, keepdim=True).max()) < xtol:
            break
        g = RefExp.apply(dx).matmul(g)
        series.append(g)
    return r, torch.stack(series)


def test_closed_loop_against_the_recording_and_eager_torch(fm):
    from rrl_hip import callsites
    golden = load_golden("fmr_ic.npz")
    name = str(golden["weights"])
    c = {k[len(name) + 1:]: golden[k] for k in golden.files if k.startswith(name + "_")}
    dist, maxiter, xtol = float(c["loop_dist"]), int(c["maxiter"]), float(c["xtol"])
    assert 0 < dist <= 1e-3  # (a draw behind which no max-pool argmax cascade hides)
    K = c["f0"].shape[1]

    def encoder(device):
        torch.manual_seed(0)
        net = PointNet(K)
        net.load_state_dict({k[2:]: torch.from_numpy(v) for k, v in c.items() if k.startswith("w_")})
        return net.to(device)
    net = encoder("cuda")
    p0, p1, dt = cuda(c["p0"], c["p1"], c["dt"])
    r, g, series, stop, info = callsites.fmr_ic_algo(net, p0, p1, maxiter=maxiter, xtol=xtol, dt=dt[:1])
    assert info.tolist() == [0] * p0.shape[0] and stop.tolist() == [0] and series.shape == (maxiter, *c["g"].shape)
    err = np.abs(series.detach().cpu().numpy() - c["g_out"]).max()
    print(f"closed loop: max |pose - recording| = {err:.3e}, the recording's float32-float64 distance {dist:.3e}, ratio to 2 x {err / (2 * dist):.3f}")
    assert bits(series[-1]) == bits(g)
    assert err <= 2 * dist
    # the encoder's parameter gradients, all poses and r weighted, against eager torch of the restated formulation on this device
    rs = np.random.default_rng(3)
    Wg, Wr = rs.standard_normal(series.shape).astype(np.float32), rs.standard_normal(r.shape).astype(np.float32)

    def grads(module, r, series):
        wg, wr = (torch.from_numpy(v).to(r.device) for v in (Wg, Wr))
        return [v.cpu().numpy() for v in torch.autograd.grad((series * wg).sum() + (r * wr).sum(), list(module.parameters()))]
    mine = grads(net, r, series)
    eager_gpu = grads(net, *eager_ic_algo(net, p0, p1, dt, maxiter, xtol))
    cpu_net = encoder("cpu")
    eager_cpu = grads(cpu_net, *eager_ic_algo(cpu_net, *(torch.from_numpy(c[k]) for k in ("p0", "p1", "dt")), maxiter, xtol))
    worst = 0.0
    for (pname, _), a, b, d in zip(net.named_parameters(), mine, eager_gpu, eager_cpu):
        spread, gap = np.abs(b - d).max(), np.abs(a - b).max()
        worst = max(worst, gap / max(4 * spread, 1e-300))
        assert gap <= 4 * spread, (pname, gap, spread)
    print(f"closed loop gradients: worst |library - eager| / (4 x the CPU-GPU spread of eager) = {worst:.3f}")
    # the call replays from a captured graph with the same bits
    from rrl_hip.graph import GraphedStep
    with torch.no_grad():
        step = GraphedStep(lambda: callsites.fmr_ic_algo(net, p0, p1, maxiter=maxiter, xtol=xtol, dt=dt[:1])[2])
        replayed = step().clone()
    assert bits(replayed) == bits(series)
