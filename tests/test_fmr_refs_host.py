"""The host twins of FMR's inverse-compositional head (tests/fmr_refs.py) against the reference's
recording (tests/golden/fmr_ic.npz), their analytic backwards against float64 torch autograd of the formulation (the
reference's two custom rules restated as autograd functions here), the stop rule and the deviation, and the refusals of the
Python layer and the C entries that need no GPU."""
import numpy as np
import pytest
import torch

import fmr_refs as FR
from conftest import load_golden

U24 = 2.0 ** -24
E_ARG, E_WS = -1, -3
FAKE = 0x10000  # an address that is never dereferenced: every refusal happens before a HIP call


@pytest.fixture(scope="module")
def golden():
    return load_golden("fmr_ic.npz")


def case_names():
    return [str(c) for c in load_golden("fmr_ic.npz")["cases"]]


def case(golden, name):
    return {k[len(name) + 1:]: golden[k] for k in golden.files if k.startswith(name + "_")}


# ---- the twin against the reference's recording ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", case_names())
def test_twin_reproduces_the_recording_open_loop(golden, name):
    """Recorded features and incoming poses in, pinv / dx / g out.  The reference's float32 head is `*_dist` away from a float64
    evaluation of the same recorded features (recorded by the generator with the reference's own functions); the twin IS that
    evaluation up to 2^-53 terms, rounded once, so it lies within that distance times 1 plus its own final rounding:
      pinv  dist + 2^-24 |pinv|
      dx    dist + 2^-24 |dx| + 2^-24 sum_k |pinv| |r|            (the twin's dx starts from the ROUNDED pinv)
      g     dist + 2^-24 |g| + (1 + |dx|) sum_k delta_k |gen_k g|   (delta = the twin's own part of the dx bound, its last two
                                                                  terms; exp's derivative in direction k is gen_k exp(dx) up to a
                                                                  factor 1 + |dx| / 2)."""
    c = case(golden, name)
    assert (c["cond"] <= 1e4).all()
    pinv, info, steps = FR.open_loop(c["f0"], c["fp"], c["dt"], c["f1"], c["g_in"], float(c["xtol"]))
    assert info.tolist() == [0] * c["f0"].shape[0]
    err = np.abs(pinv.astype(np.float64) - c["pinv"])
    assert (err <= float(c["pinv64_dist"]) + U24 * np.abs(c["pinv"])).all(), err.max()
    worst = {"pinv": float(err.max() / (float(c["pinv64_dist"]) + U24 * np.abs(c["pinv"]).max()))}
    for i, (r, dx, g_new, stopped) in enumerate(steps):
        assert np.array_equal(r, c["r"][i])  # one float32 subtraction
        assert stopped == 1 - int(c["moved"][i])
        mag = np.einsum("bik,bk->bi", np.abs(pinv.astype(np.float64)), np.abs(r.astype(np.float64)))
        delta = float(c["dx64_dist"][i]) + U24 * np.abs(c["dx"][i]) + U24 * mag
        err = np.abs(dx.astype(np.float64) - c["dx"][i])
        assert (err <= delta).all(), (i, err.max())
        worst["dx"] = max(worst.get("dx", 0.0), float((err / np.maximum(delta, 1e-300)).max()))
        if stopped:
            assert g_new.tobytes() == c["g_in"][i].tobytes() and np.array_equal(c["g_out"][i], c["g_in"][i])
            continue
        gen_g = np.abs(FR.GEN[None] @ c["g_out"][i].astype(np.float64)[:, None])                      # (B, 6, 4, 4)
        own = U24 * np.abs(c["dx"][i]) + U24 * mag     # the twin's OWN distance from the float64 dx (the reference's is inside g64_dist)
        slack = (1.0 + np.linalg.norm(c["dx"][i], axis=1))[:, None, None] * np.einsum("bk,bkij->bij", own, gen_g)
        bound = float(c["g64_dist"][i]) + U24 * np.abs(c["g_out"][i]) + slack
        err = np.abs(g_new.astype(np.float64) - c["g_out"][i])
        assert (err <= bound).all(), (i, (err / bound).max())
        worst["g"] = max(worst.get("g", 0.0), float((err / bound).max()))
    print(name, "worst ratio to the bound:", {k: round(v, 3) for k, v in worst.items()})


def test_fixture_jacobian_is_the_header_rule(golden):
    """J as the reference's approx_Jac returned it (float32 arithmetic) against the twin's float64 J from the same features:
    one float32 subtraction and one division, 2^-23 of the subtraction's operands' scale over dt."""
    for name in case_names():
        c = case(golden, name)
        for b in range(c["f0"].shape[0]):
            tw = FR.pinv_fwd(c["f0"][b], c["fp"][b], c["dt"][b])
            scale = (np.abs(c["f0"][b])[:, None] + np.abs(c["fp"][b]).T) / np.abs(c["dt"][b])[None]
            assert (np.abs(tw["J"] - c["J"][b]) <= 2.0 ** -23 * (scale + np.abs(tw["J"]))).all()
            assert abs(tw["kappa"] - c["cond"][b]) <= 1e-3 * c["cond"][b]


# ---- the analytic backwards against float64 autograd of the formulation --------------------------------------------------------
class InvMatrix(torch.autograd.Function):
    """se_math/invmat.py:83-112 restated: y = x^-1, grad_input[m][n] = -sum_jk y[j][m] y[n][k] grad[j][k]."""

    @staticmethod
    def forward(ctx, x):
        y = torch.linalg.inv(x)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, go):
        y, = ctx.saved_tensors
        return -(y.transpose(-1, -2) @ go @ y.transpose(-1, -2))


def torch_exp(x):
    """se_math/se3.py:57-80 exp with sinc.py's branches, (B, 6) -> (B, 4, 4), float64."""
    out = []
    for row in x:
        w, v = row[:3], row[3:]
        t = w.norm()
        W = torch.zeros(3, 3, dtype=x.dtype)
        W[0, 1], W[0, 2], W[1, 0], W[1, 2], W[2, 0], W[2, 1] = -w[2], w[1], w[2], -w[0], -w[1], w[0]
        S = W @ W
        t2 = t * t
        if float(t) < 0.01:
            s1 = 1 - t2 / 6 * (1 - t2 / 20 * (1 - t2 / 42))
            s2 = 0.5 * (1 - t2 / 12 * (1 - t2 / 30 * (1 - t2 / 56)))
            s3 = 1 / 6 * (1 - t2 / 20 * (1 - t2 / 42 * (1 - t2 / 72)))
        else:
            s1, s2, s3 = torch.sin(t) / t, (1 - torch.cos(t)) / t2, (t - torch.sin(t)) / (t2 * t)
        eye = torch.eye(3, dtype=x.dtype)
        g = torch.eye(4, dtype=x.dtype)
        g[:3, :3] = eye + s1 * W + s2 * S
        g[:3, 3] = (eye + s2 * W + s3 * S) @ v
        out.append(g)
    return torch.stack(out)


class ExpMap(torch.autograd.Function):
    """se_math/se3.py:133-165 restated: forward exp, backward grad_x[k] = sum_ij grad[i][j] [gen_k exp(x)]_ij."""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return torch_exp(x)

    @staticmethod
    def backward(ctx, go):
        x, = ctx.saved_tensors
        dg = torch.from_numpy(FR.GEN).to(x)[None] @ torch_exp(x)[:, None]      # (B, 6, 4, 4)
        return (go[:, None] * dg).sum((-1, -2))


def close(mine, want, mag, what):
    err = np.abs(mine - want)
    assert (err <= 1e-12 * mag + 1e-300).all(), (what, float((err / np.maximum(mag, 1e-300)).max()))


@pytest.mark.parametrize("K", [6, 7, 64, 257])
def test_pinv_backward_against_autograd(K):
    f0, fp, dt, _, G = FR.make_features(K, B=2, seed=3, dt=[1e-2, 2e-2, 5e-3, 1e-2, 3e-2, 1e-2])
    for b in range(2):
        tw = FR.pinv_fwd(f0[b], fp[b], dt[b])
        bw = FR.pinv_bwd(tw, dt[b], G[b])
        a, p, d = (torch.from_numpy(v[b].astype(np.float64)).requires_grad_(True) for v in (f0, fp, dt))
        J = (a[:, None] - p.T) / d[None]
        pinv = InvMatrix.apply(J.T @ J) @ J.T
        close(tw["pinv"], pinv.detach().numpy(), tw["kappa"] * tw["mag"], "pinv")
        ga, gp, gd = torch.autograd.grad((pinv * torch.from_numpy(G[b].astype(np.float64))).sum(), (a, p, d))
        k = 1.0 + 3.0 * tw["kappa"]
        close(bw["d_f0"], ga.numpy(), k * bw["mag_f0"], "d_f0")
        close(bw["d_fp"], gp.numpy(), k * bw["mag_fp"], "d_fp")
        close(bw["d_dt"], gd.numpy(), k * bw["mag_dt"], "d_dt")


@pytest.mark.parametrize("scale", [1e-3, 0.05, 0.5])
def test_update_backward_against_autograd(scale):
    """dx from 0.001 (the Taylor branch) to 0.5 rad: ExpMap's rule, not the exact derivative, on both sides."""
    B, K = 2, 40
    rs = np.random.default_rng(11)
    pinv, r = scale * rs.standard_normal((B, 6, K)) / K, rs.standard_normal((B, K))
    f0 = rs.standard_normal((B, K))
    f1 = f0 + r
    g = np.stack([FR.exp6(0.3 * rs.standard_normal(6)) for _ in range(B)])
    Gg, Gr, Gdx = rs.standard_normal((B, 4, 4)), rs.standard_normal((B, K)), rs.standard_normal((B, 6))
    tp, t0, t1, tg = (torch.from_numpy(v).requires_grad_(True) for v in (pinv, f0, f1, g))
    tr = t1 - t0
    tdx = -(tp @ tr[:, :, None])[:, :, 0]
    tnew = ExpMap.apply(tdx) @ tg
    for use in ((1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0)):
        loss = sum(u * (a * torch.from_numpy(b)).sum() for u, a, b in zip(use, (tnew, tr, tdx), (Gg, Gr, Gdx)))
        want = torch.autograd.grad(loss, (tp, t0, t1, tg), retain_graph=True, allow_unused=True)
        want = [np.zeros_like(v) if w is None else w.numpy() for w, v in zip(want, (pinv, f0, f1, g))]
        bw = FR.update_bwd(pinv, tr.detach().numpy(), tdx.detach().numpy(), g, 0, *(x if u else None for u, x in zip(use, (Gg, Gr, Gdx))))
        close(bw["d_pinv"], want[0], bw["mag_pinv"], "d_pinv")
        close(bw["d_f0"], want[1], bw["mag_f1"], "d_f0")
        close(bw["d_f1"], want[2], bw["mag_f1"], "d_f1")
        close(bw["d_g"], want[3], bw["mag_g"], "d_g")
    stopped = FR.update_bwd(pinv, r, tdx.detach().numpy(), g, 1, Gg, Gr, Gdx)
    assert np.array_equal(stopped["d_g"], Gg) and np.array_equal(stopped["d_f1"], Gr) and np.array_equal(stopped["d_f0"], -Gr)
    assert not stopped["d_pinv"].any()


def test_perturb_backward_against_autograd_and_differences():
    rs = np.random.default_rng(5)
    p0 = FR.ellipsoid_cloud(rs, 2, 37)
    dt = np.array([[1e-2] * 6, [1e-3, 0.5, 2e-2, 0.3, 1e-3, 5e-2]], np.float32)
    g_out = rs.standard_normal((2, 6, 37, 3)).astype(np.float32)
    mine, mag = FR.perturb_bwd(p0, dt, g_out)
    td = torch.from_numpy(dt.astype(np.float64)).requires_grad_(True)
    out = []
    for b in range(2):
        D = ExpMap.apply(-torch.diag(td[b]))                                    # approx_Jac's own lines (fmr/model.py:418-424)
        out.append(torch.einsum("ijk,nk->inj", D[:, :3, :3], torch.from_numpy(p0[b].astype(np.float64))) + D[:, None, :3, 3])
    out = torch.stack(out)
    assert np.abs(out.detach().numpy() - FR.perturb_exact(p0, dt)).max() < 1e-14
    want, = torch.autograd.grad((out * torch.from_numpy(g_out.astype(np.float64))).sum(), td)
    close(mine, want.numpy(), mag, "g_dt")
    h = 1e-6  # central differences of the plain float64 function: h^2 / 6 of the third derivative and 2^-53 / h of the sum
    for b in range(2):
        for i in range(6):
            e = np.zeros((2, 6))
            e[b, i] = h
            hi = (FR.perturb_exact(p0, dt.astype(np.float64) + e) * g_out).sum()
            lo = (FR.perturb_exact(p0, dt.astype(np.float64) - e) * g_out).sum()
            fd = (hi - lo) / (2 * h)
            assert abs(fd - mine[b, i]) <= 1e-6 * abs(fd) + 2 * 2.0 ** -53 / h * np.abs(g_out).sum() * 2.0, (b, i, fd, mine[b, i])
    # the float32 chain of the forward against the plain float64 function: three roundings of the products' scale and one of the sum
    chain = FR.perturb_fwd(p0, dt)
    exactv = FR.perturb_exact(p0, dt)
    assert (np.abs(chain - exactv) <= 5 * U24 * (np.abs(p0).sum(2)[:, None, :, None] + 1.0 + np.abs(exactv))).all()


# ---- the stop rule and the deviation ---------------------------------------------------------------------------------------
def test_stop_rule_and_the_deviation(golden):
    f0, fp, dt, f1, _ = FR.make_features(32, B=3, seed=2)
    pinv, info, _ = FR.head_pinv(f0, fp, dt)
    g = np.stack([FR.exp6(0.2 * np.random.default_rng(b).standard_normal(6)) for b in range(3)]).astype(np.float32)
    # r = 0: the batch stops, the poses keep their bits
    r, dx, g_new, stopped = FR.update_fwd(pinv, f0, f0, g, 1e-7, 0)
    assert not r.any() and not dx.any() and stopped == 1 and g_new.tobytes() == g.tobytes()
    # once stopped, a later call with r != 0 still leaves g
    r, dx, g_new, stopped = FR.update_fwd(pinv, f0, f1, g, 1e-7, 1)
    assert dx.any() and stopped == 1 and g_new.tobytes() == g.tobytes()
    # one moving sample keeps the whole batch going (the reference's max over the batch): the still samples get exp(0) g = g
    f1_one = f0.copy()
    f1_one[1] = f1[1]
    r, dx, g_new, stopped = FR.update_fwd(pinv, f0, f1_one, g, 1e-7, 0)
    assert stopped == 0 and not dx[0].any() and dx[1].any() and np.array_equal(g_new[0], g[0]) and not np.array_equal(g_new[1], g[1])
    # xtol = 0 never stops, not even at r = 0
    assert FR.update_fwd(pinv, f0, f0, g, 0.0, 0)[3] == 0
    # a NaN dx is not < xtol: the batch moves on and that sample's pose is NaN
    f1_nan = f0.copy()
    f1_nan[2, 0] = np.nan
    r, dx, g_new, stopped = FR.update_fwd(pinv, f0, f1_nan, g, 1e-7, 0)
    assert stopped == 0 and np.isnan(g_new[2, :3]).all() and np.array_equal(g_new[0], g[0])
    # the deviation: the reference's stop case breaks at iteration 0 and leaves g_series_gpu zero; the loop here holds the last
    # pose in every later entry and `stop` reproduces the zeros
    c = case(golden, "b2_n64_k32_stop")
    assert c["moved"].tolist() == [0] and np.array_equal(c["g"], np.broadcast_to(np.eye(4, dtype=np.float32), c["g"].shape))
    pinv, _, _ = FR.head_pinv(c["f0"], c["fp"], c["dt"])
    stop, series, gcur = 0, [], c["g_in"][0]
    for _ in range(int(c["maxiter"])):
        _, _, gcur, stop = FR.update_fwd(pinv, c["f0"], c["f1"][0], gcur, float(c["xtol"]), stop)
        series.append(gcur)
    assert stop == 1 and all(s.tobytes() == c["g"].tobytes() for s in series)
    assert not np.where(stop, np.zeros_like(series[-1]), series[-1]).any()


def test_flags_of_the_pinv_twin():
    f0, fp, dt, _, G = FR.make_features(64, B=1, seed=4)
    assert FR.pinv_fwd(f0[0], fp[0], dt[0])["flag"] == 0
    for K in (1, 5):
        a, p, d, _, _ = FR.make_features(K, B=1, seed=4)
        tw = FR.pinv_fwd(a[0], p[0], d[0])
        assert tw["flag"] == 1 and not tw["pinv"].any()
    twin_rows = fp.copy()
    twin_rows[0, 4] = twin_rows[0, 1]        # two equal perturbation rows: a rank-deficient J
    assert FR.pinv_fwd(f0[0], twin_rows[0], dt[0])["flag"] == 1
    zero_dt = dt.copy()
    zero_dt[0, 3] = 0.0
    assert FR.pinv_fwd(f0[0], fp[0], zero_dt[0])["flag"] == 1
    for bad in (np.nan, np.inf, -np.inf):
        spoiled = f0.copy()
        spoiled[0, 7] = bad
        tw = FR.pinv_fwd(spoiled[0], fp[0], dt[0])
        assert tw["flag"] == 1 and not FR.pinv_bwd(tw, dt[0], G[0])["d_fp"].any()


def test_closed_loop_twin_recovers_the_pose(golden):
    """The twin's closed loop around a smooth stand-in encoder (moments of the cloud): a 0.1 rad pose comes back."""
    rs = np.random.default_rng(9)
    p0 = FR.ellipsoid_cloud(rs, 2, 80)
    T = np.stack([FR.exp6(x) for x in 0.06 * rs.standard_normal((2, 6))])
    p1 = (np.einsum("bij,bnj->bni", T[:, :3, :3], p0.astype(np.float64)) + T[:, None, :3, 3]).astype(np.float32)

    def encoder(p):
        p = p.astype(np.float64)
        second = np.einsum("bni,bnj->bij", p, p).reshape(len(p), 9) / p.shape[1]
        third = np.einsum("bni,bnj,bnk->bijk", p, p, p).reshape(len(p), 27) / p.shape[1]
        return np.concatenate([p.mean(1), second, third], 1).astype(np.float32)
    r, g, series, stop, info = FR.closed_loop(encoder, p0, p1, [[1e-2] * 6], 10, 1e-7)
    assert info.tolist() == [0, 0] and series.shape == (10, 2, 4, 4)
    want = np.linalg.inv(T)
    assert np.abs(g - want).max() < 1e-3 and np.abs(r).max() < 1e-4


# ---- the Python layer and the C entries ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from rrl_hip import _lib, build
    build.build_lib()
    return _lib.load()


def test_entries_in_the_header_and_the_binding(lib):
    from rrl_hip import _abi, _lib, callsites, fmr
    names = ("rrl_ic_perturb_fwd", "rrl_ic_perturb_bwd", "rrl_ic_pinv_workspace_bytes", "rrl_ic_pinv_fwd", "rrl_ic_pinv_bwd",
             "rrl_ic_update_workspace_bytes", "rrl_ic_update_fwd", "rrl_ic_update_bwd")
    for name in names:
        assert name in _abi.PROTOS and name in _lib.EXPORTS and hasattr(lib, name)
    assert not any("ic_" in s for s in _abi.STRUCTS)
    assert _abi.CONSTANTS["RRL_IC_MAX_K"] == fmr.MAX_K == 16384 and _abi.CONSTANTS["RRL_IC_WS_DOUBLES"] == FR.WS_DOUBLES
    assert all(callable(f) for f in (fmr.ic_perturb, fmr.ic_pinv, fmr.ic_update, callsites.fmr_approx_jac, callsites.fmr_ic_algo))
    assert lib.rrl_ic_pinv_workspace_bytes(3, 64) == 3 * 40 * 8 and lib.rrl_ic_update_workspace_bytes(3) == 16
    for shape in ((-1, 8), (65536, 8), (1, 0), (1, 16385)):
        assert lib.rrl_ic_pinv_workspace_bytes(*shape) == 0, shape


def test_c_refusals_return_their_codes_without_a_launch(lib):
    F = FAKE
    # perturb: (p0, dt, out, B, N, stream) and (p0, dt, g_out, g_dt, B, N, stream)
    for args in ((None, F, F, 2, 10), (F, None, F, 2, 10), (F, F, None, 2, 10), (F, F, F, -1, 10), (F, F, F, 65536, 10), (F, F, F, 2, 0)):
        assert lib.rrl_ic_perturb_fwd(*args, None) == E_ARG, args
    for args in ((None, F, F, F, 2, 10), (F, F, None, F, 2, 10), (F, F, F, None, 2, 10), (F, F, F, F, 65536, 10), (F, F, F, F, 2, 0)):
        assert lib.rrl_ic_perturb_bwd(*args, None) == E_ARG, args
    assert lib.rrl_ic_perturb_fwd(F, F, F, 0, 10, None) == 0 and lib.rrl_ic_perturb_bwd(F, F, F, F, 0, 10, None) == 0
    # pinv: (f0, fp, dt, ws, ws_bytes, pinv, info, B, K, stream) and (f0, fp, dt, ws, ws_bytes, g_pinv, d_f0, d_fp, d_dt, B, K, stream)
    wsb = int(lib.rrl_ic_pinv_workspace_bytes(2, 64))
    for args in ((None, F, F, F, wsb, F, F, 2, 64), (F, None, F, F, wsb, F, F, 2, 64), (F, F, None, F, wsb, F, F, 2, 64),
                 (F, F, F, None, wsb, F, F, 2, 64), (F, F, F, F, wsb, None, F, 2, 64), (F, F, F, F, wsb, F, F, -1, 64),
                 (F, F, F, F, wsb, F, F, 65536, 64), (F, F, F, F, wsb, F, F, 2, 0), (F, F, F, F, wsb, F, F, 2, 16385)):
        assert lib.rrl_ic_pinv_fwd(*args, None) == E_ARG, args
    for args in ((F, F, F, F, wsb - 1, F, F, 2, 64), (F, F, F, F + 4, wsb, F, F, 2, 64)):
        assert lib.rrl_ic_pinv_fwd(*args, None) == E_WS, args
    for args in ((None, F, F, F, wsb, F, F, F, F, 2, 64), (F, F, F, F, wsb, None, F, F, F, 2, 64), (F, F, F, F, wsb, F, F, F, F, 2, 16385)):
        assert lib.rrl_ic_pinv_bwd(*args, None) == E_ARG, args
    for args in ((F, F, F, F, wsb - 1, F, F, F, F, 2, 64), (F, F, F, F + 4, wsb, F, F, F, F, 2, 64)):
        assert lib.rrl_ic_pinv_bwd(*args, None) == E_WS, args
    assert lib.rrl_ic_pinv_fwd(F, F, F, F, 0, F, F, 0, 64, None) == 0 and lib.rrl_ic_pinv_bwd(F, F, F, F, 0, F, F, F, F, 0, 64, None) == 0
    # update: (pinv, f0, f1, g, xtol, stop, ws, ws_bytes, r, dx, g_new, stopped, B, K, stream)
    ok = [F, F, F, F, 1e-7, F, F, 8, F, F, F, F, 2, 64]
    for i in (0, 1, 2, 3, 5, 6, 8, 9, 10, 11):
        args = list(ok)
        args[i] = None
        assert lib.rrl_ic_update_fwd(*args, None) == E_ARG, i
    # the batch's upper end: 65535 samples are served (here: the workspace refusal behind the shape check), 65536 are not
    assert lib.rrl_ic_update_fwd(*ok[:12], 65536, 1, None) == E_ARG
    assert lib.rrl_ic_update_workspace_bytes(65535) == 65535 * 4 + 4 and lib.rrl_ic_update_workspace_bytes(65536) == 0
    assert lib.rrl_ic_update_fwd(*ok[:7], 65535 * 4, *ok[8:12], 65535, 1, None) == E_WS
    assert lib.rrl_ic_update_fwd(*ok[:7], 7, *ok[8:], None) == E_WS and lib.rrl_ic_update_fwd(*ok[:6], F + 4, *ok[7:], None) == E_WS
    assert lib.rrl_ic_update_fwd(*ok[:12], 0, 64, None) == 0
    # update backward: (pinv, r, dx, g, stopped, g_g_new, g_r, g_dx, d_g, d_pinv, d_f0, d_f1, B, K, stream)
    okb = [F, F, F, F, F, None, None, None, F, F, F, F, 2, 64]
    for i in (0, 1, 2, 3, 4):
        args = list(okb)
        args[i] = None
        assert lib.rrl_ic_update_bwd(*args, None) == E_ARG, i
    assert lib.rrl_ic_update_bwd(*okb[:12], 2, 0, None) == E_ARG and lib.rrl_ic_update_bwd(*okb[:12], 0, 64, None) == 0


def test_python_refusals_need_no_gpu():
    from rrl_hip import fmr
    fmr.check_request("perturb", (2, 64, 3), (2, 6))
    fmr.check_request("pinv", (2, 32), (2, 6, 32), (2, 6))
    fmr.check_request("update", (2, 6, 32), (2, 32), (2, 32), (2, 4, 4))
    for kind, args, match in (("perturb", ((2, 64, 4), (2, 6)), r"\(B, N, 3\)"), ("perturb", ((2, 64, 3), (1, 6)), "expand"),
                              ("perturb", ((2, 0, 3), (2, 6)), "empty"), ("perturb", ((0, 5, 3), (0, 6)), "65535"),
                              ("perturb", ((65536, 5, 3), (65536, 6)), "65535"),
                              ("pinv", ((2, 32, 1), (2, 6, 32), (2, 6)), r"\(B, K\)"), ("pinv", ((2, 32), (2, 32, 6), (2, 6)), "viewed as"),
                              ("pinv", ((2, 32), (2, 6, 32), (2, 5)), "dt must be"), ("pinv", ((2, 16385), (2, 6, 16385), (2, 6)), "16384"),
                              ("pinv", ((2, 0), (2, 6, 0), (2, 6)), "16384"),
                              ("update", ((2, 5, 32), (2, 32), (2, 32), (2, 4, 4)), r"\(B, 6, K\)"),
                              ("update", ((2, 6, 32), (2, 31), (2, 32), (2, 4, 4)), "f0 must be"),
                              ("update", ((2, 6, 32), (2, 32), (3, 32), (2, 4, 4)), "f1 must be"),
                              ("update", ((2, 6, 32), (2, 32), (2, 32), (2, 3, 4)), "g must be"),
                              ("update", ((2, 6, 32), (2, 32), (2, 32), (2, 4, 4), (2,)), "one int32 word"),
                              ("update", ((65536, 6, 1), (65536, 1), (65536, 1), (65536, 4, 4)), "65535"),
                              ("other", ((1,),), "kind must be")):
        with pytest.raises(ValueError, match=match):
            fmr.check_request(kind, *args)
    fmr.check_request("update", (65535, 6, 1), (65535, 1), (65535, 1), (65535, 4, 4))   # the boundary itself is served
    with pytest.raises(ValueError, match="xtol"):
        fmr.check_request("update", (2, 6, 32), (2, 32), (2, 32), (2, 4, 4), xtol=-1.0)
    with pytest.raises(TypeError):
        fmr.ic_pinv(np.zeros((1, 8)), torch.zeros(1, 6, 8), torch.zeros(1, 6))
    with pytest.raises(ValueError, match="on the GPU"):
        fmr.ic_update(torch.zeros(1, 6, 8), torch.zeros(1, 8), torch.zeros(1, 8), torch.zeros(1, 4, 4), torch.zeros(1, dtype=torch.int32))


@pytest.mark.skipif(torch.cuda.is_available(), reason="the refusal of a machine without a GPU")
def test_without_a_gpu_the_call_raises():
    from rrl_hip import callsites, fmr
    from rrl_hip._lib import RRLError
    with pytest.raises(RRLError):
        fmr.ic_perturb(torch.zeros(1, 5, 3), torch.full((1, 6), 0.01))
    with pytest.raises(RRLError):
        fmr.ic_pinv(torch.zeros(1, 8), torch.zeros(1, 6, 8), torch.full((1, 6), 0.01))
    with pytest.raises(RRLError):
        callsites.fmr_ic_algo(lambda p: p.mean(1), torch.zeros(1, 5, 3), torch.zeros(1, 5, 3))
