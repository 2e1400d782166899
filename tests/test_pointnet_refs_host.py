"""CPU checks of the PointNet encoder's host twin (tests/pointnet_refs.py) against tests/golden/pointnet.npz (recorded from the
reference's own PointNet by tests/golden/make_golden_pointnet.py), of the Python layer's refusals, of the binding and of the
state_dict round trip.  DESIGN.md section 24.

The bound that ties the twin to the fixture is the issue's: the twin's features may be no further from the float64 recording
than the reference's own float32 run is, times 2 -- both are float32 evaluations of the same function that differ in
summation order; the factor 2 covers one unlucky draw over four cases.
"""
import ctypes

import numpy as np
import pytest
import torch

import pointnet_refs as PR
from conftest import load_golden

FAKE = 0x10000   # a non-NULL, 8-byte aligned address the refusals never dereference
E_ARG, E_WS = -1, -3
FMR_GROUPS = (8, 8, 8, 8, 8)


@pytest.fixture(scope="module")
def golden():
    return load_golden("pointnet.npz")


@pytest.fixture(scope="module")
def twin_runs(golden):
    """{case: [forward() of every sample]}, computed once."""
    out = {}
    for name in golden["cases"].tolist():
        p, w = PR.fixture_case(golden, name)
        prm = PR.fmr_params(w)
        out[name] = [PR.forward(p[b], prm, FMR_GROUPS) for b in range(p.shape[0])]
    return out


def test_fixture_holds_the_issues_cases(golden):
    assert golden["cases"].tolist() == ["b2_n64_k32", "b3_n33_k64", "b2_n130_k64", "b1_n257_k1024"]
    for name in golden["cases"].tolist():
        B, N, K = (int(s[1:]) for s in name.split("_"))
        assert golden[f"{name}_p"].shape == (B, N, 3) and golden[f"{name}_f32"].shape == (B, K) and golden[f"{name}_f64"].dtype == np.float64
        assert golden[f"{name}_w_h2.6.weight"].shape == (K, 128, 1) and golden[f"{name}_w_h1.0.weight"].shape == (64, 3, 1)
        rel = float(golden[f"{name}_dist"]) / np.abs(golden[f"{name}_f64"]).max()
        assert 1e-8 < rel < 2e-6, rel    # the reference's own float32 run: a few 1e-7 of max |f|


@pytest.mark.parametrize("name", ["b2_n64_k32", "b3_n33_k64", "b2_n130_k64", "b1_n257_k1024"])
def test_twin_features_within_twice_the_references_own_distance(golden, twin_runs, name):
    f64 = golden[f"{name}_f64"]
    mine = np.stack([r["f"] for r in twin_runs[name]]).astype(np.float64)
    dist, ref = np.abs(mine - f64).max(), float(golden[f"{name}_dist"])
    print(f"{name}: twin {dist:.3e}, reference's float32 {ref:.3e}, ratio {dist / ref:.3f}")
    assert dist <= 2.0 * ref, (dist, ref)


@pytest.mark.parametrize("name", ["b2_n64_k32", "b3_n33_k64"])
def test_exact_float64_restates_the_references_float64_run(golden, name):
    """The plain float64 formulation (conv, biased group variance, relu, max) IS what the reference computes: 1e-12."""
    p, w = PR.fixture_case(golden, name)
    prm = PR.fmr_params(w)
    for b in range(p.shape[0]):
        assert np.abs(PR.exact(p[b], prm, FMR_GROUPS) - golden[f"{name}_f64"][b]).max() < 1e-12


@pytest.mark.parametrize("name", ["b2_n64_k32", "b3_n33_k64"])
def test_twin_pools_the_recorded_point_where_the_feature_is_positive(golden, twin_runs, name):
    """The gradient cases were drawn without near-ties: the extremum rule picks the point the reference's max-pool picks."""
    for b, run in enumerate(twin_runs[name]):
        on = golden[f"{name}_f64"][b] > 0
        assert on.any() and np.array_equal(run["arg"][on], golden[f"{name}_arg"][b][on])


def test_extremum_rule_is_the_max_of_the_activation():
    """max_n h[c][n] = h at the extremum, exactly -- with a gamma < 0 channel, a gamma = 0 channel and duplicated points."""
    rs = np.random.default_rng(5)
    pts = rs.standard_normal((37, 4)).astype(np.float32)
    pts[11] = pts[3]
    pts[30] = pts[3]
    prm = PR.make_stack(4, (8, 24, 40), (8, 8, 4), seed=1)
    run = PR.forward(pts, prm, (8, 8, 4))
    h = PR.act(run["y"][-1], run["a"][-1], run["d"][-1])
    assert run["a"][-1][1] < 0 and run["a"][-1][2] == 0
    assert np.array_equal(h.max(1), run["f"])
    assert np.array_equal(h[np.arange(40), run["arg"]], run["f"])
    y = run["y"][-1]
    up = run["a"][-1] >= 0
    for c in range(40):
        first = np.flatnonzero(y[c] == (y[c].max() if up[c] else y[c].min()))[0]
        assert run["arg"][c] == first
    assert not np.isin(run["arg"], (11, 30)).any()             # a duplicate never wins over its first occurrence


def test_fmaf_chain_starts_at_the_bias():
    W = np.array([[2.0 ** -12, 1.0]], np.float32)
    b = np.array([1.0], np.float32)
    h = np.array([[2.0 ** -12], [2.0 ** -24]], np.float32)
    # bias first: 1 + 2^-24 (exact product) rounds to 1 (tie to even), then + 2^-24 rounds to 1 again; a final addition of the
    # bias to the exact-ish sum 2^-23 would give 1 + 2^-23
    assert PR.chain(W, b, h)[0, 0] == np.float32(1.0)


# ---- the Python layer and the C entries ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from rrl_hip import _lib, build
    build.build_lib()
    return _lib.load()


def _ints(v):
    return (ctypes.c_int32 * len(v))(*v)


def test_entries_in_the_header_and_the_binding(lib):
    from rrl_hip import _abi, _lib, build, callsites, pointnet
    for name in ("rrl_pointnet_workspace_bytes", "rrl_pointnet_fwd", "rrl_pointnet_bwd_workspace_bytes", "rrl_pointnet_bwd"):
        assert name in _abi.PROTOS and name in _lib.EXPORTS and hasattr(lib, name)
    res, args = _abi.PROTOS["rrl_pointnet_fwd"]
    assert res is ctypes.c_int and len(args) == 15 and args[1] is ctypes.c_void_p and args[4] is ctypes.c_double
    assert _abi.PROTOS["rrl_pointnet_workspace_bytes"][0] is ctypes.c_size_t
    C = _abi.CONSTANTS
    assert (C["RRL_PN_MAX_C0"], C["RRL_PN_MAX_LAYERS"], C["RRL_PN_MAX_HIDDEN"]) == (8, 8, 128)
    assert [C["RRL_PN_" + f] for f in pointnet.FIELDS] == list(range(7)) and C["RRL_PN_FIELDS"] == 7
    assert "rrl_pointnet.hip" in build.SOURCES and "-ffp-contract=off" in build.FLAGS
    assert callable(callsites.fmr_encoder)
    # the workspace: the hidden y are 4 * 320 = 1280 bytes per point for FMR, and nothing is K wide per point
    w, g = (64, 64, 64, 128, 1024), FMR_GROUPS
    small, off = pointnet.workspace_layout(1, 1024, 3, w, g)
    big, _ = pointnet.workspace_layout(1, 2048, 3, w, g)
    assert small - off["Y"] == 1280 * 1024
    assert big - small == 1024 * 1280 + 8 * (16 * 1344 + 8 * 1024)   # 1024 points more: their y and eight more chunks' partials
    assert all(off[f] % 8 == 0 for f in ("STAT", "COEF", "PART")) and all(o % 4 == 0 for o in off.values())
    for bad in ((-1, 64, 3, w, g), (65536, 64, 3, w, g), (1, 0, 3, w, g), (1, 64, 0, w, g), (1, 64, 9, w, g), (1, 64, 3, (64,), (8,)),
                (1, 64, 3, (64, 129, 32), (8, 1, 8)), (1, 64, 3, (64, 30), (8, 8)), (1, 64, 3, (64, 16392), (8, 8)),
                (1, 64, 3, (8,) * 9, (8,) * 9)):
        assert pointnet.workspace_layout(*bad)[0] == 0, bad
    assert pointnet.workspace_layout(65535, 1, 1, (1, 1), (1, 1))[0] > 0


def test_c_refusals_return_their_codes_without_a_launch(lib):
    F = FAKE
    w, g = _ints((64, 64, 64, 128, 32)), _ints(FMR_GROUPS)
    wsb = int(lib.rrl_pointnet_workspace_bytes(2, 64, 3, 5, w, g, None))
    prm = (ctypes.c_void_p * 20)(*([F] * 20))
    # (points, params, widths, groups, eps, ws, ws_bytes, feat, arg, info, B, N, c0, L, stream)
    ok = [F, prm, w, g, 1e-5, F, wsb, F, F, F, 2, 64, 3, 5]
    assert wsb > 0
    for i in (0, 1, 2, 3, 5, 7, 8):
        args = list(ok)
        args[i] = None
        assert lib.rrl_pointnet_fwd(*args, None) == E_ARG, i
    for i, v in ((4, 0.0), (4, -1.0), (10, -1), (10, 65536), (11, 0), (12, 0), (12, 9), (13, 1), (13, 9)):
        args = list(ok)
        args[i] = v
        assert lib.rrl_pointnet_fwd(*args, None) == E_ARG, (i, v)
    hole = (ctypes.c_void_p * 20)(*([F] * 7 + [None] + [F] * 12))
    assert lib.rrl_pointnet_fwd(F, hole, *ok[2:], None) == E_ARG
    assert lib.rrl_pointnet_fwd(*ok[:3], _ints((8, 8, 8, 8, 5)), *ok[4:], None) == E_ARG       # 32 % 5 != 0
    assert lib.rrl_pointnet_fwd(*ok[:6], wsb - 1, *ok[7:], None) == E_WS and lib.rrl_pointnet_fwd(*ok[:5], F + 4, *ok[6:], None) == E_WS
    assert lib.rrl_pointnet_fwd(*ok[:5], F + 8, *ok[6:], None) == E_WS                         # 16-byte alignment: the partials are read 16 bytes at a time
    # the batch's upper end: 65535 clouds are served (here: the workspace refusal behind the shape check), 65536 are not
    assert lib.rrl_pointnet_fwd(*ok[:6], 8, *ok[7:10], 65535, *ok[11:], None) == E_WS
    assert lib.rrl_pointnet_fwd(*ok[:10], 0, *ok[11:], None) == 0                              # B = 0: no launch


def test_python_refusals_need_no_gpu():
    from rrl_hip import pointnet
    shapes = []
    last = 3
    for c in (64, 64, 64, 128, 32):
        shapes += [(c, last, 1), (c,), (c,), (c,)]
        last = c
    assert pointnet.check_request((2, 64, 3), shapes, FMR_GROUPS) == (2, 64, 3, (64, 64, 64, 128, 32))
    pointnet.check_request((65535, 1, 3), shapes, FMR_GROUPS)                                   # the boundary itself is served
    flat = [s[:2] if len(s) == 3 else s for s in shapes]
    pointnet.check_request((2, 64, 3), flat, FMR_GROUPS)
    for pts, shp, grp, kw, match in (((2, 64), shapes, FMR_GROUPS, {}, r"\(B, N, c0\)"), ((0, 64, 3), shapes, FMR_GROUPS, {}, "65535"),
                                     ((65536, 64, 3), shapes, FMR_GROUPS, {}, "65535"), ((2, 0, 3), shapes, FMR_GROUPS, {}, "N must"),
                                     ((2, 64, 9), shapes, FMR_GROUPS, {}, "c0"), ((2, 64, 4), shapes, FMR_GROUPS, {}, "W of layer 1"),
                                     ((2, 64, 3), shapes[:4], (8,), {}, "layers"), ((2, 64, 3), shapes[:16], FMR_GROUPS, {}, "20 tensors"),
                                     ((2, 64, 3), shapes, (8, 8, 8, 8, 5), {}, "no multiple"), ((2, 64, 3), shapes, (8, 8, 8, 0, 8), {}, "no multiple"),
                                     ((2, 64, 3), shapes[:5] + [(63,)] + shapes[6:], FMR_GROUPS, {}, "b, gamma and beta"),
                                     ((2, 64, 3), shapes, FMR_GROUPS, dict(eps=0.0), "eps")):
        with pytest.raises(ValueError, match=match):
            pointnet.check_request(pts, shp, grp, **kw)
    wide = [(129, 3), (129,), (129,), (129,), (8, 129), (8,), (8,), (8,)]
    with pytest.raises(ValueError, match="exceeds 128"):
        pointnet.check_request((1, 5, 3), wide, (1, 1))
    with pytest.raises(ValueError, match="exceeds 16384"):
        pointnet.check_request((1, 5, 3), [(8, 3), (8,), (8,), (8,), (16392, 8), (16392,), (16392,), (16392,)], (1, 1))
    with pytest.raises(TypeError):
        pointnet.encode(np.zeros((1, 5, 3)), [], (8, 8))
    with pytest.raises(ValueError, match="widths"):
        pointnet.Encoder(3, (8, 8), (8,))


def test_state_dict_round_trip_is_strict(golden):
    """The module has the reference's keys and shapes: a recorded state_dict loads with strict=True and comes back bit for bit."""
    from rrl_hip import pointnet
    for name in ("b2_n64_k32", "b1_n257_k1024"):
        _, w = PR.fixture_case(golden, name)
        K = int(name.split("_k")[1])
        net = pointnet.Encoder.fmr(K)
        assert tuple(net.state_dict()) == PR.FMR_KEYS and set(w) == set(PR.FMR_KEYS)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
        for k, v in net.state_dict().items():
            assert np.array_equal(v.numpy(), w[k]), k
        for got, want in zip(net.params(), PR.fmr_params(w)):
            assert np.array_equal(got.detach().numpy(), want)
        with pytest.raises(RuntimeError):
            net.load_state_dict({k: torch.from_numpy(v) for k, v in list(w.items())[:-1]}, strict=True)
    rpm = pointnet.Encoder.rpm_prepool()
    sd = rpm.state_dict()
    assert sd["prepool.0.weight"].shape == (64, 4, 1) and sd["prepool.12.weight"].shape == (1024, 128, 1) and sd["prepool.13.bias"].shape == (1024,)
    assert rpm.groups == (8, 8, 8, 8, 16) and len(sd) == 20


@pytest.mark.skipif(torch.cuda.is_available(), reason="the refusal of a machine without a GPU")
def test_without_a_gpu_the_call_raises():
    from rrl_hip import pointnet
    from rrl_hip._lib import RRLError
    with pytest.raises(RRLError):
        pointnet.Encoder.fmr(32)(torch.zeros(1, 5, 3))


# ---- the backward twin -------------------------------------------------------------------------------------------------------
GRAD_NAMES = ("dW", "db", "dgamma", "dbeta")


@pytest.fixture(scope="module")
def golden_grads():
    return load_golden("pointnet_grads.npz")


def _last_layer_case(pts, prm, groups, g):
    fw = PR.forward(pts, prm, groups)
    W, b, gamma, _ = PR.split(prm)[-1]
    h = PR.act(fw["y"][-2], fw["a"][-2], fw["d"][-2])
    st = fw["st"][-1]
    s = np.where(fw["f"] > 0, g.astype(np.float64), 0.0)
    y64 = W.astype(np.float64) @ h.astype(np.float64) + b.astype(np.float64)[:, None]
    ext64 = y64[np.arange(W.shape[0]), fw["arg"]]     # the closed form on the SAME y the dense rule sees: exact algebra
    return h, W, b, gamma, st["mu"], st["r"], groups[-1], ext64, fw["arg"], s


@pytest.mark.parametrize("which", ["narrow", "b2_n64_k32", "b3_n33_k64"])
def test_last_layer_closed_form_is_the_dense_rule(golden, golden_grads, which):
    """dh, dW, db, dgamma, dbeta of the last layer from S1 and the Gram matrix against GroupNorm's dense rule on y_L = W h + b with
    dout = s_c at (c, arg_c): within 1e-12 of the closed form's own sum of |terms|."""
    if which == "narrow":
        rs = np.random.default_rng(2)
        pts, prm, groups = rs.standard_normal((37, 4)).astype(np.float32), PR.make_stack(4, (8, 24, 40), (8, 8, 4), seed=5), (8, 8, 4)
        pts[20] = pts[3]
        g = rs.standard_normal(40).astype(np.float32)
    else:
        p, w = PR.fixture_case(golden, which)
        pts, prm, groups, g = p[1], PR.fmr_params(w), FMR_GROUPS, golden_grads[f"{which}_g"][1]
    case = _last_layer_case(pts, prm, groups, g)
    closed = PR.last_closed(*case)
    mags = PR.last_closed(*case[:-1], np.abs(case[-1]), absmode=True)
    dense = PR.last_dense(*case[:7], case[8], case[9])
    assert np.abs(case[-1]).sum() > 0
    for name, c, d, m in zip(("dh", "dW", "db", "dgamma", "dbeta"), closed, dense, mags):
        assert (np.abs(c - d) <= 1e-12 * m + 1e-300).all(), (name, np.abs(c - d).max())


@pytest.mark.parametrize("name", ["b2_n64_k32", "b3_n33_k64"])
def test_twin_gradients_within_four_times_the_references_own_distance(golden, golden_grads, name):
    """Every gradient of sum(f g) of the twin (float64 backward of its float32 forward) against the reference's float64 run, held
    to 4 x the reference's own float32-to-float64 distance of that gradient."""
    p, w = PR.fixture_case(golden, name)
    prm, g = PR.fmr_params(w), golden_grads[f"{name}_g"]
    runs = [PR.backward_of_forward(p[b], prm, FMR_GROUPS, g[b]) for b in range(p.shape[0])]
    got = {"p": np.stack([r["d_points"] for r in runs])}
    for i, key in enumerate(PR.FMR_KEYS):
        got[key] = sum(r[GRAD_NAMES[i % 4]][i // 4] for r in runs)
    worst = 0.0
    for key, mine in got.items():
        d64, d32 = golden_grads[f"{name}_d64_{key}"].reshape(mine.shape), golden_grads[f"{name}_d32_{key}"].reshape(mine.shape)
        err, ref = np.abs(mine - d64).max(), np.abs(d32.astype(np.float64) - d64).max()
        worst = max(worst, err / ref)
        assert err <= 4 * ref, (key, err, ref)
    print(f"{name}: worst twin gradient distance / the reference's own = {worst:.3f}")


def test_backward_entry_in_the_header_and_its_refusals(lib):
    from rrl_hip import _abi
    res, args = _abi.PROTOS["rrl_pointnet_bwd"]
    assert res is ctypes.c_int and len(args) == 17 and _abi.PROTOS["rrl_pointnet_bwd_workspace_bytes"][0] is ctypes.c_size_t
    F = FAKE
    w, g = _ints((64, 64, 64, 128, 32)), _ints(FMR_GROUPS)
    wsb = int(lib.rrl_pointnet_workspace_bytes(2, 64, 3, 5, w, g, None))
    bwb = int(lib.rrl_pointnet_bwd_workspace_bytes(2, 64, 3, 5, w, g))
    assert bwb == 8 * 2 * (3 * 32 + 2 * 8 + 2 * 128 * 129 + 2 * 128 + 2 * 128 * 64)
    assert lib.rrl_pointnet_bwd_workspace_bytes(65536, 64, 3, 5, w, g) == 0
    prm = (ctypes.c_void_p * 20)(*([F] * 20))
    # (points, params, widths, groups, ws, ws_bytes, arg, g_feat, bws, bws_bytes, d_points, d_params, B, N, c0, L, stream)
    ok = [F, prm, w, g, F, wsb, F, F, F, bwb, None, None, 2, 64, 3, 5]
    for i in (0, 1, 2, 3, 4, 6, 7, 8):
        args = list(ok)
        args[i] = None
        assert lib.rrl_pointnet_bwd(*args, None) == E_ARG, i
    for i, v in ((12, -1), (12, 65536), (13, 0), (14, 9), (15, 1)):
        args = list(ok)
        args[i] = v
        assert lib.rrl_pointnet_bwd(*args, None) == E_ARG, (i, v)
    for i, v in ((5, wsb - 1), (9, bwb - 1), (4, F + 8), (8, F + 4)):
        args = list(ok)
        args[i] = v
        assert lib.rrl_pointnet_bwd(*args, None) == E_WS, (i, v)
    assert lib.rrl_pointnet_bwd(*ok[:12], 0, *ok[13:], None) == 0
