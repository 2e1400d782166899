"""CPU checks of the grouped PointNet's host twin (tests/pointnet_group_refs.py) against tests/golden/pointnet_group.npz and
pointnet_group_grads.npz (recorded from the reference's own get_prepool + torch.max by tests/golden/make_golden_pointnet_group.py),
of the binding, the refusals and the state_dict keys.  DESIGN.md section 25.

Bounds, as the issue sets them: the twin's features no further from the float64 recording than 2 x the recording's own
float32-to-float64 distance; its gradients within 4 x that distance of each gradient (section 24's allowance); the closed form
of the last layer's backward equal to the dense rule within 1e-12 sum|terms|.
"""
import ctypes

import numpy as np
import pytest
import torch

import pointnet_group_refs as GP
import pointnet_refs as PR
from conftest import load_golden

FAKE = 0x10000   # a non-NULL, 16-byte aligned address the refusals never dereference
E_ARG, E_WS = -1, -3
G3 = (8, 8, 8)


@pytest.fixture(scope="module")
def golden():
    return load_golden("pointnet_group.npz")


@pytest.fixture(scope="module")
def grads():
    return load_golden("pointnet_group_grads.npz")


@pytest.fixture(scope="module")
def rpm130(golden):
    """(x (B, N, S, 10), params, [twin forward of every sample]) of the forward-only case, computed once."""
    x = GP.rpm_raw_case(load_golden("ball_query_rpm.npz"))
    prm = GP.rpm_params(GP.fixture_weights(golden, "rpm130"))
    return x, prm, [GP.forward(x[b], prm, G3) for b in range(x.shape[0])]


@pytest.fixture(scope="module")
def grad_twins(grads):
    """{case: (x, params, [twin forward per sample])}, computed once."""
    out = {}
    for name in grads["cases"].tolist():
        x, prm = grads[f"{name}_x"], GP.rpm_params(GP.fixture_weights(grads, name))
        out[name] = (x, prm, [GP.forward(x[b], prm, G3) for b in range(x.shape[0])])
    return out


def test_fixture_holds_the_issues_cases(golden, grads, rpm130):
    assert golden["cases"].tolist() == ["rpm130"] and grads["cases"].tolist() == ["b2_n5_s20_f96", "b2_n7_s64_f32"]
    x = rpm130[0]
    assert x.shape == (2, 130, 16, 10) and golden["rpm130_f64"].shape == (2, 192, 130)
    assert (x[:, :, 1:] == x[:, :, :-1]).all(-1).any()          # repeated slots: ball-query's padding
    assert grads["b2_n5_s20_f96_x"].shape == (2, 5, 20, 10) and grads["b2_n7_s64_f32_x"].shape == (2, 7, 64, 10)
    for name in grads["cases"].tolist():
        assert float(grads[f"{name}_gap"]) >= 1.0e-3


def test_twin_features_within_twice_the_recordings_own_distance(golden, rpm130):
    out = np.stack([fw["out"] for fw in rpm130[2]])
    err = float(np.abs(out.astype(np.float64) - golden["rpm130_f64"]).max())
    print("twin / recording distance:", err / float(golden["rpm130_dist"]))
    assert err <= 2.0 * float(golden["rpm130_dist"])


def test_exact_float64_restates_the_float64_recording(golden, rpm130):
    x, prm, _ = rpm130
    out = np.stack([GP.exact(x[b], prm, G3) for b in range(x.shape[0])])
    assert np.abs(out - golden["rpm130_f64"]).max() <= 1e-12 * np.abs(golden["rpm130_f64"]).max()


@pytest.mark.parametrize("name", ["b2_n5_s20_f96", "b2_n7_s64_f32"])
def test_twin_pools_the_recorded_slot_and_its_gradients_hold(grads, grad_twins, name):
    x, prm, fws = grad_twins[name]
    out = np.stack([fw["out"] for fw in fws])
    assert np.abs(out.astype(np.float64) - grads[f"{name}_f64"]).max() <= 2.0 * float(grads[f"{name}_dist"])
    on = grads[f"{name}_f64"] > 0
    arg = np.stack([fw["arg"] for fw in fws])
    assert (arg[on] == grads[f"{name}_arg"][on]).all()
    runs = [GP.backward_of_forward(x[b], prm, G3, grads[f"{name}_g"][b]) for b in range(x.shape[0])]
    twin = {"x": np.stack([r["d_x"] for r in runs])}
    for i, key in enumerate(GP.RPM_KEYS):
        twin[key] = sum(r[("dW", "db", "dgamma", "dbeta")[i % 4]][i // 4] for r in runs)
    for key, val in twin.items():
        d32, d64 = grads[f"{name}_d32_{key}"].astype(np.float64), grads[f"{name}_d64_{key}"]
        own = np.abs(d32 - d64).max()
        err = np.abs(val.reshape(d64.shape) - d64).max()
        print(name, key, "twin / recording distance:", err / own)
        assert err <= 4.0 * own, key


def _random_last(seed, N, S, H, K, G, dup):
    rs = np.random.default_rng(seed)
    h = np.maximum(0, rs.standard_normal((H, N * S))).astype(np.float32)
    if dup:
        h3 = h.reshape(H, N, S)
        h3[:, :, 3] = h3[:, :, 1]
    W = (rs.standard_normal((K, H)) / np.sqrt(H)).astype(np.float32)
    b, gamma, beta = (0.1 * rs.standard_normal(K)).astype(np.float32), (1 + 0.2 * rs.standard_normal(K)).astype(np.float32), \
        (0.2 * rs.standard_normal(K)).astype(np.float32)
    gamma[1], gamma[2] = -0.7, 0.0
    y = PR.chain(W, b, h)
    st = PR.stats(y, G)
    a, d = PR.coef(gamma, beta, st["mu"], st["r"])
    ext, arg, out = GP.pool_points(y, a, d, S)
    s = np.where(out > 0, rs.standard_normal((K, N)), 0.0)
    return h, W, b, gamma, st, y, a, d, ext, arg, out, s


@pytest.mark.parametrize("N,S,dup", [(5, 20, False), (3, 7, True), (9, 1, False)])
def test_last_layer_closed_form_is_the_dense_rule(N, S, dup):
    h, W, b, gamma, st, y, a, d, ext, arg, out, s = _random_last(5, N, S, 12, 16, 4, dup and S > 3)
    closed = GP.last_closed(h, W, b, gamma, st["mu"], st["r"], 4, ext, arg, s, S)
    mags = GP.last_closed(h, W, b, gamma, st["mu"], st["r"], 4, ext, arg, np.abs(s), S, absmode=True)
    # the dense rule runs on the float64 y = W h + b, the closed form on ext taken from it: feed the dense rule's own extrema
    y64 = W.astype(np.float64) @ h.astype(np.float64) + b.astype(np.float64)[:, None]
    ext64 = np.take_along_axis(y64, GP.positions(arg, S), 1)
    closed = GP.last_closed(h, W, b, gamma, st["mu"], st["r"], 4, ext64, arg, s, S)
    dense = GP.last_dense(h, W, b, gamma, st["mu"], st["r"], 4, arg, s, S)
    for got, want, mag in zip(closed, dense, mags):
        assert (np.abs(got - want) <= 1e-12 * mag + 1e-300).all()


def test_one_slot_is_the_plain_activation_and_ties_go_to_the_lowest_slot():
    h, W, b, gamma, st, y, a, d, ext, arg, out, s = _random_last(7, 9, 1, 12, 16, 4, False)
    assert (arg == 0).all() and np.array_equal(out, PR.act(y, a, d)) and np.array_equal(ext, y)
    h, W, b, gamma, st, y, a, d, ext, arg, out, s = _random_last(8, 6, 8, 12, 16, 4, True)
    y3 = y.reshape(16, 6, 8)
    assert np.array_equal(y3[:, :, 3], y3[:, :, 1])          # equal slots give exactly equal chains
    assert not (arg == 3).any() and (arg == 1).any()          # a copy never wins over its first occurrence
    assert np.array_equal(out, PR.act(y, a, d).reshape(16, 6, 8).max(2))   # the extremum rule is the max of the activation
    up = a >= 0
    assert np.array_equal(ext[up], y3.max(2)[up]) and np.array_equal(ext[~up], y3.min(2)[~up]) and (~up).any()


# ---- the binding and the C entries ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from rrl_hip import _lib, build
    build.build_lib()
    return _lib.load()


def _ints(v):
    return (ctypes.c_int32 * len(v))(*v)


def test_entries_and_constants_in_the_header_and_the_binding(lib):
    from rrl_hip import _abi, _lib, build, callsites, pointnet
    for name in ("rrl_pointnet_group_workspace_bytes", "rrl_pointnet_group_fwd", "rrl_pointnet_group_bwd_workspace_bytes",
                 "rrl_pointnet_group_bwd"):
        assert name in _abi.PROTOS and name in _lib.EXPORTS and hasattr(lib, name)
    res, args = _abi.PROTOS["rrl_pointnet_group_fwd"]
    assert res is ctypes.c_int and len(args) == 16 and args[4] is ctypes.c_double
    assert len(_abi.PROTOS["rrl_pointnet_group_bwd"][1]) == 18
    assert _abi.PROTOS["rrl_pointnet_group_workspace_bytes"][0] is ctypes.c_size_t
    C = _abi.CONSTANTS
    assert (C["RRL_PG_MAX_C0"], C["RRL_PG_MAX_S"], C["RRL_PG_MAX_K"]) == (16, 128, 1024)
    assert (C["RRL_PN_MAX_C0"], C["RRL_PN_MAX_LAYERS"], C["RRL_PN_MAX_HIDDEN"]) == (8, 8, 128)   # the existing limits stay
    assert [C["RRL_PG_" + f] for f in pointnet.PG_FIELDS] == list(range(6)) and C["RRL_PG_FIELDS"] == 6
    assert "rrl_pointnet_group.hip" in build.SOURCES
    assert callable(callsites.rpm_feat_prepool_pool) and callable(callsites.rpm_feat_extractor)
    # the workspace: y_1, y_2 over the positions (4 * 192 bytes each) and ext per point; nothing K wide per position
    w = (96, 96, 192)
    small, off = pointnet.group_workspace_layout(1, 1024, 64, 10, w, G3)
    assert small - off["Y"] == 4 * 192 * 1024 * 64 and off["FLAG"] - off["EXT"] == 4 * 192 * 1024
    assert off["EXT"] - off["PART"] == 16 * 384 * 512                     # 512 chunks of two points
    assert all(off[f] % 16 == 0 for f in ("STAT", "COEF", "PART")) and all(o % 4 == 0 for o in off.values())
    for bad in ((-1, 8, 4, 10, w, G3), (65536, 8, 4, 10, w, G3), (1, 0, 4, 10, w, G3), (1, 8, 0, 10, w, G3), (1, 8, 129, 10, w, G3),
                (1, 8, 4, 0, w, G3), (1, 8, 4, 17, w, G3), (1, (1 << 20) + 1, 1, 10, w, G3), (1, 1 << 16, 128, 10, w, G3),
                (1, 8, 4, 10, (96,), (8,)), (1, 8, 4, 10, (96, 129, 32), (8, 1, 8)), (1, 8, 4, 10, (96, 30), (8, 8)),
                (1, 8, 4, 10, (96, 1032), (8, 8)), (1, 8, 4, 10, (8,) * 9, (8,) * 9)):
        assert pointnet.group_workspace_layout(*bad)[0] == 0, bad
        assert lib.rrl_pointnet_group_bwd_workspace_bytes(*bad[:4], len(bad[4]), _ints(bad[4]), _ints(bad[5])) == 0, bad
    assert pointnet.group_workspace_layout(1, 1 << 15, 128, 16, (128, 1024), (8, 8))[0] > 0     # N S = 2^22 is served
    assert lib.rrl_pointnet_group_bwd_workspace_bytes(2, 7, 64, 10, 3, _ints(w), _ints(G3)) > 0


def test_c_refusals_return_their_codes_without_a_launch(lib):
    F = FAKE
    w, g = _ints((96, 96, 192)), _ints(G3)
    wsb = int(lib.rrl_pointnet_group_workspace_bytes(2, 7, 64, 10, 3, w, g, None))
    bwb = int(lib.rrl_pointnet_group_bwd_workspace_bytes(2, 7, 64, 10, 3, w, g))
    prm = (ctypes.c_void_p * 12)(*([F] * 12))
    # (x, params, widths, groups, eps, ws, ws_bytes, out, arg, info, B, N, S, c0, L, stream)
    ok = [F, prm, w, g, 1e-5, F, wsb, F, F, F, 2, 7, 64, 10, 3]
    assert wsb > 0 and bwb > 0
    for i in (0, 1, 2, 3, 5, 7, 8):
        args = list(ok)
        args[i] = None
        assert lib.rrl_pointnet_group_fwd(*args, None) == E_ARG, i
    for i, v in ((4, 0.0), (4, -1.0), (10, -1), (10, 65536), (11, 0), (11, (1 << 20) + 1), (12, 0), (12, 129), (13, 0), (13, 17),
                 (14, 1), (14, 9)):
        args = list(ok)
        args[i] = v
        assert lib.rrl_pointnet_group_fwd(*args, None) == E_ARG, (i, v)
    hole = (ctypes.c_void_p * 12)(*([F] * 7 + [None] + [F] * 4))
    assert lib.rrl_pointnet_group_fwd(F, hole, *ok[2:], None) == E_ARG
    assert lib.rrl_pointnet_group_fwd(*ok[:3], _ints((8, 8, 5)), *ok[4:], None) == E_ARG       # 192 % 5 != 0
    assert lib.rrl_pointnet_group_fwd(*ok[:6], wsb - 1, *ok[7:], None) == E_WS
    assert lib.rrl_pointnet_group_fwd(*ok[:5], F + 8, *ok[6:], None) == E_WS                   # 16-byte alignment
    assert lib.rrl_pointnet_group_fwd(*ok[:10], 0, *ok[11:], None) == 0                        # B = 0: no launch
    # (x, params, widths, groups, ws, ws_bytes, arg, g_out, bws, bws_bytes, d_x, d_params, B, N, S, c0, L, stream)
    okb = [F, prm, w, g, F, wsb, F, F, F, bwb, F, None, 2, 7, 64, 10, 3]
    for i in (0, 1, 2, 3, 4, 6, 7, 8):
        args = list(okb)
        args[i] = None
        assert lib.rrl_pointnet_group_bwd(*args, None) == E_ARG, i
    for i, v in ((12, -1), (13, 0), (14, 129), (15, 17), (16, 1)):
        args = list(okb)
        args[i] = v
        assert lib.rrl_pointnet_group_bwd(*args, None) == E_ARG, (i, v)
    assert lib.rrl_pointnet_group_bwd(*okb[:5], wsb - 1, *okb[6:], None) == E_WS
    assert lib.rrl_pointnet_group_bwd(*okb[:9], bwb - 1, *okb[10:], None) == E_WS
    assert lib.rrl_pointnet_group_bwd(*okb[:8], F + 4, *okb[9:], None) == E_WS
    assert lib.rrl_pointnet_group_bwd(*okb[:12], 0, *okb[13:], None) == 0


def test_python_refusals_need_no_gpu():
    from rrl_hip import pointnet
    prm = [torch.zeros(s) for s in ((96, 10, 1, 1), (96,), (96,), (96,), (192, 96), (192,), (192,), (192,))]
    shapes = [tuple(p.shape) for p in prm]
    assert pointnet.check_group_request((2, 7, 64, 10), shapes, (8, 8)) == (2, 7, 64, 10, (96, 192))
    for bad_shape in ((2, 7, 64), (0, 7, 64, 10), (2, 7, 129, 10), (2, 7, 64, 17), (2, 1 << 16, 128, 10), (2, 7, 64, 9)):
        with pytest.raises(ValueError):
            pointnet.check_group_request(bad_shape, shapes, (8, 8))
    for bad_groups in ((8,), (8, 5), (8, True), (8, 8, 8)):
        with pytest.raises(ValueError):
            pointnet.check_group_request((2, 7, 64, 10), shapes, bad_groups)
    with pytest.raises(ValueError):
        pointnet.check_group_request((2, 7, 64, 10), shapes, (8, 8), eps=0.0)
    with pytest.raises(ValueError):
        pointnet.check_group_request((2, 7, 64, 10), shapes[:4] + [(1032, 96), (1032,), (1032,), (1032,)], (8, 8))
    with pytest.raises(TypeError):
        pointnet.encode_grouped(np.zeros((2, 7, 64, 10), np.float32), prm, (8, 8))
    with pytest.raises(ValueError):
        pointnet.encode_grouped(torch.zeros(2, 7, 64, 9), prm, (8, 8))
    with pytest.raises(ValueError):
        pointnet.GroupedEncoder(10, (96, 100), (8, 8))


def test_module_keys_and_shapes_are_the_references(golden):
    from rrl_hip import pointnet
    net = pointnet.GroupedEncoder.rpm_feat_prepool()
    weights = GP.fixture_weights(golden, "rpm130")
    assert list(net.state_dict()) == golden["rpm130_keys"].tolist()
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == {k: v.shape for k, v in weights.items()}
    assert tuple(net.state_dict()["prepool.0.weight"].shape) == (96, 10, 1, 1) and tuple(net.state_dict()["prepool.7.bias"].shape) == (192,)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items()}, strict=True)
    assert all(np.array_equal(p.detach().numpy().reshape(q.shape), q) for p, q in zip(net.params(), GP.rpm_params(weights)))
    small = pointnet.GroupedEncoder.rpm_feat_prepool(raw_dim=10, feature_dim=32)
    assert small.widths == (32, 32, 64) and small.groups == (8, 8, 8)


def test_without_a_gpu_the_call_raises():
    if torch.cuda.is_available():
        return   # (with a GPU the call is served: tests/test_gpu_pointnet_group.py)
    from rrl_hip import pointnet
    from rrl_hip._lib import RRLError
    net = pointnet.GroupedEncoder.rpm_feat_prepool(10, 32)
    with pytest.raises(RRLError):
        net(torch.zeros(1, 3, 4, 10))
