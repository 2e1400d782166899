"""CPU-side checks of the second-order pose path (include/rrl.h rrl_pose_normal_eq, rrl_se3_newton_step_batch,
rrl_register_newton_epoch; rrl_hip/newton.py).

1. tests/newton_refs.py -- the float64 twin tests/test_gpu_newton.py holds the kernels to -- is tied to what existed before
   it: fed with the workspace fields of the float64 loss twin (tests/loss_refs.py, on the C oracle's scan), its gradient g
   equals the chain-rule image of that twin's dL/dR, dL/dT; H is symmetric positive semi-definite; the frozen-weight
   objective with the linearised residual IS F(0) + g delta + delta^T H delta / 2, and the linearisation is the derivative
   of Q1(delta); and the loss twin's own directional derivative along -H^-1 g is negative.
2. What the three entries refuse and with which code -- fake pointers, no GPU: every refusal happens on the host before the
   first launch, RRL_E_ARG before RRL_E_WS --, the header's status codes against the twin's, and the ValueErrors of NewtonRegistration that need no GPU.  tools/register_newton_refusals.cpp makes the same calls
   from a stand-alone program, which tools/refusals_sanitize.sh runs under AddressSanitizer + UBSan."""
import ctypes

import numpy as np
import pytest
import torch

import loss_refs
import newton_refs as NR
from conftest import load_golden

# (fixture, bucket range, pose of the source: rotation vector and translation)
CASES = [("loss_synth_s0.npz", (1, 1, 5, 5), (0.05, -0.02, 0.03), (0.02, 0.01, -0.015)),
         ("loss_synth_s1.npz", (1, 1, 5, 5), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)),
         ("loss_demo_scale.npz", (1, 1, 5, 5), (-0.1, 0.04, 0.02), (0.3, -0.2, 0.1)),
         ("loss_ref_airplane0.npz", (1, 2, 3, 5), (0.01, 0.02, -0.03), (0.0, 0.01, 0.0))]


def moved_case(oracle, name, rng, rot, trans):
    """The source of a golden fixture moved by (R, T) (y = x R + T), the loss twin on the oracle's scan of the moved clouds,
    its (dL/dR, dL/dT), and the workspace fields as the twin's float64 values."""
    g = load_golden(name)
    src, tar, lines = g["tri1"], g["tri2"], g["lines"]
    R = NR.rodrigues(np.array(rot)).T
    T = np.array(trans)
    moved = (src.reshape(-1, 3).astype(np.float64) @ R + T).astype(np.float32).reshape(-1, 9)
    s1, s2 = oracle.scan(moved, lines, cap=8), oracle.scan(tar, lines, cap=8)
    ref = loss_refs.post_scan_ref(moved, tar, s1, s2, rng)
    assert ref is not None, name
    gR, gt = loss_refs.rigid_grads_ref(src, R, T, ref["g1"], False)
    return dict(src=src, R=R, T=T, ref=ref, gR=gR, gt=gt, fields=NR.fields_from_ref(ref, len(lines)))


@pytest.fixture(scope="module")
def cases(oracle):
    return {c[0]: moved_case(oracle, *c) for c in CASES}


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_the_twins_gradient_is_the_chain_rule_image_of_the_loss_twins(cases, name):
    """g_v = dL/dT and g_w = vee(A - A^T) + T x dL/dT with A = R^T dL/dR, to 1e-9 of the sums of |terms| (float64 twice; the
    moved cloud is rounded to float32 before the scan, so y differs from x R + T by 2^-24 relative -- hence not 1e-12)."""
    c = cases[name]
    sums, abs_sums, n = NR.normal_sums(c["fields"], np.float64)
    assert n > 0
    gw, gv = NR.chain_rule_gradient(c["gR"], c["gt"], c["R"], c["T"])
    scale = abs_sums[10:16]
    assert np.all(scale > 0)
    np.testing.assert_array_less(np.abs(sums[13:16] - gv), 1e-9 * scale[3:] + 1e-300)
    # g_w from dL/dR goes through y = x R + T in float64, the twin's through the float32 moved points' q: 2^-22 of the terms
    np.testing.assert_array_less(np.abs(sums[10:13] - gw), 2.0 ** -22 * scale[:3])


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_h_is_symmetric_psd_and_is_the_hessian_of_the_frozen_problem(cases, name):
    """H = H^T, its smallest eigenvalue >= -1e-12 of the largest; the frozen-weight objective with the LINEARISED residual,
    sum a |e + omega x Q + s v|^2, equals F(0) + g delta + delta^T H delta / 2 exactly (1e-12: it is that quadratic -- Gauss-
    Newton drops the residual times the rotation's curvature, nothing else); and the linearisation itself is the derivative of
    Q1(delta) = Q Rot(omega)^T + s v (central difference, h = 1e-5)."""
    c = cases[name]
    sums, _, _ = NR.normal_sums(c["fields"], np.float64)
    H, g = NR.assemble(sums)
    assert np.array_equal(H, H.T)
    ev = np.linalg.eigvalsh(H)
    assert ev[0] >= -1e-12 * ev[-1] and ev[-1] > 0
    p = NR.selected_pairs(c["fields"], np.float64)
    a, Q, e, s = p["a"], p["Q"], p["e"], p["s"]

    def lin(d):
        return np.cross(d[:3], Q) + s[:, None] * d[3:]

    def F(d):
        r = e + lin(d)
        return float((a * (r * r).sum(1)).sum())
    rs = np.random.default_rng(3)
    for _ in range(8):
        d = rs.standard_normal(6)
        model = F(np.zeros(6)) + g @ d + 0.5 * d @ H @ d
        assert abs(F(d) - model) <= 1e-12 * (F(np.zeros(6)) + np.abs(g) @ np.abs(d) + 0.5 * np.abs(d) @ np.abs(H) @ np.abs(d))
        h = 1e-5
        qp = Q @ NR.rodrigues(h * d[:3]).T + s[:, None] * (h * d[3:])
        qm = Q @ NR.rodrigues(-h * d[:3]).T - s[:, None] * (h * d[3:])
        assert np.abs((qp - qm) / (2 * h) - lin(d)).max() <= 1e-8 * (1.0 + np.abs(Q).max()) * np.linalg.norm(d) ** 3


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_the_loss_decreases_along_the_newton_direction(cases, name):
    """The directional derivative of the LOSS twin (its chain-rule gradient, not the Newton twin's own g) along the damped
    step -(H + damping diag H + eps I)^-1 g is negative, for every damping of the sweep."""
    c = cases[name]
    sums, _, _ = NR.normal_sums(c["fields"], np.float64)
    H, g = NR.assemble(sums)
    gw, gv = NR.chain_rule_gradient(c["gR"], c["gt"], c["R"], c["T"])
    for damping in (0.0, 1e-3, 1e-2, 1e-1):
        x = NR.solve(H, g, damping, 1e-12)
        assert x is not None
        assert np.concatenate([gw, gv]) @ x < 0.0
        A = NR.damped(H, damping, 1e-12)
        assert np.linalg.norm(A @ x + g) <= 1e-10 * np.linalg.norm(A, 2) * np.linalg.norm(x)


def test_the_pose_step_of_the_twin():
    """Clamps, composition (rotation matrix out, the twist applied to a point), failure and the stopping rule."""
    rs = np.random.default_rng(5)
    R0, T0 = NR.rodrigues(rs.standard_normal(3)).T, rs.standard_normal(3)
    w, v, nw, nv = NR.clamp(np.array([3.0, 0, 0, 0, 4.0, 0]), 0.5, 0.2, 10.0)
    assert nw == 0.2 and abs(np.linalg.norm(w) - 0.2) < 1e-15 and nv == 2.0 and v[1] == 2.0
    Rn, Tn = NR.compose(R0, T0, w, v)
    assert np.abs(Rn @ Rn.T - np.eye(3)).max() < 1e-15 and abs(np.linalg.det(Rn) - 1) < 1e-14
    x = rs.standard_normal(3)
    y = x @ R0 + T0
    np.testing.assert_allclose(x @ Rn + Tn, y @ NR.rodrigues(w).T + v, atol=1e-14)
    zero = np.zeros(16)
    st = np.array([0, 0, -1, 0])
    args = dict(damping=1e-2, step_scale=1.0, max_rot=0.2, max_trans=0.1, tol_rot=1e-3, tol_trans=1e-3, patience=2, eps=1e-12)
    assert NR.step(zero, 1, R0, T0, st, **args)[2].tolist() == [1, 0, -1, NR.FAILED]
    assert NR.step(zero, 0, R0, T0, st, **args)[2].tolist() == [1, 0, -1, NR.GATED]
    nan = zero.copy(); nan[4] = np.nan
    assert NR.step(nan, 1, R0, T0, st, **args)[2][3] == NR.FAILED
    # a well-posed system whose step is tiny: calm twice -> done at epoch 2, frozen afterwards
    neq = np.array([2.0, 0, 0, 3.0, 0, 4.0, 0, 0, 0, 1.0, 1e-6, 0, 0, 0, 1e-6, 0])
    Rn, Tn, st1, x1, ls = NR.step(neq, 5, R0, T0, st, **args)
    assert st1.tolist() == [1, 1, -1, NR.STEPPED] and ls[0] < 1e-3
    Rn, Tn, st2, _, _ = NR.step(neq, 5, Rn, Tn, st1, **args)
    assert st2.tolist() == [2, 2, 2, NR.STEPPED]
    R3, T3, st3, _, _ = NR.step(neq, 5, Rn, Tn, st2, **args)
    assert st3.tolist() == [3, 2, 2, NR.DONE] and np.array_equal(R3, Rn) and np.array_equal(T3, Tn)


# ------------------------------------------------------------------------------------------------- the refusals
FAKE = ctypes.c_void_p(256)
BIG = 1 << 50
E_ARG, E_WS = -1, -3
CAP1 = "sort capacity + 1"

NEQ_ARGS = ("ws", "ws_bytes", "B", "N", "M", "L", "s_m", "s_n", "e_m", "e_n", "neq", "part", "part_bytes", "opts")
NEQ_BASE = dict(ws=FAKE, ws_bytes=BIG, B=3, N=300, M=300, L=2048, s_m=1, s_n=1, e_m=5, e_n=5, neq=FAKE, part=FAKE, part_bytes=BIG,
                opts=None)
NEQ = [
    ("null workspace", dict(ws=None), E_ARG),
    ("null output", dict(neq=None), E_ARG),
    ("null scratch", dict(part=None), E_ARG),
    ("misaligned scratch", dict(part=ctypes.c_void_p(260)), E_ARG),
    ("empty batch", dict(B=0), E_ARG),
    ("negative batch", dict(B=-1), E_ARG),
    ("a batch beyond the grid", dict(B=65536), E_ARG),
    ("empty source", dict(N=0), E_ARG),
    ("empty target", dict(M=0), E_ARG),
    ("no lines", dict(L=0), E_ARG),
    ("L = 2^24", dict(L=1 << 24), E_ARG),
    ("a wide range (rows)", dict(e_m=9), E_ARG),
    ("a wide range (columns)", dict(e_n=6), E_ARG),
    ("a range from 0", dict(s_n=0), E_ARG),
    ("an empty range", dict(s_m=3, e_m=3), E_ARG),
    ("multi-pose", dict(B=4, opts=dict(problems=2)), E_ARG),
    ("problems = B is one pose per problem", dict(B=4, opts=dict(problems=4), ws_bytes=0), E_WS),
    ("short workspace", dict(ws_bytes=4096), E_WS),
    ("short scratch", dict(part_bytes=3 * 32 * 16 * 8 - 8), E_WS),
    ("the scratch to the byte", dict(part_bytes=3 * 32 * 16 * 8, ws_bytes=0), E_WS),
    ("a wide range + short workspace", dict(e_m=9, ws_bytes=0), E_ARG),
    ("multi-pose + short scratch", dict(B=4, opts=dict(problems=2), part_bytes=0), E_ARG),
    ("null pointer + short workspace", dict(neq=None, ws_bytes=0), E_ARG),
]

STEP_ARGS = ("neq", "gate", "gate_stride", "damping", "step", "max_rot", "max_trans", "tol_rot", "tol_trans", "patience", "eps", "R",
             "T", "loss", "value", "table", "cursor", "nrows", "row", "aabb_rows", "row_stride", "count1", "N", "box", "delta",
             "last_step", "state", "B")
STEP_BASE = dict({k: FAKE for k in STEP_ARGS}, gate_stride=4, patience=3, eps=1e-12, nrows=16, row_stride=16, N=300, B=3)
STEP = [
    ("null pointer (neq)", dict(neq=None), E_ARG),
    ("null pointer (damping)", dict(damping=None), E_ARG),
    ("null pointer (step)", dict(step=None), E_ARG),
    ("null pointer (max_rot)", dict(max_rot=None), E_ARG),
    ("null pointer (max_trans)", dict(max_trans=None), E_ARG),
    ("null pointer (R)", dict(R=None), E_ARG),
    ("null pointer (T)", dict(T=None), E_ARG),
    ("null pointer (state)", dict(state=None), E_ARG),
    ("negative batch", dict(B=-1), E_ARG),
    ("negative gate stride", dict(gate_stride=-4), E_ARG),
    ("negative eps", dict(eps=-1e-12), E_ARG),
    ("NaN eps", dict(eps=float("nan")), E_ARG),
    ("a stopping rule without its tolerances", dict(tol_rot=None), E_ARG),
    ("a stopping rule without its translation tolerance", dict(tol_trans=None), E_ARG),
    ("a box without rows", dict(aabb_rows=None), E_ARG),
    ("a box over no capacity", dict(N=0), E_ARG),
    ("a box whose samples' rows overlap", dict(row_stride=8), E_ARG),
    ("negative batch + null pointer", dict(B=-1, T=None), E_ARG),
    ("an empty batch + a box without rows", dict(B=0, aabb_rows=None), E_ARG),
    ("an empty batch is valid: no launch", dict(B=0), 0),
    ("an empty batch without the optional pointers", dict(B=0, gate=None, tol_rot=None, tol_trans=None, patience=0, loss=None,
                                                          value=None, table=None, cursor=None, row=None, aabb_rows=None,
                                                          count1=None, box=None, delta=None, last_step=None), 0),
]

EPOCH_INTS = dict(B=3, N=300, M=300, L=2048, rounds=10, patience=3, ws_bytes=BIG, cham_ws_bytes=BIG, part_bytes=BIG, table_rows=16)
NO_MONITOR = dict(value=None)
RAGGED = dict(count1=512, count2=512)
EPOCH = [
    ("null struct", dict(args=None), E_ARG),
    ("a struct too short", dict(struct_bytes=64), E_ARG),
    ("a struct one field short", dict(struct_bytes="sizeof - 8"), E_ARG),
    ("empty batch", dict(B=0), E_ARG),
    ("negative batch", dict(B=-1), E_ARG),
    ("a batch beyond the grid", dict(B=65536, **NO_MONITOR), E_ARG),
    ("negative size", dict(N=-1), E_ARG),
    ("empty target", dict(M=0), E_ARG),
    ("no lines", dict(L=0), E_ARG),
    ("no sampler rounds", dict(rounds=0), E_ARG),
    ("a sampler without its radius", dict(radius=None), E_ARG),
    ("a sampler without its target box", dict(box2=None), E_ARG),
    ("a sampler whose ballots are misaligned", dict(tile_counts=260), E_ARG),
    ("multi-pose", dict(B=4, opts=dict(problems=2)), E_ARG),
    ("line counts: the sampler owns the line set", dict(opts=dict(nlines=512)), E_ARG),
    ("the monitor on a ragged batch", dict(opts=RAGGED), E_ARG),
    ("the monitor on a ragged source alone", dict(opts=dict(count1=512)), E_ARG),
    ("the monitor without its scratch", dict(cham_ws=None), E_ARG),
    ("the monitor without its pooled mean", dict(cham_mean=None), E_ARG),
    ("the monitor beyond the sort capacity", dict(N=CAP1), E_ARG),
    ("null pointer (neq)", dict(neq=None), E_ARG),
    ("null pointer (part)", dict(part=None), E_ARG),
    ("null pointer (state)", dict(state=None), E_ARG),
    ("null pointer (damping)", dict(damping=None), E_ARG),
    ("null pointer (max_trans)", dict(max_trans=None), E_ARG),
    ("null pointer (box1)", dict(box1=None), E_ARG),
    ("negative eps", dict(eps=-1.0), E_ARG),
    ("a stopping rule without its tolerances", dict(tol_rot=None), E_ARG),
    ("null pointer of the forward (src_tri)", dict(src_tri=None), E_ARG),
    ("null pointer of the forward (lines)", dict(lines=None), E_ARG),
    ("null pointer of the forward (loss)", dict(loss=None), E_ARG),
    ("null pointer of the forward (ws)", dict(ws=None), E_ARG),
    ("the forward's refusal: ragged beyond the sort capacity", dict(N=CAP1, opts=RAGGED, **NO_MONITOR), E_ARG),
    ("the forward's refusal: L = 2^24", dict(L=1 << 24, **NO_MONITOR), E_ARG),
    ("short workspace", dict(ws_bytes=4096), E_WS),
    ("short workspace, ragged, no monitor", dict(ws_bytes=0, opts=RAGGED, **NO_MONITOR), E_WS),
    ("short Chamfer workspace", dict(cham_ws_bytes=64), E_WS),
    ("short scratch of the normal equations", dict(part_bytes=64), E_WS),
    ("given lines need no rounds", dict(rng_state=None, rounds=0, radius=None, box2=None, ws_bytes=0), E_WS),
    ("no stopping rule needs no tolerances", dict(patience=0, tol_rot=None, tol_trans=None, ws_bytes=0), E_WS),
    # the chain flags are dropped, not refused: the call gets as far as the workspace check
    ("chain flags are dropped", dict(opts=dict(flags=2 | 4), ws_bytes=0), E_WS),
    # invalid in two ways: RRL_E_ARG before RRL_E_WS
    ("multi-pose + short workspace", dict(B=4, opts=dict(problems=2), ws_bytes=0), E_ARG),
    ("the monitor on a ragged batch + short workspace", dict(opts=RAGGED, ws_bytes=0), E_ARG),
    ("null pointer + short workspace", dict(state=None, ws_bytes=0), E_ARG),
    ("no sampler rounds + short Chamfer workspace", dict(rounds=0, cham_ws_bytes=0), E_ARG),
    ("the forward's null pointer + short scratch", dict(tar_tri=None, part_bytes=0), E_ARG),
    ("line counts + short workspace", dict(opts=dict(nlines=512), ws_bytes=0), E_ARG),
    ("short struct + everything else", dict(struct_bytes=8, B=-1, ws_bytes=0), E_ARG),
]


@pytest.fixture(scope="module")
def lib():
    from rrl_hip import _lib, build
    build.build_lib()
    return _lib.load()


def call_neq(lib, over):
    from rrl_hip import _lib
    v = dict(NEQ_BASE, **over)
    opts = _lib.Opts(**v["opts"]) if v["opts"] is not None else None
    v["opts"] = ctypes.addressof(opts) if opts is not None else None
    return lib.rrl_pose_normal_eq(*[v[k] for k in NEQ_ARGS], None)


def call_step(lib, over):
    v = dict(STEP_BASE, **over)
    return lib.rrl_se3_newton_step_batch(*[v[k] for k in STEP_ARGS], None)


def call_epoch(lib, over):
    from rrl_hip import _lib
    over = dict(over)
    if "args" in over:
        return lib.rrl_register_newton_epoch(None, None)
    cap1 = lib.rrl_sort_capacity() + 1
    a = _lib.RegisterNewtonArgs()
    for name, kind in _lib.RegisterNewtonArgs._fields_:
        if kind is ctypes.c_void_p and name != "opts":
            setattr(a, name, 256)
    a.struct_bytes = ctypes.sizeof(_lib.RegisterNewtonArgs)
    a.eps = 1e-12
    for k, v in EPOCH_INTS.items():
        setattr(a, k, v)
    opts = _lib.Opts(**over.pop("opts")) if "opts" in over else None
    if opts is not None:
        a.opts = ctypes.addressof(opts)
    for k, v in over.items():
        if v == "sizeof - 8":
            v = ctypes.sizeof(_lib.RegisterNewtonArgs) - 8
        setattr(a, k, cap1 if v is CAP1 else v)
    return lib.rrl_register_newton_epoch(ctypes.byref(a), None)


def test_the_tables_cover_the_documented_codes(lib):
    for table in (NEQ, STEP, EPOCH):
        assert len({r[0] for r in table}) == len(table)
    assert {r[2] for r in NEQ} == {E_ARG, E_WS} and {r[2] for r in STEP} == {E_ARG, 0} and {r[2] for r in EPOCH} == {E_ARG, E_WS}
    assert sum(" + " in r[0] for r in EPOCH) >= 6 and sum(" + " in r[0] for r in NEQ) >= 3
    assert lib.rrl_pose_normal_eq_part_bytes(3, 2048) == 3 * 32 * 16 * 8 and lib.rrl_pose_normal_eq_part_bytes(1, 1) == 16 * 16 * 8
    assert lib.rrl_pose_normal_eq_part_bytes(0, 5) == 0 and lib.rrl_pose_normal_eq_part_bytes(2, -1) == 0


@pytest.mark.parametrize("row", NEQ, ids=lambda r: r[0])
def test_the_normal_equations_refuse_before_any_launch(lib, row):
    _, over, code = row
    assert call_neq(lib, over) == code


@pytest.mark.parametrize("row", STEP, ids=lambda r: r[0])
def test_the_newton_step_refuses_before_any_launch(lib, row):
    _, over, code = row
    assert call_step(lib, over) == code


@pytest.mark.parametrize("row", EPOCH, ids=lambda r: r[0])
def test_the_newton_epoch_refuses_before_its_first_launch(lib, row):
    _, over, code = row
    assert call_epoch(lib, over) == code


def test_the_twin_uses_the_headers_codes():
    """The status codes and the number of sums as the header defines them (each against gcc's value, and the layout of
    rrl_register_newton_args: tests/test_abi_host.py) are the float64 twin's."""
    from rrl_hip import _abi, _lib
    assert _abi.CONSTANTS["RRL_NEQ_SUMS"] == NR.NSUMS
    assert (NR.STEPPED, NR.GATED, NR.FAILED, NR.DONE) == (_lib.NEWTON_STEPPED, _lib.NEWTON_GATED, _lib.NEWTON_FAILED, _lib.NEWTON_DONE)


def test_newton_registration_refuses_without_a_gpu(lib):
    """The constructor's own ValueErrors, and PairRegistration's (shared by import), before anything touches a GPU."""
    from rrl_hip import newton, ops, register
    assert issubclass(newton.NewtonRegistration, register.PairRegistration)
    tri = torch.zeros(2, 64, 9)
    with pytest.raises(ValueError, match="R0 and T0 together"):
        newton.NewtonRegistration(tri, tri, 2048, R0=torch.eye(3).expand(2, 3, 3))
    with pytest.raises(ValueError, match="R0 and T0 together"):
        newton.NewtonRegistration(tri, tri, 2048, R0=torch.eye(3).expand(2, 3, 3), T0=torch.zeros(2, 3), xi0=torch.zeros(2, 6))
    with pytest.raises(ValueError, match="non-negative"):
        newton.NewtonRegistration(tri, tri, 2048, patience=-1)
    with pytest.raises(ValueError, match=r"ops\.chamfer\(.*counts_x=.*per_sample=True"):
        newton.NewtonRegistration(tri, tri, 2048, counts1=[64, 30], counts2=[64, 64], monitor=True)
    big = torch.zeros(1, 1, 9).expand(1, ops.sort_capacity() + 1, 9)  # (no memory behind it)
    with pytest.raises(ValueError, match=r"sort_capacity"):
        newton.register_pairs_newton(tri[:1], big, 2048, n_epoch=1)
    with pytest.raises(ValueError, match="same B"):
        newton.NewtonRegistration(tri, tri[:1], 2048)
