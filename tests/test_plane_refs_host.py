"""The host twins of the point-to-plane entries (tests/plane_refs.py) against exact cases, numpy's eigen-decomposition and a
float64 autograd Gauss-Newton; the float64 restatement of both ICP loops on the pairs the GPU test uses; the new entries and
structs in the header and the binding; and every refusal that needs no GPU (fake pointers: nothing is launched)."""
import ctypes

import numpy as np
import pytest
import torch

import plane_refs as PR

FAKE = 0x1000  # a non-NULL, 8-aligned pointer that is never dereferenced
E_ARG, E_WS = -1, -3


# ---- rule 1 -----------------------------------------------------------------------------------------------------------------
def lattice(nx, ny, step=0.125):
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij"), -1).reshape(-1, 2) * step
    return np.concatenate([g, np.zeros((len(g), 1))], 1).astype(np.float32)


def test_lattice_normals_are_exact_and_a_line_has_none():
    x = lattice(6, 5)[None]
    t = PR.estimate_normals(x, 0.3, 16)
    assert (t["found"] >= 3).all() and np.array_equal(t["normals"], np.broadcast_to([0.0, 0.0, 1.0], t["normals"].shape))
    assert (t["quality"] > 0.1).all()
    line = (np.arange(12)[:, None] * np.array([[0.25, 0.0, 0.0]])).astype(np.float32)[None]
    tl = PR.estimate_normals(line, 0.6, 8)
    assert (tl["found"] >= 3).all() and not tl["normals"].any() and not tl["quality"].any()
    skew = (np.linspace(-1, 1, 12)[:, None] * np.array([[1.0, 2.0, -0.5]]) + 0.3).astype(np.float32)[None]  # collinear up to rounding
    assert not PR.estimate_normals(skew, 1.0, 8)["normals"].any()
    # fewer than three members, duplicated points (coincident members), a NaN member: zero rows
    few = PR.estimate_normals(x, 0.13, 2)
    assert not few["normals"].any()
    dup = np.repeat(x[:, :1], 5, 1)
    assert not PR.estimate_normals(dup, 0.5, 8)["normals"].any()
    bad = x.copy()
    bad[0, 7, 1] = np.nan
    tb = PR.estimate_normals(bad, 0.3, 16)
    assert not tb["normals"][0, 7].any() and tb["normals"][0, 0].tolist() == [0.0, 0.0, 1.0]
    # dropped slots: an index at or beyond the count, or negative, is no member
    idx = np.array([[[0, 1, 6, 99, -1, 7]]], np.int32)
    got = PR.idx_normals(x, idx, np.array([[6]], np.int32), counts=[30])
    assert got["normals"][0, 0].tolist() == [0.0, 0.0, 1.0]
    assert not PR.idx_normals(x, idx, np.array([[6]], np.int32), counts=[2])["normals"].any()


def test_jacobi_against_numpy_and_the_sign_rule():
    from rrl_hip import synth
    x = synth.surface_cloud(3, 130)[None]
    t = PR.estimate_normals(x, 0.5, 64)
    worst = 0.0
    for i in range(130):
        mem = t["idx"][0, i, :t["found"][0, i]]
        C = PR.scatter(x[0, mem].astype(np.float64))
        lam, V = np.linalg.eigh(C)
        n, q, l = PR.normal_of(C)
        assert n.any() and abs(np.linalg.norm(n) - 1.0) < 1e-14
        assert np.abs(np.array(l) - lam).max() <= 1e-13 * lam[2] and abs(q - (lam[1] - lam[0]) / lam[2]) < 1e-12
        worst = max(worst, min(np.abs(n - V[:, 0]).max(), np.abs(n + V[:, 0]).max()) * q)
        big = np.argmax(np.abs(n) >= np.abs(n).max())
        assert n[big] > 0.0
    assert worst < 1e-13  # (the eigenvector's error grows with 1 / quality)
    assert np.array_equal(t["normals"][0, 5], PR.idx_normals(x, t["idx"], t["found"])["normals"][0, 5])


# ---- rules 2 and 3 ------------------------------------------------------------------------------------------------------------
def moved_pose(w, v, y, c):
    """c + Rot(w)(y - c) + v on rows, differentiable (Rodrigues through the matrix exponential)."""
    K = torch.zeros(3, 3, dtype=torch.float64)
    K[0, 1], K[0, 2], K[1, 0], K[1, 2], K[2, 0], K[2, 1] = -w[2], w[1], w[2], -w[0], -w[1], w[0]
    return (y - c) @ torch.linalg.matrix_exp(K).T + c + v


def test_sums_are_the_gauss_newton_of_the_plane_residual():
    rs = np.random.default_rng(11)
    n, m = 40, 37
    y = rs.uniform(-1, 1, (n, 3)).astype(np.float32)
    tar = rs.uniform(-1, 1, (m, 9)).astype(np.float32)
    nrm = rs.standard_normal((m, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    nrm[3] = 0.0
    nrm[5, 1] = np.nan
    w = rs.uniform(0.1, 1.0, n).astype(np.float32)
    idx = rs.integers(0, m, n).astype(np.uint64)
    dist = rs.uniform(0, 1, n).astype(np.float32)
    keys = (dist.view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx
    keys[4] = np.uint64(PR.ALL_ONES)
    keys[9] = (keys[9] & ~np.uint64(0xFFFFFFFF)) | np.uint64(m + 2)
    pivot = np.array([0.3, -0.2, 0.1], np.float32)
    t = PR.normal_eq(y, tar, nrm, keys, count1=36, count2=30, w=w, gate_sq=0.8, pivot=pivot)
    rows = [i for i in range(36) if i not in (4, 9) and int(idx[i]) < 30 and dist[i] <= np.float32(0.8) and int(idx[i]) not in (3, 5)]
    skipped = 4 + sum(1 for i in range(36) if i in (4, 9) or int(idx[i]) >= 30)
    assert t["info"] == [len(rows), PR.FIT_OK, 0, skipped] and t["neq"][PR.USED] == len(rows) and t["neq"][PR.SKIPPED] == skipped
    cols = idx[rows].astype(np.int64)
    Y, Bt, Nn = (torch.tensor(a.astype(np.float64)) for a in (y[rows], tar[cols, :3], nrm[cols]))
    Wt, c = torch.tensor(w[rows].astype(np.float64)), torch.tensor(pivot.astype(np.float64))

    def residuals(x):
        return ((moved_pose(x[:3], x[3:], Y, c) - Bt) * Nn).sum(1)
    x0 = torch.zeros(6, dtype=torch.float64)
    J = torch.autograd.functional.jacobian(residuals, x0)
    r = residuals(x0)
    H = (J.T * Wt) @ J / Wt.sum()
    g = (J.T * Wt) @ r / Wt.sum()
    assert np.abs(t["H"] - H.numpy()).max() <= 1e-13 and np.abs(t["g"] - g.numpy()).max() <= 1e-13
    assert abs(t["neq"][PR.RES] - float((Wt * r * r).sum() / Wt.sum())) <= 1e-14
    assert abs(t["neq"][PR.KEYMEAN] - float((w[rows].astype(np.float64) * dist[rows]).sum() / w[rows].astype(np.float64).sum())) <= 1e-14
    assert abs(t["neq"][PR.W_] - float(Wt.sum())) <= 1e-13
    # the solved step lowers the linearised cost to its minimum: the gradient of 1/2 sum w (r + J x)^2 vanishes (no damping)
    x = PR.solve(t["H"], t["g"], 0.0, 0.0)
    assert np.abs(t["H"] @ x + t["g"]).max() <= 1e-12
    # fewer than six pairs, or no weight: RRL_FIT_FEW with zero sums; dense pairs need no keys
    few = PR.normal_eq(y[:5], tar[:5], nrm[10:15], pivot=pivot)
    assert few["info"] == [5, PR.FIT_FEW, 0, 0] and not few["neq"][:PR.W_].any() and few["neq"][PR.W_] == 5.0
    assert PR.normal_eq(y[:8], tar[:8], nrm[10:18], w=np.zeros(8, np.float32))["info"][:2] == [8, PR.FIT_FEW]


def test_step_rule():
    rs = np.random.default_rng(2)
    y = rs.uniform(-1, 1, (50, 3)).astype(np.float32)
    nrm = rs.standard_normal((50, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    tar = (y + 0.01 * rs.standard_normal((50, 3))).astype(np.float32)
    t = PR.normal_eq(y, tar, nrm)
    R0, T0 = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    R, T, last, st = PR.step(t["neq"], t["info"], R0, T0, [0, 0, -1, 0], damping=0.0, tol_rot=1.0, tol_trans=1.0, patience=2)
    assert st == [1, 1, -1, PR.STEPPED] and np.abs(R.T @ R - np.eye(3)).max() < 1e-15 and last[0] > 0
    R2, T2, _, st2 = PR.step(t["neq"], t["info"], R, T, st, damping=0.0, tol_rot=1.0, tol_trans=1.0, patience=2)
    assert st2 == [2, 2, 2, PR.STEPPED]
    R3, T3, last3, st3 = PR.step(t["neq"], t["info"], R2, T2, st2, patience=2)
    assert st3 == [3, 2, 2, PR.DONE] and last3 is None and np.array_equal(R3, R2.astype(np.float32).astype(np.float64))
    # the clamps: a clamped length IS the clamp
    _, _, lc, _ = PR.step(t["neq"], t["info"], R0, T0, [0, 0, -1, 0], max_rot=1e-4, max_trans=1e-5)
    assert lc == (float(np.float32(1e-4)), float(np.float32(1e-5)))
    # all normals equal: H is singular, the pose is kept; fewer than six pairs: kept as well
    flat = PR.normal_eq(y, tar, np.broadcast_to(np.array([0, 0, 1], np.float32), (50, 3)))
    assert PR.step(flat["neq"], flat["info"], R0, T0, [0, 0, -1, 0])[3] == [1, 0, -1, PR.FAILED]
    few = PR.normal_eq(y[:4], tar[:4], nrm[:4])
    assert PR.step(few["neq"], few["info"], R0, T0, [4, 1, -1, 0])[3] == [5, 0, -1, PR.FEW]
    # the pivot reparametrises the same linear problem (v' = v - omega x c): the undamped step has the same rotation, and its
    # translation differs only by the second-order term of Rot(omega) c, below |omega|^2 |c|
    c = np.array([0.4, 0.1, -0.3], np.float32)
    far = PR.normal_eq(y, tar, nrm, pivot=c)
    Rp, Tp, lp, _ = PR.step(far["neq"], far["info"], R0, T0, [0, 0, -1, 0], pivot=c, damping=0.0)
    Ro, To, _, _ = PR.step(t["neq"], t["info"], R0, T0, [0, 0, -1, 0], damping=0.0)
    assert np.abs(Rp - Ro).max() < 1e-12 and np.abs(Tp - To).max() <= lp[0] ** 2 * np.linalg.norm(c)


# ---- the loops: what the GPU test's inputs give in float64 ---------------------------------------------------------------------
PAIR_SEEDS = range(40, 48)
PAIR_N, PAIR_RADIUS = 256, 0.4


def test_plane_loop_beats_point_loop_on_the_table_pairs():
    """Eight make_pair pairs at 20 degrees, N = M = 256, ball-PCA normals of radius 0.4: after 10 epochs point-to-plane is below
    point-to-point's 30-epoch rotation error on all eight."""
    for s in PAIR_SEEDS:
        pr, Rt = PR.pair_with_rotation(s, PAIR_N, PAIR_N)
        nrm = PR.estimate_normals(pr["tar"][None], PAIR_RADIUS, 64)["normals"][0].astype(np.float32)
        assert nrm.any(1).all()
        Rp, _ = PR.plane_loop(pr["src"], pr["tar"], nrm, 10)
        Rq, _ = PR.point_loop(pr["src"], pr["tar"], 30)
        ep, eq = PR.rotation_error_deg(Rp, Rt), PR.rotation_error_deg(Rq, Rt)
        print(f"seed {s}: plane after 10 epochs {ep:.3f} deg, point after 30 epochs {eq:.3f} deg")
        assert ep < eq and 0.1 < ep < 3.6 and 3.3 < eq < 14.0, (s, ep, eq)


def test_exact_pairs_converge_in_the_float32_pose_restatement():
    from rrl_hip import synth
    for n, radius in ((65, 0.7), (130, 0.5), (257, 0.4)):
        tar = synth.surface_cloud(100, n)
        Rg = synth._rotation(np.random.default_rng(7).standard_normal(3), 10.0).T
        src = ((tar.astype(np.float64) - np.array([0.05, -0.03, 0.02])) @ Rg.T).astype(np.float32)
        nrm = PR.estimate_normals(tar[None], radius, 64)["normals"][0].astype(np.float32)
        R, T = PR.plane_loop(src, tar, nrm, 6, round_pose=True)
        err = np.abs(src.astype(np.float64) @ R + T - tar).max() / (2.0 ** -23 * np.abs(tar).max())
        print(f"n = {n}: {err:.2f} x 2^-23 max|coordinate| after 6 epochs")
        assert err <= 1.2


# ---- the C entries: every refusal on the host, before anything is launched -----------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from rrl_hip import _lib, build
    build.build_lib()
    return _lib.load()


def normals_call(lib, **over):
    a = dict(pts=FAKE, stride=3, idx=FAKE, found=FAKE, counts=None, nsample=64, rank_tol=1e-10, normals=FAKE, quality=None, B=2, n=130, S=130)
    a.update(over)
    return lib.rrl_idx_normals(a["pts"], a["stride"], a["idx"], a["found"], a["counts"], a["nsample"], a["rank_tol"], a["normals"],
                               a["quality"], a["B"], a["n"], a["S"], None)


NORMALS_REFUSALS = [dict(pts=None), dict(idx=None), dict(found=None), dict(normals=None), dict(B=0), dict(B=-1), dict(B=32768), dict(n=0),
                    dict(n=(1 << 20) + 1), dict(S=-1), dict(stride=2), dict(nsample=0), dict(nsample=65), dict(rank_tol=-1e-9),
                    dict(rank_tol=float("nan")), dict(rank_tol=1.0)]


def plane_args(lib, **over):
    from rrl_hip import _lib
    k = _lib.PlaneArgs()
    base = dict(struct_bytes=ctypes.sizeof(k), B=2, N=1000, M=1000, tar_stride=3, moved=FAKE, keys=None, tar=FAKE, normals=FAKE, count1=None,
                count2=None, w=None, gate_sq=None, pivot=None, part=FAKE, part_bytes=int(lib.rrl_plane_part_bytes(2, 1000)), neq=FAKE, info=FAKE)
    base.update(over)
    for name, v in base.items():
        setattr(k, name, v)
    return k


PLANE_REFUSALS = [dict(moved=None), dict(tar=None), dict(normals=None), dict(neq=None), dict(info=None), dict(part=None), dict(B=-1),
                  dict(B=32768), dict(N=0), dict(M=0), dict(tar_stride=2), dict(M=999), dict(gate_sq=FAKE), dict(struct_bytes=8),
                  dict(part=FAKE + 4), dict(neq=FAKE + 4)]

STEP_DEFAULTS = (("neq", FAKE), ("info", FAKE), ("pivot", None), ("damping", FAKE), ("step", FAKE), ("max_rot", FAKE), ("max_trans", FAKE),
                 ("tol_rot", FAKE), ("tol_trans", FAKE), ("patience", 3), ("eps", 1e-12), ("R", FAKE), ("T", FAKE), ("value", None),
                 ("table", None), ("cursor", None), ("nrows", 0), ("row", None), ("last_step", None), ("state", FAKE), ("B", 2))
STEP_REFUSALS = [dict(neq=None), dict(info=None), dict(damping=None), dict(step=None), dict(max_rot=None), dict(max_trans=None), dict(R=None),
                 dict(T=None), dict(state=None), dict(B=-1), dict(tol_rot=None), dict(tol_trans=None), dict(eps=-1.0), dict(eps=float("nan")),
                 dict(neq=FAKE + 4)]


def step_call(lib, **over):
    return lib.rrl_plane_step_batch(*[over.get(k, d) for k, d in STEP_DEFAULTS], None)


def epoch_args(lib, **over):
    from rrl_hip import _lib
    a = _lib.PlaneEpochArgs()
    base = dict(struct_bytes=ctypes.sizeof(a), B=2, N=1000, M=900, patience=3, src=FAKE, tar=FAKE, normals=FAKE, count1=None, count2=None,
                R=FAKE, T=FAKE, moved=FAKE, cham_ws=FAKE, cham_ws_bytes=int(lib.rrl_chamfer_workspace_bytes(2, 1000, 900)), best_x=FAKE,
                best_y=FAKE, values=FAKE, order_x=None, order_y=None, w=None, gate_sq=None, pivot=None, part=FAKE,
                part_bytes=int(lib.rrl_plane_part_bytes(2, 1000)), neq=FAKE, info=FAKE, damping=FAKE, step=FAKE, max_rot=FAKE,
                max_trans=FAKE, tol_rot=FAKE, tol_trans=FAKE, eps=1e-12, last_step=None, state=FAKE, table=None, cursor=None,
                table_rows=0, row=None)
    base.update(over)
    for name, v in base.items():
        setattr(a, name, v)
    return a


def test_c_refusals_return_their_codes_without_a_launch(lib):
    for over in NORMALS_REFUSALS:
        assert normals_call(lib, **over) == E_ARG, over
    assert normals_call(lib, S=0) == 0  # no rows: no launch
    assert lib.rrl_plane_normal_eq(None, None) == E_ARG
    for over in PLANE_REFUSALS:
        assert lib.rrl_plane_normal_eq(ctypes.byref(plane_args(lib, **over)), None) == E_ARG, over
    assert lib.rrl_plane_normal_eq(ctypes.byref(plane_args(lib, part_bytes=int(lib.rrl_plane_part_bytes(2, 1000)) - 1)), None) == E_WS
    assert lib.rrl_plane_normal_eq(ctypes.byref(plane_args(lib, keys=FAKE, M=77, part_bytes=0)), None) == E_WS  # (keys: M is free)
    assert lib.rrl_plane_normal_eq(ctypes.byref(plane_args(lib, B=0, part_bytes=0)), None) == 0  # no sample: no launch
    assert lib.rrl_plane_part_bytes(0, 5) == 0 and lib.rrl_plane_part_bytes(3, 513) == 8 * 32 * 3 * 2
    for over in STEP_REFUSALS:
        assert step_call(lib, **over) == E_ARG, over
    assert step_call(lib, B=0) == 0 and step_call(lib, B=0, patience=0, tol_rot=None, tol_trans=None) == 0


def test_plane_epoch_refuses_before_its_first_launch(lib):
    assert lib.rrl_plane_icp_epoch(None, None) == E_ARG
    refusals = [dict(struct_bytes=16), dict(B=0), dict(B=32768), dict(N=0), dict(M=0), dict(N=lib.rrl_sort_capacity() + 1),
                dict(count1=FAKE), dict(count2=FAKE), dict(order_x=FAKE), dict(order_y=FAKE), dict(tol_rot=None), dict(part=FAKE + 4),
                dict(neq=FAKE + 4), dict(eps=-1.0), dict(eps=float("nan"))]
    refusals += [{k: None} for k in ("src", "tar", "normals", "R", "T", "moved", "cham_ws", "best_x", "best_y", "values", "part", "neq",
                                     "info", "damping", "step", "max_rot", "max_trans", "state")]
    for over in refusals:
        assert lib.rrl_plane_icp_epoch(ctypes.byref(epoch_args(lib, **over)), None) == E_ARG, over
    assert lib.rrl_plane_icp_epoch(ctypes.byref(epoch_args(lib, cham_ws_bytes=64)), None) == E_WS
    assert lib.rrl_plane_icp_epoch(ctypes.byref(epoch_args(lib, part_bytes=8)), None) == E_WS
    assert lib.rrl_plane_icp_epoch(ctypes.byref(epoch_args(lib, part_bytes=8, state=None)), None) == E_ARG  # RRL_E_ARG before RRL_E_WS


def test_entries_and_structs_in_the_header_and_the_binding(lib):
    from rrl_hip import _abi, _lib, build, icp, neighbors
    assert "rrl_plane.hip" in build.SOURCES and "-ffp-contract=off" in build.FLAGS
    names = ("H", "G", "W", "RES", "KEYMEAN", "USED", "SKIPPED", "DOUBLES")
    got = {k: _abi.CONSTANTS["RRL_PLANE_" + k] for k in names + ("STEPPED", "FEW", "FAILED", "DONE")}  # (against gcc: test_abi_host.py)
    assert [got[k] for k in names] == [getattr(_lib, "PLANE_" + k) for k in names] == [PR.H0, PR.G0, PR.W_, PR.RES, PR.KEYMEAN, PR.USED, PR.SKIPPED, PR.DOUBLES]
    assert [got[k] for k in ("STEPPED", "FEW", "FAILED", "DONE")] == [_lib.PLANE_STEPPED, _lib.PLANE_FEW, _lib.PLANE_FAILED, _lib.PLANE_DONE] == [PR.STEPPED, PR.FEW, PR.FAILED, PR.DONE]
    assert callable(neighbors.estimate_normals) and callable(icp.plane_icp_pairs) and issubclass(icp.PlaneIcpRegistration, icp.StoppingLoop)
    assert float(np.float32(neighbors.NORMAL_RANK_TOL)) == PR.RANK_TOL
    from rrl_hip import newton
    import inspect
    sig = inspect.signature(icp.PlaneIcpRegistration.__init__).parameters
    assert [sig[k].default for k in ("damping", "step", "max_rot", "max_trans", "eps")] == [newton.DAMPING, newton.STEP, newton.MAX_ROT, newton.MAX_TRANS, newton.EPS]
    assert sig["normals"].default is None and sig["normal_radius"].default is None and sig["nsample"].default == 64


def test_python_refusals_need_no_gpu():
    from rrl_hip import icp, neighbors
    x = torch.zeros(2, 8, 3)
    with pytest.raises(ValueError, match="normal_radius"):
        icp.PlaneIcpRegistration(x, x)
    with pytest.raises(ValueError, match=r"\(2, 8, 3\)"):
        icp.PlaneIcpRegistration(x, x, torch.zeros(2, 7, 3))
    for kw, match in ((dict(normal_radius=0.0), "positive"), (dict(normal_radius=0.3, nsample=2), "nsample"),
                      (dict(normal_radius=0.3, nsample=65), "nsample"), (dict(normal_radius=0.3, eps=-1.0), "eps"),
                      (dict(normal_radius=0.3, patience=-1), "patience"), (dict(normal_radius=0.3, max_dist=0.0), "max_dist"),
                      (dict(normal_radius=0.3, R0=torch.eye(3)[None]), "R0 and T0 together")):
        with pytest.raises(ValueError, match=match):
            icp.PlaneIcpRegistration(x, x, **kw)
    with pytest.raises(ValueError, match="same B"):
        icp.PlaneIcpRegistration(x, torch.zeros(3, 8, 3), torch.zeros(3, 8, 3))
    for kw, match in ((dict(nsample=0), "nsample"), (dict(nsample=65), "nsample"), (dict(radius=-0.1), "radius"), (dict(counts=[9, 1]), r"\[0, 8\]")):
        args = dict(radius=0.3, nsample=8)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            neighbors.estimate_normals(x, args.pop("radius"), args.pop("nsample"), **args)
    with pytest.raises(ValueError, match="int32"):
        neighbors.normals_from_groups(x, torch.zeros(2, 8, 4), torch.zeros(2, 8, dtype=torch.int32))


@pytest.mark.skipif(torch.cuda.is_available(), reason="the refusal of a machine without a GPU")
def test_without_a_gpu_the_call_raises():
    from rrl_hip import icp, neighbors
    from rrl_hip._lib import RRLError
    x = torch.zeros(1, 8, 3)
    with pytest.raises(RRLError):
        neighbors.estimate_normals(x, 0.3, 8)
    with pytest.raises(RRLError):
        icp.PlaneIcpRegistration(x, x, normal_radius=0.3)
