"""The float64 twins of the closed-form fit and the ICP step (tests/kabsch_refs.py) against the reference's own solve
(tests/golden/kabsch_rpm.npz, recorded from rpm/models/rpmnet.py compute_rigid_transform by make_golden_kabsch.py), the
closed-form residual against the residual evaluated pair by pair, the step rule, and every refusal that needs no GPU -- the
Python layer's and the C entries' (fake pointers: nothing is launched)."""
import ctypes

import numpy as np
import pytest
import torch

import kabsch_refs as KR
import newton_refs as NR
from conftest import load_golden

FAKE = 0x1000  # a non-NULL, 8-byte aligned pointer that is never dereferenced
E_ARG, E_WS = -1, -3


@pytest.fixture(scope="module")
def golden():
    return load_golden("kabsch_rpm.npz")


def cases(g):
    return [str(c) for c in g["cases"]]


def test_twin_reproduces_the_reference_transform_and_gradients(golden):
    """Both are float64 on the same inputs: they differ by the SVD routine's rounding only (1e-12 of the largest entry; the
    gradients carry 1 / gap, two more digits)."""
    for name in cases(golden):
        a, b, w, C = (golden[f"{name}_{k}"] for k in ("a", "b", "w", "C"))
        got = KR.rpm_transform(torch.tensor(a), torch.tensor(b), torch.tensor(w)).numpy()
        want = golden[f"{name}_transform"]
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), name
        ga, gb, gw = KR.grads_torch(a, b, w, C[:, :, :3], C[:, :, 3], eps=1e-5, transpose_r=True)
        for mine, key in ((ga, "ga"), (gb, "gb"), (gw, "gw")):
            ref = golden[f"{name}_{key}"]
            assert np.abs(mine - ref).max() <= 1e-10 * np.abs(ref).max(), (name, key)


def test_numpy_twin_agrees_with_the_torch_twin_and_dcp_is_the_unit_weight_case(golden):
    for name in cases(golden):
        a, b, w = (golden[f"{name}_{k}"] for k in ("a", "b", "w"))
        R, T = KR.fit_torch(torch.tensor(a), torch.tensor(b), torch.tensor(w), eps=1e-5)
        for s in range(a.shape[0]):
            f = KR.fit(a[s].astype(np.float32), b[s].astype(np.float32), w[s].astype(np.float32), eps=1e-5)
            assert f["info"][1] == KR.FIT_OK and np.abs(f["R"] - R[s].numpy()).max() <= 1e-12
            assert np.abs(f["T"] - T[s].numpy()).max() <= 1e-12 * max(1.0, np.abs(T[s].numpy()).max())
        Rd, td = KR.dcp_head(torch.tensor(a).transpose(1, 2), torch.tensor(b).transpose(1, 2))
        R1, T1 = KR.fit_torch(torch.tensor(a), torch.tensor(b), torch.ones(a.shape[:2], dtype=torch.float64), transpose_r=True)
        assert torch.equal(Rd, R1) and torch.equal(td, T1)


@pytest.mark.parametrize("eps", [0.0, 1e-5, 1e-2])
def test_closed_form_residual_equals_the_direct_one(eps):
    rs = np.random.default_rng(5)
    for n, offset, mirror in ((3, 0.0, False), (40, 0.0, True), (257, 1000.0, False)):
        pa = rs.uniform(-1, 1, (n, 3)) + offset
        pb = pa @ KR.fit_pairs(rs.standard_normal((9, 3)), rs.standard_normal((9, 3)), np.ones(9))["R"] + 0.1 * rs.standard_normal((n, 3))
        if mirror:
            pb[:, 0] *= -1.0
        w = rs.uniform(0.1, 1.0, n)
        f = KR.fit_pairs(pa, pb, w, None, eps)
        direct = KR.residual_direct(pa, pb, w, f["R"], f["T"], eps)
        scale = float((w / (w.sum() + eps) * ((pa - f["abar"]) ** 2).sum(1)).sum())
        assert abs(f["res_after"] - direct) <= 1e-12 * max(scale, direct), (n, offset, mirror)
        assert f["delta"] == (-1.0 if mirror else 1.0) and f["info"][2] == int(mirror)
        # the fit is the minimiser (eps = 0): no perturbed pose does better
        if eps == 0.0:
            for _ in range(5):
                dR = KR.fit_pairs(pa, pa + 1e-3 * rs.standard_normal((n, 3)), w)["R"]
                assert KR.residual_direct(pa, pb, w, f["R"] @ dR, f["T"] + 1e-3 * rs.standard_normal(3)) >= direct * (1 - 1e-12)


def test_statuses_of_the_twin():
    rs = np.random.default_rng(6)
    p = rs.standard_normal((10, 3)).astype(np.float32)
    assert KR.fit(p[:2], p[:2])["info"][1] == KR.FIT_FEW
    assert KR.fit(p, p, np.zeros(10, np.float32))["info"][1] == KR.FIT_FEW
    line = (np.linspace(-1, 1, 10)[:, None] * np.array([[1.0, 2.0, -0.5]])).astype(np.float32)
    f = KR.fit(line, line + np.float32(0.25))
    assert f["info"][1] == KR.FIT_DEGENERATE and abs(np.linalg.det(f["R"]) - 1.0) < 1e-12
    keys = np.array([(np.float32(0.5).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(i) for i in range(10)], np.uint64)
    keys[3], keys[4] = np.uint64(KR.ALL_ONES), np.uint64(99)
    f = KR.fit(p, p, None, keys, count_a=9, count_b=8, gate_sq=1.0)
    assert f["info"] == [6, KR.FIT_OK, 0, 4] and abs(f["key_mean"] - 0.5) < 1e-15  # rows 3, 4 (keys), 8 (count_b), 9 (count_a)
    assert KR.fit(p, p, None, keys, gate_sq=0.25)["info"][:2] == [0, KR.FIT_FEW]


def test_step_rule():
    I, z = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    Rk = KR.fit_pairs(np.eye(3), np.eye(3), np.ones(3))["R"]  # (identity)
    th = 0.01
    Rs = np.array([[np.cos(th), np.sin(th), 0], [-np.sin(th), np.cos(th), 0], [0, 0, 1]], np.float32)
    abar = np.array([1.0, 2.0, 3.0])
    # a step of 0.01 rad: committed, not calm at tol 1e-3, calm at tol 0.1
    R, T, last, st = KR.icp_step(Rs, z + 0.5, KR.FIT_OK, abar, I, z, [0, 0, -1, 0], 1e-3, 1e-3, 2)
    assert R is Rs and abs(last[0] - th) < 1e-7 and st == [1, 0, -1, KR.FIT_OK]
    want = np.linalg.norm(abar @ Rs.astype(np.float64) + 0.5 - abar)
    assert abs(last[1] - want) < 1e-12
    R, T, last, st = KR.icp_step(Rs, z, KR.FIT_OK, np.zeros(3), I, z, [4, 1, -1, 0], 0.1, 0.1, 2)
    assert st == [5, 2, 5, KR.FIT_OK]  # the second calm epoch in a row ends the pair at epoch 5
    # done: frozen, whatever the fit says
    R, T, last, st = KR.icp_step(Rs, z + 1, KR.FIT_OK, abar, I, z, st, 0.1, 0.1, 2)
    assert R is I and T is z and last is None and st == [6, 2, 5, KR.ICP_DONE]
    # a failed fit keeps the pose and resets the calm count; patience 0 never ends a pair
    for status in (KR.FIT_FEW, KR.FIT_DEGENERATE):
        R, T, last, st = KR.icp_step(Rs, z, status, abar, I, z, [2, 1, -1, 0], 0.1, 0.1, 2)
        assert R is I and st == [3, 0, -1, status]
    R, T, last, st = KR.icp_step(Rk.astype(np.float32), z, KR.FIT_OK, abar, I, z, [7, 0, -1, 0], 0.1, 0.1, 0)
    assert st == [8, 0, -1, KR.FIT_OK] and last[0] < 1e-7
    R, T, last, st = KR.icp_step(Rs * np.float32("nan"), z, KR.FIT_OK, abar, I, z, [0, 1, -1, 0], 0.1, 0.1, 2)
    assert R is I and st == [1, 0, -1, KR.FIT_DEGENERATE]


def test_step_rule_is_the_newton_twins_rule():
    """The two twins' step rules, written apart, on ONE sequence of (rotation, translation) step lengths, patience 3 and both
    tolerances 1e-3 (every length a factor 4 from them): not calm, calm, calm, a reset (the rotation alone is calm), calm x 3
    -> done at 7, then two epochs after done.  Columns 0 .. 2 of the two states agree after every epoch."""
    calm, far, mixed = (2.5e-4, 2.5e-4), (4e-3, 4e-3), (2.5e-4, 4e-3)
    lengths = [far, calm, calm, mixed, calm, calm, calm, far, calm]
    want = [[1, 0, -1], [2, 1, -1], [3, 2, -1], [4, 0, -1], [5, 1, -1], [6, 2, -1], [7, 3, 7], [8, 3, 7], [9, 3, 7]]
    Rn, Tn, sn = np.eye(3), np.zeros(3), [0, 0, -1, 0]
    Ri, Ti, si = np.eye(3, dtype=np.float32), np.zeros(3, np.float32), [0, 0, -1, 0]
    for (rot, trans), w in zip(lengths, want):
        Rn, Tn, sn, _, _ = NR.step(NR.diagonal_neq(rot, trans), 1, Rn, Tn, sn, 0.0, 1.0, 1.0, 1.0, 1e-3, 1e-3, 3, 1e-12)
        Rk, Tk = KR.stepped_fit(Ri, Ti, rot, trans)
        Ri, Ti, _, si = KR.icp_step(Rk, Tk, KR.FIT_OK, np.zeros(3), Ri, Ti, si, 1e-3, 1e-3, 3)
        assert [int(x) for x in sn[:3]] == [int(x) for x in si[:3]] == w, (w, sn, si)
    assert sn[3] == NR.DONE and si[3] == KR.ICP_DONE


def test_python_refusals_need_no_gpu():
    from rrl_hip import icp, kabsch
    ok = ((2, 8, 3), (2, 8, 3))
    kabsch.check_request(*ok, (2, 8), None, (2,))
    kabsch.check_request((2, 8, 9), (2, 12, 3), None, (2, 8), None, 0.5)
    for args, match in ((((2, 8, 3), (3, 8, 3)), "same B"), (((2, 8, 4), (2, 8, 3)), "pseudo-triangles"),
                        (((2, 8, 3), (2, 9, 3)), "n must equal m"), (((2, 0, 3), (2, 0, 3)), "empty"),
                        (((40000, 8, 3), (40000, 8, 3)), "32767"), ((*ok, (2, 7)), "w must be"),
                        ((*ok, None, (2, 9)), "keys must be"), ((*ok, None, None, (3,)), "counts must be"),
                        ((*ok, None, None, None, 0.5), "needs keys")):
        with pytest.raises(ValueError, match=match):
            kabsch.check_request(*args)
    with pytest.raises(TypeError):
        kabsch.kabsch(np.zeros((1, 4, 3)), np.zeros((1, 4, 3)))
    with pytest.raises(ValueError, match="n must equal m"):
        kabsch.kabsch(torch.zeros(1, 4, 3), torch.zeros(1, 5, 3))
    with pytest.raises(ValueError, match="int64"):
        kabsch.kabsch_from_keys(torch.zeros(1, 4, 3), torch.zeros(1, 4), torch.zeros(1, 5, 3))
    with pytest.raises(ValueError, match=r"\[0, 4\]"):
        kabsch.kabsch(torch.zeros(1, 4, 3), torch.zeros(1, 4, 3), counts=[5])
    icp.check_request((2, 8, 3), (2, 12, 9), 1 << 20, 0.1, 3)
    for args, match in ((((2, 8, 3), (3, 8, 3), 1 << 20), "same B"), (((2, 8, 5), (2, 8, 3), 1 << 20), "points"),
                        (((2, 8, 3), (2, 8, 3), 4), "sort_capacity"), (((2, 8, 3), (2, 8, 3), 64, 0.0), "max_dist"),
                        (((2, 8, 3), (2, 8, 3), 64, None, -1), "patience")):
        with pytest.raises(ValueError, match=match):
            icp.check_request(*args)
    with pytest.raises(ValueError, match="R0 and T0 together"):
        icp.IcpRegistration(torch.zeros(1, 4, 3), torch.zeros(1, 4, 3), R0=torch.eye(3)[None])


# ---- the C entries: every refusal on the host, before anything is launched -------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from rrl_hip import _lib, build
    build.build_lib()
    return _lib.load()


def kabsch_args(lib, **over):
    from rrl_hip import _lib
    k = _lib.KabschArgs()
    base = dict(struct_bytes=ctypes.sizeof(k), B=2, n=1000, m=1000, a_stride=3, b_stride=3, transpose_r=0, a=FAKE, b=FAKE, w=None,
                keys=None, count_a=None, count_b=None, gate_sq=None, eps_w=0.0, rank_tol=1e-6, part=FAKE,
                part_bytes=int(lib.rrl_kabsch_part_bytes(2, 1000)), R=FAKE, T=FAKE, fit=FAKE, info=FAKE)
    base.update(over)
    for name, v in base.items():
        setattr(k, name, v)
    return k


KABSCH_REFUSALS = [dict(a=None), dict(b=None), dict(R=None), dict(T=None), dict(fit=None), dict(info=None), dict(part=None), dict(B=-1),
                   dict(n=0), dict(m=0), dict(a_stride=2), dict(b_stride=2), dict(m=999), dict(gate_sq=FAKE), dict(B=32768),
                   dict(struct_bytes=8), dict(part=FAKE + 4), dict(fit=FAKE + 4)]


def test_c_refusals_return_their_codes_without_a_launch(lib):
    assert lib.rrl_kabsch_fwd(None, None) == E_ARG
    for over in KABSCH_REFUSALS:
        assert lib.rrl_kabsch_fwd(ctypes.byref(kabsch_args(lib, **over)), None) == E_ARG, over
    assert lib.rrl_kabsch_fwd(ctypes.byref(kabsch_args(lib, part_bytes=int(lib.rrl_kabsch_part_bytes(2, 1000)) - 1)), None) == E_WS
    assert lib.rrl_kabsch_fwd(ctypes.byref(kabsch_args(lib, keys=FAKE, m=77, part_bytes=0)), None) == E_WS  # (keys: m is free)
    assert lib.rrl_kabsch_fwd(ctypes.byref(kabsch_args(lib, B=0, part_bytes=0)), None) == 0  # no sample: no launch
    assert lib.rrl_kabsch_bwd(ctypes.byref(kabsch_args(lib, keys=FAKE)), None, None, None, None, None, None) == E_ARG
    assert lib.rrl_kabsch_bwd(ctypes.byref(kabsch_args(lib, m=999)), None, None, None, None, None, None) == E_ARG
    assert lib.rrl_kabsch_bwd(ctypes.byref(kabsch_args(lib, B=0)), None, None, None, None, None, None) == 0
    assert lib.rrl_kabsch_part_bytes(0, 5) == 0 and lib.rrl_kabsch_part_bytes(3, 513) == 8 * 21 * 3 * 2
    step = lambda **o: lib.rrl_icp_step_batch(*[o.get(k, d) for k, d in (  # noqa: E731
        ("Rk", FAKE), ("Tk", FAKE), ("info", FAKE), ("fit", FAKE), ("R", FAKE), ("T", FAKE), ("tol_rot", FAKE), ("tol_trans", FAKE),
        ("patience", 3), ("value", None), ("table", None), ("cursor", None), ("nrows", 0), ("row", None), ("last_step", None),
        ("state", FAKE), ("B", 2))], None)
    for over in (dict(Rk=None), dict(Tk=None), dict(info=None), dict(fit=None), dict(R=None), dict(T=None), dict(state=None), dict(B=-1),
                 dict(tol_rot=None), dict(tol_trans=None)):
        assert step(**over) == E_ARG, over
    assert step(B=0) == 0


def icp_args(lib, **over):
    from rrl_hip import _lib
    a = _lib.IcpEpochArgs()
    base = dict(struct_bytes=ctypes.sizeof(a), B=2, N=1000, M=900, patience=3, src=FAKE, tar=FAKE, count1=None, count2=None, R=FAKE,
                T=FAKE, moved=FAKE, cham_ws=FAKE, cham_ws_bytes=int(lib.rrl_chamfer_workspace_bytes(2, 1000, 900)), best_x=FAKE,
                best_y=FAKE, values=FAKE, order_x=None, order_y=None, w=None, gate_sq=None, eps_w=0.0, rank_tol=1e-6, part=FAKE,
                part_bytes=int(lib.rrl_kabsch_part_bytes(2, 1000)), Rk=FAKE, Tk=FAKE, fit=FAKE, info=FAKE, tol_rot=FAKE,
                tol_trans=FAKE, last_step=None, state=FAKE, table=None, cursor=None, table_rows=0, row=None)
    base.update(over)
    for name, v in base.items():
        setattr(a, name, v)
    return a


def test_icp_epoch_refuses_before_its_first_launch(lib):
    assert lib.rrl_icp_epoch(None, None) == E_ARG
    refusals = [dict(struct_bytes=16), dict(B=0), dict(B=32768), dict(N=0), dict(M=0), dict(N=lib.rrl_sort_capacity() + 1),
                dict(count1=FAKE), dict(count2=FAKE), dict(order_x=FAKE), dict(order_y=FAKE), dict(tol_rot=None), dict(part=FAKE + 4)]
    refusals += [{k: None} for k in ("src", "tar", "R", "T", "moved", "cham_ws", "best_x", "best_y", "values", "part", "Rk", "Tk", "fit",
                                     "info", "state")]
    for over in refusals:
        assert lib.rrl_icp_epoch(ctypes.byref(icp_args(lib, **over)), None) == E_ARG, over
        assert lib.rrl_icp_epoch(ctypes.byref(icp_args(lib, cham_ws_bytes=64, part_bytes=8, **over)), None) == E_ARG, over  # RRL_E_ARG comes before RRL_E_WS
    assert lib.rrl_icp_epoch(ctypes.byref(icp_args(lib, cham_ws_bytes=64)), None) == E_WS
    assert lib.rrl_icp_epoch(ctypes.byref(icp_args(lib, part_bytes=8)), None) == E_WS


def test_entries_in_the_header_and_the_binding(lib):
    from rrl_hip import callsites, icp, kabsch
    assert callable(kabsch.kabsch) and callable(kabsch.kabsch_from_keys) and callable(icp.icp_pairs)
    assert callable(callsites.rpm_compute_rigid_transform) and callable(callsites.dcp_svd_head_pose)
