"""The twins of the robust ICP loop (tests/robust_refs.py) against torch.median and against themselves on the acceptance
pairs, the annealing rule's state machine, and every refusal that needs no GPU -- the Python layer's and the C entries' (fake
pointers: nothing is launched)."""
import ctypes

import numpy as np
import pytest
import torch

import kabsch_refs as KR
import robust_refs as RR

FAKE = 0x1000  # a non-NULL, 8-byte aligned pointer that is never dereferenced
E_ARG, E_WS = -1, -3
BOUND_DEG, FACTOR = 0.05, 5.0  # every robust pair ends within BOUND_DEG; the plain twin FACTOR times farther on every pair


@pytest.mark.parametrize("k", [1, 2, 7, 8, 255, 256])
def test_key_median_is_torch_median(k):
    rs = np.random.default_rng(k)
    for words in (rs.uniform(0, 4, k).astype(np.float32), np.full(k, 0.375, np.float32),
                  rs.integers(0, 3, k).astype(np.float32), np.concatenate([[0.0, np.inf], rs.uniform(0, 1, k)]).astype(np.float32)[:max(k, 2)]):
        keys = RR.pack_keys(words, rs.integers(0, 50, len(words)))
        med, cnt = RR.key_median_ref(keys, 50)
        assert cnt == len(words) and med.tobytes() == torch.median(torch.from_numpy(words)).numpy().tobytes()
    # rows that do not count: beyond count_a, all ones, an index >= m or >= count_b
    words = rs.uniform(0, 4, 12).astype(np.float32)
    keys = RR.pack_keys(words, np.arange(12))
    keys[2] = np.uint64(RR.ALL_ONES)
    keys[5] = RR.pack_keys([0.5], [40])[0]
    med, cnt = RR.key_median_ref(keys, 30, count_a=10, count_b=9)
    keep = [i for i in range(10) if i not in (2, 5, 9)]  # (row 9's index 9 >= count_b)
    assert cnt == len(keep) and med == torch.median(torch.from_numpy(words[keep])).item()
    assert RR.key_median_ref(keys, 30, count_a=0) == (np.float32(0.0), 0)


def test_weights_and_starting_scale_of_the_twin():
    d2 = np.array([0.0, 0.03125, 0.5, 2000.0, np.inf], np.float32)  # nu = 1 / 8: d2 / (2 nu^2) = 0, 1, 16, ...
    keys = RR.pack_keys(d2, np.arange(5))
    w = RR.welsch_weights_ref(keys, 0.125, 5)
    assert w.dtype == np.float32 and w[0] == 1.0 and abs(w[1] - np.exp(-1.0)) < 2.0 ** -24 and w[3] == 0.0 and w[4] == 0.0
    assert (RR.welsch_weights_ref(keys[:4], 1e30, 5) == 1.0).all()
    for bad in (0.0, -1.0, np.nan, np.inf):
        assert not RR.welsch_weights_ref(keys, bad, 5).any()
    keys[1] = np.uint64(RR.ALL_ONES)
    assert RR.welsch_weights_ref(keys, 0.125, 5, count_a=3)[1:].tolist() == [0.0, float(np.float32(np.exp(-16.0))), 0.0, 0.0]
    assert RR.nu_start_ref(np.float32(0.04), 3.0, 0.01) == np.float32(3.0 * np.sqrt(np.float64(np.float32(0.04))))
    assert RR.nu_start_ref(np.float32(0.0), 3.0, 0.01) == np.float32(0.01)


def test_annealing_rule_of_the_twin():
    I, z, ab = np.eye(3, dtype=np.float32), np.zeros(3, np.float32), np.zeros(3)
    calm, far = KR.stepped_fit(I, z, 2.5e-4, 2.5e-4), KR.stepped_fit(I, z, 4e-3, 4e-3)
    rule = lambda fit, status, st, lv, nu, patience=2, cap=0: RR.robust_step_rule_ref(  # noqa: E731
        fit[0], fit[1], status, ab, I, z, st, lv, nu, 0.25, 1e-3, 1e-3, patience, 0.5, cap)
    # a calm epoch that completes the patience above nu_end: halved, not done, counters reset
    R, T, last, st, lv, nu = rule(calm, KR.FIT_OK, [4, 1, -1, 0], [3, 0], 1.0)
    assert R is calm[0] and st == [5, 0, -1, KR.FIT_OK] and lv == [0, 1] and nu == np.float32(0.5)
    # ... whose product falls below nu_end: clamped
    assert rule(calm, KR.FIT_OK, [4, 1, -1, 0], [3, 2], 0.375)[3:] == ([5, 0, -1, KR.FIT_OK], [0, 3], np.float32(0.25))
    # ... at nu_end: done now, frozen from the next call on
    R, T, last, st, lv, nu = rule(calm, KR.FIT_OK, [4, 1, -1, 0], [3, 2], 0.25)
    assert st == [5, 2, 5, KR.FIT_OK] and lv == [4, 2] and nu == np.float32(0.25)
    R2, T2, last, st, lv, nu = rule(far, KR.FIT_OK, st, lv, nu)
    assert R2 is I and last is None and st == [6, 2, 5, KR.ICP_DONE] and lv == [4, 2]
    # not calm: the level goes on; the cap ends it; a failed fit resets the calm count and still counts
    assert rule(far, KR.FIT_OK, [4, 1, -1, 0], [3, 0], 1.0)[3:] == ([5, 0, -1, KR.FIT_OK], [4, 0], np.float32(1.0))
    assert rule(far, KR.FIT_OK, [4, 0, -1, 0], [3, 0], 1.0, cap=4)[3:] == ([5, 0, -1, KR.FIT_OK], [0, 1], np.float32(0.5))
    R, T, last, st, lv, nu = rule(calm, KR.FIT_FEW, [4, 1, -1, 0], [2, 0], 1.0, cap=4)
    assert R is I and last is None and st == [5, 0, -1, KR.FIT_FEW] and lv == [3, 0] and nu == np.float32(1.0)
    # patience 0: the cap alone
    assert rule(calm, KR.FIT_OK, [9, 0, -1, 0], [1, 0], 0.25, patience=0, cap=2)[3] == [10, 0, 10, KR.FIT_OK]


@pytest.fixture(scope="module")
def acceptance():
    """{(n, seed): (robust run, plain run, generating rotation)} of the twins, computed once."""
    out = {}
    for n in (256, 64):
        for seed in range(8):
            src, tar, Rg = RR.outlier_pair(seed, n, 10.0, 0.2)
            out[n, seed] = (RR.robust_icp_ref(src, tar, n_epoch=60), RR.robust_icp_ref(src, tar, n_epoch=200, robust=False), Rg)
    return out


def test_outlier_pair_recipe():
    src, tar, Rg = RR.outlier_pair(3, 256, 10.0, 0.2)
    assert src.dtype == tar.dtype == np.float32 and src.shape == tar.shape == (256, 3)
    assert abs(RR.rot_err_deg(np.eye(3), Rg) - 10.0) < 1e-9 and abs(np.linalg.det(Rg) - 1.0) < 1e-12
    back = (tar.astype(np.float64) - RR.SHIFT) @ Rg.T  # the clean source, permuted
    d = np.sqrt(((src[:, None, :].astype(np.float64) - back[None, :, :]) ** 2).sum(-1)).min(1)
    assert (d < 1e-6).sum() == 256 - 51 and (d > 1e-3).sum() == 51  # 20 % of the rows have no partner
    again = RR.outlier_pair(3, 256, 10.0, 0.2)
    assert again[0].tobytes() == src.tobytes() and again[1].tobytes() == tar.tobytes()


@pytest.mark.parametrize("n", [256, 64])
def test_robust_twin_registers_the_acceptance_pairs(acceptance, n):
    for seed in range(8):
        rob, plain, Rg = acceptance[n, seed]
        err, err_plain = RR.rot_err_deg(rob["R"], Rg), RR.rot_err_deg(plain["R"], Rg)
        print(f"n {n} seed {seed}: robust {err:.5f} deg in {rob['epochs']} epochs, {rob['level'][1]} levels; plain {err_plain:.4f} deg")
        assert 0 <= rob["state"][2] <= 60 and rob["level"][1] >= 1 and rob["nu"] == rob["nu_end"], (n, seed, rob)
        assert err <= BOUND_DEG, (n, seed, err)
        assert plain["state"][2] >= 0 and err_plain >= FACTOR * err, (n, seed, err, err_plain)


def test_python_refusals_need_no_gpu():
    from rrl_hip import icp
    icp.check_robust_request()
    icp.check_robust_request(2.0, 0.01, 0.7, 0, 3)
    icp.check_robust_request(3.0, [0.01, 0.02], 0.5, 10, 0, B=2)
    icp.check_robust_request(3.0, torch.tensor([0.01, 0.02]), B=2)
    for kw, match in ((dict(nu_start=0.0), "nu_start"), (dict(nu_start=float("nan")), "nu_start"), (dict(anneal=0.0), "anneal"),
                      (dict(anneal=1.0), "anneal"), (dict(level_cap=-1), "level_cap"), (dict(level_cap=2.5), "level_cap"),
                      (dict(patience=0, level_cap=0), "nothing would anneal"), (dict(nu_end=0.0), "nu_end"),
                      (dict(nu_end=[0.1, -0.1], B=2), "nu_end"), (dict(nu_end=[0.1, 0.1, 0.1], B=2), "one per pair")):
        with pytest.raises(ValueError, match=match):
            icp.check_robust_request(**kw)
    with pytest.raises(ValueError, match="anneal"):
        icp.RobustIcpRegistration(torch.zeros(1, 4, 3), torch.zeros(1, 4, 3), anneal=1.5)
    with pytest.raises(ValueError, match="same B"):
        icp.RobustIcpRegistration(torch.zeros(1, 4, 3), torch.zeros(2, 4, 3))
    assert callable(icp.robust_icp_pairs)


# ---- the C entries: every refusal on the host, before anything is launched -------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from rrl_hip import _lib, build
    build.build_lib()
    return _lib.load()


def test_names_in_the_header_and_the_binding(lib):
    from rrl_hip import _abi, _lib
    for name in ("rrl_key_median", "rrl_welsch_weights", "rrl_robust_step_batch", "rrl_robust_icp_epoch"):
        assert name in _abi.PROTOS and _abi.PROTOS[name][0] is ctypes.c_int and hasattr(lib, name) and name in _lib.EXPORTS
    # the epoch runs on rrl_icp_epoch's own struct (the header gains no struct); what the annealing adds are plain arguments:
    # args, init, w, nu, nu_end, med_sq, med_info, nu_scale, anneal, level_cap, level, stream
    V = ctypes.c_void_p
    assert _abi.PROTOS["rrl_robust_icp_epoch"][1] == [V, ctypes.c_int, V, V, V, V, V, ctypes.c_double, ctypes.c_float, ctypes.c_int, V, V]
    assert "rrl_icp_epoch_args" in _abi.STRUCTS and not [n for n in _abi.STRUCTS if "robust" in n]
    assert _abi.PROTOS["rrl_key_median"][1][9] is ctypes.c_double and _abi.PROTOS["rrl_robust_step_batch"][1][18] is ctypes.c_float


def call(fn, spec, **over):
    return fn(*[over.get(k, d) for k, d in spec], None)


MEDIAN = (("keys", FAKE), ("count_a", None), ("count_b", None), ("B", 2), ("n", 1000), ("m", 900), ("med_sq", FAKE), ("info", FAKE),
          ("nu", None), ("nu_scale", 0.0), ("nu_end", None))
WEIGHTS = (("keys", FAKE), ("count_a", None), ("count_b", None), ("nu", FAKE), ("w", FAKE), ("B", 2), ("n", 1000), ("m", 900))
STEP = (("Rk", FAKE), ("Tk", FAKE), ("info", FAKE), ("fit", FAKE), ("R", FAKE), ("T", FAKE), ("tol_rot", FAKE), ("tol_trans", FAKE),
        ("patience", 3), ("value", None), ("table", None), ("cursor", None), ("nrows", 0), ("row", None), ("last_step", None),
        ("state", FAKE), ("nu", FAKE), ("nu_end", FAKE), ("anneal", 0.5), ("level_cap", 10), ("level", FAKE), ("B", 2))
NAN = float("nan")


def test_stand_alone_entries_refuse_before_a_launch(lib):
    for over in (dict(keys=None), dict(med_sq=None), dict(info=None), dict(B=-1), dict(B=32768), dict(n=0), dict(m=0),
                 dict(n=lib.rrl_sort_capacity() + 1), dict(count_a=FAKE), dict(count_b=FAKE), dict(nu=FAKE, nu_scale=3.0),
                 dict(nu=FAKE, nu_end=FAKE, nu_scale=0.0), dict(nu=FAKE, nu_end=FAKE, nu_scale=NAN)):
        assert call(lib.rrl_key_median, MEDIAN, **over) == E_ARG, over
    assert call(lib.rrl_key_median, MEDIAN, B=0) == 0
    for over in (dict(keys=None), dict(nu=None), dict(w=None), dict(B=-1), dict(B=32768), dict(n=0), dict(m=0), dict(count_a=FAKE),
                 dict(count_b=FAKE)):
        assert call(lib.rrl_welsch_weights, WEIGHTS, **over) == E_ARG, over
    assert call(lib.rrl_welsch_weights, WEIGHTS, B=0) == 0
    for over in (dict(Rk=None), dict(Tk=None), dict(info=None), dict(fit=None), dict(R=None), dict(T=None), dict(state=None), dict(B=-1),
                 dict(tol_rot=None), dict(tol_trans=None), dict(nu=None), dict(nu_end=None), dict(level=None), dict(anneal=0.0),
                 dict(anneal=1.0), dict(anneal=NAN), dict(level_cap=-1), dict(patience=0, level_cap=0)):
        assert call(lib.rrl_robust_step_batch, STEP, **over) == E_ARG, over
    assert call(lib.rrl_robust_step_batch, STEP, B=0) == 0
    assert call(lib.rrl_robust_step_batch, STEP, B=0, patience=0, tol_rot=None, tol_trans=None) == 0  # (the cap alone is a rule)


EXTRA = (("init", 1), ("w_out", FAKE), ("nu", FAKE), ("nu_end", FAKE), ("med_sq", FAKE), ("med_info", FAKE), ("nu_scale", 3.0), ("anneal", 0.5),
         ("level_cap", 10), ("level", FAKE))


def robust_epoch(lib, **over):
    """rrl_robust_icp_epoch on fake pointers: `over` names fields of rrl_icp_epoch_args or the plain arguments (w: the struct's
    field, which must stay NULL; w_out: the plain argument, the weights).  Only ever called with something to refuse."""
    from rrl_hip import _lib
    a = _lib.IcpEpochArgs()
    base = dict(struct_bytes=ctypes.sizeof(a), B=2, N=1000, M=900, patience=3, src=FAKE, tar=FAKE, count1=None, count2=None, R=FAKE,
                T=FAKE, moved=FAKE, cham_ws=FAKE, cham_ws_bytes=int(lib.rrl_chamfer_workspace_bytes(2, 1000, 900)), best_x=FAKE,
                best_y=FAKE, values=FAKE, order_x=None, order_y=None, w=None, gate_sq=None, eps_w=0.0, rank_tol=1e-6, part=FAKE,
                part_bytes=int(lib.rrl_kabsch_part_bytes(2, 1000)), Rk=FAKE, Tk=FAKE, fit=FAKE, info=FAKE, tol_rot=FAKE,
                tol_trans=FAKE, last_step=None, state=FAKE, table=None, cursor=None, table_rows=0, row=None)
    plain = dict(EXTRA)
    for name, v in over.items():
        (plain if name in plain else base)[name] = v
    for name, v in base.items():
        setattr(a, name, v)
    return lib.rrl_robust_icp_epoch(ctypes.byref(a), *[plain[k] for k, _ in EXTRA], None)


def test_robust_epoch_refuses_before_its_first_launch(lib):
    epoch = lambda **over: robust_epoch(lib, **over)  # noqa: E731
    assert lib.rrl_robust_icp_epoch(None, *[d for _, d in EXTRA], None) == E_ARG
    refusals = [dict(struct_bytes=16), dict(B=0), dict(B=32768), dict(N=0), dict(M=0), dict(N=lib.rrl_sort_capacity() + 1),
                dict(M=lib.rrl_sort_capacity() + 1), dict(count1=FAKE), dict(count2=FAKE), dict(order_x=FAKE), dict(order_y=FAKE),
                dict(tol_rot=None), dict(tol_trans=None), dict(part=FAKE + 4), dict(fit=FAKE + 4), dict(anneal=0.0), dict(anneal=1.0),
                dict(anneal=NAN), dict(level_cap=-1), dict(nu_scale=0.0), dict(nu_scale=-1.0), dict(nu_scale=NAN),
                dict(patience=0, level_cap=0), dict(w=FAKE), dict(w_out=None)]
    refusals += [{k: None} for k in ("src", "tar", "R", "T", "moved", "cham_ws", "best_x", "best_y", "values", "part", "Rk", "Tk", "fit",
                                     "info", "state", "nu", "nu_end", "level", "med_sq", "med_info")]
    for over in refusals:
        assert epoch(**over) == E_ARG, over
        assert epoch(cham_ws_bytes=64, part_bytes=8, **over) == E_ARG, over  # RRL_E_ARG comes before RRL_E_WS
    assert epoch(cham_ws_bytes=64) == E_WS
    assert epoch(part_bytes=8) == E_WS
    assert epoch(part_bytes=8, init=0) == E_WS
