"""Robust ICP on the GPU (include/rrl.h rrl_key_median, rrl_welsch_weights, rrl_robust_step_batch, rrl_robust_icp_epoch;
rrl_hip/icp.py RobustIcpRegistration) against the twins of tests/robust_refs.py.

1. rrl_key_median: the twin's word, bit for bit, on keys a real walk left and on crafted keys; info and nu exactly.
2. rrl_welsch_weights: within 2^-24 of the twin, the stated exact values.
3. rrl_robust_step_batch: the twin's state machine word for word over 12 calls.
4. One rrl_robust_icp_epoch call == the six public entries in sequence, bit for bit.
5. With all weights 1.0 the loop is IcpRegistration's, bit for bit.
6. Two runs give the same bits; a sample of a ragged batch has the bits of its own B = 1 loop.
7. One epoch against the float64 twin fed the device's keys: 2^-22 max(1, |coordinate|).
8. The acceptance pairs: every pair done within 60 epochs, within 0.05 degrees; IcpRegistration five times farther.
9. The steady epoch replays from a captured graph with the eager bits."""
import ctypes

import numpy as np
import pytest
import torch

import kabsch_refs as KR
import robust_refs as RR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods():
    from rrl_hip import _lib, icp, ops
    _lib.load()
    assert torch.cuda.is_available()
    return _lib, icp, ops


def dev(x):
    x = np.ascontiguousarray(x)
    return torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).cuda()


def bits(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


def host_keys(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint64)


def clouds(B, N, M, c1=None, c2=None, seed=40, rot_deg=15.0):
    """synth.make_pair point clouds stacked to (B, N, 3), (B, M, 3); rows beyond a count NaN."""
    from rrl_hip import synth
    src, tar = np.full((B, N, 3), np.nan, np.float32), np.full((B, M, 3), np.nan, np.float32)
    for b in range(B):
        nb, mb = (N if c1 is None else c1[b]), (M if c2 is None else c2[b])
        pr = synth.make_pair(seed + b, max(nb, 3), max(mb, 3), rot_deg=rot_deg)
        src[b, :nb], tar[b, :mb] = pr["src"][:nb], pr["tar"][:mb]
    return torch.from_numpy(src).cuda(), torch.from_numpy(tar).cuda()


# ---- 1. the median ----------------------------------------------------------------------------------------------------------
def run_median(ops, keys, m, ca=None, cb=None, nu_scale=3.0, nu_end=None):
    """rrl_key_median on keys (B, n) uint64 -> (med_sq (B,) float32, info (B, 2), nu (B,) or None) as numpy."""
    B, n = keys.shape
    tk = dev(keys)
    tca, tcb = (None if ca is None else dev(np.asarray(ca, np.int32))), (None if cb is None else dev(np.asarray(cb, np.int32)))
    med, info = torch.full((B,), -1.0, device="cuda"), torch.full((B, 2), -1, dtype=torch.int32, device="cuda")
    tend = None if nu_end is None else dev(np.asarray(nu_end, np.float32))
    nu = None if nu_end is None else torch.full((B,), -1.0, device="cuda")
    P = ops._p
    ops._run(tk.device, "rrl_key_median", P(tk), P(tca), P(tcb), B, n, m, P(med), P(info), P(nu), float(nu_scale), P(tend))
    torch.cuda.synchronize()
    return med.cpu().numpy(), info.cpu().numpy(), None if nu is None else nu.cpu().numpy()


def check_median(ops, keys, m, ca=None, cb=None, what=""):
    B = keys.shape[0]
    ends = np.array([1e-3, 0.5, 1e3] * B, np.float32)[:B]  # below, about and above three median residuals
    med, info, nu = run_median(ops, keys, m, ca, cb, 3.0, ends)
    for b in range(B):
        want, k = RR.key_median_ref(keys[b], m, None if ca is None else ca[b], None if cb is None else cb[b])
        assert med[b].tobytes() == want.tobytes() and info[b].tolist() == [k, int(k == 0)], (what, b, med[b], want, info[b], k)
        assert nu[b].tobytes() == RR.nu_start_ref(want, 3.0, ends[b]).tobytes(), (what, b, nu[b])
    med2, info2, _ = run_median(ops, keys, m, ca, cb)  # (without nu; and the same bits on every call)
    assert med2.tobytes() == med.tobytes() and info2.tobytes() == info.tobytes(), what


def words_to_keys(words, rs, m):
    return RR.pack_keys(words, rs.integers(0, m, words.shape))


MEDIAN_N = [1, 2, 63, 64, 65, 255, 256, 257, 513, 1000]


@pytest.fixture(scope="module")
def walk_keys(mods):
    """Keys a real walk left: one ragged ICP epoch of three pairs at capacity 1000 x 700; a test takes the first n columns."""
    _, icp, _ = mods
    c1, c2 = [1000, 600, 257], [700, 350, 700]
    src, tar = clouds(3, 1000, 700, c1, c2, seed=90)
    reg = icp.IcpRegistration(src, tar, counts1=c1, counts2=c2)
    reg.epoch()
    torch.cuda.synchronize()
    return host_keys(reg.best_x).copy(), c1, c2


@pytest.mark.parametrize("n", MEDIAN_N)
def test_median_is_the_twins_word(mods, walk_keys, n):
    _, _, ops = mods
    B, m = 3, 700
    rs = np.random.default_rng(n)
    wk, c1, c2 = walk_keys
    keys = np.ascontiguousarray(wk[:, :n])
    check_median(ops, keys, m, [min(c, n) for c in c1], c2, "walk")
    check_median(ops, np.ascontiguousarray(wk[:1, :n]), m, None, None, "walk, no counts")
    f32 = lambda a: np.asarray(a, np.uint32).view(np.float32)  # noqa: E731
    base = np.float32(0.375).view(np.uint32)
    crafted = {
        "equal": np.full((B, n), 0.375, np.float32),
        "two": np.where(np.arange(n)[None, :] % 2 == np.arange(B)[:, None] % 2, np.float32(0.25), np.float32(4.0)).astype(np.float32),
        "low byte": f32(base + rs.integers(0, 256, (B, n)).astype(np.uint32)),
        "high byte": f32(rs.integers(0, 0x7F, (B, n)).astype(np.uint32) << np.uint32(24)),
        "each byte once": f32((rs.integers(0, 0x7F, (B, n)).astype(np.uint32) << np.uint32(24)) | (rs.integers(0, 4, (B, n)).astype(np.uint32) * np.uint32(0x010101))),
        "zero and inf": np.where(rs.uniform(size=(B, n)) < 0.3, np.float32(0.0), np.where(rs.uniform(size=(B, n)) < 0.5, np.float32(np.inf), rs.uniform(0, 2, (B, n)).astype(np.float32))).astype(np.float32),
        "random": rs.uniform(0, 4, (B, n)).astype(np.float32),
    }
    for what, words in crafted.items():
        keys = words_to_keys(words, rs, m)
        check_median(ops, keys, m, None, None, what)
        for kk in (n, n - 1):  # "two": even and odd k
            if kk >= 1:
                check_median(ops, keys, m, [kk, max(kk - 1, 0), kk // 2], [m, m, m], what + f" k={kk}")
        # ragged: counts 0 and 1, all-ones keys and indices beyond m / count_b interleaved
        mixed = keys.copy()
        mixed[:, ::3] = np.uint64(RR.ALL_ONES)
        mixed[:, 1::5] = RR.pack_keys(words[:, 1::5], rs.integers(m, m + 50, words[:, 1::5].shape))
        check_median(ops, mixed, m, [n, 1, 0], [m // 2, m, m], what + " mixed")
        check_median(ops, mixed, m, [0, n, min(n, 2)], [m, 1, 0], what + " mixed, few")


def test_median_of_65536_rows(mods):
    _, _, ops = mods
    rs = np.random.default_rng(65536)
    words = (rs.uniform(0, 1, (1, 65536)) ** 4).astype(np.float32)
    keys = words_to_keys(words, rs, 65536)
    keys[0, ::7] = np.uint64(RR.ALL_ONES)
    check_median(ops, keys, 65536, None, None, "65536")
    check_median(ops, keys, 65536, [65535], [40000], "65536 ragged")


# ---- 2. the weights ---------------------------------------------------------------------------------------------------------
def run_weights(ops, keys, nu, m, ca=None, cb=None):
    B, n = keys.shape
    tk, tnu = dev(keys), dev(np.asarray(nu, np.float32))
    tca, tcb = (None if ca is None else dev(np.asarray(ca, np.int32))), (None if cb is None else dev(np.asarray(cb, np.int32)))
    w = torch.full((B, n), -1.0, device="cuda")
    P = ops._p
    ops._run(tk.device, "rrl_welsch_weights", P(tk), P(tca), P(tcb), P(tnu), P(w), B, n, m)
    torch.cuda.synchronize()
    return w.cpu().numpy()


@pytest.mark.parametrize("n", [1, 255, 300])
def test_weights_against_the_twin(mods, n):
    _, _, ops = mods
    m = 77
    nus = np.array([0.3, 1.0, 1e30, 1e-3, 0.0, -1.0, np.nan, np.inf], np.float32)
    B = len(nus)
    rs = np.random.default_rng(n)
    words = rs.uniform(0.01, 4.0, (B, n)).astype(np.float32)
    words[:, ::11] = 0.0
    keys = words_to_keys(words, rs, m)
    keys[:, 2::7] = np.uint64(RR.ALL_ONES)
    keys[:, 3::9] = RR.pack_keys(words[:, 3::9], rs.integers(m, m + 9, words[:, 3::9].shape))
    for ca, cb in ((None, None), ([n, n // 2, n, n, 0, 1, n, n], [m, m, m // 2, m, m, m, 0, m])):
        w = run_weights(ops, keys, nus, m, ca, cb)
        assert np.isfinite(w).all()
        for b in range(B):
            cab, cbb = (None if ca is None else ca[b]), (None if cb is None else cb[b])
            want = RR.welsch_weights_ref(keys[b], nus[b], m, cab, cbb)
            ok = RR.valid_rows(keys[b], m, cab, cbb)
            assert np.abs(w[b].astype(np.float64) - want.astype(np.float64)).max() <= 2.0 ** -24, (b, ca)
            assert not w[b][~ok].any()
            if b == 2:
                assert (w[b][ok] == 1.0).all()       # nu = 1e30
            if b == 3:                                # d^2 / nu^2 >= 1e4 (>= 2000): exactly 0, except the zero distances' 1.0
                far = ok & (words[b] > 0)
                assert not w[b][far].any() and (w[b][ok & (words[b] == 0)] == 1.0).all()
            if b >= 4:
                assert not w[b].any()                 # nu = 0, negative, NaN, inf


# ---- 3. the step rule ---------------------------------------------------------------------------------------------------------
CALM, FAR = (2.5e-4, 2.5e-4), (4e-3, 4e-3)  # step lengths a factor 4 below / above the tolerances 1e-3
# per pair: twelve (step lengths or None for a fit that is not RRL_FIT_OK, fit status); NaN: a non-finite Rk
STEP_PAIRS = [
    dict(nu=1.0, nu_end=0.01, seq=[(CALM, 0)] * 12),                                     # calms above nu_end: halved, never done
    dict(nu=0.25, nu_end=0.25, seq=[(CALM, 0)] * 2 + [(FAR, 0), (FAR, 1), (FAR, 0)] * 3 + [(CALM, 0)]),  # done at 2, then frozen
    dict(nu=1.0, nu_end=0.25, seq=[(FAR, 0)] * 12),                                      # the cap alone: 0.5 at 4, 0.25 at 8, done at 12
    dict(nu=0.3, nu_end=0.2, seq=[(CALM, 0)] * 12),                                      # 0.3 x 0.5 clamps to 0.2 at 2; done at 4
    dict(nu=1.0, nu_end=0.1, seq=[(CALM, 0), (CALM, 1), (CALM, 0), (CALM, 0), (FAR, 0), (CALM, 2), (CALM, 0), ("nan", 0)] + [(CALM, 0)] * 4),
    dict(nu=0.5, nu_end=0.125, seq=[(CALM, 0), (FAR, 0)] * 6),                           # never two calm epochs in a row: the cap again
]


@pytest.mark.parametrize("patience,cap", [(2, 4), (0, 3), (3, 0)])
def test_step_rule_word_for_word(mods, patience, cap):
    _, _, ops = mods
    B, tol, anneal = len(STEP_PAIRS), 1e-3, 0.5
    rs = np.random.default_rng(7)
    R = np.stack([KR.stepped_fit(np.eye(3), np.zeros(3), 0.1 * (b + 1), 0.0)[0] for b in range(B)])
    T = rs.standard_normal((B, 3)).astype(np.float32)
    state, level = [[0, 0, -1, 0] for _ in range(B)], [[0, 0] for _ in range(B)]
    nu = [np.float32(p["nu"]) for p in STEP_PAIRS]
    ends = np.array([p["nu_end"] for p in STEP_PAIRS], np.float32)
    last = [(np.float32(-1.0), np.float32(-1.0))] * B
    tR, tT, tstate, tlevel, tnu, tend = dev(R), dev(T), dev(np.array(state, np.int32)), dev(np.array(level, np.int32)), dev(np.array(nu)), dev(ends)
    tlast, tols = torch.full((B, 2), -1.0, device="cuda"), torch.full((B,), tol, device="cuda")
    table, cursor, row = torch.zeros(12, B, 3, device="cuda"), torch.zeros(B, dtype=torch.int64, device="cuda"), torch.zeros(B, 3, device="cuda")
    value = dev(np.arange(1, B + 1, dtype=np.float32))
    P = ops._p
    for call in range(12):
        Rk, Tk, info, fit = np.zeros((B, 3, 3), np.float32), np.zeros((B, 3), np.float32), np.zeros((B, 4), np.int32), np.zeros((B, 32))
        for b, p in enumerate(STEP_PAIRS):
            lengths, status = p["seq"][call]
            Rk[b], Tk[b] = KR.stepped_fit(R[b], T[b], *(CALM if lengths == "nan" else lengths))
            if lengths == "nan":
                Rk[b, 1, 1] = np.nan
            info[b, 1] = status
            fit[b, 29] = 0.5 ** (call + b)
        tRk, tTk, tinfo, tfit = dev(Rk), dev(Tk), dev(info), dev(fit)
        ops._run(tR.device, "rrl_robust_step_batch", P(tRk), P(tTk), P(tinfo), P(tfit), P(tR), P(tT), P(tols), P(tols), patience, P(value),
                 P(table), P(cursor), 12, P(row), P(tlast), P(tstate), P(tnu), P(tend), anneal, cap, P(tlevel), B)
        torch.cuda.synchronize()
        Rn, Tn = R.copy(), T.copy()
        for b in range(B):
            Rb, Tb, ls, state[b], level[b], nu[b] = RR.robust_step_rule_ref(Rk[b], Tk[b], int(info[b, 1]), np.zeros(3), R[b], T[b], state[b],
                                                                            level[b], nu[b], ends[b], tol, tol, patience, anneal, cap)
            Rn[b], Tn[b] = Rb, Tb
            last[b] = ls if ls is not None else last[b]
        R, T = Rn, Tn
        where = (patience, cap, call)
        assert tstate.cpu().tolist() == state, (where, tstate.cpu().tolist(), state)
        assert tlevel.cpu().tolist() == level, (where, tlevel.cpu().tolist(), level)
        assert bits(tnu) == np.array(nu, np.float32).tobytes(), (where, tnu.tolist(), nu)
        assert bits(tR) == R.tobytes() and bits(tT) == T.tobytes(), where
        assert bits(tlast) == np.array(last, np.float32).tobytes(), (where, tlast.tolist(), last)
        want_row = [[float(np.float32(fit[b, 29])), float(b + 1), float(info[b, 1] == 0)] for b in range(B)]
        assert row.cpu().tolist() == want_row and table[call].cpu().tolist() == want_row and cursor.tolist() == [call + 1] * B, where
    if (patience, cap) == (2, 4):  # the six stories, as the twin tells them
        assert [s[2] for s in state] == [-1, 2, 12, 4, -1, 12] and [lv[1] for lv in level] == [6, 0, 2, 1, 4, 2], (state, level)
        assert [float(x) for x in nu] == [2.0 ** -6, 0.25, 0.25, float(np.float32(0.2)), float(np.float32(0.1)), 0.125]
        assert state[1][3] == KR.ICP_DONE and state[3][3] == KR.ICP_DONE


# ---- 4. composition -------------------------------------------------------------------------------------------------------
def composed_epoch(_lib, ops, r, init):
    """One epoch on RobustIcpRegistration r's buffers from the six public entries."""
    P, d = ops._p, r.dev
    ops._run(d, "rrl_rigid_apply_fwd", P(r.src), P(r.R), P(r.T), P(r.moved), r.B, r.N, 0, 0)
    ops._run(d, "rrl_chamfer_tree_fwd_counted", P(r.moved), P(r.tar), P(r.counts1), P(r.counts2), P(r.cham_ws), r.cham_ws.numel(),
             P(r.best_x), P(r.best_y), P(r.value), None, r.B, r.N, r.M, P(r.order_x), P(r.order_y))
    if init:
        ops._run(d, "rrl_key_median", P(r.best_x), P(r.counts1), P(r.counts2), r.B, r.N, r.M, P(r.med_sq), P(r.med_info), P(r.nu),
                 r.nu_start, P(r.nu_end))
    ops._run(d, "rrl_welsch_weights", P(r.best_x), P(r.counts1), P(r.counts2), P(r.nu), P(r.weights), r.B, r.N, r.M)
    k = _lib.KabschArgs()
    k.struct_bytes = ctypes.sizeof(k)
    k.B, k.n, k.m, k.a_stride, k.b_stride, k.transpose_r = r.B, r.N, r.M, 3, 3, 0
    k.a, k.b, k.w, k.keys, k.count_a, k.count_b, k.gate_sq = P(r.src), P(r.tar), P(r.weights), P(r.best_x), P(r.counts1), P(r.counts2), P(r.gate_sq)
    k.eps_w, k.rank_tol = 0.0, r._args.rank_tol
    k.part, k.part_bytes, k.R, k.T, k.fit, k.info = P(r.part), r.part.numel() * 8, P(r.Rk), P(r.Tk), P(r.fit), P(r.info)
    ops._run(d, "rrl_kabsch_fwd", ctypes.byref(k))
    ops._run(d, "rrl_robust_step_batch", P(r.Rk), P(r.Tk), P(r.info), P(r.fit), P(r.R), P(r.T), P(r.tol_rot), P(r.tol_trans), r.patience,
             P(r.value), P(r.table), P(r.cursor), r.table.shape[0], P(r.row), P(r.last_step), P(r.state), P(r.nu), P(r.nu_end), r.anneal,
             r.level_cap, P(r.level), r.B)


FIELDS = ("moved", "best_x", "best_y", "value", "med_sq", "med_info", "nu", "weights", "fit", "info", "Rk", "Tk", "R", "T", "state",
          "level", "last_step", "table", "cursor", "row")
C1, C2 = [200, 150, 64, 3], [257, 130, 257, 200]


@pytest.mark.parametrize("ragged", [False, True])
def test_one_call_equals_the_six_entries(mods, ragged):
    _lib, icp, ops = mods
    B, N, M = 4, 200, 257
    c1, c2 = (C1, C2) if ragged else (None, None)
    src, tar = clouds(B, N, M, c1, c2)
    kw = dict(counts1=c1, counts2=c2, max_dist=0.2, tol_rot=1e-2, tol_trans=1e-2, patience=2, level_cap=3, table_rows=4)
    one, six = icp.RobustIcpRegistration(src, tar, **kw), icp.RobustIcpRegistration(src, tar, **kw)
    assert bits(one.nu_end) == bits(six.nu_end) and (one.nu_end > 0).all()
    for e in range(6):
        one.epoch()
        composed_epoch(_lib, ops, six, e == 0)
        torch.cuda.synchronize()
        for f in FIELDS:
            x, y = getattr(one, f), getattr(six, f)
            if f == "moved" and ragged:  # (rows beyond a count are NaN filler moved: compare what a sample has)
                assert all(bits(x[b, :c1[b]]) == bits(y[b, :c1[b]]) for b in range(B)), (e, f)
            else:
                assert bits(x) == bits(y), (e, f)
    assert one.cursor.tolist() == [6] * B and one.state[:, 0].tolist() == [6] * B
    assert (one.levels >= 1).all() and (one.med_info[:, 0] == torch.tensor(c1 if ragged else [N] * B, device="cuda")).all()
    assert ((one.weights >= 0) & (one.weights <= 1)).all()
    h = one.history()
    assert len(h) == B and len(h[0]) == 4 and h[0][3][1] is not None and h[0][3][2] > 0


# ---- 5. all weights 1: plain ICP -----------------------------------------------------------------------------------------------
def test_unit_weights_are_plain_icp(mods):
    """nu_end = 1e30 starts (and ends) every scale at 1e30: every weight is exactly 1.0, a level that ends is the pair's end, and
    the fit's sums with w = 1.0f are the sums without w."""
    _, icp, _ = mods
    src, tar = clouds(4, 256, 256, seed=60, rot_deg=10.0)
    plain = icp.IcpRegistration(src, tar).run(20)
    rob = icp.RobustIcpRegistration(src, tar, nu_end=1e30, level_cap=10000).run(20)
    torch.cuda.synchronize()
    assert (rob.weights == 1.0).all() and (rob.nu == 1e30).all() and not rob.levels.any()
    for f in ("R", "T", "state", "last_step", "fit", "table"):
        assert bits(getattr(rob, f)) == bits(getattr(plain, f)), f
    assert rob.level[:, 0].tolist() == [min(20, d) if d >= 0 else 20 for d in plain.done_epoch.tolist()]


# ---- 6. reproducibility and raggedness ---------------------------------------------------------------------------------------
def test_same_bits_twice_and_a_ragged_sample_is_its_own_loop(mods):
    _, icp, _ = mods
    B, N, M = 4, 200, 257
    src, tar = clouds(B, N, M, C1, C2, seed=45)
    kw = dict(tol_rot=1e-2, tol_trans=1e-2, patience=2, level_cap=3)
    a = icp.RobustIcpRegistration(src, tar, counts1=C1, counts2=C2, **kw).run(12)
    b = icp.RobustIcpRegistration(src, tar, counts1=C1, counts2=C2, **kw).run(12)
    torch.cuda.synchronize()
    for f in FIELDS[1:]:
        assert bits(getattr(a, f)) == bits(getattr(b, f)), f
    assert (a.levels >= 1)[:3].all()
    for s in range(B):
        own = icp.RobustIcpRegistration(src[s:s + 1], tar[s:s + 1], counts1=C1[s:s + 1], counts2=C2[s:s + 1], **kw).run(12)
        for f in ("R", "T", "nu", "nu_end", "level", "state", "med_sq", "med_info"):
            assert bits(getattr(a, f)[s]) == bits(getattr(own, f)[0]), (s, f)
        assert bits(a.weights[s, :C1[s]]) == bits(own.weights[0, :C1[s]]), s
        assert not a.weights[s, C1[s]:].any()


# ---- 7. one epoch against the float64 twin -----------------------------------------------------------------------------------
def test_epochs_against_the_twin_from_the_devices_keys(mods):
    _, icp, _ = mods
    B, N, M = 3, 200, 260
    c1, c2 = [200, 150, 64], [260, 130, 260]
    src, tar = clouds(B, N, M, c1, c2, seed=40, rot_deg=10.0)
    xi0 = torch.tensor([[0.0] * 6, [0.05, -0.02, 0.03, 0.01, 0.0, -0.01], [0.0, 0.04, 0.0, 0.0, 0.02, 0.0]])
    reg = icp.RobustIcpRegistration(src, tar, counts1=c1, counts2=c2, xi0=xi0, tol_rot=1e-2, tol_trans=1e-2, patience=2, level_cap=2)
    hs, ht = src.cpu().numpy(), tar.cpu().numpy()
    ends, tol_t = reg.nu_end.cpu().numpy(), reg.tol_trans.cpu().numpy()
    # nu_end = None: the target's lower median nearest-neighbour spacing over 3 sqrt(3)
    for b in range(B):
        want = RR.nu_end_ref(ht[b, :c2[b]])
        assert abs(float(ends[b]) - want) <= 4 * 2.0 ** -24 * want, (b, ends[b], want)
    for e in range(4):
        R0, T0 = reg.R.cpu().numpy(), reg.T.cpu().numpy()
        st0, lv0, nu0 = reg.state.cpu().tolist(), reg.level.cpu().tolist(), reg.nu.cpu().numpy()
        reg.epoch()
        torch.cuda.synchronize()
        keys, R1, T1, w1 = host_keys(reg.best_x), reg.R.cpu().numpy(), reg.T.cpu().numpy(), reg.weights.cpu().numpy()
        for b in range(B):
            f, w, Rn, Tn, _, st, lv, nu = RR.robust_epoch_from_keys(hs[b], ht[b], keys[b], R0[b], T0[b], st0[b], lv0[b], nu0[b], ends[b], e == 0,
                                                                    c1[b], c2[b], 3.0, 0.5, 2, 1e-2, tol_t[b], 2)
            big = max(1.0, float(np.nanmax(np.abs(hs[b, :c1[b]]))), float(np.nanmax(np.abs(ht[b, :c2[b]]))))
            assert f["info"][1] == KR.FIT_OK and reg.info[b].tolist() == f["info"], (e, b)
            assert np.abs(R1[b] - Rn).max() <= 2.0 ** -22 * big and np.abs(T1[b] - Tn).max() <= 2.0 ** -22 * big, (e, b)
            assert np.abs(w1[b].astype(np.float64) - w).max() <= 2.0 ** -24, (e, b)
            assert reg.state[b].tolist() == st and reg.level[b].tolist() == lv and reg.nu[b].item() == float(nu), (e, b, st, lv, nu)
    assert (reg.levels >= 1).all()


# ---- 8. what the loop is for --------------------------------------------------------------------------------------------------
def test_outlier_pairs_are_registered(mods):
    """outlier_pair(seed, 256, 10 degrees, 20 % outliers), seeds 0 .. 7, as one batch with the defaults: every pair done within 60
    epochs, within 0.05 degrees of the generating rotation (the float64 twin: <= 0.003 degrees; the bound leaves the float32
    path and the tie rule a factor 8 and more); IcpRegistration on the same batch ends at least five times farther on every pair
    (twin: 0.5 ... 1.5 degrees)."""
    _, icp, _ = mods
    pairs = [RR.outlier_pair(seed, 256, 10.0, 0.2) for seed in range(8)]
    src, tar = dev(np.stack([p[0] for p in pairs])), dev(np.stack([p[1] for p in pairs]))
    rob = icp.RobustIcpRegistration(src, tar).run(60)
    plain = icp.IcpRegistration(src, tar).run(100)
    torch.cuda.synchronize()
    Rr, Rp = rob.R.cpu().numpy(), plain.R.cpu().numpy()
    err = [RR.rot_err_deg(Rr[b], pairs[b][2]) for b in range(8)]
    err_plain = [RR.rot_err_deg(Rp[b], pairs[b][2]) for b in range(8)]
    print("robust", err, "epochs", rob.done_epoch.tolist(), "levels", rob.levels.tolist(), "plain", err_plain, plain.done_epoch.tolist())
    done = rob.done_epoch.tolist()
    assert all(0 < d <= 60 for d in done), done
    assert all(e <= 0.05 for e in err), err
    assert all(p >= 5.0 * e for p, e in zip(err_plain, err)), (err, err_plain)
    assert (rob.levels >= 1).all() and bits(rob.nu) == bits(rob.nu_end)
    assert (rob.failed == KR.ICP_DONE).all()
    R, T, history = icp.robust_icp_pairs(src[:2], tar[:2], n_epoch=80, check_every=10)
    assert bits(R) == bits(rob.R[:2]) and bits(T) == bits(rob.T[:2]) and len(history) == 2 and len(history[0]) < 80


# ---- 9. graph capture ---------------------------------------------------------------------------------------------------------
def test_steady_epoch_in_a_captured_graph(mods):
    """No host read-back: after the first (init) epoch, the steady epoch replays from a graph with the bits of the plain calls."""
    _, icp, _ = mods
    src, tar = clouds(2, 257, 200, seed=80)
    kw = dict(tol_rot=1e-2, tol_trans=1e-2, patience=2, level_cap=3)
    eager = icp.RobustIcpRegistration(src, tar, **kw).run(6)
    reg = icp.RobustIcpRegistration(src, tar, **kw)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        reg.epoch()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        reg.epoch()
    for _ in range(5):
        graph.replay()
    torch.cuda.synchronize()
    for f in ("R", "T", "nu", "level", "weights", "state", "fit"):
        assert bits(getattr(reg, f)) == bits(getattr(eager, f)), f
    assert reg.state[:, 0].tolist() == [6, 6] and (reg.levels >= 1).all()
