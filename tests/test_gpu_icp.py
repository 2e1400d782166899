"""The ICP epoch on the GPU (include/rrl.h rrl_icp_step_batch, rrl_icp_epoch; rrl_hip/icp.py).

1. One rrl_icp_epoch call == rrl_rigid_apply_fwd + rrl_chamfer_tree_fwd_counted + rrl_kabsch_fwd + rrl_icp_step_batch, bit for
   bit, epoch after epoch: moved, keys, values, fit, info, (Rk, Tk), (R, T), state, last_step, the table and the cursor.
2. rrl_icp_step_batch against the twin's rule (tests/kabsch_refs.py) on cases well away from the thresholds.
3. A done pair's pose is frozen; a pair whose fit has status 1 or 2 keeps its pose and `failed` says so.
4. With unit weights and no gate, per pair and epoch: res_after <= key_mean (the previous pose is feasible for the fit) and the
   next epoch's key_mean <= res_after (nearest neighbours only come closer), each with 8 2^-24 max|coordinate| sqrt(key_mean)
   of slack for the float32 rounding of the moved points."""
import ctypes

import numpy as np
import pytest
import torch

import kabsch_refs as KR

pytestmark = pytest.mark.gpu

B3, N3, M3 = 3, 200, 260
C1, C2 = [200, 150, 64], [260, 130, 260]
SHAPES = {"ragged-3x200x260": (B3, N3, M3, C1, C2), "full-2x257x200": (2, 257, 200, None, None)}


@pytest.fixture(scope="module")
def mods():
    from rrl_hip import _lib, icp, ops
    _lib.load()
    assert torch.cuda.is_available()
    return _lib, icp, ops


def clouds(B, N, M, c1=None, c2=None, seed=40, rot_deg=15.0, nine=False):
    """synth.make_pair point clouds stacked to (B, N, 3), (B, M, 3) (nine: pseudo-triangles (.., 9)); rows beyond a count NaN."""
    from rrl_hip import synth
    k = 9 if nine else 3
    src, tar = np.full((B, N, k), np.nan, np.float32), np.full((B, M, k), np.nan, np.float32)
    for b in range(B):
        nb, mb = (N if c1 is None else c1[b]), (M if c2 is None else c2[b])
        pr = synth.make_pair(seed + b, max(nb, 3), max(mb, 3), rot_deg=rot_deg)
        src[b, :nb], tar[b, :mb] = pr["src_tri" if nine else "src"][:nb], pr["tar_tri" if nine else "tar"][:mb]
    return torch.from_numpy(src).cuda(), torch.from_numpy(tar).cuda()


def bits(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


def composed_epoch(_lib, ops, r):
    """One epoch on IcpRegistration r's buffers from the four public entries."""
    P, dev = ops._p, r.dev
    ops._run(dev, "rrl_rigid_apply_fwd", P(r.src), P(r.R), P(r.T), P(r.moved), r.B, r.N, 0, 0)
    ops._run(dev, "rrl_chamfer_tree_fwd_counted", P(r.moved), P(r.tar), P(r.counts1), P(r.counts2), P(r.cham_ws), r.cham_ws.numel(),
             P(r.best_x), P(r.best_y), P(r.value), None, r.B, r.N, r.M, P(r.order_x), P(r.order_y))
    k = _lib.KabschArgs()
    k.struct_bytes = ctypes.sizeof(k)
    k.B, k.n, k.m, k.a_stride, k.b_stride, k.transpose_r = r.B, r.N, r.M, 3, 3, 0
    k.a, k.b, k.w, k.keys, k.count_a, k.count_b, k.gate_sq = P(r.src), P(r.tar), None, P(r.best_x), P(r.counts1), P(r.counts2), P(r.gate_sq)
    k.eps_w, k.rank_tol = 0.0, r._args.rank_tol
    k.part, k.part_bytes, k.R, k.T, k.fit, k.info = P(r.part), r.part.numel() * 8, P(r.Rk), P(r.Tk), P(r.fit), P(r.info)
    ops._run(dev, "rrl_kabsch_fwd", ctypes.byref(k))
    ops._run(dev, "rrl_icp_step_batch", P(r.Rk), P(r.Tk), P(r.info), P(r.fit), P(r.R), P(r.T), P(r.tol_rot), P(r.tol_trans), r.patience,
             P(r.value), P(r.table), P(r.cursor), r.table.shape[0], P(r.row), P(r.last_step), P(r.state), r.B)


FIELDS = ("moved", "best_x", "best_y", "value", "fit", "info", "Rk", "Tk", "R", "T", "state", "last_step", "table", "cursor", "row")


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("gated", [False, True])
def test_one_call_equals_the_four_entries(mods, shape, gated):
    _lib, icp, ops = mods
    B, N, M, c1, c2 = SHAPES[shape]
    src, tar = clouds(B, N, M, c1, c2)
    kw = dict(counts1=c1, counts2=c2, max_dist=0.05 if gated else None, tol_rot=1e-3, tol_trans=1e-3, patience=2, table_rows=4)
    one, four = icp.IcpRegistration(src, tar, **kw), icp.IcpRegistration(src, tar, **kw)
    for e in range(6):
        one.epoch()
        composed_epoch(_lib, ops, four)
        torch.cuda.synchronize()
        for f in FIELDS:
            x, y = getattr(one, f), getattr(four, f)
            if f == "moved" and c1 is not None:  # (rows beyond a count are NaN filler moved: compare what a sample has)
                x, y = [x[b, :c1[b]] for b in range(B)], [y[b, :c1[b]] for b in range(B)]
                assert all(bits(p) == bits(q) for p, q in zip(x, y)), (e, f)
            else:
                assert bits(x) == bits(y), (e, f)
    assert one.cursor.tolist() == [6] * B and one.state[:, 0].tolist() == [6] * B
    assert (one.info[:, 0] > 0).all() and (gated or (one.info[:, 1] == 0).all())
    h = one.history()
    assert len(h) == B and len(h[0]) == 4 and h[0][0][0] == 0 and h[0][3][1] is not None and h[0][3][2] > 0


def rodrigues_rows(axis, th):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return (np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K).T


def test_step_against_the_twin_rule(mods):
    """Five pairs: a 0.3 rad step (not calm), a 1e-6 rad step that completes the patience (done now), a 2e-3 rad step that
    resets a calm count, a fit of status 1, a pair that was done before.  Tolerances 1e-3: every decision is a factor 2 or
    more from its threshold.  state and the committed pose exactly; last_step within 2^-23 of the twin's (its float32
    rounding), the log row and cursor as rrl_se3_adam_step_batch logs."""
    _lib, icp, ops = mods
    B, patience, tol = 5, 3, 1e-3
    rs = np.random.default_rng(3)
    R0 = np.stack([rodrigues_rows(rs.standard_normal(3), 0.5) for _ in range(B)]).astype(np.float32)
    T0 = rs.standard_normal((B, 3)).astype(np.float32)
    steps = [0.3, 1e-6, 2e-3, 0.1, 0.1]
    Rk = np.stack([(R0[b].astype(np.float64) @ rodrigues_rows(rs.standard_normal(3), steps[b])) for b in range(B)]).astype(np.float32)
    Tk = (T0 + np.array([[0.2, 0, 0], [1e-7, 0, 0], [0, 0, 0], [0.1, 0, 0], [0.1, 0, 0]], np.float32)).astype(np.float32)
    fit = np.zeros((B, 32))
    fit[:, 1:4] = rs.standard_normal((B, 3)) * 1e-3  # centroids near the origin: the rotation barely moves them
    fit[:, 29] = [0.5, 0.25, 0.125, 0.0625, 0.03125]
    info = np.zeros((B, 4), np.int32)
    info[3, 1] = KR.FIT_FEW
    state = np.array([[4, 0, -1, 0], [4, 2, -1, 0], [4, 2, -1, 0], [4, 1, -1, 0], [9, 3, 7, 0]], np.int32)
    value = np.arange(1, B + 1, dtype=np.float32)
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    tR, tT, tRk, tTk, tfit, tinfo, tstate, tvalue = d(R0), d(T0), d(Rk), d(Tk), d(fit), d(info), d(state), d(value)
    tols = torch.full((B,), tol, device="cuda")
    table, cursor = torch.zeros(3, B, 3, device="cuda"), torch.tensor([0, 1, 2, 3, 1], dtype=torch.int64, device="cuda")
    row, last = torch.zeros(B, 3, device="cuda"), torch.full((B, 2), -1.0, device="cuda")
    P = ops._p
    ops._run(tR.device, "rrl_icp_step_batch", P(tRk), P(tTk), P(tinfo), P(tfit), P(tR), P(tT), P(tols), P(tols), patience, P(tvalue),
             P(table), P(cursor), 3, P(row), P(last), P(tstate), B)
    torch.cuda.synchronize()
    want_state = [[5, 0, -1, 0], [5, 3, 5, 0], [5, 0, -1, 0], [5, 0, -1, KR.FIT_FEW], [10, 3, 7, KR.ICP_DONE]]
    for b in range(B):
        Rn, Tn, ls, st = KR.icp_step(Rk[b], Tk[b], int(info[b, 1]), fit[b, 1:4], R0[b], T0[b], state[b].tolist(), tol, tol, patience)
        assert st == want_state[b] and tstate[b].tolist() == st, (b, st, tstate[b].tolist())
        assert bits(tR[b]) == Rn.tobytes() and bits(tT[b]) == Tn.tobytes(), b
        if ls is None:
            assert last[b].tolist() == [-1.0, -1.0]
        else:
            for got, ref in zip(last[b].tolist(), ls):
                assert abs(got - ref) <= 2.0 ** -23 * abs(ref) + 1e-12, (b, got, ref)
        ok = float(info[b, 1] == 0)
        assert row[b].tolist() == [float(np.float32(fit[b, 29])), float(value[b]), ok]
    assert cursor.tolist() == [1, 2, 3, 4, 2]
    assert table[0, 0].tolist() == row[0].tolist() and table[1, 1].tolist() == row[1].tolist() and table[2, 2].tolist() == row[2].tolist()
    assert table[1, 4].tolist() == row[4].tolist() and not table[:, 3].any()  # (pair 3's cursor is past the table: unlogged)


def test_done_pairs_freeze_and_failed_pairs_keep_their_pose(mods):
    """Pair 1 has two source points (status 1), pair 2 a collinear source (status 2): both keep the starting pose and say so;
    pair 0 converges, is declared done, and its pose keeps its bits from then on while the epochs go on."""
    _lib, icp, ops = mods
    src, tar = clouds(3, 128, 160, [128, 2, 128], [160, 160, 160], seed=50, rot_deg=10.0)
    line = torch.linspace(-1, 1, 128, device="cuda")[:, None] * torch.tensor([[0.5, 0.25, -0.125]], device="cuda")
    src[2] = line
    tar[2] = torch.linspace(-1, 1, 160, device="cuda")[:, None] * torch.tensor([[0.5, 0.25, -0.125]], device="cuda") + 0.01
    xi0 = torch.tensor([[0.0] * 6, [0.1, 0.0, 0.0, 0.01, 0.0, 0.0], [0.0, 0.1, 0.0, 0.0, 0.0, 0.0]])
    reg = icp.IcpRegistration(src, tar, counts1=[128, 2, 128], counts2=[160, 160, 160], xi0=xi0, tol_rot=1e-4, tol_trans=1e-5, patience=3)
    R_start, T_start = reg.R.clone(), reg.T.clone()
    reg.run(80, check_every=1000)
    done = reg.done_epoch.tolist()
    assert 3 <= done[0] < 80 and done[1] == -1 and done[2] == -1, done
    assert reg.failed.tolist() == [KR.ICP_DONE, KR.FIT_FEW, KR.FIT_DEGENERATE]
    assert bits(reg.R[1:]) == bits(R_start[1:]) and bits(reg.T[1:]) == bits(T_start[1:])
    assert reg.info[1, 0].item() == 2 and reg.info[1, 3].item() == 126
    R_done, T_done = reg.R[0].clone(), reg.T[0].clone()
    reg.run(5)
    assert bits(reg.R[0]) == bits(R_done) and bits(reg.T[0]) == bits(T_done) and reg.done_epoch.tolist() == done
    assert reg.state[:, 0].tolist() == [85] * 3
    h = reg.history()
    assert h[1][0] == (0, None, None) and h[0][0][1] is not None
    mp = reg.moved_points()
    want = reg.src[0].double() @ reg.R[0].double() + reg.T[0].double()
    assert (mp[0].double() - want).abs().max() <= 4 * 2.0 ** -24 * (3 ** 0.5 * float(reg.src[0].abs().max()) + float(reg.T[0].abs().max()))


@pytest.mark.parametrize("shape", list(SHAPES))
def test_epoch_inequalities(mods, shape):
    _lib, icp, ops = mods
    B, N, M, c1, c2 = SHAPES[shape]
    nine = shape.startswith("full")  # (pseudo-triangles in: their first points are the clouds)
    src, tar = clouds(B, N, M, c1, c2, seed=70, rot_deg=25.0, nine=nine)
    reg = icp.IcpRegistration(src, tar, counts1=c1, counts2=c2, patience=0)
    big0 = max(float(torch.nan_to_num(src[..., :3]).abs().max()), float(torch.nan_to_num(tar[..., :3]).abs().max()))
    res_prev = None
    for e in range(10):
        reg.epoch()
        fit = reg.fit.cpu().numpy()
        res, key = fit[:, 29], fit[:, 30]
        big = max(big0, float(torch.nan_to_num(reg.moved).abs().max()))  # the largest |coordinate| among given and moved points
        slack = 8 * 2.0 ** -24 * big * np.sqrt(key)
        assert (reg.info[:, 1] == 0).all() and (key > 0).all()
        assert (res <= key + slack).all(), (e, res, key)
        if res_prev is not None:
            assert (key <= res_prev + slack).all(), (e, key, res_prev)
        res_prev = res
    assert (reg.done_epoch == -1).all() and (reg.failed == 0).all()
