"""Point-to-plane ICP on the GPU (include/rrl.h rrl_idx_normals, rrl_plane_normal_eq, rrl_plane_step_batch, rrl_plane_icp_epoch;
rrl_hip/neighbors.py estimate_normals, rrl_hip/icp.py PlaneIcpRegistration) against the float64 twins of
tests/plane_refs.py.

Bounds, from the arithmetic rule (fixed-order double sums of float32 inputs, double eigen-decomposition and Cholesky, one rounding
to float32), none taken from what the kernels give:
- normals: a zero row of the twin is a zero row of the device, exactly; every other row within 2^-22 per component (one float32
  rounding of a unit vector is 2^-25; the double errors, 1e-16 / quality, are orders below at quality >= 1e-2).  Rows whose twin
  quality is below 1e-2 would be excluded; the clouds and radii below have none, so the cap on excluded rows is 0;
- sums: counts and info exactly; each of the 29 real sums within N 2^-53 sum|terms| of the twin (the terms themselves are the
  same double expressions on both sides; only the order of the additions differs); a neq entry is its sum divided by W, one more
  rounding;
- step: the twin step fed the device's own neq gives R and T within 2^-23 max(1, |T|_inf) per entry;
- epoch: one call == the four entries, bit for bit; two runs give the same bits; sample b of a ragged batch has the bits of its
  own B = 1 loop;
- exact pairs: after 12 epochs max |src R + T - tar| <= 8 2^-23 max|coordinate|;
- against IcpRegistration: closer to the generating rotation after 10 epochs than it is after 30, on at least 7 of 8 pairs."""
import ctypes

import numpy as np
import pytest
import torch

import newton_refs as NR
import plane_refs as PR
from test_plane_refs_host import lattice

pytestmark = pytest.mark.gpu

U22, U23, U53 = 2.0 ** -22, 2.0 ** -23, 2.0 ** -53
QUALITY_MIN = 1e-2
# the radius per (n, nsample): chosen on the TWIN so that the shapes together hold rows with fewer than three members, partly
# filled rows and truncated rows, and no row's quality is below QUALITY_MIN
RADII = {(1, 3): 1.5, (1, 8): 1.5, (1, 64): 1.5, (2, 3): 1.5, (2, 8): 1.5, (2, 64): 1.5, (3, 3): 1.5, (3, 8): 1.5, (3, 64): 1.5,
         (63, 3): 1.5, (63, 8): 0.6, (63, 64): 0.6, (64, 3): 1.5, (64, 8): 0.5, (64, 64): 0.5, (65, 3): 1.5, (65, 8): 0.45, (65, 64): 0.45,
         (257, 3): 1.5, (257, 8): 0.35, (257, 64): 0.7}


@pytest.fixture(scope="module")
def mods():
    from rrl_hip import _lib, icp, neighbors, ops
    _lib.load()
    assert torch.cuda.is_available()
    return _lib, icp, neighbors, ops


def cuda(*xs):
    return tuple(torch.from_numpy(np.ascontiguousarray(x)).cuda() if x is not None else None for x in xs)


def bits(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


def surface(n, B, base=200):
    from rrl_hip import synth
    return np.stack([synth.surface_cloud(base + n + 1000 * b, n) for b in range(B)])


def check_normals(got_n, got_q, twin, what):
    """Device normals / quality (numpy) against the twin's dict: zero rows exactly, the others within 2^-22, none excluded."""
    tn, tq = twin["normals"], twin["quality"]
    zero = ~tn.any(-1)
    assert not got_n[zero].any() and not got_q[zero].any(), (what, "zero rows")
    excluded = (~zero) & (tq < QUALITY_MIN)
    assert excluded.sum() == 0, (what, "rows below the quality floor", int(excluded.sum()), tq[~zero].min())
    live = ~zero
    if live.any():
        err = np.abs(got_n[live].astype(np.float64) - tn[live]).max()
        print(f"{what}: {int(live.sum())} rows, worst normal error {err / U22:.3f} of 2^-22, least quality {tq[live].min():.4f}")
        assert err <= U22, (what, err / U22)
        assert np.abs(got_q[live] - tq[live]).max() <= 1e-6, what


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("nsample", [3, 8, 64])
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 257])
def test_normals_against_the_twin(mods, n, nsample, B):
    _, _, nb, _ = mods
    x = surface(n, B)
    radius = RADII[(n, nsample)]
    twin = PR.estimate_normals(x, radius, nsample)
    assert not twin["border"].any()
    (tx,) = cuda(x)
    normals, quality = nb.estimate_normals(tx, radius, nsample, return_quality=True)
    idx, found = nb.ball_query(tx, radius, nsample, exclude_self=False)
    assert np.array_equal(idx.cpu().numpy(), twin["idx"]) and np.array_equal(found.cpu().numpy(), twin["found"])
    check_normals(normals.cpu().numpy(), quality.cpu().numpy(), twin, (n, nsample, B))
    if (n, nsample, B) == (65, 8, 3):  # the three kinds of rows are all there
        f = twin["found"]
        assert (f < 3).any() and ((f >= 3) & (f < nsample)).any() and (f == nsample).any()
    if n < 3:
        assert not normals.any()


def test_normals_special_rows(mods):
    """The z = 0 lattice: exactly (0, 0, 1).  Duplicated points and a line: no plane.  A NaN point inside the count: it is a
    member of no row and its own row is zero, the others keep their normals.  Ragged counts (0 and 1 among them) with NaN beyond."""
    _, _, nb, _ = mods
    lat = lattice(6, 5)[None]
    (tl,) = cuda(lat)
    nl = nb.estimate_normals(tl, 0.3, 16)
    assert torch.equal(nl.cpu(), torch.tensor([0.0, 0.0, 1.0]).expand(1, 30, 3))
    dup = np.repeat(lat[:, :1], 5, 1)
    line = (np.arange(12)[:, None] * np.array([[0.25, 0.0, 0.0]])).astype(np.float32)[None]
    assert not nb.estimate_normals(cuda(dup)[0], 0.5, 8).any() and not nb.estimate_normals(cuda(line)[0], 0.6, 8).any()
    x = surface(130, 1)
    x[0, 17, 2] = np.nan
    twin = PR.estimate_normals(x, 0.5, 64)
    n, q = nb.estimate_normals(cuda(x)[0], 0.5, 64, return_quality=True)
    assert not twin["normals"][0, 17].any() and twin["normals"][0].any(-1).sum() >= 120
    check_normals(n.cpu().numpy(), q.cpu().numpy(), twin, "a NaN point")
    B, cap = 4, 65
    counts = [65, 0, 1, 40]
    xr = surface(cap, B, base=800)
    for b, c in enumerate(counts):
        xr[b, c:] = np.nan
    twin = PR.estimate_normals(xr, 0.45, 16, counts=counts)
    for cnt in (counts, torch.tensor(counts, dtype=torch.int32, device="cuda")):
        n, q = nb.estimate_normals(cuda(xr)[0], 0.45, 16, counts=cnt, return_quality=True)
        check_normals(n.cpu().numpy(), q.cpu().numpy(), twin, "ragged")
        assert not n[1].any() and not n[2].any() and not n[3, 40:].any() and n[3, :40].any()
    own = nb.estimate_normals(cuda(xr[3:4, :40])[0], 0.45, 16)
    assert bits(n[3, :40]) == bits(own[0])  # sample b of a ragged batch has the bits of its own call


def test_normals_outputs_have_borders_and_repeat_their_bits(mods):
    """Sentinels around normals and quality survive the launch; a second call and a captured graph give the same bits."""
    _lib, _, nb, ops = mods
    B, n, k = 2, 131, 16
    (tx,) = cuda(surface(n, B, base=900))
    idx, found = nb.ball_query(tx, 0.4, k, exclude_self=False)
    first = nb.estimate_normals(tx, 0.4, k, return_quality=True)
    pad = 64
    big_n = torch.full((B * n * 3 + 2 * pad,), 7.0, device="cuda")
    big_q = torch.full((B * n + 2 * pad,), 7.0, device="cuda")
    out_n, out_q = big_n[pad:pad + B * n * 3], big_q[pad:pad + B * n]
    P = ops._p
    ops._run(tx.device, "rrl_idx_normals", P(tx), 3, P(idx), P(found), None, k, nb.NORMAL_RANK_TOL, P(out_n), P(out_q), B, n, n)
    torch.cuda.synchronize()
    assert bits(out_n) == bits(first[0]) and bits(out_q) == bits(first[1])
    for big in (big_n, big_q):
        assert (big[:pad] == 7).all() and (big[-pad:] == 7).all()
    # a wider stride reads the same points: pseudo-triangle rows in place
    wide = torch.zeros(B, n, 9, device="cuda")
    wide[:, :, :3] = tx
    out9 = torch.empty(B, n, 3, device="cuda")
    ops._run(tx.device, "rrl_idx_normals", P(wide), 9, P(idx), P(found), None, k, nb.NORMAL_RANK_TOL, P(out9), None, B, n, n)
    assert bits(out9) == bits(first[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        nb.estimate_normals(tx, 0.4, k, return_quality=True)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = nb.estimate_normals(tx, 0.4, k, return_quality=True)
    for _ in range(2):
        for o in outs:
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for o, want in zip(outs, first):
            assert bits(o) == bits(want)


# ---- the sums ---------------------------------------------------------------------------------------------------------------------
def unit(rs, shape):
    v = rs.standard_normal(shape)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def run_normal_eq(mods, moved, tar, normals, keys=None, c1=None, c2=None, w=None, gate=None, pivot=None):
    """rrl_plane_normal_eq on numpy inputs -> (neq (B, 32), info (B, 4), raw sums (B, 32): the partial rows added in index order)."""
    _lib, _, _, ops = mods
    lib = _lib.load()
    B, N, M = moved.shape[0], moved.shape[1], tar.shape[1]
    tm, tt, tn, tw, tg, tp = cuda(moved, tar, normals, w, gate, pivot)
    tk = None if keys is None else torch.from_numpy(keys.view(np.int64)).cuda()
    i32 = lambda c: None if c is None else torch.tensor(c, dtype=torch.int32, device="cuda")  # noqa: E731
    tc1, tc2 = i32(c1), i32(c2)
    nblk = (N + 511) // 512
    part = torch.full((B * nblk * 32 + 16,), 7.0, dtype=torch.float64, device="cuda")
    neq = torch.full((B * 32 + 16,), 7.0, dtype=torch.float64, device="cuda")
    info = torch.full((B * 4 + 16,), 7, dtype=torch.int32, device="cuda")
    P = ops._p
    a = _lib.PlaneArgs()
    a.struct_bytes = ctypes.sizeof(a)
    a.B, a.N, a.M, a.tar_stride = B, N, M, tar.shape[2]
    a.moved, a.keys, a.tar, a.normals, a.count1, a.count2 = P(tm), P(tk), P(tt), P(tn), P(tc1), P(tc2)
    a.w, a.gate_sq, a.pivot = P(tw), P(tg), P(tp)
    a.part, a.part_bytes, a.neq, a.info = P(part), int(lib.rrl_plane_part_bytes(B, N)), P(neq), P(info)
    assert a.part_bytes == B * nblk * 32 * 8
    outs = []
    for _ in range(2):
        ops._run(tm.device, "rrl_plane_normal_eq", ctypes.byref(a))
        torch.cuda.synchronize()
        outs.append((bits(neq), bits(info), bits(part)))
    assert outs[0] == outs[1]  # the same bits on every call
    assert (part[-16:] == 7).all() and (neq[-16:] == 7).all() and (info[-16:] == 7).all()  # nothing beyond the outputs
    raw = part[:-16].reshape(B, nblk, 32).cpu().numpy()
    tot = np.zeros((B, 32))
    for k in range(nblk):
        tot = tot + raw[:, k]
    return neq[:-16].reshape(B, 32).cpu().numpy(), info[:-16].reshape(B, 4).cpu().numpy(), tot


def check_sums(neq, info, raw, twin, N, what):
    """One sample against the twin: counts and info exactly, the 29 real sums (and the key sum) within N 2^-53 sum|terms|, neq =
    the sums over W rounded once."""
    assert info.tolist() == twin["info"], (what, info.tolist(), twin["info"])
    assert raw[PR.USED] == twin["sums"][PR.USED] and raw[PR.SKIPPED] == twin["sums"][PR.SKIPPED]
    assert neq[PR.USED] == twin["info"][0] and neq[PR.SKIPPED] == twin["info"][3]
    real = list(range(PR.W_ + 1)) + [PR.RES, PR.KEYMEAN]
    lim = N * U53 * twin["terms"][real]
    err = np.abs(raw[real] - twin["sums"][real])
    assert (err <= lim).all(), (what, "sums", np.nanmax(err / np.maximum(lim, 1e-300)))
    W = raw[PR.W_]
    assert neq[PR.W_] == W
    few = twin["info"][1] == PR.FIT_FEW
    for q in real:
        if q == PR.W_:
            continue
        want = 0.0 if few else raw[q] / W
        assert abs(neq[q] - want) <= U53 * abs(want), (what, "neq", q)


@pytest.mark.parametrize("N", [1, 5, 6, 7, 64, 65, 511, 512, 513, 1025])
def test_sums_against_the_twin(mods, N):
    """Handcrafted keys (all-ones, an index >= M, an index >= count2), a gate, weights, zero and NaN normals, a 9-wide target,
    M != N, ragged counts with NaN beyond them; sample 0 is full and unweighted."""
    rs = np.random.default_rng(5000 + N)
    B, M = 3, N + 3
    c1, c2 = [N, max(N - 2, 0), N], [M, M, max(M - 4, 1)]
    moved = rs.uniform(-1, 1, (B, N, 3)).astype(np.float32)
    tar = rs.uniform(-1, 1, (B, M, 9)).astype(np.float32)
    normals = unit(rs, (B, M, 3))
    normals[:, 1::11] = 0.0
    normals[:, 2::13, 1] = np.nan
    for b in range(B):
        moved[b, c1[b]:] = np.nan
        tar[b, c2[b]:] = np.nan
        normals[b, c2[b]:] = np.nan
    idx = rs.integers(0, M, (B, N)).astype(np.uint64)
    dist = rs.uniform(0.0, 1.0, (B, N)).astype(np.float32)
    keys = (dist.view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx
    if N >= 64:
        keys[:, 5::17] = np.uint64(PR.ALL_ONES)
        keys[:, 3::29] = (keys[:, 3::29] & ~np.uint64(0xFFFFFFFF)) | np.uint64(M + 5)
        keys[:, 7::31] = (keys[:, 7::31] & ~np.uint64(0xFFFFFFFF)) | np.uint64(0xFFFFFFFE)
    w = rs.uniform(0.1, 1.0, (B, N)).astype(np.float32)
    w[0] = 1.0
    gate = np.array([2.0, 0.75, 0.5], np.float32)
    pivot = rs.uniform(-0.5, 0.5, (B, 3)).astype(np.float32)
    neq, info, raw = run_normal_eq(mods, moved, tar, normals, keys, c1, c2, w, gate, pivot)
    for b in range(B):
        twin = PR.normal_eq(moved[b], tar[b], normals[b], keys[b], c1[b], c2[b], w[b], gate[b], pivot[b])
        check_sums(neq[b], info[b], raw[b], twin, N, (N, b))
    if N >= 64:
        assert (info[:, 3] > 0).all() and (info[:, 0] > 0).all() and info[1, 3] >= 2
    if N < 6:
        assert (info[:, 1] == PR.FIT_FEW).all()
    if N >= 64:
        assert (info[:, 1] == PR.FIT_OK).all()
    # dense pairs (no keys, M == N), no pivot, no gate, no weights
    neq, info, raw = run_normal_eq(mods, moved, tar[:, :N], normals[:, :N], None, c1, [min(c, N) for c in c2])
    for b in range(B):
        twin = PR.normal_eq(moved[b], tar[b, :N], normals[b, :N], None, c1[b], min(c2[b], N))
        check_sums(neq[b], info[b], raw[b], twin, N, (N, b, "dense"))


def test_sums_about_a_pivot_far_from_the_origin(mods):
    """Unit clouds 1000 from the origin, the pivot among them: the sums keep their bound, and H stays as well conditioned as
    it is at the origin (about the origin its rotation block would be a million times its translation block)."""
    rs = np.random.default_rng(8)
    B, N = 2, 700
    off = np.array([1000.0, -1000.0, 500.0])
    moved0 = rs.uniform(-1, 1, (B, N, 3))
    tar0 = moved0 + 0.01 * rs.standard_normal((B, N, 3))
    moved, tar = (moved0 + off).astype(np.float32), (tar0 + off).astype(np.float32)
    normals = unit(rs, (B, N, 3))
    pivot = np.broadcast_to(off.astype(np.float32), (B, 3)).copy()
    neq, info, raw = run_normal_eq(mods, moved, tar, normals, pivot=pivot)
    for b in range(B):
        twin = PR.normal_eq(moved[b], tar[b], normals[b], pivot=pivot[b])
        check_sums(neq[b], info[b], raw[b], twin, N, ("far", b))
        H, _ = PR.unpack(neq[b])
        assert np.linalg.cond(H) < 100.0


# ---- the step -------------------------------------------------------------------------------------------------------------------
def test_step_against_the_twin_on_the_device_sums(mods):
    """Six pairs: a free step, a clamped step, a step that completes the patience (done now), a pair done before (frozen bit for
    bit), fewer than six pairs (pose kept), all normals equal (singular: pose kept)."""
    _lib, _, _, ops = mods
    rs = np.random.default_rng(12)
    B, N, patience = 6, 300, 2
    moved = rs.uniform(-1, 1, (B, N, 3)).astype(np.float32)
    tar = (moved + 0.1 * rs.standard_normal((B, N, 3))).astype(np.float32)
    tar[2] = (moved[2] + 1e-6 * rs.standard_normal((N, 3))).astype(np.float32)
    normals = unit(rs, (B, N, 3))
    normals[5] = np.array([0.0, 0.6, 0.8], np.float32)
    c1 = [N, N, N, N, 5, N]
    pivot = rs.uniform(-0.3, 0.3, (B, 3)).astype(np.float32)
    neq, info, _ = run_normal_eq(mods, moved, tar, normals, None, c1, [N] * B, pivot=pivot)
    assert info[:, 1].tolist() == [0, 0, 0, 0, PR.FIT_FEW, 0]
    R0 = np.stack([PR.rodrigues(0.3 * rs.standard_normal(3)).T for _ in range(B)]).astype(np.float32)
    T0 = (5.0 * rs.standard_normal((B, 3))).astype(np.float32)
    state = np.array([[4, 0, -1, 0], [4, 1, -1, 0], [4, 1, -1, 0], [9, 2, 7, 0], [4, 1, -1, 0], [4, 1, -1, 0]], np.int32)
    damping = np.array([1e-2, 1e-2, 0.0, 1e-2, 1e-2, 0.0], np.float32)
    step = np.array([1.0, 1.0, 1.0, 1.0, 1.0, 1.0], np.float32)
    max_rot = np.array([0.2, 1e-3, 0.2, 0.2, 0.2, 0.2], np.float32)
    max_trans = np.array([0.5, 2e-3, 0.5, 0.5, 0.5, 0.5], np.float32)
    tol = np.full(B, 1e-3, np.float32)
    value = np.arange(1, B + 1, dtype=np.float32)
    tneq, tinfo, tpiv, tR, tT, tstate, tdamp, tstep, tmr, tmt, ttol, tval = cuda(neq, info, pivot, R0, T0, state, damping, step, max_rot,
                                                                                 max_trans, tol, value)
    table, cursor = torch.zeros(3, B, 3, device="cuda"), torch.tensor([0, 1, 2, 1, 0, 3], dtype=torch.int64, device="cuda")
    row, last = torch.zeros(B, 3, device="cuda"), torch.full((B, 2), -1.0, device="cuda")
    P = ops._p
    ops._run(tR.device, "rrl_plane_step_batch", P(tneq), P(tinfo), P(tpiv), P(tdamp), P(tstep), P(tmr), P(tmt), P(ttol), P(ttol), patience,
             1e-12, P(tR), P(tT), P(tval), P(table), P(cursor), 3, P(row), P(last), P(tstate), B)
    torch.cuda.synchronize()
    want_status = [PR.STEPPED, PR.STEPPED, PR.STEPPED, PR.DONE, PR.FEW, PR.FAILED]
    want_state = [[5, 0, -1], [5, 0, -1], [5, 2, 5], [10, 2, 7], [5, 0, -1], [5, 0, -1]]
    gotR, gotT = tR.cpu().numpy(), tT.cpu().numpy()
    for b in range(B):
        Rn, Tn, ls, st = PR.step(neq[b], info[b].tolist(), R0[b], T0[b], state[b].tolist(), pivot[b], damping[b], step[b], max_rot[b],
                                 max_trans[b], 1e-12, tol[b], tol[b], patience)
        assert st == want_state[b] + [want_status[b]] and tstate[b].tolist() == st, (b, st, tstate[b].tolist())
        if ls is None:  # the pose keeps its bits
            assert gotR[b].tobytes() == R0[b].tobytes() and gotT[b].tobytes() == T0[b].tobytes() and last[b].tolist() == [-1.0, -1.0], b
        else:
            lim = U23 * max(1.0, np.abs(Tn).max())
            eR, eT = np.abs(gotR[b] - Rn).max(), np.abs(gotT[b] - Tn).max()
            print(f"pair {b}: R error {eR / lim:.3f}, T error {eT / lim:.3f} of 2^-23 max(1, |T|)")
            assert eR <= lim and eT <= lim, (b, eR / lim, eT / lim)
            for got, ref in zip(last[b].tolist(), ls):
                assert abs(got - ref) <= U23 * abs(ref) + 1e-30, (b, got, ref)
        assert row[b].tolist() == [float(np.float32(neq[b, PR.RES])), float(value[b]), float(info[b, 1] == 0)]
    assert last[1].tolist() == [float(max_rot[1]), float(max_trans[1])]  # a clamped length IS the clamp
    assert cursor.tolist() == [1, 2, 3, 2, 1, 4]
    assert table[0, 0].tolist() == row[0].tolist() and table[1, 1].tolist() == row[1].tolist() and table[2, 2].tolist() == row[2].tolist()
    assert table[1, 3].tolist() == row[3].tolist() and not table[:, 5].any()  # (pair 5's cursor is past the table: unlogged)


def test_both_steps_apply_one_composition(mods):
    """rrl_se3_newton_step_batch and rrl_plane_step_batch (no pivot) fed ONE system -- NR.diagonal_neq as the sixteen sums of
    the one, its H and g packed into the 32-double row of the other -- with the same damping, scale, clamps and tolerances, on
    three generic poses, pose 1 clamped in rotation: R, T and last_step leave both with the same bytes, state words 0 .. 2 agree.
    Every given value is exact in float32 (the sums reach the Newton step as floats)."""
    _, _, _, ops = mods
    rs = np.random.default_rng(21)
    B, patience = 3, 2
    lengths = [(0.125, 0.25), (0.5, 0.0625), (0.03125, 0.375)]
    sums = np.stack([NR.diagonal_neq(*x) for x in lengths])
    rows = np.zeros((B, 32))
    for b in range(B):
        H, g = NR.assemble(sums[b])
        rows[b, PR.H0:PR.H0 + 21], rows[b, PR.G0:PR.G0 + 6] = H[np.triu_indices(6)], g
    info = np.zeros((B, 4), np.int32)  # [1] = RRL_FIT_OK
    R0 = np.stack([PR.rodrigues(0.4 * rs.standard_normal(3)).T for _ in range(B)]).astype(np.float32)
    T0 = (3.0 * rs.standard_normal((B, 3))).astype(np.float32)
    state0 = np.array([[4, 1, -1, 0]] * B, np.int32)
    damping, step, max_trans, tol = (np.full(B, v, np.float32) for v in (0.25, 0.5, 1.0, 2.0 ** -10))
    max_rot = np.array([1.0, 0.03125, 1.0], np.float32)
    tsum, trow, tinfo, tdamp, tstep, tmr, tmt, ttol = cuda(sums, rows, info, damping, step, max_rot, max_trans, tol)
    Rn, Tn, sn, Rp, Tp, sp = cuda(R0, T0, state0, R0, T0, state0)
    ln, lp = torch.full((B, 2), -1.0, device="cuda"), torch.full((B, 2), -1.0, device="cuda")
    P = ops._p
    ops.se3_newton_step_batch(tsum, None, Rn, Tn, sn, damping=tdamp, step=tstep, max_rot=tmr, max_trans=tmt, tol_rot=ttol, tol_trans=ttol,
                              patience=patience, eps=1e-12, last_step=ln)
    ops._run(Rp.device, "rrl_plane_step_batch", P(trow), P(tinfo), None, P(tdamp), P(tstep), P(tmr), P(tmt), P(ttol), P(ttol), patience,
             1e-12, P(Rp), P(Tp), None, None, None, 0, None, P(lp), P(sp), B)
    torch.cuda.synchronize()
    assert sn[:, 3].tolist() == [NR.STEPPED] * B and sp[:, 3].tolist() == [PR.STEPPED] * B
    assert bits(Rn) == bits(Rp) and bits(Tn) == bits(Tp) and bits(ln) == bits(lp), (Rn - Rp, Tn - Tp, ln - lp)
    assert torch.equal(sn[:, :3], sp[:, :3]) and sn[:, 0].tolist() == [5] * B
    assert bits(Rn) != R0.tobytes() and bits(Tn) != T0.tobytes()  # (a step was applied)
    assert ln[1, 0].item() == 0.03125 and 0.0 < ln[0, 0].item() < 1.0 and 0.0 < ln[2, 0].item() < 1.0  # pose 1 alone is clamped


# ---- the epoch --------------------------------------------------------------------------------------------------------------------
B3, N3, M3 = 3, 200, 260
C1, C2 = [200, 150, 64], [260, 130, 260]
SHAPES = {"ragged-3x200x260": (B3, N3, M3, C1, C2), "full-2x257x200": (2, 257, 200, None, None)}
FIELDS = ("moved", "best_x", "best_y", "value", "neq", "info", "R", "T", "state", "last_step", "table", "cursor", "row")


def clouds(B, N, M, c1=None, c2=None, seed=40, rot_deg=15.0):
    """synth.make_pair point clouds stacked to (B, N, 3), (B, M, 3); rows beyond a count NaN."""
    from rrl_hip import synth
    src, tar = np.full((B, N, 3), np.nan, np.float32), np.full((B, M, 3), np.nan, np.float32)
    for b in range(B):
        nb, mb = (N if c1 is None else c1[b]), (M if c2 is None else c2[b])
        pr = synth.make_pair(seed + b, max(nb, 3), max(mb, 3), rot_deg=rot_deg)
        src[b, :nb], tar[b, :mb] = pr["src"][:nb], pr["tar"][:mb]
    return torch.from_numpy(src).cuda(), torch.from_numpy(tar).cuda()


def composed_epoch(_lib, ops, r):
    """One epoch on PlaneIcpRegistration r's buffers from the four public entries."""
    P, dev = ops._p, r.dev
    ops._run(dev, "rrl_rigid_apply_fwd", P(r.src), P(r.R), P(r.T), P(r.moved), r.B, r.N, 0, 0)
    ops._run(dev, "rrl_chamfer_tree_fwd_counted", P(r.moved), P(r.tar), P(r.counts1), P(r.counts2), P(r.cham_ws), r.cham_ws.numel(),
             P(r.best_x), P(r.best_y), P(r.value), None, r.B, r.N, r.M, P(r.order_x), P(r.order_y))
    k = _lib.PlaneArgs()
    k.struct_bytes = ctypes.sizeof(k)
    k.B, k.N, k.M, k.tar_stride = r.B, r.N, r.M, 3
    k.moved, k.keys, k.tar, k.normals, k.count1, k.count2 = P(r.moved), P(r.best_x), P(r.tar), P(r.normals), P(r.counts1), P(r.counts2)
    k.w, k.gate_sq, k.pivot = None, P(r.gate_sq), P(r.pivot)
    k.part, k.part_bytes, k.neq, k.info = P(r.part), r.part.numel() * 8, P(r.neq), P(r.info)
    ops._run(dev, "rrl_plane_normal_eq", ctypes.byref(k))
    ops._run(dev, "rrl_plane_step_batch", P(r.neq), P(r.info), P(r.pivot), P(r.damping), P(r.step_scale), P(r.max_rot), P(r.max_trans),
             P(r.tol_rot), P(r.tol_trans), r.patience, r.eps, P(r.R), P(r.T), P(r.value), P(r.table), P(r.cursor), r.table.shape[0],
             P(r.row), P(r.last_step), P(r.state), r.B)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("gated", [False, True])
def test_one_call_equals_the_four_entries(mods, shape, gated):
    """... bit for bit, epoch after epoch, and the sums of an epoch are the twin's on the walk's own keys."""
    _lib, icp, _, ops = mods
    B, N, M, c1, c2 = SHAPES[shape]
    src, tar = clouds(B, N, M, c1, c2)
    kw = dict(normal_radius=0.45, nsample=32, counts1=c1, counts2=c2, max_dist=0.05 if gated else None, tol_rot=1e-3, tol_trans=1e-3,
              patience=2, table_rows=4)
    one, four = icp.PlaneIcpRegistration(src, tar, **kw), icp.PlaneIcpRegistration(src, tar, **kw)
    assert bits(one.normals) == bits(four.normals)
    for e in range(6):
        one.epoch()
        composed_epoch(_lib, ops, four)
        torch.cuda.synchronize()
        for f in FIELDS:
            x, y = getattr(one, f), getattr(four, f)
            if f == "moved" and c1 is not None:  # (rows beyond a count are NaN filler moved: compare what a sample has)
                assert all(bits(x[b, :c1[b]]) == bits(y[b, :c1[b]]) for b in range(B)), (e, f)
            else:
                assert bits(x) == bits(y), (e, f)
        if e == 0:  # keys from a real walk
            moved, keys = one.moved.cpu().numpy(), one.best_x.cpu().numpy().view(np.uint64)
            tn, nn, piv = one.tar.cpu().numpy(), one.normals.cpu().numpy(), one.pivot.cpu().numpy()
            gate = None if one.gate_sq is None else one.gate_sq.cpu().numpy()
            for b in range(B):
                twin = PR.normal_eq(moved[b], tn[b], nn[b], keys[b], None if c1 is None else c1[b], None if c2 is None else c2[b],
                                    None, None if gate is None else gate[b], piv[b])
                got = one.neq[b].cpu().numpy()
                assert one.info[b].tolist() == twin["info"], (b, one.info[b].tolist(), twin["info"])
                lim = N * U53 * twin["terms"][:PR.W_] / twin["sums"][PR.W_] + (N + 2) * U53 * np.abs(twin["neq"][:PR.W_])
                assert (np.abs(got[:PR.W_] - twin["neq"][:PR.W_]) <= lim).all(), b
    assert one.cursor.tolist() == [6] * B and one.state[:, 0].tolist() == [6] * B
    assert (one.info[:, 0] > 0).all() and (gated or (one.info[:, 1] == 0).all())
    h = one.history()
    assert len(h) == B and len(h[0]) == 4 and h[0][0][0] == 0 and h[0][3][1] is not None and h[0][3][2] > 0
    mp = one.moved_points()
    want = one.src[0].double() @ one.R[0].double() + one.T[0].double()
    assert (mp[0].double() - want)[:N if c1 is None else c1[0]].abs().max() <= 1e-6


def test_loop_repeats_its_bits_and_a_ragged_sample_is_its_own_loop(mods):
    _, icp, _, _ = mods
    src, tar = clouds(B3, N3, M3, C1, C2, seed=60)
    kw = dict(normal_radius=0.45, nsample=32, max_dist=0.2)
    runs = [icp.PlaneIcpRegistration(src, tar, counts1=C1, counts2=C2, **kw).run(8) for _ in range(2)]
    for f in ("R", "T", "last_step", "value", "neq", "info", "state", "table", "normals"):
        assert bits(getattr(runs[0], f)) == bits(getattr(runs[1], f)), f
    for b in range(B3):
        own = icp.PlaneIcpRegistration(src[b:b + 1], tar[b:b + 1], counts1=C1[b:b + 1], counts2=C2[b:b + 1], **kw).run(8)
        for f in ("R", "T", "last_step", "value", "neq", "info", "state", "normals"):
            assert bits(getattr(own, f)[0]) == bits(getattr(runs[0], f)[b]), (b, f)
        assert bits(own.table[:, 0]) == bits(runs[0].table[:, b]), b
    # given normals are used as they are
    given = icp.PlaneIcpRegistration(src, tar, runs[0].normals.clone(), counts1=C1, counts2=C2, max_dist=0.2).run(8)
    assert bits(given.R) == bits(runs[0].R) and bits(given.T) == bits(runs[0].T)


def test_done_pairs_freeze_and_failed_pairs_keep_their_pose(mods):
    """Pair 1 has five source points (fewer than six pairs), pair 2 a flat target with one normal (a singular system): both keep
    the starting pose and say so; pair 0 converges (the host restatement's steps fall below both tolerances from epoch 5 on), is
    declared done, and its pose keeps its bits while the epochs go on."""
    _, icp, _, _ = mods
    c1, c2 = [512, 5, 128], [600, 600, 160]
    src, tar = clouds(3, 512, 600, c1, c2, seed=52, rot_deg=10.0)
    g = torch.stack(torch.meshgrid(torch.arange(16.0), torch.arange(10.0), indexing="ij"), -1).reshape(160, 2).cuda() / 8.0
    tar[2, :160] = torch.cat([g, torch.zeros(160, 1, device="cuda")], 1)
    src[2, :128] = tar[2, :128] + 0.01
    xi0 = torch.tensor([[0.0] * 6, [0.1, 0.0, 0.0, 0.01, 0.0, 0.0], [0.0, 0.1, 0.0, 0.0, 0.0, 0.0]])
    reg = icp.PlaneIcpRegistration(src, tar, normal_radius=0.3, counts1=c1, counts2=c2, xi0=xi0)
    assert torch.equal(reg.normals[2, :160].cpu(), torch.tensor([0.0, 0.0, 1.0]).expand(160, 3)) and not reg.normals[2, 160:].any()
    R_start, T_start = reg.R.clone(), reg.T.clone()
    reg.run(40, check_every=1000)
    done = reg.done_epoch.tolist()
    assert 3 <= done[0] < 40 and done[1] == -1 and done[2] == -1, done
    assert reg.failed.tolist() == [PR.DONE, PR.FEW, PR.FAILED]
    assert bits(reg.R[1:]) == bits(R_start[1:]) and bits(reg.T[1:]) == bits(T_start[1:])
    assert reg.info[1, 0].item() == 5 and reg.info[1, 3].item() == 507
    R_done, T_done = reg.R[0].clone(), reg.T[0].clone()
    reg.run(5)
    assert bits(reg.R[0]) == bits(R_done) and bits(reg.T[0]) == bits(T_done) and reg.done_epoch.tolist() == done
    assert reg.state[:, 0].tolist() == [45] * 3
    h = reg.history()
    assert h[1][0] == (0, None, None) and h[0][0][1] is not None and h[2][0][1] is not None


def test_epoch_in_a_captured_graph(mods):
    """No host read-back: an epoch replays from a graph with the bits of the plain calls."""
    _, icp, _, _ = mods
    src, tar = clouds(2, 257, 200, seed=80)
    plain = icp.PlaneIcpRegistration(src, tar, normal_radius=0.45).run(4)
    reg = icp.PlaneIcpRegistration(src, tar, normal_radius=0.45)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        reg.epoch()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        reg.epoch()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert bits(reg.R) == bits(plain.R) and bits(reg.T) == bits(plain.T) and reg.state[:, 0].tolist() == [4, 4]


# ---- what the loop is for -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,radius", [(65, 0.7), (130, 0.5), (257, 0.4)])
def test_exact_pairs_are_registered_to_rounding(mods, n, radius):
    """The target and the same points under the inverse of a 10 degree pose: after 12 epochs the moved source is the target to
    8 2^-23 max|coordinate| (the float32-pose restatement on the host reaches 1.2 2^-23 by epoch 6)."""
    from rrl_hip import synth
    _, icp, _, _ = mods
    B = 3
    tar = np.stack([synth.surface_cloud(100 + s, n) for s in range(B)])
    src = np.empty_like(tar)
    for s in range(B):
        Rg = synth._rotation(np.random.default_rng(7 + s).standard_normal(3), 10.0).T
        src[s] = ((tar[s].astype(np.float64) - np.array([0.05, -0.03, 0.02])) @ Rg.T).astype(np.float32)
    reg = icp.PlaneIcpRegistration(*cuda(src, tar), normal_radius=radius, patience=0).run(12)
    R, T = reg.R.cpu().numpy().astype(np.float64), reg.T.cpu().numpy().astype(np.float64)
    for s in range(B):
        err = np.abs(src[s].astype(np.float64) @ R[s] + T[s] - tar[s]).max()
        lim = 8 * U23 * np.abs(tar[s]).max()
        print(f"n = {n}, pair {s}: worst distance {err / (U23 * np.abs(tar[s]).max()):.2f} x 2^-23 max|coordinate| (bound 8)")
        assert err <= lim, (n, s, err / lim)
    assert (reg.failed == 0).all()


def test_plane_icp_beats_point_icp_on_the_table_pairs(mods):
    """Eight make_pair pairs at 20 degrees, N = M = 256, normals of radius 0.4: after 10 epochs closer to the generating rotation
    than IcpRegistration after 30, on at least 7 of 8 pairs (the float64 restatement: 8 of 8; one pair for float32 pairing ties)."""
    from test_plane_refs_host import PAIR_N, PAIR_RADIUS, PAIR_SEEDS
    _, icp, _, _ = mods
    pairs = [PR.pair_with_rotation(s, PAIR_N, PAIR_N) for s in PAIR_SEEDS]
    src, tar = cuda(np.stack([p["src"] for p, _ in pairs]), np.stack([p["tar"] for p, _ in pairs]))
    plane = icp.PlaneIcpRegistration(src, tar, normal_radius=PAIR_RADIUS, patience=0).run(10)
    point = icp.IcpRegistration(src, tar, patience=0).run(30)
    Rp, Rq = plane.R.cpu().numpy(), point.R.cpu().numpy()
    wins = 0
    for b, (_, Rt) in enumerate(pairs):
        ep, eq = PR.rotation_error_deg(Rp[b], Rt), PR.rotation_error_deg(Rq[b], Rt)
        print(f"seed {PAIR_SEEDS[b]}: plane after 10 epochs {ep:.3f} deg, point after 30 epochs {eq:.3f} deg")
        wins += ep < eq
    assert wins >= 7, wins


def test_c_refusals_leave_the_outputs_untouched(mods):
    """Every refusal of the sums' entry returns its code before a launch: real buffers, prefilled, keep their bits."""
    from test_plane_refs_host import E_ARG, E_WS, FAKE, PLANE_REFUSALS, plane_args
    _lib, _, _, ops = mods
    lib = _lib.load()
    B, N = 2, 1000
    moved, tar, nrm = (torch.randn(B, N, 3, device="cuda") for _ in range(3))
    neq = torch.full((B, 32), 7.0, dtype=torch.float64, device="cuda")
    info = torch.full((B, 4), 7, dtype=torch.int32, device="cuda")
    part = torch.full((int(lib.rrl_plane_part_bytes(B, N)) // 8,), 7.0, dtype=torch.float64, device="cuda")
    real = dict(moved=moved.data_ptr(), tar=tar.data_ptr(), normals=nrm.data_ptr(), neq=neq.data_ptr(), info=info.data_ptr(), part=part.data_ptr())
    stream = ops._stream(moved.device)

    def realise(k, v):  # the host test's overrides on real buffers: NULL stays NULL, a misaligned fake becomes a misaligned real
        if v is None or k in ("B", "N", "M", "tar_stride", "struct_bytes"):
            return v
        return moved.data_ptr() if k == "gate_sq" else real[k] + (v - FAKE)
    for over in PLANE_REFUSALS:
        fix = {k: realise(k, v) for k, v in over.items()}
        assert lib.rrl_plane_normal_eq(ctypes.byref(plane_args(lib, **{**real, **fix})), stream) == E_ARG, over
    assert lib.rrl_plane_normal_eq(ctypes.byref(plane_args(lib, **real, part_bytes=part.numel() * 8 - 1)), stream) == E_WS
    torch.cuda.synchronize()
    assert (neq == 7).all() and (info == 7).all() and (part == 7).all()
    assert lib.rrl_plane_normal_eq(ctypes.byref(plane_args(lib, **real)), stream) == 0
    torch.cuda.synchronize()
    assert info[:, 1].tolist() == [0, 0] and info[:, 0].tolist() == [N, N]
