"""The kernels that run before the loss sees a line -- farthest-point sampling and 3-NN (csrc/rrl_neigh.hip), the two AABB
kernels (csrc/rrl_geom.hip), candidate generation from the caller's uniforms and from the library's Philox generator
(csrc/rrl_sampler.h) -- against the host twins of tests/prep_refs.py (tied to the reference's recorded data on the CPU by
tests/test_prep_refs_host.py).

Indices, boxes, counters and layouts are compared for EQUALITY.  Candidate lines are measured against the float64 twin and
allowed 4 x the error of numpy's float32 evaluation of the same candidates + 2 ulp of max(radius, |centre|), directions and
origins separately (prep_refs.candidate_bound); the measured figures are printed (DESIGN.md section 6 quotes them)."""
import numpy as np
import pytest
import torch

import prep_refs as PF

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def N():
    from rrl_hip import _lib, neighbors
    _lib.load()  # fail loudly if the HIP library is missing
    assert torch.cuda.is_available()
    return neighbors


@pytest.fixture(scope="module")
def O(N):
    from rrl_hip import ops
    return ops


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy(), np.float32).view(np.uint32)


# ----------------------------------------------------------------------------------------------------------------- FPS
def assert_fps(N, pts, S, starts):
    """neighbors.fps on (B, n, 3) equals fps_ref cloud by cloud, every one of the S indices; returns the (B, S) reference."""
    got = N.fps(torch.from_numpy(pts), S, start=torch.tensor(starts)).cpu().numpy()
    assert got.shape == (len(pts), S) and got.dtype == np.int32
    ref = np.stack([PF.fps_ref(pts[b], S, starts[b]) for b in range(len(pts))])
    bad = np.argwhere(got != ref)
    assert len(bad) == 0, f"{len(bad)} of {ref.size} indices differ, first at {bad[0]}: {got[tuple(bad[0])]} != {ref[tuple(bad[0])]}"
    return ref


@pytest.mark.parametrize("n", PF.FPS_N)
def test_fps_equals_the_reference_loop(N, n):
    """S = n: from one point over the wave edge (63, 64, 65) to a lane owning two (1025) and three (2049) points."""
    ref = assert_fps(N, PF.gaussian_cloud(100 + n, 1, n), n, [n // 3])
    assert sorted(ref[0].tolist()) == list(range(n))  # distinct points: a permutation


def test_fps_batch_of_different_clouds(N):
    B, n = PF.FPS_BATCH
    assert_fps(N, PF.gaussian_cloud(7, B, n), n, PF.FPS_BATCH_STARTS)


@pytest.mark.parametrize("B, n, S", PF.FPS_SWITCH)
def test_fps_on_both_sides_of_the_lds_switch(N, B, n, S):
    """n = 8192: points and distances in 128 KiB of dynamic LDS (+ 256 B static); n = 8193: in global memory."""
    assert (n <= PF.FPS_LDS_MAX) == (n * 16 <= 128 * 1024)
    assert_fps(N, PF.gaussian_cloud(n, B, n), S, [n - 1, 4097])


def test_fps_lattice_ties_and_the_tail_of_zeros(N):
    """Integer lattice with copies: every distance an exact integer, ties everywhere (first occurrence), and once all
    1728 positions are taken every distance is 0 and the reference emits index 0 for the remaining 300 samples."""
    p = PF.lattice_cloud(43)
    k = PF.LATTICE_SIDE ** 3
    ref = assert_fps(N, p[None], len(p), [17])[0]
    assert len(set(ref[:k].tolist())) == k and ref[:k].max() < k
    np.testing.assert_array_equal(ref[k:], 0)


def test_fps_cap_decides_above_1e10(N):
    p = PF.far_cloud(41)
    assert np.count_nonzero(PF.sq_dist(p, p[5]) > PF.FPS_CAP) > PF.FAR_N // 2  # some squared distances do exceed the cap
    ref = assert_fps(N, p[None], PF.FAR_S, [5])[0]
    assert ref[1] != int(np.argmax(PF.sq_dist(p, p[5])))  # (without the cap the farthest point would come second)


# ----------------------------------------------------------------------------------------------------------------- 3-NN
def assert_knn3(N, pts, q):
    got = N.knn3(torch.from_numpy(pts), torch.from_numpy(q)).cpu().numpy()
    assert got.shape == q.shape + (3,) and got.dtype == np.int32
    ref = np.stack([PF.knn3_ref(pts[b], q[b]) for b in range(len(pts))])
    bad = np.argwhere(got != ref)
    assert len(bad) == 0, f"{len(bad)} of {ref.size} neighbours differ, first at {bad[0]}: {got[tuple(bad[0][:2])]} != {ref[tuple(bad[0][:2])]}"
    return ref


@pytest.mark.parametrize("n, S", PF.KNN_SHAPES)
def test_knn3_equals_the_stable_sort(N, n, S):
    """Two different Gaussian clouds, queries in arbitrary order with repeats, S around the 256-lane workgroup."""
    g = np.random.default_rng(n * 1000 + S)
    assert_knn3(N, PF.gaussian_cloud(n + S, 2, n), g.integers(0, n, (2, S)))


def test_knn3_lattice_lowest_index_among_equals(N):
    """Two shuffles of the lattice with copies: up to six neighbours at distance 1 (index order decides), and a query whose
    twin has a lower index gets the TWIN first and itself second."""
    pts = np.stack([PF.lattice_cloud(43), PF.lattice_cloud(44)])
    k, n = PF.LATTICE_SIDE ** 3, pts.shape[1]
    g = np.random.default_rng(5)
    q = np.concatenate([np.tile(np.arange(k, k + 100), (2, 1)), g.integers(0, n, (2, PF.KNN_LATTICE_S - 100))], axis=1)
    assert_knn3(N, pts, g.permuted(q, axis=1))
    ref = np.stack([PF.knn3_ref(pts[b], q[b]) for b in range(2)])
    for b in range(2):
        twins = ref[b, :100]
        assert np.all(twins[:, 0] < k) and np.all(twins[:, 0] != q[b, :100])
        np.testing.assert_array_equal(pts[b][twins[:, 0]], pts[b][q[b, :100]])


# ----------------------------------------------------------------------------------------------------------------- AABB
def rigid_case(seed, B):
    """R (B, 3, 3) orthonormal, t (B, 3) standard normal, float32."""
    g = np.random.default_rng(seed)
    R = np.stack([np.linalg.qr(g.standard_normal((3, 3)))[0] for _ in range(B)]).astype(np.float32)
    return R, g.standard_normal((B, 3)).astype(np.float32)


def assert_rigid_aabb(O, v, R, t):
    """rigid_apply_aabb_into: out bit-equal to rigid_apply_into, the box the exact min / max of that out; both layouts of R."""
    x = cu(v)
    for tr in (False, True):
        y0, y1, box = torch.empty_like(x), torch.full_like(x, np.nan), torch.full((len(v), 6), np.nan, device="cuda")
        O.rigid_apply_into(x, cu(R), cu(t), y0, transpose_r=tr)
        O.rigid_apply_aabb_into(x, cu(R), cu(t), y1, box, transpose_r=tr)
        np.testing.assert_array_equal(bits(y1), bits(y0), err_msg=f"transpose_r {tr}")
        np.testing.assert_array_equal(box.cpu().numpy(), PF.aabb_ref(y0.cpu().numpy()), err_msg=f"transpose_r {tr}")
    return y0.cpu().numpy()


@pytest.mark.parametrize("n", PF.AABB_N)
def test_aabb_is_the_exact_min_and_max(O, n):
    v = PF.gaussian_cloud(200 + n, 3, n)
    np.testing.assert_array_equal(O.aabb(cu(v)).cpu().numpy(), PF.aabb_ref(v))
    assert_rigid_aabb(O, v, *rigid_case(n, 3))


@pytest.mark.parametrize("i", PF.AABB_HOT_AT)
def test_aabb_one_hot_sweep(O, i):
    """All coordinates in [-1, 1] except that point i carries the unique minimum of one axis and point j the unique maximum
    of another (sample b: axes b and b + 1; sample 2 with -inf / +inf), i and j on every lane, wave and trip edge of the
    reduction: an extreme dropped at a boundary fails here by its position.  The rigid variant with signed permutation
    matrices and integer translations (exact), so the extremes stay where they were put."""
    n = PF.AABB_HOT_N
    base = np.random.default_rng(i).uniform(-1.0, 1.0, (3, n, 3)).astype(np.float32)
    perm = np.zeros((3, 3, 3), np.float32)
    perm[0, [0, 1, 2], [1, 2, 0]] = (1, -1, 1)
    perm[1, [0, 1, 2], [2, 0, 1]] = (-1, 1, 1)
    perm[2] = np.diag([1, 1, -1])
    t = np.array([[2, -3, 1], [0, 4, -2], [-1, 0, 5]], np.float32)
    for j in PF.AABB_HOT_AT:
        v = base.copy()
        for b in range(3):
            v[b, i, b] = -5.0 - b
            v[b, j, (b + 1) % 3] = 7.0 + b
        want = PF.aabb_ref(v)
        for b in range(3):
            assert want[b, b] == -5.0 - b and want[b, 3 + (b + 1) % 3] == 7.0 + b
        y = assert_rigid_aabb(O, v, perm, t)
        for b in range(3):  # (the hot points are extremes of the moved cloud too)
            assert {i, j} <= set(y[b].argmin(0).tolist()) | set(y[b].argmax(0).tolist())
        v[2, i, 2], v[2, j, 0] = -np.inf, np.inf
        want = PF.aabb_ref(v)
        assert want[2, 2] == -np.inf and want[2, 3] == np.inf
        np.testing.assert_array_equal(O.aabb(cu(v)).cpu().numpy(), want, err_msg=f"min at {i}, max at {j}")


# ----------------------------------------------------------------------------------------------------------------- candidates
def assert_candidates(lines, u, rad, centre, what):
    """lines (n, 6) from the device against the twin on uniforms u (4, n): within candidate_bound; the measured figures are printed."""
    cb = PF.candidate_bound(u, rad, centre)
    ed, eo = PF.candidate_errors(lines, cb)
    print(f"{what}: direction device {ed:.2e} host {cb['host'][0]:.2e} bound {cb['bound'][0]:.2e} | origin device {eo:.2e} "
          f"host {cb['host'][1]:.2e} bound {cb['bound'][1]:.2e} | short chords left out {cb['left_out']:.6f}")
    assert cb["left_out"] <= PF.SHORT_CHORD_CAP
    assert ed <= cb["bound"][0], (what, "direction", ed, cb["bound"][0])
    assert eo <= cb["bound"][1], (what, "origin", eo, cb["bound"][1])


def batch_rands(seed, rounds, B, n):
    """(rounds, 4, B, n) float32 from synth.uniform_streams: sample b takes its own slice of one stream."""
    from rrl_hip import synth
    return np.ascontiguousarray(synth.uniform_streams(seed, rounds, B * n).reshape(rounds, 4, B, n))


@pytest.mark.parametrize("n", PF.CAND_N)
def test_candidates_from_the_callers_uniforms(O, n):
    """B = 3 with a radius and a centre per sample (one far from the origin): every sample of the batched call equals the
    B = 1 call on its slice of `rands` bit for bit (the [rd][4][b][i] layout) and lies within the bound of the twin."""
    B = PF.CAND_B
    rands = batch_rands(n, 1, B, n)
    r, c = torch.from_numpy(PF.CAND_RADII), torch.from_numpy(PF.CAND_CENTRES)
    lines, filled = O.sample_lines(torch.from_numpy(rands), r, c, None, None)
    assert lines.shape == (B, n, 6) and filled.tolist() == [n] * B
    for b in range(B):
        one, f1 = O.sample_lines(torch.from_numpy(rands[:, :, b:b + 1]), r[b:b + 1], c[b:b + 1], None, None)
        assert f1.tolist() == [n]
        np.testing.assert_array_equal(bits(lines[b]), bits(one[0]), err_msg=f"sample {b}")
        assert_candidates(lines[b].cpu().numpy(), rands[0, :, b], PF.CAND_RADII[b], PF.CAND_CENTRES[b], f"rands n {n} sample {b}")


def test_resampled_batch_equals_its_samples(O):
    """10 rounds, a box pair per sample: `lines` and `filled` of the batched call equal the three B = 1 calls bit for bit."""
    from rrl_hip import synth
    B, n = PF.CAND_B, 1025
    rands = batch_rands(77, PF.CAND_ROUNDS, B, n)
    pairs = [synth.make_pair(20 + b, 300, 280) for b in range(B)]
    scale = np.array([1.0, 2.5, 0.6], np.float32)
    shift = np.array([[0, 0, 0], [0.5, -0.25, 0.125], [40, -25, 17]], np.float32)
    b1 = O.aabb(cu(np.stack([p["src"] * s + o for p, s, o in zip(pairs, scale, shift)])))
    b2 = O.aabb(cu(np.stack([p["tar"] * s + o for p, s, o in zip(pairs, scale, shift)])))
    r = torch.tensor([float(p["radius"]) * s for p, s in zip(pairs, scale)])
    c = torch.from_numpy(np.stack([p["center"] * s + o for p, s, o in zip(pairs, scale, shift)]))
    lines, filled = O.sample_lines(torch.from_numpy(rands), r, c, b1, b2)
    assert len(set(filled.tolist())) > 1 and min(filled.tolist()) > 0  # the samples really differ
    for b in range(B):
        one, f1 = O.sample_lines(torch.from_numpy(rands[:, :, b:b + 1]), r[b:b + 1], c[b:b + 1], b1[b:b + 1], b2[b:b + 1])
        assert int(f1[0]) == int(filled[b])
        np.testing.assert_array_equal(bits(lines[b]), bits(one[0]), err_msg=f"sample {b}")


# ----------------------------------------------------------------------------------------------------------------- generator
def draw(O, r, c, B, n, out=None):
    lines, filled = O.sample_lines(None, r, c, None, None, out=out, rng_shape=(1, B, n))
    return lines, filled


def state_of(O):
    return [int(x) for x in O.sampler_rng().cpu().tolist()]


def assert_call(lines, seed, call, rad, centre, what):
    """Every sample b of `lines` (B, n, 6) is the twin's candidates of (seed, call, b, round 0)."""
    lines = lines.cpu().numpy()
    for b in range(len(lines)):
        u = PF.sampler_uniforms(seed, call, b, 0, np.arange(lines.shape[1]))
        assert_candidates(lines[b], u, rad, centre, f"{what} call {call} sample {b}")


@pytest.mark.parametrize("seed", PF.RNG_SEEDS)
def test_library_generator_matches_the_philox_twin(O, seed):
    """No boxes, one round, the same radius and centre for all samples: row i of sample b is the twin's candidate of the
    counter (i, 0 | b << 16, call, call >> 32) under the key (seed, seed >> 32) -- for both seeds (the second uses the high key
    word), for successive calls (the counter grows by exactly 1 per call, the ticket returns to 0; one call's write pass
    spans 9 workgroups), with the call counter beyond 2^32, and under graph replay (one replay, one counter step)."""
    from rrl_hip.graph import GraphedStep
    rad, centre = PF.CAND_RADII[0], PF.CAND_CENTRES[1]
    r, c = torch.tensor([rad] * 3).cuda(), torch.from_numpy(np.tile(centre, (3, 1))).cuda()
    st = O.sampler_rng(seed=seed)
    assert state_of(O) == [seed, 0, 0, 0]
    shapes = [PF.RNG_PLAIN, PF.RNG_WIDE, (1, 1025)]
    for call, (B, n) in enumerate(shapes):
        lines, filled = draw(O, r[:B], c[:B], B, n)
        assert filled.tolist() == [n] * B
        assert state_of(O) == [seed, call + 1, 0, 0]
        assert_call(lines, seed, call, rad, centre, f"seed {seed:#x}")
        if B > 1:  # the samples of a batch differ from each other
            ln = lines.cpu().numpy()
            assert all(np.count_nonzero(np.all(ln[a] == ln[b], axis=1)) == 0 for a in range(B) for b in range(a))
    # the high word of the call counter
    st[1] = PF.RNG_HIGH_CALL
    B, n = PF.RNG_PLAIN
    lines, _ = draw(O, r, c, B, n)
    assert state_of(O) == [seed, PF.RNG_HIGH_CALL + 1, 0, 0]
    assert_call(lines, seed, PF.RNG_HIGH_CALL, rad, centre, f"seed {seed:#x}")
    low, _ = draw(O, r, c, B, n)  # (call 2^32 + 6; then the same low word without the high one)
    st[1] = (PF.RNG_HIGH_CALL + 1) & 0xFFFFFFFF
    low2, _ = draw(O, r, c, B, n)
    assert not np.any(np.all(low.cpu().numpy() == low2.cpu().numpy(), axis=2))
    # captured: every replay is one call
    buf = torch.empty(B, n, 6, device="cuda")
    g = GraphedStep(lambda: draw(O, r, c, B, n, out=buf))
    c0 = state_of(O)[1]
    for k in range(3):
        g()
        got = buf.clone()
        assert state_of(O) == [seed, c0 + k + 1, 0, 0]
        assert_call(got, seed, c0 + k, rad, centre, f"seed {seed:#x} replay {k}")


def test_library_generator_rounds_with_boxes(O):
    """10 rounds with boxes at n = 2000, B = 2: accept decisions are knife-edge, so the rows are matched to the twin's
    candidates instead -- every filled row is exactly one twin candidate (rd, i) of its own sample (nearest by origin,
    within the bound, the second nearest beyond it), the matched candidates come in strictly increasing (rd, i) order,
    rounds >= 1 contribute, the matched directions hold the bound too, and every filled row passes rrl_box_accept."""
    from scipy.spatial import cKDTree
    from rrl_hip import synth
    seed, B, n, rounds = PF.RNG_SEEDS[1], 2, PF.RNG_ROUNDS_N, PF.CAND_ROUNDS
    pr = synth.make_pair(3, 800, 700)
    b1, b2 = O.aabb(cu(pr["src"])[None]).repeat(B, 1), O.aabb(cu(pr["tar"])[None]).repeat(B, 1)
    rad, centre = np.float32(pr["radius"]), pr["center"]
    r, c = torch.tensor([float(rad)] * B).cuda(), torch.from_numpy(np.tile(centre, (B, 1))).cuda()
    O.sampler_rng(seed=seed)
    lines, filled = O.sample_lines(None, r, c, b1, b2, rng_shape=(rounds, B, n))
    assert state_of(O) == [seed, 1, 0, 0]
    mask, _ = O.box_accept(lines, b1, b2)
    lines, mask = lines.cpu().numpy(), mask.cpu().numpy()
    for b in range(B):
        nf = min(int(filled[b]), n)
        assert nf > n // 2 and not np.any(lines[b, nf:]) and np.all(np.abs(lines[b, :nf]).sum(1) > 0)
        assert np.all((mask[b, :nf] & 3) == 3)
        u = np.concatenate([PF.sampler_uniforms(seed, 0, b, rd, np.arange(n)) for rd in range(rounds)], axis=1)  # (4, rounds n)
        cb = PF.candidate_bound(u, rad, centre)
        dist, idx = cKDTree(cb["ref"][:, 3:]).query(lines[b, :nf, 3:].astype(np.float64), k=2, p=np.inf)
        assert dist[:, 0].max() <= cb["bound"][1], (b, dist[:, 0].max(), cb["bound"][1])
        assert dist[:, 1].min() > cb["bound"][1]  # unique
        key = idx[:, 0]  # = rd * n + i
        assert np.all(np.diff(key) > 0), f"sample {b}: rows out of candidate order"
        assert key.max() >= n, "no row from a round >= 1"
        print(f"rounds with boxes, sample {b}: {nf} rows from rounds 0..{key.max() // n}")
        assert_candidates(lines[b, :nf], u[:, key], rad, centre, f"rounds with boxes sample {b}")  # (the matched set's own bound)
    assert not np.array_equal(lines[0], lines[1])
