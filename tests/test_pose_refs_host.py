"""CPU-side check of tests/pose_refs.py: the references and yardsticks that tests/test_gpu_pose_kernels.py holds the pose
kernels to are sound by themselves -- the "exact" cases really are exact in float32 under any summation order, the
summation yardstick of the rigid backward can be met by the kernel's own order (emulated in numpy), every SE(3) magnitude
group has a finite yardstick, and the Chamfer scales are powers of two."""
import math

import numpy as np
import pytest

import pose_refs as PR


def _shuffled_f32_sum(terms, rng):
    """Sum along the last axis in float32 in a random order, one term after the other (every partial sum rounded)."""
    t = np.asarray(terms, np.float32)[..., rng.permutation(terms.shape[-1])]
    return np.cumsum(t, axis=-1, dtype=np.float32)[..., -1]


@pytest.mark.parametrize("n", [1, 1025, 40000, PR.RIGID_N_GRID_LOOP])
def test_rigid_integer_cases_are_exact_in_float32(n):
    """Every output of the integer case is an integer below 2^24, and float32 sums of its terms in the given order, in a
    shuffled order and in the kernel's order all equal the int64 reference."""
    B = 1 if n > 40000 else 3
    c = PR.rigid_int_case(7 + n, B, n)
    for tr in (False, True):
        ref = PR.rigid_reference(c, tr)
        assert max(np.abs(ref[k]).max() for k in ref) < 1 << 24 and ref["y"].dtype == np.int64
        terms = PR.rigid_sum_terms(c)
        assert np.abs(terms).sum(-1).max() <= 1 << 24  # no partial sum in any order leaves the exact range
        want = PR.outputs_as_sums(ref["gR"], ref["gt"], tr)
        rng = np.random.default_rng(n)
        for got in (PR.sequential_f32_sums(terms), _shuffled_f32_sum(terms, rng), PR.kernel_order_f32_sums(terms)):
            np.testing.assert_array_equal(got.astype(np.int64), want)
        # y and gx in float32, products and sums rounded one by one (no FMA) in a permuted order of the three terms
        x, R, t, gy = (c[k] for k in ("x", "R", "t", "gy"))
        m = R.transpose(0, 2, 1) if tr else R
        y = ((x[:, :, 2, None] * m[:, None, 2, :] + x[:, :, 0, None] * m[:, None, 0, :]) + x[:, :, 1, None] * m[:, None, 1, :]) + t[:, None]
        gx = (gy[:, :, 1, None] * m[:, None, :, 1] + gy[:, :, 2, None] * m[:, None, :, 2]) + gy[:, :, 0, None] * m[:, None, :, 0]
        assert y.dtype == np.float32 and gx.dtype == np.float32
        np.testing.assert_array_equal(y.astype(np.int64), ref["y"])
        np.testing.assert_array_equal(gx.astype(np.int64), ref["gx"])


@pytest.mark.parametrize("at", PR.ONE_HOT_AT)
def test_one_hot_reference_is_the_outer_product(at):
    c = PR.rigid_one_hot_case(3, 2, PR.ONE_HOT_N, at)
    assert np.count_nonzero(c["gy"]) == 2 * 3 and np.all(c["x"][:, at] != 0)
    for tr in (False, True):
        ref = PR.rigid_reference(c, tr)
        outer = np.einsum("bi,bj->bij", c["x"][:, at], c["gy"][:, at]).astype(np.int64)
        np.testing.assert_array_equal(ref["gR"], outer.transpose(0, 2, 1) if tr else outer)
        np.testing.assert_array_equal(ref["gt"], c["gy"][:, at].astype(np.int64))
        assert np.all(ref["gR"] != 0) and np.all(ref["gt"] != 0)


@pytest.mark.parametrize("n", [16385, 40000])
def test_kernel_summation_order_beats_the_sequential_sum(n):
    """The condition of the GPU test -- the largest normalised error over the 12 B outputs is at most that of a sequential
    float32 sum -- holds for the kernel's summation order by a factor of more than ten (so a correct kernel has that
    margin, and one that loses or doubles a single point of 40 000, 2.5e-5 normalised, has none)."""
    worst = 0.0
    for seed in range(6):
        terms = PR.rigid_sum_terms(PR.rigid_float_case(seed, 3, n))
        kern = PR.normalised_error(PR.kernel_order_f32_sums(terms), terms).max()
        seq = PR.normalised_error(PR.sequential_f32_sums(terms), terms).max()
        assert 10.0 * kern <= seq < 1e-6, (seed, kern, seq)
        worst = max(worst, seq)
    assert worst < 2.5e-5 / 10  # the yardstick itself is far below one lost point


def test_se3_yardstick_is_finite_and_exact_where_claimed():
    import torch
    c = PR.se3_case()
    assert c["xi"].shape == (832, 6) and len(PR.SE3_MAGS) == 13
    t = np.linalg.norm(c["xi"][:, :3].astype(np.float64), axis=1).reshape(13, -1)
    for g, m in enumerate(PR.SE3_MAGS):  # each group sits at its magnitude, on the same side of the Taylor boundary in both precisions
        assert np.all(np.abs(t[g] - m) <= 1e-6 * max(m, 1e-30)) and abs(m - 0.01) > 1e-6
        assert np.all((t[g] < 0.01) == (m < 0.01))
    ref, host = PR.se3_host(c, torch.float64), PR.se3_host(c, torch.float32)
    yard = PR.se3_yardstick(ref, host)
    for k, (herr, bound) in yard.items():
        assert np.all(np.isfinite(herr)) and np.all(np.isfinite(bound)) and np.all(bound > 0), k
        # a yardstick is a few float32 roundings of the output, never a loose bound: the worst group (cancellation in
        # (t - sin t) / t^3 just above the boundary, sin of a float32 angle of 30) stays below 1e-2 of the output
        assert np.all(bound <= 1e-2 * np.maximum(PR._group_max(ref[k]), 1.0)), (k, bound)
    for m in PR.SE3_EXACT_MAGS:
        g = PR.SE3_MAGS.index(m)
        assert yard["R"][0][g] == 0.0 and yard["T"][0][g] == 0.0, m
    sl = slice(0, PR.SE3_PER_MAG)  # |w| = 0: the identity and T = v
    np.testing.assert_array_equal(ref["R"][sl], np.broadcast_to(np.eye(3), (PR.SE3_PER_MAG, 3, 3)))
    np.testing.assert_array_equal(ref["T"][sl], c["xi"][sl, 3:].astype(np.float64))
    print("\n" + PR.se3_table(PR.se3_group_errors(host, ref), yard))


def test_se3_one_sided_contractions_differ():
    import torch
    c = PR.se3_case()
    full, only_R, only_T = (PR.se3_host(c, torch.float64, r, t)["gxi"] for r, t in ((True, True), (True, False), (False, True)))
    np.testing.assert_allclose(only_R + only_T, full, rtol=1e-12, atol=1e-12)
    assert np.abs(only_R).max() > 0.1 and np.abs(only_T).max() > 0.1
    assert np.all(only_R[:, 3:] == 0.0)  # R does not depend on the translational part


@pytest.mark.parametrize("n", PR.ADAM_N)
def test_adam_reference_moves_and_gates(n):
    c = PR.adam_case(n)
    ref = PR.adam_reference(c)
    assert ref.shape == (PR.ADAM_STEPS, n) and np.all(np.isfinite(ref))
    for it in range(PR.ADAM_STEPS):
        prev = c["p0"] if it == 0 else ref[it - 1]
        if c["gates"][it]:
            assert np.all(ref[it] != prev), it
        else:
            np.testing.assert_array_equal(ref[it], prev)
    assert sum(1 for q in c["gates"] if q) == 6 and len(set(c["lrs"])) == 2
    # the first step of Adam moves every parameter by lr against the gradient's sign (m / sqrt(v) = sign g)
    np.testing.assert_allclose(ref[0] - c["p0"], -c["lrs"][0] * np.sign(c["grads"][0]), rtol=1e-4, atol=1e-7)


@pytest.mark.parametrize("shape", PR.CHAMFER_SHAPES + [PR.CHAMFER_ONE_TARGET])
def test_chamfer_exact_cases_have_representable_scales(shape):
    B, N, M = shape
    one = shape == PR.CHAMFER_ONE_TARGET
    x, y = PR.chamfer_int_case(31, B, N, M, one_target=one)
    ix, iy, value = PR.chamfer_nearest(x, y, np.int64)
    ix32, iy32, value32 = PR.chamfer_nearest(x, y, np.float32)  # the kernels' arithmetic gives the same minima
    np.testing.assert_array_equal(ix, ix32)
    np.testing.assert_array_equal(iy, iy32)
    assert value == value32
    if one:
        assert np.all(ix == 0)
    for gval in PR.CHAMFER_GVALS:
        sc = PR.chamfer_scale(B, N, M, gval)
        mant, _ = math.frexp(abs(sc))
        assert mant == 0.5 and np.float32(sc) == sc, (shape, gval, sc)  # a power of two
        r = PR.chamfer_backward_reference(x, y, ix, iy, gval)
        # every contribution is an integer multiple of |sc| and every sum of magnitudes stays below 2^24 |sc|: exact
        for k in ("gx", "gy"):
            q = r[k] / abs(sc)
            np.testing.assert_array_equal(q, np.round(q))
            assert (r["a" + k[1]] / abs(sc)).max() < 1 << 24
            np.testing.assert_array_equal(r[k].astype(np.float32).astype(np.float64), r[k])
        # a shuffled float32 accumulation of the contributions gives the same bits
        b = B - 1
        pi, pj = np.concatenate([np.arange(N), iy[b]]), np.concatenate([ix[b], np.arange(M)])
        c = ((x[b, pi] - y[b, pj]) * np.float32(sc)).astype(np.float32)
        gx = np.zeros((N, 3), np.float32)
        for t in np.random.default_rng(5).permutation(len(pi)):
            gx[pi[t]] += c[t]
        np.testing.assert_array_equal(gx, r["gx"][b].astype(np.float32))
        assert r["kx"].sum() == r["ky"].sum() == B * (N + M) and r["kx"].min() >= 1 and r["ky"].min() >= 1
        assert abs(r["gx"].sum() + r["gy"].sum()) == 0.0  # every contribution enters once with each sign


def test_chamfer_float_case_has_unambiguous_minima():
    """The general-float case: float32 (the kernels' arithmetic) and float64 agree on every nearest neighbour, so the
    contribution lists of the reference are the kernel's; the bound (k + 3) 2^-24 sum |contributions| is finite."""
    x, y = PR.chamfer_float_case()
    ix32, iy32, _ = PR.chamfer_nearest(x, y, np.float32)
    ix64, iy64, _ = PR.chamfer_nearest(x, y, np.float64)
    np.testing.assert_array_equal(ix32, ix64)
    np.testing.assert_array_equal(iy32, iy64)
    r = PR.chamfer_backward_reference(x, y, ix64, iy64, PR.CHAMFER_FLOAT_GVAL)
    assert r["kx"].max() > 2 and r["ky"].max() > 2 and np.all(r["ax"] > 0) and np.all(r["ay"] > 0)
    # a float32 evaluation in the kernel's operation order, contributions added in index order, is inside the bound
    B, N, M = PR.CHAMFER_FLOAT_SHAPE
    sc = np.float32(2.0) * np.float32(PR.CHAMFER_FLOAT_GVAL) / (np.float32(B) * np.float32(N + M))
    for b in range(B):
        pi, pj = np.concatenate([np.arange(N), iy64[b]]), np.concatenate([ix64[b], np.arange(M)])
        c = (x[b, pi] - y[b, pj]) * sc
        assert c.dtype == np.float32
        gx, gy = np.zeros((N, 3), np.float32), np.zeros((M, 3), np.float32)
        for t in range(len(pi)):
            gx[pi[t]] += c[t]
            gy[pj[t]] -= c[t]
        assert np.all(np.abs(gx - r["gx"][b]) <= (r["kx"][b][:, None] + 3) * PR.U32 * r["ax"][b])
        assert np.all(np.abs(gy - r["gy"][b]) <= (r["ky"][b][:, None] + 3) * PR.U32 * r["ay"][b])


@pytest.mark.parametrize("N, M", [(0, 5), (5, 0), (0, 0)])
def test_chamfer_backward_refuses_an_empty_cloud(N, M):
    """The backward follows an index out of the forward's keys, and the forwards refuse an empty cloud: so does the
    backward, on the host and before any launch (fake pointers, no GPU)."""
    import ctypes
    from rrl_hip import _lib, build
    build.build_lib()
    lib, fake = _lib.load(), ctypes.c_void_p(256)
    assert lib.rrl_chamfer_bwd(fake, fake, fake, fake, fake, fake, fake, 2, N, M, None) == -1
    assert lib.rrl_chamfer_fwd(fake, fake, fake, fake, fake, 2, N, M, None) == -1
    assert lib.rrl_chamfer_bwd(fake, fake, fake, fake, fake, fake, fake, 0, N, M, None) == 0
