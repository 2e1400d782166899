"""The pose-side kernels of csrc/rrl_geom.hip -- rigid apply forward / backward (+ finalize), the SE(3) exponential and its
dual-number backward, the gated Adam update, the Chamfer backward -- against the exact and float64 references of
tests/pose_refs.py (shown sound on the CPU by tests/test_pose_refs_host.py).

Method: inputs whose answer is exact in float32 under any summation order and with or without FMA, so the assertion is
equality; where the inputs must be general floats the kernel is measured against float64 and allowed the error of a plain
float32 evaluation of the same reference, computed here (never taken from the code under test)."""
import numpy as np
import pytest
import torch

import pose_refs as PR

pytestmark = pytest.mark.gpu

LAYOUTS = [(False, False), (False, True), (True, False), (True, True)]  # (transpose_r, channel_first)


@pytest.fixture(scope="module")
def L():
    import loss
    from rrl_hip import _lib
    _lib.load()  # fail loudly if the HIP library is missing
    assert torch.cuda.is_available()
    return loss


def cu(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda().requires_grad_(grad)


def bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy(), np.float32).view(np.uint32)


# ----------------------------------------------------------------------------------------------------------------- rigid
def run_rigid(c, transpose_r, channel_first, x_grad=True):
    """ops.rigid_apply forward and backward of a pose_refs case in the given layout: dict(y, gx, gR, gt) as numpy arrays in
    the reference's point-major layout (gx None when x does not require grad)."""
    from rrl_hip import ops
    to = (lambda a: a.transpose(0, 2, 1)) if channel_first else (lambda a: a)
    x, gy = cu(to(c["x"]), x_grad), cu(to(c["gy"]))
    R, t = cu(c["R"], True), cu(c["t"], True)
    y = ops.rigid_apply(x, R, t, transpose_r=transpose_r, channel_first=channel_first)
    y.backward(gy)
    back = lambda v: to(v.detach().cpu().numpy())
    assert x_grad == (x.grad is not None)
    return dict(y=back(y), gx=back(x.grad) if x_grad else None, gR=R.grad.cpu().numpy(), gt=t.grad.cpu().numpy())


def assert_rigid_exact(got, ref, what):
    for k in ("y", "gx", "gR", "gt"):
        if got[k] is None:
            continue
        assert got[k].dtype == np.float32 and got[k].shape == ref[k].shape, (what, k)
        bad = np.argwhere(got[k].astype(np.float64) != ref[k])
        assert len(bad) == 0, f"{what}: {k} differs at {len(bad)} places, first {bad[0]}: {got[k][tuple(bad[0])]} != {ref[k][tuple(bad[0])]}"


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", PR.RIGID_N)
def test_rigid_apply_exact_on_the_integer_grid(L, n, B):
    """y, gx, gR, gt of an integer-grid case equal the int64 reference bit for bit in all four layouts, from one point to
    three workgroups of the backward (one launch up to 16384 points, partials + finalize beyond)."""
    c = PR.rigid_int_case(1000 * B + n, B, n)
    for tr, cf in LAYOUTS:
        assert_rigid_exact(run_rigid(c, tr, cf), PR.rigid_reference(c, tr), (n, B, tr, cf))


def test_rigid_apply_exact_through_the_forward_grid_loop(L):
    """524 293 points: rigid_fwd_kernel's 2048 workgroups loop over the points, the backward takes 33 workgroups."""
    from rrl_hip import _lib
    n = PR.RIGID_N_GRID_LOOP
    assert n > 2048 * 256 and _lib.load().rrl_rigid_bwd_blocks(n) == 33
    c = PR.rigid_int_case(5, 1, n)
    assert_rigid_exact(run_rigid(c, False, False), PR.rigid_reference(c, False), n)


@pytest.mark.parametrize("n", [1025, 16384, 40000])
def test_rigid_apply_exact_without_the_gradient_of_x(L, n):
    """x does not require grad: the backward runs with gx == NULL and gives the same gR, gt."""
    c = PR.rigid_int_case(77 + n, 3, n)
    for tr, cf in ((False, False), (True, True)):
        assert_rigid_exact(run_rigid(c, tr, cf, x_grad=False), PR.rigid_reference(c, tr), (n, tr, cf))


@pytest.mark.parametrize("at", PR.ONE_HOT_AT)
def test_rigid_backward_one_hot_sweep(L, at):
    """gy is zero except at one point on a lane, wave or workgroup edge: gR is x_i (x) gy_i in R's layout and gt is gy_i --
    a point skipped (zero) or visited twice (double) fails here by its index."""
    c = PR.rigid_one_hot_case(300 + at, 3, PR.ONE_HOT_N, at)
    outer = np.einsum("bi,bj->bij", c["x"][:, at], c["gy"][:, at])
    for tr, cf in LAYOUTS:
        got = run_rigid(c, tr, cf)
        np.testing.assert_array_equal(got["gR"], outer.transpose(0, 2, 1) if tr else outer, err_msg=f"point {at}, layout {(tr, cf)}")
        np.testing.assert_array_equal(got["gt"], c["gy"][:, at], err_msg=f"point {at}, layout {(tr, cf)}")
        assert_rigid_exact(got, PR.rigid_reference(c, tr), (at, tr, cf))


@pytest.mark.parametrize("n", [16385, 40000])
def test_rigid_backward_sums_at_least_as_well_as_a_sequential_sum(L, n):
    """General floats (standard normal x, gy, orthonormal R; B = 3): the error of each of the 36 sums against float64,
    normalised by the float64 sum of |terms|, is at most the largest such error of a sequential float32 sum of the same
    terms.  The kernel's order (16 per lane, wave tree, 16 waves, workgroups in double) measures 2e-9 ... 5e-9 in numpy
    against 7e-8 ... 8e-8 sequential (tests/test_pose_refs_host.py); one point of 40 000 lost or doubled is 2.5e-5.
    y and gx (three-term dot products) within 4 float32 roundings of sum |terms|."""
    c = PR.rigid_float_case(n, 3, n)
    terms = PR.rigid_sum_terms(c)
    yard = PR.normalised_error(PR.sequential_f32_sums(terms), terms).max()
    for tr, cf in LAYOUTS:
        got = run_rigid(c, tr, cf)
        err = PR.normalised_error(PR.outputs_as_sums(got["gR"], got["gt"], tr), terms)
        print(f"n {n} layout {(tr, cf)}: kernel {err.max():.2e}  sequential float32 {yard:.2e}")
        assert err.max() <= yard, (tr, cf, err.max(), yard)
        ref = PR.rigid_reference(c, tr, np.float64)
        m = np.abs(c["R"].astype(np.float64).transpose(0, 2, 1) if tr else c["R"].astype(np.float64))
        ay = np.einsum("bni,bij->bnj", np.abs(c["x"].astype(np.float64)), m) + np.abs(c["t"].astype(np.float64))[:, None]
        agx = np.einsum("bnj,bij->bni", np.abs(c["gy"].astype(np.float64)), m)
        assert np.all(np.abs(got["y"] - ref["y"]) <= 4 * PR.U32 * ay)
        assert np.all(np.abs(got["gx"] - ref["gx"]) <= 4 * PR.U32 * agx)


# ----------------------------------------------------------------------------------------------------------------- SE(3)
@pytest.fixture(scope="module")
def se3():
    """The 832-twist case, its float64 reference and float32 host evaluation (computed once, never modified)."""
    c = PR.se3_case()
    ref = {(r, t): PR.se3_host(c, torch.float64, r, t) for r, t in ((True, True), (True, False), (False, True))}
    host = {k: PR.se3_host(c, torch.float32, *k) for k in ref}
    return c, ref, host


def run_se3(c, rows=slice(None), use_R=True, use_T=True):
    """ops.se3_exp and the backward of the contraction on the twists `rows`: (R, T, gxi) GPU tensors."""
    from rrl_hip import ops
    x = cu(c["xi"][rows], True)
    R, T = ops.se3_exp(x)
    s = 0
    if use_R:
        s = s + (R * cu(c["cR"][rows])).sum()
    if use_T:
        s = s + (T * cu(c["cT"][rows])).sum()
    s.backward()
    return R.detach(), T.detach(), x.grad


@pytest.mark.parametrize("use", [(True, True), (True, False), (False, True)], ids=["R+T", "R only", "T only"])
def test_se3_exp_and_backward_against_float64(L, se3, use):
    """B = 832 (13 magnitudes |w| from 0 over the Taylor boundary 0.01, pi and 2 pi to 30, 64 twists each; samples straddle
    workgroups in both kernels) against LieAlgebra.se3.exp3 in float64.  Per magnitude group and output the largest
    absolute error is at most 4 x that of the float32 host evaluation of the same formulas (the device's sinf / cosf:
    1-2 ulp against libm's half; FMA contraction) + 8 float32 roundings (2^-24) of the group's largest value (the host is
    exact at |w| = 0 and 1e-20).  The yardstick is per group because the formulas' own float32 error differs by three orders
    of magnitude: just above the boundary (t - sin t) / t^3 cancels (gxi 7.5e-4 at |w| = 0.0101 against 3e-7 at 0.0099).
    "R only" / "T only": the other output is unused in the contraction (autograd hands the backward zeros for it)."""
    c, ref, host = se3
    R, T, gxi = run_se3(c, use_R=use[0], use_T=use[1])
    got = dict(R=R.cpu().numpy(), T=T.cpu().numpy(), gxi=gxi.cpu().numpy())
    assert got["gxi"].shape == (832, 6) and np.all(np.isfinite(got["gxi"]))
    errs, yard = PR.se3_group_errors(got, ref[use]), PR.se3_yardstick(ref[use], host[use])
    print("\n" + PR.se3_table(errs, yard))
    for k in ("R", "T", "gxi"):
        over = [(PR.SE3_MAGS[g], errs[k][g], yard[k][1][g]) for g in range(len(PR.SE3_MAGS)) if not errs[k][g] <= yard[k][1][g]]
        assert not over, f"{k}: (|w|, error, allowed) {over}"
    # |w| = 0: the identity and T = v, bit for bit
    n0 = PR.SE3_PER_MAG
    assert PR.SE3_MAGS[0] == 0.0
    np.testing.assert_array_equal(got["R"][:n0], np.broadcast_to(np.eye(3, dtype=np.float32), (n0, 3, 3)))
    np.testing.assert_array_equal(got["T"][:n0], c["xi"][:n0, 3:])


@pytest.mark.parametrize("chunk", PR.SE3_CHUNKS)
def test_se3_sample_does_not_depend_on_its_place_in_the_batch(L, se3, chunk):
    """Every sample of the B = 832 call equals, bit for bit, forward and backward, the same twist evaluated in calls of
    `chunk` twists (1: alone; 10 / 11: the first sizes at which the backward's 6 lanes per sample stay in / leave one
    workgroup; 64 / 65: one and two workgroups of the forward)."""
    c = se3[0]
    R, T, gxi = (bits(v) for v in run_se3(c))
    for a in range(0, 832, chunk):
        rows = slice(a, min(832, a + chunk))
        r, t, g = (bits(v) for v in run_se3(c, rows))
        assert np.array_equal(r, R[rows]) and np.array_equal(t, T[rows]), (chunk, a)
        assert np.array_equal(g, gxi[rows]), (chunk, a, np.argwhere(g != gxi[rows])[:4])


def test_se3_backward_with_a_missing_upstream_gradient(L, se3):
    """rrl_se3_exp_bwd with gR == NULL and with gT == NULL (the C entry directly: autograd materialises zeros): the same
    bits as a zero tensor in its place and as the wrapper's one-sided contractions."""
    from rrl_hip import ops
    c = se3[0]
    P = ops._p
    x, cR, cT = cu(c["xi"]), cu(c["cR"]), cu(c["cT"])
    B = x.shape[0]

    def bwd(gR, gT):
        out = torch.full((B, 6), float("nan"), device="cuda")
        ops._run(x.device, "rrl_se3_exp_bwd", P(x), P(gR), P(gT), P(out), B)
        return out
    only_R, only_T, full = bwd(cR, None), bwd(None, cT), bwd(cR, cT)
    assert torch.equal(only_R, bwd(cR, torch.zeros_like(cT))) and torch.equal(only_T, bwd(torch.zeros_like(cR), cT))
    assert torch.isfinite(full).all() and torch.equal(full, run_se3(c)[2])
    assert torch.equal(only_R, run_se3(c, use_T=False)[2]) and torch.equal(only_T, run_se3(c, use_R=False)[2])
    assert torch.equal(only_R[:, 3:], torch.zeros(B, 3, device="cuda"))  # R does not depend on v


# ----------------------------------------------------------------------------------------------------------------- Adam
def run_adam(c, rows=slice(None)):
    """The 8 steps of a pose_refs Adam case on the parameters `rows`: (p after every step (8, n), m, v, state) on the host."""
    from rrl_hip import ops
    p = cu(c["p0"][rows].copy())
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    state, lr = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")
    trail = []
    for it in range(PR.ADAM_STEPS):
        lr.fill_(c["lrs"][it])
        gate = torch.tensor([c["gates"][it], 0, 0, 0], dtype=torch.int32, device="cuda")
        ops.adam_gated(p, cu(c["grads"][it][rows]), m, v, state, lr, gate)
        trail.append(p.cpu().numpy())
    return np.stack(trail), m.cpu().numpy(), v.cpu().numpy(), float(state[0])


@pytest.mark.parametrize("n", PR.ADAM_N)
def test_adam_gated_beyond_one_pass_of_the_workgroup(L, n):
    """adam_gated_kernel is ONE workgroup of 256 lanes looping over the parameters: 1, 255, 256, 257 and 1000 of them
    against torch.optim.Adam on the CPU over 8 steps (two gated off, one learning-rate change) at the tolerance of
    test_adam_gated_kernel_vs_torch_adam; the step count advances once per ungated call whatever n is."""
    c = PR.adam_case(n)
    ref = PR.adam_reference(c)
    trail, m, v, state = run_adam(c)
    for it in range(PR.ADAM_STEPS):
        np.testing.assert_allclose(trail[it], ref[it], rtol=1e-6, atol=2e-8, err_msg=f"step {it}")
        if not c["gates"][it]:
            np.testing.assert_array_equal(trail[it], trail[it - 1])
    assert state == float(sum(1 for q in c["gates"] if q)) == 6.0
    assert np.all(trail[-1] != c["p0"]) and np.all(m != 0) and np.all(v > 0)  # every parameter was updated


def test_adam_gated_elementwise_equals_calls_of_at_most_256(L):
    """p, m, v of the n = 1000 run equal, element by element, the same elements run as separate calls of 256, 256, 256 and
    232 parameters (each with its own step count): a parameter's update does not depend on the pass that reaches it."""
    c = PR.adam_case(1000)
    trail, m, v, state = run_adam(c)
    for a in range(0, 1000, 256):
        rows = slice(a, min(1000, a + 256))
        t1, m1, v1, s1 = run_adam(c, rows)
        assert s1 == state == 6.0
        np.testing.assert_array_equal(t1.view(np.uint32), trail[:, rows].view(np.uint32))
        np.testing.assert_array_equal(m1.view(np.uint32), m[rows].view(np.uint32))
        np.testing.assert_array_equal(v1.view(np.uint32), v[rows].view(np.uint32))


# ----------------------------------------------------------------------------------------------------------------- Chamfer
@pytest.fixture(params=[True, False], ids=["tree", "brute force"])
def route(request):
    """Both forward routes of ops.chamfer (they leave the same keys for the backward)."""
    from rrl_hip import ops
    keep = ops.CHAMFER_TREE
    ops.CHAMFER_TREE = request.param
    yield request.param
    ops.CHAMFER_TREE = keep


def run_chamfer(x, y, gval, x_grad=True, y_grad=True):
    """(value, gx, gy) of gval * ops.chamfer(x, y); a gradient is None where its input does not require it."""
    from rrl_hip import ops
    xg, yg = cu(x, x_grad), cu(y, y_grad)
    val = ops.chamfer(xg, yg)
    (val * gval).backward()
    assert (xg.grad is not None) == x_grad and (yg.grad is not None) == y_grad
    return (float(val), xg.grad.cpu().numpy() if x_grad else None, yg.grad.cpu().numpy() if y_grad else None)


@pytest.mark.parametrize("shape", PR.CHAMFER_SHAPES + [PR.CHAMFER_ONE_TARGET], ids=str)
def test_chamfer_backward_exact_on_the_integer_grid(L, route, shape):
    """Integer coordinates in [-8, 8] (heavy ties: the first nearest neighbour counts), B (N + M) a power of two and an
    upstream gradient of 4 or -0.5: gx AND gy equal the int64 / float64 reference bit for bit, with both inputs requiring
    grad, with only x, and with only y (gx == NULL).  The last shape has one target point repeated: every query scatters
    into target 0, 768 atomics onto one address."""
    B, N, M = shape
    x, y = PR.chamfer_int_case(41 + N, B, N, M, one_target=shape == PR.CHAMFER_ONE_TARGET)
    ix, iy, value = PR.chamfer_nearest(x, y, np.int64)
    for gval in PR.CHAMFER_GVALS:
        ref = PR.chamfer_backward_reference(x, y, ix, iy, gval)
        for xg, yg in ((True, True), (True, False), (False, True)):
            val, gx, gy = run_chamfer(x, y, gval, xg, yg)
            assert val == float(np.float32(value)), (gval, xg, yg)
            for got, k in ((gx, "gx"), (gy, "gy")):
                if got is None:
                    continue
                assert got.dtype == np.float32
                bad = np.argwhere(got.astype(np.float64) != ref[k])
                assert len(bad) == 0, f"{k} (gval {gval}, grads {(xg, yg)}): {len(bad)} entries differ, first {bad[0]}: {got[tuple(bad[0])]} != {ref[k][tuple(bad[0])]}"


def test_chamfer_backward_general_floats(L, route):
    """(3, 300, 257) standard normal, upstream gradient -2.5: every entry of gx and gy within (k + 3) 2^-24 sum
    |contributions| of float64, k = the entry's number of contributions from the nearest-neighbour lists -- 3 roundings per
    term (the scale's division, the subtraction, the product) and k - 1 for a sum of k terms in any order.  The lists are
    the same in float32 and float64 for this case (tests/test_pose_refs_host.py)."""
    x, y = PR.chamfer_float_case()
    ix, iy, value = PR.chamfer_nearest(x, y, np.float64)
    ref = PR.chamfer_backward_reference(x, y, ix, iy, PR.CHAMFER_FLOAT_GVAL)
    for xg, yg in ((True, True), (False, True)):
        val, gx, gy = run_chamfer(x, y, PR.CHAMFER_FLOAT_GVAL, xg, yg)
        # a float32 squared distance carries <= 5 roundings (the squares of rounded differences count twice), the mean one more
        assert abs(val - value) <= 8 * PR.U32 * value
        for got, s in ((gx, "x"), (gy, "y")):
            if got is None:
                continue
            err, bound = np.abs(got - ref["g" + s]), (ref["k" + s][..., None] + 3) * PR.U32 * ref["a" + s]
            print(f"g{s}: largest error / bound {np.max(err / bound):.3f}, most contributions to one point {ref['k' + s].max()}")
            assert np.all(err <= bound), (s, np.max(err / bound))
