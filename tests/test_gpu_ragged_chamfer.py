"""The ragged Chamfer distance on the GPU (include/rrl.h rrl_chamfer_tree_fwd_counted / rrl_chamfer_bwd_counted; DESIGN.md
"Ragged batches"): B pairs whose clouds differ in size in ONE call.  The bar: the keys of a sample's present rows are the
oracle's on the truncated pair bit for bit (minimum bits << 32 | first argmin), the key rows beyond a count are all-ones,
rows beyond a count are never read as data -- NaN, zeros and DECOYS (copies of the other cloud's present points: any read
makes a zero-distance minimum) give identical outputs -- and get a zero gradient, and the counts are read on the device.

values[b] and value are compared with the float64 mean of the oracle's minima, rounded to float32, within ONE float32 ulp:
the kernel's fixed-order double sums of <= 2^21 float32 terms err by << 2^-24 relative, so only the final rounding can differ.
Inputs: tests/ragged_chamfer_cases.py (shown unambiguous by tests/test_ragged_chamfer_host.py)."""
import numpy as np
import pytest
import torch

import pose_refs as PR
import ragged_chamfer_cases as CC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from rrl_hip import _lib, ops
    _lib.load()
    assert torch.cuda.is_available()
    return ops


def cu(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda().requires_grad_(grad)


def i32(v):
    return torch.tensor(v, dtype=torch.int32, device="cuda")


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def run(ops, x, y, cx, cy, **kw):
    """(values, value, best_x, best_y) as numpy arrays."""
    out = ops._chamfer_counted(cu(x), cu(y), i32(cx) if cx is not None else None, i32(cy) if cy is not None else None, **kw)
    return tuple(t.detach().cpu().numpy() for t in out)


def one_ulp(got, want, what):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    print(f"{what}: got {got}, reference {want}, |diff| in ulps {np.max(err / np.spacing(np.abs(want)).astype(np.float64)) if want.size else 0}")
    assert np.all(err <= np.spacing(np.abs(want)).astype(np.float64)), (what, got, want)


def check_against_oracle(oracle, out, x, y, cx, cy, what):
    vals, val, bx, by = out
    parts, ref_vals, ref_val = CC.reference(oracle, x, y, cx, cy)
    for b, p in enumerate(parts):
        wx = CC.expected_keys(None if p is None else (p[0], p[1]), cx[b] if p is not None else 0, x.shape[1])
        wy = CC.expected_keys(None if p is None else (p[2], p[3]), cy[b] if p is not None else 0, y.shape[1])
        bad = np.flatnonzero(bx[b] != wx)
        assert len(bad) == 0, f"{what}: best_x[{b}] differs at {bad[:8]} ({len(bad)} rows): {bx[b][bad[:4]]} != {wx[bad[:4]]}"
        bad = np.flatnonzero(by[b] != wy)
        assert len(bad) == 0, f"{what}: best_y[{b}] differs at {bad[:8]} ({len(bad)} rows): {by[b][bad[:4]]} != {wy[bad[:4]]}"
        if p is None:
            assert bits(vals[b]) == 0, (what, b, vals[b])  # +0.0
    live = [b for b, p in enumerate(parts) if p is not None]
    one_ulp(vals[live], ref_vals[live], f"{what}: values")
    one_ulp(val, ref_val, f"{what}: value")


def same_outputs(a, b, what):
    for u, v, k in zip(a, b, ("values", "value", "best_x", "best_y")):
        u, v = (bits(u), bits(v)) if u.dtype == np.float32 else (u, v)
        assert np.array_equal(u, v), f"{what}: {k} differs"


@pytest.fixture(scope="module")
def fillers_out(ops):
    """The outputs of a float case under its three fillers, computed once per case."""
    memo = {}

    def get(name):
        if name not in memo:
            memo[name] = {f: run(ops, *CC.float_case(name, f)) for f in CC.FILLERS}
        return memo[name]
    return get


# ------------------------------------------------------------------------------------------------------------ 1, 4: edges
@pytest.mark.parametrize("name", ["edges", "wide_sort"])
def test_present_keys_are_the_oracles_and_absent_rows_are_never_read(ops, oracle, fillers_out, name):
    """1 (B = 4, 130 / 200: counts 1, 17, 63, 64, 65, 129 and the capacities) and 4 (4097 / 4200: the whole-cloud sort beyond
    4096, counts on both sides of it): keys, values and value against the oracle, and the three fillers give the same bits."""
    outs = fillers_out(name)
    x, y, cx, cy = CC.float_case(name, "decoy")
    check_against_oracle(oracle, outs["decoy"], x, y, cx, cy, name)
    for f in ("nan", "zero"):
        same_outputs(outs[f], outs["decoy"], f"{name}: filler {f} against decoys")


# ------------------------------------------------------------------------------------------------------------ 2: zero counts
def test_zero_counts(ops, oracle, fillers_out):
    """counts (0, 70), (70, 0), (5, 5): a sample with an empty cloud has no minima -- values 0, every key all-ones --, value is
    sample 2's; a call whose counts are all zero gives value 0."""
    outs = fillers_out("zero_counts")
    x, y, cx, cy = CC.float_case("zero_counts", "decoy")
    check_against_oracle(oracle, outs["decoy"], x, y, cx, cy, "zero_counts")
    vals, val, bx, by = outs["nan"]
    same_outputs(outs["nan"], outs["decoy"], "zero_counts: NaN filler")
    assert bits(vals[0]) == 0 and bits(vals[1]) == 0 and vals[2] > 0
    assert bits(val) == bits(vals[2])  # the same double sum over the same denominator
    assert (bx[:2] == -1).all() and (by[:2] == -1).all() and (bx[2, 5:] == -1).all() and (bx[2, :5] != -1).all()
    vals0, val0, bx0, by0 = run(ops, x, y, [0, 0, 0], [0, 70, 0])
    assert bits(val0) == 0 and (bits(vals0) == 0).all() and (bx0 == -1).all() and (by0 == -1).all()


# ------------------------------------------------------------------------------------------------------------ 3: counts = capacities
def test_counts_at_the_capacities_are_the_uniform_call(ops, oracle):
    """B = 2, 300 / 257: keys and value bit-equal to rrl_chamfer_tree_fwd on the same tensors; values[b] bit-equal to the
    B = 1 uniform call's value (absent patches add +0.0 at the same lane positions of the same fixed-order sums).  Also with
    per_sample / counts through the public entries."""
    import loss
    x, y, cx, cy = CC.float_case("full")
    xs, ys = cu(x), cu(y)
    B, N, M = x.shape[0], x.shape[1], y.shape[1]
    nb = ops._scratch_size("rrl_chamfer_workspace_bytes", B, N, M)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    ubx, uby = torch.empty(B, N, dtype=torch.int64, device="cuda"), torch.empty(B, M, dtype=torch.int64, device="cuda")
    uval = torch.empty(1, device="cuda")
    ops._run(xs.device, "rrl_chamfer_tree_fwd", ops._p(xs), ops._p(ys), ops._p(ws), nb, ops._p(ubx), ops._p(uby), ops._p(uval), B, N, M)
    out = run(ops, x, y, cx, cy)
    vals, val, bx, by = out
    assert np.array_equal(bx, ubx.cpu().numpy()) and np.array_equal(by, uby.cpu().numpy())
    assert bits(val) == bits(uval.cpu().numpy()[0]), (val, uval)
    assert bits(val) == bits(ops.chamfer(xs, ys).cpu().numpy())
    for b in range(B):
        one = ops.chamfer(xs[b:b + 1], ys[b:b + 1]).cpu().numpy()
        assert bits(vals[b]) == bits(one), (b, vals[b], one, int(bits(vals[b])) - int(bits(one)))
    check_against_oracle(oracle, out, x, y, cx, cy, "full")
    same_outputs(run(ops, x, y, None, None), out, "per_sample without counts")
    assert np.array_equal(bits(ops.chamfer(xs, ys, per_sample=True).cpu().numpy()), bits(vals))
    assert np.array_equal(bits(loss.chamfer_dist(xs, ys, counts_x=cx, counts_y=cy, per_sample=True).cpu().numpy()), bits(vals))
    assert bits(loss.chamfer_dist(xs, ys, counts_x=i32(cx), counts_y=i32(cy)).cpu().numpy()) == bits(val)


# ------------------------------------------------------------------------------------------------------------ 5: prepared orders
def test_prepared_orders_give_the_same_bits(ops, oracle):
    """B = 2, 300 / 257, counts (300, 65) / (64, 257): the orders of ops.cloud_order(tri, counts=) on (B, n, 9) rows whose
    first three floats are the points replace the per-call sort; every output bit-equal to the unprepared ragged call."""
    x, y, cx, cy = CC.float_case("prepared", "nan")
    tri = lambda p: torch.cat([cu(p), torch.zeros(p.shape[0], p.shape[1], 6, device="cuda")], dim=2).contiguous()  # noqa: E731
    ox, oy = ops.cloud_order(tri(x), counts=i32(cx)), ops.cloud_order(tri(y), counts=i32(cy))
    for b in range(len(cx)):
        assert sorted(ox[b, :cx[b]].tolist()) == list(range(cx[b])) and sorted(oy[b, :cy[b]].tolist()) == list(range(cy[b]))
    plain = run(ops, x, y, cx, cy)
    same_outputs(run(ops, x, y, cx, cy, order_x=ox, order_y=oy), plain, "prepared")
    check_against_oracle(oracle, plain, *CC.float_case("prepared", "decoy"), "prepared (unprepared call)")


# ------------------------------------------------------------------------------------------------------------ 6: NaN
def test_nan_is_per_sample_and_over_present_rows_only(ops, oracle):
    """B = 2, 200 / 150, counts (200, 100) / (150, 90): a NaN in the present row x[1, 17] and NaNs in rows beyond the counts
    (ragged_chamfer_cases.nan_case).  The NaN pattern of the present minima is torch's on the truncated pairs; sample 0 and
    values[0] are finite, values[1] and value are NaN."""
    x, y, cx, cy = CC.nan_case()
    vals, val, bx, by = run(ops, x, y, cx, cy)
    mins = lambda k: (k.view(np.uint64) >> np.uint64(32)).astype(np.uint32).view(np.float32)  # noqa: E731
    for b in range(2):
        xt, yt = torch.from_numpy(x[b, :cx[b]]), torch.from_numpy(y[b, :cy[b]])
        d = ((xt[:, None, :] - yt[None, :, :]) ** 2).sum(-1)
        assert np.array_equal(np.isnan(mins(bx[b, :cx[b]])), torch.isnan(d.min(1).values).numpy()), b
        assert np.array_equal(np.isnan(mins(by[b, :cy[b]])), torch.isnan(d.min(0).values).numpy()), b
        assert (bx[b, cx[b]:] == -1).all() and (by[b, cy[b]:] == -1).all()
    assert not np.isnan(mins(bx[0])).any() and not np.isnan(mins(by[0])).any() and np.isfinite(vals[0])
    assert np.isnan(mins(bx[1, :cx[1]])).sum() == 1 and np.isnan(mins(by[1, :cy[1]])).all()
    assert np.isnan(vals[1]) and np.isnan(val)
    # sample 0 and the finite minima of sample 1 are the oracle's
    p0 = oracle.chamfer_parts(x[0], y[0])
    assert np.array_equal(bx[0], CC.expected_keys((p0[0], p0[1]), cx[0], x.shape[1]))
    assert np.array_equal(by[0], CC.expected_keys((p0[2], p0[3]), cy[0], y.shape[1]))
    one_ulp(vals[0], np.float32(np.concatenate([p0[0], p0[2]]).astype(np.float64).mean()), "nan case: values[0]")
    keep = np.arange(cx[1]) != 17
    p1 = oracle.chamfer_parts(x[1, :cx[1]][keep], y[1, :cy[1]])
    assert np.array_equal(bits(mins(bx[1, :cx[1]][keep])), bits(p1[0]))
    assert np.array_equal((bx[1, :cx[1]][keep] & 0xffffffff).astype(np.int32), p1[1])


# ------------------------------------------------------------------------------------------------------------ 7: device counts
def test_counts_live_on_the_device(ops):
    """One call, then new counts written IN PLACE into the same GPU tensors by device copies -- nothing of the first call is
    read back in between --, then the second call: equal to a fresh call with the new counts."""
    x, y, c1x, c1y = CC.float_case("device_counts", "nan")
    _, _, c2x, c2y = CC.float_case("device_counts_after", "nan")
    xs, ys, dcx, dcy = cu(x), cu(y), i32(c1x), i32(c1y)
    new_x, new_y = i32(c2x), i32(c2y)
    first = ops._chamfer_counted(xs, ys, dcx, dcy)
    dcx.copy_(new_x)
    dcy.copy_(new_y)
    second = ops._chamfer_counted(xs, ys, dcx, dcy)
    first, second = ([t.cpu().numpy() for t in o] for o in (first, second))
    same_outputs(first, run(ops, x, y, c1x, c1y), "first call")
    same_outputs(second, run(ops, x, y, c2x, c2y), "second call, counts written in place")
    assert not np.array_equal(first[2], second[2])


# ------------------------------------------------------------------------------------------------------------ 8: backward, exact
def _int_reference(x, y, cx, cy, gvals):
    gx, gy = np.zeros(x.shape, np.float64), np.zeros(y.shape, np.float64)
    for b in range(len(cx)):
        xs, ys = x[b:b + 1, :cx[b]], y[b:b + 1, :cy[b]]
        ix, iy, _ = PR.chamfer_nearest(xs, ys, np.int64)
        r = PR.chamfer_backward_reference(xs, ys, ix, iy, gvals[b])  # B = 1: the scale is 2 g / (cx + cy)
        gx[b, :cx[b]], gy[b, :cy[b]] = r["gx"][0], r["gy"][0]
    return gx, gy


@pytest.mark.parametrize("route", ["per_sample", "scalar"])
def test_backward_exact_on_the_integer_grid(ops, route):
    """B = 3, 256 / 256, counts (100, 156), (256, 256), (1, 255) on integer coordinates (heavy ties): x.grad and y.grad equal
    the int64 / float64 reference -- per sample, B = 1, that sample's scale -- bit for bit; absent rows exactly zero.  The
    per-sample route takes upstream (4, -0.5, 2), the scalar route 4 (the counts add up to 1024: every scale a power of two)."""
    seed, B, N, M, cx, cy = CC.BACKWARD_INT
    x, y = PR.chamfer_int_case(seed, B, N, M)
    xg, yg = cu(x, True), cu(y, True)
    if route == "per_sample":
        gvals = CC.BACKWARD_INT_UPSTREAM
        vals = ops.chamfer(xg, yg, counts_x=i32(cx), counts_y=i32(cy), per_sample=True)
        vals.backward(torch.tensor(gvals, device="cuda"))
    else:
        tot = sum(cx) + sum(cy)
        gvals = [CC.BACKWARD_INT_SCALAR * (cx[b] + cy[b]) / tot for b in range(B)]
        (ops.chamfer(xg, yg, counts_x=cx, counts_y=cy) * CC.BACKWARD_INT_SCALAR).backward()
    wx, wy = _int_reference(x, y, cx, cy, gvals)
    for got, want, cnt, k in ((xg.grad, wx, cx, "gx"), (yg.grad, wy, cy, "gy")):
        got = got.cpu().numpy()
        assert got.dtype == np.float32
        bad = np.argwhere(got.astype(np.float64) != want)
        assert len(bad) == 0, f"{k} ({route}): {len(bad)} entries differ, first {bad[0]}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"
        for b in range(B):
            assert not got[b, cnt[b]:].any() and got[b, :cnt[b]].any()


# ------------------------------------------------------------------------------------------------------------ 9: backward, floats
def test_backward_general_floats(ops):
    """B = 3, 300 / 257, counts (300, 1, 129) / (257, 200, 64), upstream (-2.5, 1.5, 0.75) on the per-sample values: every
    gradient entry with k contributions within (k + 3) 2^-24 sum |contributions| of the float64 reference (DESIGN section 6:
    three roundings per term -- the scale's division, the subtraction, the product -- and k - 1 for the sum); absent rows
    zero.  NaN beyond the counts."""
    x, y, cx, cy = CC.float_case("backward_float", "nan")
    xg, yg = cu(x, True), cu(y, True)
    ops.chamfer(xg, yg, counts_x=i32(cx), counts_y=i32(cy), per_sample=True).backward(torch.tensor(CC.BACKWARD_FLOAT_UPSTREAM, device="cuda"))
    gx, gy = xg.grad.cpu().numpy(), yg.grad.cpu().numpy()
    for b in range(len(cx)):
        xs, ys = x[b:b + 1, :cx[b]], y[b:b + 1, :cy[b]]
        ix, iy, _ = PR.chamfer_nearest(xs, ys, np.float64)
        r = PR.chamfer_backward_reference(xs, ys, ix, iy, CC.BACKWARD_FLOAT_UPSTREAM[b])
        for got, s, cnt in ((gx[b], "x", cx[b]), (gy[b], "y", cy[b])):
            err, bound = np.abs(got[:cnt] - r["g" + s][0]), (r["k" + s][0][:, None] + 3) * PR.U32 * r["a" + s][0]
            print(f"sample {b} g{s}: largest error / bound {np.max(err / bound):.3f}, most contributions to one point {r['k' + s].max()}")
            assert np.all(err <= bound), (b, s, np.max(err / bound))
            assert not got[cnt:].any()
