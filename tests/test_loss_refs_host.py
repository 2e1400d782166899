"""Ties tests/loss_refs.py -- the float64 twin of the stages behind the scan -- to the reference before anything trusts it,
and shows on the CPU that the bounds of tests/test_gpu_loss_stages.py are met by a correct float32 implementation (the C
oracle) on every input set that file uses.  CPU only."""
import numpy as np
import pytest

import loss_cases
import loss_refs as R
from conftest import load_golden, merge_by_point
from test_oracle_golden import LOSS_FIXTURES

WIDE = load_golden("loss_wide.npz")


def twin(oracle, tri1, tri2, lines, rng, dtype=np.float64, grad_out=1.0):
    s1, s2 = oracle.scan(tri1, lines, cap=8), oracle.scan(tri2, lines, cap=8)
    return R.post_scan_ref(tri1, tri2, s1, s2, rng, grad_out, dtype)


def reference_order(ref, key="D"):
    return np.concatenate([ref["blocks"][kj][key].reshape(-1) for kj in sorted(ref["blocks"])])


def against_golden(tri1, ref, loss, grad1, D, what):
    assert abs(float(ref["loss"]) - float(loss)) <= 1e-6 * abs(float(loss)), what
    want, mine = merge_by_point(tri1, grad1), merge_by_point(tri1, ref["g1"])
    assert np.abs(mine - want).max() <= 3e-6 * np.abs(want).max(), what
    if D is not None:
        mine = reference_order(ref)
        assert len(mine) == len(D) == ref["n_values"], what
        np.testing.assert_allclose(mine, D, rtol=2e-5, atol=1e-9, err_msg=what)


@pytest.mark.parametrize("name", LOSS_FIXTURES)
def test_twin_reproduces_the_golden_fixtures(oracle, name):
    """Every range of every single-sample fixture: golden loss within 1e-6 relative, golden per-point gradient within 3e-6
    of the largest entry, golden D within rtol 2e-5."""
    g = load_golden(name)
    for i, rng in enumerate(g["ranges"]):
        ref = twin(oracle, g["tri1"], g["tri2"], g["lines"], tuple(int(v) for v in rng))
        against_golden(g["tri1"], ref, g[f"r{i}_loss"], g[f"r{i}_grad1"], g[f"r{i}_D"], (name, i))
        assert abs(float(ref["med"]) - float(g[f"r{i}_median"])) <= 2e-5 * float(ref["med"])


@pytest.mark.parametrize("name", [str(n) for n in WIDE["fixtures"]])
def test_twin_reproduces_the_wide_ranges(oracle, name):
    g = load_golden(f"loss_{name}.npz")
    for i, rng in enumerate(WIDE["ranges"]):
        ref = twin(oracle, g["tri1"], g["tri2"], g["lines"], tuple(int(v) for v in rng))
        if bool(WIDE[f"{name}_r{i}_empty"]):
            assert ref is None
            continue
        against_golden(g["tri1"], ref, WIDE[f"{name}_r{i}_loss"], WIDE[f"{name}_r{i}_grad1"], WIDE[f"{name}_r{i}_D"], (name, i))
    if name == str(WIDE["grad2_pair"]):
        ref = twin(oracle, g["tri1"], g["tri2"], g["lines"], tuple(int(v) for v in WIDE["grad2_range"]))
        want, mine = merge_by_point(g["tri2"], WIDE["grad2_grad2"]), merge_by_point(g["tri2"], ref["g2"])
        assert np.abs(mine - want).max() <= 3e-6 * np.abs(want).max()


def test_twin_pooled_and_empty(oracle):
    g = load_golden("loss_b2_quirk.npz")
    s1 = [oracle.scan(g["tri1"][b], g["lines"][b], cap=8) for b in range(2)]
    s2 = [oracle.scan(g["tri2"][b], g["lines"][b], cap=8) for b in range(2)]
    ref = R.post_scan_ref(list(g["tri1"]), list(g["tri2"]), s1, s2, (1, 1, 5, 5), pool=True)
    assert abs(float(ref["loss"]) - float(g["loss"])) <= 1e-6 * abs(float(g["loss"]))
    for b in range(2):
        want, mine = merge_by_point(g["tri1"][b], g["grad1"][b]), merge_by_point(g["tri1"][b], ref["g1"][b])
        assert np.abs(mine - want).max() <= 3e-6 * np.abs(want).max()
    e = load_golden("loss_edge_allmiss.npz")
    assert twin(oracle, e["tri1"], e["tri2"], e["lines"], (1, 1, 5, 5)) is None


@pytest.mark.parametrize("name,rng", [("loss_synth_s0.npz", (1, 1, 5, 5)), ("loss_ref_human0.npz", (1, 1, 9, 9)),
                                      ("loss_demo_scale.npz", (1, 2, 3, 5))])
def test_numpy_backward_equals_autograd_and_finite_differences(oracle, name, rng):
    """The written-out backward against torch's float64 autograd of the same forward (1e-12 relative), and a central
    finite difference of the float64 loss along 8 random directions of tri1 and of tri2 (1e-6 relative) with the median
    and the labels frozen, as the reference detaches them."""
    g = load_golden(name)
    ref = twin(oracle, g["tri1"], g["tri2"], g["lines"], rng, grad_out=-0.75)
    loss, a1, a2 = R.post_scan_torch(g["tri1"], g["tri2"], ref, rng, grad_out=-0.75)
    assert abs(loss - float(ref["loss"])) <= 1e-13 * abs(loss)
    for mine, auto in ((ref["g1"], a1), (ref["g2"], a2)):
        assert np.abs(mine - auto).max() <= 1e-12 * np.abs(auto).max()
    for key in ("1", "2"):  # the bookkeeping of the bound: |g| <= a, k counts, nothing where nothing contributes
        assert np.all(np.abs(ref["g" + key]) <= ref["a" + key] * (1 + 1e-12)) and np.all((ref["k" + key] > 0) == (ref["a" + key] > 0))
    gen = np.random.default_rng(11)
    t1, t2 = g["tri1"].astype(np.float64), g["tri2"].astype(np.float64)
    for which in (0, 1):
        base = (t1, t2)[which]
        for _ in range(8):
            # a direction per 3-D POINT: rows such as [A, B, C] and [B, A, C] tie exactly, and moving them apart would
            # put the difference quotient on the kink of the min (conftest.merge_by_point)
            _, inv = np.unique(base.reshape(-1, 3), axis=0, return_inverse=True)
            v = gen.standard_normal((inv.max() + 1, 3))[inv.reshape(-1)].reshape(base.shape)
            h = 1e-6 * np.abs(base).max()
            hi = R.post_scan_torch(*((t1 + h * v, t2) if which == 0 else (t1, t2 + h * v)), ref, rng)[0]
            lo = R.post_scan_torch(*((t1 - h * v, t2) if which == 0 else (t1, t2 - h * v)), ref, rng)[0]
            fd, an = -0.75 * (hi - lo) / (2 * h), float(((ref["g1"], ref["g2"])[which] * v).sum())
            assert abs(fd - an) <= 1e-6 * abs(an), (which, fd, an)


def test_rigid_grads_ref():
    """dL/dR, dL/dt from a per-point gradient against a finite difference of sum(g . (src m + t))."""
    gen = np.random.default_rng(2)
    src, g = gen.standard_normal((50, 9)), gen.standard_normal((50, 9))
    Rm, t = np.linalg.qr(gen.standard_normal((3, 3)))[0], gen.standard_normal(3)
    for tr in (False, True):
        gR, gt = R.rigid_grads_ref(src, Rm, t, g, tr)
        f = lambda Rx, tx: float((g.reshape(-1, 3) * (src.reshape(-1, 3) @ (Rx.T if tr else Rx) + tx)).sum())  # noqa: E731
        for i in range(3):
            e = np.zeros(3)
            e[i] = 1e-6
            assert abs((f(Rm, t + e) - f(Rm, t - e)) / 2e-6 - gt[i]) <= 1e-6 * np.abs(gt).max()
            for j in range(3):
                E = np.zeros((3, 3))
                E[i, j] = 1e-6
                assert abs((f(Rm + E, t) - f(Rm - E, t)) / 2e-6 - gR[i, j]) <= 1e-6 * np.abs(gR).max()


def oracle_inside_the_bounds(oracle, s, rng, what):
    """One sample (tri1, tri2, lines): the input conditions, and the C oracle's loss, median and per-point gradients inside
    the bounds the GPU test applies.  Returns the figures."""
    tri1, tri2, lines = s.get("moved", s["tri1"]), s["tri2"], s["lines"]
    s1, s2 = oracle.scan(tri1, lines, cap=8), oracle.scan(tri2, lines, cap=8)
    assert not s1["nan"] and not s2["nan"], what
    r64 = R.post_scan_ref(tri1, tri2, s1, s2, rng)
    r32 = R.post_scan_ref(tri1, tri2, s1, s2, rng, dtype=np.float32)
    assert r64 is not None and r64["n_selected"] >= 64, what
    assert r64["tie_share"] <= loss_cases.TIE_CAP, (what, r64["tie_share"])
    o = oracle.loss(tri1, tri2, lines, rng=rng, want_grad2=True, want_D=True)
    assert (o["n_selected"], o["n_values"], o["n_buckets"]) == (r64["n_selected"], r64["n_values"], r64["n_buckets"])
    # D and the median
    D64, ED = reference_order(r64), reference_order(r64, "ED")
    rD = float((np.abs(o["D"] - D64) / ED).max())
    assert rD <= 1.0, (what, rD)
    rank = (len(D64) - 1) // 2
    assert np.sort(D64 - ED)[rank] <= float(o["median"]) <= np.sort(D64 + ED)[rank], what
    # the loss
    bl = R.scalar_bound(r64["loss"], r32["loss"])
    assert abs(float(o["loss"]) - float(r64["loss"])) <= bl, (what, float(o["loss"]), float(r64["loss"]), bl)
    ex1, ex2 = R.tie_points(tri1, tri2, r64["blocks"])
    w1, t1 = R.check_grad(f"{what} grad1", tri1, o["grad1"], r64, r32, "1", merge_by_point, ex1)
    w2, t2 = R.check_grad(f"{what} grad2", tri2, o["grad2"], r64, r32, "2", merge_by_point, ex2)
    print(f"{what}: selected {r64['n_selected']}, near-tie share {r64['tie_share']:.4f}, D error / bound {rD:.3f}, loss error "
          f"{abs(float(o['loss']) - float(r64['loss'])):.2e} (float32 twin {abs(float(r32['loss']) - float(r64['loss'])):.2e}, bound {bl:.2e})")
    print("  " + t1 + "\n  " + t2)
    assert w1 <= 1.0 and w2 <= 1.0, (what, w1, w2)


@pytest.mark.parametrize("far", [False, True])
@pytest.mark.parametrize("scale", loss_cases.SCALES)
def test_oracle_meets_the_bounds_at_every_scale(oracle, scale, far):
    oracle_inside_the_bounds(oracle, loss_cases.scaled_pair(oracle, scale, far), (1, 1, 5, 5), f"scale {scale} far {far}")


def test_scale_at_which_nothing_is_selected(oracle):
    s = loss_cases.scaled_pair(oracle, 0.01, False)
    o = oracle.loss(s["tri1"], s["tri2"], s["lines"])
    assert o["loss"] is None and o["n_selected"] == 0 and not o["nan"]


@pytest.mark.parametrize("name", sorted(loss_cases.HOST_SETS))
def test_oracle_meets_the_bounds_on_every_input_set(oracle, name):
    """Every input set of the GPU file that is built on the host: NaN flag clear, at least 64 selected lines, near-tie share
    under the cap, and the oracle inside every bound."""
    samples, rng = loss_cases.HOST_SETS[name](oracle)
    for b, s in enumerate(samples):
        if s.get("empty"):
            assert oracle.loss(s.get("moved", s["tri1"]), s["tri2"], s["lines"], rng=rng)["n_selected"] == 0
            continue
        oracle_inside_the_bounds(oracle, s, rng, f"{name}[{b}]")


def test_ragged_base_set_meets_the_input_conditions(oracle):
    """The BASE batch of tests/ragged_cases.py (fixed by that file, not searched): NaN flags clear and the near-tie share of
    the SET under the cap (its samples select 230 ... 360 lines each, where a single tie is 0.3 ... 0.4 %)."""
    import ragged_cases
    ties = selected = 0
    for s in ragged_cases.batch(oracle, "BASE")[3]:
        s1, s2 = oracle.scan(s["tri1"], s["lines"], cap=8), oracle.scan(s["tri2"], s["lines"], cap=8)
        assert not s1["nan"] and not s2["nan"]
        ref = R.post_scan_ref(s["tri1"], s["tri2"], s1, s2, (1, 1, 5, 5))
        ties, selected = ties + ref["n_tie"], selected + ref["n_selected"]
        assert ref["n_selected"] >= 64
    assert ties <= loss_cases.TIE_CAP * selected


def test_bucket_sum_bound_term_by_term(oracle):
    """Why the bucket sums are held to the float32 twin's error term by term and not to |x32 - x64| of the two sums: a second
    correct float32 evaluation of the same twin (the intersection point with another association and a reciprocal, `alt`)
    leaves the plain form 4 |x32 - x64| + 8 u |x64| on these sets -- by 1.6 x at scale 5000 with the offset, bucket (2, 3),
    where the first evaluation's term errors happen to cancel to 2.8e-7 and the second's add up to 3.0e-5 of a sum of 36.8
    -- and stays inside the term-by-term form everywhere (at most half of it)."""
    worst_plain = worst_used = 0.0
    for s, rng in [(loss_cases.scaled_pair(oracle, 5000.0, True), (1, 1, 5, 5)), (loss_cases.scaled_pair(oracle, 300.0, True), (1, 1, 5, 5))] + \
            [(s, (1, 1, 5, 5)) for s in loss_cases.route_batch(oracle, 600)]:
        tri1 = s.get("moved", s["tri1"])
        s1, s2 = oracle.scan(tri1, s["lines"], cap=8), oracle.scan(s["tri2"], s["lines"], cap=8)
        r64, r32, alt = (R.post_scan_ref(tri1, s["tri2"], s1, s2, rng, dtype=d, alt=a)
                         for d, a in ((np.float64, False), (np.float32, False), (np.float32, True)))
        for kj in r64["bcnt"]:
            for key in ("rows", "cols"):
                x64, used, plain = R.bucket_sum_bounds(r64, r32, kj, key)
                err = abs(float(alt[key][kj]) - x64)
                worst_plain, worst_used = max(worst_plain, err / plain), max(worst_used, err / used)
    print(f"a second float32 evaluation of the bucket sums: {worst_plain:.3f} of the plain form, {worst_used:.3f} of the term-by-term one")
    assert worst_used <= 1.0 < worst_plain
