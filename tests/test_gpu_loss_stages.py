"""The stages behind the scan -- intersection points, D tiles, lower median, Welsch min / mean reduce and every backward
route of csrc/rrl_stage_pair.h, rrl_stage_reduce.h, rrl_stage_tail.h, rrl_stage_bwd.h and rrl_wide.hip -- held to the float64
twin of tests/loss_refs.py.

The boundary: the scan's outputs (COUNT, KJ, HS, W) equal the C oracle's BIT FOR BIT on the triangles the library itself
used (its own moved triangles where a pose is applied); everything behind them is compared with the twin evaluated in
float64 on the oracle's hit lists and float32 weights, with bounds that are derived (Q, D: loss_refs' docstring) or come
from the float32 evaluation of the same twin (loss, bucket sums, payload: 4 x its error + 8 roundings; gradients: the
error normalised by the sum of |contributions|, 4 x the float32 twin's worst + (k + 3) 2^-24; deterministic mode: + k 2^-37
of the largest possible contribution).  None of them is taken from the library's output.  The input sets come from
tests/loss_cases.py; tests/test_loss_refs_host.py shows on the CPU that the C oracle meets the same bounds on them.
Every test prints its largest observed value next to its bound (pytest -s)."""
import numpy as np
import pytest
import torch

import loss_cases as C
import loss_refs as R
from conftest import load_golden, merge_by_point
from pose_refs import U32

pytestmark = pytest.mark.gpu
NARROW = (1, 1, 5, 5)
FIX = 2.0 ** -40


@pytest.fixture(scope="module")
def L():
    import loss
    from rrl_hip import _lib
    _lib.load()
    assert torch.cuda.is_available()
    return loss


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def stack(samples, key):
    return np.stack([s[key] for s in samples])


# ---------------------------------------------------------------------------------------------------- the twin, once per input
_twins = {}


def twin_of(oracle, tri1, tri2, lines, rng):
    """(scan1, scan2, float64 twin, float32 twin) at upstream gradient 1, cached by content."""
    key = (tri1.tobytes(), tri2.tobytes(), lines.tobytes(), tuple(rng))
    key = (hash(key), tri1.shape, tri2.shape, lines.shape, tuple(rng))
    if key not in _twins:
        s1, s2 = oracle.scan(tri1, lines, cap=8), oracle.scan(tri2, lines, cap=8)
        assert not s1["nan"] and not s2["nan"]
        r64 = R.post_scan_ref(tri1, tri2, s1, s2, rng)
        r32 = R.post_scan_ref(tri1, tri2, s1, s2, rng, dtype=np.float32) if r64 is not None else None
        _twins[key] = (s1, s2, r64, r32)
    return _twins[key]


class Worst:
    """The largest error / bound ratio per quantity of one test, printed at its end."""

    def __init__(self, what):
        self.what, self.v, self.notes = what, {}, []

    def add(self, name, ratio):
        self.v[name] = max(self.v.get(name, 0.0), float(ratio))
        assert ratio <= 1.0, f"{self.what}: {name} error / bound = {ratio:.3f}"

    def show(self):
        print(f"\n[{self.what}] worst error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(self.v.items())))
        for n in self.notes:
            print("    " + n)


# ---------------------------------------------------------------------------------------------------- forward checks
def check_scan_outputs(st, b, s1, s2, rng, counts_cleared=False, nl=None):
    """COUNT, KJ, HS, W of sample b against the oracle's scan, bit for bit (HS / W where a line is selected)."""
    s_m, s_n, e_m, e_n = rng
    nl = len(s1["count"]) if nl is None else nl
    c1, c2 = s1["count"][:nl], s2["count"][:nl]
    sel = (c1 >= s_m) & (c1 < e_m) & (c2 >= s_n) & (c2 < e_n)
    kj = np.where(sel, c1 | (c2 << 4), 0).astype(np.uint8)
    np.testing.assert_array_equal(st.kj[b].cpu().numpy()[:nl], kj)
    if not counts_cleared:
        np.testing.assert_array_equal(st.count1[b].cpu().numpy()[:nl], c1)
        np.testing.assert_array_equal(st.count2[b].cpu().numpy()[:nl], c2)
    for cnt, sc, hs, w in ((c1, s1, st.hs1, st.w1), (c2, s2, st.hs2, st.w2)):
        hs, w = hs[b].cpu().numpy()[:nl], w[b].cpu().numpy()[:nl]
        live = sel[:, None] & (np.arange(4)[None, :] < cnt[:, None])
        np.testing.assert_array_equal(hs[live], sc["hit_idx"][:nl, :4][live])
        np.testing.assert_array_equal(w[live].view(np.uint32), sc["hit_w"][:nl, :4][live].view(np.uint32))
    return sel


def check_points_and_D(st, b, r64, worst):
    """Q1, Q2 and the D block of every selected line of sample b inside the derived bounds; returns the library's valid D
    values in the twin's order (bucket-major, then line)."""
    Q1, Q2, D = st.Q1[b].cpu().numpy(), st.Q2[b].cpu().numpy(), st.D[b].cpu().numpy()
    vals = []
    for (k, j), v in sorted(r64["blocks"].items()):
        ln = v["lines"]
        for Q, q, Eq, n in ((Q1, v["q1"], v["Eq1"], k), (Q2, v["q2"], v["Eq2"], j)):
            err = np.abs(Q[ln, :n, :3].astype(np.float64) - q)
            worst.add("Q", float(np.divide(err, Eq, out=np.where(err > 0, np.inf, 0.0), where=Eq > 0).max()))
        mine = D[ln, :k * j].reshape(-1, k, j)
        err = np.abs(mine.astype(np.float64) - v["D"])
        worst.add("D", float(np.divide(err, v["ED"], out=np.where(err > 0, np.inf, 0.0), where=v["ED"] > 0).max()))
        vals.append(mine.reshape(-1))
    return np.concatenate(vals)


def check_reduce(st, g, r64, r32, vals, worst, loss=None, bsum_stride=4):
    """MED, BCNT, BSUM, INFO and the loss of group g: counts by equality, the median an element of the library's own values
    at rank (n - 1) // 2 and inside the D bound of the twin's, sums and loss inside 4 x the float32 twin's error + 8 u."""
    info = st.info[g].cpu().numpy()
    assert list(info[:3]) == [r64["n_buckets"], r64["n_selected"], r64["n_values"]] and info[3] == 0
    med = st.med[g].cpu().numpy()
    rank = (len(vals) - 1) // 2
    assert len(vals) == r64["n_values"]
    assert med.view(np.uint32) == np.sort(vals)[rank].view(np.uint32)
    lo, hi = np.sort(r64["values"] - r64["EDvalues"])[rank], np.sort(r64["values"] + r64["EDvalues"])[rank]
    assert lo <= float(med) <= hi, (lo, float(med), hi)
    worst.add("median", abs(float(med) - float(r64["med"])) / max(hi - float(r64["med"]), float(r64["med"]) - lo, 1e-300))
    bcnt, bsum = st.bcnt[g].cpu().numpy(), st.bsum[g].cpu().numpy()
    want = np.zeros_like(bcnt)
    for (k, j), S in r64["bcnt"].items():
        bi = (k - 1) * bsum_stride + (j - 1)
        want[bi] = S
        for side, key in ((0, "rows"), (1, "cols")):
            x64, bound, plain = R.bucket_sum_bounds(r64, r32, (k, j), key)  # (term by term: see there)
            x = float(bsum[bi, side]) * FIX
            if abs(x - x64) > 0.5 * bound:
                worst.notes.append(f"group {g} bucket {(k, j)} {key}, S = {S}: sum {x64:.6e}, error {x - x64:.2e}, float32 host "
                                   f"{float(r32[key][(k, j)]) - x64:.2e}, bound {bound:.2e} (plain form {plain:.2e})")
            worst.add("bucket sums", abs(x - x64) / bound)
            worst.v["bucket sums / plain form"] = max(worst.v.get("bucket sums / plain form", 0.0), abs(x - x64) / plain)
    np.testing.assert_array_equal(bcnt, want)
    lv = float(st.loss[g]) if loss is None else float(loss)
    worst.add("loss", abs(lv - float(r64["loss"])) / R.scalar_bound(r64["loss"], r32["loss"]))
    worst.notes.append(f"group {g}: loss error {abs(lv - float(r64['loss'])):.2e}, float32 host "
                       f"{abs(float(r32['loss']) - float(r64['loss'])):.2e}, bound {R.scalar_bound(r64['loss'], r32['loss']):.2e}")


def check_forward(oracle, st, b, tri1, tri2, lines, rng, worst, counts_cleared=False, loss=None):
    """Everything the forward leaves for sample b (independent samples); returns (r64, r32) or None for an empty sample."""
    s1, s2, r64, r32 = twin_of(oracle, tri1, tri2, lines, rng)
    check_scan_outputs(st, b, s1, s2, rng, counts_cleared, len(lines))
    if r64 is None:
        assert list(st.info[b].cpu().numpy()[:3]) == [0, 0, 0] and float(st.loss[b] if loss is None else loss) == 0.0
        return None
    assert r64["tie_share"] <= C.TIE_CAP, r64["tie_share"]
    vals = check_points_and_D(st, b, r64, worst)
    check_reduce(st, b, r64, r32, vals, worst, loss)
    return r64, r32


# ---------------------------------------------------------------------------------------------------- backward checks
def check_point_grad(name, tri, got, twins, key, gl, worst, det, tri_other=None):
    r64, r32 = twins
    ex = R.tie_points(tri, tri_other, r64["blocks"])[0] if key == "1" else R.tie_points(tri_other, tri, r64["blocks"])[1]
    extra = (lambda k: R.det_extra(k, gl, r64["n_buckets"], r64["med"])) if det else None
    w, text = R.check_grad(name, tri, got, r64, r32, key, merge_by_point, ex, extra, scale=float(gl))
    worst.notes.append(text)
    worst.add(name.split("[")[0], w)


def check_rigid_grads(name, src, Rm, t, tr, got_R, got_t, twins, gl, worst):
    """dR, dt against rigid_grads_ref of the twin's point gradient: normalised by the sums of |contributions|, within 4 x
    the float32 twin's worst + (k + 3) u.  (A sum cannot leave the near-tie lines' points out; on these sets what they
    carry -- saturated Welsch terms -- disappears in that allowance.)"""
    r64, r32 = twins
    gl = float(gl)
    if gl == 0.0:
        assert not np.any(got_R) and not np.any(got_t), name
        return np.zeros(12), np.zeros(12)
    assert np.isfinite(got_R).all() and np.isfinite(got_t).all(), name
    g64 = np.concatenate([x.reshape(-1) for x in R.rigid_grads_ref(src, Rm, t, r64["g1"] * gl, tr)])
    g32 = np.concatenate([x.reshape(-1) for x in R.rigid_grads_ref(src, Rm, t, r32["g1"] * gl, tr)])
    aR, at = R.rigid_abs_sums(src, r64["a1"] * abs(gl), tr)
    a = np.concatenate([aR.reshape(-1), at])
    kcol = r64["k1"].reshape(-1, 3).sum(0)                       # contributions per coordinate of the moved points
    kR = np.tile(kcol, (3, 1)).T if tr else np.tile(kcol, (3, 1))  # gR[i][j] in R's layout sums coordinate i (tr) or j
    k = np.concatenate([kR.reshape(-1), kcol])
    bound, worst32 = R.grad_bound(g64, g32, a, k)
    allowed = bound * a
    err = np.abs(np.concatenate([got_R.reshape(-1), got_t.reshape(-1)]).astype(np.float64) - g64)
    worst.notes.append(f"{name}: normalised error device {float(R.normalised(err, a).max()):.3e}, float32 host {worst32:.3e}")
    assert not np.any(err[allowed == 0]), f"{name}: an output nothing contributes to must be exactly zero"
    worst.add(name.split("[")[0], float(np.divide(err, allowed, out=np.zeros_like(err), where=allowed > 0).max()))
    return g64, allowed


# ---------------------------------------------------------------------------------------------------- the entries
def run_entry(L, oracle, entry, samples, rng, gl, worst, det=False, mode="cull", reduce_mode=None, precondition=None):
    """One call form on one batch, held to the twin sample by sample.  entry: points1 | both | loss_step | loss_step_cold |
    registration | registration_src | registration_step.  Samples with a pose (loss_cases.with_pose) are moved by the
    library in the step / registration entries and handed over moved to the two entries that take points; samples
    without one go through the step / registration entries with the identity."""
    from rrl_hip import ops
    B = len(samples)
    with_pose = "R" in samples[0]
    tr = samples[0].get("tr", True)
    pts = entry in ("points1", "both")
    src, tar, ln = cu(stack(samples, "moved" if (pts and with_pose) else "tri1")), cu(stack(samples, "tri2")), cu(stack(samples, "lines"))
    glt = cu(np.asarray(gl, np.float32))
    Rm = cu(stack(samples, "R")) if with_pose else torch.eye(3).repeat(B, 1, 1).cuda()
    T = cu(stack(samples, "T")) if with_pose else torch.zeros(B, 3).cuda()
    nl = ln.shape[1]
    out = {}
    try:
        if reduce_mode is not None:
            ops.set_reduce_mode(reduce_mode)
        if entry in ("points1", "both"):
            ops.set_deterministic(det)
            p1 = src.clone().requires_grad_(True)
            p2 = tar.clone().requires_grad_(entry == "both")
            runs = []
            for _ in range(2 if det else 1):
                p1.grad = p2.grad = None
                loss, info, status = ops.intersection_loss(p1, p2, ln, rng, mode=mode)
                (loss * glt).sum().backward()
                runs.append((p1.grad.clone(), p2.grad.clone() if entry == "both" else None))
            st, moved = ops.last_state(), None
            out = dict(loss=loss.detach(), g1=runs[0][0], g2=runs[0][1])
        elif entry in ("loss_step", "loss_step_cold"):
            step = ops.LossStep(src, tar, nl, rng, transpose_r=tr, mode=mode, prepared=entry == "loss_step", deterministic=det or None)
            runs = []
            for _ in range(2):  # (prepared: the second call is the chained one)
                loss, g1, info = step(Rm, T, ln, grad_loss=glt) if with_pose else step(None, None, ln, grad_loss=glt)
                runs.append((g1.clone(), None))
            st, moved = step.st, (step.st.tri1t if with_pose else None)
            out = dict(loss=loss.clone(), g1=runs[1][0], g2=None, cleared=bool(getattr(st, "counts_cleared", False)))
        elif entry in ("registration", "registration_src"):
            ops.set_deterministic(det)
            s_ = src.clone().requires_grad_(entry == "registration_src")
            Rg, Tg = Rm.clone().requires_grad_(True), T.clone().requires_grad_(True)
            runs = []
            for _ in range(2 if det else 1):
                Rg.grad = Tg.grad = s_.grad = None
                loss, info, status = ops.registration_loss(s_, Rg, Tg, tar, ln, rng, transpose_r=tr, mode=mode)
                (loss * glt).sum().backward()
                runs.append((Rg.grad.clone(), Tg.grad.clone()))
            st = ops.last_state()
            moved = st.tri1t
            out = dict(loss=loss.detach(), gR=runs[0][0], gt=runs[0][1], gsrc=s_.grad)
        else:
            step = ops.RegistrationStep(src, tar, nl, rng, transpose_r=tr, mode=mode, want_payload=True, deterministic=det or None)
            runs = []
            for _ in range(2):
                loss, gR, gt, pay, info = step(Rm, T, ln, grad_loss=glt)
                runs.append((gR.clone(), gt.clone()))
            st, moved = step.st, step.st.tri1t
            out = dict(loss=loss.clone(), gR=runs[1][0], gt=runs[1][1], payload=pay.clone())
        torch.cuda.synchronize()
        if precondition is not None:
            precondition(st)
    finally:
        ops.set_deterministic(False)
        if reduce_mode is not None:
            ops.set_reduce_mode("auto")
    if det:  # two calls: bit-identical results
        for a, b in zip(runs[0], runs[1]):
            assert a is None or torch.equal(a, b), "deterministic mode: two calls differ"
    assert int(st.status[0]) == 0
    moved = moved.cpu().numpy() if moved is not None else None
    twins, pay_loss, pay_g, pay_a = [], 0.0, np.zeros(12), np.zeros(12)
    for b, s in enumerate(samples):
        tri1 = moved[b] if moved is not None else (s["moved"] if (pts and with_pose) else s["tri1"])
        tw = check_forward(oracle, st, b, tri1, s["tri2"], s["lines"], rng, worst, out.get("cleared", False), out["loss"][b])
        assert (tw is None) == bool(s.get("empty")), "an input set's sample is empty (or not) against its label"
        twins.append(tw)
        glb = float(np.float32(gl[b]))
        if tw is None:
            for k in ("g1", "g2", "gR", "gt", "gsrc"):
                if out.get(k) is not None:
                    assert not bool(out[k][b].any()), (k, b)
            continue
        pay_loss += float(tw[0]["loss"])
        if out.get("g1") is not None:
            check_point_grad(f"points1.grad[{b}]", tri1, out["g1"][b].cpu().numpy(), tw, "1", glb, worst, det, s["tri2"])
        if out.get("g2") is not None:
            check_point_grad(f"points2.grad[{b}]", s["tri2"], out["g2"][b].cpu().numpy(), tw, "2", glb, worst, det, tri1)
        if out.get("gR") is not None:
            g12, a12 = check_rigid_grads(f"dR,dt[{b}]", s["tri1"], Rm[b].cpu().numpy(), T[b].cpu().numpy(), tr,
                                         out["gR"][b].cpu().numpy(), out["gt"][b].cpu().numpy(), tw, glb, worst)
            pay_g, pay_a = pay_g + g12, pay_a + a12
        if out.get("gsrc") is not None:  # dL/dsrc = dL/dmoved m^T: a three-term sum per element
            m = Rm[b].cpu().numpy().astype(np.float64)
            m = m.T if tr else m
            back = lambda g, mm=m: (np.asarray(g, np.float64).reshape(-1, 3) @ mm.T).reshape(-1, 9)  # noqa: E731
            f64 = {"g1": back(tw[0]["g1"]), "a1": back(tw[0]["a1"], np.abs(m)), "k1": back(tw[0]["k1"], np.ones((3, 3))) + 3,
                   "blocks": tw[0]["blocks"], "n_buckets": tw[0]["n_buckets"], "med": tw[0]["med"]}
            f32 = {"g1": back(tw[1]["g1"])}
            ex = np.concatenate([s["tri1"][v["f1"][v["tie"]].reshape(-1)].reshape(-1, 3) for v in tw[0]["blocks"].values()]
                                + [np.zeros((0, 3), np.float32)])
            extra = (lambda k: R.det_extra(k, glb, tw[0]["n_buckets"], tw[0]["med"])) if det else None
            w, text = R.check_grad(f"src.grad[{b}]", s["tri1"], out["gsrc"][b].cpu().numpy(), f64, f32, "1", merge_by_point, ex,
                                   extra, scale=glb)
            worst.notes.append(text)
            worst.add("src.grad", w)
    if out.get("payload") is not None:
        pay = out["payload"].cpu().numpy()
        assert pay[1] == sum(t is not None for t in twins)
        # (the sum of the samples' losses, each with its own bound, and the rounding of the sum itself)
        bound = sum(R.scalar_bound(t[0]["loss"], t[1]["loss"]) for t in twins if t is not None) + 2 * U32 * abs(pay_loss)
        assert abs(float(pay[0]) - pay_loss) <= bound
        if bound > 0:
            worst.add("payload loss", abs(float(pay[0]) - pay_loss) / bound)
        # the payload's gradient part: the batch sums of dR, dt, against the twin's with the samples' allowances added up
        # (+ one rounding of the sum per sample)
        perr = np.abs(pay[2:].astype(np.float64) - pay_g)
        pall = pay_a + (B + 1) * U32 * np.abs(pay_g)
        assert not np.any(perr[pall == 0])
        worst.add("payload dR,dt", float(np.divide(perr, pall, out=np.zeros(12), where=pall > 0).max()))
    return st, twins


# ---------------------------------------------------------------------------------------------------- routes at unit scale
GL3 = (1.0, -0.5, 2.0)


def _blk(st, B, tiles):
    return st.blkcnt[:B * tiles].cpu().numpy()


def _live_tiles(st, B):
    """Per sample, the 1024-line tiles that hold a selected line (BLKCNT: one row of ceil(L / 1024) tiles per sample)."""
    tiles = (st.dims[3] + 1023) // 1024
    return (_blk(st, B, tiles).reshape(B, tiles) > 0).sum(1)


def _route(oracle, name, tr=True):
    """(samples, reduce mode, precondition) of a route of the table in DESIGN.md section 6."""
    if name == "one_tile_small":
        return C.route_batch(oracle, 600, tr), None, lambda st: _assert(0 < int(st.info[:, 1].max()) <= 128)
    if name == "one_tile":
        return C.route_batch(oracle, 1000, tr), None, lambda st: _assert(int(st.info[:, 1].max()) > 128)
    if name == "one_tile_dense":
        return C.dense_batch(1000), None, lambda st: _assert(int(_blk(st, 3, 1).max()) > 256)
    if name == "tail":
        return C.route_batch(oracle, 4500, tr), None, lambda st: _assert(_live_tiles(st, 3).min() >= 2)
    if name == "tail_forced":
        return C.route_batch(oracle, 900), "tiled", lambda st: _assert(st.dims[3] <= 1024)  # (one tile: only the knob sends it here)
    if name == "dense_tiles":
        return C.dense_batch(2600), None, lambda st: _assert(int(_blk(st, 3, 3).max()) > 256 and _live_tiles(st, 3).min() >= 2)
    if name == "single_workgroup":
        return C.route_batch(oracle, 4500), "single", None
    if name == "empty_sample":
        return C.empty_sample_batch(oracle), None, lambda st: _assert(int(st.info[1, 1]) == 0 and int(st.info[0, 1]) > 0)
    raise KeyError(name)


def _assert(cond):
    assert cond, "the route's precondition does not hold"


ROUTES = ["one_tile_small", "one_tile", "one_tile_dense", "tail", "tail_forced", "dense_tiles", "single_workgroup", "empty_sample"]
ENTRIES = ["points1", "both", "loss_step", "loss_step_cold", "registration", "registration_src", "registration_step"]


@pytest.mark.parametrize("det", [False, True], ids=["atomics", "deterministic"])
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("route", ROUTES)
def test_routes_at_unit_scale(L, oracle, route, entry, det):
    """Every reduce route x every entry that can take it x float atomics / deterministic, B = 3, dL/dloss = (1, -0.5, 2): the
    scan outputs equal the oracle's, Q, D, median, bucket counts and sums, loss and every gradient stay inside the twin's
    bounds.  The dense constructions carry no pose (their lines are built for the triangles as given); the step's one-call
    entry runs both layouts of R (x R^T + t and x R + t) on the routes with sampled lines."""
    worst = Worst(f"{route} / {entry} / {'deterministic' if det else 'atomics'}")
    both_layouts = entry == "registration_step" and route in ("one_tile_small", "one_tile", "tail")
    for tr in ((True, False) if both_layouts else (True,)):
        samples, reduce_mode, pre = _route(oracle, route, tr)
        run_entry(L, oracle, entry, samples, NARROW, GL3, worst, det=det, reduce_mode=reduce_mode, precondition=pre)
    worst.show()


def _exchange_precondition(st):
    B, L = st.dims[0], st.dims[3]
    _assert(B * ((L + 1023) // 1024) > 256 and _live_tiles(st, B).min() >= 2)  # beyond the tail kernel's 256 (sample, tile) pairs


@pytest.mark.parametrize("det", [False, True], ids=["atomics", "deterministic"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_exchange_reduce_route(L, oracle, entry, det):
    """B x tiles > 256 (B = 40, L = 8000: 320): the exchange reduce and the backward in a launch of its own, through every entry."""
    samples = C.xchg_batch(oracle)
    gl = [(1.0, -0.5, 2.0, 0.25)[b % 4] for b in range(len(samples))]
    worst = Worst(f"exchange / {entry} / {'deterministic' if det else 'atomics'}")
    run_entry(L, oracle, entry, samples, NARROW, gl, worst, det=det, precondition=_exchange_precondition)
    worst.show()


@pytest.mark.parametrize("det", [False, True], ids=["atomics", "deterministic"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_beyond_the_sort_capacity(L, oracle, entry, det):
    """N = 65540, more than 65536 source triangles (indices beyond 16 bits, 17 chunks of the sort), through every entry."""
    worst = Worst(f"large cloud / {entry} / {'deterministic' if det else 'atomics'}")
    run_entry(L, oracle, entry, C.big_cloud(oracle), NARROW, [-0.5], worst, det=det,
              precondition=lambda st: _assert(st.dims[1] > 65536))
    worst.show()


# ---------------------------------------------------------------------------------------------------- scale
@pytest.mark.parametrize("mode", ["cull", "strict"])
@pytest.mark.parametrize("det", [False, True], ids=["atomics", "deterministic"])
@pytest.mark.parametrize("far", [False, True], ids=["origin", "offset"])
@pytest.mark.parametrize("scale", C.SCALES)
def test_scale(L, oracle, scale, far, det, mode):
    """make_pair(77, 1500, 1100) x scale (+ offset), 6000 lines, through LossStep (tail route), registration_loss (the direct
    backward in a launch of its own) and RegistrationStep (the direct backward riding in the tail kernel): at scale the
    scan-output equality is itself a pin of the strict and culled scans against the oracle."""
    s = C.scaled_pair(oracle, scale, far)
    worst = Worst(f"scale {scale:g} {'offset' if far else 'origin'} / {mode} / {'deterministic' if det else 'atomics'}")
    for entry in ("loss_step", "registration", "registration_step"):
        run_entry(L, oracle, entry, [s], NARROW, [-0.5], worst, det=det, mode=mode)
    worst.show()


def test_scale_at_which_nothing_is_selected(L, oracle):
    """Scale 0.01: the 2e-4 epsilon swallows every hit; the oracle and the library agree that nothing is selected."""
    s = dict(C.scaled_pair(oracle, 0.01, False), empty=True)
    worst = Worst("scale 0.01")
    for entry in ("loss_step", "registration", "registration_step", "both"):
        run_entry(L, oracle, entry, [s], NARROW, [1.0], worst)  # (asserts zero counts, loss and gradients)
    worst.show()


# ---------------------------------------------------------------------------------------------------- upstream gradient
GL4 = (2.0 ** -60, -2.0 ** 60, 0.0, 1.0)


@pytest.mark.parametrize("det", [False, True], ids=["atomics", "deterministic"])
@pytest.mark.parametrize("case", ["c_is_1_tail", "scale_5000", "one_tile", "one_tile_dense"])
def test_upstream_gradient(L, oracle, case, det):
    """dL/dloss = (2^-60, -2^60, 0, 1) over one batch of four equal samples, on the tail route and the single-tile route: the
    bounds scale with |gl|, gl = 0 gives an exactly zero gradient, nothing overflows the 64-bit fixed-point scatter and nothing
    is flushed to zero -- with C = 1 (range (2, 1, 3, 2), and the dense construction's single (1, 1) bucket), a large median
    (scale 5000) and a tiny one (the dense construction, ~1e-5): both ends of |gl| / (C sqrt(med))."""
    rng = NARROW
    if case == "c_is_1_tail":
        s, rng = C.scaled_pair(oracle, 1.0, False), (2, 1, 3, 2)
    elif case == "scale_5000":
        s = C.scaled_pair(oracle, 5000.0, False)
    elif case == "one_tile":
        s = C.route_batch(oracle, 1000)[0]
    else:
        s = C.dense_batch(1000)[0]
    worst = Worst(f"upstream gradient / {case} / {'deterministic' if det else 'atomics'}")
    for entry in ("both", "loss_step", "registration_step"):
        _, twins = run_entry(L, oracle, entry, [s] * 4, rng, GL4, worst, det=det)
        if case in ("c_is_1_tail", "one_tile_dense"):
            assert twins[0][0]["n_buckets"] == 1
    worst.show()


# ---------------------------------------------------------------------------------------------------- other call forms
def test_non_default_narrow_range(L, oracle):
    worst = Worst("range (1, 2, 3, 5)")
    for entry in ("both", "loss_step", "registration_step"):
        run_entry(L, oracle, entry, [C.golden_sample("loss_ref_real0.npz")], (1, 2, 3, 5), [-0.5], worst)
    worst.show()


def test_wide_range(L, oracle):
    """(1, 1, 9, 9) through ops.intersection_loss with both gradients (rrl_wide.hip): the wide workspace's HS / W / Q / D
    by slot, median, bucket sums over 64 buckets, loss, both gradients."""
    from rrl_hip import ops
    s, rng, gl = C.golden_sample("loss_ref_human0.npz"), (1, 1, 9, 9), -0.5
    s1, s2, r64, r32 = twin_of(oracle, s["tri1"], s["tri2"], s["lines"], rng)
    assert r64["tie_share"] <= C.TIE_CAP
    p1, p2 = cu(s["tri1"])[None].requires_grad_(True), cu(s["tri2"])[None].requires_grad_(True)
    loss, info, _ = ops.intersection_loss(p1, p2, cu(s["lines"])[None], rng)
    (loss * gl).sum().backward()
    st = ops.last_state()
    assert isinstance(st, ops.WideState) and int(st.status[0]) == 0
    worst = Worst("wide range (1, 1, 9, 9)")
    np.testing.assert_array_equal(st.scan.count1[0].cpu().numpy(), s1["count"])
    np.testing.assert_array_equal(st.scan.count2[0].cpu().numpy(), s2["count"])
    nsel = int(st.nsel[0])
    assert nsel == r64["n_selected"]
    slot_of = np.full(len(s["lines"]), -1)
    slot_of[st.sel[0].cpu().numpy()[:nsel]] = np.arange(nsel)
    kj, D = st.kj[0].cpu().numpy(), st.D[0].cpu().numpy()
    vals = []
    for (k, j), v in sorted(r64["blocks"].items()):
        sl = slot_of[v["lines"]]
        assert (sl >= 0).all() and np.all(kj[sl] == (k | (j << 4)))
        for hs, w, Q, sc, q, Eq, f, n in ((st.hs1, st.w1, st.Q1, s1, v["q1"], v["Eq1"], v["f1"], k),
                                          (st.hs2, st.w2, st.Q2, s2, v["q2"], v["Eq2"], v["f2"], j)):
            np.testing.assert_array_equal(hs[0].cpu().numpy()[sl, :n], f)
            np.testing.assert_array_equal(w[0].cpu().numpy()[sl, :n].view(np.uint32), sc["hit_w"][v["lines"], :n].view(np.uint32))
            worst.add("Q", float((np.abs(Q[0].cpu().numpy()[sl, :n, :3].astype(np.float64) - q) / Eq).max()))
        mine = D[sl, :k, :j]
        worst.add("D", float((np.abs(mine.astype(np.float64) - v["D"]) / v["ED"]).max()))
        vals.append(mine.reshape(-1))
    check_reduce(st, 0, r64, r32, np.concatenate(vals), worst, bsum_stride=8)
    check_point_grad("points1.grad[0]", s["tri1"], p1.grad[0].cpu().numpy(), (r64, r32), "1", gl, worst, False, s["tri2"])
    check_point_grad("points2.grad[0]", s["tri2"], p2.grad[0].cpu().numpy(), (r64, r32), "2", gl, worst, False, s["tri1"])
    worst.show()


def test_pooled_call_of_the_reference_signature(L, oracle):
    """B = 2 through the reference's signature: all lines in one set of buckets, the last sample's median, one loss."""
    g = load_golden("loss_b2_quirk.npz")
    scans = [[oracle.scan(t[b], g["lines"][b], cap=8) for b in range(2)] for t in (g["tri1"], g["tri2"])]
    r64 = R.post_scan_ref(list(g["tri1"]), list(g["tri2"]), scans[0], scans[1], NARROW, pool=True)
    r32 = R.post_scan_ref(list(g["tri1"]), list(g["tri2"]), scans[0], scans[1], NARROW, dtype=np.float32, pool=True)
    assert r64["tie_share"] <= C.TIE_CAP
    p1 = cu(g["tri1"]).requires_grad_(True)
    out = L.cal_loss_intersection_batch_whole_median_pts_lines(1, 1, 5, 5, p1, cu(g["tri2"]), cu(g["lines"]), "cuda")
    (out * -0.5).sum().backward()
    worst = Worst("pooled B = 2")
    worst.add("loss", abs(out.item() - float(r64["loss"])) / R.scalar_bound(r64["loss"], r32["loss"]))
    for b in range(2):
        one64 = dict(r64, g1=r64["g1"][b], a1=r64["a1"][b], k1=r64["k1"][b], blocks=r64["blocks"][b])
        one32 = dict(g1=r32["g1"][b])
        check_point_grad(f"points1.grad[{b}]", g["tri1"][b], p1.grad[b].cpu().numpy(), (one64, one32), "1", -0.5, worst, False, g["tri2"][b])
    worst.show()


@pytest.mark.parametrize("det", [False, True], ids=["atomics", "deterministic"])
def test_ragged_loss_step(L, oracle, det):
    """A ragged LossStep on the BASE set of tests/ragged_cases.py: the twin sees each sample at its own counts; the rows
    beyond a count carry NaN and get a zero gradient."""
    import ragged_cases
    from rrl_hip import ops
    p1, p2, ln, c1, c2, nl, ss = ragged_cases.packed(oracle, "BASE")
    B = len(ss)
    gl = np.array([(1.0, -0.5, 2.0, 0.25)[b % 4] for b in range(B)], np.float32)
    step = ops.LossStep(cu(p1), cu(p2), ln.shape[1], deterministic=det or None, counts1=cu(c1), counts2=cu(c2), nlines=cu(nl))
    for _ in range(2):
        loss, g1, info = step(None, None, cu(ln), grad_loss=cu(gl))
    torch.cuda.synchronize()
    st, g1, loss = step.st, g1.cpu().numpy(), loss.cpu().numpy()
    worst = Worst(f"ragged BASE / {'deterministic' if det else 'atomics'}")
    live = ties = selected = 0
    for b, s in enumerate(ss):
        s1, s2, r64, r32 = twin_of(oracle, s["tri1"], s["tri2"], s["lines"], NARROW)
        check_scan_outputs(st, b, s1, s2, NARROW, bool(getattr(st, "counts_cleared", False)), len(s["lines"]))
        assert not np.any(g1[b, len(s["tri1"]):])
        if r64 is None:
            assert loss[b] == 0.0 and not np.any(g1[b])
            continue
        live += 1
        ties, selected = ties + r64["n_tie"], selected + r64["n_selected"]
        vals = check_points_and_D(st, b, r64, worst)
        check_reduce(st, b, r64, r32, vals, worst, loss[b])
        check_point_grad(f"points1.grad[{b}]", s["tri1"], g1[b, :len(s["tri1"])], (r64, r32), "1", gl[b], worst, det, s["tri2"])
    assert live >= 6 and ties <= C.TIE_CAP * selected  # (the cap on the set: its samples select 230 ... 360 lines each)
    worst.show()
