"""GPU: bucket ranges up to 8 hits per line and cloud (the wide pipeline, include/rrl.h rrl_loss_forward_wide) through
the drop-in call, ops.intersection_loss and loss.batched_intersection_loss, against the reference's values
(tests/golden/loss_wide.npz) and the CPU oracle."""
import numpy as np
import pytest
import torch

from conftest import load_golden, merge_by_point

pytestmark = pytest.mark.gpu

W = load_golden("loss_wide.npz")
FIXTURES = [str(x) for x in W["fixtures"]]
RANGES = [tuple(int(v) for v in r) for r in W["ranges"]]


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def pair(name):
    g = load_golden(f"loss_{name}.npz")
    return g["tri1"], g["tri2"], g["lines"]


def close_by_point(tri, mine, want, tol):
    a, b = merge_by_point(tri, mine), merge_by_point(tri, want)
    return np.abs(a - b).max() <= tol * np.abs(b).max() + 1e-9, np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def f32bits(x):
    return np.float32(x).view(np.uint32)


@pytest.mark.parametrize("ri", range(len(RANGES)))
@pytest.mark.parametrize("name", FIXTURES)
def test_reference_parity(oracle, name, ri):
    """All 14 pairs x the 4 wide ranges through the drop-in: loss vs the reference, bucket / line / value counts and the
    median bit for bit vs the oracle, points1.grad per point vs the reference."""
    import loss as L
    from rrl_hip import ops
    rng = RANGES[ri]
    tri1, tri2, lines = pair(name)
    p1 = cu(tri1)[None].requires_grad_(True)
    out = L.cal_loss_intersection_batch_whole_median_pts_lines(*rng, p1, cu(tri2)[None], cu(lines)[None], "cuda", max_hits=8)
    ref = oracle.loss(tri1, tri2, lines, rng, want_grad=False)
    if bool(W[f"{name}_r{ri}_empty"]):
        assert out is None and ref["loss"] is None
        return
    want = float(W[f"{name}_r{ri}_loss"])
    assert out is not None and out.shape == (1,) and out.device.type == "cuda"
    assert abs(out.item() - want) <= 1e-5 * abs(want), (out.item(), want)
    assert list(ops._DropinLoss.flags[:3]) == [ref["n_buckets"], ref["n_selected"], ref["n_values"]]
    st = ops.last_state()
    assert isinstance(st, ops.WideState) and int(st.status[0]) == 0
    assert f32bits(st.med[0].item()) == f32bits(ref["median"])
    out.backward()
    ok, err = close_by_point(tri1, p1.grad[0].cpu().numpy(), W[f"{name}_r{ri}_grad1"], 1e-4)
    assert ok, err


def test_both_gradients(oracle):
    """ops.intersection_loss with both clouds requiring grad: points1.grad and points2.grad vs the oracle (and the
    reference's own pair of gradients)."""
    from rrl_hip import ops
    name, rng = str(W["grad2_pair"]), tuple(int(v) for v in W["grad2_range"])
    tri1, tri2, lines = pair(name)
    p1, p2 = cu(tri1)[None].requires_grad_(True), cu(tri2)[None].requires_grad_(True)
    loss, info, _ = ops.intersection_loss(p1, p2, cu(lines)[None], rng)
    loss.sum().backward()
    ref = oracle.loss(tri1, tri2, lines, rng, want_grad2=True)
    assert abs(loss.item() - float(ref["loss"])) <= 1e-5 * abs(float(ref["loss"]))
    for tri, mine, want in ((tri1, p1.grad[0], ref["grad1"]), (tri2, p2.grad[0], ref["grad2"]),
                            (tri1, p1.grad[0], W["grad2_grad1"]), (tri2, p2.grad[0], W["grad2_grad2"])):
        ok, err = close_by_point(tri, mine.cpu().numpy(), want, 1e-4)
        assert ok, err


def _c2_batch(B=8, N=4096, M=4096, Ll=10000, seed=700):
    import loss as L
    from rrl_hip import synth
    prs = [synth.make_pair(seed + b, N, M) for b in range(B)]
    ln = []
    for b, p in enumerate(prs):
        torch.manual_seed(seed + b)
        ln.append(L.Random_uniform_distribution_lines_batch_efficient_resample(
            torch.tensor([[float(p["radius"])]]), torch.from_numpy(p["center"]).reshape(1, 3), Ll,
            cu(p["src"])[None], cu(p["tar"])[None], "cuda")[0])
    return (np.stack([p["src_tri"] for p in prs]), np.stack([p["tar_tri"] for p in prs]),
            torch.stack(ln).cpu().numpy())


@pytest.fixture(scope="module")
def c2():
    return _c2_batch()


def test_c2_shape_batched(oracle, c2):
    """B = 8, N = M = 4096, L = 10000 at (1, 1, 9, 9) through loss.batched_intersection_loss, against the oracle per sample."""
    import loss as L
    from rrl_hip import ops
    tri1, tri2, lines = c2
    p1 = cu(tri1).requires_grad_(True)
    lv, valid = L.batched_intersection_loss(p1, cu(tri2), cu(lines), (1, 1, 9, 9))
    st = ops.last_state()
    assert int(st.status[0]) == 0 and int(st.status[1]) > 0  # lines with more than 4 hits were recovered, all consistent
    lv.sum().backward()
    info = st.info.cpu().numpy()
    for b in range(tri1.shape[0]):
        ref = oracle.loss(tri1[b], tri2[b], lines[b], (1, 1, 9, 9))
        assert bool(valid[b]) and abs(lv[b].item() - float(ref["loss"])) <= 1e-5 * abs(float(ref["loss"])), b
        assert list(info[b, :3]) == [ref["n_buckets"], ref["n_selected"], ref["n_values"]], b
        assert f32bits(st.med[b].item()) == f32bits(ref["median"]), b
        ok, err = close_by_point(tri1[b], p1.grad[b].cpu().numpy(), ref["grad1"], 1e-4)
        assert ok, (b, err)


def test_scan_mode_invariance(c2):
    """cull / strict / auto, with and without prepared orders: the same loss bits, and the hit recovery agrees with the
    scan every time (status word 0)."""
    from rrl_hip import ops
    tri1, tri2, lines = (cu(a[:2]) for a in c2)
    o1, o2 = ops.cloud_order(tri1), ops.cloud_order(tri2)
    got = []
    for mode in ("cull", "strict", "auto"):
        for orders in (False, True):
            kw = dict(order1=o1, order2=o2) if orders else {}
            lv = ops.intersection_loss(tri1, tri2, lines, (1, 1, 9, 9), mode=mode, **kw)[0]
            assert int(ops.last_state().status[0]) == 0, (mode, orders)
            got.append((mode, orders, lv.clone()))
    for mode, orders, lv in got[1:]:
        assert torch.equal(lv, got[0][2]), (mode, orders)


def test_narrow_range_through_the_wide_kernels(c2):
    """(1, 1, 5, 5) through the wide pipeline (test hook) against the narrow path on the same inputs: loss bits equal
    (both sum the buckets in 2^-40 fixed point and take the same median), gradients to the rounding of the atomics."""
    from rrl_hip import ops
    tri1, tri2, lines = (cu(a) for a in c2)
    grads = []
    losses = []
    for wide in (False, True):
        p1, p2 = tri1.clone().requires_grad_(True), tri2.clone().requires_grad_(True)
        lv, info, _ = ops.intersection_loss(p1, p2, lines, (1, 1, 5, 5), _force_wide=wide)
        assert isinstance(ops.last_state(), ops.WideState) == wide
        lv.sum().backward()
        losses.append((lv.detach().clone(), info.clone()))
        grads.append((p1.grad.clone(), p2.grad.clone()))
    assert torch.equal(losses[0][0], losses[1][0]) and torch.equal(losses[0][1], losses[1][1])
    for a, b in zip(grads[0], grads[1]):
        assert (a - b).abs().max().item() <= 1e-6 * a.abs().max().item() + 1e-12


def test_lines_with_nine_or_more_hits_are_excluded(oracle):
    """Every triangle of cloud 1 twice: every hit count doubles, so lines with 5 .. 8 hits before now have 10 .. 16 and
    fall out of (1, 1, 9, 9); the selection, the values and the loss follow the oracle."""
    from rrl_hip import ops
    tri1, tri2, lines = pair("ref_human0")
    dup = np.concatenate([tri1, tri1])
    sc = oracle.scan(dup, lines, cap=8)
    assert (sc["count"] >= 9).sum() > 0
    lv, info, _ = ops.intersection_loss(cu(dup)[None], cu(tri2)[None], cu(lines)[None], (1, 1, 9, 9))
    ref = oracle.loss(dup, tri2, lines, (1, 1, 9, 9), want_grad=False)
    assert list(info[0, :3].cpu().numpy()) == [ref["n_buckets"], ref["n_selected"], ref["n_values"]]
    assert abs(lv.item() - float(ref["loss"])) <= 1e-5 * abs(float(ref["loss"]))


def test_range_of_wide_lines_only(oracle):
    """(5, 5, 9, 9): every selected line has more than 4 hits in both clouds -- all of them go through the hit recovery."""
    from rrl_hip import ops
    tri1, tri2, lines = pair("ref_real0")
    lv, info, _ = ops.intersection_loss(cu(tri1)[None], cu(tri2)[None], cu(lines)[None], (5, 5, 9, 9))
    st = ops.last_state()
    ref = oracle.loss(tri1, tri2, lines, (5, 5, 9, 9), want_grad=False)
    assert ref["n_selected"] > 0 and int(st.status[1]) == 2 * ref["n_selected"] and int(st.status[0]) == 0
    assert abs(lv.item() - float(ref["loss"])) <= 1e-5 * abs(float(ref["loss"]))


def test_all_lines_missing_and_non_unit_direction():
    import loss as L
    tri1, tri2, lines = pair("ref_human0")
    far = lines.copy()
    far[:, 3:] = 1000.0  # every line far away from both clouds: no bucket
    p1 = cu(tri1)[None]
    assert L.cal_loss_intersection_batch_whole_median_pts_lines(1, 1, 9, 9, p1, cu(tri2)[None], cu(far)[None], "cuda",
                                                              max_hits=8) is None
    lv, valid = L.batched_intersection_loss(p1, cu(tri2)[None], cu(far)[None], (1, 1, 9, 9))
    assert not bool(valid[0]) and lv.item() == 0.0
    bad = lines.copy()
    bad[:, :3] *= 3.0
    with pytest.raises(ValueError, match="NaN"):
        L.cal_loss_intersection_batch_whole_median_pts_lines(1, 1, 9, 9, p1, cu(tri2)[None], cu(bad)[None], "cuda", max_hits=8)


def _quirk_restatement(oracle, tri1s, tri2s, liness, rng):
    """The reference's B > 1 behaviour: the lines of all samples pooled per (k, j) bucket, the Welsch term
    normalised by the LAST sample's median -- restated here from the oracle's scan (cap = 8) in fp32 / fp64."""
    s_m, s_n, e_m, e_n = rng
    per = []
    for tri1, tri2, lines in zip(tri1s, tri2s, liness):
        a, b = oracle.scan(tri1, lines, cap=8), oracle.scan(tri2, lines, cap=8)

        def q(tri, sc, l, c):
            out = []
            for h in range(c):
                f, w = sc["hit_idx"][l, h], sc["hit_w"][l, h]
                p = tri[f].reshape(3, 3)
                s = w[0] * p[0]
                s = s + w[1] * p[1]
                s = s + w[2] * p[2]
                out.append((s / np.float32(3)).astype(np.float32))
            return np.array(out, np.float32)
        rows = []
        for l in range(lines.shape[0]):
            k, j = int(a["count"][l]), int(b["count"][l])
            if s_m <= k < e_m and s_n <= j < e_n:
                q1, q2 = q(tri1, a, l, k), q(tri2, b, l, j)
                d = q1[:, None, :] - q2[None, :, :]
                D = d[..., 0] * d[..., 0]
                D = D + d[..., 1] * d[..., 1]
                D = D + d[..., 2] * d[..., 2]
                rows.append((k, j, D.astype(np.float32)))
        per.append(rows)
    vals = np.sort(np.concatenate([D.reshape(-1) for _, _, D in per[-1]]))
    med = vals[(len(vals) - 1) // 2]
    loss, C = 0.0, 0
    for k in range(s_m, e_m):
        for j in range(s_n, e_n):
            Ds = [D for rows in per for (kk, jj, D) in rows if kk == k and jj == j]
            if not Ds:
                continue
            C += 1
            Wl = [1 - np.exp(-(D.astype(np.float64) / med) / 2) for D in Ds]
            mrow = np.mean([w.min(1).sum() / k for w in Wl])
            mcol = np.mean([w.min(0).sum() / j for w in Wl])
            loss += np.exp(-0.5 * abs(k - j)) * (mrow + mcol)
    return loss / C


def test_pool_semantics(oracle):
    """B = 2 through the drop-in: one sample twice gives the B = 1 value; two distinct samples match the restatement of
    the reference's pooling quirk."""
    import loss as L
    rng = (1, 1, 9, 9)
    tri1, tri2, lines = pair("synth_s0")
    one = L.cal_loss_intersection_batch_whole_median_pts_lines(*rng, cu(tri1)[None], cu(tri2)[None], cu(lines)[None], "cuda",
                                                               max_hits=8)
    two = L.cal_loss_intersection_batch_whole_median_pts_lines(*rng, cu(np.stack([tri1, tri1])), cu(np.stack([tri2, tri2])),
                                                               cu(np.stack([lines, lines])), "cuda", max_hits=8)
    assert abs(two.item() - one.item()) <= 1e-6 * abs(one.item())
    b1, b2, bl = pair("synth_s1")
    n = min(tri1.shape[0], b1.shape[0]), min(tri2.shape[0], b2.shape[0]), min(lines.shape[0], bl.shape[0])
    t1s, t2s, ls = np.stack([tri1[:n[0]], b1[:n[0]]]), np.stack([tri2[:n[1]], b2[:n[1]]]), np.stack([lines[:n[2]], bl[:n[2]]])
    p1 = cu(t1s).requires_grad_(True)
    out = L.cal_loss_intersection_batch_whole_median_pts_lines(*rng, p1, cu(t2s), cu(ls), "cuda", max_hits=8)
    want = _quirk_restatement(oracle, t1s, t2s, ls, rng)
    assert abs(out.item() - want) <= 1e-5 * abs(want), (out.item(), want)
    out.backward()
    assert torch.isfinite(p1.grad).all() and p1.grad.abs().sum() > 0


def test_trainer_loop_form_equals_the_batched_call(c2):
    """The reference trainers' loop (B = 1 slices + backward, rpm/Train_RPM.py:226-231) at (1, 1, 9, 9): the same
    points1.grad as one batched call."""
    import loss as L
    from rrl_hip import ops
    tri1, tri2, lines = (cu(a[:4]) for a in c2)
    p1 = tri1.clone().requires_grad_(True)
    total = 0
    for j in range(p1.shape[0]):
        one = L.cal_loss_intersection_batch_whole_median_pts_lines(1, 1, 9, 9, p1[j:j + 1], tri2[j:j + 1], lines[j:j + 1], "cuda",
                                                                   max_hits=8)
        if one is not None:
            total = total + one
    total.backward()
    q1 = tri1.clone().requires_grad_(True)
    lv, valid = L.batched_intersection_loss(q1, tri2, lines, (1, 1, 9, 9))
    lv.sum().backward()
    assert abs(total.item() - lv.sum().item()) <= 1e-6 * abs(lv.sum().item())
    assert (p1.grad - q1.grad).abs().max().item() <= 1e-6 * q1.grad.abs().max().item() + 1e-12
    assert isinstance(ops.last_state(), ops.WideState)


def test_dropin_range_limits():
    """The reference-signature call keeps its default: a range beyond 1..4 raises unless max_hits=8 asks for the wide
    pipeline; with max_hits=8 a range beyond 8 hits per line (or a bad max_hits) still raises, and (1, 1, 6, 5) on lines
    that miss both clouds is a valid call without a populated bucket."""
    import loss as L
    g = load_golden("loss_edge_allmiss.npz")
    args = (cu(g["tri1"])[None], cu(g["tri2"])[None], cu(g["lines"])[None], "cuda")
    with pytest.raises(ValueError, match="max_hits=8"):
        L.cal_loss_intersection_batch_whole_median_pts_lines(1, 1, 6, 5, *args)
    for rng in ((1, 1, 10, 5), (0, 1, 6, 5), (1, 1, 6, 10)):
        with pytest.raises(ValueError):
            L.cal_loss_intersection_batch_whole_median_pts_lines(*rng, *args, max_hits=8)
    with pytest.raises(ValueError, match="max_hits"):
        L.cal_loss_intersection_batch_whole_median_pts_lines(1, 1, 5, 5, *args, max_hits=6)
    assert L.cal_loss_intersection_batch_whole_median_pts_lines(1, 1, 6, 5, *args, max_hits=8) is None
    assert L.cal_loss_intersection_batch_whole_median_pts_lines(1, 1, 5, 5, *args, max_hits=8) is None  # (narrow path)


def test_out_of_scope_entries_refuse_wide_ranges():
    from rrl_hip import dist, ops
    tri1, tri2, lines = pair("synth_s0")
    src, tar, ln = cu(tri1)[None], cu(tri2)[None], cu(lines)[None]
    R, t = torch.eye(3, device="cuda")[None].contiguous(), torch.zeros(1, 3, device="cuda")
    rng = (1, 1, 9, 9)
    ops.intersection_loss(src, tar, ln)  # a narrow evaluation whose target scan a later call could carry over
    narrow = ops.last_state()
    cases = [
        lambda: ops.registration_loss(src, R, t, tar, ln, rng),
        lambda: ops.registration_loss(src, torch.cat([R, R]), torch.cat([t, t]), tar, ln, rng),  # multi-pose problems
        lambda: ops.RegistrationStep(src, tar, ln.shape[1], rng=rng),
        lambda: ops.LossStep(src, tar, ln.shape[1], rng=rng),
        lambda: ops.registration_step_raw(src, R, t, tar, ln, rng),
        lambda: ops.intersection_loss(src, tar, ln, rng, target_from=narrow),
        lambda: ops.loss_forward_raw(src, tar, ln, rng),
        lambda: dist.sharded_batch_loss(src, tar, ln, rng),
        lambda: dist.line_sharded_loss(src, tar, ln, rng),
    ]
    for case in cases:
        with pytest.raises(ValueError, match=r"ops\.intersection_loss"):
            case()
    ops.set_deterministic(True)
    try:
        with pytest.raises(ValueError, match=r"ops\.intersection_loss"):
            ops.intersection_loss(src, tar, ln, rng)
    finally:
        ops.set_deterministic(False)
