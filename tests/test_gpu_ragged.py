"""Ragged batches on the GPU (include/rrl.h rrl_opts.count1 / count2 / nlines; DESIGN.md "Ragged batches"): samples with
different numbers of source triangles, target triangles and lines in ONE call.  The bar: sample b of a ragged call gives
what a B = 1 call on its own rows gives -- loss, INFO row, median and hit lists bit for bit --, rows beyond a count are
never read as data (any filler: 0, NaN, +-inf, 1e30) and get a zero gradient, the counts are read on the device.  Inputs:
tests/ragged_cases.py (shown not to be vacuous by tests/test_ragged_host.py)."""
import numpy as np
import pytest
import torch

import ragged_cases as RC
from conftest import load_golden, merge_by_point

pytestmark = pytest.mark.gpu

MODES = [("cull", False), ("cull", True), ("strict", False), ("lazy", False)]  # (scan mode, prepared orders)


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def L():
    import loss
    from rrl_hip import _lib
    _lib.load()
    assert torch.cuda.is_available()
    return loss


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def _orders(ops, t1, t2, c1, c2, prepared):
    return dict(order1=ops.cloud_order(t1, counts=c1), order2=ops.cloud_order(t2, counts=c2)) if prepared else {}


def _hits_sorted(st, which):
    """(count, the <= 4 hit indices ascending) per line; lines with more than 4 hits keep only their count."""
    cnt = (st.count1 if which == 1 else st.count2).clone()
    hit = (st.hit1 if which == 1 else st.hit2).clone()
    k = torch.where(cnt <= 4, cnt, torch.zeros_like(cnt))
    mask = torch.arange(4, device=hit.device)[None, None, :] < k[..., None]
    return cnt, torch.where(mask, hit, torch.full_like(hit, 1 << 30)).sort(-1).values


def _snapshot(step, out):
    """What a step leaves of its evaluation: KJ (k | j << 4 per line), the ascending hit lists of the selected lines, median,
    buckets, info, loss, gradient (a chained step clears COUNT1 / COUNT2 behind the per-line stage's read)."""
    st = step.st
    kj = st.kj.clone()
    sel = kj != 0
    k, j = (kj & 15).long(), (kj >> 4).long()
    a4 = torch.arange(4, device=kj.device)
    hs1 = torch.where(sel[..., None] & (a4 < k[..., None]), st.hs1, torch.full_like(st.hs1, -1))
    hs2 = torch.where(sel[..., None] & (a4 < j[..., None]), st.hs2, torch.full_like(st.hs2, -1))
    return dict(loss=out[0].clone(), grad=out[1].clone(), info=out[2].clone(), kj=kj, hs1=hs1, hs2=hs2, med=st.med.clone(),
                bsum=st.bsum.clone(), bcnt=st.bcnt.clone())


def _close(got, want, what):
    """The bounds of test_loss_step_equals_the_autograd_chain for two float-atomic accumulations of the same terms."""
    g, w = got.detach().cpu().numpy(), want.detach().cpu().numpy()
    top = float(np.abs(w).max()) if w.size else 0.0
    print(f"{what}: max |diff| {float(np.abs(g - w).max()) if w.size else 0.0:.3e}, largest entry {top:.3e}")
    np.testing.assert_allclose(g, w, rtol=2e-5, atol=1e-6 * top)


# ---------------------------------------------------------------------------------- 1: the reference's pairs in one call
@pytest.mark.parametrize("mode,prepared", MODES)
def test_reference_pairs_in_one_call(L, oracle, mode, prepared):
    """The eleven loss_ref_* pairs (N, M in {1024, 2048}, L in {2000, 2500, 3000}: they cannot form a uniform batch), two
    synthetic ones and two edge cases as ONE batch with NaN in every absent row: against the reference's own values."""
    from rrl_hip import ops
    gs = [load_golden(f"loss_{n}.npz") for n in RC.REF_NAMES]
    B = len(gs)
    p1, p2, ln = (np.full((B, c, w), np.nan, np.float32) for c, w in ((2048, 9), (2048, 9), (3000, 6)))
    for b, g in enumerate(gs):
        p1[b, :len(g["tri1"])], p2[b, :len(g["tri2"])], ln[b, :len(g["lines"])] = g["tri1"], g["tri2"], g["lines"]
    c1, c2, nl = (cu(np.array([len(g[k]) for g in gs], np.int32)) for k in ("tri1", "tri2", "lines"))
    t1, t2, tl = cu(p1).requires_grad_(True), cu(p2), cu(ln)
    if not prepared:  # the public spelling (it takes no orders)
        la, valid = L.batched_intersection_loss(t1.detach(), t2, tl, mode=mode, counts1=c1, counts2=c2, nlines=nl)
    loss, info, status = ops.intersection_loss(t1, t2, tl, mode=mode, counts1=c1, counts2=c2, nlines=nl,
                                               **_orders(ops, t1.detach(), t2, c1, c2, prepared))
    st = ops.last_state()
    loss.sum().backward()
    torch.cuda.synchronize()
    assert int(status[0]) == 0 and int(info[:, 3].max()) == 0, "NaN flag"
    if not prepared:
        assert torch.equal(la, loss.detach()) and torch.equal(valid, info[:, 0] > 0)
    grad = t1.grad.cpu().numpy()
    assert np.isfinite(grad).all()
    for b, (name, g) in enumerate(zip(RC.REF_NAMES, gs)):
        n, m, l = len(g["tri1"]), len(g["tri2"]), len(g["lines"])
        assert not grad[b, n:].any(), (name, "gradient rows beyond the count")
        assert int(st.count1[b, l:].abs().sum()) == 0 and int(st.count2[b, l:].abs().sum()) == 0, name
        ref = oracle.loss(g["tri1"], g["tri2"], g["lines"])
        assert [int(v) for v in info[b, :3].tolist()] == [ref["n_buckets"], ref["n_selected"], ref["n_values"]], name
        if name == "edge_allmiss":
            assert ref["loss"] is None and float(loss[b]) == 0.0 and int(info[b, 0]) == 0 and not grad[b].any()
            continue
        np.testing.assert_array_equal(st.count1[b, :l].cpu().numpy(), g["count1"], err_msg=name)
        np.testing.assert_array_equal(st.count2[b, :l].cpu().numpy(), g["count2"], err_msg=name)
        want = float(g["r0_loss"])
        print(name, "loss", float(loss[b]), "reference", want)
        assert abs(float(loss[b]) - want) <= 1e-5 * abs(want), name
        assert bits(st.med[b].item()) == bits(ref["median"]), name
        a, w = merge_by_point(g["tri1"], grad[b, :n]), merge_by_point(g["tri1"], g["r0_grad1"])
        print(name, "gradient", np.abs(a - w).max() / np.abs(w).max())
        assert np.abs(a - w).max() <= 1e-4 * np.abs(w).max() + 1e-9, name


# ---------------------------------------------------------------------------------- 2: ragged = sample by sample
@pytest.mark.parametrize("prepared", [False, True])
@pytest.mark.parametrize("name", ["TAIL", "TILE", "XCHG"])
def test_ragged_equals_sample_by_sample(L, oracle, name, prepared):
    """One step (forward + scatter backward; a step is what reaches the tail kernel and the single-tile kernel) on the
    ragged batch against B = 1 steps on the truncated tensors: loss, INFO, median, buckets and the selected lines' hit
    lists bit for bit, the gradient to the rounding of its float atomics, zero beyond the counts; two samples per shape
    against the oracle itself."""
    from rrl_hip import ops
    p1, p2, ln, c1, c2, nl, ss = RC.packed(oracle, name)
    capL = ln.shape[1]
    # (chain=False: a chained step clears COUNT1 / COUNT2 behind the per-line stage; the FULL hit lists are compared here)
    step = ops.LossStep(cu(p1), cu(p2), capL, prepared=prepared, chain=False, counts1=cu(c1), counts2=cu(c2), nlines=cu(nl))
    got = _snapshot(step, step(None, None, cu(ln)))
    torch.cuda.synchronize()
    got_hits = [_hits_sorted(step.st, w) for w in (1, 2)]
    kind = {"TAIL": (8, 4096, 10000), "TILE": (4, 16384, 512), "XCHG": (32, 1024, 10000)}[name]
    assert (len(ss), p1.shape[1], capL) == kind
    assert int(got["info"][:, 3].max()) == 0 and bool(torch.isfinite(got["grad"]).all()) and bool(torch.isfinite(got["loss"]).all())
    populated = 0
    for b, s in enumerate(ss):
        n, m, l = len(s["tri1"]), len(s["tri2"]), len(s["lines"])
        assert not bool(got["grad"][b, n:].any()) and int(got["kj"][b, l:].abs().sum()) == 0, (name, b)
        for cnt, _ in got_hits:  # no hit on a line the sample does not have
            assert int(cnt[b, l:].abs().sum()) == 0, (name, b)
        if n == 0:
            assert int(got_hits[0][0][b].abs().sum()) == 0, (name, b)
        if m == 0:
            assert int(got_hits[1][0][b].abs().sum()) == 0, (name, b)
        if n == 0 or m == 0 or l == 0:  # no populated bucket: loss 0, INFO 0, zero gradient
            assert float(got["loss"][b]) == 0.0 and got["info"][b, :3].tolist() == [0, 0, 0] and not bool(got["grad"][b].any()), (name, b)
            continue
        one = ops.LossStep(cu(s["tri1"][None]), cu(s["tri2"][None]), l, prepared=prepared, chain=False)
        want = _snapshot(one, one(None, None, cu(s["lines"][None])))
        torch.cuda.synchronize()
        what = (name, b, (n, m, l))
        # the sorted hit lists of EVERY line (selected or not), both clouds: count, and the <= 4 hits ascending
        for w in (1, 2):
            (gc, gh), (wc, wh) = got_hits[w - 1], _hits_sorted(one.st, w)
            assert torch.equal(gc[b, :l], wc[0]) and torch.equal(gh[b, :l], wh[0]), (what, "hit lists of cloud", w)
        assert bits(got["loss"][b].item()) == bits(want["loss"][0].item()), what
        assert torch.equal(got["info"][b], want["info"][0]) and bits(got["med"][b].item()) == bits(want["med"][0].item()), what
        assert torch.equal(got["bsum"][b], want["bsum"][0]) and torch.equal(got["bcnt"][b], want["bcnt"][0]), what
        assert torch.equal(got["kj"][b, :l], want["kj"][0]), what
        assert torch.equal(got["hs1"][b, :l], want["hs1"][0]) and torch.equal(got["hs2"][b, :l], want["hs2"][0]), what
        ga, gb = got["grad"][b, :n], want["grad"][0]
        assert torch.equal(ga.abs().sum(-1) > 0, gb.abs().sum(-1) > 0), what
        _close(ga, gb, f"{name}[{b}] gradient vs the B = 1 step")
        populated += int(want["info"][0, 0]) > 0
        if b in (0, 3):  # ... and against the oracle directly
            ref = oracle.loss(s["tri1"], s["tri2"], s["lines"])
            assert got["info"][b].tolist() == [ref["n_buckets"], ref["n_selected"], ref["n_values"], int(ref["nan"])], what
            assert ref["n_buckets"] > 0 and abs(float(got["loss"][b]) - float(ref["loss"])) <= 1e-5 * abs(float(ref["loss"])), what
            assert bits(got["med"][b].item()) == bits(ref["median"]), what
            a, w = merge_by_point(s["tri1"], ga.cpu().numpy()), merge_by_point(s["tri1"], ref["grad1"])
            assert np.abs(a - w).max() <= 1e-4 * np.abs(w).max() + 1e-9, what
    assert populated >= sum(not RC.may_be_empty(s) for s in ss)


# ---------------------------------------------------------------------------------- 3: absent rows are not read as data
@pytest.mark.parametrize("mode,prepared", MODES)
def test_absent_rows_are_not_read_as_data(L, oracle, mode, prepared):
    from rrl_hip import ops
    runs = []
    for fill in (0.0, float("nan"), float("inf"), float("-inf"), 1e30):
        p1, p2, ln, c1, c2, nl, ss = RC.packed_step(oracle, 0, fill)
        t1, t2 = cu(p1), cu(p2)
        d1, d2, dl = cu(c1), cu(c2), cu(nl)
        loss, info, status = ops.intersection_loss(t1, t2, cu(ln), mode=mode, counts1=d1, counts2=d2, nlines=dl,
                                                   **_orders(ops, t1, t2, d1, d2, prepared))
        st = ops.last_state()
        torch.cuda.synchronize()
        assert int(status[0]) == 0 and int(info[:, 3].max()) == 0, (fill, "NaN flag")
        runs.append((loss.clone(), info.clone(), st.med.clone(), st.bsum.clone(), *_hits_sorted(st, 1), *_hits_sorted(st, 2)))
    for r in runs[1:]:
        for x, y in zip(runs[0], r):
            assert torch.equal(x, y)
    assert int((runs[0][1][:, 0] > 0).sum()) == len(ss)  # every sample is populated
    # ... while a NaN in a PRESENT row still raises the flag of the call, as it does today.  The flag is the reference's NaN: a
    # negative sqrt argument (code/loss.py:88-91), which a non-unit direction produces -- in an absent row it is not seen, in
    # the sample's last present row it is; a literal NaN coordinate in a present row gives the flag of the uniform call on
    # that sample's own rows (whatever that is: the same arithmetic sees the same row)
    def flag(edit, b=3):
        p1, p2, ln, c1, c2, nl, ss = RC.packed_step(oracle, 0, 0.0)
        edit(p1, p2, ln)
        t1, t2 = cu(p1), cu(p2)
        d1, d2 = cu(c1), cu(c2)
        _, _, status = ops.intersection_loss(t1, t2, cu(ln), mode=mode, counts1=d1, counts2=d2, nlines=cu(nl),
                                             **_orders(ops, t1, t2, d1, d2, prepared))
        u1, u2 = cu(p1[b:b + 1, :c1[b]]), cu(p2[b:b + 1, :c2[b]])
        kw = dict(order1=ops.cloud_order(u1), order2=ops.cloud_order(u2)) if prepared else {}
        _, _, alone = ops.intersection_loss(u1, u2, cu(ln[b:b + 1, :nl[b]]), mode=mode, **kw)
        torch.cuda.synchronize()
        return int(status[0]), int(alone[0])

    unit = RC.step_samples(oracle, 0)[3]["lines"][77, :3].copy()
    def absent_bad(p1, p2, ln): ln[3, RC.STEP_NL[3], :3] = 40.0 * unit      # noqa: E306  (the first ABSENT line of sample 3)
    def present_bad(p1, p2, ln): ln[3, RC.STEP_NL[3] - 1, :3] *= 40.0       # noqa: E306  (its last PRESENT line)
    def present_nan(p1, p2, ln): p1[3, 5, 0] = np.nan                       # noqa: E306
    assert flag(absent_bad) == (0, 0)
    assert flag(present_bad) == (1, 1)
    got, alone = flag(present_nan)
    assert got == alone


# ---------------------------------------------------------------------------------- 4: step objects
def _step_inputs(oracle, it):
    """BASE with uneven line counts; step `it` takes the lines of sample (b + it) % B (new lines in every step) and a new pose."""
    from LieAlgebra import se3
    p1, p2, ln, c1, c2, nl, ss = RC.packed_step(oracle, it)
    gen = torch.Generator().manual_seed(40 + it)
    R, t = (x.cuda().contiguous() for x in se3.exp3(0.03 * torch.randn(len(ss), 6, generator=gen)))
    return p1, p2, ln, c1, c2, nl, R, t


def test_loss_step_with_counts_equals_the_ragged_autograd_chain(L, oracle):
    from rrl_hip import ops
    p1, p2, _, c1, c2, nl, _, _ = _step_inputs(oracle, 0)
    src, tar, d1, d2, dl = cu(p1), cu(p2), cu(c1), cu(c2), cu(nl)
    B, N = src.shape[:2]
    step = ops.LossStep(src, tar, 2048, want_payload=True, counts1=d1, counts2=d2, nlines=dl)  # (prepared, kept target, chain=True)
    for it in range(3):
        ln, (R, t) = cu(_step_inputs(oracle, it)[2]), _step_inputs(oracle, it)[6:]
        moved = ops.rigid_apply(src.reshape(B, -1, 3), R, t, transpose_r=True).reshape(B, N, 9).detach().requires_grad_(True)
        loss, info, _ = ops.intersection_loss(moved, tar, ln, counts1=d1, counts2=d2, nlines=dl)
        ref = ops.last_state()
        loss.sum().backward()
        out = step(R, t, ln)
        torch.cuda.synchronize()
        assert step.prepared and not step.fused  # a ragged chained step takes the plain build
        assert torch.equal(out[0], loss.detach()) and torch.equal(out[2], info), it
        assert torch.equal(step.st.med, ref.med) and torch.equal(step.st.bsum, ref.bsum), it
        a, g = moved.grad, out[1]
        assert torch.equal(a.abs().sum(-1) > 0, g.abs().sum(-1) > 0), it
        _close(g, a, f"LossStep call {it}: points1.grad")
        for b in range(B):
            assert not bool(g[b, int(c1[b]):].any())
        valid = info[:, 0] > 0
        _close(step.payload, ops.shard_payload(loss.detach(), state=ref), f"LossStep call {it}: payload")
        assert float(step.payload[1]) == float(valid.sum()) and int(valid.sum()) >= B // 2


def test_registration_step_with_counts_equals_ragged_registration_loss(L, oracle):
    from rrl_hip import ops
    p1, p2, _, c1, c2, nl, _, _ = _step_inputs(oracle, 0)
    src, tar, d1, d2, dl = cu(p1), cu(p2), cu(c1), cu(c2), cu(nl)
    step = ops.RegistrationStep(src, tar, 2048, chain=True, want_payload=True, counts1=d1, counts2=d2, nlines=dl)
    for it in range(3):
        ln, (R, t) = cu(_step_inputs(oracle, it)[2]), _step_inputs(oracle, it)[6:]
        Rg, tg = R.clone().requires_grad_(True), t.clone().requires_grad_(True)
        loss, info, _ = ops.registration_loss(src, Rg, tg, tar, ln, want_payload=True, counts1=d1, counts2=d2, nlines=dl)
        ref = ops.last_state()
        loss.sum().backward()
        want_pay = ref.payload.clone()
        out = step(R, t, ln)
        torch.cuda.synchronize()
        assert torch.equal(out[0], loss.detach()) and torch.equal(out[4], info), it
        assert torch.equal(step.st.med, ref.med) and torch.equal(step.st.bsum, ref.bsum), it
        assert bool(torch.isfinite(out[1]).all()) and bool(torch.isfinite(out[2]).all())
        _close(out[1], Rg.grad, f"RegistrationStep call {it}: dR")
        _close(out[2], tg.grad, f"RegistrationStep call {it}: dt")
        _close(out[3], want_pay, f"RegistrationStep call {it}: payload (sum of valid losses, #valid, sum dR, sum dt)")
    # dL/dsrc of the fused op: rows beyond counts1 are exactly zero although the absent source rows hold NaN
    sg = src.clone().requires_grad_(True)
    loss, _, _ = ops.registration_loss(sg, R, t, tar, ln, counts1=d1, counts2=d2, nlines=dl)
    loss.sum().backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(sg.grad).all()) and float(sg.grad.abs().sum()) > 0
    for b in range(len(c1)):
        assert not bool(sg.grad[b, int(c1[b]):].any())


# ---------------------------------------------------------------------------------- 5: deterministic mode
def test_deterministic_mode_with_counts(L, oracle):
    from rrl_hip import ops
    p1, p2, ln, c1, c2, nl, R, t = _step_inputs(oracle, 1)
    src, tar, tl, d1, d2, dl = cu(p1), cu(p2), cu(ln), cu(c1), cu(c2), cu(nl)
    plain = ops.LossStep(src, tar, 2048, counts1=d1, counts2=d2, nlines=dl)
    l0, g0, i0 = (x.clone() for x in plain(R, t, tl))
    det = ops.LossStep(src, tar, 2048, deterministic=True, counts1=d1, counts2=d2, nlines=dl)
    l1, g1, i1 = (x.clone() for x in det(R, t, tl))
    l2, g2, i2 = (x.clone() for x in det(R, t, tl))
    torch.cuda.synchronize()
    assert torch.equal(l1, l0) and torch.equal(i1, i0) and torch.equal(l2, l1)
    assert torch.equal(g1, g2), "two deterministic calls: bit-identical gradients"
    print("deterministic vs float atomics:", float((g1 - g0).abs().max()), "of", float(g0.abs().max()))
    assert float((g1 - g0).abs().max()) <= 1e-6 * float(g0.abs().max())
    for b in range(len(c1)):
        assert not bool(g1[b, int(c1[b]):].any())


# ---------------------------------------------------------------------------------- 6: counts live on the device
@pytest.mark.parametrize("prepared", [False, True])
def test_captured_step_follows_counts_written_in_place(L, oracle, prepared):
    """A captured LossStep replayed after counts1 and nlines were overwritten IN PLACE evaluates the new counts (equal to
    a fresh eager step), which a host-side read at capture time could not do.  counts2 stays: the target is kept.  (A
    prepared step's source order belongs to its counts: it is rewritten in place as well.)"""
    from rrl_hip import ops
    from rrl_hip.graph import GraphedStep
    p1, p2, ln, c1, c2, nl, R, t = _step_inputs(oracle, 0)
    src, tar, tl, d2 = cu(p1), cu(p2), cu(ln), cu(c2)
    d1, dl = cu(c1), cu(nl)
    st = ops.LossStep(src, tar, 2048, prepared=prepared, counts1=d1, counts2=d2, nlines=dl)
    st(R, t, tl)
    g = GraphedStep(lambda: st(R, t, tl))
    for cc1, ccl in RC.GRAPH_VARIANTS:
        cc1, ccl = np.array(cc1, np.int32), np.array(ccl, np.int32)
        d1.copy_(cu(cc1))
        dl.copy_(cu(ccl))
        if prepared:
            st.order1.copy_(ops.cloud_order(src, counts=d1))
        out = g()
        torch.cuda.synchronize()
        got = _snapshot(st, out)
        fresh = ops.LossStep(src, tar, 2048, prepared=prepared, counts1=cu(cc1), counts2=d2, nlines=cu(ccl))
        want = _snapshot(fresh, fresh(R, t, tl))
        torch.cuda.synchronize()
        for key in ("loss", "info", "kj", "hs1", "hs2", "med", "bsum", "bcnt"):
            assert torch.equal(got[key], want[key]), key
        assert torch.equal(got["grad"].abs().sum(-1) > 0, want["grad"].abs().sum(-1) > 0)
        _close(got["grad"], want["grad"], "replayed step: points1.grad")
        for b in range(len(cc1)):
            assert not bool(got["grad"][b, int(cc1[b]):].any()) and int(got["kj"][b, int(ccl[b]):].abs().sum()) == 0
    assert int((want["info"][:, 0] > 0).sum()) >= 4


def test_a_ragged_state_refuses_whole_capacity_consumers(L, oracle):
    """The workspace of a ragged evaluation holds each sample's own rows only: the Chamfer monitor from that state and a
    carried-over target scan are refused (ValueError naming the alternative), whichever entry left the state."""
    from rrl_hip import ops
    p1, p2, ln, c1, c2, nl, R, t = _step_inputs(oracle, 0)
    src, tar, tl, d1, d2, dl = cu(p1), cu(p2), cu(ln), cu(c1), cu(c2), cu(nl)
    kw = dict(counts1=d1, counts2=d2, nlines=dl)
    step = ops.LossStep(src, tar, 2048, **kw)
    for make in (lambda: ops.intersection_loss(src, tar, tl, **kw), lambda: ops.registration_loss(src, R, t, tar, tl, **kw),
                 lambda: step(R, t, tl)):
        make()
        st = ops.last_state()
        assert st.ragged
        for fn in (ops.chamfer_from_state, lambda: ops.chamfer_group_means(groups=1)):
            with pytest.raises(ValueError, match=r"ops\.chamfer"):
                fn()
        with pytest.raises(ValueError, match="scan its target"):
            ops.intersection_loss(src, tar, tl, target_from=st)
    ops.intersection_loss(src[7:8], tar[7:8], tl[7:8, :700].contiguous())  # a uniform evaluation (sample 7 is full): served as before
    assert not ops.last_state().ragged and float(ops.chamfer_from_state()) > 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------- 7: counted order and box
def test_cloud_order_and_aabb_with_counts(L, oracle):
    from rrl_hip import ops
    for name in ("BASE", "TILE"):  # (TILE: 16384 rows -- the levels above one LDS window)
        p1, p2, _, c1, c2, _, ss = RC.packed(oracle, name)
        for p, c in ((p1, c1), (p2, c2)):
            t = cu(p)
            order = ops.cloud_order(t, counts=cu(c)).cpu().numpy()
            assert order.shape == (len(c), (p.shape[1] + 63) // 64 * 64) and order.dtype == np.int32
            for b, n in enumerate(c):
                np.testing.assert_array_equal(np.sort(order[b, :n]), np.arange(n))
            assert torch.equal(ops.cloud_order(t, counts=[int(v) for v in c]), torch.from_numpy(order).cuda())  # (host counts: uploaded)
            pts = np.ascontiguousarray(p[:, :, :3])
            box = ops.aabb(cu(pts), counts=cu(c)).cpu().numpy()
            for b, n in enumerate(c):
                if n:
                    np.testing.assert_array_equal(box[b], np.concatenate([pts[b, :n].min(0), pts[b, :n].max(0)]))
                else:
                    assert np.all(box[b, :3] == np.inf) and np.all(box[b, 3:] == -np.inf)
    # without counts: the entries' own results (a full count gives the same order, too)
    t = cu(RC.packed(oracle, "BASE", 0.0)[0])
    full = torch.full((t.shape[0],), t.shape[1], dtype=torch.int32, device="cuda")
    assert torch.equal(ops.cloud_order(t), ops.cloud_order(t, counts=full))
    assert torch.equal(ops.aabb(t[:, :, :3].contiguous()), ops.aabb(t[:, :, :3].contiguous(), counts=full))
    with pytest.raises(ValueError):
        ops.cloud_order(t, counts=[t.shape[1] + 1] * t.shape[0])


def test_full_counts_give_the_uniform_call_bit_for_bit(L, oracle):
    """Counts equal to the capacities select the same kernels' uniform path: every output equals the call without counts."""
    from rrl_hip import ops
    _, _, _, ss = RC.batch(oracle, "BASE")
    s = ss[7]  # 2048 x 2048 triangles, 2048 lines
    t1, t2, tl = (cu(np.stack([s[k]] * 3)) for k in ("tri1", "tri2", "lines"))
    full = lambda n: torch.full((3,), n, dtype=torch.int32, device="cuda")  # noqa: E731
    for mode in ("cull", "strict"):
        a = ops.intersection_loss(t1, t2, tl, mode=mode)
        sa = ops.last_state()
        b = ops.intersection_loss(t1, t2, tl, mode=mode, counts1=full(2048), counts2=full(2048), nlines=full(2048))
        sb = ops.last_state()
        torch.cuda.synchronize()
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(sa.med, sb.med) and torch.equal(sa.bsum, sb.bsum)
        for w in (1, 2):
            for x, y in zip(_hits_sorted(sa, w), _hits_sorted(sb, w)):
                assert torch.equal(x, y)


def test_a_new_counts2_is_a_new_target(L, oracle):
    """The kept target's records belong to its row counts: a new counts2 tensor (set_counts) and an in-place torch write to
    the current one both make the next call rebuild the target; the results equal a fresh step's."""
    from rrl_hip import ops
    p1, p2, ln, c1, c2, nl, R, t = _step_inputs(oracle, 0)
    src, tar, tl, d1, dl = cu(p1), cu(p2), cu(ln), cu(c1), cu(nl)
    half = np.array(RC.HALF_C2, np.int32)
    assert np.array_equal(half, np.maximum(c2 // 2, 1))
    step = ops.LossStep(src, tar, 2048, counts1=d1, counts2=cu(c2), nlines=dl)
    for _ in range(2):
        step(R, t, tl)  # (the second call keeps the target)
    for how, cc2 in (("set_counts", half), ("in place", c2)):
        if how == "set_counts":
            step.set_counts(counts2=cu(cc2))
        else:
            step.counts2.copy_(cu(cc2))
            step.order2.copy_(ops.cloud_order(tar, counts=step.counts2))
        got = _snapshot(step, step(R, t, tl))
        fresh = ops.LossStep(src, tar, 2048, counts1=d1, counts2=cu(cc2), nlines=dl)
        want = _snapshot(fresh, fresh(R, t, tl))
        torch.cuda.synchronize()
        for key in ("loss", "info", "kj", "hs1", "hs2", "med", "bsum", "bcnt"):
            assert torch.equal(got[key], want[key]), (how, key)
        _close(got["grad"], want["grad"], f"{how}: points1.grad")
        assert int((want["info"][:, 0] > 0).sum()) == len(c1)
