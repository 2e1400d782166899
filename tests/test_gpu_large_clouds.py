"""Clouds beyond 65536 triangles on the sorted, culled layout (include/rrl.h rrl_sort_capacity: 2^20).

Up to the sort capacity every feature of the sorted layout -- the culled scan, prepared orders, multi-pose steps, the
Chamfer tree and its rider -- serves a cloud of any size; beyond it the dense legacy path does.  The bar is the one of the
smaller clouds: labels, hit lists, median, bucket sums, loss and the NaN flag of the culled scan BIT-IDENTICAL to the strict
scan, which is the reference at these sizes (the oracle serves only where it is cheap).

At unit scale a dense cloud has pseudo-triangles whose threshold is below sqrt(2e-4), so no line could hit one: every
pair here is scaled up with the density, and every case checks that enough lines were selected.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CAP = 1 << 20


@pytest.fixture(scope="module")
def L():
    import loss
    from rrl_hip import _lib
    _lib.load()
    assert torch.cuda.is_available()
    return loss


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _pairs(seed, B, n, m):
    """B synthetic pairs scaled so that the denser cloud's median threshold is ~0.06 (well above sqrt(2e-4))."""
    from rrl_hip import synth
    s = np.float32(10.0 * math.sqrt(max(n, m) / 65536.0))
    prs = []
    for b in range(B):
        p = synth.make_pair(seed + b, n, m)
        prs.append({k: (v * s if isinstance(v, np.ndarray) or k == "radius" else v) for k, v in p.items()})
    return prs, cu(np.stack([p["src_tri"] for p in prs])), cu(np.stack([p["tar_tri"] for p in prs]))


def _lines(L, prs, nl):
    out = []
    for b, p in enumerate(prs):
        torch.manual_seed(200 + b)
        out.append(L.Random_uniform_distribution_lines_batch_efficient_resample(
            torch.tensor([[float(p["radius"])]]), torch.from_numpy(p["center"]).reshape(1, 3), nl, cu(p["src"])[None],
            cu(p["tar"])[None], "cuda")[0])
    return torch.stack(out).contiguous()


def _hits_sorted(st, which):
    cnt = (st.count1 if which == 1 else st.count2).clone()
    hit = (st.hit1 if which == 1 else st.hit2).clone()
    k = torch.where(cnt <= 4, cnt, torch.zeros_like(cnt))  # beyond 4 hits only the first four arrivals are kept
    mask = torch.arange(4, device=hit.device)[None, None, :] < k[..., None]
    hit = torch.where(mask, hit, torch.full_like(hit, 1 << 30))
    return cnt, hit.sort(-1).values


def _selected_hits(st, which):
    """HS1 / HS2 of the selected lines: their k (j) ascending hit indices, -1 elsewhere (unselected lines, unused slots)."""
    kj = st.kj.long()
    k = (kj & 15) if which == 1 else (kj >> 4)
    hs = st.hs1 if which == 1 else st.hs2
    mask = torch.arange(4, device=hs.device)[None, None, :] < k[..., None]
    return torch.where(mask, hs, torch.full_like(hs, -1))


def _bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def _same_evaluation(a, b):
    for w in (1, 2):
        ca, ha = _hits_sorted(a, w)
        cb, hb = _hits_sorted(b, w)
        assert torch.equal(ca, cb) and torch.equal(ha, hb)
        assert torch.equal(_selected_hits(a, w), _selected_hits(b, w))
    assert torch.equal(a.kj, b.kj)
    for x, y in ((a.loss, b.loss), (a.med, b.med), (a.info, b.info), (a.bsum, b.bsum), (a.bcnt, b.bcnt), (a.status[:1], b.status[:1])):
        assert torch.equal(_bits(x), _bits(y))  # (bit patterns: a NaN loss equals itself)


def _selected(st):
    return [int(v) for v in st.info[:, 1].cpu()]


def test_library_capacity():
    from rrl_hip import ops
    assert ops.sort_capacity() == CAP


@pytest.mark.parametrize("B,n,m,nl,bad", [
    (1, 65537, 4096, 3000, False),
    (2, 131072, 131072, 2000, False),
    (2, 307200, 70000, 2000, False),
    (2, CAP, 5000, 2000, False),
    (2, 131072, 70000, 2000, True),    # non-unit directions and a NaN triangle: the strict fallback and the NaN flag
])
def test_culled_equals_strict(L, B, n, m, nl, bad):
    from rrl_hip import ops
    prs, t1, t2 = _pairs(700 + n % 97, B, n, m)
    ln = _lines(L, prs, nl)
    if bad:
        ln[0, 5:300:7, :3] *= 1.01        # |dir|^2 > 1 + 1e-6: their wavefronts take the strict loop
        t1[1, 12345, 4] = float("nan")    # a NaN point 1: the reference's exit(0) flag
    strict = ops.loss_forward_raw(t1, t2, ln, mode="strict")
    ops.scan_counters(True, rows=1 << 19)
    counted = ops.loss_forward_raw(t1, t2, ln, mode="cull")
    c = ops.scan_counters(False)
    cull = ops.loss_forward_raw(t1, t2, ln, mode="cull")
    torch.cuda.synchronize()
    _same_evaluation(strict, cull)
    _same_evaluation(strict, counted)
    assert min(_selected(strict)) >= 20, _selected(strict)
    assert int(c[5]) > 0  # the culled scan's wavefronts ran
    if bad:  # a non-finite cloud sends all of its wavefronts, a non-unit line its own, through the strict loop
        assert int(cull.status[0]) == 1 and int(cull.status[1]) > 0 and int(c[6]) > 0 and int(c[7]) > 0
    else:  # ... and the culled walk made far fewer exact (line, triangle) tests than the dense scan's L (N + M)
        exact = int(c[4]) + int(c[7])
        assert int(cull.status[1]) == 0 and int(c[6]) == 0 and exact < B * nl * (n + m) // 20, (exact, B * nl * (n + m))


def test_cull_matches_oracle_at_70000(L, oracle):
    """The oracle where it is cheap: 70 000 x 4096 triangles, 1000 lines, counts and loss."""
    from rrl_hip import ops
    prs, t1, t2 = _pairs(31, 1, 70000, 4096)
    ln = _lines(L, prs, 1000)
    st = ops.loss_forward_raw(t1, t2, ln, mode="cull")
    torch.cuda.synchronize()
    lines = ln[0].cpu().numpy()
    o = oracle.loss(prs[0]["src_tri"], prs[0]["tar_tri"], lines, want_grad=False)
    np.testing.assert_array_equal(st.count1[0].cpu().numpy(), oracle.scan(prs[0]["src_tri"], lines, cap=4)["count"])
    np.testing.assert_array_equal(st.count2[0].cpu().numpy(), oracle.scan(prs[0]["tar_tri"], lines, cap=4)["count"])
    assert o["n_selected"] >= 20
    np.testing.assert_allclose(float(st.loss[0]), o["loss"], rtol=2e-6)


@pytest.mark.parametrize("n", [100000, CAP])
def test_cloud_order_is_a_permutation(n):
    from rrl_hip import ops
    prs, t1, _ = _pairs(41, 1, n, 64)
    o = ops.cloud_order(t1)
    torch.cuda.synchronize()
    assert o.shape == (1, (n + 63) // 64 * 64) and o.dtype == torch.int32
    oc = o[0].cpu().numpy()
    assert np.array_equal(np.sort(oc[:n]), np.arange(n)) and not oc[n:].any()


@pytest.mark.parametrize("N,M", [(100000, 90000), (CAP, 5000)])
def test_prepared_steps_equal_cold_steps(L, N, M):
    from rrl_hip import ops
    from LieAlgebra import se3
    prs, src, tar = _pairs(51, 1, N, M)
    nl = 2000
    ln = _lines(L, prs, nl)
    R, t = se3.exp3(0.02 * torch.randn(1, 6, generator=torch.Generator().manual_seed(3)))
    R, t = R.cuda().contiguous(), t.cuda().contiguous()
    prep = ops.LossStep(src, tar, nl, prepared=True)
    cold = ops.LossStep(src, tar, nl, prepared=False)
    assert prep.prepared and not cold.prepared
    for _ in range(2):  # (the second call: kept target, chained build)
        lp, gp, ip = [x.clone() for x in prep(R, t, ln)]
    lc, gc, ic = [x.clone() for x in cold(R, t, ln)]
    torch.cuda.synchronize()
    assert torch.equal(lp, lc) and torch.equal(ip, ic) and int(ic[0, 1]) >= 20
    assert float((gp - gc).abs().max()) <= 1e-6 * float(gc.abs().max())
    rp = ops.RegistrationStep(src, tar, nl, prepared=True)
    rc = ops.RegistrationStep(src, tar, nl, prepared=False)
    for _ in range(2):
        a = [x.clone() for x in rp(R, t, ln) if x is not None]
    b = [x.clone() for x in rc(R, t, ln) if x is not None]
    torch.cuda.synchronize()
    assert rp.prepared and torch.equal(a[0], b[0]) and torch.equal(a[0], lc) and torch.equal(a[-1], b[-1])
    for x, y in zip(a[1:3], b[1:3]):
        assert float((x - y).abs().max()) <= 1e-6 * float(y.abs().max())


def test_multi_pose_equals_pose_after_pose(L):
    from rrl_hip import ops
    from LieAlgebra import se3
    k, N, M, nl = 3, 100000, 80000, 2000
    prs, src, tar = _pairs(61, 1, N, M)
    ln = _lines(L, prs, nl)
    R, t = se3.exp3(0.03 * torch.randn(k, 6, generator=torch.Generator().manual_seed(7)))
    R, t = R.cuda().contiguous(), t.cuda().contiguous()
    multi = ops.RegistrationStep(src, tar, nl, poses=k)
    lm, gRm, gtm, _, im = [x.clone() if x is not None else None for x in multi(R, t, ln)]
    torch.cuda.synchronize()
    assert lm.shape == (k,)
    for i in range(k):
        one = ops.RegistrationStep(src, tar, nl)
        l1, gR1, gt1, _, i1 = one(R[i:i + 1], t[i:i + 1], ln)
        torch.cuda.synchronize()
        assert torch.equal(lm[i:i + 1], l1) and torch.equal(im[i:i + 1], i1) and int(i1[0, 1]) >= 20
        for got, want in ((gRm[i:i + 1], gR1), (gtm[i:i + 1], gt1)):
            assert bool(((got - want).abs() <= 2e-5 * want.abs() + 2e-6 * float(want.abs().max())).all())


def _chamfer_keys(x, y, tree):
    from rrl_hip import ops, _lib
    B, N, _ = x.shape
    M = y.shape[1]
    bx = torch.full((B, N), -1, dtype=torch.int64, device="cuda")
    by = torch.full((B, M), -1, dtype=torch.int64, device="cuda")
    val = torch.empty(1, device="cuda")
    lib = _lib.load()
    if tree:
        nb = int(lib.rrl_chamfer_workspace_bytes(B, N, M))
        ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
        rc = lib.rrl_chamfer_tree_fwd(ops._p(x), ops._p(y), ops._p(ws), nb, ops._p(bx), ops._p(by), ops._p(val), B, N, M,
                                      ops._stream())
    else:
        rc = lib.rrl_chamfer_fwd(ops._p(x), ops._p(y), ops._p(bx), ops._p(by), ops._p(val), B, N, M, ops._stream())
    assert rc == 0
    torch.cuda.synchronize()
    return bx, by, val.item()


def test_chamfer_tree_on_large_clouds():
    from rrl_hip import ops, synth
    p = synth.make_pair(71, 150000, 120000)
    x, y = cu(p["src"])[None], cu(p["tar"])[None]
    tx, ty, tv = _chamfer_keys(x, y, True)
    bx, by, bv = _chamfer_keys(x, y, False)
    assert torch.equal(tx, bx) and torch.equal(ty, by) and abs(tv - bv) <= 2e-7 * abs(bv)
    vals, grads = [], []
    for tree in (True, False):
        ops.CHAMFER_TREE = tree
        try:
            xg, yg = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
            v = ops.chamfer(xg, yg)
            v.backward()
        finally:
            ops.CHAMFER_TREE = True
        vals.append(float(v.detach()))
        grads.append((xg.grad, yg.grad))
    assert abs(vals[0] - vals[1]) <= 2e-7 * abs(vals[1]) and abs(vals[0] - tv) <= 2e-7 * abs(tv)
    for g, h in zip(grads[0], grads[1]):  # the same minima; the backward scatters with float atomics
        torch.testing.assert_close(g, h, rtol=1e-5, atol=1e-6 * float(h.abs().max()))


def test_chamfer_rider_rides_on_large_clouds(L):
    from rrl_hip import ops
    N, M, nl = 100000, 90000, 2000
    prs, src, tar = _pairs(81, 1, N, M)
    ln = _lines(L, prs, nl)
    R = torch.eye(3, device="cuda")[None].contiguous()
    t = torch.zeros(1, 3, device="cuda")
    step = ops.RegistrationStep(src, tar, nl, chamfer=True)
    out = step(R, t, ln)
    torch.cuda.synchronize()
    assert step.ride is not None and step.ride.done
    x, y = src[:, :, :3].contiguous(), tar[:, :, :3].contiguous()
    _, _, want = _chamfer_keys(x, y, True)
    got = float(step.chamfer_value)
    assert abs(got - want) <= 2e-6 * abs(want) and int(out[-1][0, 1]) >= 20


def test_beyond_the_capacity_takes_the_legacy_path(L):
    """capacity + 1 triangles: the dense scan (cull behaves like auto) and the fused registration's separate rigid backward
    + payload kernels, against the unfused composition; a prepared order is refused."""
    from rrl_hip import ops
    from LieAlgebra import se3
    n, m, nl = CAP + 1, 3000, 300
    prs, src, tar = _pairs(91, 1, n, m)
    ln = _lines(L, prs, nl)
    with pytest.raises(ValueError):
        ops.cloud_order(src)
    cull = ops.loss_forward_raw(src, tar, ln, mode="cull")
    strict = ops.loss_forward_raw(src, tar, ln, mode="strict")
    torch.cuda.synchronize()
    _same_evaluation(strict, cull)
    assert _selected(strict)[0] >= 5
    R0, T0 = se3.exp3(0.02 * torch.randn(1, 6, generator=torch.Generator().manual_seed(13)))

    def run(fused):
        R, T = R0.cuda().requires_grad_(True), T0.cuda().requires_grad_(True)
        if fused:
            loss, info, _ = ops.registration_loss(src, R, T, tar, ln, transpose_r=True, want_payload=True)
        else:
            moved = ops.rigid_apply(src.reshape(1, -1, 3), R, T, transpose_r=True).reshape(src.shape)
            loss, info, _ = ops.intersection_loss(moved, tar, ln)
        loss.sum().backward()
        return loss.detach(), R.grad, T.grad, info

    ref, got = run(False), run(True)
    assert torch.equal(got[0], ref[0]) and int(ref[3][0, 1]) >= 5
    pay = ops.last_state().payload
    for a, b in ((got[1], ref[1]), (got[2], ref[2])):
        scale = float(b.abs().max()) + 1e-12
        torch.testing.assert_close(a, b, rtol=2e-4, atol=2e-6 * scale)
    assert float(pay[1]) == 1.0
