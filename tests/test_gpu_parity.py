"""Parity of the HIP path (through the C ABI, via the drop-in loss.py) against the golden
vectors captured from the reference and against the CPU oracle on identical inputs.

Tolerances (stated per BASELINE.json north_star: loss within 1e-5 rel):
  labels / counts / hit lists / Chamfer minima      bit-exact
  hit weights, D values                              bit-exact vs oracle, 2e-5 vs reference
  loss                                               1e-5 rel vs reference and oracle
  gradient (per-point sums, see merge_by_point)      1e-4 rel, 1e-5 of max abs
"""
import os

import numpy as np
import pytest
import torch

from conftest import load_golden, merge_by_point

pytestmark = pytest.mark.gpu

LOSS_FIXTURES = ["loss_synth_s0.npz", "loss_synth_s1.npz", "loss_demo_scale.npz",
                 "loss_edge_zero_dup.npz",
                 # the reference's OWN sample pairs (code/sample_data/: airplane 1024 / 1024, human 1024 / 2048,
                 # real-scan fragments 2048 / 2048), prepared like its demo does -- make_golden.py refdata
                 "loss_ref_airplane0.npz", "loss_ref_airplane3.npz", "loss_ref_human0.npz", "loss_ref_real0.npz",
                 # ... and the other seven pairs it ships (refdata_rest; challenge_data/0 is loss_demo_scale): all twelve
                 "loss_ref_airplane1.npz", "loss_ref_airplane2.npz", "loss_ref_airplane4.npz", "loss_ref_human1.npz",
                 "loss_ref_human2.npz", "loss_ref_real1.npz", "loss_ref_real2.npz"]


@pytest.fixture(scope="module")
def L():
    import loss
    from rrl_hip import _lib
    _lib.load()  # fail loudly if the HIP library is missing
    assert torch.cuda.is_available()
    return loss


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_state(tri1, tri2, lines, rng=(1, 1, 5, 5), pool=False, mode="auto", chunk=0, staged=False):
    from rrl_hip import ops
    t1, t2, ln = cu(tri1), cu(tri2), cu(lines)
    if t1.dim() == 2:
        t1, t2, ln = t1[None], t2[None], ln[None]
    st = ops.loss_forward_raw(t1, t2, ln, rng, pool, mode, chunk, staged)
    torch.cuda.synchronize()
    return st


# ---------------------------------------------------------------------------------- K1'
def test_tri_prepare_exact(L, oracle):
    g = load_golden("loss_demo_scale.npz")
    st = run_state(g["tri1"], g["tri2"], g["lines"])
    pt = st.ptri1[0].cpu().numpy()
    np.testing.assert_array_equal(pt[:, 11].copy().view(np.int32), np.arange(len(pt)))
    np.testing.assert_array_equal(pt[:, :9], g["tri1"])
    thr = oracle.tri_threshold(g["tri1"])
    np.testing.assert_array_equal(pt[:, 10], thr)
    # thr2 is the smallest float whose correctly rounded sqrt reaches thr
    thr2 = pt[:, 9]
    below = np.nextafter(thr2, np.float32(0), dtype=np.float32)
    assert np.all(np.sqrt(thr2) >= thr) and np.all(np.sqrt(below) < thr)
    # cell order: a permutation; every node of the sphere tree (supergroup of 64, groups of 16,
    # halves of 8) contains the P0s of its sorted records with the threshold margin
    n = len(pt)
    idx = st.idx1[0].cpu().numpy()[:n]
    assert sorted(idx.tolist()) == list(range(n))
    tree = st.grp1[0].cpu().numpy()
    assert tree.shape == ((n + 63) // 64, 13, 4)
    P0 = pt[idx, :3].astype(np.float64)
    for sg in range(len(tree)):
        nodes = [(0, 64 * sg, 64)] + [(1 + k, 64 * sg + 16 * k, 16) for k in range(4)] + \
                [(5 + k, 64 * sg + 8 * k, 8) for k in range(8)]
        for slot, s0, cnt in nodes:
            sl = slice(s0, min(s0 + cnt, n))
            if sl.start >= n:
                assert np.isnan(tree[sg, slot, 3])  # empty node: never passes
                continue
            d = np.linalg.norm(P0[sl] - tree[sg, slot, :3].astype(np.float64), axis=1) + thr[idx[sl]]
            assert np.all(d <= tree[sg, slot, 3])  # the stored conservative radius
    p0s = st.p0s1[0].cpu().numpy()
    for s_ in (0, 17, n - 1):
        slot = s_
        np.testing.assert_array_equal(p0s[slot], np.append(pt[idx[s_], :3], thr2[idx[s_]]))


def _check_sorted_layout(st, tri, thr, cloud=1, b=0):
    """Invariants of the build step for one cloud: IDX is a permutation, P0S holds (P0, thr2) of the indexed
    triangle, every tree node contains its sorted records with the threshold margin, empty nodes are NaN."""
    n = len(tri)
    pt = (st.ptri1 if cloud == 1 else st.ptri2)[b].cpu().numpy()
    idx = (st.idx1 if cloud == 1 else st.idx2)[b].cpu().numpy()
    p0s = (st.p0s1 if cloud == 1 else st.p0s2)[b].cpu().numpy()
    tree = (st.grp1 if cloud == 1 else st.grp2)[b].cpu().numpy()
    assert sorted(idx[:n].tolist()) == list(range(n))
    # the 48-byte records carry their triangle index: in original order (cold build) or at the sorted positions (prepared
    # build) -- by triangle from here on
    own = pt[:, 11].copy().view(np.int32)
    assert np.array_equal(own, np.arange(n)) or np.array_equal(own, idx[:n])
    pt = pt[np.argsort(own, kind="stable")]
    np.testing.assert_array_equal(p0s[:n, :3], pt[idx[:n], :3])
    np.testing.assert_array_equal(p0s[:n, 3], pt[idx[:n], 9])
    assert np.all(p0s[n:] == 0)
    P0 = pt[idx[:n], :3].astype(np.float64)
    for sg in range(len(tree)):
        nodes = [(0, 64 * sg, 64)] + [(1 + k, 64 * sg + 16 * k, 16) for k in range(4)] + \
                [(5 + k, 64 * sg + 8 * k, 8) for k in range(8)]
        for slot, s0, cnt in nodes:
            sl = slice(s0, min(s0 + cnt, n))
            if sl.start >= n:
                assert np.isnan(tree[sg, slot, 3])
                continue
            d = np.linalg.norm(P0[sl] - tree[sg, slot, :3].astype(np.float64), axis=1) + thr[idx[sl]]
            assert np.all(d <= tree[sg, slot, 3])


@pytest.mark.parametrize("parts", [1, 2, 3, 4, 7, 16])
def test_sort_parts_layout_and_results(L, oracle, parts):
    """The sort + tree kernel split over `parts` workgroups per cloud that share nothing but their input: same
    invariants of the sorted layout, same scan counts, same loss, same Chamfer keys as one workgroup -- on a cloud
    whose grid cells hold many records (600 of 3000 points are copies of three points: cells that straddle the
    parts' boundaries take the deterministic-rank route), ragged sizes and a chunked large cloud."""
    from rrl_hip import ops, synth
    pr = synth.make_pair(21, 3000, 1111)
    tri1, tri2 = pr["src_tri"].copy(), pr["tar_tri"].copy()
    tri1[200:500] = tri1[7]; tri1[900:1100] = tri1[8]; tri1[2000:2100] = tri1[9]
    rands = synth.uniform_streams(2, 10, 2500)
    lines = oracle.resample_lines(rands, pr["radius"], pr["center"], pr["src"], pr["tar"], 2500)
    big = synth.make_pair(22, 5000, 4100)
    res = {}
    try:
        for k in (1, parts):
            ops.set_sort_parts(k)
            st = run_state(tri1, tri2, lines, mode="cull")
            _check_sorted_layout(st, tri1, oracle.tri_threshold(tri1), 1)
            _check_sorted_layout(st, tri2, oracle.tri_threshold(tri2), 2)
            stb = run_state(big["src_tri"], big["tar_tri"], lines, mode="cull")  # chunks of 4096 + a ragged last chunk
            cx = ops.chamfer_from_state(st, keys=True)
            cy = ops.chamfer(cu(tri1[None, :, :3].copy()), cu(tri2[None, :, :3].copy()))
            res[k] = [t.cpu().numpy().copy() for t in (st.count1, st.count2, st.loss, stb.count1, stb.count2, stb.loss,
                                                         cx[0].reshape(1), cx[1], cx[2], cy.reshape(1))]
    finally:
        ops.set_sort_parts(0)
    for a, b in zip(res[1], res[parts]):
        np.testing.assert_array_equal(a, b)
    s_ = run_state(tri1, tri2, lines, mode="strict")
    np.testing.assert_array_equal(res[parts][0], s_.count1.cpu().numpy())
    np.testing.assert_array_equal(res[parts][1], s_.count2.cpu().numpy())


@pytest.mark.parametrize("tr", [True, False])
def test_registration_step_equals_the_autograd_op(L, tr):
    """ops.RegistrationStep (forward + backward as two C calls on preallocated buffers, no autograd node)
    against ops.registration_loss + autograd: same loss bits, same info, dR / dt / payload to the rounding
    noise of the float atomics; repeated calls on the same object and a non-unit grad_loss."""
    from rrl_hip import ops, synth
    B, N, M, Ll = 3, 1500, 1100, 2500
    prs = [synth.make_pair(50 + b, N, M) for b in range(B)]
    src, tar = cu(np.stack([p["src_tri"] for p in prs])), cu(np.stack([p["tar_tri"] for p in prs]))
    ln = []
    for b, p in enumerate(prs):
        torch.manual_seed(b)
        ln.append(L.Random_uniform_distribution_lines_batch_efficient_resample(
            torch.tensor([[float(p["radius"])]]), torch.from_numpy(p["center"]).reshape(1, 3), Ll,
            cu(p["src"])[None], cu(p["tar"])[None], "cuda")[0])
    ln = torch.stack(ln)
    ang = torch.tensor([0.05, -0.1, 0.2], device="cuda")
    R0 = torch.zeros(B, 3, 3, device="cuda")
    R0[:, 0, 0] = R0[:, 1, 1] = torch.cos(ang); R0[:, 0, 1] = -torch.sin(ang); R0[:, 1, 0] = torch.sin(ang); R0[:, 2, 2] = 1
    t0 = torch.tensor([[0.01, 0.0, -0.02]] * B, device="cuda")
    gout = torch.tensor([1.0, 0.5, 2.0], device="cuda")
    R, t = R0.clone().requires_grad_(True), t0.clone().requires_grad_(True)
    loss, info, _ = ops.registration_loss(src, R, t, tar, ln, transpose_r=tr, want_payload=True)
    torch.autograd.backward([loss], [gout])
    want_payload = ops.last_state().payload.clone()
    step = ops.RegistrationStep(src, tar, Ll, transpose_r=tr, want_payload=True)
    for rep in range(3):  # the buffers are reused: every call must stand on its own
        l2, gR, gt, payload, info2 = step(R0, t0, ln, gout)
        torch.cuda.synchronize()
        assert torch.equal(l2, loss.detach()) and torch.equal(info2, info)
        np.testing.assert_allclose(gR.cpu().numpy(), R.grad.cpu().numpy(), rtol=2e-5, atol=1e-7)
        np.testing.assert_allclose(gt.cpu().numpy(), t.grad.cpu().numpy(), rtol=2e-5, atol=1e-7)
        np.testing.assert_allclose(payload.cpu().numpy(), want_payload.cpu().numpy(), rtol=2e-5, atol=1e-7)
    l1 = step(R0, t0, ln)[0]  # default grad_loss = ones
    assert torch.equal(l1, loss.detach())
    # a new batch of the same shape through the same object
    l3 = step(R0, t0, ln, gout, src_tri=src.flip(0).contiguous(), tar_tri=tar.flip(0).contiguous())[0].clone()
    want3, _, _ = ops.registration_loss(src.flip(0).contiguous(), R0, t0, tar.flip(0).contiguous(), ln, transpose_r=tr)
    assert torch.equal(l3, want3)


@pytest.mark.parametrize("wide", [0, 1])
@pytest.mark.parametrize("N,M", [(5000, 4100), (16400, 9000), (65536, 4097)])
def test_large_cloud_layouts(L, N, M, wide, monkeypatch):
    """Clouds of more than 4096 triangles: the chunked single-launch sort (default: every chunk of 4096 records in
    its own Hilbert order) and the wide whole-cloud sort (RRL_SORT_WIDE=1) both leave a permutation whose real
    records occupy the sorted positions [0, n), tree nodes that bound their records, and the same labels,
    loss and hit lists as the strict scan."""
    from rrl_hip import ops, synth
    monkeypatch.setenv("RRL_SORT_WIDE", str(wide))
    pr = synth.make_pair(7, N, M)
    src, tar = cu(pr["src_tri"])[None], cu(pr["tar_tri"])[None]
    torch.manual_seed(2)
    ln = L.Random_uniform_distribution_lines_batch_efficient_resample(
        torch.tensor([[float(pr["radius"])]]), torch.from_numpy(pr["center"]).reshape(1, 3), 700,
        cu(pr["src"])[None], cu(pr["tar"])[None], "cuda")
    st = ops.loss_forward_raw(src, tar, ln, mode="cull")
    ref = ops.loss_forward_raw(src, tar, ln, mode="strict")
    torch.cuda.synchronize()
    assert torch.equal(st.count1, ref.count1) and torch.equal(st.count2, ref.count2) and torch.equal(st.loss, ref.loss)
    assert int(st.status[0]) == 0 and int(st.status[1]) == 0
    for l in torch.nonzero((st.count1[0] > 0) & (st.count1[0] <= 4))[:50, 0].tolist():  # beyond 4 hits any 4 are kept
        k = int(st.count1[0, l])
        assert sorted(st.hit1[0, l, :k].tolist()) == sorted(ref.hit1[0, l, :k].tolist())
    for n, idx_t, p0s_t, tree_t, ptri_t in ((N, st.idx1, st.p0s1, st.grp1, st.ptri1), (M, st.idx2, st.p0s2, st.grp2, st.ptri2)):
        idx = idx_t[0].cpu().numpy()
        assert sorted(idx[:n].tolist()) == list(range(n))          # real records at the positions [0, n)
        pt = ptri_t[0].cpu().numpy()
        p0s = p0s_t[0].cpu().numpy()
        np.testing.assert_array_equal(p0s[:n, :3], pt[idx[:n], :3])
        np.testing.assert_array_equal(p0s[:n, 3], pt[idx[:n], 9])
        assert np.all(p0s[n:, 3] == 0)                              # pad records never pass
        tree = tree_t[0].cpu().numpy()
        P0, thr = pt[idx[:n], :3].astype(np.float64), pt[idx[:n], 10].astype(np.float64)
        rng = np.random.default_rng(N + M)
        for sg in set(rng.integers(0, len(tree), 40).tolist()) | {0, len(tree) - 1, (n - 1) // 64}:
            nodes = [(0, 64 * sg, 64)] + [(1 + k, 64 * sg + 16 * k, 16) for k in range(4)] + \
                    [(5 + k, 64 * sg + 8 * k, 8) for k in range(8)]
            for slot, s0, cnt in nodes:
                sl = slice(s0, min(s0 + cnt, n))
                if sl.start >= n:
                    assert np.isnan(tree[sg, slot, 3])
                    continue
                d = np.linalg.norm(P0[sl] - tree[sg, slot, :3].astype(np.float64), axis=1) + thr[sl]
                assert np.all(d <= tree[sg, slot, 3])


# ---------------------------------------------------------------------------------- K1
@pytest.mark.parametrize("name", LOSS_FIXTURES)
@pytest.mark.parametrize("mode", ["strict", "lazy", "auto", "cull"])
def test_scan_counts_and_hits(L, oracle, name, mode):
    g = load_golden(name)
    st = run_state(g["tri1"], g["tri2"], g["lines"], mode=mode)
    assert int(st.status[0]) == 0
    # no wavefront of the culled scan leaves the culled path -- at the demo's scale (radius 11.7) neither
    assert int(st.status[1]) == 0
    for tag, cnt, hit in (("1", st.count1, st.hit1), ("2", st.count2, st.hit2)):
        cnt = cnt[0].cpu().numpy()
        hit = hit[0].cpu().numpy()
        np.testing.assert_array_equal(cnt, g["count" + tag])  # vs the reference
        o = oracle.scan(g["tri" + tag], g["lines"], cap=8)
        for l in np.nonzero((cnt > 0) & (cnt <= 4))[0]:
            assert sorted(hit[l, :cnt[l]].tolist()) == o["hit_idx"][l, :cnt[l]].tolist()


@pytest.mark.parametrize("name", LOSS_FIXTURES)
def test_dense_public_scan(L, name):
    """cal_intersection_batch2_points_with_line: labels equal the reference's exactly, weights at
    the hits to 2e-5 (torch's CPU sqrt is build-specific), every weight row sums to 1, and
    `points` is a stride-0 view of the input that carries its grad."""
    g = load_golden(name)
    for tri, sfx in ((g["tri1"], "1"), (g["tri2"], "2")):
        p = cu(tri)[None].requires_grad_(True)
        points, norm_d, label = L.cal_intersection_batch2_points_with_line(p, cu(g["lines"])[None])
        nl, nf = g["lines"].shape[0], tri.shape[0]
        assert points.shape == (nl, nf, 9) and norm_d.shape == (nl, nf, 3) and label.shape == (1, nl, nf)
        assert label.dtype == torch.bool and not norm_d.requires_grad and points.requires_grad
        assert points.stride(0) == 0 and points.data_ptr() == p.data_ptr()
        li, fi = np.nonzero(label[0].cpu().numpy())
        np.testing.assert_array_equal(li, g["hit_line" + sfx])
        np.testing.assert_array_equal(fi, g["hit_tri" + sfx])
        np.testing.assert_array_equal(label[0].sum(1).cpu().numpy(), g["count" + sfx])
        np.testing.assert_allclose(norm_d.cpu().numpy()[li, fi], g["hit_w" + sfx], rtol=2e-5)
        np.testing.assert_allclose(norm_d.sum(-1).cpu().numpy(), 1.0, rtol=3e-7)
    with pytest.raises(ValueError):
        L.cal_intersection_batch2_points_with_line(cu(g["tri1"]), cu(g["lines"])[None])
    bad = g["lines"].copy()
    bad[:, :3] *= 3.0
    with pytest.raises(ValueError):
        L.cal_intersection_batch2_points_with_line(cu(g["tri1"])[None], cu(bad)[None])


@pytest.mark.parametrize("variant", [1, 2, 4, 8])
@pytest.mark.parametrize("chunk", [0, 64, 1000])
@pytest.mark.parametrize("mode", ["strict", "lazy"])
def test_scan_variants_identical(L, variant, chunk, mode):
    from rrl_hip import _lib
    g = load_golden("loss_synth_s1.npz")
    lib = _lib.load()
    try:
        assert lib.rrl_set_scan_variant(variant) == 0
        st = run_state(g["tri1"], g["tri2"], g["lines"], chunk=chunk, mode=mode, staged=True)
        np.testing.assert_array_equal(st.count1[0].cpu().numpy(), g["count1"])
        np.testing.assert_array_equal(st.count2[0].cpu().numpy(), g["count2"])
        np.testing.assert_allclose(st.loss.cpu().numpy()[0], g["r0_loss"], rtol=1e-5)
    finally:
        lib.rrl_set_scan_variant(0)


def test_auto_mode_picks_lazy_only_when_nan_is_impossible(L):
    """Unit-scale data: auto == lazy == strict bit for bit.  Demo-scale data ((|x0|+|P|)^2 > 100)
    and non-unit directions must take the strict loop, so the NaN flag is still raised."""
    g = load_golden("loss_synth_s0.npz")
    a, s_, z, c = (run_state(g["tri1"], g["tri2"], g["lines"], mode=m)
                   for m in ("auto", "strict", "lazy", "cull"))
    assert a.loss[0].item() == s_.loss[0].item() == z.loss[0].item() == c.loss[0].item()
    assert float(a.pmax.max()) < 4.0
    d = load_golden("loss_demo_scale.npz")
    bad = d["lines"].copy()
    bad[5, :3] *= 1.5  # one non-unit direction among thousands of good lines
    assert int(run_state(d["tri1"], d["tri2"], bad, mode="strict").status[0]) == 1
    assert int(run_state(d["tri1"], d["tri2"], bad, mode="auto").status[0]) == 1
    assert int(run_state(d["tri1"], d["tri2"], bad, mode="cull").status[0]) == 1
    bad2 = g["lines"].copy()
    bad2[77, :3] *= 40.0
    assert int(run_state(g["tri1"], g["tri2"], bad2, mode="strict").status[0]) == 1
    assert int(run_state(g["tri1"], g["tri2"], bad2, mode="auto").status[0]) == 1
    cs = run_state(g["tri1"], g["tri2"], bad2, mode="cull")
    ss = run_state(g["tri1"], g["tri2"], bad2, mode="strict")
    assert int(cs.status[0]) == 1  # the bad line's 512-tile went to the strict loop
    np.testing.assert_array_equal(cs.count1.cpu().numpy(), ss.count1.cpu().numpy())
    np.testing.assert_array_equal(cs.count2.cpu().numpy(), ss.count2.cpu().numpy())


# ---------------------------------------------------------------------------------- K2..K4
@pytest.mark.parametrize("name", LOSS_FIXTURES)
def test_sparse_stage_vs_oracle(L, oracle, name):
    g = load_golden(name)
    for i, rng in enumerate(g["ranges"]):
        rng = tuple(int(v) for v in rng)
        st = run_state(g["tri1"], g["tri2"], g["lines"], rng)
        kj = st.kj[0].cpu().numpy()
        D = st.D[0].cpu().numpy()
        k, j = kj & 15, kj >> 4
        # D values in the reference's concatenation order: bucket-major, then line
        mine = []
        for kk in range(rng[0], rng[2]):
            for jj in range(rng[1], rng[3]):
                for l in np.nonzero((k == kk) & (j == jj))[0]:
                    mine.append(D[l, :kk * jj])
        mine = np.concatenate(mine)
        o = oracle.loss(g["tri1"], g["tri2"], g["lines"], rng=rng, want_D=True)
        np.testing.assert_array_equal(mine, o["D"])  # same arithmetic, same bits
        np.testing.assert_allclose(mine, g[f"r{i}_D"], rtol=2e-5, atol=1e-9)
        assert float(st.med[0]) == float(o["median"])
        assert int(st.info[0, 2]) == o["n_values"] and int(st.nbuckets[0]) == o["n_buckets"]
        assert int(st.info[0, 1]) == o["n_selected"]
        np.testing.assert_allclose(float(st.loss[0]), o["loss"], rtol=2e-6)
        np.testing.assert_allclose(float(st.loss[0]), g[f"r{i}_loss"], rtol=1e-5)


# ---------------------------------------------------------------------------------- W + G
@pytest.mark.parametrize("name", LOSS_FIXTURES)
def test_public_loss_and_gradient(L, oracle, name):
    g = load_golden(name)
    for i, rng in enumerate(g["ranges"]):
        p1 = cu(g["tri1"])[None].requires_grad_(True)
        out = L.cal_loss_intersection_batch_whole_median_pts_lines(
            *[int(v) for v in rng], p1, cu(g["tri2"])[None], cu(g["lines"])[None], "cuda")
        assert out.shape == (1,) and out.dtype == torch.float32 and out.is_cuda
        np.testing.assert_allclose(out.item(), g[f"r{i}_loss"], rtol=1e-5)
        (3.0 * out).backward()
        mine = merge_by_point(g["tri1"], p1.grad[0].cpu().numpy() / 3.0)
        ref = merge_by_point(g["tri1"], g[f"r{i}_grad1"])
        np.testing.assert_allclose(mine, ref, rtol=1e-4, atol=1e-5 * np.abs(ref).max())
        o = oracle.loss(g["tri1"], g["tri2"], g["lines"], rng=tuple(int(v) for v in rng))
        om = merge_by_point(g["tri1"], o["grad1"])
        np.testing.assert_allclose(mine, om, rtol=1e-4, atol=1e-6 * np.abs(om).max())


def test_gradient_wrt_target(L, oracle):
    g = load_golden("loss_synth_s0.npz")
    p2 = cu(g["tri2"])[None].requires_grad_(True)
    out = L.cal_loss_intersection_batch_whole_median_pts_lines(
        1, 1, 5, 5, cu(g["tri1"])[None], p2, cu(g["lines"])[None], "cuda")
    out.backward()
    o = oracle.loss(g["tri1"], g["tri2"], g["lines"], want_grad2=True)
    mine, om = merge_by_point(g["tri2"], p2.grad[0].cpu().numpy()), merge_by_point(g["tri2"], o["grad2"])
    np.testing.assert_allclose(mine, om, rtol=1e-4, atol=1e-6 * np.abs(om).max())


def test_cpu_inputs_and_result_device(L):
    """Callers may hand CPU tensors / non-contiguous slices and ask for the result on 'cpu'."""
    g = load_golden("loss_synth_s1.npz")
    big = torch.from_numpy(np.stack([g["tri1"], g["tri1"]]))
    p1 = big[1:2].clone().requires_grad_(True)
    out = L.cal_loss_intersection_batch_whole_median_pts_lines(
        1, 1, 5, 5, p1, torch.from_numpy(g["tri2"])[None], torch.from_numpy(g["lines"])[None], "cpu")
    assert out.device.type == "cpu"
    np.testing.assert_allclose(out.item(), g["r0_loss"], rtol=1e-5)
    out.backward()
    assert p1.grad is not None and p1.grad.device.type == "cpu" and p1.grad.abs().sum() > 0


def test_empty_returns_none(L):
    g = load_golden("loss_edge_allmiss.npz")
    out = L.cal_loss_intersection_batch_whole_median_pts_lines(
        1, 1, 5, 5, cu(g["tri1"])[None], cu(g["tri2"])[None], cu(g["lines"])[None], "cuda")
    assert out is None


def test_nan_raises(L):
    g = load_golden("loss_demo_scale.npz")
    bad = g["lines"].copy()
    bad[:, :3] *= 3.0  # non-unit directions -> sqrt of a negative number in the reference
    with pytest.raises(ValueError, match="NaN"):
        L.cal_loss_intersection_batch_whole_median_pts_lines(
            1, 1, 5, 5, cu(g["tri1"])[None], cu(g["tri2"])[None], cu(bad)[None], "cuda")


def test_bad_rank_and_range(L):
    g = load_golden("loss_edge_allmiss.npz")
    with pytest.raises(ValueError):
        L.cal_loss_intersection_batch_whole_median_pts_lines(
            1, 1, 5, 5, cu(g["tri1"]), cu(g["tri2"])[None], cu(g["lines"])[None], "cuda")
    with pytest.raises(ValueError):
        L.cal_loss_intersection_batch_whole_median_pts_lines(
            1, 1, 6, 5, cu(g["tri1"])[None], cu(g["tri2"])[None], cu(g["lines"])[None], "cuda")


def test_b2_pooling_quirk(L):
    """B > 1 through the reference signature pools lines and uses the last sample's median."""
    g = load_golden("loss_b2_quirk.npz")
    p1 = cu(g["tri1"]).requires_grad_(True)
    out = L.cal_loss_intersection_batch_whole_median_pts_lines(
        1, 1, 5, 5, p1, cu(g["tri2"]), cu(g["lines"]), "cuda")
    np.testing.assert_allclose(out.item(), g["loss"], rtol=1e-5)
    out.backward()
    for b in range(2):
        mine = merge_by_point(g["tri1"][b], p1.grad[b].cpu().numpy())
        ref = merge_by_point(g["tri1"][b], g["grad1"][b])
        np.testing.assert_allclose(mine, ref, rtol=1e-4, atol=1e-5 * np.abs(ref).max())


def test_batched_equals_per_sample(L):
    """Independent-sample semantics: batch result == B single calls, bit for bit."""
    g = load_golden("loss_b2_quirk.npz")
    p1, p2, ln = cu(g["tri1"]), cu(g["tri2"]), cu(g["lines"])
    loss, valid = L.batched_intersection_loss(p1, p2, ln)
    assert bool(valid.all())
    for b in range(2):
        one = L.cal_loss_intersection_batch_whole_median_pts_lines(
            1, 1, 5, 5, p1[b:b + 1], p2[b:b + 1], ln[b:b + 1], "cuda")
        assert one.item() == loss[b].item()


@pytest.fixture
def per_call_dropin():
    """the reference-signature call evaluated per call (round 3's path), not served from a whole-batch evaluation"""
    from rrl_hip import ops
    old, ops.DROPIN_BATCH = ops.DROPIN_BATCH, False
    yield
    ops.DROPIN_BATCH = old
    ops.dropin_batch_clear()


def test_trainer_loop_over_samples(L, per_call_dropin):
    """The reference trainers' literal pattern (rpm/Train_RPM.py:226-231): B reference-signature calls on [j:j+1]
    slices summed in Python, ONE backward at the end.  The calls lease their workspaces from a per-shape pool
    (ops._DropinLoss): every forward must keep its own state until the backward has used it, results held by the
    caller must not alias, and a second round must reuse the pool instead of growing it.  (Per-call evaluation:
    ops.DROPIN_BATCH off; the batched serving of the same loop is the next test.)"""
    from rrl_hip import ops, synth
    B, N, M, Ll = 4, 700, 600, 1500
    prs = [synth.make_pair(400 + b, N, M) for b in range(B)]
    tri1 = cu(np.stack([p["src_tri"] for p in prs]))
    tri2 = cu(np.stack([p["tar_tri"] for p in prs]))
    ln = []
    for b, p in enumerate(prs):
        torch.manual_seed(b)
        ln.append(L.Random_uniform_distribution_lines_batch_efficient_resample(
            torch.tensor([[float(p["radius"])]]), torch.from_numpy(p["center"]).reshape(1, 3), Ll,
            cu(p["src"])[None], cu(p["tar"])[None], "cuda")[0])
    ln = torch.stack(ln)
    ref_in = tri1.clone().requires_grad_(True)
    ref_loss, ref_info, _ = ops.intersection_loss(ref_in, tri2, ln)
    ref_loss.sum().backward()
    assert int((ref_info[:, 0] > 0).sum()) == B
    for rnd in range(2):
        p1 = tri1.clone().requires_grad_(True)
        parts, total = [], 0
        for j in range(B):
            one = L.cal_loss_intersection_batch_whole_median_pts_lines(1, 1, 5, 5, p1[j:j + 1], tri2[j:j + 1], ln[j:j + 1], "cuda")
            assert one is not None and one.shape == (1,)
            parts.append(one)
            total = total + one
        for j in range(B):  # nothing was overwritten by the later calls
            assert parts[j].item() == ref_loss[j].item()
        total.backward()
        np.testing.assert_allclose(p1.grad.cpu().numpy(), ref_in.grad.cpu().numpy(), rtol=2e-5, atol=1e-9)  # float atomics
        if rnd == 0:
            pooled = sum(len(v) for v in ops._pool.values())
    assert sum(len(v) for v in ops._pool.values()) == pooled  # the second round reused the leased states
    with torch.no_grad():  # no autograd node keeps the state: still no aliasing between successive results
        a = L.cal_loss_intersection_batch_whole_median_pts_lines(1, 1, 5, 5, tri1[0:1], tri2[0:1], ln[0:1], "cuda")
        b_ = L.cal_loss_intersection_batch_whole_median_pts_lines(1, 1, 5, 5, tri1[1:2], tri2[1:2], ln[1:2], "cuda")
    assert a.item() == ref_loss[0].item() and b_.item() == ref_loss[1].item()


def test_trainer_loop_served_by_one_batch_evaluation(L):
    """Round 4: the same literal loop, but the first call of a loop over [j:j+1] slices evaluates the WHOLE batch once
    (ops._serve_from_batch) and the other calls are slices of that one autograd node.  Against the per-call path
    (ops.DROPIN_BATCH off) on the same inputs: every returned loss bit for bit, None for the sample without a
    populated bucket, gradients to the rounding of the scatter's atomics, exactly one evaluation per batch -- also for
    out-of-order j, under no_grad, after an in-place edit between two calls (re-evaluated), with bases that do not
    belong together (per-call path) and with a NaN sample in the batch (raises at that sample's call only)."""
    from rrl_hip import ops, synth
    B, N, M, Ll = 5, 600, 500, 1500
    prs = [synth.make_pair(430 + b, N, M) for b in range(B)]
    tri1 = cu(np.stack([p["src_tri"] for p in prs]))
    tri2 = cu(np.stack([p["tar_tri"] for p in prs]))
    ln = []
    for b, p in enumerate(prs):
        torch.manual_seed(b)
        ln.append(L.Random_uniform_distribution_lines_batch_efficient_resample(
            torch.tensor([[float(p["radius"])]]), torch.from_numpy(p["center"]).reshape(1, 3), Ll,
            cu(p["src"])[None], cu(p["tar"])[None], "cuda")[0])
    ln = torch.stack(ln)
    ln[2] = torch.tensor([1.0, 0, 0, 0, 50, 50], device="cuda")  # sample 2: every line misses both clouds -> None

    def loop(p1, t2, lines, order, batch):
        old, ops.DROPIN_BATCH = ops.DROPIN_BATCH, batch
        try:
            out = {}
            for j in order:
                out[j] = L.cal_loss_intersection_batch_whole_median_pts_lines(1, 1, 5, 5, p1[j:j + 1], t2[j:j + 1], lines[j:j + 1], "cuda")
            return out
        finally:
            ops.DROPIN_BATCH = old

    def run(order, batch, lines=ln):
        p1 = tri1.clone().requires_grad_(True)
        out = loop(p1, tri2, lines, order, batch)
        total = 0
        for j in order:
            if out[j] is not None:
                total = total + out[j]
        total.backward()
        return out, p1.grad.clone(), float(total)

    ops.dropin_batch_clear()
    for order in (list(range(B)), [3, 1, 0, 4, 2], [1, 1, 3]):
        ref, gref, tref = run(order, False)
        ev0, sv0 = ops.dropin_batch_stats["evaluations"], ops.dropin_batch_stats["served"]
        got, ggot, tgot = run(order, True)
        assert ops.dropin_batch_stats["evaluations"] == ev0 + 1 and ops.dropin_batch_stats["served"] == sv0 + len(order)
        assert tref == tgot
        for j in set(order):
            if ref[j] is None:
                assert got[j] is None and j == 2
            else:
                assert got[j].shape == (1,) and got[j].item() == ref[j].item() and got[j].grad_fn is not None
        np.testing.assert_allclose(ggot.cpu().numpy(), gref.cpu().numpy(), rtol=2e-5, atol=1e-9)
        assert float(ggot[2].abs().sum()) == 0.0
    # under no_grad: plain tensors, the same values, one evaluation
    with torch.no_grad():
        ev0 = ops.dropin_batch_stats["evaluations"]
        got = loop(tri1, tri2, ln, range(B), True)
        assert ops.dropin_batch_stats["evaluations"] == ev0 + 1
    ref, _, _ = run(list(range(B)), False)
    assert all((got[j] is None) == (ref[j] is None) and (got[j] is None or (got[j].item() == ref[j].item() and got[j].grad_fn is None))
               for j in range(B))
    # an in-place edit of a base between two calls: the cached evaluation is stale, the next call evaluates again
    ln2 = ln.clone()
    p1 = tri1.clone().requires_grad_(True)
    ev0 = ops.dropin_batch_stats["evaluations"]
    a0 = loop(p1, tri2, ln2, [0, 1], True)
    with torch.no_grad():
        ln2[3] = ln[4]  # (lines of another sample: still unit directions)
    a1 = loop(p1, tri2, ln2, [3, 4], True)
    assert ops.dropin_batch_stats["evaluations"] == ev0 + 2
    want = loop(tri1.clone().requires_grad_(True), tri2, ln2, [0, 1, 3, 4], False)
    for j, got_j in ((0, a0[0]), (1, a0[1]), (3, a1[3]), (4, a1[4])):
        assert (got_j is None) == (want[j] is None) and (got_j is None or got_j.item() == want[j].item())
    # bases that do not belong together (another batch size / another j): the per-call path, same values
    tri2_big = torch.cat([tri2, tri2[:1]])  # B + 1 samples
    ev0 = ops.dropin_batch_stats["evaluations"]
    mixed = loop(tri1, tri2_big, ln, [0, 1], True)
    assert ops.dropin_batch_stats["evaluations"] == ev0
    old, ops.DROPIN_BATCH = ops.DROPIN_BATCH, True
    try:
        crossed = L.cal_loss_intersection_batch_whole_median_pts_lines(1, 1, 5, 5, tri1[0:1], tri2[1:2], ln[0:1], "cuda")
    finally:
        ops.DROPIN_BATCH = old
    assert ops.dropin_batch_stats["evaluations"] == ev0
    assert mixed[0].item() == ref[0].item() and mixed[1].item() == ref[1].item() and crossed is not None
    # a NaN sample (non-unit direction): raises at ITS call, the others return their values
    ln3 = ln.clone()
    ln3[1, :, :3] *= 1.5
    for batch in (False, True):
        p1 = tri1.clone().requires_grad_(True)
        old, ops.DROPIN_BATCH = ops.DROPIN_BATCH, batch
        try:
            vals = {}
            for j in range(B):
                if j == 1:
                    with pytest.raises(ValueError):
                        L.cal_loss_intersection_batch_whole_median_pts_lines(1, 1, 5, 5, p1[j:j + 1], tri2[j:j + 1], ln3[j:j + 1], "cuda")
                else:
                    vals[j] = L.cal_loss_intersection_batch_whole_median_pts_lines(1, 1, 5, 5, p1[j:j + 1], tri2[j:j + 1], ln3[j:j + 1], "cuda")
        finally:
            ops.DROPIN_BATCH = old
        assert vals[0].item() == ref[0].item() and vals[3].item() == ref[3].item() and vals[2] is None
    assert ops.dropin_batch_stats["nan_fallbacks"] >= 1
    # a caller that accumulates IN PLACE into the first returned loss (`total = first; total += second`): allowed (the B
    # outputs are not views of one tensor as far as autograd is concerned), same sum, same gradient
    p1 = tri1.clone().requires_grad_(True)
    out = loop(p1, tri2, ln, [0, 1, 3], True)
    total = out[0]
    total += out[1]
    total += out[3]
    total.backward()
    want, gwant, _ = run([0, 1, 3], False)
    assert float(total) == float(want[0] + want[1] + want[3])
    np.testing.assert_allclose(p1.grad.cpu().numpy(), gwant.cpu().numpy(), rtol=2e-5, atol=1e-9)
    ops.dropin_batch_clear()


def test_shard_payload(L):
    from rrl_hip import ops
    g = load_golden("loss_b2_quirk.npz")
    p1 = cu(g["tri1"]).requires_grad_(True)
    loss, info, _ = ops.intersection_loss(p1, cu(g["tri2"]), cu(g["lines"]))
    gR = torch.arange(18.0, device="cuda").reshape(2, 3, 3)
    gT = torch.arange(6.0, device="cuda").reshape(2, 3)
    out = ops.shard_payload(loss, gR, gT).cpu().numpy()
    np.testing.assert_allclose(out[0], loss.sum().item(), rtol=1e-6)
    assert out[1] == 2.0
    np.testing.assert_allclose(out[2:11], gR.sum(0).reshape(-1).cpu().numpy())
    np.testing.assert_allclose(out[11:], gT.sum(0).cpu().numpy())
    sel = ops._IntersectionLoss.last_state
    n0 = int(sel.nsel[0])
    assert n0 == int(info[0, 1]) and sorted(sel.sel[0, :n0].tolist()) == \
        torch.nonzero(sel.kj[0]).reshape(-1).tolist()


def test_line_permutation_invariance(L):
    """Fixed-point bucket sums and the radix-select median are order independent: permuting
    the lines must not change a single bit of the loss."""
    g = load_golden("loss_synth_s0.npz")
    perm = np.random.default_rng(0).permutation(len(g["lines"]))
    a = run_state(g["tri1"], g["tri2"], g["lines"])
    b = run_state(g["tri1"], g["tri2"], g["lines"][perm])
    assert a.loss[0].item() == b.loss[0].item() and a.med[0].item() == b.med[0].item()


# ---------------------------------------------------------------------------------- full size
def test_full_size_sample_vs_oracle(L, oracle):
    """One BASELINE.json config-2 sample (N=M=4096, L=10000) against the oracle: counts exact,
    loss 2e-6, plus strict == lazy and batch invariance at B=3."""
    from rrl_hip import synth
    pr = synth.make_pair(0, 4096, 4096)
    rands = synth.uniform_streams(0, 10, 10000)
    lines = oracle.resample_lines(rands, pr["radius"], pr["center"], pr["src"], pr["tar"], 10000)
    st = run_state(pr["src_tri"], pr["tar_tri"], lines)
    o1 = oracle.scan(pr["src_tri"], lines, cap=4)
    o2 = oracle.scan(pr["tar_tri"], lines, cap=4)
    np.testing.assert_array_equal(st.count1[0].cpu().numpy(), o1["count"])
    np.testing.assert_array_equal(st.count2[0].cpu().numpy(), o2["count"])
    o = oracle.loss(pr["src_tri"], pr["tar_tri"], lines)
    assert o["n_selected"] > 300
    np.testing.assert_allclose(float(st.loss[0]), o["loss"], rtol=2e-6)
    for m in ("lazy", "strict", "auto"):
        other = run_state(pr["src_tri"], pr["tar_tri"], lines, mode=m)
        assert float(other.loss[0]) == float(st.loss[0])
        np.testing.assert_array_equal(other.count1.cpu().numpy(), st.count1.cpu().numpy())
        np.testing.assert_array_equal(other.count2.cpu().numpy(), st.count2.cpu().numpy())
    t1 = np.stack([pr["src_tri"]] * 3)
    t1[1] += 0.3  # a different middle sample must not disturb its neighbours
    bt = run_state(t1, np.stack([pr["tar_tri"]] * 3), np.stack([lines] * 3))
    assert float(bt.loss[0]) == float(st.loss[0]) == float(bt.loss[2])
    assert float(bt.loss[1]) != float(st.loss[0])


@pytest.mark.parametrize("mode", ["cull", "strict", "auto"])
@pytest.mark.parametrize("n,m", [(300, 200), (200, 300), (16390, 500), (65540, 300)])
def test_target_scan_reuse_is_bit_identical(L, mode, n, m):
    """rrl_*_forward_cached: a second source pose against the same target and lines, with the
    target's counts/hits carried over from the first call, equals the full evaluation bit for bit
    (loss, every workspace field the later stages read, and the gradient)."""
    from rrl_hip import ops, synth
    B, nl = 2, 1500
    prs = [synth.make_pair(60 + b, n, m) for b in range(B)]
    src = cu(np.stack([p["src_tri"] for p in prs]))
    tar = cu(np.stack([p["tar_tri"] for p in prs]))
    g = load_golden("sampler.npz")
    lines = cu(np.stack([np.resize(g["final"], (nl, 6))] * B))
    first = ops.loss_forward_raw(src, tar, lines, mode=mode)
    moved = src + 0.01
    full = ops.loss_forward_raw(moved, tar, lines, mode=mode)
    cached = ops.loss_forward_raw(moved, tar, lines, mode=mode, target_from=first)
    torch.cuda.synchronize()
    assert float(full.info[:, 1].sum()) > 0 or n > 20000  # very dense clouds: tiny triangles, few hits
    for f in ("loss", "count1", "count2", "med", "info", "status"):
        assert torch.equal(getattr(full, f), getattr(cached, f)), f
    c2 = full.count2.cpu().numpy()[..., None]  # slots >= count are scratch; > 4 hits: any 4 are kept
    live = (np.arange(4)[None, None, :] < c2) & (c2 <= 4)
    hf = np.where(live, full.hit2.cpu().numpy().reshape(live.shape), 1 << 30)
    hc = np.where(live, cached.hit2.cpu().numpy().reshape(live.shape), 1 << 30)
    np.testing.assert_array_equal(np.sort(hf, -1), np.sort(hc, -1))
    # a chain: the target carried over from an evaluation that itself carried it over -- resolved to the workspace that holds the
    # target's scan (round 4b: the per-line stage reads cloud 2's counts and hit lists THERE, nothing is copied any more)
    moved2 = src - 0.02
    full2 = ops.loss_forward_raw(moved2, tar, lines, mode=mode)
    chained = ops.loss_forward_raw(moved2, tar, lines, mode=mode, target_from=cached)
    torch.cuda.synchronize()
    assert chained.target_state is first
    for f in ("loss", "count1", "count2", "med", "info"):
        assert torch.equal(getattr(full2, f), getattr(chained, f)), f
    # through autograd, fused with the rigid transform
    R = torch.eye(3, device="cuda").repeat(B, 1, 1).requires_grad_(True)
    t = torch.full((B, 3), 0.01, device="cuda").requires_grad_(True)
    outs = []
    for tf in (None, first):
        R.grad = t.grad = None
        loss, _, _ = ops.registration_loss(src, R, t, tar, lines, mode=mode, target_from=tf)
        loss.sum().backward()
        outs.append((loss.detach().clone(), R.grad.clone(), t.grad.clone()))
    assert torch.equal(outs[0][0], outs[1][0])
    for a, b in zip(outs[0][1:], outs[1][1:]):  # float atomics in the backward: order-dependent bits
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6 * float(a.abs().max()))
    with pytest.raises(ValueError):
        ops.loss_forward_raw(moved[:, :-1], tar, lines, mode=mode, target_from=first)


@pytest.mark.parametrize("n,m,nl", [(1, 1, 1), (3, 2, 5), (16, 17, 63), (17, 16, 64), (33, 100, 65), (100, 31, 129),
                                    (250, 250, 1023), (64, 640, 1025), (5, 5, 4000)])
def test_ragged_sizes_vs_oracle(L, oracle, n, m, nl):
    """Sizes around every tile boundary of the kernels (16-triangle groups, 64-lane waves, 128-line
    workgroups, 1024-line tiles): counts exact, loss 2e-6 against the oracle, in the culled and the
    strict scan, through the fused op as well (B = 2: a real sample next to a shifted copy)."""
    from rrl_hip import ops, synth
    pr = synth.make_pair(300 + n + m, max(n, 8), max(m, 8))
    t1, t2 = pr["src_tri"][:n], pr["tar_tri"][:m]
    rands = synth.uniform_streams(n * 7 + m, 10, nl)
    lines = oracle.resample_lines(rands, pr["radius"], pr["center"], pr["src"], pr["tar"], nl)
    o = oracle.loss(t1, t2, lines)
    o1, o2 = oracle.scan(t1, lines, cap=4), oracle.scan(t2, lines, cap=4)
    for mode in ("cull", "strict"):
        st = run_state(t1, t2, lines, mode=mode)
        np.testing.assert_array_equal(st.count1[0].cpu().numpy(), o1["count"])
        np.testing.assert_array_equal(st.count2[0].cpu().numpy(), o2["count"])
        if o["loss"] is None:
            assert int(st.info[0, 0]) == 0 and float(st.loss[0]) == 0.0
        else:
            np.testing.assert_allclose(float(st.loss[0]), o["loss"], rtol=2e-6)
    src = cu(np.stack([t1, t1 + 0.02]))
    tar = cu(np.stack([t2, t2]))
    ln = cu(np.stack([lines, lines]))
    R = torch.eye(3, device="cuda").repeat(2, 1, 1).requires_grad_(True)
    t = torch.zeros(2, 3, device="cuda").requires_grad_(True)
    loss, info, _ = ops.registration_loss(src, R, t, tar, ln)
    loss.sum().backward()
    assert torch.isfinite(R.grad).all() and torch.isfinite(t.grad).all()
    if o["loss"] is None:
        assert int(info[0, 0]) == 0 and float(loss.detach()[0]) == 0.0 and float(R.grad[0].abs().sum()) == 0.0
    else:
        np.testing.assert_allclose(float(loss.detach()[0]), o["loss"], rtol=2e-6)
        # dL/dt of the fused op = sum of the per-point gradient of the oracle
        np.testing.assert_allclose(t.grad[0].cpu().numpy(), np.asarray(o["grad1"], np.float64).reshape(-1, 3).sum(0),
                                   rtol=2e-3, atol=2e-6)


def test_empty_line_set_and_empty_batch(L):
    """L = 0 lines: nothing selected -> None from the drop-in call, zero loss and gradient from the
    fused op; B = 0: empty tensors in, empty tensors out."""
    from rrl_hip import ops, synth
    pr = synth.make_pair(3, 40, 50)
    t1, t2 = cu(pr["src_tri"])[None], cu(pr["tar_tri"])[None]
    none = torch.zeros(1, 0, 6, device="cuda")
    assert L.cal_loss_intersection_batch_whole_median_pts_lines(1, 1, 5, 5, t1.clone().requires_grad_(True), t2,
                                                                none, "cuda") is None
    R = torch.eye(3, device="cuda")[None].requires_grad_(True)
    t = torch.zeros(1, 3, device="cuda").requires_grad_(True)
    loss, info, _ = ops.registration_loss(t1, R, t, t2, none, want_payload=True)
    loss.sum().backward()
    assert float(loss.detach()[0]) == 0.0 and int(info[0, 0]) == 0 and R.grad is None
    e = torch.zeros(0, 40, 9, device="cuda")
    loss, info, _ = ops.intersection_loss(e, torch.zeros(0, 50, 9, device="cuda"), torch.zeros(0, 10, 6, device="cuda"))
    assert loss.shape == (0,) and info.shape == (0, 4)
    loss, info, _ = ops.registration_loss(e, torch.zeros(0, 3, 3, device="cuda"), torch.zeros(0, 3, device="cuda"),
                                          torch.zeros(0, 50, 9, device="cuda"), torch.zeros(0, 10, 6, device="cuda"))
    assert loss.shape == (0,) and info.shape == (0, 4)


# BASELINE.json configs[0], [3], [4] (the bench runs configs[1]; [2] is its 8-GPU shard), plus a
# clouds beyond 4096 triangles (sort kernel re-reads its records) and one past the 65536-triangle
# limit of the sorted/culled layout (falls back to the dense scan)
@pytest.mark.parametrize("n,m,nl,crop,noise", [
    (1024, 1024, 20000, False, 0.01),    # C1 demo
    (2048, 1024, 10000, True, 0.02),     # C4 partial overlap + noise
    (16384, 16384, 512, False, 0.01),    # C5 fragments, 512 lines
    (16385, 1000, 768, False, 0.01),     # ragged N != M, large-cloud sort path
    (65537, 4096, 3000, False, 0.01),    # beyond the cull limit
])
def test_baseline_configs_vs_oracle(L, oracle, n, m, nl, crop, noise):
    from rrl_hip import synth
    pr = synth.make_pair(17, n, m, crop=crop, noise=noise)
    if n > 60000:  # at unit scale such a dense cloud has thr < sqrt(2e-4): no line can hit; enlarge it
        pr = {k: (v * np.float32(6.0) if isinstance(v, np.ndarray) or k == "radius" else v) for k, v in pr.items()}
    rands = synth.uniform_streams(17, 10, nl)
    lines = oracle.resample_lines(rands, pr["radius"], pr["center"], pr["src"], pr["tar"], nl)
    o = oracle.loss(pr["src_tri"], pr["tar_tri"], lines)
    o1 = oracle.scan(pr["src_tri"], lines, cap=4)
    o2 = oracle.scan(pr["tar_tri"], lines, cap=4)
    assert o["n_selected"] >= 4  # dense clouds have tiny pseudo-triangles: few of 512 lines hit
    for mode in ("cull", "strict"):
        st = run_state(pr["src_tri"], pr["tar_tri"], lines, mode=mode)
        np.testing.assert_array_equal(st.count1[0].cpu().numpy(), o1["count"])
        np.testing.assert_array_equal(st.count2[0].cpu().numpy(), o2["count"])
        np.testing.assert_allclose(float(st.loss[0]), o["loss"], rtol=2e-6)
    p1 = cu(pr["src_tri"])[None].requires_grad_(True)
    out = L.cal_loss_intersection_batch_whole_median_pts_lines(
        1, 1, 5, 5, p1, cu(pr["tar_tri"])[None], cu(lines)[None], "cuda")
    np.testing.assert_allclose(out.item(), o["loss"], rtol=2e-6)
    out.backward()
    mine = merge_by_point(pr["src_tri"], p1.grad[0].cpu().numpy())
    om = merge_by_point(pr["src_tri"], o["grad1"])
    np.testing.assert_allclose(mine, om, rtol=1e-4, atol=1e-6 * np.abs(om).max())


def test_config3_global_batch_64(L, oracle):
    """BASELINE.json configs[2]: B = 64 at N = M = 4096, L = 10000 -- what the eight ranks of a node hold
    together, here as ONE batch on one GPU (the shards are independent, so rank r's result is rows
    8r .. 8r+7 of this batch: `bench.py --global-batch 64`).  The fused op on the whole batch equals the
    per-shard evaluation bit for bit (loss, valid flags; dR / dt to atomics' rounding noise), the 14-float
    payload is the sum of the shard payloads, and three samples spread over the batch match the oracle."""
    from rrl_hip import ops, synth
    from LieAlgebra import se3
    B, N, M, nl = 64, 4096, 4096, 10000
    prs = [synth.make_pair(300 + b, N, M) for b in range(B)]
    src = cu(np.stack([p["src_tri"] for p in prs]))
    tar = cu(np.stack([p["tar_tri"] for p in prs]))
    lines = torch.stack([L.Random_uniform_distribution_lines_batch_efficient_resample(
        torch.tensor([[p["radius"]]]), torch.from_numpy(p["center"])[None], nl, cu(p["src"])[None], cu(p["tar"])[None],
        "cuda", device_rng=True)[0] for p in prs])
    R0, T0 = se3.exp3(0.03 * torch.randn(B, 6, generator=torch.Generator().manual_seed(9)))

    def run(lo, hi):
        R, t = R0[lo:hi].cuda().requires_grad_(True), T0[lo:hi].cuda().requires_grad_(True)
        loss, info, _ = ops.registration_loss(src[lo:hi], R, t, tar[lo:hi], lines[lo:hi], transpose_r=True,
                                              want_payload=True)
        loss.sum().backward()
        return loss.detach().clone(), (info[:, 0] > 0).clone(), R.grad.clone(), t.grad.clone(), ops.last_state().payload.clone()
    whole = run(0, B)
    pay = torch.zeros(14, device="cuda")
    for r in range(8):
        sh = run(8 * r, 8 * r + 8)
        assert torch.equal(sh[0], whole[0][8 * r:8 * r + 8]) and torch.equal(sh[1], whole[1][8 * r:8 * r + 8])
        np.testing.assert_allclose(sh[2].cpu().numpy(), whole[2][8 * r:8 * r + 8].cpu().numpy(), rtol=2e-5, atol=1e-7)
        np.testing.assert_allclose(sh[3].cpu().numpy(), whole[3][8 * r:8 * r + 8].cpu().numpy(), rtol=2e-5, atol=1e-7)
        pay += sh[4]
    np.testing.assert_allclose(pay.cpu().numpy(), whole[4].cpu().numpy(), rtol=2e-5, atol=1e-6)
    assert float(whole[4][1]) == B
    moved = ops.rigid_apply(src.reshape(B, -1, 3), R0.cuda(), T0.cuda(), transpose_r=True).reshape(B, N, 9).cpu().numpy()
    for b in (0, 29, 63):
        o = oracle.loss(moved[b], prs[b]["tar_tri"], lines[b].cpu().numpy(), want_grad=False)
        np.testing.assert_allclose(float(whole[0][b]), o["loss"], rtol=1e-5)


# ---------------------------------------------------------------------------------- K7
def test_chamfer(L, oracle):
    g = load_golden("chamfer.npz")
    x = cu(g["x"]).requires_grad_(True)
    val = L.chamfer_dist(x, cu(g["y"]))
    np.testing.assert_allclose(val.item(), g["value"], rtol=1e-6)
    val.backward()
    np.testing.assert_allclose(x.grad.cpu().numpy(), g["grad_x"], rtol=1e-5, atol=1e-8)


def test_chamfer_minima_bit_exact(L, oracle):
    from rrl_hip import ops, _lib
    rng = np.random.default_rng(5)
    x = rng.standard_normal((1, 1500, 3)).astype(np.float32)
    y = rng.standard_normal((1, 2300, 3)).astype(np.float32)
    y[0, 7] = y[0, 3]  # duplicate target: first occurrence must win
    xs, ys = cu(x), cu(y)
    bx = torch.empty(1, 1500, dtype=torch.int64, device="cuda")
    by = torch.empty(1, 2300, dtype=torch.int64, device="cuda")
    val = torch.empty(1, device="cuda")
    rc = _lib.load().rrl_chamfer_fwd(ops._p(xs), ops._p(ys), ops._p(bx), ops._p(by), ops._p(val),
                                     1, 1500, 2300, ops._stream())
    assert rc == 0
    mx, ax, my, ay = oracle.chamfer_parts(x[0], y[0])
    kx, ky = bx[0].cpu().numpy().view(np.uint64), by[0].cpu().numpy().view(np.uint64)
    np.testing.assert_array_equal((kx >> np.uint64(32)).astype(np.uint32).view(np.float32), mx)
    np.testing.assert_array_equal((kx & np.uint64(0xffffffff)).astype(np.int32), ax)
    np.testing.assert_array_equal((ky >> np.uint64(32)).astype(np.uint32).view(np.float32), my)
    np.testing.assert_array_equal((ky & np.uint64(0xffffffff)).astype(np.int32), ay)


def _chamfer_keys(x, y, tree):
    from rrl_hip import ops, _lib
    B, N, _ = x.shape
    M = y.shape[1]
    xs, ys = cu(x), cu(y)
    bx = torch.full((B, N), -1, dtype=torch.int64, device="cuda")
    by = torch.full((B, M), -1, dtype=torch.int64, device="cuda")
    val = torch.empty(1, device="cuda")
    lib = _lib.load()
    if tree:
        nb = int(lib.rrl_chamfer_workspace_bytes(B, N, M))
        ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
        rc = lib.rrl_chamfer_tree_fwd(ops._p(xs), ops._p(ys), ops._p(ws), nb, ops._p(bx), ops._p(by), ops._p(val),
                                      B, N, M, ops._stream())
    else:
        rc = lib.rrl_chamfer_fwd(ops._p(xs), ops._p(ys), ops._p(bx), ops._p(by), ops._p(val), B, N, M, ops._stream())
    assert rc == 0
    torch.cuda.synchronize()
    return bx.cpu().numpy().view(np.uint64), by.cpu().numpy().view(np.uint64), val.item()


@pytest.mark.parametrize("B,N,M,kind", [
    (1, 1, 1, "gauss"), (2, 17, 63, "gauss"), (1, 64, 65, "gauss"), (3, 300, 257, "gauss"),
    (1, 1500, 2300, "dups"), (2, 4096, 4096, "surface"), (1, 4097, 700, "surface"),
    (1, 16384, 16384, "surface"), (1, 2000, 1800, "flat"), (1, 500, 400, "point")])
def test_chamfer_tree_equals_brute_force(L, oracle, B, N, M, kind):
    """The sorted-cloud / sphere-tree Chamfer (rrl_chamfer_tree_fwd) against the brute-force kernel and
    the CPU oracle: every u64 key (distance bits, first-occurrence argmin) identical, the mean equal
    to double rounding -- over ragged sizes at every tile boundary, both sort paths (<= 4096 and the
    wide sort), duplicated points (ties), flat and single-point clouds."""
    from rrl_hip import synth
    rng = np.random.default_rng(100 + N + M)
    if kind == "surface":
        prs = [synth.make_pair(40 + b, N, M) for b in range(B)]
        x, y = np.stack([p["src"] for p in prs]), np.stack([p["tar"] for p in prs])
    else:
        x = rng.standard_normal((B, N, 3)).astype(np.float32)
        y = rng.standard_normal((B, M, 3)).astype(np.float32)
        if kind == "dups":
            y[0, 7] = y[0, 3]
            y[0, 1000:1100] = y[0, 50:150]      # 100 duplicated targets: the first occurrence must win
            x[0, 200:260] = x[0, 0:60]
        if kind == "flat":
            x[..., 2] = 0.5
            y[..., 1] = -0.25
        if kind == "point":
            y[:] = y[:, :1]                       # every target is the same point: argmin 0 everywhere
    tx, ty, tv = _chamfer_keys(x, y, True)
    bx, by, bv = _chamfer_keys(x, y, False)
    np.testing.assert_array_equal(tx, bx)
    np.testing.assert_array_equal(ty, by)
    assert abs(tv - bv) <= 2e-7 * abs(bv)
    if N * M <= 4096 * 4096:
        for b in range(B):
            mx, ax, my, ay = oracle.chamfer_parts(x[b], y[b])
            np.testing.assert_array_equal((tx[b] >> np.uint64(32)).astype(np.uint32).view(np.float32), mx)
            np.testing.assert_array_equal((tx[b] & np.uint64(0xffffffff)).astype(np.int32), ax)
            np.testing.assert_array_equal((ty[b] >> np.uint64(32)).astype(np.uint32).view(np.float32), my)
            np.testing.assert_array_equal((ty[b] & np.uint64(0xffffffff)).astype(np.int32), ay)
    if kind == "point":
        assert np.all((tx & np.uint64(0xffffffff)) == 0)


def test_chamfer_counters(L):
    """rrl_chamfer_counters: the instrumented walk writes one row per wavefront; same value as the plain one."""
    from rrl_hip import ops, synth
    prs = [synth.make_pair(90 + b, 1000, 700) for b in range(2)]
    x, y = cu(np.stack([p["src"] for p in prs])), cu(np.stack([p["tar"] for p in prs]))
    plain = float(ops.chamfer(x, y))
    ops.chamfer_counters(True)
    try:
        counted = float(ops.chamfer(x, y))
        torch.cuda.synchronize()
    finally:
        c = ops.chamfer_counters(False)
    assert counted == plain and ops.chamfer_counters(False) is None
    c = c.cpu().numpy()
    nsg = (1000 + 63) // 64 + (700 + 63) // 64        # query patches of both directions, per sample
    assert c[4] == 2 * nsg * 8                           # 8 wavefronts per patch
    assert 0 < c[3] <= 2 * 2 * 1000 * 700                # (query, target) pairs evaluated <= dense, both directions
    assert float(ops.chamfer(x, y)) == plain


def test_chamfer_nan_propagates(L):
    """torch.min propagates NaN: a NaN coordinate in a target cloud makes every minimum of that sample
    (and the batch mean) NaN, a NaN query only its own (code/loss.py:236-252 with torch semantics)."""
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 200, 3)).astype(np.float32)
    y = rng.standard_normal((2, 150, 3)).astype(np.float32)
    x[1, 17, 1] = np.nan
    tx, ty, tv = _chamfer_keys(x, y, True)
    dx = (tx >> np.uint64(32)).astype(np.uint32).view(np.float32)
    dy = (ty >> np.uint64(32)).astype(np.uint32).view(np.float32)
    assert np.isnan(dx[1, 17]) and np.isfinite(np.delete(dx[1], 17)).all() and np.isfinite(dx[0]).all()
    assert np.isnan(dy[1]).all() and np.isfinite(dy[0]).all()   # sample 1's targets (dir 1) contain the NaN
    assert np.isnan(tv)
    ref = torch.from_numpy
    want = torch.cat([((ref(x)[:, :, None] - ref(y)[:, None]) ** 2).sum(-1).min(2)[0].reshape(-1),
                      ((ref(x)[:, :, None] - ref(y)[:, None]) ** 2).sum(-1).min(1)[0].reshape(-1)])
    np.testing.assert_array_equal(np.isnan(np.concatenate([dx.reshape(-1), dy.reshape(-1)])), torch.isnan(want).numpy())


@pytest.mark.parametrize("B,N,M,Ll", [(2, 1024, 700, 3000), (8, 4096, 4096, 2000), (1, 5000, 4100, 1500), (1, 65, 64, 300)])
def test_chamfer_from_state_equals_chamfer_of_first_points(L, B, N, M, Ll):
    """rrl_chamfer_from_loss (no second sort: the loss workspace's sorted records, index arrays and
    sphere trees) against the brute-force kernel on (P0 of cloud 1, P0 of cloud 2): every u64 key
    identical, for the plain loss, the fused op (cloud 1 = the MOVED source) and an evaluation whose
    target was carried over from an earlier one (its records live in that workspace)."""
    from rrl_hip import ops, synth
    prs = [synth.make_pair(70 + b, N, M) for b in range(B)]
    src = cu(np.stack([p["src_tri"] for p in prs]))
    tar = cu(np.stack([p["tar_tri"] for p in prs]))
    torch.manual_seed(5)
    ln = torch.randn(B, Ll, 6, device="cuda")
    ln[..., :3] = torch.nn.functional.normalize(ln[..., :3], dim=-1)
    ln[..., 3:] *= 0.3

    def check(st, p0_src, p0_tar):
        val, bx, by = ops.chamfer_from_state(st, keys=True)
        wx, wy, wv = _chamfer_keys(p0_src.cpu().numpy(), p0_tar.cpu().numpy(), False)
        np.testing.assert_array_equal(bx.cpu().numpy().view(np.uint64), wx)
        np.testing.assert_array_equal(by.cpu().numpy().view(np.uint64), wy)
        assert abs(val.item() - wv) <= 2e-7 * abs(wv)

    st = ops.loss_forward_raw(src, tar, ln)
    check(st, src[..., :3].contiguous(), tar[..., :3].contiguous())
    # fused op: a rotation about z and a shift per sample
    ang = torch.linspace(0.1, 0.6, B, device="cuda")
    R = torch.zeros(B, 3, 3, device="cuda")
    R[:, 0, 0] = R[:, 1, 1] = torch.cos(ang); R[:, 0, 1] = -torch.sin(ang); R[:, 1, 0] = torch.sin(ang); R[:, 2, 2] = 1
    t = torch.full((B, 3), 0.05, device="cuda")
    _, _, _ = ops.registration_loss(src, R, t, tar, ln)
    first = ops.last_state()
    moved = first.tri1t[..., :3].contiguous()
    np.testing.assert_array_equal(moved.cpu().numpy(),
                                  ops.rigid_apply(src[..., :3].contiguous(), R, t, transpose_r=True).cpu().numpy())
    check(first, moved, tar[..., :3].contiguous())
    # a second pose against the same target and lines: the target's records stay in `first`'s workspace
    _, _, _ = ops.registration_loss(src, R.transpose(1, 2).contiguous(), -t, tar, ln, target_from=first)
    second = ops.last_state()
    assert second is not first and second.target_state is first
    check(second, second.tri1t[..., :3].contiguous(), tar[..., :3].contiguous())


# ---------------------------------------------------------------------------------- K6 + R
def test_reconstruction_point(L):
    g = load_golden("reconstruction_point.npz")
    rec = L.Reconstruction_point()
    assert list(rec.state_dict().keys()) == ["parameters_"]
    with torch.no_grad():
        rec.parameters_.copy_(torch.from_numpy(g["xi"]))
    rec = rec.cuda()
    pts, tri = rec(cu(g["src"]), cu(g["src_tri"]).reshape(1, -1, 3))
    assert pts.shape == g["out_pts"].shape and tri.shape == g["out_tri"].shape
    np.testing.assert_allclose(pts.detach().cpu().numpy(), g["out_pts"], atol=2e-6)
    np.testing.assert_allclose(tri.detach().cpu().numpy(), g["out_tri"], atol=2e-6)
    ((pts * cu(g["g_pts"])).sum() + (tri * cu(g["g_tri"])).sum()).backward()
    np.testing.assert_allclose(rec.parameters_.grad.cpu().numpy(), g["grad_xi"], rtol=2e-4,
                               atol=2e-4)


def test_se3_exp_kernel_vs_host_lie_algebra(L):
    """rrl_se3_exp / rrl_se3_exp_bwd against the host LieAlgebra package (itself pinned to the
    reference by tests/golden/se3_exp_log.npz): values and the gradient of a random contraction,
    across the Taylor boundary |w| = 0.01 and at w = 0."""
    from LieAlgebra import se3
    from rrl_hip import ops
    gen = torch.Generator().manual_seed(5)
    dirs = torch.randn(7, 3, generator=gen)
    dirs = dirs / dirs.norm(dim=1, keepdim=True)
    mags = torch.tensor([0.0, 1e-4, 0.0099, 0.0101, 0.5, 3.1, 1e-3]).reshape(-1, 1)
    xi = torch.cat([dirs * mags, torch.randn(7, 3, generator=gen)], dim=1)
    cR, cT = torch.randn(7, 3, 3, generator=gen), torch.randn(7, 3, generator=gen)
    xh = xi.clone().requires_grad_(True)
    Rh, Th = se3.exp3(xh)
    ((Rh * cR).sum() + (Th * cT).sum()).backward()
    xg = xi.clone().cuda().requires_grad_(True)
    Rg, Tg = ops.se3_exp(xg)
    ((Rg * cR.cuda()).sum() + (Tg * cT.cuda()).sum()).backward()
    np.testing.assert_allclose(Rg.detach().cpu().numpy(), Rh.detach().numpy(), rtol=0, atol=3e-7)
    np.testing.assert_allclose(Tg.detach().cpu().numpy(), Th.detach().numpy(), rtol=2e-6, atol=3e-7)
    np.testing.assert_allclose(xg.grad.cpu().numpy(), xh.grad.numpy(), rtol=2e-5, atol=2e-6)
    # a single twist of shape (6,), only T used (gR is None in the backward)
    x1 = xi[4].clone().cuda().requires_grad_(True)
    R1, T1 = ops.se3_exp(x1)
    T1.sum().backward()
    x1h = xi[4].clone().requires_grad_(True)
    se3.exp3(x1h)[1].sum().backward()
    np.testing.assert_allclose(x1.grad.cpu().numpy(), x1h.grad.numpy(), rtol=2e-5, atol=2e-6)


def test_adam_gated_kernel_vs_torch_adam(L):
    """rrl_adam_gated against torch.optim.Adam(lr, betas 0.9/0.999, eps 1e-8) over 30 steps with a
    learning-rate change, skipping the steps whose gate is 0 (the demo's `loss_di is None`)."""
    from rrl_hip import ops
    gen = torch.Generator().manual_seed(3)
    p0 = torch.randn(6, generator=gen)
    ref = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([ref], lr=2e-2)
    p = p0.clone().cuda()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    state, lr = torch.zeros(1, device="cuda"), torch.full((1,), 2e-2, device="cuda")
    for it in range(30):
        g = torch.randn(6, generator=gen) * (0.1 + it)
        gate = 0 if it in (3, 4, 17) else 2
        if it == 10:
            opt.param_groups[0]["lr"] = 1e-2
            lr.fill_(1e-2)
        if gate:
            ref.grad = g.clone()
            opt.step()
        ops.adam_gated(p, g.cuda(), m, v, state, lr, torch.tensor([gate, 0, 0, 0], dtype=torch.int32, device="cuda"))
        # round 4: the kernel follows torch's evaluation (double bias corrections, float(1 - beta) weights): a few ulps
        # (round 3 allowed 2e-5: 1 - 0.999^t in fp32 is 3e-5 off at small t)
        np.testing.assert_allclose(p.cpu().numpy(), ref.detach().numpy(), rtol=1e-6, atol=2e-8)
    assert float(state[0]) == 27.0


def test_pose_step_in_one_launch_equals_the_four(L):
    """rrl_se3_adam_step == rrl_se3_exp_bwd, rrl_adam_gated, rrl_se3_exp (of the updated xi), rrl_log_row, bit for
    bit over 12 steps with empty (gated-off) steps in between; rrl_rigid_apply_aabb == rigid apply + rrl_aabb."""
    from rrl_hip import ops
    P = ops._p
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(11)
    xi0 = torch.cat([torch.randn(3, generator=gen) * 0.004, torch.randn(3, generator=gen) * 0.1])
    mk = lambda: dict(xi=xi0.clone().cuda(), m=torch.zeros(6, device=dev), v=torch.zeros(6, device=dev),
                      st=torch.zeros(1, device=dev), R=torch.empty(1, 3, 3, device=dev), T=torch.empty(1, 3, device=dev),
                      table=torch.zeros(12, 3, device=dev), cur=torch.zeros(1, dtype=torch.long, device=dev),
                      row=torch.zeros(3, device=dev))
    a, b = mk(), mk()
    lr = torch.full((1,), 2e-2, device=dev)
    gx_a, gx_b = torch.empty(1, 6, device=dev), torch.empty(6, device=dev)
    for it in range(12):
        gR, gT = torch.randn(1, 3, 3, generator=gen).cuda(), torch.randn(1, 3, generator=gen).cuda()
        loss, val = torch.rand(1, generator=gen).cuda(), torch.rand(1, generator=gen).cuda()
        gate = torch.tensor([0 if it in (2, 7) else 5, 0, 0, 0], dtype=torch.int32, device=dev)
        if it == 6:
            lr.fill_(1e-2)
        ops._run(dev, "rrl_se3_exp_bwd", P(a["xi"]), P(gR), P(gT), P(gx_a), 1)
        ops.adam_gated(a["xi"], gx_a.view(-1), a["m"], a["v"], a["st"], lr, gate)
        ops._run(dev, "rrl_se3_exp", P(a["xi"]), P(a["R"]), P(a["T"]), 1)
        ops.log_row(loss, val, gate, a["table"], a["cur"], a["row"])
        ops.se3_adam_step(b["xi"], gR, gT, b["m"], b["v"], b["st"], lr, gate, b["R"], b["T"], gxi=gx_b, loss=loss,
                          value=val, table=b["table"], cursor=b["cur"], row=b["row"])
        assert torch.equal(gx_a.view(-1), gx_b)
        for k in a:
            assert torch.equal(a[k], b[k]), (it, k)
    assert float(a["st"][0]) == 10.0 and int(a["cur"][0]) == 12 and not torch.equal(a["xi"].cpu(), xi0)
    x = torch.randn(2, 3000, 3, generator=gen).cuda()
    R = torch.linalg.qr(torch.randn(2, 3, 3, generator=gen))[0].cuda()
    t = torch.randn(2, 3, generator=gen).cuda()
    y0, y1, box = torch.empty_like(x), torch.empty_like(x), torch.empty(2, 6, device=dev)
    ops.rigid_apply_into(x, R, t, y0)
    ops.rigid_apply_aabb_into(x, R, t, y1, box)
    assert torch.equal(y0, y1) and torch.equal(box, ops.aabb(y0))
    assert torch.equal(box, torch.cat([y0.amin(1), y0.amax(1)], dim=1))


@pytest.mark.parametrize("transpose_r", [False, True])
@pytest.mark.parametrize("channel_first", [False, True])
def test_rigid_apply_layouts(L, transpose_r, channel_first):
    from rrl_hip import ops
    gen = torch.Generator().manual_seed(3)
    B, n = 3, 1000
    x = torch.randn(B, n, 3, generator=gen, dtype=torch.float64)
    R = torch.linalg.qr(torch.randn(B, 3, 3, generator=gen, dtype=torch.float64))[0]
    t = torch.randn(B, 3, generator=gen, dtype=torch.float64)
    gy = torch.randn(B, n, 3, generator=gen, dtype=torch.float64)
    xr, Rr, tr = (v.clone().requires_grad_(True) for v in (x, R, t))
    yr = xr @ (Rr.transpose(1, 2) if transpose_r else Rr) + tr[:, None, :]
    (yr * gy).sum().backward()
    xin = x.float().cuda()
    gin = gy.float().cuda()
    if channel_first:
        xin, gin = xin.transpose(1, 2).contiguous(), gin.transpose(1, 2).contiguous()
    xin.requires_grad_(True)
    Rg, tg = R.float().cuda().requires_grad_(True), t.float().cuda().requires_grad_(True)
    y = ops.rigid_apply(xin, Rg, tg, transpose_r=transpose_r, channel_first=channel_first)
    (y * gin).sum().backward()
    yy = y.transpose(1, 2) if channel_first else y
    gxx = xin.grad.transpose(1, 2) if channel_first else xin.grad
    np.testing.assert_allclose(yy.detach().cpu().numpy(), yr.detach().numpy(), atol=2e-6)
    np.testing.assert_allclose(gxx.cpu().numpy(), xr.grad.numpy(), atol=2e-6)
    np.testing.assert_allclose(Rg.grad.cpu().numpy(), Rr.grad.numpy(), rtol=1e-4, atol=1e-3)
    np.testing.assert_allclose(tg.grad.cpu().numpy(), tr.grad.numpy(), rtol=1e-4, atol=1e-3)


def test_utils_transform_point_cloud(L):
    import utils
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(2, 3, 500, generator=gen)
    R = torch.linalg.qr(torch.randn(2, 3, 3, generator=gen))[0]
    t = torch.randn(2, 3, generator=gen)
    y = utils.transform_point_cloud(x.cuda(), R.cuda(), t.cuda())
    ref = torch.matmul(R.double(), x.double()) + t.double().unsqueeze(2)
    np.testing.assert_allclose(y.cpu().numpy(), ref.numpy(), atol=2e-6)


# ---------------------------------------------------------------------------------- K8
def test_sampler(L, oracle):
    g = load_golden("sampler.npz")
    n = g["cand0"].shape[0]
    torch.manual_seed(int(g["seed"]))
    cand = L.Random_uniform_distribution_lines_batch_efficient(
        torch.tensor([[float(g["radius"])]]), torch.from_numpy(g["center"]).reshape(1, 3), n, "cuda")
    np.testing.assert_allclose(cand[0].cpu().numpy(), g["cand0"], atol=2e-5)
    np.testing.assert_array_equal(L.generate_bbox(cu(g["src"])[None])[0].numpy(), g["bbox1"])
    torch.manual_seed(int(g["seed"]))
    final = L.Random_uniform_distribution_lines_batch_efficient_resample(
        torch.tensor([[float(g["radius"])]]), torch.from_numpy(g["center"]).reshape(1, 3), n,
        cu(g["src"])[None], cu(g["tar"])[None], "cuda")[0].cpu().numpy()
    assert final.shape == (n, 6)
    mine = oracle.resample_lines(g["rands"], g["radius"], g["center"], g["src"], g["tar"], n)
    # same candidates in the same order as the oracle wherever both accepted the same set
    nf = int((np.abs(final).sum(1) > 0).sum())
    nm = int((np.abs(mine).sum(1) > 0).sum())
    nr = int((np.abs(g["final"]).sum(1) > 0).sum())
    assert abs(nf - nm) <= 20 and abs(nf - nr) <= 40
    d = np.linalg.norm(final[:nf, :3], axis=1)
    np.testing.assert_allclose(d, 1.0, atol=1e-5)  # unit directions
    # every kept line is one of the candidates, in candidate order
    torch.manual_seed(int(g["seed"]))
    big = L.Random_uniform_distribution_lines_batch_efficient_resample(
        torch.tensor([[4 * float(g["radius"])]]), torch.from_numpy(g["center"]).reshape(1, 3), n,
        cu(g["src"])[None], cu(g["tar"])[None], "cuda")[0].cpu().numpy()
    nb = int((np.abs(big).sum(1) > 0).sum())
    assert 0 < nb < n and not np.any(big[nb:])  # unfilled rows stay zero at the tail
    assert abs(nb - int((np.abs(g["final_big"]).sum(1) > 0).sum())) <= 15


def _align_rows(A, Bm, tol, look=6):
    """Greedy alignment of two row sequences that are the SAME candidate stream filtered by two accept masks that may disagree on
    a few knife-edge candidates: returns (matched pairs, rows only in A, rows only in B, largest difference of a matched pair)."""
    i = j = 0
    matched, only_a, only_b, worst = 0, 0, 0, 0.0
    same = lambda x, y: float(np.abs(x - y).max()) <= tol  # noqa: E731
    while i < len(A) and j < len(Bm):
        if same(A[i], Bm[j]):
            worst = max(worst, float(np.abs(A[i] - Bm[j]).max()))
            matched += 1; i += 1; j += 1
            continue
        da = next((d for d in range(1, look + 1) if i + d < len(A) and same(A[i + d], Bm[j])), None)
        db = next((d for d in range(1, look + 1) if j + d < len(Bm) and same(A[i], Bm[j + d])), None)
        if da is not None and (db is None or da <= db):
            only_a += da; i += da
        elif db is not None:
            only_b += db; j += db
        else:
            only_a += 1; only_b += 1; i += 1; j += 1
    return matched, only_a, only_b, worst


def test_sampler_rows_vs_reference(L, oracle):
    """not the NUMBER of filled rows but the ROWS.  For the reference's seed the GPU buffer and the
    reference's `final` (code/loss.py:365-381, 415-432; tests/golden/sampler.npz) are the same candidate stream -- ten rounds
    of candidates in index order -- filtered by the accept test.  That test (code/loss.py:303-312) keeps a box triangle when
    A + B + C <= S for the three sub-areas around the crossing point -- an EQUALITY in exact arithmetic for every true crossing, so
    the decision of a crossing is the rounding of those four numbers: bit-equal for bit-equal candidates
    (test_box_accept_bit_exact pins the reference's decisions), a coin flip under a 1e-7 change of the candidate.  The two
    generators' candidates differ by ~1e-7 (sin / cos / sqrt of different libraries), so the two accepted streams are aligned row
    by row: every row BOTH kept agrees to 2e-5 (measured 1.2e-7), and the candidates only one of them kept are counted and
    bounded (measured: 364 of 400 rows matched, 32 + 36 kept by one side only; printed).  The same against the oracle (same
    uniforms, CPU libm)."""
    g = load_golden("sampler.npz")
    n = g["cand0"].shape[0]
    res = {}
    for name, radius in (("final", float(g["radius"])), ("final_big", 4 * float(g["radius"]))):
        torch.manual_seed(int(g["seed"]))
        mine = L.Random_uniform_distribution_lines_batch_efficient_resample(
            torch.tensor([[radius]]), torch.from_numpy(g["center"]).reshape(1, 3), n, cu(g["src"])[None], cu(g["tar"])[None],
            "cuda")[0].cpu().numpy()
        ref = g[name]
        nm, nr = int((np.abs(mine).sum(1) > 0).sum()), int((np.abs(ref).sum(1) > 0).sum())
        assert not np.any(mine[nm:]) and not np.any(ref[nr:])
        matched, only_mine, only_ref, worst = _align_rows(mine[:nm], ref[:nr], 2e-5 * max(1.0, radius))
        res[name] = (nm, nr, matched, only_mine, only_ref, worst)
        print(f"sampler rows [{name}]: filled {nm} (reference {nr}), matched {matched}, only here {only_mine}, only in the reference {only_ref}, "
              f"largest difference of a matched row {worst:.2e}")
        # every row but the knife-edge ones is the reference's row; a full buffer drops the stream's tail, so a disagreement
        # early in the stream also costs the rows it pushes past the end
        assert worst <= 2e-5 * max(1.0, radius)
        assert only_mine + only_ref <= 0.25 * max(nm, nr, 1) + 4, res[name]
        assert matched >= 0.85 * min(nm, nr) - 4, res[name]
    # the oracle on the fixture's uniforms (pinned to the reference's decisions) against the reference's rows
    orc = oracle.resample_lines(g["rands"], g["radius"], g["center"], g["src"], g["tar"], n)
    no = int((np.abs(orc).sum(1) > 0).sum())
    m2, a2, b2, w2 = _align_rows(orc[:no], g["final"][:int((np.abs(g["final"]).sum(1) > 0).sum())], 2e-5)
    print(f"sampler rows [oracle vs reference]: matched {m2}, only oracle {a2}, only reference {b2}, worst {w2:.2e}")
    assert a2 + b2 <= 0.25 * no + 4


def test_sampler_library_generator(L):
    """device_rng=True: the uniforms come from the library's counter-based generator INSIDE the sampler kernels
    (rrl_sample_lines_rng): unit directions on chords of the sphere, the accept test still applied (every filled row
    passes rrl_box_accept), a fresh stream per call, the same stream after re-seeding, and -- captured in a graph --
    a fresh stream per REPLAY (the call counter lives on the device)."""
    from rrl_hip import ops, synth
    from rrl_hip.graph import GraphedStep
    pr = synth.make_pair(3, 800, 700)
    src, tar = cu(pr["src"])[None], cu(pr["tar"])[None]
    r = torch.tensor([[float(pr["radius"])]])
    c = torch.from_numpy(pr["center"]).reshape(1, 3)
    n = 5000

    def draw(out=None):
        return L.Random_uniform_distribution_lines_batch_efficient_resample(r, c, n, src, tar, "cuda", device_rng=True, out=out)
    ops.sampler_rng(seed=1234)
    a, b_ = draw().clone(), draw().clone()
    ops.sampler_rng(seed=1234)
    a2 = draw().clone()
    assert torch.equal(a, a2) and not torch.equal(a, b_)
    for ln in (a, b_):
        filled = ln[0].abs().sum(1) > 0
        assert int(filled.sum()) > 0.5 * n
        d = ln[0][filled, :3]
        np.testing.assert_allclose(d.norm(dim=1).cpu().numpy(), 1.0, atol=2e-6)
        x0 = ln[0][filled, 3:] - c.cuda()
        np.testing.assert_allclose(x0.norm(dim=1).cpu().numpy(), float(pr["radius"]), rtol=1e-5)
        mask, _ = ops.box_accept(ln, ops.aabb(src), ops.aabb(tar))
        assert bool(((mask[0][filled] & 3) == 3).all())
    # all candidates of one round, no boxes: uniform on the sphere (mean offset ~ 0, second moments ~ r^2 / 3)
    allc = L.Random_uniform_distribution_lines_batch_efficient(r, c, 200000, "cuda", device_rng=True)
    x0 = (allc[0, :, 3:] - c.cuda()) / float(pr["radius"])
    assert float(x0.mean(0).abs().max()) < 0.01 and float(((x0 ** 2).mean(0) - 1 / 3).abs().max()) < 0.01
    # captured: every replay draws the next block
    buf = torch.empty(1, n, 6, device="cuda")
    rg, cg, box2 = r.cuda(), c.cuda(), ops.aabb(tar)  # (a captured step works on GPU-resident arguments)
    g = GraphedStep(lambda: L.Random_uniform_distribution_lines_batch_efficient_resample(
        rg, cg, n, src, tar, "cuda", device_rng=True, out=buf, box2=box2))
    g(); first = buf.clone()
    g(); second = buf.clone()
    assert not torch.equal(first, second)
    # seeding follows torch's SEED without touching torch's generator (round 4): a new torch seed starts a new
    # stream, the same seed after a re-seed reproduces it, other GPU draws in between neither re-seed the sampler nor are
    # they shifted by it (torch's offset is never moved), and successive calls differ
    gen = torch.cuda.default_generators[torch.cuda.current_device()]
    torch.manual_seed(7)
    off0 = gen.get_offset()
    m1 = draw().clone()
    assert gen.get_offset() == off0  # the sampler left torch's generator where it was
    torch.rand(1000, device="cuda")  # somebody else draws on the GPU (dropout, rand ...): no re-seed, the stream goes on
    m1b = draw().clone()
    torch.manual_seed(8)
    m3 = draw().clone()
    torch.manual_seed(7)             # seen: the seed changed
    m2 = draw().clone()
    torch.rand(1000, device="cuda")
    m2b = draw().clone()
    torch.manual_seed(7)             # seen: same seed, but torch's offset went backwards
    m4 = draw().clone()
    assert torch.equal(m1, m2) and torch.equal(m1b, m2b) and torch.equal(m1, m4)
    assert not torch.equal(m1, m1b) and not torch.equal(m1, a) and not torch.equal(m1, m3)
    ops.sampler_rng(seed=99)         # explicit
    e1 = draw().clone()
    ops.sampler_rng(seed=99)
    assert torch.equal(e1, draw())


def test_box_accept_bit_exact(L, oracle):
    """Row F pinned: on IDENTICAL candidate lines the HIP accept test (rrl_box_accept: the sampler's own
    face table / face_hit / slab pre-test) gives the reference's per-box hit counts bit for bit --
    on the sampler fixture's cand0 and on the five candidate sets of accept.npz (regular, flat,
    single-point, far-from-origin, demo-scale boxes; label1 / label2 of code/loss.py:427-428 computed
    by the reference itself) -- and equals the CPU oracle on 10^5 random lines per box pair.  The
    slab pre-test never rejects a line the exact test accepts."""
    from rrl_hip import ops

    def gpu(v1, v2, lines):
        m, h = ops.box_accept(cu(lines)[None], ops.aabb(cu(v1)[None]), ops.aabb(cu(v2)[None]))
        return m[0].cpu().numpy(), h[0].cpu().numpy()
    g = load_golden("sampler.npz")
    m, h = gpu(g["src"], g["tar"], g["cand0"])
    np.testing.assert_array_equal(h[:, 0], g["hits1"])
    np.testing.assert_array_equal(h[:, 1], g["hits2"])
    a = load_golden("accept.npz")
    total = 0
    for tag in a["cases"]:
        m, h = gpu(a[f"{tag}_v1"], a[f"{tag}_v2"], a[f"{tag}_cand"])
        np.testing.assert_array_equal(h[:, 0], a[f"{tag}_hits1"])
        np.testing.assert_array_equal(h[:, 1], a[f"{tag}_hits2"])
        acc = (m & 3) == 3
        np.testing.assert_array_equal(acc, (a[f"{tag}_hits1"] * a[f"{tag}_hits2"]) > 0)
        assert np.all((m[acc] & 4) == 4)  # accepted => the pre-test let it through
        total += int(acc.sum())
    assert total > 1500
    # 10^5 random chords per box pair against the oracle (no reference needed on the GPU box)
    rng = np.random.default_rng(17)
    pr_src = a["regular_v1"]
    boxes = [(pr_src, a["regular_v2"], 1.0, np.zeros(3)), (a["flat_v1"], a["regular_v2"], 1.0, np.zeros(3)),
             (a["single_v1"], a["regular_v2"], 0.6, np.zeros(3)),
             (a["far_v1"], a["far_v2"], 1.0, np.array([40.0, -25.0, 17.0]))]
    for v1, v2, rad, ctr in boxes:
        n = 100000
        p = rng.standard_normal((2, n, 3))
        p /= np.linalg.norm(p, axis=2, keepdims=True)
        q1, q2 = (rad * 1.3 * p[0] + ctr).astype(np.float32), (rad * 1.3 * p[1] + ctr).astype(np.float32)
        d = (q2 - q1).astype(np.float64)
        lines = np.concatenate([(d / np.linalg.norm(d, axis=1, keepdims=True)), q1], 1).astype(np.float32)
        m, h = gpu(v1, v2, lines)
        np.testing.assert_array_equal(h[:, 0], oracle.box_hits(oracle.bbox(v1), lines))
        np.testing.assert_array_equal(h[:, 1], oracle.box_hits(oracle.bbox(v2), lines))
        acc = (m & 3) == 3
        assert np.all((m[acc] & 4) == 4)


def test_resample_is_accept_of_own_candidates(L):
    """The 10-round resampler end to end: its output buffer equals, bit for bit, what the reference's
    fill rule (code/loss.py:365-381: candidate order, `counter > N` skips the round, truncation,
    zero tail) produces from the SAME kernel's unfiltered candidates and the pinned accept test."""
    from rrl_hip import ops, synth
    # (the last two: 108 tiles x 10 rounds -- more tile counts than the write pass's workgroup scans at once --, once with
    # the usual fill and once with a small sphere that fills the buffer early, so that rounds are skipped)
    for seed, n, scale in ((5, 3000, 1.0), (6, 1200, 0.5), (7, 700, 4.0), (8, 110000, 1.0), (9, 110000, 0.45)):
        pr = synth.make_pair(seed, 400, 350)
        rands = torch.from_numpy(synth.uniform_streams(seed, 10, n))[:, :, None, :]
        r, c = torch.tensor([pr["radius"] * scale]), torch.from_numpy(pr["center"])[None]
        b1, b2 = ops.aabb(cu(pr["src"])[None]), ops.aabb(cu(pr["tar"])[None])
        final, filled = ops.sample_lines(rands, r, c, b1, b2)
        final = final[0].cpu().numpy()
        want = np.zeros((n, 6), np.float32)
        count = 0
        for rd in range(10):
            cand, _ = ops.sample_lines(rands[rd:rd + 1], r, c, None, None)  # every candidate of the round
            m, _ = ops.box_accept(cand, b1, b2)
            keep = cand[0].cpu().numpy()[((m[0] & 3) == 3).cpu().numpy()]
            if count > n:
                continue
            take = keep[:max(0, n - count)]
            want[count:count + len(take)] = take
            count += len(keep)
        np.testing.assert_array_equal(final, want)
        assert int(filled[0]) == count


def test_sampler_prefilter_is_exact(tmp_path):
    """The conservative slab pre-test of the sampler's count pass never changes the result: the
    same lines bit-for-bit with RRL_SAMPLER_PREFILTER=0 (every candidate through the exact test),
    over regular, flat, single-point and far-from-origin boxes at several radii."""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    outs = []
    for flag in ("1", "0"):
        path = str(tmp_path / f"s{flag}.npz")
        env = dict(os.environ, RRL_SAMPLER_PREFILTER=flag)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "sampler_check.py"), path],
                           capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
        outs.append(np.load(path))
    assert sorted(outs[0].files) == sorted(outs[1].files) and len(outs[0].files) == 24
    filled = 0
    for name in outs[0].files:
        np.testing.assert_array_equal(outs[0][name], outs[1][name])
        filled += int((np.abs(outs[0][name]).sum(1) > 0).sum())
    assert filled > 10000  # the cases are not degenerate: lines were accepted


def test_cull_dense_hits(L, oracle):
    """Stress the culled scan's overflow paths: a tiny cloud hit by almost every line (every
    (line, group) pair survives the sphere test) must still match the strict scan and the oracle."""
    rng = np.random.default_rng(11)
    pts = rng.standard_normal((200, 3)).astype(np.float32)
    pts[:, 2] *= 0.02  # a small flat patch: long lines through it graze many pseudo-triangles
    from rrl_hip import synth
    tri = synth.knn_triangles(pts)
    n_lines = 700
    d = rng.standard_normal((n_lines, 3))
    d[:, 2] *= 0.01  # nearly in-plane directions
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    x0 = rng.standard_normal((n_lines, 3)) * 0.5
    x0[:, 2] *= 0.02
    lines = np.concatenate([d, x0], 1).astype(np.float32)
    c = run_state(tri, tri, lines, mode="cull")
    s_ = run_state(tri, tri, lines, mode="strict")
    o = oracle.scan(tri, lines, cap=4)
    np.testing.assert_array_equal(c.count1[0].cpu().numpy(), o["count"])
    np.testing.assert_array_equal(s_.count1[0].cpu().numpy(), o["count"])
    assert o["count"].max() > 4 and (o["count"] > 0).mean() > 0.5  # really dense


@pytest.mark.parametrize("scale", [1.0, 12.0, 40.0, 300.0, 5000.0])
@pytest.mark.parametrize("far", [False, True])
def test_cull_is_exact_at_any_scale(L, scale, far):
    """The culling bound carries a per-wavefront slack derived from (|x0| + max|P|)^2 instead of
    refusing to cull beyond a fixed scale: counts, hit lists and the loss equal the strict scan's
    bit for bit on clouds scaled up to 5000x (where the 2e-4 eps is far below the rounding noise of
    the reference's own arithmetic), with no wavefront taking the strict fallback; `far` moves the
    clouds away from the origin (large |a|, cancellation-heavy)."""
    from rrl_hip import synth
    pr = synth.make_pair(77, 1500, 1100)
    off = np.array([3.0, -2.0, 1.5] * 3, np.float32) * np.float32(scale) if far else np.float32(0)
    tri1 = pr["src_tri"] * np.float32(scale) + off
    tri2 = pr["tar_tri"] * np.float32(scale) + off
    rands = synth.uniform_streams(3, 10, 6000)
    ctr = pr["center"] * np.float32(scale) + (off[:3] if far else 0)
    from rrl_hip import ops
    lines, _ = ops.sample_lines(torch.from_numpy(rands)[:, :, None, :], torch.tensor([pr["radius"] * scale]),
                                torch.from_numpy(np.asarray(ctr, np.float32))[None],
                                ops.aabb(cu(tri1[None, :, :3])), ops.aabb(cu(tri2[None, :, :3])))
    ln = lines[0].cpu().numpy()
    c = run_state(tri1, tri2, ln, mode="cull")
    s_ = run_state(tri1, tri2, ln, mode="strict")
    # the NaN flag (the reference's print-and-exit, code/loss.py:88-91) equals the strict scan's at every scale:
    # beyond the provably NaN-free one the walk is widened by the triangles' NaN reach (rrl_cull.hip, "NaN")
    assert int(c.status[1]) == 0 and int(c.status[0]) == int(s_.status[0])
    if scale == 1.0:
        assert int(s_.status[0]) == 0
    for a, b in ((c.count1, s_.count1), (c.count2, s_.count2)):
        np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy())
    for cnt, hc, hs in ((c.count1, c.hit1, s_.hit1), (c.count2, c.hit2, s_.hit2)):
        k = cnt[0].cpu().numpy()
        hc, hs = hc[0].cpu().numpy(), hs[0].cpu().numpy()
        for l in np.nonzero((k > 0) & (k <= 4))[0]:
            assert sorted(hc[l, :k[l]].tolist()) == sorted(hs[l, :k[l]].tolist())
    assert c.loss[0].item() == s_.loss[0].item()
    assert int((c.count1 > 0).sum()) > 100  # not degenerate: lines do hit


@pytest.mark.parametrize("scale", [12.0, 300.0, 5000.0])
def test_cull_nan_detection_equals_strict(L, oracle, scale):
    """A negative sqrt argument at point 1 of a triangle that is NO point-0 candidate (its P0 sits far from the
    line, farther than thr and than the prefilter's slack): the reference flags a NaN on ANY pair
    (code/loss.py:88-91), the strict scan does, and the culled scan must too -- its walk is widened by every
    triangle's NaN reach max(|P1-P0|, |P2-P0|) - thr wherever a NaN is not provably impossible.  Constructed:
    64 triangles with P1 exactly on "their" line, P0 at 0.04 * scale from it (thr = 0.58 of that), P2 next to P0;
    beyond the provably NaN-free scale rounding decides the sign of |a|^2 - (a.d)^2 + 2e-4 for the on-line point."""
    from rrl_hip import synth, ops
    rng = np.random.default_rng(3)
    pr = synth.make_pair(78, 1200, 900)
    sc = np.float32(scale)
    tri1, tri2 = pr["src_tri"] * sc, pr["tar_tri"] * sc
    rands = synth.uniform_streams(5, 10, 3000)
    lines, _ = ops.sample_lines(torch.from_numpy(rands)[:, :, None, :], torch.tensor([pr["radius"] * scale]),
                                torch.from_numpy(np.asarray(pr["center"] * sc, np.float32))[None],
                                ops.aabb(cu(tri1[None, :, :3])), ops.aabb(cu(tri2[None, :, :3])))
    ln = lines[0].cpu().numpy()
    ln = ln[np.abs(ln).sum(1) > 0]
    ns = 64
    d = rng.standard_normal((ns, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    d = (d.astype(np.float64) / np.linalg.norm(d.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
    x0 = (rng.standard_normal((ns, 3)) * 0.7 * scale).astype(np.float32)
    t = rng.uniform(0.3, 0.9, (ns, 1)) * scale
    P1 = (x0.astype(np.float64) + t * d.astype(np.float64)).astype(np.float32)            # on the line, up to rounding
    nrm = np.cross(d.astype(np.float64), rng.standard_normal((ns, 3)))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    P0 = (P1.astype(np.float64) + 0.04 * scale * nrm).astype(np.float32)                  # far from the line: no hit
    P2 = (P0.astype(np.float64) + 0.0002 * scale * rng.standard_normal((ns, 3))).astype(np.float32)
    special = np.concatenate([P0, P1, P2], 1).astype(np.float32)
    tri1s = np.concatenate([tri1, special]).astype(np.float32)
    lns = np.concatenate([ln, np.concatenate([d, x0], 1)]).astype(np.float32)
    c = run_state(tri1s, tri2, lns, mode="cull")
    s_ = run_state(tri1s, tri2, lns, mode="strict")
    assert int(c.status[1]) == 0  # unit directions: nobody left the culled walk
    assert int(c.status[0]) == int(s_.status[0])
    assert bool(int(s_.status[0])) == (oracle.scan(tri1s, lns, cap=4)["nan"] or oracle.scan(tri2, lns, cap=4)["nan"])
    if scale >= 300.0:
        assert int(s_.status[0]) == 1  # the construction does produce negative arguments there
    np.testing.assert_array_equal(c.count1.cpu().numpy(), s_.count1.cpu().numpy())
    np.testing.assert_array_equal(c.count2.cpu().numpy(), s_.count2.cpu().numpy())
    # and the drop-in call raises like the reference exits
    if int(s_.status[0]):
        with pytest.raises(ValueError, match="NaN"):
            L.cal_loss_intersection_batch_whole_median_pts_lines(1, 1, 5, 5, cu(tri1s)[None], cu(tri2)[None], cu(lns)[None], "cuda")


def test_scan_counters(L):
    """rrl_scan_counters: the instrumented instantiation gives the same results and plausible
    executed-work counts (every level sees fewer pairs than the dense product)."""
    from rrl_hip import ops
    g = load_golden("loss_synth_s1.npz")
    plain = run_state(g["tri1"], g["tri2"], g["lines"], mode="cull")
    ops.scan_counters(True)
    try:
        counted = run_state(g["tri1"], g["tri2"], g["lines"], mode="cull")
    finally:
        c = ops.scan_counters(False).cpu().numpy()
    np.testing.assert_array_equal(plain.count1.cpu().numpy(), counted.count1.cpu().numpy())
    np.testing.assert_array_equal(plain.count2.cpu().numpy(), counted.count2.cpu().numpy())
    assert plain.loss[0].item() == counted.loss[0].item()
    nl, n1, n2 = g["lines"].shape[0], g["tri1"].shape[0], g["tri2"].shape[0]
    nsg = (n1 + 63) // 64 + (n2 + 63) // 64
    assert c[0] == nl * nsg                      # level A tests every (line, supergroup)
    # level B: 8 half spheres per surviving (line, supergroup) pair; level D: 8 records per surviving half
    assert 0 < c[1] <= 8 * c[0] and c[1] % 8 == 0 and 0 < c[2] <= c[1] and c[3] == 8 * c[2]
    assert c[3] < nl * (n1 + n2)                 # fewer exact tests than the dense scan's pairs
    assert c[4] >= int(g["count1"].sum() + g["count2"].sum())  # every hit was a resolved candidate
    assert c[6] == 0 and c[7] == 0 and c[5] > 0
    assert c[9] > c[8] > 0  # every wavefront's start / end on the wall clock (summed over the rows)


@pytest.mark.parametrize("n_lines,spread", [(3000, 0.0), (3000, 1e-4), (600, 0.0), (9000, 1e-5)])
def test_median_with_crowded_bins(L, oracle, n_lines, spread):
    """The median's radix select hands the values of one 11-bit bin to a single wavefront when
    there are at most 2048 of them and otherwise runs its workgroup-wide passes: thousands of
    (nearly) identical D values exercise both routes and the rank bookkeeping inside the bin."""
    rng = np.random.default_rng(5)
    base = np.array([[0.0, 0.0, 0.0, 0.05, 0.0, 0.0, 0.0, 0.05, 0.0]], np.float32)
    tri1 = np.concatenate([base, base + np.float32(3.0)]).astype(np.float32)          # second triangle far away
    tri2 = (tri1 + np.array([0.004, -0.003, 0.002] * 3, np.float32)).astype(np.float32)
    d = np.tile(np.array([[0.0, 0.0, 1.0]]), (n_lines, 1))
    x0 = np.tile(np.array([[0.012, 0.011, -1.0]]), (n_lines, 1)) + spread * rng.standard_normal((n_lines, 3))
    lines = np.concatenate([d, x0], 1).astype(np.float32)
    ref = oracle.loss(tri1, tri2, lines, want_grad=False)
    assert ref["n_selected"] > 0.9 * n_lines  # nearly every line is selected: > 2048 values in one bin for 3000+
    st = run_state(tri1, tri2, lines, mode="cull")
    np.testing.assert_array_equal(st.med.cpu().numpy().view(np.uint32), np.float32(ref["median"]).reshape(1).view(np.uint32))
    np.testing.assert_allclose(st.loss.cpu().numpy()[0], ref["loss"], rtol=1e-5)


@pytest.mark.parametrize("case", ["golden", "batch", "crowded3000", "crowded9000", "one_tile", "sparse_tiles"])
def test_tiled_reduce_equals_single_workgroup(L, case):
    """The tiled reduce (one workgroup per 1024-line tile, bin values exchanged through the workspace, device-atomic
    fixed-point bucket sums, last arriver writes the loss) against the single 1024-lane workgroup per sample:
    median, loss, info, bucket counts and bucket sums bit for bit -- on the fixtures, a batch, crowded bins (more
    than 2048 values in the median's bin: the streaming route; tiles with ~1000 selected lines: rows beyond the
    256 held in registers), a single tile and tiles without any selected line -- and a repeated reduce on the
    same prepared state."""
    from rrl_hip import ops, synth, _lib
    if case == "golden":
        g = load_golden("loss_demo_scale.npz")
        tri1, tri2, lines = g["tri1"][None], g["tri2"][None], g["lines"][None]
    elif case == "batch":
        prs = [synth.make_pair(300 + b, 1500, 1300) for b in range(5)]
        tri1, tri2 = np.stack([p["src_tri"] for p in prs]), np.stack([p["tar_tri"] for p in prs])
        ln = []
        for b, p in enumerate(prs):
            torch.manual_seed(b)
            ln.append(L.Random_uniform_distribution_lines_batch_efficient_resample(
                torch.tensor([[float(p["radius"])]]), torch.from_numpy(p["center"]).reshape(1, 3), 5000,
                cu(p["src"])[None], cu(p["tar"])[None], "cuda")[0].cpu().numpy())
        lines = np.stack(ln)
        lines[4, 1024:] = 0  # sample 4: every tile but the first is empty (zero lines hit nothing here)
    elif case in ("crowded3000", "crowded9000", "one_tile"):
        n_lines = {"crowded3000": 3000, "crowded9000": 9000, "one_tile": 700}[case]
        rng = np.random.default_rng(5)
        base = np.array([[0.0, 0.0, 0.0, 0.05, 0.0, 0.0, 0.0, 0.05, 0.0]], np.float32)
        tri1 = np.concatenate([base, base + np.float32(3.0)]).astype(np.float32)[None]
        tri2 = (tri1 + np.array([0.004, -0.003, 0.002] * 3, np.float32)).astype(np.float32)
        d = np.tile(np.array([[0.0, 0.0, 1.0]]), (n_lines, 1))
        x0 = np.tile(np.array([[0.012, 0.011, -1.0]]), (n_lines, 1)) + (1e-5 if case == "crowded9000" else 0.0) * rng.standard_normal((n_lines, 3))
        lines = np.concatenate([d, x0], 1).astype(np.float32)[None]
    else:  # sparse_tiles: 6000 lines of which only a handful hit both clouds, spread over the tiles
        pr = synth.make_pair(9, 400, 300)
        tri1, tri2 = pr["src_tri"][None], pr["tar_tri"][None]
        torch.manual_seed(1)
        lines = L.Random_uniform_distribution_lines_batch_efficient_resample(
            torch.tensor([[float(pr["radius"])]]), torch.from_numpy(pr["center"]).reshape(1, 3), 6000,
            cu(pr["src"])[None], cu(pr["tar"])[None], "cuda").cpu().numpy()
        lines[:, 40:5200] = 0
    out = {}
    try:
        for mode in ("single", "tiled", "xchg"):  # tiled: the tail kernel (no exchange); xchg: the exchange kernel
            ops.set_reduce_mode(mode)
            st = run_state(tri1, tri2, lines, mode="cull")
            out[mode] = [t.cpu().numpy().copy() for t in (st.loss, st.med, st.info, st.bcnt, st.bsum)]
            if mode != "single":  # the reduce once more on the same prepared state (its control words reset themselves)
                B, N, M, Ll, _ = st.dims
                st.loss.fill_(-1.0)
                ops._run(st.ws.device, "rrl_loss_reduce", ops._p(st.ws), st.nbytes, ops._p(st.loss), B, N, M, Ll, 1, 1, 5, 5, 0)
                torch.cuda.synchronize()
                out["again_" + mode] = [t.cpu().numpy().copy() for t in (st.loss, st.med, st.info, st.bcnt, st.bsum)]
                assert int(st.mctl[:, _lib.MCTL_ERR].sum()) == 0  # no spin ran into its time-out
    finally:
        ops.set_reduce_mode("auto")
    for other in ("tiled", "xchg", "again_tiled", "again_xchg"):
        for a, b in zip(out["single"], out[other]):
            np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))
    assert out["single"][2][:, 1].sum() > 0  # lines were selected


def test_tail_kernel_reports_a_missing_value_list(L):
    """The tail kernel streams the dense D-value lists that the per-line stage builds WHEN it knows the tail kernel
    follows.  A reduce-mode switch between the two stages (a misuse of the knob) must not give a silently wrong median:
    the kernel finds the lists marked absent and returns NaN."""
    from rrl_hip import ops
    g = load_golden("loss_demo_scale.npz")
    try:
        ops.set_reduce_mode("xchg")
        st = run_state(g["tri1"][None], g["tri2"][None], g["lines"][None], mode="cull")
        good = float(st.loss[0])
        B, N, M, Ll, _ = st.dims
        ops.set_reduce_mode("tiled")  # the per-line stage above ran for the exchange kernel: no lists
        ops._run(st.ws.device, "rrl_loss_reduce", ops._p(st.ws), st.nbytes, ops._p(st.loss), B, N, M, Ll, 1, 1, 5, 5, 0)
        torch.cuda.synchronize()
        assert np.isfinite(good) and good > 0 and np.isnan(float(st.loss[0]))
        st2 = run_state(g["tri1"][None], g["tri2"][None], g["lines"][None], mode="cull")  # both stages under "tiled"
        assert float(st2.loss[0]) == good
    finally:
        ops.set_reduce_mode("auto")


@pytest.mark.parametrize("case", ["batch", "dense_tiles", "long_lists", "one_tile", "one_tile_small", "one_tile_dense",
                                  "one_tile_forced", "empty_sample"])
def test_step_in_one_call_equals_forward_then_backward(L, case):
    """rrl_registration_step (the direct backward inside the tail kernel's launch) against rrl_registration_forward +
    rrl_registration_backward: loss, median, info, bucket sums bit for bit; dR, dt, payload to the rounding of their float
    atomics -- a batch with 3-5 line tiles per sample, tiles with more than 256 selected lines (the kernel's second
    pass over a tile, and the crowded-bin route of the median), value lists longer than one streaming round
    of the kernel (32 tiles per sample), a single tile (per-line stage + reduce + backward by one workgroup per sample: the
    C5 route -- with more than 128 selected lines (through the workspace), with fewer (round 5: from the per-line stage's
    registers and LDS, SoloReduce), with ~1000 near-identical ones; and with the tail kernel forced), a sample whose lines hit nothing; with and without payload,
    both R layouts, non-unit dL/dloss."""
    from rrl_hip import ops, synth
    from LieAlgebra import se3
    B = 3
    nl = {"batch": 4500, "dense_tiles": 2600, "long_lists": 32000, "one_tile": 1000, "one_tile_small": 600,
          "one_tile_dense": 1000, "one_tile_forced": 900, "empty_sample": 3000}[case]
    gen = torch.Generator().manual_seed(2)
    R, T = se3.exp3(0.03 * torch.randn(B, 6, generator=gen))
    if case in ("dense_tiles", "one_tile_dense"):  # two tiny triangles per cloud, every line through the first: ~1000 selected lines per tile,
        rng = np.random.default_rng(5)  # near-identical D values (the crowded-bin route of the median) -- no motion
        base = np.array([[0.0, 0.0, 0.0, 0.05, 0.0, 0.0, 0.0, 0.05, 0.0]], np.float32)
        t1 = np.concatenate([base, base + np.float32(3.0)]).astype(np.float32)
        src = cu(np.stack([t1] * B))
        tar = cu(np.stack([(t1 + np.array([0.004, -0.003, 0.002] * 3, np.float32) * (1 + 0.1 * b)).astype(np.float32) for b in range(B)]))
        d = np.tile(np.array([[0.0, 0.0, 1.0]]), (nl, 1))
        ln = cu(np.stack([np.concatenate([d, np.tile(np.array([[0.012, 0.011, -1.0]]), (nl, 1)) + 1e-5 * b * rng.standard_normal((nl, 3))], 1)
                          for b in range(B)]).astype(np.float32))
        R, T = torch.eye(3).repeat(B, 1, 1), torch.zeros(B, 3)
    else:
        prs = [synth.make_pair(40 + b, 900, 800) for b in range(B)]
        src, tar = cu(np.stack([p["src_tri"] for p in prs])), cu(np.stack([p["tar_tri"] for p in prs]))
        ln = []
        for b, p in enumerate(prs):
            torch.manual_seed(b)
            rad = float(p["radius"]) * (0.75 if case == "long_lists" else 1.0)  # a tighter sphere: more lines through both clouds
            ln.append(L.Random_uniform_distribution_lines_batch_efficient_resample(
                torch.tensor([[rad]]), torch.from_numpy(p["center"]).reshape(1, 3), nl, cu(p["src"])[None],
                cu(p["tar"])[None], "cuda")[0])
        ln = torch.stack(ln)
    if case == "empty_sample":
        ln[1] = torch.tensor([1.0, 0, 0, 0, 50, 50], device="cuda")
    R, T = R.cuda().contiguous(), T.cuda().contiguous()
    gl = torch.tensor([1.0, 0.5, 2.0], device="cuda")
    try:
        if case in ("one_tile_forced", "long_lists"):  # (long_lists: 32 tiles per sample, beyond the automatic choice's 16)
            ops.set_reduce_mode("tiled")
        for tr in (True, False):
            res = {}
            for one in (False, True):
                ops.RegistrationStep.ONE_CALL = one
                rs = ops.RegistrationStep(src, tar, nl, transpose_r=tr, want_payload=True)
                for _ in range(2):  # twice: the control words reset themselves
                    loss, gR, gt, pay, info = rs(R, T, ln, grad_loss=gl)
                torch.cuda.synchronize()
                res[one] = [t.cpu().numpy().copy() for t in (loss, rs.st.med, info, rs.st.bcnt, rs.st.bsum, gR, gt, pay)]
            for a, b_ in zip(res[False][:5], res[True][:5]):
                np.testing.assert_array_equal(a.view(np.uint8), b_.view(np.uint8))
            for a, b_ in zip(res[False][5:], res[True][5:]):
                np.testing.assert_allclose(b_, a, rtol=2e-5, atol=2e-6 * float(np.abs(a).max()) + 1e-12)
            nsel = res[True][2][:, 1]
            assert nsel[0] > 0 and (case != "empty_sample" or nsel[1] == 0)
            if case == "dense_tiles":
                assert int(rs.st.blkcnt[:B * 3].max()) > 256
            if case == "one_tile_dense":
                assert int(rs.st.blkcnt[:B].max()) > 256
            if case == "one_tile_small":
                assert 0 < int(nsel.max()) <= 128
            if case == "one_tile":
                assert int(nsel.max()) > 128
            if case == "long_lists":  # more than the 8192 values one streaming round of the tail kernel covers, and a median
                assert int(rs.st.vlcnt[:B * 32].reshape(B, 32).sum(1).max()) > 8192  # bin that is NOT crowded (the usual route)
                assert int(rs.st.mhist.max()) <= 2048
            assert res[True][7][1] == float((res[True][2][:, 0] > 0).sum())  # payload[1] = number of valid samples
            assert res[True][7][1] == (2.0 if case == "empty_sample" else 3.0)
    finally:
        ops.RegistrationStep.ONE_CALL = True
        ops.set_reduce_mode("auto")


@pytest.mark.parametrize("world", [1, 3, 4])
def test_line_sharded_single_sample(L, world):
    """SURVEY 8(e), last sentence: ONE sample with its lines partitioned over `world` ranks (simulated here in one process:
    every share goes through rrl_hip.dist.line_shard_local, the rows are concatenated in rank order as the all-gather
    would, every share's state is reduced with line_shard_merge).  Loss, median, bucket counts and sums of every rank are
    bit-identical to the unsharded evaluation, and the sum of the ranks' point gradients equals its gradient."""
    from rrl_hip import ops, synth, dist as rdist
    pr = synth.make_pair(77, 2500, 2200)
    tri1, tri2 = cu(pr["src_tri"])[None], cu(pr["tar_tri"])[None]
    nl = 7001  # ragged shares, a last tile that is not full
    torch.manual_seed(4)
    ln = L.Random_uniform_distribution_lines_batch_efficient_resample(
        torch.tensor([[float(pr["radius"])]]), torch.from_numpy(pr["center"]).reshape(1, 3), nl, cu(pr["src"])[None],
        cu(pr["tar"])[None], "cuda")
    p1 = tri1.clone().requires_grad_(True)
    p2 = tri2.clone().requires_grad_(True)
    ref_loss, ref_info, _ = ops.intersection_loss(p1, p2, ln)
    ref_state = ops.last_state()
    ref = [t.clone() for t in (ref_loss.detach(), ref_state.med, ref_state.bcnt, ref_state.bsum, ref_info)]
    (2.0 * ref_loss.sum()).backward()
    if world == 1:  # the public entry without a process group
        q1, q2 = tri1.clone().requires_grad_(True), tri2.clone().requires_grad_(True)
        loss, info, _ = rdist.line_sharded_loss(q1, q2, ln)
        assert torch.equal(loss.detach(), ref[0]) and torch.equal(info, ref[4])
        (2.0 * loss.sum()).backward()
        np.testing.assert_allclose(q1.grad.cpu().numpy(), p1.grad.cpu().numpy(), rtol=1e-5, atol=1e-9)
        np.testing.assert_allclose(q2.grad.cpu().numpy(), p2.grad.cpu().numpy(), rtol=1e-5, atol=1e-9)
        return
    shares = [rdist.line_shard_local(tri1, tri2, ln[:, lo:hi].contiguous())
              for lo, hi in (rdist.shard_bounds(nl, r, world) for r in range(world))]
    rows = torch.cat([s[1] for s in shares])
    kj = torch.cat([s[2] for s in shares])
    assert rows.shape[0] == int(ref[4][0, 1]) > 300  # every selected line arrives exactly once
    g1 = torch.zeros_like(tri1)
    g2 = torch.zeros_like(tri2)
    gl = torch.full((1,), 2.0, device="cuda")
    for r, (st, _, _) in enumerate(shares):
        rdist.line_shard_merge(st, rows, kj)
        for a, b_ in zip((st.loss, st.med, st.bcnt, st.bsum, st.info), ref):
            assert torch.equal(a.reshape(-1), b_.reshape(-1)), r
        lo, hi = rdist.shard_bounds(nl, r, world)
        a1, a2 = torch.empty_like(tri1), torch.empty_like(tri2)
        ops._run(tri1.device, "rrl_loss_backward", ops._p(tri1), ops._p(tri2), ops._p(st.ws), st.nbytes, ops._p(gl),
                 ops._p(a1), ops._p(a2), 1, tri1.shape[1], tri2.shape[1], hi - lo, 0)
        g1 += a1
        g2 += a2
    np.testing.assert_allclose(g1.cpu().numpy(), p1.grad.cpu().numpy(), rtol=1e-5, atol=1e-9)
    np.testing.assert_allclose(g2.cpu().numpy(), p2.grad.cpu().numpy(), rtol=1e-5, atol=1e-9)
    assert float(p1.grad.abs().sum()) > 0


def _line_shard_worker(rank, world, port, out):
    import sys
    from conftest import ROOT, PKG
    for p in (ROOT, PKG):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK="0")
    import torch.distributed as tdist
    from rrl_hip import dist as rdist
    tdist.init_process_group(backend="gloo", rank=rank, world_size=world)  # (one GPU here: RCCL wants a GPU per rank)
    d = np.load(out + ".in.npz")
    t1 = torch.from_numpy(d["tri1"]).cuda().requires_grad_(True)
    t2 = torch.from_numpy(d["tri2"]).cuda().requires_grad_(True)
    ln = torch.from_numpy(d["lines"]).cuda()
    loss, info, status = rdist.line_sharded_loss(t1, t2, ln)
    (3.0 * loss.sum()).backward()
    torch.cuda.synchronize()
    torch.save(dict(loss=loss.detach().cpu(), info=info.cpu(), g1=t1.grad.cpu(), g2=t2.grad.cpu()), f"{out}.{rank}.pt")
    tdist.barrier()
    tdist.destroy_process_group()


@pytest.mark.timeout(600)
def test_line_sharded_two_processes(L, tmp_path):
    """rrl_hip.dist.line_sharded_loss end to end with real collectives: two processes (both on this GPU, gloo moving the
    device tensors) share the lines of one sample; each returns the unsharded loss bit for bit and the full gradient."""
    import socket
    import torch.multiprocessing as mp
    from rrl_hip import ops, synth
    pr = synth.make_pair(78, 1800, 1600)
    tri1, tri2 = pr["src_tri"][None], pr["tar_tri"][None]
    torch.manual_seed(2)
    ln = L.Random_uniform_distribution_lines_batch_efficient_resample(
        torch.tensor([[float(pr["radius"])]]), torch.from_numpy(pr["center"]).reshape(1, 3), 5003, cu(pr["src"])[None],
        cu(pr["tar"])[None], "cuda")
    p1, p2 = cu(tri1).requires_grad_(True), cu(tri2).requires_grad_(True)
    ref_loss, ref_info, _ = ops.intersection_loss(p1, p2, ln)
    (3.0 * ref_loss.sum()).backward()
    out = str(tmp_path / "ls")
    np.savez(out + ".in.npz", tri1=tri1, tri2=tri2, lines=ln.cpu().numpy())
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_line_shard_worker, args=(2, port, out), nprocs=2, join=True)
    for rank in range(2):
        r = torch.load(f"{out}.{rank}.pt")
        assert torch.equal(r["loss"], ref_loss.detach().cpu()) and torch.equal(r["info"], ref_info.cpu())
        np.testing.assert_allclose(r["g1"].numpy(), p1.grad.cpu().numpy(), rtol=1e-5, atol=1e-9)
        np.testing.assert_allclose(r["g2"].numpy(), p2.grad.cpu().numpy(), rtol=1e-5, atol=1e-9)
    assert int(ref_info[0, 1]) > 200


def test_step_with_a_carried_target(L):
    """RPM / FMR: several poses against ONE target and ONE line set.  The second pose's step takes the target's scan from
    the first pose's state (target_from): loss, median, info, bucket sums and hit counts bit for bit what a full step of
    that pose gives, gradients to the rounding of their atomics -- for the one-call step and for forward + backward.
    (Hit lists are committed in atomic order: the counts are compared, the lists through everything derived from them.)"""
    from rrl_hip import ops, synth
    from LieAlgebra import se3
    B, nl = 4, 6000
    prs = [synth.make_pair(60 + b, 1200, 1000) for b in range(B)]
    src, tar = cu(np.stack([p["src_tri"] for p in prs])), cu(np.stack([p["tar_tri"] for p in prs]))
    ln = []
    for b, p in enumerate(prs):
        torch.manual_seed(b)
        ln.append(L.Random_uniform_distribution_lines_batch_efficient_resample(
            torch.tensor([[float(p["radius"])]]), torch.from_numpy(p["center"]).reshape(1, 3), nl, cu(p["src"])[None],
            cu(p["tar"])[None], "cuda")[0])
    ln = torch.stack(ln)
    gen = torch.Generator().manual_seed(9)
    poses = [tuple(x.cuda().contiguous() for x in se3.exp3(0.02 * torch.randn(B, 6, generator=gen))) for _ in range(2)]
    try:
        for one in (True, False):
            ops.RegistrationStep.ONE_CALL = one
            first, full, carried = (ops.RegistrationStep(src, tar, nl, want_payload=True) for _ in range(3))
            first(*poses[0], ln)
            a = full(*poses[1], ln)
            b_ = carried(*poses[1], ln, target_from=first.st)
            torch.cuda.synchronize()
            for x, y in ((a[0], b_[0]), (full.st.med, carried.st.med), (a[4], b_[4]), (full.st.bsum, carried.st.bsum),
                         (full.st.count2, carried.st.count2), (full.st.count1, carried.st.count1)):
                assert torch.equal(x, y)
            for x, y in ((a[1], b_[1]), (a[2], b_[2]), (a[3], b_[3])):
                np.testing.assert_allclose(y.cpu().numpy(), x.cpu().numpy(), rtol=2e-5, atol=2e-6 * float(x.abs().max()))
            assert int(a[4][:, 1].min()) > 0
            with pytest.raises(ValueError):
                carried(*poses[1], ln, target_from=carried.st)
    finally:
        ops.RegistrationStep.ONE_CALL = True


def test_step_in_one_call_at_the_bench_shape(L):
    """BASELINE configs[1] at full size (B=8, N=M=4096, L=10000; bench.py's workload): the one-call step equals forward +
    backward (loss / median / info / bucket sums bit for bit, gradients to the rounding of their atomics) and reproduces
    itself over 50 calls."""
    import sys
    from conftest import ROOT
    sys.path.insert(0, ROOT)
    import bench
    from rrl_hip import ops
    dev = torch.device("cuda:0")
    B, N, nl = 8, 4096, 10000
    w = bench.make_workload(B, N, N, nl, 0, dev)
    R, t = torch.eye(3, device=dev).repeat(B, 1, 1), torch.zeros(B, 3, device=dev)
    try:
        res = {}
        for one in (False, True):
            ops.RegistrationStep.ONE_CALL = one
            rs = ops.RegistrationStep(w["tri1"], w["tri2"], nl, want_payload=True)
            out = rs(R, t, w["lines"])
            torch.cuda.synchronize()
            res[one] = [x.clone() for x in (out[0], rs.st.med, out[4], rs.st.bsum, out[3][:2], out[1], out[2])]
            if one:
                for _ in range(50):
                    out = rs(R, t, w["lines"])
                    again = [out[0], rs.st.med, out[4], rs.st.bsum, out[3][:2]]
                    assert all(torch.equal(a, b_) for a, b_ in zip(again, res[True][:5]))
    finally:
        ops.RegistrationStep.ONE_CALL = True
    for a, b_ in zip(res[False][:4], res[True][:4]):
        assert torch.equal(a, b_)
    np.testing.assert_allclose(res[True][4].cpu().numpy(), res[False][4].cpu().numpy(), rtol=1e-6)
    for a, b_ in zip(res[False][5:], res[True][5:]):
        np.testing.assert_allclose(b_.cpu().numpy(), a.cpu().numpy(), rtol=2e-5, atol=2e-6 * float(a.abs().max()))
    assert float(res[True][4][1]) == 8.0 and int(res[True][2][:, 1].min()) > 500


@pytest.mark.parametrize("B,n,m,nl,with_pose,prepared", [
    (2, 1200, 1000, 6000, True, True), (2, 1200, 1000, 6000, True, False), (3, 700, 900, 3000, False, True),
    (1, 900, 800, 800, True, True), (20, 300, 260, 8000, True, True), (1, 5000, 4100, 2500, True, True),
    (40, 200, 180, 8000, True, True), (3, 700, 900, 1000, False, False), (4, 2000, 2000, 1024, True, True),
    (2, 16384, 16384, 512, True, True), (1, 1024, 1024, 20000, True, True), (2, 900, 800, 32768, True, False)])
def test_loss_step_equals_the_autograd_chain(L, B, n, m, nl, with_pose, prepared):
    """rrl_loss_step_ex (ops.LossStep): SURVEY 8(d)'s definition -- rigid apply + loss + backward to points1.grad -- in one
    C call.  Against the drop-in autograd chain rigid_apply -> intersection_loss -> backward: loss / median / info /
    bucket sums bit for bit, points1.grad to the rounding of the scatter's float atomics (1e-6 of the largest entry),
    the same rows non-zero.  Shapes: the tail kernel carrying the scatter (2 .. 32 tiles), a single tile of lines (the
    single-tile kernel carrying it: pair_reduce_scatter_kernel; with / without a pose, cold / prepared, C5's shape), a
    grid at the edge of the tail kernel's (B x tiles = 160) and beyond it (320 > 256: exchange reduce + scatter launch), a chunked large cloud; without a pose (R = t = None); cold and
    prepared builds; a non-unit dL/dloss; repeated calls (the records launch clears the gradient each time)."""
    from rrl_hip import ops, synth
    from LieAlgebra import se3
    prs = [synth.make_pair(500 + b, n, m) for b in range(B)]
    src, tar = cu(np.stack([p["src_tri"] for p in prs])), cu(np.stack([p["tar_tri"] for p in prs]))
    ln = []
    for b, p in enumerate(prs):
        torch.manual_seed(b)
        ln.append(L.Random_uniform_distribution_lines_batch_efficient_resample(
            torch.tensor([[float(p["radius"])]]), torch.from_numpy(p["center"]).reshape(1, 3), nl, cu(p["src"])[None],
            cu(p["tar"])[None], "cuda")[0])
    ln = torch.stack(ln)
    gen = torch.Generator().manual_seed(11)
    R, t = (x.cuda().contiguous() for x in se3.exp3(0.03 * torch.randn(B, 6, generator=gen)))
    gl = (0.5 + torch.rand(B, generator=gen)).cuda()
    step = ops.LossStep(src, tar, nl, prepared=prepared)
    for rnd, g in enumerate((None, gl, gl)):
        tri = (ops.rigid_apply(src.reshape(B, -1, 3), R, t, transpose_r=True).reshape(B, n, 9) if with_pose else src.clone()).detach().requires_grad_(True)
        loss, info, _ = ops.intersection_loss(tri, tar, ln)
        ref_st = ops.last_state()
        torch.autograd.backward([loss], [g if g is not None else torch.ones_like(loss)])
        out = step(R if with_pose else None, t if with_pose else None, ln, grad_loss=g)
        torch.cuda.synchronize()
        assert torch.equal(out[0], loss.detach()) and torch.equal(out[2], info)
        assert torch.equal(step.st.med, ref_st.med) and torch.equal(step.st.bsum, ref_st.bsum)
        a, b_ = tri.grad, out[1]
        assert torch.equal(a.abs().sum(-1) > 0, b_.abs().sum(-1) > 0)
        np.testing.assert_allclose(b_.cpu().numpy(), a.cpu().numpy(), rtol=2e-5, atol=1e-6 * float(a.abs().max()))
        if with_pose:
            assert torch.equal(step.st.tri1t, tri.detach())
    assert int(out[2][:, 1].min()) > 0


def test_fused_registration_op(L):
    """rrl_registration_forward/backward == rigid apply + loss + rigid backward, incl. payload."""
    from rrl_hip import ops
    from LieAlgebra import se3
    g = load_golden("loss_b2_quirk.npz")
    src, tar, ln = cu(g["tri1"]), cu(g["tri2"]), cu(g["lines"])
    gen = torch.Generator().manual_seed(5)
    R0, T0 = se3.exp3(0.05 * torch.randn(2, 6, generator=gen))
    res = {}
    for fused in (False, True):
        R, T = R0.cuda().requires_grad_(True), T0.cuda().requires_grad_(True)
        if fused:
            loss, info, _ = ops.registration_loss(src, R, T, tar, ln, want_payload=True)
        else:
            moved = ops.rigid_apply(src.reshape(2, -1, 3), R, T, transpose_r=True).reshape(src.shape)
            loss, info, _ = ops.intersection_loss(moved, tar, ln)
        (loss * torch.tensor([1.0, 2.0], device="cuda")).sum().backward()
        res[fused] = (loss.detach().cpu().numpy(), R.grad.cpu().numpy(), T.grad.cpu().numpy())
    np.testing.assert_array_equal(res[True][0], res[False][0])
    np.testing.assert_allclose(res[True][1], res[False][1], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(res[True][2], res[False][2], rtol=1e-4, atol=1e-6)
    pay = ops.last_state().payload.cpu().numpy()
    np.testing.assert_allclose(pay[0], res[True][0].sum(), rtol=1e-6)
    assert pay[1] == 2.0
    np.testing.assert_allclose(pay[2:11], res[True][1].sum(0).reshape(-1), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(pay[11:], res[True][2].sum(0), rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("n,m,transpose_r", [(300, 200, True), (300, 200, False), (16390, 400, True), (65540, 300, True),
                                              (5, 40, True)])
def test_fused_registration_backward_paths(L, n, m, transpose_r):
    """The three backward routes of the fused op agree with the unfused composition: (a) direct
    (dR, dt) kernel, (b) with d/dsrc (per-triangle scatter + rigid backward tail), (c) clouds beyond
    the sorted-path limit (separate rigid backward + payload kernels); repeated backward on the
    same graph (retain_graph) gives the same result (the ticket counters reset themselves)."""
    from rrl_hip import ops, synth
    from LieAlgebra import se3
    B, nl = 3, 1200
    prs = [synth.make_pair(90 + b, max(n, 16), max(m, 16)) for b in range(B)]
    src = cu(np.stack([p["src_tri"][:n] for p in prs]))
    tar = cu(np.stack([p["tar_tri"][:m] for p in prs]))
    g = load_golden("sampler.npz")
    lines = cu(np.stack([np.resize(g["final"], (nl, 6))] * B))
    gen = torch.Generator().manual_seed(11)
    R0, T0 = se3.exp3(0.03 * torch.randn(B, 6, generator=gen))
    wts = torch.tensor([1.0, -0.5, 2.0], device="cuda")

    def run(fused, want_src):
        R, T = R0.cuda().requires_grad_(True), T0.cuda().requires_grad_(True)
        s = src.clone().requires_grad_(want_src)
        if fused:
            loss, info, _ = ops.registration_loss(s, R, T, tar, lines, transpose_r=transpose_r, want_payload=True)
        else:
            moved = ops.rigid_apply(s.reshape(B, -1, 3), R, T, transpose_r=transpose_r).reshape(s.shape)
            loss, info, _ = ops.intersection_loss(moved, tar, lines)
        (loss * wts).sum().backward(retain_graph=True)
        first = (R.grad.clone(), T.grad.clone())
        R.grad = T.grad = None
        (loss * wts).sum().backward()
        for a, b2 in zip(first, (R.grad, T.grad)):
            torch.testing.assert_close(a, b2, rtol=1e-5, atol=1e-7)
        return loss.detach(), R.grad, T.grad, (s.grad if want_src else None), info

    ref = run(False, True)
    assert int(ref[4][:, 1].sum()) > 0 or n < 16
    for want_src in (False, True):
        got = run(True, want_src)
        assert torch.equal(got[0], ref[0])
        scale = float(ref[1].abs().max()) + 1e-12
        torch.testing.assert_close(got[1], ref[1], rtol=2e-4, atol=2e-6 * scale)
        torch.testing.assert_close(got[2], ref[2], rtol=2e-4, atol=2e-6 * scale)
        if want_src:
            a, b2 = got[3].cpu().numpy(), ref[3].cpu().numpy()
            for bb in range(B):
                ma = merge_by_point(src[bb].cpu().numpy(), a[bb])
                mb = merge_by_point(src[bb].cpu().numpy(), b2[bb])
                np.testing.assert_allclose(ma, mb, rtol=1e-4, atol=1e-6 * (np.abs(mb).max() + 1e-12))


def test_deterministic_direct_backward(L):
    """rrl_set_deterministic: the direct (dR, dt) backward with fixed-order partial sums is bit-reproducible
    run to run (the default accumulates with float atomics: equal to rounding noise only) and agrees
    with the default and with the d/dsrc route."""
    from rrl_hip import ops, synth
    from LieAlgebra import se3
    B, N, M, nl = 3, 1500, 1300, 5000
    prs = [synth.make_pair(60 + b, N, M) for b in range(B)]
    src = cu(np.stack([p["src_tri"] for p in prs]))
    tar = cu(np.stack([p["tar_tri"] for p in prs]))
    torch.manual_seed(2)
    lines = L.Random_uniform_distribution_lines_batch_efficient_resample(
        torch.tensor([[p["radius"]] for p in prs]), torch.from_numpy(np.stack([p["center"] for p in prs])), nl,
        src.reshape(B, -1, 3), tar.reshape(B, -1, 3), "cuda")
    R0, T0 = se3.exp3(0.05 * torch.randn(B, 6, generator=torch.Generator().manual_seed(1)))

    def grads():
        R, t = R0.cuda().requires_grad_(True), T0.cuda().requires_grad_(True)
        loss, _, _ = ops.registration_loss(src, R, t, tar, lines, transpose_r=True, want_payload=True)
        loss.sum().backward()
        return R.grad.clone(), t.grad.clone(), ops.last_state().payload.clone(), loss.detach().clone()
    ref = grads()
    ops.set_deterministic(True)
    try:
        runs = [grads() for _ in range(12)]
    finally:
        ops.set_deterministic(False)
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert torch.equal(a, b)
    for a, b in zip(runs[0], ref):
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=2e-5, atol=1e-7)
    assert float(runs[0][0].abs().sum()) > 0 and float(runs[0][2][1]) == B


def test_grad_src_path_hand_over_stress(L):
    """The d/dsrc route (scatter + reg_bwd_kernel: per-workgroup partials handed to the last workgroup through
    write-through stores and a ticket -- outside the HIP memory model, csrc/rrl_geom.hip) run 60 times at two
    shapes: a stale or missing partial would change dR / dt by a whole workgroup's share; the scatter's float
    atomics alone only cause rounding noise (compared to 1e-4; loss and payload head bit for bit)."""
    from rrl_hip import ops, synth
    from LieAlgebra import se3
    for B, N, M, nl in ((4, 3000, 2500, 6000), (8, 4096, 4096, 10000)):
        prs = [synth.make_pair(80 + b, N, M) for b in range(B)]
        src0 = np.stack([p["src_tri"] for p in prs])
        tar = cu(np.stack([p["tar_tri"] for p in prs]))
        lines = L.Random_uniform_distribution_lines_batch_efficient_resample(
            torch.tensor([[p["radius"]] for p in prs]), torch.from_numpy(np.stack([p["center"] for p in prs])), nl,
            cu(src0).reshape(B, -1, 3), tar.reshape(B, -1, 3), "cuda", device_rng=True)
        R0, T0 = se3.exp3(0.05 * torch.randn(B, 6, generator=torch.Generator().manual_seed(4)))
        ref = None
        for it in range(30):
            src = cu(src0).requires_grad_(True)
            R, t = R0.cuda().requires_grad_(True), T0.cuda().requires_grad_(True)
            loss, _, _ = ops.registration_loss(src, R, t, tar, lines, transpose_r=True, want_payload=True)
            loss.sum().backward()
            # the scatter into the per-triangle gradient uses float atomics (order-dependent rounding): compare what
            # reg_bwd_kernel's hand-over produces from it only through values that do not depend on that order
            out = (loss.detach().clone(), ops.last_state().payload[:2].clone())
            assert torch.isfinite(src.grad).all() and torch.isfinite(R.grad).all() and float(src.grad.abs().sum()) > 0
            if ref is None:
                ref = out + (R.grad.clone(), t.grad.clone(), src.grad.clone())
            else:
                assert torch.equal(out[0], ref[0]) and torch.equal(out[1], ref[1])
                np.testing.assert_allclose(R.grad.cpu().numpy(), ref[2].cpu().numpy(), rtol=1e-4, atol=1e-7)
                np.testing.assert_allclose(t.grad.cpu().numpy(), ref[3].cpu().numpy(), rtol=1e-4, atol=1e-7)
                np.testing.assert_allclose(src.grad.cpu().numpy(), ref[4].cpu().numpy(), rtol=1e-3, atol=1e-8)


def test_identity_registration_is_nan_like_the_reference(L, oracle):
    """src == tar: every D is 0, the median is 0 and Welsch1(0, 0) = 1 - exp(-(0/0)/2) is NaN in the
    reference (code/loss.py:20-21, 223-229; the oracle and the torch-eager restatement agree): the loss must
    be NaN, not a finite under-count."""
    g = load_golden("loss_synth_s0.npz")
    assert np.isnan(oracle.loss(g["tri1"], g["tri1"], g["lines"], want_grad=False)["loss"])
    st = run_state(g["tri1"], g["tri1"], g["lines"], mode="cull")
    assert int(st.info[0, 0]) > 0 and float(st.med[0]) == 0.0
    assert np.isnan(st.loss.cpu().numpy()[0])
    out = L.cal_loss_intersection_batch_whole_median_pts_lines(1, 1, 5, 5, cu(g["tri1"])[None], cu(g["tri1"])[None],
                                                                cu(g["lines"])[None], "cuda")
    assert out is not None and torch.isnan(out).all()


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs")
def test_inputs_on_a_non_current_device(L):
    """Every op launches on the device that owns its data (ops._guard), whatever the current device is."""
    from rrl_hip import ops
    g = load_golden("loss_synth_s1.npz")
    d1 = torch.device("cuda", 1)
    torch.cuda.set_device(0)
    t1, t2, ln = (torch.from_numpy(g[k])[None].to(d1) for k in ("tri1", "tri2", "lines"))
    p = t1.clone().requires_grad_(True)
    out = L.cal_loss_intersection_batch_whole_median_pts_lines(1, 1, 5, 5, p, t2, ln, d1)
    np.testing.assert_allclose(out.item(), g["r0_loss"], rtol=1e-5)
    out.backward()
    assert p.grad.device == d1 and torch.isfinite(p.grad).all()
    assert L.chamfer_dist(t1[..., :3], t2[..., :3]).device == d1
    lines = L.Random_uniform_distribution_lines_batch_efficient_resample(
        torch.tensor([[1.0]]), torch.zeros(1, 3), 500, t1[..., :3], t2[..., :3], d1)
    assert lines.device == d1 and torch.cuda.current_device() == 0


def test_graphed_step_matches_eager(L):
    from rrl_hip import ops
    from rrl_hip.graph import GraphedStep
    g = load_golden("loss_b2_quirk.npz")
    src, tar, ln = cu(g["tri1"]), cu(g["tri2"]), cu(g["lines"])
    R = torch.eye(3, device="cuda").repeat(2, 1, 1).requires_grad_(True)
    T = torch.zeros(2, 3, device="cuda", requires_grad=True)
    ones = torch.ones(2, device="cuda")

    def fn():
        R.grad = T.grad = None
        loss, _, _ = ops.registration_loss(src, R, T, tar, ln, want_payload=True)
        torch.autograd.backward([loss], [ones])
        return loss, ops.last_state().payload

    e_loss, e_pay = (t.detach().clone() for t in fn())  # no reference to the eager autograd graph
    gs = GraphedStep(fn)
    for _ in range(3):
        g_loss, g_pay = gs()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(g_loss.detach().cpu().numpy(), e_loss.cpu().numpy())
    np.testing.assert_allclose(g_pay.cpu().numpy(), e_pay.cpu().numpy(), rtol=1e-5, atol=1e-7)


# ---------------------------------------------------------------------------------- Sample_neighs
def test_sample_neighs_vs_reference(L):
    """GPU FPS + 3-NN reproduce the reference's Sample_neighs rows for the same torch seed
    (the FPS start index comes from torch.randint on the CPU generator, like the reference)."""
    g = load_golden("sample_neighs.npz")
    torch.manual_seed(77)
    full = L.Sample_neighs(g["points"])
    assert full.shape == g["full"].shape and full.dtype == g["points"].dtype
    np.testing.assert_array_equal(full, g["full"])
    torch.manual_seed(78)
    sub = L.Sample_neighs(g["points"], num_sample=300)
    np.testing.assert_array_equal(sub, g["sub"])


def test_fps_and_knn_properties(L):
    from rrl_hip import neighbors
    gen = torch.Generator().manual_seed(3)
    pts = torch.randn(2, 9000, 3, generator=gen)  # > 8192 points: the global-memory FPS path
    idx = neighbors.fps(pts, 500, start=torch.tensor([5, 7])).cpu().numpy()
    assert idx.shape == (2, 500) and idx[0, 0] == 5 and idx[1, 0] == 7
    for b in range(2):
        assert len(set(idx[b].tolist())) == 500
        p = pts[b].numpy().astype(np.float32)
        d = np.full(9000, 1e10, np.float32)
        cur = idx[b, 0]
        for it in range(1, 40):  # replay the first steps on the host
            diff = p - p[cur]
            s = (diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]) + diff[:, 2] * diff[:, 2]
            d = np.minimum(d, s)
            cur = int(np.argmax(d))
            assert cur == idx[b, it]
    nn = neighbors.knn3(pts, torch.from_numpy(idx)).cpu().numpy()
    from scipy.spatial import cKDTree
    for b in range(2):
        p = pts[b].numpy().astype(np.float64)
        _, ref = cKDTree(p).query(p[idx[b]], k=3)
        np.testing.assert_array_equal(nn[b], ref)
