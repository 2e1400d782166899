"""SURVEY.md §8a-H on the GPU: the trainers' loss fragments (rrl_hip.callsites) and the demo
optimisation loop (test_demo_optimized_Lie_Algebra.py), against values recorded from the
reference's own functions (tests/golden/make_golden.py: callsites, demo_trajectory).

Tolerances: the fused op moves the source triangles on the GPU (x R^T + t per point in fp32)
while the fixture used torch's CPU matmul; vertices differ by an ulp, which can flip a
borderline hit decision and move one line between buckets.  Loss values are therefore compared
to 2e-4 relative (1e-5 when the recorded, already-moved triangles are fed in), gradients to
2e-3 of the largest entry; the optimisation trajectory (8 Adam steps) to 2e-3 absolute in xi.
"""
import os

import numpy as np
import pytest
import torch

from conftest import load_golden  # noqa: F401 (the `oracle` fixture comes from conftest, too)

pytestmark = pytest.mark.gpu


def cu(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda().requires_grad_(grad)


@pytest.fixture(scope="module")
def C():
    from rrl_hip import _lib, callsites
    _lib.load()
    assert torch.cuda.is_available()
    return callsites


@pytest.fixture(scope="module")
def G():
    return load_golden("callsites.npz")


def data_dict(g, channel_first=False):
    d = {'points_src_sample': cu(g["src"]), 'points_tar_sample': cu(g["tar"]),
         'points_based_neighs_src': cu(g["nb_src"]), 'points_based_neighs_tar': cu(g["nb_tar"]),
         'tar_box': cu(g["tar_box"]), 'centers': cu(g["centers"])}
    if channel_first:
        for k in ('points_src_sample', 'points_tar_sample', 'points_based_neighs_src',
                  'points_based_neighs_tar'):
            d[k] = d[k].transpose(2, 1).contiguous()
    return d


def close_grad(got, want, rel=2e-3):
    got, want = got.detach().cpu().numpy(), np.asarray(want)
    assert np.abs(got - want).max() <= rel * np.abs(want).max(), (np.abs(got - want).max(), np.abs(want).max())


def test_rpm_fragment(C, G):
    R, t = cu(G["R"], True), cu(G["t"], True)
    pred = [torch.cat([R[i], t[i][..., None]], dim=-1) for i in range(R.shape[0])]  # (B, 3, 4)
    out = C.rpm_intersection_loss(pred, data_dict(G), lines=cu(G["rpm_lines"]))
    assert out['loss_intersection'].shape == (1,)
    np.testing.assert_allclose([x.item() for x in out['per_iter']], G["rpm_per_iter"], rtol=2e-4)
    np.testing.assert_allclose(out['loss_intersection'].item(), G["rpm_loss"], rtol=2e-4)
    np.testing.assert_allclose(out['loss_chamfer'].item(), G["rpm_chamfer"], rtol=1e-5)
    assert bool(out['valid'].all()) and not out['loss_chamfer'].requires_grad
    out['loss_intersection'].backward()
    close_grad(R.grad, G["rpm_grad_R"])
    close_grad(t.grad, G["rpm_grad_t"])


def test_rpm_per_sample_matches_the_python_loop(C, G):
    """`for j in range(B): acc += cal_loss(...[j:j+1])` on the moved triangles == one batched call."""
    import loss as L
    R, t = cu(G["R"][0]), cu(G["t"][0])
    nb = cu(G["nb_src"])
    tri = (nb @ R.transpose(-1, -2) + t[:, None, :]).reshape(nb.shape[0], -1, 9)
    tar_tri = cu(G["nb_tar"]).reshape(nb.shape[0], -1, 9)
    lines = cu(G["rpm_lines"])
    loop = [L.cal_loss_intersection_batch_whole_median_pts_lines(
        1, 1, 5, 5, tri[j:j + 1], tar_tri[j:j + 1], lines[j:j + 1], 'cuda').item() for j in range(3)]
    np.testing.assert_allclose(loop, G["rpm_per_sample"][0], rtol=2e-4)
    fused, ok = C.per_sample_loss(nb, R, t, tar_tri, lines)
    np.testing.assert_allclose(fused.cpu().numpy(), loop, rtol=2e-4)
    assert bool(ok.all())


def test_dcp_fragment(C, G):
    R, t = cu(G["R"][0], True), cu(G["t"][0], True)
    loss, chamfer, lines, ok = C.dcp_intersection_loss(data_dict(G, channel_first=True), R, t,
                                                       lines=cu(G["dcp_lines"]))
    np.testing.assert_allclose(loss.item(), G["dcp_loss"], rtol=2e-4)
    np.testing.assert_allclose(chamfer.item(), G["dcp_chamfer"], rtol=1e-5)
    loss.backward()
    close_grad(R.grad, G["dcp_grad_R"])
    close_grad(t.grad, G["dcp_grad_t"])


def test_fragment_loss_on_the_references_moved_triangles(C, G):
    """The TIGHT W check of the fragments (round 5): tests/golden/callsites_moved.npz holds the reference's MOVED
    pseudo-triangles of every RPM iteration, its labels (per-line hit counts), per-sample losses and dL/dpoints1.  On those
    identical inputs -- SURVEY 8a-R's definition of W's parity -- the HIP loss is label-exact and within 1e-5 per sample (the
    end-to-end fragment checks above stay at 2e-4: there the source is moved on the GPU with FMAs, an ulp in a vertex may
    flip a borderline label).  All three entries that evaluate given triangles: the batched op, the section-8(d) step with
    R = t = None, and the reference-signature per-sample call."""
    import loss as L
    from conftest import merge_by_point
    from rrl_hip import ops
    M_ = load_golden("callsites_moved.npz")
    assert M_["margin"] > 1e-5
    B = G["nb_tar"].shape[0]
    tar_tri, lines = cu(G["nb_tar"]).reshape(B, -1, 9), cu(G["rpm_lines"])
    for ni in range(M_["moved_tri"].shape[0]):
        tri = cu(M_["moved_tri"][ni], True)
        loss, info, _ = ops.intersection_loss(tri, tar_tri, lines)
        st = ops.last_state()
        np.testing.assert_array_equal(st.count1.cpu().numpy(), M_["count1"][ni])   # labels: exact
        np.testing.assert_array_equal(st.count2.cpu().numpy(), M_["count2"])
        np.testing.assert_allclose(loss.detach().cpu().numpy(), M_["per_sample"][ni], rtol=1e-5)
        loss.sum().backward()
        step = ops.LossStep(tri.detach(), tar_tri, lines.shape[1])
        sl, sg, _ = step(None, None, lines)
        assert torch.equal(sl, loss.detach())
        for j in range(B):
            ref = merge_by_point(M_["moved_tri"][ni, j], M_["grad_tri"][ni, j])
            for got in (tri.grad[j], sg[j]):
                mine = merge_by_point(M_["moved_tri"][ni, j], got.cpu().numpy())
                np.testing.assert_allclose(mine, ref, rtol=1e-4, atol=1e-5 * np.abs(ref).max())
            one = L.cal_loss_intersection_batch_whole_median_pts_lines(1, 1, 5, 5, tri.detach()[j:j + 1], tar_tri[j:j + 1],
                                                                       lines[j:j + 1], "cuda")
            np.testing.assert_allclose(one.item(), M_["per_sample"][ni, j], rtol=1e-5)


def test_dcp_and_fmr_losses_on_the_references_moved_triangles(C, G):
    """round 6: callsites_moved.npz's tight check for the other two trainers' layouts --
    tests/golden/callsites_moved_dcp_fmr.npz holds the reference's moved pseudo-triangles of the DCP fragment (CHANNEL-FIRST
    clouds moved by code/utils.py:32-37 transform_point_cloud; dcp/Train_DCP.py:233-270) and of the FMR fragment's last three
    estimates (4 x 4 matrices through fmr/se_math/se3.py:110-124; fmr/model.py:265-313), its labels, per-sample losses and
    dL/dpoints1.  On those identical inputs: labels exact, 1e-5 per sample, per-point gradient 1e-4 -- the batched op and the
    section-8(d) step (R = t = None); and the library's own rigid apply in those two layouts (ops.rigid_apply channel_first /
    the 4 x 4 split) lands within 1e-6 of the extent of the reference's moved triangles."""
    from conftest import merge_by_point
    from rrl_hip import ops
    M_ = load_golden("callsites_moved_dcp_fmr.npz")
    assert M_["margin"] > 1e-6
    B = G["nb_tar"].shape[0]
    tar_tri = cu(G["nb_tar"]).reshape(B, -1, 9)
    cases = [("dcp", M_["dcp_moved_tri"], M_["dcp_grad_tri"], M_["dcp_per_sample"], M_["dcp_count1"], M_["dcp_count2"], cu(G["dcp_lines"]), 0)]
    k = M_["fmr_moved_tri"].shape[0]
    cases += [("fmr", M_["fmr_moved_tri"][i], M_["fmr_grad_tri"][i], M_["fmr_per_sample"][i], M_["fmr_count1"][i], M_["fmr_count2"],
               cu(G["fmr_lines"]), G["R"].shape[0] - k + i) for i in range(k)]
    for name, tris, grads, per, c1, c2, lines, pose in cases:
        tri = cu(tris, True)
        loss, info, _ = ops.intersection_loss(tri, tar_tri, lines)
        st = ops.last_state()
        np.testing.assert_array_equal(st.count1.cpu().numpy(), c1)   # labels: exact
        np.testing.assert_array_equal(st.count2.cpu().numpy(), c2)
        np.testing.assert_allclose(loss.detach().cpu().numpy(), per, rtol=1e-5)
        loss.sum().backward()
        step = ops.LossStep(tri.detach(), tar_tri, lines.shape[1])
        sl, sg, _ = step(None, None, lines)
        assert torch.equal(sl, loss.detach())
        for j in range(B):
            ref = merge_by_point(tris[j], grads[j])
            for got in (tri.grad[j], sg[j]):
                np.testing.assert_allclose(merge_by_point(tris[j], got.cpu().numpy()), ref, rtol=1e-4, atol=1e-5 * np.abs(ref).max())
        # T in this trainer's layout: the library's rigid apply against the reference's moved triangles
        R, t = cu(G["R"][pose]), cu(G["t"][pose])
        nb = cu(G["nb_src"])
        if name == "dcp":  # channel-first (B, 3, 3N) through the drop-in utils.transform_point_cloud (rot @ cloud + t)
            import utils
            mine = utils.transform_point_cloud(nb.transpose(2, 1).contiguous(), R, t).transpose(2, 1).reshape(B, -1, 9)
        else:              # R, t split out of the 4 x 4 matrix (callsites.fmr_intersection_loss)
            mine = ops.rigid_apply(nb, R, t, transpose_r=True).reshape(B, -1, 9)
        assert float((mine - tri.detach()).abs().max()) <= 1e-6 * float(tri.detach().abs().max())


def test_fmr_fragment(C, G):
    R, t = cu(G["R"], True), cu(G["t"], True)
    bottom = torch.tensor([0.0, 0, 0, 1], device='cuda').expand(R.shape[1], 1, 4)
    gs = [torch.cat([torch.cat([R[i], t[i][..., None]], dim=-1), bottom], dim=1) for i in range(R.shape[0])]
    loss, chamfer, lines, ok = C.fmr_intersection_loss(gs, data_dict(G), lines=cu(G["fmr_lines"]))
    np.testing.assert_allclose(loss.item(), G["fmr_loss"], rtol=2e-4)
    np.testing.assert_allclose(chamfer.item(), G["fmr_chamfer"], rtol=1e-5)
    loss.backward()
    close_grad(R.grad, G["fmr_grad_R"])
    close_grad(t.grad, G["fmr_grad_t"])


def test_fragments_monitor_from_the_loss_state(C, G):
    """callsites.CHAMFER_FROM_LOSS: the trainers' Chamfer monitor walks the clouds the loss evaluation
    just sorted (ops.chamfer_from_state) instead of sorting the point samples again.  The fixture's samples
    are the first points of its pseudo-triangles, so the values equal the reference-generated ones.  "auto" (the
    default) finds that out itself -- from the dataset's `p0_rows` flag or one device comparison per data dict --
    and falls back to the standalone kernel when the contract does not hold."""
    from rrl_hip import ops
    assert C.CHAMFER_FROM_LOSS == "auto"
    nb, src = np.asarray(G["nb_src"]), np.asarray(G["src"])
    np.testing.assert_array_equal(nb.reshape(nb.shape[0], -1, 9)[..., :3], src[..., :3])  # the contract
    calls = {"state": 0, "plain": 0}
    real_state, real_plain = ops.chamfer_from_state, ops.chamfer

    def spy_state(*a, **k):
        calls["state"] += 1
        return real_state(*a, **k)

    def spy_plain(*a, **k):
        calls["plain"] += 1
        return real_plain(*a, **k)
    ops.chamfer_from_state, ops.chamfer = spy_state, spy_plain
    try:
        for setting in ("auto", True):
            C.CHAMFER_FROM_LOSS = setting
            calls["state"] = calls["plain"] = 0
            R, t = cu(G["R"]), cu(G["t"])
            pred = [torch.cat([R[i], t[i][..., None]], dim=-1) for i in range(R.shape[0])]
            d = data_dict(G)
            out = C.rpm_intersection_loss(pred, d, lines=cu(G["rpm_lines"]))
            np.testing.assert_allclose(out['loss_chamfer'].item(), G["rpm_chamfer"], rtol=1e-5)
            np.testing.assert_allclose(out['loss_intersection'].item(), G["rpm_loss"], rtol=2e-4)
            if setting == "auto":
                assert d['_rrl_p0'] is True  # decided once for the dict, reused by the later iterations
            _, chamfer, _, _ = C.dcp_intersection_loss(data_dict(G, channel_first=True), R[0], t[0], lines=cu(G["dcp_lines"]))
            np.testing.assert_allclose(chamfer.item(), G["dcp_chamfer"], rtol=1e-5)
            bottom = torch.tensor([0.0, 0, 0, 1], device='cuda').expand(R.shape[1], 1, 4)
            gs = [torch.cat([torch.cat([R[i], t[i][..., None]], dim=-1), bottom], dim=1) for i in range(R.shape[0])]
            _, chamfer, _, _ = C.fmr_intersection_loss(gs, data_dict(G), lines=cu(G["fmr_lines"]))
            np.testing.assert_allclose(chamfer.item(), G["fmr_chamfer"], rtol=1e-5)
            # (round 5: RPM's iterations are one multi-pose evaluation -- one look at its state serves all of them)
            assert calls["plain"] == 0 and calls["state"] == (0 if C.MULTI_POSE and len(pred) > 1 else len(pred)) + \
                (1 if C.MULTI_POSE else 2)  # (DCP: one look at its state; FMR's estimates: group means of the walk's own sums)
        # a batch whose samples are NOT the triangles' first points: auto takes the standalone kernel, same value
        C.CHAMFER_FROM_LOSS = "auto"
        calls["state"] = calls["plain"] = 0
        d = data_dict(G)
        d['points_src_sample'] = d['points_src_sample'].flip(1).contiguous()  # the same cloud in another order
        out = C.rpm_intersection_loss(pred, d, lines=cu(G["rpm_lines"]))
        assert d['_rrl_p0'] is False and calls["state"] == 0 and calls["plain"] == len(pred)
        np.testing.assert_allclose(out['loss_chamfer'].item(), G["rpm_chamfer"], rtol=1e-5)
        # the dataset's flag decides without looking at the data
        d = data_dict(G)
        d['p0_rows'] = torch.zeros(3, dtype=torch.bool)
        C.rpm_intersection_loss(pred, d, lines=cu(G["rpm_lines"]))
        assert d['_rrl_p0'] is False
        C.CHAMFER_FROM_LOSS = False
        calls["state"] = 0
        C.rpm_intersection_loss(pred, data_dict(G), lines=cu(G["rpm_lines"]))
        assert calls["state"] == 0
    finally:
        C.CHAMFER_FROM_LOSS = "auto"
        ops.chamfer_from_state, ops.chamfer = real_state, real_plain


def test_fragments_draw_their_own_lines(C, G):
    """lines=None: the sampler runs with the trainer's radius convention; rows are unit
    directions or unfilled zeros, and the loss is finite and reproducible under a seed."""
    R, t = cu(G["R"][0]), cu(G["t"][0])
    d = data_dict(G, channel_first=True)
    assert C.DEVICE_RNG is False  # default: the reference's CPU stream (a drop-in keeps its RNG behaviour)
    torch.manual_seed(3)
    c0 = C.dcp_intersection_loss(d, R, t, n_lines=500)
    torch.manual_seed(3)
    c0b = C.dcp_intersection_loss(d, R, t, n_lines=500)
    assert torch.equal(c0[2], c0b[2]) and torch.equal(c0[0], c0b[0])  # reproducible under the CPU seed
    C.DEVICE_RNG = True           # opt-in: the GPU generator draws the candidates
    try:
        from rrl_hip import ops
        ops.sampler_rng(seed=3)   # (explicit: re-seeding torch with the SAME seed while nothing else drew from its CUDA
        a = C.dcp_intersection_loss(d, R, t, n_lines=2000)  # generator is invisible to the sampler, ops.sampler_rng)
        ops.sampler_rng(seed=3)
        b = C.dcp_intersection_loss(d, R, t, n_lines=2000)
    finally:
        C.DEVICE_RNG = False
    try:
        torch.manual_seed(3)
        c1 = C.draw_lines(C.bounding_radius(d['tar_box'], 0.5), d['centers'], 500, d['points_tar_sample'].transpose(2, 1).contiguous(), d['points_tar_sample'].transpose(2, 1).contiguous())
        torch.manual_seed(3)
        import loss as Lm
        c2 = Lm.Random_uniform_distribution_lines_batch_efficient_resample(
            C.bounding_radius(d['tar_box'], 0.5), d['centers'], 500, d['points_tar_sample'].transpose(2, 1).contiguous(),
            d['points_tar_sample'].transpose(2, 1).contiguous(), 'cuda')
        assert torch.equal(c1, c2)
    finally:
        C.DEVICE_RNG = False
    assert a[2].shape == (3, 2000, 6) and torch.equal(a[2], b[2]) and torch.equal(a[0], b[0])
    nrm = a[2][..., :3].norm(dim=-1)
    assert bool(((nrm - 1).abs().lt(1e-5) | nrm.eq(0)).all())
    assert np.isfinite(a[0].item()) and a[0].item() > 0


# ------------------------------------------------------------------------ the demo loop
@pytest.fixture(scope="module")
def demo():
    import importlib
    return importlib.import_module("test_demo_optimized_Lie_Algebra")


def demo_inputs(g):
    import loss as L
    data = {'bounding_box': cu(g["bbox"]), 'vertics1_tensor': cu(g["src"]),
            'vertics2_tensor': cu(g["tar"]),
            'vertics1_faces_tensor': cu(g["src_tri"]).reshape(1, -1, 3),
            'vertics2_faces_tensor': cu(g["tar_tri"]), 'centers': cu(g["centers"])}
    model = L.Reconstruction_point()
    with torch.no_grad():
        model.parameters_.copy_(torch.from_numpy(g["xi0"]))
    lines = cu(g["lines"])
    return data, model, (lambda epoch, moved: lines[epoch])


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("fixture", ["demo_trajectory.npz", "demo_trajectory_airplane.npz"])
def test_demo_trajectory(demo, tmp_path, graph, fixture):
    """8 reference epochs with the reference's recorded lines: a synthetic pair, and (round 4) a pair of the reference's
    OWN sample data (code/sample_data/airplane_data/1, N = M = 1024, prepared like its demo does)."""
    from rrl_hip import ops
    g = load_golden(fixture)
    data, model, lines_fn = demo_inputs(g)
    n = len(g["loss"])
    log = demo.ScalarLog(str(tmp_path / "log"))
    # the captured step's direct backward sums (dR, dt) with float atomics: run-to-run rounding noise of 1e-7, which at the
    # reference's data scale (the airplane pair) is enough to move a line between buckets in one run and not in the next.
    # The trajectory comparison uses the bit-reproducible backward (rrl_set_deterministic) so that it tests the path,
    # not the scheduler.
    ops.set_deterministic(True)
    try:
        hist, model = demo.test_one_case(data, str(tmp_path), writer=log, n_epoch=n, device='cuda:0',
                                         lines_fn=lines_fn, graph=graph, print_every=0, model=model)
    finally:
        ops.set_deterministic(False)
    log.close()
    assert [h[0] for h in hist] == list(range(n))
    # measured (gpurun_out/r02v_demo.txt): loss within 8.6e-4 (eager, last step) / 3.3e-5 (graph), Chamfer
    # within 1.3e-6, xi within 1.7e-5 of the reference's trajectory; see test_demo_moved_source_flips_no_label
    # Round 4 (the airplane pair; Adam's scalars now follow torch's double arithmetic): xi stays within 2.3e-6 (eager) /
    # 1.3e-6 (captured) of the reference's while no line changes its bucket.  At the reference's data scale (AABB diagonal
    # 13) the labels are noisy enough ("culling bound") that a 1e-7 difference in xi moves one line
    # between buckets somewhere in the last epochs: that epoch's loss then differs by a few 1e-3, the next Adam step by a
    # few per cent, the Chamfer by 1e-4.  So: the first five epochs tight, the tail loose.
    loss, cham = np.array([h[1] for h in hist]), np.array([h[2] for h in hist])
    if fixture == "demo_trajectory.npz":
        np.testing.assert_allclose(loss, g["loss"], rtol=2e-3)
        np.testing.assert_allclose(cham, g["chamfer"], rtol=1e-5)
        np.testing.assert_allclose(model.parameters_.detach().cpu().numpy(), g["xi"][-1], atol=1e-4)
    else:
        np.testing.assert_allclose(loss[:5], g["loss"][:5], rtol=2e-4)
        np.testing.assert_allclose(cham[:5], g["chamfer"][:5], rtol=1e-5)
        np.testing.assert_allclose(loss, g["loss"], rtol=8e-3)
        np.testing.assert_allclose(cham, g["chamfer"], rtol=5e-4)
        np.testing.assert_allclose(model.parameters_.detach().cpu().numpy(), g["xi"][-1], atol=5e-4)
    # first step: lr already halved to 1e-2 at epoch 0 -> Adam moves every coordinate by ~lr
    np.testing.assert_allclose(np.abs(g["xi"][0] - g["xi0"]), 1e-2, rtol=1e-3)
    for name in ("0.obj", "target.obj", "model.pkl", "0_transform.txt", os.path.join("log", "scalars.csv")):
        assert (tmp_path / name).exists(), name
    tr = np.loadtxt(tmp_path / "0_transform.txt")
    assert tr.shape == (3, 4) and abs(np.linalg.det(tr[:, :3]) - 1) < 1e-5
    assert demo.read_obj_vertices(str(tmp_path / "target.obj")).shape == g["tar"].shape
    rows = open(tmp_path / "log" / "scalars.csv").read().strip().splitlines()
    assert len(rows) == 1 + 2 * n


def test_graphed_demo_with_the_sampler_in_the_graph_saves_the_moved_source(demo, tmp_path):
    """Round 4: with the sampler inside the captured epoch nothing computes the moved POINTS any more (the sampler's box
    comes from the loss step's partial rows via the pose launch); a checkpoint reads the moved first points from the
    step's TRI1 field.  `0.obj` must hold the source moved by the epoch's own pose, bit for bit what ops.rigid_apply gives,
    and the optimisation must run as before (the sampler box of epoch 1 is the AABB of exactly those points)."""
    from rrl_hip import ops
    from LieAlgebra import se3
    g = load_golden("demo_trajectory.npz")
    data, model, _ = demo_inputs(g)
    xi0 = model.parameters_.detach().cpu().clone()
    hist, model = demo.test_one_case(data, str(tmp_path), n_epoch=4, n_sample_line=3000, device='cuda:0', graph=True,
                                     device_rng=True, save_every=1, print_every=0, model=model)
    assert all(h[1] is not None for h in hist)
    R, T = se3.exp3(xi0)
    want = ops.rigid_apply(data['vertics1_tensor'].reshape(1, -1, 3), R.cuda(), T.cuda()).reshape(-1, 3).cpu().numpy()
    got = demo.read_obj_vertices(str(tmp_path / "0.obj"))
    np.testing.assert_array_equal(got, want)
    later = demo.read_obj_vertices(str(tmp_path / "3.obj"))
    assert later.shape == want.shape and np.abs(later - want).max() > 1e-3  # three Adam steps moved it


def test_demo_moved_source_flips_no_label(oracle):
    """Why the trajectory is not bit-equal: the source is moved on the GPU (FMA rigid apply) where the
    reference uses torch's CPU matmul -- the moved vertices differ by <= 2 ulp.  With the REFERENCE's own
    xi of every step, that difference flips NO hit decision on the recorded line sets (counted with the
    oracle's exact scan on both versions of the moved triangles); the remaining 1e-5 .. 1e-3 deviations of
    the loss come from the ulp-level differences propagating through D, the median and 8 Adam steps."""
    from rrl_hip import ops
    from LieAlgebra import se3
    g = load_golden("demo_trajectory.npz")
    xi_prev = [g["xi0"]] + [g["xi"][k] for k in range(len(g["xi"]) - 1)]
    tri = torch.from_numpy(g["src_tri"]).reshape(-1, 3)
    flips = hits = 0
    for k, xi in enumerate(xi_prev):
        R, T = se3.exp3(torch.from_numpy(xi))
        cpu = (tri @ R.reshape(3, 3) + T.reshape(1, 3)).reshape(-1, 9).numpy()
        gpu = ops.rigid_apply(tri.reshape(1, -1, 3).cuda(), R.cuda(), T.cuda()).reshape(-1, 9).cpu().numpy()
        assert np.abs(cpu - gpu).max() <= 2.4e-7
        a, b = oracle.scan(cpu, g["lines"][k], cap=8), oracle.scan(gpu, g["lines"][k], cap=8)
        flips += int((a["count"] != b["count"]).sum())
        hits += int(a["count"].sum())
    assert flips == 0 and hits > 10000


def test_demo_skips_empty_steps(demo, tmp_path):
    """A line set without hits: the reference skips backward/step (`if loss_di is not None`)."""
    g = load_golden("demo_trajectory.npz")
    for graph in (False, True):
        data, model, _ = demo_inputs(g)
        far = torch.tensor([[1.0, 0, 0, 0, 50, 50]], device='cuda').repeat(64, 1)
        hist, model = demo.test_one_case(data, str(tmp_path), n_epoch=3, device='cuda:0',
                                         lines_fn=lambda e, m: far, graph=graph, print_every=0,
                                         model=model)
        assert all(h[1] is None for h in hist)
        np.testing.assert_array_equal(model.parameters_.detach().cpu().numpy(), g["xi0"])


@pytest.mark.parametrize("device_rng", [False, True])
def test_demo_end_to_end_reduces_chamfer(demo, tmp_path, device_rng):
    """Synthetic pair, the script's own sampler and Sample_neighs, 60 graphed epochs.  device_rng:
    the sampler (GPU generator, lines written in place), the exp map, Adam and the log row are all
    inside the captured step -- one graph launch per epoch."""
    import argparse
    args = argparse.Namespace(data_path=None, device='cuda:0', seed=5, label1='s', Save_path=str(tmp_path),
                              n_epoch=60, n_sample_line=4000, synthetic=400, graph=True, print_every=0,
                              device_rng=device_rng, save_every=0 if device_rng else 10)
    hist, model = demo.main(args)
    done = [h for h in hist if h[1] is not None]
    assert len(done) >= 50
    assert done[-1][2] < 0.8 * done[0][2], (done[0], done[-1])


def test_demo_epoch_chamfer_rides_in_the_scans_launch(demo, tmp_path, monkeypatch):
    """Round 4b: in the one-call epoch (rrl_demo_epoch) the Chamfer walk of the step's clouds is carried by the culled
    scan's launch (cull_scan_chamfer_kernel: workgroups [0, 2 B x supergroups) walk, the others scan) instead of being a
    launch of its own behind the step, and the COUNT pass of the next epoch's line sampler by the per-line launch
    (pair_count_kernel; it takes the moved source's box from the records launch's partial rows -- the sampler is software-
    pipelined across epochs through rrl_demo_epoch_args.pipeline).  Same bodies, same inputs: the whole run -- per-epoch
    loss, Chamfer value, validity, the final pose -- is bit-identical to the run with RRL_DEMO_RIDE=0 (every kernel in a
    launch of its own, the sampler at the start of its epoch), at two sizes (ragged clouds, 4 and 9 line tiles)."""
    import argparse
    from rrl_hip import ops
    out = {}
    ops.set_deterministic(True)  # (the backward's float atomics would make two runs differ by themselves)
    try:
        _rides(demo, tmp_path, monkeypatch, ops, out, argparse)
    finally:
        ops.set_deterministic(False)


def _rides(demo, tmp_path, monkeypatch, ops, out, argparse):
    for n_pts, n_lines in ((400, 4000), (1000, 9000)):
        for ride in ("1", "0"):
            monkeypatch.setenv("RRL_DEMO_RIDE", ride)
            ops._sampler_key.clear()  # (both runs re-seed the device generator from torch's seed: the same lines)
            args = argparse.Namespace(data_path=None, device='cuda:0', seed=11, label1='s', Save_path=str(tmp_path),
                                      n_epoch=25, n_sample_line=n_lines, synthetic=n_pts, graph=True, print_every=0,
                                      device_rng=True, save_every=0)
            hist, model = demo.main(args)
            out[ride] = (np.array([[np.nan if v is None else v for v in h[1:4]] for h in hist], np.float64),
                         model.parameters_.detach().cpu().numpy().copy())
        assert np.isfinite(out["1"][0][:, 1]).all() and (out["1"][0][:, 1] > 0).all()   # the monitor ran in every epoch
        np.testing.assert_array_equal(out["1"][0], out["0"][0])
        np.testing.assert_array_equal(out["1"][1], out["0"][1])


# ------------------------------------------------------- dataset files -> trainer fragment
def test_dataset_to_fragments(C, tmp_path):
    """Pairs on disk (pre_dataloader layout) -> DataLoader batch -> RPM and DCP fragments."""
    import pre_dataloader as P
    from rrl_hip import synth
    d = str(tmp_path / "pairs")
    for i in range(3):  # tar = src @ A + b plus an independent resampling: a registrable pair
        pr = synth.make_pair(80 + i, 256, 256)
        P.write_pair(d, i, 0, pr["src"], pr["tar"], pr["src_tri"].reshape(-1, 3),
                     pr["tar_tri"].reshape(-1, 3), np.concatenate([np.eye(3), np.zeros((3, 1))], 1))
    src, tar = P.list_pairs(d, range(3), range(1))
    batch = next(iter(torch.utils.data.DataLoader(P.Dataset_2021_8_29(src, tar), batch_size=3)))
    data = {k: v.cuda() for k, v in batch.items()}
    eye = torch.cat([torch.eye(3), torch.zeros(3, 1)], 1).cuda().repeat(3, 1, 1).requires_grad_(True)
    torch.manual_seed(0)
    out = C.rpm_intersection_loss([eye, eye], data, n_lines=3000)
    assert bool(out['valid'].all()) and out['lines'].shape == (3, 3000, 6)
    out['loss_intersection'].backward()
    assert torch.isfinite(eye.grad).all() and float(eye.grad.abs().sum()) > 0
    # identical poses in both iterations: per-iteration sums are equal (target scan reused in #2)
    assert torch.equal(out['per_iter'][0], out['per_iter'][1])
    # round 4: the items carry the clouds' spatial orders (pre_dataloader.kd_order, computed once per item on the host);
    # the fragments hand them to the fused op (prepared build, no cell sort) -- the same loss bits as without them, and
    # the host-side order is a valid permutation with the layout of ops.cloud_order
    assert data['order_src'].dtype == torch.int32 and data['order_src'].shape == (3, 256)
    for b_ in range(3):
        assert sorted(data['order_src'][b_].tolist()) == list(range(256))
    try:
        C.USE_ORDERS = False
        plain = C.rpm_intersection_loss([eye, eye], data, lines=out['lines'])
    finally:
        C.USE_ORDERS = True
    again = C.rpm_intersection_loss([eye, eye], data, lines=out['lines'])
    assert torch.equal(plain['loss_intersection'], again['loss_intersection']) and torch.equal(plain['per_iter'][0], out['per_iter'][0])
    from rrl_hip import ops
    # the prepared build ran with the dataset's order -- for both poses of the (round 5) multi-pose evaluation
    assert ops.last_state().dims[0] == 6
    assert torch.equal(ops.last_state().idx1[:3, :256], data['order_src']) and torch.equal(ops.last_state().idx1[3:, :256], data['order_src'])
    batch = next(iter(torch.utils.data.DataLoader(P.Dataset_2021_8_29(src, tar, DCP_True=True), batch_size=3)))
    data = {k: v.cuda() for k, v in batch.items()}
    assert data['points_src_sample'].shape == (3, 3, 256)
    torch.manual_seed(0)
    loss, chamfer, lines, ok = C.dcp_intersection_loss(data, data['R'].transpose(2, 1).contiguous(), data['T'],
                                                       n_lines=3000)
    assert bool(ok.all()) and np.isfinite(loss.item()) and np.isfinite(chamfer.item())


# ------------------------------------------------------------------------ bench.py under torch.distributed.run
def _bench_child(extra, launcher, base=("--steps", "200", "--warmup", "20", "--no-cpu-baseline", "--no-extras")):
    import json
    import subprocess
    import sys
    import socket
    from conftest import ROOT
    with socket.socket() as so:  # a free port per launch
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    cmd = ([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr",
            "127.0.0.1", "--master-port", str(port)] if launcher else [sys.executable])
    cmd += [os.path.join(ROOT, "bench.py"), "--gpus", "1", *base] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-1500:]
    return json.loads(lines[0])


def test_bench_under_torchrun_uses_rccl_in_graph():
    """The multi-GPU path with one rank, as a fresh child process launched exactly like the driver
    launches N > 1 (python -m torch.distributed.run ... bench.py --gpus 1): the direct RCCL binding
    comes up (communicator of 1 rank), the 14-float all-reduce is a node of the captured step, the
    reduced payload equals the local one.  STRUCTURAL assertions only: every timing of the children is
    reported in the line (and printed here), never compared -- a stopwatch must not decide a test."""
    run = _bench_child(["--issue", "graph", "--full"], launcher=True)
    ar = run["config"]["allreduce"]
    assert ar["reducer"] == "RcclReducer" and ar["placement"] == "inline" and ar["in_graph"] is True
    assert ar["backend"] == "nccl" and ar["rccl"]["nranks"] == 1 and ar["rccl"]["rank"] == 0
    assert run["n_gpus"] == 1 and run["scaling"] == "weak" and run["extras"]["valid"] == 8.0
    assert run["config"]["step"].startswith("loss_step") and run["config"]["issue"] == "graph"
    plain = _bench_child(["--no-dist", "--issue", "graph"], launcher=False)
    assert plain["config"]["allreduce"]["reducer"] == "PayloadReducer" and plain["config"]["allreduce"]["process_group"] is False
    assert plain["extras"]["loss_sum"] == run["extras"]["loss_sum"]          # sum over one rank == the local payload
    # the default invocation (what the driver runs at N = 1) carries the same RCCL all-reduce, inline on the step's stream
    # (how the launches are issued -- the C call of ops.LossStep or one graph replay of it -- is measured in warm-up)
    default = _bench_child([], launcher=False)
    dar = default["config"]["allreduce"]
    assert dar["reducer"] == "RcclReducer" and dar["placement"] == "inline" and default["config"]["issue"] in ("graph", "direct")
    assert dar["in_graph"] is (default["config"]["issue"] == "graph")
    assert default["extras"]["loss_sum"] == run["extras"]["loss_sum"]
    direct = _bench_child(["--issue", "direct"], launcher=True)
    assert direct["config"]["issue"] == "direct" and direct["config"]["allreduce"]["reducer"] == "RcclReducer"
    assert direct["extras"]["loss_sum"] == run["extras"]["loss_sum"]
    # the cold build of the same step: same sums, and each line carries the other build's figure at top level
    cold = _bench_child(["--cold", "--issue", "direct", "--full"], launcher=False)
    assert cold["config"]["prepared_order"] is False and "COLD" in cold["config"]["workload"]
    assert cold["extras"]["loss_sum"] == run["extras"]["loss_sum"] and cold["value_prepared"] > 0
    assert run["config"]["prepared_order"] is True and run["value_cold"] > 0 and run["ms_per_step_cold"] > 0
    # strong scaling flag: a fixed global batch sharded over the ranks (configs[2] with --global-batch 64)
    strong = _bench_child(["--global-batch", "16"], launcher=True)
    assert strong["scaling"] == "strong" and strong["config"]["global_batch"] == 16 and strong["extras"]["valid"] == 16.0
    print("ms_per_step:", {k: round(v["ms_per_step"], 4) for k, v in
                           dict(graph=run, plain=plain, default=default, direct=direct, cold=cold, b16=strong).items()})


def test_bench_line_describes_what_it_times():
    """The JSON line's headline is SURVEY 8(d)'s step (points1.grad) and says so; its top-level roofline belongs to the
    dominant kernel of the TIMED step (the culled scan) at the timed shape AND at the chip-filling B = 64 shape; the strict
    scan sits under dense_reference; the fused dR/dT op, the autograd chain and the reference trainers' literal per-sample
    loop are variants of the same line with the same loss bits; a plain `--no-dist` invocation runs without a process
    group.  No assertion here compares two wall-clock figures."""
    run = _bench_child(["--no-dist"], launcher=False, base=("--steps", "60", "--warmup", "10", "--no-cpu-baseline", "--full"))
    assert run["config"]["step"].startswith("loss_step") and "points1.grad" in run["config"]["workload"]
    assert run["config"]["prepared_order"] is True and run["config"]["prepare_us"] > 0 and "PREPARED" in run["config"]["workload"]
    assert run["config"]["allreduce"]["process_group"] is False
    rf = run["roofline"]
    assert run["config"]["chained"] is True and "CHAINED" in run["config"]["workload"]  # (round 6: records + both scans as ONE launch)
    assert rf["kernel"].startswith("cull_scan_build_kernel") and rf["bound"] == "valu" and rf["peak"] == 78.6
    assert rf["launch_ms"] > 0 and rf["executed_flops"] > 0 and rf["work_ratio"] > 10
    assert abs(rf["frac"] - rf["executed_flops"] / (rf["launch_ms"] * 1e-3) / 1e12 / rf["peak"]) < 1e-9
    assert "launch_ms_rocprof" in rf and "frac_rocprof" in rf  # (null unless the committed PMC pass is of this build)
    dr = rf["dense_reference"]
    assert dr["kernel"].startswith("scan_kernel") and dr["loss_bit_identical_to_default_mode"] is True
    assert abs(dr["frac"] - dr["algorithmic_flops_per_launch"] / (dr["launch_ms"] * 1e-3) / 1e12 / rf["peak"]) < 1e-9
    b64 = rf["at_B64"]
    assert b64["valid_samples"] == 64 and b64["executed_flops"] > 4 * rf["executed_flops"] and b64["ms_per_step"] > 0
    assert abs(b64["frac"] - b64["executed_flops"] / (b64["launch_ms"] * 1e-3) / 1e12 / rf["peak"]) < 1e-9
    v = run["variants"]
    assert run["value_cold"] == v["loss_step_cold"]["value"] and run["ms_per_step_cold"] == v["loss_step_cold"]["ms_per_step"]
    assert v["loss_step_cold"]["loss_bit_identical_to_timed_step"] is True
    assert v["fused_dRdT"]["loss_bit_identical_to_timed_step"] is True
    ag = v["points1_grad_autograd"]
    assert ag["loss_bit_identical_to_timed_step"] is True and ag["points1_grad_max_rel_diff_vs_timed_step"] < 1e-5
    assert ag["points1_grad_nonzero_rows"] == run["extras"]["points1_grad_nonzero_rows"] > 0
    assert v["dropin_loop"]["loss_sum"] == pytest.approx(ag["loss_sum"], rel=1e-6)
    assert v["dropin_loop"]["dR_max_rel_diff_vs_fused"] < 1e-5 and ag["dR_max_rel_diff_vs_fused"] < 1e-5
    assert run["extras"]["loss_sum"] == pytest.approx(ag["loss_sum"], rel=1e-6) and run["extras"]["valid"] == 8.0
    mp = run["extras"]["multi_pose"]
    assert mp.get("loss_bits_equal") is True and mp["two_poses_one_evaluation_ms"] > 0 and mp["one_pose_ms"] > 0, mp
    # round 6: the line checks ITSELF against the oracle on its own workload, and times loops whose inputs change
    pr = run["parity_in_run"]
    assert pr["ok"] is True and pr["labels_equal"] is True and pr["loss_rel_max"] <= 1e-5 and pr["grad_per_point_rel_max"] <= 1e-4, pr
    assert pr["samples"] == [0, 7] and pr["rigid_apply_rel_max"] <= 1e-6
    assert v["fresh_lines"]["chained"] is True and v["fresh_lines"]["ms_per_step"] > 0 and v["fresh_clouds_cold"]["ms_per_step"] > 0
    assert v["deterministic_grad"]["grad_bit_identical_between_calls"] is True and v["deterministic_grad"]["loss_bit_identical_to_timed_step"] is True
    assert run["config"]["break_even_steps"] is None or run["config"]["break_even_steps"] > 0
    print("ms_per_step:", {"timed": run["ms_per_step"], "cold": run["ms_per_step_cold"], "B64": b64["ms_per_step"],
                           **{k: x["ms_per_step"] for k, x in v.items()}})


def test_bench_plain_run_dumps_the_timed_outputs(tmp_path):
    """A plain run (no --full) prints the headline of exactly --steps timed steps and nothing that takes a run of its own;
    --dump-outputs writes the last timed step's outputs.  The inputs are seeded, so two runs with different step counts agree
    output for output: loss, counts and payload bit for bit, points1.grad to the rounding of the scatter's float atomics."""
    got = []
    for k, steps in enumerate((30, 50)):
        d = tmp_path / f"out{k}"
        run = _bench_child(["--dump-outputs", str(d)], launcher=False, base=("--steps", str(steps), "--warmup", "5"))
        assert run["steps"] == steps and run["ms_per_step"] > 0 and run["higher_is_better"] is True and run["dtype"] == "f32"
        assert run["value"] == pytest.approx(8 * 10000 * 3 * 8192 / (run["ms_per_step"] * 1e-3), rel=1e-9)
        for key in ("roofline", "parity_in_run", "variants", "cpu_baseline", "value_cold"):
            assert key not in run, key
        out = {f.stem: np.load(f) for f in d.glob("*.npy")}
        assert sorted(out) == ["info", "loss", "payload", "points1_grad"]
        assert all(a.dtype in (np.float32, np.float64) for a in out.values()) and sum(a.nbytes for a in out.values()) <= 64 << 20
        assert out["loss"].shape == (8,) and out["points1_grad"].shape == (8, 4096, 9) and out["info"].shape == (8, 4)
        assert float(out["payload"][0]) == run["extras"]["loss_sum"] and float(out["payload"][1]) == run["extras"]["valid"] == 8.0
        assert float(out["loss"].astype(np.float64).sum()) == pytest.approx(run["extras"]["loss_sum"], rel=1e-6)
        got.append(out)
    a, b = got
    for name in ("loss", "info", "payload"):
        assert np.array_equal(a[name], b[name]), name
    assert np.abs(a["points1_grad"] - b["points1_grad"]).max() <= 1e-5 * np.abs(a["points1_grad"]).max()
    assert (np.abs(a["points1_grad"]).sum(-1) > 0).sum() > 0


def test_fragments_multi_pose_equals_the_loop(C, G):
    """round 5: RPM's num_iter poses and FMR's last three estimates go through ONE multi-pose evaluation
    (callsites.multi_pose_loss); RRL_MULTI_POSE=0 / callsites.MULTI_POSE = False is round 4's loop, pose after pose with the
    target's scan carried over.  Per-iteration losses BIT-identical, the discounted sums and the monitors equal, gradients
    equal to the rounding of the backward's float atomics."""
    R, t = cu(G["R"], True), cu(G["t"], True)
    outs = {}
    for multi in (True, False):
        C.MULTI_POSE = multi
        try:
            R.grad = t.grad = None
            pred = [torch.cat([R[i], t[i][..., None]], dim=-1) for i in range(R.shape[0])]
            out = C.rpm_intersection_loss(pred, data_dict(G), lines=cu(G["rpm_lines"]))
            out['loss_intersection'].backward()
            bottom = torch.tensor([0.0, 0, 0, 1], device='cuda').expand(R.shape[1], 1, 4)
            g4 = torch.stack([torch.cat([torch.cat([R[i], t[i][..., None]], dim=-1), bottom], dim=1)
                              for i in range(R.shape[0])]).detach().requires_grad_(True)
            fl, fc, _, fok = C.fmr_intersection_loss([g4[i] for i in range(g4.shape[0])], data_dict(G), lines=cu(G["fmr_lines"]))
            fl.backward()
            outs[multi] = ([x.detach().clone() for x in out['per_iter']], out['loss_intersection'].detach().clone(),
                           out['loss_chamfer'].clone(), out['valid'].clone(), R.grad.clone(), t.grad.clone(),
                           fl.detach().clone(), fc.clone(), fok.clone(), g4.grad.clone())
        finally:
            C.MULTI_POSE = True
    a, b = outs[True], outs[False]
    rel = lambda x, y: float((x - y).abs().max()) <= 1e-6 * float(y.abs().max())  # noqa: E731 (sums of bit-identical instance
    for x, y in zip(a[0], b[0]):                                                   #  losses, associated differently)
        assert rel(x, y)
    assert rel(a[1], b[1]) and torch.equal(a[3].reshape(-1), b[3].reshape(-1)) and rel(a[6], b[6]) and torch.equal(a[8].reshape(-1), b[8].reshape(-1))
    assert abs(float(a[2]) - float(b[2])) <= 1e-6 * abs(float(b[2])) and abs(float(a[7]) - float(b[7])) <= 1e-6 * abs(float(b[7]))
    for i in (4, 5, 9):
        assert bool(((a[i] - b[i]).abs() <= 2e-5 * b[i].abs() + 2e-6 * float(b[i].abs().max())).all())


def test_fragment_with_a_source_that_requires_grad(C, G):
    """the multi-pose node differentiates with respect to the transforms only.  A source that requires grad must
    not silently lose its gradient: multi_pose_loss declines (None) and the fragment takes the per-pose loop, whose fused op
    returns dL/dsrc -- equal to the loop's with multi-pose switched off."""
    R, t = cu(G["R"], True), cu(G["t"], True)
    got = {}
    for multi in (True, False):
        C.MULTI_POSE = multi
        try:
            d = data_dict(G)
            d['points_based_neighs_src'] = d['points_based_neighs_src'].detach().clone().requires_grad_(True)
            pred = [torch.cat([R[i], t[i][..., None]], dim=-1) for i in range(R.shape[0])]
            if multi:
                B = d['points_tar_sample'].shape[0]
                assert C.multi_pose_loss(d['points_based_neighs_src'], pred, d['points_based_neighs_tar'].reshape(B, -1, 9),
                                         cu(G["rpm_lines"])) is None
            out = C.rpm_intersection_loss(pred, d, lines=cu(G["rpm_lines"]))
            out['loss_intersection'].backward()
            g = d['points_based_neighs_src'].grad
            assert g is not None and float(g.abs().sum()) > 0
            got[multi] = (out['loss_intersection'].detach().clone(), g.clone())
        finally:
            C.MULTI_POSE = True
    assert torch.equal(got[True][0], got[False][0])
    assert bool(((got[True][1] - got[False][1]).abs() <= 2e-5 * got[False][1].abs() + 2e-6 * float(got[False][1].abs().max())).all())


def test_bench_two_ranks_sharing_one_gpu():
    """The N > 1 HOST LOGIC of bench.py on a 1-GPU box: two ranks under `python -m torch.distributed.run --nproc-per-node 2`,
    both on cuda:0 (RRL_SHARE_GPU=1), the payload all-reduced over gloo (RRL_DIST_BACKEND=gloo: RCCL refuses two ranks on one
    device) -- the shard bounds, the collective choice of the issue / reducer placement (max over ranks), the barrier-fenced
    timing with its MAX all-reduce, rank 0's line with the WHOLE job's pairs and sums.  Throughput means nothing here (two
    processes time-slice one GPU); the structure is what is checked.  (No multi-GPU node was available to any round.)"""
    import json
    import subprocess
    import sys
    from conftest import ROOT
    env = dict(os.environ, RRL_SHARE_GPU="1", RRL_DIST_BACKEND="gloo")
    out = {}
    import socket
    for name, extra in (("weak", []), ("strong", ["--global-batch", "8"])):
        with socket.socket() as so:  # a free port per launch (a lingering TIME_WAIT socket must not fail the suite)
            so.bind(("127.0.0.1", 0))
            port = so.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "40", "--warmup", "5",
               "--no-cpu-baseline", "--no-extras", "--no-other", "--points", "1024", "--lines", "4000", "--batch", "4"] + extra
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout[-1500:]  # rank 0 alone prints
        out[name] = json.loads(lines[0])
    w, s = out["weak"], out["strong"]
    assert w["n_gpus"] == 2 and w["scaling"] == "weak" and w["config"]["global_batch"] == 8 and w["extras"]["valid"] == 8.0
    assert w["config"]["allreduce"]["backend"] == "gloo" and w["config"]["allreduce"]["reducer"] == "PayloadReducer"
    assert w["config"]["parallelism"] == "batch-shard dp2" and w["config"]["step"].startswith("loss_step")
    assert w["value"] == pytest.approx(2 * 4 * 4000 * 3 * 2048 * w["steps"] / (w["ms_per_step"] * 1e-3 * w["steps"]), rel=1e-9)
    assert s["scaling"] == "strong" and s["config"]["global_batch"] == 8 and s["extras"]["valid"] == 8.0
    assert s["extras"]["loss_sum"] > 0 and w["extras"]["loss_sum"] > 0
    print("two ranks on one GPU (gloo):", {k: round(v["ms_per_step"], 4) for k, v in out.items()})


def test_named_views_sit_at_the_librarys_offsets(oracle):
    """(B, N, M, L) = (2, 70, 130, 1030) -- N != M, a padded supergroup, two line tiles: every named view of a LossState and
    a WideState starts at the library's offset of its field, has the dtype and shape the library's field table gives
    (rrl_workspace_field) and lies inside the allocation; after a forward + backward at (1, 1, 5, 5) and at (1, 1, 9, 9)
    the state's info, status and loss views hold what ops.intersection_loss returned (info as the oracle counts it; the
    second sample has a line with more than 4 hits)."""
    from rrl_hip import ops
    B, N, M, Ll = 2, 70, 130, 1030
    g = load_golden("loss_synth_s0.npz")
    tri1, tri2 = np.stack([g["tri1"][:N]] * B), np.stack([g["tri2"][:M]] * B)
    lines = np.stack([g["lines"][:Ll], g["lines"][-Ll:]])
    tri2, lines = cu(tri2), cu(lines)

    def views_ok(st, W, ws, offsets, nbytes):
        assert len(offsets) == len(W.index)
        assert ws.numel() == nbytes == W.layout(B, N, M, Ll)[0] and offsets == W.layout(B, N, M, Ll)[1]
        for name, i in W.index.items():
            v = getattr(st, name)
            _, dtype, shape = W._field(i, st.dims)
            assert v.data_ptr() == ws.data_ptr() + offsets[i] and v.dtype == dtype and tuple(v.shape) == shape, name
            assert v.is_contiguous() and offsets[i] + v.numel() * v.element_size() <= nbytes, name
        with pytest.raises(AttributeError):
            st.no_such_field

    def is_(v, dtype, *shape):
        return v.dtype == dtype and tuple(v.shape) == shape

    for rng, kind in (((1, 1, 5, 5), ops.LossState), ((1, 1, 9, 9), ops.WideState)):
        p1 = cu(tri1, grad=True)
        loss, info, status = ops.intersection_loss(p1, tri2, lines, rng)
        st = ops.last_state()
        assert type(st) is kind and st.dims == (B, N, M, Ll, B)
        loss.sum().backward()
        assert torch.isfinite(p1.grad).all() and p1.grad.abs().sum() > 0 and int(status[0]) == 0
        for b in range(B):
            ref = oracle.loss(tri1[b], g["tri2"][:M], lines[b].cpu().numpy(), rng)
            assert info[b].tolist() == [ref["n_buckets"], ref["n_selected"], ref["n_values"], 0], (rng, b)
            assert abs(loss[b].item() - float(ref["loss"])) <= 1e-5 * abs(float(ref["loss"])), (rng, b)
        scan = st.scan if kind is ops.WideState else st
        views_ok(scan, ops._WS, scan.ws, scan.offsets, scan.nbytes)
        assert is_(scan.p0s1, torch.float32, B, 128, 4) and is_(scan.grp2, torch.float32, B, 3, 13, 4) and is_(scan.kj, torch.uint8, B, Ll)
        assert is_(scan.blkcnt, torch.int32, B * 3) and is_(scan.bsum, torch.int64, B, 16, 2) and is_(scan.vals, torch.float32, B, 2048, 16)
        assert is_(scan.gfix, torch.int64, B * (N + M) * 9 + B) and is_(scan.tri1t, torch.float32, B, N, 9)
        if kind is ops.WideState:
            views_ok(st, ops._WW, st.wws, st.woffsets, st.wnbytes)
            assert is_(st.D, torch.float32, B, Ll, 8, 8) and is_(st.rec, torch.int32, 2 * B * Ll) and is_(st.bsum, torch.int64, B, 64, 2)
        assert torch.equal(st.info, info) and torch.equal(scan.status, status) and torch.equal(st.loss, loss.detach())
        assert torch.equal(st.nbuckets, info[:, 0]) and tuple(st.info.shape) == (B, 4) and tuple(st.med.shape) == (B,)
        # ... and the same call again returns the same bits
        loss2, info2, status2 = ops.intersection_loss(p1.detach(), tri2, lines, rng)
        assert torch.equal(loss2, loss.detach()) and torch.equal(info2, info) and torch.equal(status2, status)
