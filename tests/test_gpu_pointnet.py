"""GPU checks of the PointNet encoder (include/rrl.h rrl_pointnet_fwd; rrl_hip/pointnet.py) against its
host twin (tests/pointnet_refs.py), stage by stage through the workspace views, each stage on the DEVICE's own previous stage:

  y_l            bit for bit the twin's fmaf chain on the device's h_{l-1} (the MFMA from 64 input channels upward);
  sum y, sum y^2 within m 2^-53 sum|terms| of the twin's sums of the device's y_l (m terms, fixed-order double sums);
  mu, r, a, d    bit for bit from the device's own sums (IEEE double operations, not fused);
  h, ext, f      bit for bit on the device's own statistics;  arg the twin's, evaluated on the device's y.

End to end the features are held to tests/golden/pointnet.npz: no further from the reference's float64 run than the reference's
own float32 run is, times 2.  Shapes hit the tile edges (32 points per tile, 128 per chunk, two chunks per workgroup, 32 channels per wavefront, 128 per
workgroup): N in {1, 31, 32, 33, 64, 65, 257} x B in {1, 3}.

The backward (rrl_pointnet_bwd) is held to the twin's float64 backward, with the twin given the device's own arg, statistics, a, d,
ext and kept y_l (so both evaluate one function of the same inputs and no near-tie hides behind a tolerance): every gradient
within its final rounding plus 2 depth 2^-53 sum|terms| (grad_bound below), and on the fixture's two strict cases within 4 x the
reference's own float32-to-float64 distance of that gradient (tests/golden/pointnet_grads.npz).
"""
import numpy as np
import pytest
import torch

import pointnet_refs as PR
from conftest import load_golden

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53
NS = [1, 31, 32, 33, 64, 65, 257]
FMR = ((64, 64, 64, 128), (8, 8, 8, 8, 8))
STACKS = {"fmr32": (3, FMR[0] + (32,), FMR[1]), "fmr1024": (3, FMR[0] + (1024,), FMR[1]), "narrow": (4, (8, 24, 40), (8, 8, 4))}


@pytest.fixture(scope="module")
def pn():
    from rrl_hip import pointnet
    return pointnet


def cuda(*arrays):
    out = tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)
    return out[0] if len(out) == 1 else out


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.uint8).numpy().tobytes() if t.numel() else b""


def cloud(B, N, c0, seed=0, duplicates=True):
    rs = np.random.default_rng([seed, B, N, c0])
    p = rs.uniform(-1.0, 1.0, (B, N, c0)).astype(np.float32)
    if duplicates and N >= 33:   # equal points: equal chains, the lowest index must win
        p[:, 17] = p[:, 5]
        p[:, N - 1] = p[:, 5]
    return p


def run(pn, pts, prm, groups, ws=None, eps=1e-5):
    with torch.no_grad():
        return pn._forward(cuda(pts), [cuda(p) for p in prm], tuple(groups), eps, ws=ws)


def check_stages(pn, pts, prm, groups):
    """Every stage of every sample against the twin on the device's previous stage; returns the worst ratio of a sum to its bound."""
    B, N, c0 = pts.shape
    layers = PR.split(prm)
    widths = tuple(W.shape[0] for W, *_ in layers)
    feat, arg, info, ws = run(pn, pts, prm, groups)
    v = pn.workspace_views(ws, B, N, c0, widths, groups)
    stat, coef, ext = v["stat"].cpu().numpy(), v["coef"].cpu().numpy(), v["ext"].cpu().numpy()
    ys = [y.cpu().numpy() for y in v["y"]]
    feat, arg = feat.cpu().numpy(), arg.cpu().numpy()
    assert info.tolist() == [0] * B and v["flag"].tolist() == [0] * B
    worst = 0.0
    for b in range(B):
        h, c_at, g_at = np.ascontiguousarray(pts[b].T), 0, 0
        for l, ((W, bias, gamma, beta), G) in enumerate(zip(layers, groups)):
            c, last = W.shape[0], l + 1 == len(layers)
            y = PR.chain(W, bias, h)
            if not last:
                assert np.array_equal(y.view(np.uint32), ys[l][b].view(np.uint32)), (b, l)
            st = PR.stats(y, G)
            s, ss, mu, r = (stat[b, g_at:g_at + G, i] for i in range(4))
            abs_ss = (y.astype(np.float64) ** 2).reshape(G, -1).sum(1)
            assert (np.abs(s - st["s"]) <= st["m"] * U53 * st["abs_s"]).all() and (np.abs(ss - st["ss"]) <= st["m"] * U53 * abs_ss).all(), (b, l)
            worst = max(worst, float((np.abs(s - st["s"]) / (st["m"] * U53 * st["abs_s"])).max()),
                        float((np.abs(ss - st["ss"]) / (st["m"] * U53 * abs_ss)).max()))
            m = float(st["m"])
            mu_t = s / m
            r_t = 1.0 / np.sqrt(np.maximum(0.0, ss / m - mu_t * mu_t) + 1e-5)
            assert np.array_equal(mu, mu_t) and np.array_equal(r, r_t), (b, l)
            a_t, d_t = PR.coef(gamma, beta, mu, r)
            a, d = coef[b, c_at:c_at + c, 0], coef[b, c_at:c_at + c, 1]
            assert np.array_equal(a, a_t) and np.array_equal(d, d_t), (b, l)
            if last:
                e_t, arg_t, f_t = PR.pool(y, a, d)
                assert np.array_equal(e_t.view(np.uint32), ext[b].view(np.uint32)), b
                assert np.array_equal(f_t.view(np.uint32), feat[b].view(np.uint32)), b
                assert np.array_equal(arg_t, arg[b]), b
            else:
                h = PR.act(ys[l][b], a, d)
            c_at += c
            g_at += G
    return worst


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("stack", list(STACKS))
def test_forward_stage_by_stage(pn, stack, N, B):
    c0, widths, groups = STACKS[stack]
    prm = PR.make_stack(c0, widths, groups, seed=N)
    worst = check_stages(pn, cloud(B, N, c0, seed=1), prm, groups)
    print(f"{stack} N = {N} B = {B}: worst |sum - twin's| / (m 2^-53 sum|terms|) = {worst:.4f}")


def test_forward_rpm_prepool(pn):
    prm = PR.make_stack(4, pn.RPM_WIDTHS, pn.RPM_GROUPS, seed=3)
    check_stages(pn, cloud(2, 65, 4, seed=2), prm, pn.RPM_GROUPS)
    net = pn.Encoder.rpm_prepool().cuda()
    with torch.no_grad():
        f = net(cuda(cloud(2, 65, 4, seed=2)))
    assert f.shape == (2, 1024) and torch.isfinite(f).all()


def test_special_channels_and_duplicates_are_in_the_cases(pn):
    """What the stage test relies on: the random stacks carry a gamma < 0 and a gamma = 0 channel in the last layer, the clouds
    duplicated points, and on the device the gamma < 0 channel takes the minimum's index, the duplicate's first occurrence wins."""
    c0, widths, groups = STACKS["narrow"]
    prm = PR.make_stack(c0, widths, groups, seed=65)
    assert prm[-2][1] < 0 and prm[-2][2] == 0
    pts = cloud(1, 65, c0, seed=1)
    assert np.array_equal(pts[0, 17], pts[0, 5]) and np.array_equal(pts[0, 64], pts[0, 5])
    feat, arg, info, ws = run(pn, pts, prm, groups)
    twin = PR.forward(pts[0], prm, groups)
    assert twin["arg"][1] == twin["y"][-1][1].argmin() and not np.isin(arg.cpu().numpy(), (17, 64)).any()
    assert feat[0, 2].item() == np.float32(max(0.0, float(prm[-1][2])))    # a = 0: the feature is max(0, beta)


@pytest.mark.parametrize("name", ["b2_n64_k32", "b3_n33_k64", "b2_n130_k64", "b1_n257_k1024"])
def test_end_to_end_against_the_references_float64_run(pn, name):
    golden = load_golden("pointnet.npz")
    p, w = PR.fixture_case(golden, name)
    from rrl_hip import callsites
    net = callsites.fmr_encoder(golden[f"{name}_f64"].shape[1], state_dict=w)
    with torch.no_grad():
        f, info, arg = net(cuda(p), with_info=True, with_arg=True)
    dist, ref = np.abs(f.cpu().numpy().astype(np.float64) - golden[f"{name}_f64"]).max(), float(golden[f"{name}_dist"])
    print(f"{name}: device {dist:.3e}, reference's float32 {ref:.3e}, ratio {dist / ref:.3f}")
    assert info.tolist() == [0] * p.shape[0] and dist <= 2.0 * ref, (dist, ref)
    if name in ("b2_n64_k32", "b3_n33_k64"):   # drawn without near-ties: the pooled point is the recording's
        on = golden[f"{name}_f64"] > 0
        assert np.array_equal(arg.cpu().numpy()[on], golden[f"{name}_arg"][on])


# ---- house checks ----------------------------------------------------------------------------------------------------------
def test_every_byte_is_written_and_a_second_call_gives_the_same_bits(pn):
    """Two calls into workspaces prefilled with different bytes (all ones: NaN in either float width; zeros) leave the same bytes."""
    c0, widths, groups = STACKS["fmr32"]
    prm = PR.make_stack(c0, widths, groups, seed=7)
    pts = cloud(3, 257, c0)
    nbytes, _ = pn.workspace_layout(3, 257, c0, widths, groups)
    assert nbytes % 4 == 0
    outs = []
    for fill in (0xFF, 0x00, 0xFF):
        ws = torch.full((nbytes,), fill, dtype=torch.uint8, device="cuda").view(torch.float32)
        feat, arg, info, ws = run(pn, pts, prm, groups, ws=ws)
        outs.append((bits(feat), bits(arg), bits(info), bits(ws)))
    assert outs[0] == outs[1] == outs[2]
    assert not np.isnan(np.frombuffer(outs[0][0], np.float32)).any()


def test_a_sample_of_a_batch_is_its_own_single_call(pn):
    for stack, N in (("fmr1024", 257), ("narrow", 65)):
        c0, widths, groups = STACKS[stack]
        prm = PR.make_stack(c0, widths, groups, seed=9)
        pts = cloud(3, N, c0, seed=4)
        feat, arg, _, _ = run(pn, pts, prm, groups)
        for b in range(3):
            f1, a1, _, _ = run(pn, pts[b:b + 1], prm, groups)
            assert bits(f1[0]) == bits(feat[b]) and bits(a1[0]) == bits(arg[b]), (stack, b)


def test_graph_replay_equals_eager(pn):
    from rrl_hip.graph import GraphedStep
    c0, widths, groups = STACKS["fmr1024"]
    prm = [cuda(p) for p in PR.make_stack(c0, widths, groups, seed=11)]
    pts = cuda(cloud(2, 300, c0))
    with torch.no_grad():
        eager = pn.encode(pts, prm, groups)
        step = GraphedStep(lambda: pn.encode(pts, prm, groups))
        replayed = step().clone()
    assert bits(replayed) == bits(eager)


def test_info_is_optional_and_a_nan_point_flags_its_own_sample_only(pn):
    from rrl_hip import ops
    c0, widths, groups = STACKS["fmr32"]
    prm = PR.make_stack(c0, widths, groups, seed=13)
    pts = cloud(3, 65, c0)
    clean = run(pn, pts, prm, groups)[0]
    for poison in (np.nan, np.inf, -np.inf):
        bad = pts.copy()
        bad[1, 40, 2] = poison
        feat, arg, info, _ = run(pn, bad, prm, groups)
        assert info.tolist() == [0, 1, 0] and torch.isnan(feat[1]).all()
        assert bits(feat[0]) == bits(clean[0]) and bits(feat[2]) == bits(clean[2])
        assert ((arg >= 0) & (arg < 65)).all()
    for which in (0, 9, 18, 19):   # a weight, a bias, gamma and beta of the last layer: every sample
        hurt = [p.copy() for p in prm]
        hurt[which].reshape(-1)[0] = np.nan
        feat, _, info, _ = run(pn, pts, hurt, groups)
        assert info.tolist() == [1, 1, 1] and torch.isnan(feat).all(), which
    # info = NULL through the C entry: the same features
    dp, dprm = cuda(pts), [cuda(p) for p in prm]
    import ctypes
    nbytes, _ = pn.workspace_layout(3, 65, c0, widths, groups)
    ws = torch.empty(nbytes // 4, device="cuda")
    feat, arg = torch.empty(3, 32, device="cuda"), torch.empty(3, 32, dtype=torch.int32, device="cuda")
    ptrs = (ctypes.c_void_p * 20)(*[p.data_ptr() for p in dprm])
    P = ops._p
    ops._run(dp.device, "rrl_pointnet_fwd", P(dp), ptrs, pn._ints(widths), pn._ints(groups), 1e-5, P(ws), nbytes, P(feat), P(arg), None, 3, 65, c0, 5)
    assert bits(feat) == bits(clean)


def test_short_and_misaligned_workspaces_are_refused(pn):
    from rrl_hip._lib import RRLError
    c0, widths, groups = STACKS["narrow"]
    prm = PR.make_stack(c0, widths, groups)
    pts = cloud(1, 33, c0)
    nbytes, _ = pn.workspace_layout(1, 33, c0, widths, groups)
    with pytest.raises(RRLError, match="-3"):
        run(pn, pts, prm, groups, ws=torch.empty(nbytes // 4 - 1, device="cuda"))
    with pytest.raises(RRLError, match="-3"):
        run(pn, pts, prm, groups, ws=torch.empty(nbytes // 4 + 2, device="cuda")[1:])
    run(pn, pts, prm, groups, ws=torch.empty(nbytes // 4, device="cuda"))


# ---- the backward --------------------------------------------------------------------------------------------------------------
U24 = 2.0 ** -24
GRAD_NAMES = ("dW", "db", "dgamma", "dbeta")


def device_backward(pn, pts, prm, groups, g, **kw):
    """forward + backward through the raw entries -> (d_points, [parameter gradients], feat, arg, info, workspace views)."""
    B, N, c0 = pts.shape
    widths = tuple(PR.split(prm)[l][0].shape[0] for l in range(len(groups)))
    dp, dprm = cuda(pts), [cuda(p) for p in prm]
    with torch.no_grad():
        feat, arg, info, ws = pn._forward(dp, dprm, tuple(groups), 1e-5)
        d_points, d_prm = pn._backward(dp, dprm, tuple(groups), ws, arg, cuda(g), **kw)
    return d_points, d_prm, feat, arg, info, pn.workspace_views(ws, B, N, c0, widths, groups)


def twin_on_device_state(pts, prm, groups, g, v, arg, absmode=False):
    """The twin's backward of every sample, given the DEVICE's own kept y_l, statistics, a, d, ext and arg; parameter gradients
    summed over the batch."""
    B = pts.shape[0]
    widths = [W.shape[0] for W, *_ in PR.split(prm)]
    stat, coef, ext = v["stat"].cpu().numpy(), v["coef"].cpu().numpy(), v["ext"].cpu().numpy()
    ys = [y.cpu().numpy() for y in v["y"]]
    runs = []
    for b in range(B):
        mu, r, a, d, c_at, g_at = [], [], [], [], 0, 0
        for c, G in zip(widths, groups):
            mu.append(stat[b, g_at:g_at + G, 2]); r.append(stat[b, g_at:g_at + G, 3])
            a.append(coef[b, c_at:c_at + c, 0]); d.append(coef[b, c_at:c_at + c, 1])
            c_at += c
            g_at += G
        runs.append(PR.backward(pts[b], prm, groups, [y[b] for y in ys], mu, r, a, d, ext[b], arg[b], g[b], absmode))
    out = {"p": np.stack([x["d_points"] for x in runs])}
    for i in range(4 * len(groups)):
        out[i] = sum(x[GRAD_NAMES[i % 4]][i // 4] for x in runs)
    return out


def grad_bound(twin, mags, key, depth):
    """|device - twin| for one gradient: the final rounding to float32 (2^-24 |entry|, 2^-149 below the normal range) plus the
    double arithmetic behind it -- every path from the inputs to an output is at most `depth` double operations long, each off by at
    most 2^-53 of the magnitudes it combines, and the twin's absmode pass carries exactly those magnitudes through the same linear
    maps: 2 depth 2^-53 sum|terms| (the 2: the twin's own rounding, in another order)."""
    return U24 * np.abs(twin[key]) + 2.0 ** -149 + 2 * depth * U53 * mags[key]


def check_backward(pn, pts, prm, groups, g):
    B, N, _ = pts.shape
    d_points, d_prm, feat, arg, info, v = device_backward(pn, pts, prm, groups, g, fill=float("nan"))
    arg = arg.cpu().numpy()
    twin = twin_on_device_state(pts, prm, groups, g, v, arg)
    mags = twin_on_device_state(pts, prm, groups, g, v, arg, absmode=True)
    widths = [W.shape[0] for W, *_ in PR.split(prm)]
    depth = len(groups) * (128 * N + max(widths) + 16) + B * N + 16
    got = {"p": d_points.cpu().numpy()}
    got.update({i: t.cpu().numpy().reshape(twin[i].shape) for i, t in enumerate(d_prm)})
    worst = 0.0
    for key in twin:
        assert not np.isnan(got[key]).any(), key          # (pre-filled with NaN: every element written)
        err, bound = np.abs(got[key].astype(np.float64) - twin[key]), grad_bound(twin, mags, key, depth)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (key, float((err / bound).max()))
    return worst


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("stack", list(STACKS))
def test_backward_against_the_twin_on_the_devices_own_forward(pn, stack, N, B):
    c0, widths, groups = STACKS[stack]
    prm = PR.make_stack(c0, widths, groups, seed=N)
    g = np.random.default_rng([N, B]).standard_normal((B, widths[-1])).astype(np.float32)
    worst = check_backward(pn, cloud(B, N, c0, seed=1), prm, groups, g)
    print(f"backward {stack} N = {N} B = {B}: worst |gradient - twin| / bound = {worst:.3f}")


def test_backward_rpm_prepool(pn):
    prm = PR.make_stack(4, pn.RPM_WIDTHS, pn.RPM_GROUPS, seed=3)
    g = np.random.default_rng(8).standard_normal((2, 1024)).astype(np.float32)
    check_backward(pn, cloud(2, 65, 4, seed=2), prm, pn.RPM_GROUPS, g)


@pytest.mark.parametrize("name", ["b2_n64_k32", "b3_n33_k64"])
def test_gradients_against_the_references_float64_run(pn, name):
    """Every gradient within 4 x the reference's recorded float32-to-float64 distance of that gradient (the factor section 23's
    closed-loop test uses for this kind of comparison), through the module and torch's autograd."""
    golden, grads = load_golden("pointnet.npz"), load_golden("pointnet_grads.npz")
    p, w = PR.fixture_case(golden, name)
    from rrl_hip import callsites
    net = callsites.fmr_encoder(golden[f"{name}_f64"].shape[1], state_dict=w)
    pts = cuda(p).requires_grad_(True)
    f, arg = net(pts, with_arg=True)
    on = golden[f"{name}_f64"] > 0
    assert np.array_equal(arg.cpu().numpy()[on], golden[f"{name}_arg"][on])
    got = torch.autograd.grad((f * cuda(grads[f"{name}_g"])).sum(), [pts] + list(net.parameters()))
    worst = 0.0
    for key, mine in zip(["p"] + [k for k, _ in net.named_parameters()], got):
        d64, d32 = grads[f"{name}_d64_{key}"], grads[f"{name}_d32_{key}"]
        err, ref = np.abs(mine.cpu().numpy().astype(np.float64) - d64).max(), np.abs(d32.astype(np.float64) - d64).max()
        worst = max(worst, err / ref)
        assert mine.shape == d64.shape and err <= 4 * ref, (key, err, ref)
    print(f"{name}: worst gradient distance / the reference's own float32-to-float64 distance = {worst:.3f}")


def test_backward_each_output_null_in_turn_and_the_same_bits_twice(pn):
    c0, widths, groups = STACKS["narrow"]
    prm = PR.make_stack(c0, widths, groups, seed=21)
    pts, g = cloud(3, 65, c0, seed=5), np.random.default_rng(4).standard_normal((3, 40)).astype(np.float32)
    full_p, full, *_ = device_backward(pn, pts, prm, groups, g)
    again_p, again, *_ = device_backward(pn, pts, prm, groups, g)
    assert bits(full_p) == bits(again_p) and all(bits(a) == bits(b) for a, b in zip(full, again))
    n = len(prm)
    for skip in range(-1, n):       # -1: d_points NULL
        want = [i != skip for i in range(n)]
        d_points, d_prm, *_ = device_backward(pn, pts, prm, groups, g, want_points=skip != -1, want=want, fill=float("nan"))
        assert (d_points is None) == (skip == -1) and (d_points is None or bits(d_points) == bits(full_p))
        for i, (a, b) in enumerate(zip(d_prm, full)):
            assert (a is None) == (i == skip) and (a is None or bits(a) == bits(b)), (skip, i)
    d_points, d_prm, *_ = device_backward(pn, pts, prm, groups, g, want=[False] * n)      # d_params NULL altogether
    assert bits(d_points) == bits(full_p) and all(d is None for d in d_prm)
    only_w, *_ = device_backward(pn, pts, prm, groups, g, want_points=False, want=[i == 4 for i in range(n)])[1:2]
    assert bits(only_w[4]) == bits(full[4])
    for b in range(3):              # d_points of sample b = its own B = 1 call
        one_p, *_ = device_backward(pn, pts[b:b + 1], prm, groups, g[b:b + 1])
        assert bits(one_p[0]) == bits(full_p[b]), b


def test_backward_of_a_flagged_sample_is_nan_and_leaves_the_others_points(pn):
    c0, widths, groups = STACKS["fmr32"]
    prm = PR.make_stack(c0, widths, groups, seed=13)
    pts, g = cloud(3, 65, c0), np.random.default_rng(6).standard_normal((3, 32)).astype(np.float32)
    clean_p, *_ = device_backward(pn, pts, prm, groups, g)
    bad = pts.copy()
    bad[1, 40, 2] = np.nan
    d_points, d_prm, feat, arg, info, _ = device_backward(pn, bad, prm, groups, g)
    assert info.tolist() == [0, 1, 0] and torch.isnan(d_points[1]).all() and all(torch.isnan(d).all() for d in d_prm)
    assert bits(d_points[0]) == bits(clean_p[0]) and bits(d_points[2]) == bits(clean_p[2])


def test_the_node_through_autograd_and_a_captured_graph(pn):
    """The module's forward + backward through torch's autograd gives the raw entries' bits; captured, it replays them."""
    from rrl_hip.graph import GraphedStep
    c0, widths, groups = STACKS["fmr1024"]
    prm = PR.make_stack(c0, widths, groups, seed=11)
    pts, g = cloud(2, 130, c0), np.random.default_rng(2).standard_normal((2, 1024)).astype(np.float32)
    raw_p, raw, *_ = device_backward(pn, pts, prm, groups, g)
    leaves = [cuda(pts).requires_grad_(True)] + [cuda(p).requires_grad_(True) for p in prm]
    dg = cuda(g)

    def step():
        return torch.autograd.grad((pn.encode(leaves[0], leaves[1:], groups) * dg).sum(), leaves)
    eager = step()
    assert bits(eager[0]) == bits(raw_p) and all(bits(a) == bits(b) for a, b in zip(eager[1:], raw))
    only = torch.autograd.grad((pn.encode(leaves[0].detach(), [leaves[1]] + [t.detach() for t in leaves[2:]], groups) * dg).sum(), leaves[1])
    assert bits(only[0]) == bits(raw[0])          # absent gradients reach the entry as NULL
    eager = [t.clone() for t in eager]
    graph = GraphedStep(step)
    replayed = [t.clone() for t in graph()]
    assert all(bits(a) == bits(b) for a, b in zip(replayed, eager))


def test_a_short_backward_workspace_is_refused(pn):
    from rrl_hip._lib import RRLError
    c0, widths, groups = STACKS["narrow"]
    prm, pts, g = PR.make_stack(c0, widths, groups), cloud(1, 33, c0), np.ones((1, 40), np.float32)
    n = int(pn._lib.load().rrl_pointnet_bwd_workspace_bytes(1, 33, c0, 3, pn._ints(widths), pn._ints(groups))) // 8
    with pytest.raises(RRLError, match="-3"):
        device_backward(pn, pts, prm, groups, g, bws=torch.empty(n - 1, dtype=torch.float64, device="cuda"))
    device_backward(pn, pts, prm, groups, g, bws=torch.empty(n, dtype=torch.float64, device="cuda"))


def test_closed_loop_fmr_ic_algo_with_the_library_encoder():
    """fmr_ic.npz's weight-carrying case through callsites.fmr_ic_algo with callsites.fmr_encoder loaded from that fixture: every
    recorded pose within 2 x the recorded loop_dist (test_gpu_fmr_head.py's bound); the captured call replays the eager bits."""
    from rrl_hip import callsites
    from rrl_hip.graph import GraphedStep
    golden = load_golden("fmr_ic.npz")
    name = str(golden["weights"])
    c = {k[len(name) + 1:]: golden[k] for k in golden.files if k.startswith(name + "_")}
    dist, maxiter, xtol = float(c["loop_dist"]), int(c["maxiter"]), float(c["xtol"])
    assert 0 < dist <= 1e-3
    net = callsites.fmr_encoder(c["f0"].shape[1], state_dict={k[2:]: v for k, v in c.items() if k.startswith("w_")})
    p0, p1, dt = cuda(c["p0"], c["p1"], c["dt"])
    with torch.no_grad():
        r, g, series, stop, info = callsites.fmr_ic_algo(net, p0, p1, maxiter=maxiter, xtol=xtol, dt=dt[:1])
        err = np.abs(series.cpu().numpy() - c["g_out"]).max()
        print(f"closed loop: max |pose - recording| = {err:.3e}, the recording's float32-float64 distance {dist:.3e}, ratio to 2 x {err / (2 * dist):.3f}")
        assert info.tolist() == [0] * p0.shape[0] and stop.tolist() == [0] and err <= 2 * dist
        step = GraphedStep(lambda: callsites.fmr_ic_algo(net, p0, p1, maxiter=maxiter, xtol=xtol, dt=dt[:1])[2])
        replayed = step().clone()
    assert bits(replayed) == bits(series)
