"""The grouped PointNet on the device (include/rrl.h rrl_pointnet_group_fwd / _bwd) against its host twin
(tests/pointnet_group_refs.py), one stage at a time through the workspace views, each stage on the DEVICE's own previous stage:
every hidden y bit for bit (the float32 fmaf chain is exact arithmetic on stated operands), the group sums within m 2^-53
sum|terms| of the twin's (m terms, fixed-order double additions), mu, r, a, d, ext, arg and out bit for bit on the device's own
sums and y.  The backward is held to the twin's float64 backward given the device's own arg, statistics, a, d, ext and kept y_l:
every gradient within its final rounding plus 2 depth 2^-53 sum|terms| (depth: the longest chain of double operations from an
input to an output, L (128 P + c_max + 16) + B P + 16 as in section 24 with the P = N S positions for N), and on the fixture's
gradient cases within 4 x the recording's own float32-to-float64 distance.  Shapes: points that straddle the 32-position tiles
(S = 20, 33, 64, 128), S = 1, N = 1, P below one chunk, widths that are multiples of no tile, the plain-fmaf path, two layers.
"""
import functools

import numpy as np
import pytest
import torch

import pointnet_group_refs as GP
import pointnet_refs as PR
from conftest import load_golden

pytestmark = pytest.mark.gpu

U24, U53 = 2.0 ** -24, 2.0 ** -53
G3 = (8, 8, 8)
# (N, S, c0, widths, groups)
SHAPES = {
    "n5_s20": (5, 20, 10, (96, 96, 192), G3),                  # P below one chunk, points straddle tiles
    "n7_s64": (7, 64, 10, (96, 96, 192), G3),
    "n9_s33": (9, 33, 3, (32, 32, 64), G3),                    # plain-fmaf path, odd S
    "n3_s128": (3, 128, 16, (64, 128, 40), (8, 8, 5)),
    "n33_s1": (33, 1, 4, (65, 65, 30), (5, 5, 3)),             # odd input channel count, S = 1
    "n1_s7": (1, 7, 10, (96, 192), (8, 8)),                    # two layers, N = 1
    "rpm130": (130, 16, 10, (96, 96, 192), G3),                # the recorded case
}
GRAD_NAMES = ("dW", "db", "dgamma", "dbeta")


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


@functools.lru_cache(maxsize=None)
def inputs(name, B):
    """(x (B, N, S, c0), params, g (B, K, N)) of a case; the recorded case reads the fixtures, the others are drawn: slot 3 of every
    point repeats slot 1 where S > 3 (ball-query's padding: equal slots, the lowest must win), the last layer carries a gamma < 0
    and a gamma = 0 channel (pointnet_refs.make_stack)."""
    N, S, c0, widths, groups = SHAPES[name]
    rs = np.random.default_rng([B, N, S, c0])
    if name == "rpm130":
        rec = GP.rpm_raw_case(load_golden("ball_query_rpm.npz"))
        x = rec[[0, 1, 0][:B]] if B > 1 else rec[:1]
        prm = GP.rpm_params(GP.fixture_weights(load_golden("pointnet_group.npz"), "rpm130"))
    else:
        x = rs.uniform(-1.0, 1.0, (B, N, S, c0)).astype(np.float32)
        if S > 3:
            x[:, :, 3] = x[:, :, 1]
        prm = PR.make_stack(c0, widths, groups, seed=N + S)
    g = rs.standard_normal((B, widths[-1], N)).astype(np.float32)
    return np.ascontiguousarray(x), prm, g


def run(pn, x, prm, groups, ws=None, eps=1e-5):
    with torch.no_grad():
        return pn._group_forward(cuda(x), [cuda(p) for p in prm], tuple(groups), eps, ws=ws)


def device_backward(pn, x, prm, groups, g, **kw):
    """forward + backward through the raw entries -> (d_x, [parameter gradients], out, arg, info, workspace views)."""
    B, N, S, c0 = x.shape
    widths = tuple(W.shape[0] for W, *_ in PR.split(prm))
    dx, dprm = cuda(x), [cuda(p) for p in prm]
    with torch.no_grad():
        out, arg, info, ws = pn._group_forward(dx, dprm, tuple(groups), 1e-5)
        d_x, d_prm = pn._group_backward(dx, dprm, tuple(groups), ws, arg, cuda(g), **kw)
    return d_x, d_prm, out, arg, info, pn.group_workspace_views(ws, B, N, S, c0, widths, groups)


def kept(v, widths, groups, b):
    """mu, r [per layer (G,)], a, d [per layer (c,)] of sample b from the workspace views (numpy)."""
    mu, r, a, d, c_at, g_at = [], [], [], [], 0, 0
    for c, G in zip(widths, groups):
        mu.append(v["stat"][b, g_at:g_at + G, 2]); r.append(v["stat"][b, g_at:g_at + G, 3])
        a.append(v["coef"][b, c_at:c_at + c, 0]); d.append(v["coef"][b, c_at:c_at + c, 1])
        c_at += c
        g_at += G
    return mu, r, a, d


def numpy_views(v):
    return dict(stat=v["stat"].cpu().numpy(), coef=v["coef"].cpu().numpy(), ext=v["ext"].cpu().numpy(), flag=v["flag"].cpu().numpy(),
                y=[y.cpu().numpy() for y in v["y"]])


def check_stages(x, prm, groups, out, arg, info, v):
    """Every stage of every sample against the twin on the device's previous stage; returns the worst ratio of a sum to its bound."""
    B, N, S, c0 = x.shape
    layers = PR.split(prm)
    assert info.tolist() == [0] * B and v["flag"].tolist() == [0] * B
    worst = 0.0
    for b in range(B):
        h, c_at, g_at = np.ascontiguousarray(x[b].reshape(N * S, c0).T), 0, 0
        for l, ((W, bias, gamma, beta), G) in enumerate(zip(layers, groups)):
            c, last = W.shape[0], l + 1 == len(layers)
            y = PR.chain(W, bias, h)
            if not last:
                assert np.array_equal(y.view(np.uint32), v["y"][l][b].view(np.uint32)), (b, l)
            st = PR.stats(y, G)
            s, ss, mu, r = (v["stat"][b, g_at:g_at + G, i] for i in range(4))
            abs_ss = (y.astype(np.float64) ** 2).reshape(G, -1).sum(1)
            bs, bss = st["m"] * U53 * st["abs_s"], st["m"] * U53 * abs_ss
            worst = max(worst, float((np.abs(s - st["s"]) / bs).max()), float((np.abs(ss - st["ss"]) / bss).max()))
            assert (np.abs(s - st["s"]) <= bs).all() and (np.abs(ss - st["ss"]) <= bss).all(), (b, l)
            m = float(st["m"])
            assert m == (c // G) * N * S
            mu_t = s / m
            r_t = 1.0 / np.sqrt(np.maximum(0.0, ss / m - mu_t * mu_t) + 1e-5)
            assert np.array_equal(mu, mu_t) and np.array_equal(r, r_t), (b, l)
            a_t, d_t = PR.coef(gamma, beta, mu, r)
            a, d = v["coef"][b, c_at:c_at + c, 0], v["coef"][b, c_at:c_at + c, 1]
            assert np.array_equal(a, a_t) and np.array_equal(d, d_t), (b, l)
            if last:
                e_t, arg_t, o_t = GP.pool_points(y, a, d, S)
                assert np.array_equal(e_t.view(np.uint32), v["ext"][b].view(np.uint32)), b
                assert np.array_equal(arg_t, arg[b]), b
                assert np.array_equal(o_t.view(np.uint32), out[b].view(np.uint32)), b
            else:
                h = PR.act(v["y"][l][b], a, d)
            c_at += c
            g_at += G
    return worst


def twin_on_device_state(x, prm, groups, g, v, arg, absmode=False):
    """The twin's backward of every sample given the DEVICE's own kept y_l, statistics, a, d, ext and arg; parameter gradients
    summed over the batch."""
    widths = [W.shape[0] for W, *_ in PR.split(prm)]
    runs = []
    for b in range(x.shape[0]):
        mu, r, a, d = kept(v, widths, groups, b)
        runs.append(GP.backward(x[b], prm, groups, [y[b] for y in v["y"]], mu, r, a, d, v["ext"][b], arg[b], g[b], absmode))
    out = {"x": np.stack([q["d_x"] for q in runs])}
    for i in range(4 * len(groups)):
        out[i] = sum(q[GRAD_NAMES[i % 4]][i // 4] for q in runs)
    return out


def grad_bound(twin, mags, key, depth):
    """|device - twin| for one gradient: the final rounding to float32 (2^-24 |entry|, 2^-149 below the normal range) plus the
    double arithmetic behind it -- depth double operations at most on any path, each off by at most 2^-53 of the magnitudes it
    combines, which the twin's absmode pass carries through the same linear maps: 2 depth 2^-53 sum|terms| = depth 2^-52 sum|terms|."""
    return U24 * np.abs(twin[key]) + 2.0 ** -149 + 2 * depth * U53 * mags[key]


def depth_of(x, widths):
    B, N, S, _ = x.shape
    return len(widths) * (128 * N * S + max(widths) + 16) + B * N * S + 16


@functools.lru_cache(maxsize=None)
def device_case(name, B):
    """One forward + backward with every gradient of a case, outputs pre-filled with NaN, and the twin's two passes on the device's
    forward: computed once, shared by the stage test and the gradient tests."""
    from rrl_hip import pointnet as pn
    x, prm, g = inputs(name, B)
    groups = SHAPES[name][4]
    d_x, d_prm, out, arg, info, v = device_backward(pn, x, prm, groups, g, fill=float("nan"))
    v, arg = numpy_views(v), arg.cpu().numpy()
    got = {"x": d_x.cpu().numpy()}
    got.update({i: t.cpu().numpy() for i, t in enumerate(d_prm)})
    twin = twin_on_device_state(x, prm, groups, g, v, arg)
    mags = twin_on_device_state(x, prm, groups, g, v, arg, absmode=True)
    return dict(x=x, prm=prm, g=g, groups=groups, out=out.cpu().numpy(), arg=arg, info=info.cpu().numpy(), v=v, got=got, twin=twin, mags=mags)


def assert_gradients(got, c, keys=None):
    depth = depth_of(c["x"], [W.shape[0] for W, *_ in PR.split(c["prm"])])
    worst = 0.0
    for key in (c["twin"] if keys is None else keys):
        val = got[key].astype(np.float64).reshape(c["twin"][key].shape)
        assert not np.isnan(val).any(), key          # (pre-filled with NaN: every element written)
        err, bound = np.abs(val - c["twin"][key]), grad_bound(c["twin"], c["mags"], key, depth)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (key, float((err / bound).max()))
    return worst


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name", list(SHAPES))
def test_forward_stage_by_stage(name, B):
    c = device_case(name, B)
    worst = check_stages(c["x"], c["prm"], c["groups"], c["out"], c["arg"], c["info"], c["v"])
    print(f"{name} B = {B}: worst |sum - twin's| / (m 2^-53 sum|terms|) = {worst:.4f}")


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name", list(SHAPES))
def test_every_gradient_against_the_twin_on_the_devices_forward(name, B):
    c = device_case(name, B)
    worst = assert_gradients(c["got"], c)
    print(f"{name} B = {B}: worst |gradient - twin's| / bound = {worst:.4f}")


@pytest.mark.parametrize("name", ["n1_s7", "n5_s20"])
def test_each_gradient_alone(pn, name):
    """d_x and each of the 4 L parameter gradients asked for alone (the others NULL): within the same bound, and the bits of the
    call that asks for all; no gradient at all is served too."""
    c = device_case(name, 1)
    L = len(c["groups"])
    for i in [None] + list(range(4 * L)):
        want = [j == i for j in range(4 * L)]
        d_x, d_prm, *_ = device_backward(pn, c["x"], c["prm"], c["groups"], c["g"], want_x=i is None, want=want, fill=float("nan"))
        key = "x" if i is None else i
        got = {key: (d_x if i is None else d_prm[i]).cpu().numpy()}
        assert_gradients(got, c, keys=[key])
        assert got[key].tobytes() == c["got"][key].tobytes(), key
        assert all(d is None for j, d in enumerate(d_prm) if j != i) and (d_x is None) == (i is not None)
    d_x, d_prm, *_ = device_backward(pn, c["x"], c["prm"], c["groups"], c["g"], want_x=False, want=[False] * (4 * L))
    assert d_x is None and all(d is None for d in d_prm)


def test_duplicated_slots_pool_the_lowest_and_the_special_channels(pn):
    c = device_case("n7_s64", 1)
    x, prm = c["x"], c["prm"]
    assert np.array_equal(x[:, :, 3], x[:, :, 1]) and prm[-2][1] < 0 and prm[-2][2] == 0
    assert not (c["arg"] == 3).any() and (c["arg"] == 1).any()           # a copy never wins over its first occurrence
    assert (c["out"][0, 2] == np.float32(max(0.0, float(prm[-1][2])))).all()    # a = 0: the output is max(0, beta)
    rec = device_case("rpm130", 1)
    same = (rec["x"][0][:, 1:] == rec["x"][0][:, :-1]).all(-1)            # (N, S - 1): slot s + 1 repeats slot s
    hit = np.zeros(same.shape[0], bool)
    for n, s in zip(*np.nonzero(same)):
        assert not (rec["arg"][0][:, n] == s + 1).any()
        hit[n] = True
    assert hit.any()


def test_end_to_end_against_the_recording(pn):
    golden = load_golden("pointnet_group.npz")
    net = pn.GroupedEncoder.rpm_feat_prepool()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in GP.fixture_weights(golden, "rpm130").items()}, strict=True)
    net = net.cuda()
    x = GP.rpm_raw_case(load_golden("ball_query_rpm.npz"))
    with torch.no_grad():
        out, info = net(cuda(x), with_info=True)
    dist, ref = np.abs(out.cpu().numpy().astype(np.float64) - golden["rpm130_f64"]).max(), float(golden["rpm130_dist"])
    print(f"rpm130: device {dist:.3e}, recording's float32 {ref:.3e}, ratio {dist / ref:.3f}")
    assert out.shape == (2, 192, 130) and info.tolist() == [0, 0] and dist <= 2.0 * ref, (dist, ref)


@pytest.mark.parametrize("name", ["b2_n5_s20_f96", "b2_n7_s64_f32"])
def test_gradients_through_autograd_against_the_recording(pn, name):
    fx = load_golden("pointnet_group_grads.npz")
    fd = int(name.rsplit("_f", 1)[1])
    net = pn.GroupedEncoder.rpm_feat_prepool(10, fd)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in GP.fixture_weights(fx, name).items()}, strict=True)
    net = net.cuda()
    x = cuda(fx[f"{name}_x"]).requires_grad_(True)
    out, arg = net(x, with_arg=True)
    on = fx[f"{name}_f64"] > 0
    assert np.array_equal(arg.cpu().numpy()[on], fx[f"{name}_arg"][on])           # drawn without near-ties
    assert np.abs(out.detach().cpu().numpy().astype(np.float64) - fx[f"{name}_f64"]).max() <= 2.0 * float(fx[f"{name}_dist"])
    named = dict(net.named_parameters())
    grads = torch.autograd.grad((out * cuda(fx[f"{name}_g"])).sum(), [x] + list(named.values()))
    for key, val in zip(["x"] + list(named), grads):
        d32, d64 = fx[f"{name}_d32_{key}"].astype(np.float64), fx[f"{name}_d64_{key}"]
        own, err = np.abs(d32 - d64).max(), np.abs(val.cpu().numpy().astype(np.float64) - d64).max()
        print(f"{name} {key}: device {err:.3e}, recording's float32 {own:.3e}")
        assert err <= 4.0 * own, key


# ---- house checks ----------------------------------------------------------------------------------------------------------
def test_every_byte_is_written_and_a_second_call_gives_the_same_bits(pn):
    x, prm, g = inputs("n9_s33", 3)
    N, S, c0, widths, groups = SHAPES["n9_s33"]
    nbytes, _ = pn.group_workspace_layout(3, N, S, c0, widths, groups)
    assert nbytes % 4 == 0
    outs = []
    for fill in (0xFF, 0x00, 0xFF):
        ws = torch.full((nbytes,), fill, dtype=torch.uint8, device="cuda").view(torch.float32)
        out, arg, info, ws = run(pn, x, prm, groups, ws=ws)
        outs.append((bits(out), bits(arg), bits(info), bits(ws)))
    assert outs[0] == outs[1] == outs[2]
    assert not np.isnan(np.frombuffer(outs[0][0], np.float32)).any()
    a = device_backward(pn, x, prm, groups, g)
    b = device_backward(pn, x, prm, groups, g)
    assert bits(a[0]) == bits(b[0]) and all(bits(p) == bits(q) for p, q in zip(a[1], b[1]))


@pytest.mark.parametrize("name", ["n7_s64", "n9_s33"])
def test_a_sample_of_a_batch_is_its_own_single_call(pn, name):
    x, prm, g = inputs(name, 3)
    groups = SHAPES[name][4]
    d_x, _, out, arg, _, _ = device_backward(pn, x, prm, groups, g)
    for b in range(3):
        d1, _, o1, a1, _, _ = device_backward(pn, x[b:b + 1], prm, groups, g[b:b + 1])
        assert bits(o1[0]) == bits(out[b]) and bits(a1[0]) == bits(arg[b]) and bits(d1[0]) == bits(d_x[b]), (name, b)


def test_a_nan_flags_its_own_sample_only(pn):
    x, prm, g = inputs("n5_s20", 3)
    groups = SHAPES["n5_s20"][4]
    clean = device_backward(pn, x, prm, groups, g)
    bad = x.copy()
    bad[1, 2, 3, 0] = np.nan
    d_x, d_prm, out, arg, info, v = device_backward(pn, bad, prm, groups, g)
    assert info.tolist() == [0, 1, 0] and v["flag"].tolist() == [0, 1, 0]
    assert torch.isnan(out[1]).all() and bits(out[0]) == bits(clean[2][0]) and bits(out[2]) == bits(clean[2][2])
    assert int(arg.min()) >= 0 and int(arg.max()) < 20
    assert torch.isnan(d_x[1]).all() and bits(d_x[0]) == bits(clean[0][0]) and bits(d_x[2]) == bits(clean[0][2])
    assert all(torch.isnan(p).all() for p in d_prm)
    with torch.no_grad():                                     # info is optional for the C entry
        dx, dprm = cuda(x), [cuda(p) for p in prm]
        N, S, c0, widths, _ = SHAPES["n5_s20"]
        out2 = torch.empty(3, widths[-1], N, device="cuda")
        arg2 = torch.empty(3, widths[-1], N, dtype=torch.int32, device="cuda")
        nbytes, _ = pn.group_workspace_layout(3, N, S, c0, widths, groups)
        ws = torch.empty(nbytes // 4, device="cuda")
        import ctypes
        from rrl_hip import ops
        ints = lambda t: (ctypes.c_int32 * len(t))(*t)  # noqa: E731
        ptrs = (ctypes.c_void_p * (4 * len(groups)))(*[p.data_ptr() for p in dprm])
        ops._run(dx.device, "rrl_pointnet_group_fwd", ops._p(dx), ptrs, ints(widths), ints(groups), 1e-5, ops._p(ws), nbytes, ops._p(out2),
                 ops._p(arg2), None, 3, N, S, c0, len(groups))
    assert bits(out2) == bits(clean[2])


def test_the_node_through_autograd_and_a_captured_graph(pn):
    """The node through torch's autograd gives the raw entries' bits, an absent gradient reaches the entry as NULL, and the
    captured forward + backward replays the eager bits (rrl_hip/graph.py)."""
    from rrl_hip.graph import GraphedStep
    x, prm, g = inputs("n7_s64", 3)
    groups = SHAPES["n7_s64"][4]
    raw_x, raw, raw_out, *_ = device_backward(pn, x, prm, groups, g)
    leaves = [cuda(x).requires_grad_(True)] + [cuda(p).requires_grad_(True) for p in prm]
    dg = cuda(g)

    def step():
        return torch.autograd.grad((pn.encode_grouped(leaves[0], leaves[1:], groups) * dg).sum(), leaves)
    eager = step()
    assert bits(eager[0]) == bits(raw_x) and all(bits(a) == bits(b) for a, b in zip(eager[1:], raw))
    only = torch.autograd.grad((pn.encode_grouped(leaves[0].detach(), [leaves[1]] + [t.detach() for t in leaves[2:]], groups) * dg).sum(), leaves[1])
    assert bits(only[0]) == bits(raw[0])
    eager = [t.clone() for t in eager]
    graph = GraphedStep(step)
    replayed = [t.clone() for t in graph()]
    assert all(bits(a) == bits(b) for a, b in zip(replayed, eager))
    with torch.no_grad():
        fwd = GraphedStep(lambda: pn.encode_grouped(leaves[0], leaves[1:], groups))
        assert bits(fwd().clone()) == bits(raw_out)


def test_refusals(pn):
    from rrl_hip._lib import RRLError
    x, prm, g = inputs("n5_s20", 1)
    N, S, c0, widths, groups = SHAPES["n5_s20"]
    nbytes, _ = pn.group_workspace_layout(1, N, S, c0, widths, groups)
    with pytest.raises(RRLError, match="-3"):
        run(pn, x, prm, groups, ws=torch.empty(nbytes // 4 - 1, device="cuda"))
    with pytest.raises(RRLError, match="-3"):
        run(pn, x, prm, groups, ws=torch.empty(nbytes // 4 + 2, device="cuda")[1:])
    out, arg, info, ws = run(pn, x, prm, groups, ws=torch.empty(nbytes // 4, device="cuda"))
    with pytest.raises(RRLError, match="-3"):
        pn._group_backward(cuda(x), [cuda(p) for p in prm], groups, ws, arg, cuda(g), bws=torch.empty(8, dtype=torch.float64, device="cuda"))
    with pytest.raises(RRLError, match="-1"):                      # a shape the C entry refuses although the tensors exist
        pn._group_forward(torch.zeros(1, 2, 129, 10, device="cuda"), [cuda(p) for p in prm], groups, 1e-5, ws=torch.empty(64, device="cuda"))
    dprm = [cuda(p) for p in prm]
    for bad in (torch.zeros(1, N, S, device="cuda"), torch.zeros(1, N, 129, c0, device="cuda"), torch.zeros(1, N, S, 17, device="cuda"),
                torch.zeros(1, N, S, c0 - 1, device="cuda")):
        with pytest.raises(ValueError):
            pn.encode_grouped(bad, dprm, groups)
    with pytest.raises(ValueError):
        pn.encode_grouped(cuda(x), dprm, (8, 8, 7))
    with pytest.raises(ValueError):
        pn.encode_grouped(cuda(x), dprm[:8], groups)
    with pytest.raises(ValueError):
        pn.encode_grouped(cuda(x), dprm, groups, eps=0.0)
    with pytest.raises(TypeError):
        pn.encode_grouped(x, dprm, groups)


def test_rpm_feat_extractor_against_eager_torch(pn):
    """callsites.rpm_feat_extractor with a torch postpool against the same modules in eager torch on the GPU (the reference's
    formulation, rpm/models/feature_nets.py:184-203), within the forward allowance: both are float32 evaluations of one function,
    so the device may be no further from the float64 evaluation than 2 x eager torch's own float32 run is."""
    from rrl_hip import callsites
    fx = load_golden("ball_query_rpm.npz")
    xyz, normals = cuda(fx["sphere_b2_130_xyz"]), cuda(fx["sphere_b2_130_normals"])
    torch.manual_seed(3)
    net = pn.GroupedEncoder.rpm_feat_prepool(10, 32).cuda()
    nn = torch.nn
    postpool = nn.Sequential(nn.Conv1d(64, 64, 1), nn.GroupNorm(8, 64), nn.ReLU(), nn.Conv1d(64, 32, 1), nn.GroupNorm(8, 32), nn.ReLU(),
                             nn.Conv1d(32, 32, 1)).cuda()
    with torch.no_grad():
        got = callsites.rpm_feat_extractor(net, postpool, xyz, normals, ("xyz", "dxyz", "ppf"), radius=0.3, nsample=16)
        raw = callsites.rpm_raw_features(xyz, normals, ("xyz", "dxyz", "ppf"), 0.3, 16)

        def eager(dtype):
            pre, post = (m.to(dtype) for m in (net.prepool, postpool))
            pooled = torch.max(pre(raw.to(dtype).permute(0, 3, 2, 1)), 2)[0]
            out = post(pooled).permute(0, 2, 1)
            return out / torch.norm(out, dim=-1, keepdim=True)
        e32 = eager(torch.float32).double()
        e64 = eager(torch.float64)
        net.float(), postpool.float()
    own, err = float((e32 - e64).abs().max()), float((got.double() - e64).abs().max())
    print(f"rpm_feat_extractor: device {err:.3e}, eager float32 {own:.3e}")
    assert got.shape == (2, 130, 32) and err <= 2.0 * own
