"""The attention node on the GPU (include/rrl.h rrl_attention_fwd, rrl_attention_bwd, rrl_attention_scores; rrl_hip/attention.py;
DESIGN.md section 27) against the host twin of tests/attention_refs.py.

  scores  (rrl_attention_scores: the node's own gather and chain) bit for bit the twin's float32 fmaf chains times sc (compared
          as numbers: -0 == +0); -inf beyond the counts.  The row maxima the forward keeps in its workspace: the twin's, as bits.
  out     against the twin's float64 evaluation of the same z, within attention_refs.evaluate's out_bound: the expf term
          eps_k per weight, the column chain's nt 2^-24 sum |terms|, the final rounding, float32's underflow quantum.
  grads   every entry of d_q, d_k, d_v within its bound of the same derivation (the module docstring of attention_refs).
None of the bounds is measured.  The worst ratio to each bound is printed per test (pytest -s shows it)."""
import numpy as np
import pytest
import torch

import attention_refs as AR
from conftest import load_golden
from test_attention_refs_host import TRANSFORMER_FACTOR, recorded

pytestmark = pytest.mark.gpu

DKS = [1, 2, 3, 31, 32, 33, 64, 127, 128]
SHAPES = [(1, 1), (31, 33), (128, 128), (130, 257)]
HEADS = (1, 3, 4)
NAMES = ("out", "info", "d_q", "d_k", "d_v")


@pytest.fixture(scope="module")
def at():
    from rrl_hip import _lib, attention
    _lib.load()
    assert torch.cuda.is_available()
    return attention


def cuda(*xs):
    return tuple(torch.from_numpy(np.ascontiguousarray(x)).cuda() if x is not None else None for x in xs)


def counts_for(B, n):
    return None if B == 1 else [0, n, max(n // 2, 1)][:B]


def same(a, b):
    return a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def run(at, q, k, v, g, H, cq=None, ckv=None, device_counts=False, with_scores=False):
    """attend with info, and the three gradients of sum(out g) through torch.autograd -> dict of numpy (raw: the tensors)."""
    tq, tk, tv = (t.requires_grad_(True) for t in cuda(q, k, v))
    (tg,) = cuda(g)
    if device_counts:
        cq, ckv = (torch.tensor(c, dtype=torch.int32).cuda() if c is not None else None for c in (cq, ckv))
    out, info = at.attend(tq, tk, tv, H, counts_q=cq, counts_kv=ckv, with_info=True)
    assert not info.requires_grad and out.shape == q.shape
    grads = torch.autograd.grad((out * tg).sum(), (tq, tk, tv))
    raw = (out.detach(), info) + grads
    res = dict(raw=raw)
    if with_scores:
        res["scores"] = at.scores(tq, tk, H, cq, ckv).cpu().numpy()
    torch.cuda.synchronize()
    res.update({n: t.cpu().numpy() for n, t in zip(NAMES, raw)})
    return res


def check_sample(got, b, q, k, v, g, H, nq, nt, what, worst):
    """Sample b of a result against the twin, with the bounds of attention_refs; the worst ratios go into `worst`."""
    N, M = q.shape[1], k.shape[1]
    z = AR.scores(q[b], k[b], H)
    if "scores" in got:
        want = np.full((H, N, M), -np.inf, np.float32)
        want[:, :nq, :nt] = z[:, :nq, :nt]
        assert np.array_equal(got["scores"][b], want), (what, b, "scores")
    tw = AR.evaluate(z, v[b], H, nq, nt, g[b], q[b], k[b])
    assert not got["out"][b][nq:].any() and (nt > 0 or not got["out"][b].any()), (what, b, "out beyond the counts")
    assert not got["d_q"][b][nq:].any() and not got["d_k"][b][nt:].any() and not got["d_v"][b][nt:].any(), (what, b)
    if nq == 0 or nt == 0:
        assert not got["d_q"][b].any() and not got["d_k"][b].any() and not got["d_v"][b].any(), (what, b)
    for name in ("out", "d_q", "d_k", "d_v"):
        err, bound = np.abs(got[name][b].astype(np.float64) - tw[name]), tw[name + "_bound"]
        assert (err <= bound).all(), (what, b, name, float((err / np.maximum(bound, 1e-300)).max()))
        live = bound > 0
        if live.any():
            worst[name] = max(worst.get(name, 0.0), float((err[live] / bound[live]).max()))
    return tw


def check_case(at, B, H, DK, N, M, sigma, kind, seed, what, with_scores=True):
    q, k, v, g = AR.make_case(B, H, DK, N, M, sigma, kind, seed)
    cq, ckv = counts_for(B, N), counts_for(B, M)
    if cq is not None:  # what lies beyond a count is never read: poison it
        for b in range(B):
            q[b, cq[b]:], k[b, ckv[b]:], v[b, ckv[b]:] = np.nan, np.nan, np.nan
    got, again = run(at, q, k, v, g, H, cq, ckv, with_scores=with_scores), run(at, q, k, v, g, H, cq, ckv)
    for a, b2 in zip(got["raw"], again["raw"]):
        assert same(a, b2), (what, "two calls")
    assert got["info"].tolist() == [0] * B, what
    worst = {}
    for b in range(B):
        check_sample(got, b, np.nan_to_num(q), np.nan_to_num(k), np.nan_to_num(v), g, H, N if cq is None else cq[b], M if ckv is None else ckv[b],
                     what, worst)
    print(what, "worst ratio to the bound:", {n: round(x, 3) for n, x in worst.items()})
    return got


@pytest.mark.parametrize("N,M", SHAPES)
@pytest.mark.parametrize("DK", DKS)
def test_scores_bit_for_bit_out_and_gradients_within_their_bounds(at, DK, N, M):
    """Both sides of the 32-wide tile and of the 128-row workgroup, three column groups of 128 with a partial last one and an odd
    column count, odd head dimensions and those that are no multiple of 4 or 8 (the scalar gather, the padded block), 1, 3
    and 4 heads, one and three samples (ragged: counts 0 / full / half, NaN beyond them); the second call repeats the first."""
    i = DKS.index(DK) + SHAPES.index((N, M))
    for B in (1, 3):
        H = HEADS[(i + B) % 3]
        check_case(at, B, H, DK, N, M, (1.0, 4.0)[i % 2], "random", 100 + DK + N + M, (B, H, DK, N, M))


@pytest.mark.parametrize("sigma", [1.0, 4.0, 30.0])
@pytest.mark.parametrize("kind", AR.KINDS)
def test_every_kind_at_every_scale(at, kind, sigma):
    """one_hot: one weight is 1, the others underflow; equal: every row is the mean of v; sigma = 30 at DK = 32 gives scores of
    several hundred."""
    got = check_case(at, 1, 3, 32, 70, 257, sigma, kind, 12, (kind, sigma))
    if kind == "equal":
        v = AR.make_case(1, 3, 32, 70, 257, sigma, kind, 12)[2]
        mean = v[0].astype(np.float64).mean(0)
        assert np.abs(got["out"][0] - mean[None]).max() <= 257 * 2.0 ** -24 * np.abs(v[0]).mean(0).max() * 1.001 + 2.0 ** -24


# ---- the C entries, called directly ------------------------------------------------------------------------------------------
def c_call(at, q, k, v, g, H, cq=None, ckv=None, want=(True, True, True), prefill=float("nan"), info=True):
    """rrl_attention_fwd and rrl_attention_bwd on pre-filled output buffers -> dict of torch tensors (None for a NULL output)."""
    from rrl_hip import _lib, ops
    lib = _lib.load()
    tq, tk, tv, tg = cuda(q, k, v, g)
    B, N, D = q.shape
    M = k.shape[1]
    dev = tq.device
    tcq, tckv = (torch.tensor(c, dtype=torch.int32, device=dev) if c is not None else None for c in (cq, ckv))
    ws = torch.full((int(lib.rrl_attention_workspace_bytes(B, H, N, M)) // 8,), prefill, dtype=torch.float64, device=dev)
    out = torch.full((B, N, D), prefill, device=dev)
    tinfo = torch.full((B,), -7, dtype=torch.int32, device=dev) if info else None
    outs = [torch.full_like(t, prefill) if w else None for t, w in zip((tq, tk, tv), want)]
    P = ops._p
    head = (P(tq), P(tk), P(tv), P(tcq), P(tckv), P(ws), ws.numel() * 8)
    ops._run(dev, "rrl_attention_fwd", *head, P(out), P(tinfo), B, H, D // H, N, M)
    ops._run(dev, "rrl_attention_bwd", *head, P(out), P(tg), P(outs[0]), P(outs[1]), P(outs[2]), B, H, D // H, N, M)
    torch.cuda.synchronize()
    return dict(out=out, info=tinfo, d_q=outs[0], d_k=outs[1], d_v=outs[2], ws=ws.reshape(B, H, 2, N))


def test_each_gradient_output_may_be_null_and_buffers_need_no_zeroing(at):
    """Each output NULL in turn gives the others the bits of the full call; NaN and 1e30 in every output buffer and in the
    workspace beforehand change nothing; the autograd node gives the same bits as the C entries; the kept row maxima are the
    twin's, bit for bit, and the kept 1 / L is the twin's within the expf term."""
    B, H, DK, N, M = 3, 3, 33, 70, 257
    q, k, v, g = AR.make_case(B, H, DK, N, M, 4.0, "random", 21)
    cq, ckv = [70, 0, 35], [257, 5, 130]
    full = c_call(at, q, k, v, g, H, cq, ckv)
    node = run(at, q, k, v, g, H, cq, ckv)
    for i, name in enumerate(NAMES):
        assert same(full[name], node["raw"][i]), name
        assert not torch.isnan(full[name]).any(), name
    assert not torch.isnan(full["ws"]).any()
    ws = full["ws"].cpu().numpy()
    for b in range(B):
        z = AR.scores(q[b], k[b], H)
        rule = AR.forward_rule(z, v[b], H, cq[b], ckv[b])
        assert np.array_equal(ws[b, :, 0], rule["rowmax"].astype(np.float64)), b
        live = rule["L"] > 0
        assert not ws[b, :, 1][~live].any()
        ev = AR.evaluate(z, v[b], H, cq[b], ckv[b])
        ebar = (ev["w"] * ev["eps"]).sum(2)
        assert (np.abs(ws[b, :, 1][live] * rule["L"][live] - 1.0) <= 2 * ebar[live] + 2.0 ** -50).all(), b
    for skip in range(3):
        part = c_call(at, q, k, v, g, H, cq, ckv, want=tuple(i != skip for i in range(3)), prefill=1e30, info=False)
        for i, name in enumerate(("d_q", "d_k", "d_v")):
            assert (part[name] is None) if i == skip else same(part[name], full[name]), (skip, name)
        assert same(part["out"], full["out"]) and same(part["ws"], full["ws"])
    for only in range(3):
        part = c_call(at, q, k, v, g, H, cq, ckv, want=tuple(i == only for i in range(3)))
        name = ("d_q", "d_k", "d_v")[only]
        assert same(part[name], full[name]), name


def test_counts_hide_nothing(at):
    """Zero exact and zero gradient beyond count_q and for count_kv = 0; count_kv = 1 gives v_0's head slices exactly; device
    counts out of range are clamped."""
    B, H, DK, N, M = 4, 3, 16, 40, 70
    q, k, v, g = AR.make_case(B, H, DK, N, M, 4.0, "random", 22)
    got = run(at, q, k, v, g, H, [N, 17, N, 0], [M, 0, 1, M], with_scores=True)
    assert got["info"].tolist() == [0, 0, 0, 0]
    assert not got["out"][1].any() and not got["out"][3].any() and np.isneginf(got["scores"][1]).all() and np.isneginf(got["scores"][3]).all()
    for name in ("d_q", "d_k", "d_v"):
        assert not got[name][1].any() and not got[name][3].any(), name
    assert np.array_equal(got["out"][2], np.repeat(v[2, :1], N, axis=0))  # one column: its weight is exactly 1
    # (a constant softmax: ds is float32(dP) - double(delta) of the same sum, 0 to the rounding of dP's chain -- inside the bounds)
    check_sample(got, 2, q, k, v, g, H, N, 1, "count_kv = 1", {})
    assert np.abs(got["d_v"][2][0] - g[2].astype(np.float64).sum(0)).max() <= (N + 1) * 2.0 ** -24 * np.abs(g[2]).sum(0).max()
    clamped = run(at, q, k, v, g, H, [N + 5, 17, 2 ** 30, -3], [M + 1, -1, 1, M], device_counts=True)
    for a, b in zip(got["raw"], clamped["raw"]):
        assert same(a, b)


def test_nan_and_infinite_queries_set_info_only_for_their_sample(at):
    B, H, DK, N, M = 4, 3, 16, 40, 70
    q, k, v, g = AR.make_case(B, H, DK, N, M, 1.0, "random", 23)
    clean = run(at, q, k, v, g, H)
    q[1, 5, 3] = np.nan
    q[2, 39, 47] = np.inf
    q[3, 0, 20] = -np.inf
    got = run(at, q, k, v, g, H)
    assert clean["info"].tolist() == [0, 0, 0, 0] and got["info"].tolist() == [0, 1, 1, 1]
    for a, b in zip(clean["raw"], got["raw"]):
        assert same(a[0], b[0])
    got = run(at, q, k, v, g, H, [40, 5, 39, 0], None)  # (the three entries now lie beyond the counts)
    assert got["info"].tolist() == [0, 0, 0, 0]


def test_a_ragged_sample_has_the_bits_of_its_own_call(at):
    B, H, DK, N, M = 3, 4, 33, 70, 257
    q, k, v, g = AR.make_case(B, H, DK, N, M, 4.0, "random", 24)
    cq, ckv = [70, 33, 1], [M, 128, M - 1]
    batch = run(at, q, k, v, g, H, cq, ckv)
    for b in range(3):
        alone = run(at, q[b:b + 1], k[b:b + 1], v[b:b + 1], g[b:b + 1], H, cq[b:b + 1], ckv[b:b + 1])
        for a, o in zip(batch["raw"], alone["raw"]):
            assert same(a[b], o[0]), b


def test_a_captured_graph_gives_the_bits_of_the_eager_call(at):
    B, H, DK, N, M = 2, 4, 64, 70, 257
    q, k, v, g = AR.make_case(B, H, DK, N, M, 4.0, "random", 25)
    eager = run(at, q, k, v, g, H)
    tq, tk, tv = (t.requires_grad_(True) for t in cuda(q, k, v))
    (tg,) = cuda(g)

    def step():
        out = at.attend(tq, tk, tv, H)
        return (out.detach(),) + torch.autograd.grad((out * tg).sum(), (tq, tk, tv))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for _ in range(2):
        for o in outs:
            o.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for o, want in zip(outs, (eager["raw"][i] for i in (0, 2, 3, 4))):
            assert same(o, want)


def test_absent_gradients_reach_the_entry_as_null(at):
    """Only the inputs that require a gradient get one, with the bits of the full call."""
    B, H, DK, N, M = 2, 3, 16, 40, 70
    q, k, v, g = AR.make_case(B, H, DK, N, M, 1.0, "random", 26)
    full = run(at, q, k, v, g, H)
    for only in range(3):
        ts = list(cuda(q, k, v))
        ts[only].requires_grad_(True)
        (tg,) = cuda(g)
        (at.attend(*ts, H) * tg).sum().backward()
        assert same(ts[only].grad, full["raw"][2 + only]) and all(t.grad is None for i, t in enumerate(ts) if i != only)


# ---- DCP's modules -------------------------------------------------------------------------------------------------------------
def test_recorded_attention_cases(at):
    """The reference's own attention() runs (float32 and float64, CPU): the node lies within its bound of the twin, and so
    within bound + the move of the twin's scores (test_attention_refs_host.score_move) of the float64 recording."""
    from rrl_hip import callsites
    from test_attention_refs_host import CASES, score_move
    files = [load_golden(n) for n in ("attention_dcp.npz", "attention_dcp_dk128_fwd.npz")]
    golden = {key: f[key] for f in files for key in f.files}
    for name, (B, H, DK, N, M) in CASES.items():
        q, k, v = (golden[f"{name}_{x}"] for x in "qkv")
        out = callsites.dcp_attention(*cuda(q, k, v), H).cpu().numpy()
        o64 = recorded(golden, f"{name}_out")[1]
        for b in range(B):
            ev = AR.evaluate(AR.scores(q[b], k[b], H), v[b], H)
            bound = ev["out_bound"] + score_move(AR.score_bound(q[b], k[b], H), v[b], H, ev["out"]) + 1e-14
            assert (np.abs(out[b] - o64[b]) <= bound).all(), (name, b)


def test_transformer_reproduces_the_reference_recording(at):
    """attention.Transformer with the recorded state dict (strict) against the reference's CPU runs, within TRANSFORMER_FACTOR
    recorded float32-to-float64 distances (test_attention_refs_host derives the factor); MultiHeadedAttention likewise."""
    from rrl_hip import callsites
    tg = load_golden("attention_dcp_transformer.npz")
    emb, heads, ff, blocks = (int(x) for x in tg["config"])
    module = at.Transformer(emb, heads, ff, blocks)
    module.load_state_dict({str(k): torch.from_numpy(tg["sd_" + str(k)]) for k in tg["keys"]}, strict=True)
    module.cuda()
    src, tgt = cuda(tg["src"], tg["tgt"])
    src.requires_grad_(True)
    src_e, tgt_e = callsites.dcp_transformer(module, src, tgt)
    for mine, name in ((src_e, "src_embedding"), (tgt_e, "tgt_embedding")):
        r32, r64, dist = recorded(tg, name)
        e64, e32 = np.abs(mine.detach().cpu().numpy() - r64).max(), np.abs(mine.detach().cpu().numpy() - r32).max()
        print(name, "to float64", e64 / dist, "to float32", e32 / dist, "distances")
        assert mine.shape == r32.shape and e64 <= TRANSFORMER_FACTOR * dist and e32 <= TRANSFORMER_FACTOR * dist, (name, e64, e32, dist)
    (src_e.sum() + tgt_e.square().sum()).backward()   # six nodes backwards, through the torch layers to the input and the weights
    assert torch.isfinite(src.grad).all() and src.grad.abs().sum() > 0
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in module.parameters())
    g = load_golden("attention_dcp.npz")
    mha = at.MultiHeadedAttention(4, 64)
    mha.load_state_dict({str(k): torch.from_numpy(g["mha_sd_" + str(k)]) for k in g["mha_keys"]}, strict=True)
    got = mha.cuda()(*cuda(g["mha_query"], g["mha_key"], g["mha_value"])).detach().cpu().numpy()
    _, o64, dist = recorded(g, "mha_out")
    assert np.abs(got - o64).max() <= TRANSFORMER_FACTOR * dist


def test_a_call_leaves_nothing_behind(at):
    """With the cyclic collector off, a forward + backward whose results are dropped returns the allocator to where it was: no
    output, workspace or projection is held by a reference cycle through the node."""
    import gc
    import weakref
    q, k, v, g = AR.make_case(2, 4, 32, 70, 130, 1.0, "random", 27)
    tq, tk, tv = (t.requires_grad_(True) for t in cuda(q, k, v))
    (tg,) = cuda(g)
    gc.collect()
    gc.disable()
    try:
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        out = at.attend(tq, tk, tv, 4)
        ref = weakref.ref(out)
        grads = torch.autograd.grad((out * tg).sum(), (tq, tk, tv))
        del out, grads
        torch.cuda.synchronize()
        assert ref() is None and torch.cuda.memory_allocated() == base
    finally:
        gc.enable()
