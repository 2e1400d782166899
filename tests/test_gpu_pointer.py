"""The softmax pointer on the GPU (include/rrl.h rrl_pointer_fwd, rrl_pointer_bwd; rrl_hip/pointer.py)
against the host twin of tests/pointer_refs.py.

Bounds, from the arithmetic rule, none measured:
  scores  bit for bit the twin's float32 fmaf chains times sc (compared as numbers: -0 == +0); -inf beyond the counts.
  corr    against the twin's float64 head from the same z: with w_k the float64 weights and eps_k = 2^-22 + 2^-23 |z_k - M_j|,
          |corr_j - twin| <= 2 sum_k w_k eps_k |x_k - corr_j| + 2^-24 |corr_j|.  A term carries an expf ulp and the rounding of its
          float32 argument twice -- once in its (row, slice) state, once in the slice's factor -- in numerator and denominator.
  grads   per entry (1.001 n 2^-24 + max_k eps_k + 2^-22) sum|terms| + 2^-24 |entry|: n the length of the float32 chain (the
          sample's valid columns for d_src_emb, its valid rows for d_tgt_emb, 0 for d_tgt, a double sum), sum|terms| the twin's
          sum with every term replaced by its magnitude; plus float32's underflow quantum per term (pointer_refs.grad_bound:
          about 1e-42 here), which a bound made of relative roundings does not cover.
The worst ratio to each bound is printed per test (pytest -s shows it)."""
import numpy as np
import pytest
import torch

import kabsch_refs as KR
import pointer_refs as PR
from conftest import load_golden
from test_pointer_refs_host import CASES as GOLDEN_CASES
from test_pointer_refs_host import recorded_corr_bound

pytestmark = pytest.mark.gpu

CS = [1, 2, 3, 31, 32, 33, 64, 512]
SHAPES = [(1, 1), (2, 3), (31, 33), (32, 32), (33, 31), (63, 65), (64, 64), (65, 63), (130, 257)]
U23 = 2.0 ** -23


@pytest.fixture(scope="module")
def pt():
    from rrl_hip import _lib, pointer
    _lib.load()
    assert torch.cuda.is_available()
    return pointer


def cuda(*xs):
    return tuple(torch.from_numpy(np.ascontiguousarray(x)).cuda() if x is not None else None for x in xs)


def counts_for(B, n):
    return None if B == 1 else [0, n, max(n // 2, 1)][:B]


def run(pt, se, te, x, g, cs=None, ct=None, device_counts=False):
    """soft_pointer with scores and info, and the three gradients of sum(corr g) through torch.autograd -> dict of numpy."""
    tse, tte, tx = (t.requires_grad_(True) for t in cuda(se, te, x))
    (tg,) = cuda(g)
    if device_counts:
        cs, ct = (torch.tensor(c, dtype=torch.int32).cuda() if c is not None else None for c in (cs, ct))
    corr, info, z = pt.soft_pointer(tse, tte, tx, counts_src=cs, counts_tgt=ct, with_info=True, return_scores=True)
    assert not z.requires_grad and not info.requires_grad and corr.shape == (se.shape[0], 3, se.shape[2])
    grads = torch.autograd.grad((corr * tg).sum(), (tse, tte, tx))
    torch.cuda.synchronize()
    raw = (corr.detach(), info, z) + grads
    names = ("corr", "info", "scores", "d_src_emb", "d_tgt_emb", "d_tgt")
    return dict(raw=raw, **{n: t.cpu().numpy() for n, t in zip(names, raw)})


def check_sample(got, b, se, te, x, g, ns, nt, what, worst, z=None):
    """Sample b of a result against the twin, with the bounds of the file header; the worst ratios go into `worst`."""
    N, M = se.shape[2], te.shape[2]
    z = PR.scores(se[b], te[b]) if z is None else z
    want = np.full((N, M), -np.inf, np.float32)
    want[:ns, :nt] = z[:ns, :nt]
    assert np.array_equal(got["scores"][b], want), (what, b, "scores")
    tw = PR.head(z, x[b], ns, nt, g[b], se[b], te[b])
    assert not got["corr"][b][:, ns:].any() and (nt > 0 or not got["corr"][b].any()), (what, b, "corr beyond the counts")
    err = np.abs(got["corr"][b].astype(np.float64) - tw["corr"])
    assert (err <= tw["corr_bound"]).all(), (what, b, "corr", (err / np.maximum(tw["corr_bound"], 1e-300)).max())
    ratios = [("corr", err, tw["corr_bound"])]
    biggest = lambda v: float(np.abs(v).max()) if v.size else 0.0  # noqa: E731
    for name, n, terms, other in (("d_src_emb", nt, nt, biggest(te[b][:, :nt])), ("d_tgt_emb", ns, ns, biggest(se[b][:, :ns])),
                                  ("d_tgt", 0, ns, biggest(g[b][:, :ns]))):
        bound = PR.grad_bound(tw, name, n, terms, other)
        err = np.abs(got[name][b].astype(np.float64) - tw[name])
        assert (err <= bound).all(), (what, b, name, (err / np.maximum(bound, 1e-300)).max())
        ratios.append((name, err, bound))
    assert not got["d_src_emb"][b][:, ns:].any() and not got["d_tgt_emb"][b][:, nt:].any() and not got["d_tgt"][b][:, nt:].any()
    if ns == 0 or nt == 0:
        assert not got["d_src_emb"][b].any() and not got["d_tgt_emb"][b].any() and not got["d_tgt"][b].any()
    for name, err, bound in ratios:
        live = bound > 0
        if live.any():
            worst[name] = max(worst.get(name, 0.0), float((err[live] / bound[live]).max()))
    return tw


def check_case(pt, C, N, M, B, sigma, kind, seed, what):
    se, te, x, g = PR.make_case(C, N, M, B, sigma, kind, seed)
    cs, ct = counts_for(B, N), counts_for(B, M)
    if cs is not None:  # what lies beyond a count is never read: poison it
        for b in range(B):
            se[b, :, cs[b]:], te[b, :, ct[b]:], x[b, :, ct[b]:] = np.nan, np.nan, np.nan
    got, again = run(pt, se, te, x, g, cs, ct), run(pt, se, te, x, g, cs, ct)
    for a, b2 in zip(got["raw"], again["raw"]):
        assert a.cpu().numpy().tobytes() == b2.cpu().numpy().tobytes(), (what, "two calls")
    assert got["info"].tolist() == [0] * B, what
    worst = {}
    for b in range(B):
        check_sample(got, b, np.nan_to_num(se), np.nan_to_num(te), np.nan_to_num(x), g, N if cs is None else cs[b], M if ct is None else ct[b],
                     what, worst)
    print(what, "worst ratio to the bound:", {k: round(v, 3) for k, v in worst.items()})
    return got


@pytest.mark.parametrize("N,M", SHAPES)
@pytest.mark.parametrize("C", CS)
def test_scores_bit_for_bit_corr_and_gradients_within_their_bounds(pt, C, N, M):
    """Both sides of the 32-wide tile, of the two-tile pass and of the 128-row workgroup, odd channel counts, one and three
    samples (ragged: counts 0 / full / half, NaN beyond them); the second call repeats the first bit for bit."""
    for B in (1, 3):
        check_case(pt, C, N, M, B, (1.0, 4.0)[(C + N) % 2], "random", 100 + C + N + M, (C, N, M, B))


def test_the_largest_channel_count(pt):
    check_case(pt, 1024, 33, 65, 1, 1.0, "random", 7, (1024, 33, 65, 1))
    check_case(pt, 1023, 33, 65, 3, 1.0, "random", 8, (1023, 33, 65, 3))


def test_three_slices_with_a_partial_last_one(pt):
    M = 2 * pt.SLICE + 37
    for B in (1, 3):
        check_case(pt, 33, 70, M, B, 4.0, "random", 9, (33, 70, M, B))
    check_case(pt, 8, 5, 3 * pt.SLICE, 1, 4.0, "random", 10, (8, 5, 3 * pt.SLICE, 1))
    check_case(pt, 8, 5, pt.SLICE + 1, 1, 4.0, "random", 11, (8, 5, pt.SLICE + 1, 1))


@pytest.mark.parametrize("sigma", [1.0, 4.0, 30.0])
@pytest.mark.parametrize("kind", PR.KINDS)
def test_every_kind_at_every_scale(pt, kind, sigma):
    """ascending: the maximum rises from tile to tile and slice to slice; one_hot: one weight is 1, the others underflow;
    equal: the column mean; sigma = 30 at C = 64 gives scores of several hundred."""
    M = 2 * pt.SLICE + 37
    got = check_case(pt, 64, 70, M, 1, sigma, kind, 12, (kind, sigma))
    if kind == "equal":
        x = PR.make_case(64, 70, M, 1, sigma, kind, 12)[2]
        mean = x[0].astype(np.float64).mean(1)
        assert np.abs(got["corr"][0] - mean[:, None]).max() <= 2 * 2.0 ** -22 * np.abs(x[0] - mean[:, None]).max() + 2.0 ** -23


# ---- the C entries, called directly ------------------------------------------------------------------------------------------
def c_call(pt, se, te, x, g, cs=None, ct=None, want=(True, True, True), prefill=float("nan"), scores=True):
    """rrl_pointer_fwd and rrl_pointer_bwd on pre-filled output buffers -> dict of torch tensors (None for a NULL output)."""
    from rrl_hip import _lib, ops
    lib = _lib.load()
    tse, tte, tx, tg = cuda(se, te, x, g)
    B, C, N = se.shape
    M = te.shape[2]
    dev = tse.device
    tcs, tct = (torch.tensor(c, dtype=torch.int32, device=dev) if c is not None else None for c in (cs, ct))
    ws = torch.full((int(lib.rrl_pointer_workspace_bytes(B, C, N, M)) // 8,), prefill, dtype=torch.float64, device=dev)
    corr = torch.full((B, 3, N), prefill, device=dev)
    z = torch.full((B, N, M), prefill, device=dev) if scores else None
    info = torch.full((B,), -7, dtype=torch.int32, device=dev)
    outs = [torch.full_like(t, prefill) if w else None for t, w in zip((tse, tte, tx), want)]
    P = ops._p
    head = (P(tse), P(tte), P(tx), P(tcs), P(tct), P(ws), ws.numel() * 8)
    ops._run(dev, "rrl_pointer_fwd", *head, P(corr), P(z), P(info), B, C, N, M)
    ops._run(dev, "rrl_pointer_bwd", *head, P(tg), P(outs[0]), P(outs[1]), P(outs[2]), B, C, N, M)
    torch.cuda.synchronize()
    return dict(corr=corr, scores=z, info=info, d_src_emb=outs[0], d_tgt_emb=outs[1], d_tgt=outs[2])


def same(a, b):
    return a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def test_each_gradient_output_may_be_null_and_buffers_need_no_zeroing(pt):
    """Each output NULL in turn gives the others the bits of the full call; NaN and 1e30 in every output buffer and in the
    workspace beforehand change nothing; the autograd node gives the same bits as the C entries."""
    se, te, x, g = PR.make_case(33, 70, 2 * pt.SLICE + 37, 3, 4.0, "random", 21)
    cs, ct = [70, 0, 35], [2 * pt.SLICE + 37, 5, 130]
    full = c_call(pt, se, te, x, g, cs, ct)
    node = run(pt, se, te, x, g, cs, ct)
    for i, name in enumerate(("corr", "info", "scores", "d_src_emb", "d_tgt_emb", "d_tgt")):
        assert same(full[name], node["raw"][i]), name
        assert not torch.isnan(full[name]).any(), name
    for skip in range(3):
        part = c_call(pt, se, te, x, g, cs, ct, want=tuple(i != skip for i in range(3)), prefill=1e30, scores=False)
        for i, name in enumerate(("d_src_emb", "d_tgt_emb", "d_tgt")):
            assert (part[name] is None) if i == skip else same(part[name], full[name]), (skip, name)
        assert same(part["corr"], full["corr"]) and same(part["info"], full["info"])
    only = c_call(pt, se, te, x, g, cs, ct, want=(False, False, True))
    assert same(only["d_tgt"], full["d_tgt"])


def test_counts_hide_nothing(pt):
    """Zero exact and zero gradient beyond count_src and for count_tgt = 0; count_tgt = 1 gives x_0 exactly; device counts out
    of range are clamped."""
    N, M = 40, 70
    se, te, x, g = PR.make_case(16, N, M, 4, 4.0, "random", 22)
    got = run(pt, se, te, x, g, [N, 17, N, 0], [M, 0, 1, M])
    assert got["info"].tolist() == [0, 0, 0, 0]
    assert not got["corr"][1].any() and not got["corr"][3].any() and np.isneginf(got["scores"][1]).all() and np.isneginf(got["scores"][3]).all()
    for name in ("d_src_emb", "d_tgt_emb", "d_tgt"):
        assert not got[name][1].any() and not got[name][3].any(), name
    assert np.array_equal(got["corr"][2], np.repeat(x[2, :, :1], N, axis=1))  # one column: its weight is exactly 1
    assert not got["d_src_emb"][2].any() and not got["d_tgt_emb"][2].any()  # (a constant softmax: ds = 0)
    assert np.abs(got["d_tgt"][2][:, 0] - g[2].astype(np.float64).sum(1)).max() <= 2.0 ** -22 * np.abs(g[2]).sum(1).max()
    clamped = run(pt, se, te, x, g, [N + 5, 17, 2 ** 30, -3], [M + 1, -1, 1, M], device_counts=True)
    for a, b in zip(got["raw"], clamped["raw"]):
        assert same(a, b)


def test_nan_and_infinite_embeddings_set_info_only_for_their_sample(pt):
    se, te, x, g = PR.make_case(16, 40, 70, 4, 1.0, "random", 23)
    clean = run(pt, se, te, x, g)
    se[1, 3, 5] = np.nan
    te[2, 0, 69] = np.inf
    se[3, 2, 39] = -np.inf
    got = run(pt, se, te, x, g)
    assert clean["info"].tolist() == [0, 0, 0, 0] and got["info"].tolist() == [0, 1, 1, 1]
    for a, b in zip(clean["raw"], got["raw"]):
        assert same(a[0], b[0])
    got = run(pt, se, te, x, g, [40, 5, 40, 39], [70, 70, 69, 70])  # (the three entries now lie beyond the counts)
    assert got["info"].tolist() == [0, 0, 0, 0]


def test_a_ragged_sample_has_the_bits_of_its_own_call(pt):
    N, M = 70, 2 * pt.SLICE + 37
    se, te, x, g = PR.make_case(33, N, M, 3, 4.0, "random", 24)
    cs, ct = [70, 33, 1], [M, pt.SLICE, M - 1]
    batch = run(pt, se, te, x, g, cs, ct)
    for b in range(3):
        alone = run(pt, se[b:b + 1], te[b:b + 1], x[b:b + 1], g[b:b + 1], cs[b:b + 1], ct[b:b + 1])
        for a, o in zip(batch["raw"], alone["raw"]):
            assert same(a[b], o[0]), b


def test_a_captured_graph_gives_the_bits_of_the_eager_call(pt):
    se, te, x, g = PR.make_case(64, 70, 2 * pt.SLICE + 37, 2, 4.0, "random", 25)
    eager = run(pt, se, te, x, g)
    tse, tte, tx = (t.requires_grad_(True) for t in cuda(se, te, x))
    (tg,) = cuda(g)

    def step():
        corr = pt.soft_pointer(tse, tte, tx)
        return (corr.detach(),) + torch.autograd.grad((corr * tg).sum(), (tse, tte, tx))
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
        for o, want in zip(outs, (eager["raw"][i] for i in (0, 3, 4, 5))):
            assert same(o, want)


# ---- DCP's head ----------------------------------------------------------------------------------------------------------------
def test_dcp_svd_head_is_the_two_nodes_and_matches_the_reference_recording(pt):
    """callsites.dcp_svd_head is bit-identical to dcp_svd_head_pose(src, dcp_soft_pointer(...)); on the recorded cases R and t
    lie within section 16's bound (2^-23, and 2^-23 max(1, |abar| + |bbar|) for t) plus the move of the Kabsch twin
    (kabsch_refs) when the recorded src_corr is shifted by +- the corr bound: the twin's bound against the recording
    (test_pointer_refs_host.recorded_corr_bound) plus the device's bound against the twin."""
    from rrl_hip import callsites
    golden = load_golden("pointer_dcp.npz")
    for name in GOLDEN_CASES:
        se, te, src, x, Rw, tw_, cw = (golden[f"{name}_{k}"] for k in ("src_emb", "tgt_emb", "src", "tgt", "R", "t", "src_corr"))
        tse, tte, tsrc, tx = cuda(se, te, src, x)
        R, t = callsites.dcp_svd_head(tse, tte, tsrc, tx)
        corr = callsites.dcp_soft_pointer(tse, tte, tx)
        R2, t2 = callsites.dcp_svd_head_pose(tsrc, corr)
        assert same(R, R2) and same(t, t2), name
        R, t, corr = (v.cpu().numpy() for v in (R, t, corr))
        for b in range(se.shape[0]):
            tw = PR.head(PR.scores(se[b], te[b]), x[b])
            bound = recorded_corr_bound(se[b], te[b], x[b], tw) + tw["corr_bound"]
            assert (np.abs(corr[b] - cw[b]) <= bound).all(), (name, b)
            fits = [KR.fit(src[b].T, (cw[b].astype(np.float64) + s * bound).T, transpose_r=True) for s in (0.0, 1.0, -1.0)]
            assert fits[0]["gap"] >= 1e-2 * fits[0]["S"][0]
            dR = max(np.abs(f["R"] - fits[0]["R"]).max() for f in fits[1:])
            dT = max(np.abs(f["T"] - fits[0]["T"]).max() for f in fits[1:])
            lim_t = U23 * max(1.0, np.abs(fits[0]["abar"]).max() + np.abs(fits[0]["bbar"]).max())
            assert np.abs(R[b] - Rw[b]).max() <= U23 + dR, (name, b, np.abs(R[b] - Rw[b]).max(), dR)
            assert np.abs(t[b] - tw_[b]).max() <= lim_t + dT, (name, b, np.abs(t[b] - tw_[b]).max(), dT)
