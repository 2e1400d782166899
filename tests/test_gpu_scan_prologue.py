"""The culled scan's prologue branches (csrc/rrl_cull_scan.h cull_scan_body): the scan's arguments arrive in one round of
scalar loads and its partial rows, records and nodes leave as range-checked buffer loads with no wait in between.  None of
that may change a label, so every case here compares the default (culled) mode against mode="strict" on the same inputs --
hit counts, ascending hit lists, info, loss bits -- and, for steps that may chain, the chained step against chain=False the
way test_gpu_chain does, on shapes that reach the branches the rest of the suite leaves thin:

  * more than 64 partial rows (a cloud beyond 16384 triangles): the loop of the partial-row reduction, prepared plain kernel;
  * a line tensor whose tiles are not 16-byte aligned, with a partial last tile: the 8-byte line path, a wavefront without
    lines, a last slice of 3 of 8 supergroups;
  * the same at 12 x the scale: the NaN-wide staging; once with a non-finite target coordinate: the strict fallback;
  * a shape that fuses, over four chained steps with new lines and poses.
"""
import numpy as np
import pytest
import torch

from test_gpu_chain import _assert_same, _new_lines, _poses, _snapshot
from test_gpu_parity import cu
from test_gpu_prepared import _hits_sorted, _pairs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import loss
    from rrl_hip import _lib
    _lib.load()
    assert torch.cuda.is_available()
    return loss


def _same_bits(a, b):
    """bit for bit; two NaNs agree whatever their payload (no caller reads it)"""
    ai, bi = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return bool(((ai == bi) | (torch.isnan(a) & torch.isnan(b))).all())


def _same_scan(a, b, what):
    """hit counts and ascending hit lists of both clouds, NaN flag, info, loss of two states / outputs"""
    (sa, oa), (sb, ob) = a, b
    for w in (1, 2):
        ca, ha = _hits_sorted(sa, w)
        cb, hb = _hits_sorted(sb, w)
        assert torch.equal(ca, cb), (what, "count", w)
        assert torch.equal(ha, hb), (what, "hits", w)
    assert torch.equal(oa[2], ob[2]), (what, "info")
    assert _same_bits(oa[0], ob[0]), (what, "loss")


def _misaligned(ln):
    """the same lines as a contiguous view that starts one 24-byte row into a larger buffer: 8-byte, not 16-byte aligned"""
    buf = torch.zeros(ln.numel() + 6, dtype=torch.float32, device=ln.device)
    v = buf[6:].view(ln.shape)
    v.copy_(ln)
    assert v.is_contiguous() and v.data_ptr() % 16 == 8
    return v


def _run_steps(L, prs, src, tar, nl, steps, lines_of=lambda ln: ln, expect_fused=None):
    from rrl_hip import ops
    B = src.shape[0]
    strict = ops.LossStep(src, tar, nl, mode="strict")
    plain = ops.LossStep(src, tar, nl)
    plain.chain = False
    chained = ops.LossStep(src, tar, nl)
    assert plain.prepared and not strict.prepared
    for it in range(steps):
        ln = lines_of(_new_lines(L, prs, nl, it))
        R, t = _poses(B, it)
        s = strict(R, t, ln)
        p = plain(R, t, ln)
        torch.cuda.synchronize()
        _same_scan((plain.st, p), (strict.st, s), (it, "culled against strict"))
        assert int(plain.st.count1.max()) > 0 and int(plain.st.count2.max()) > 0  # not degenerate: lines do hit
        a = _snapshot(plain, p)
        b = _snapshot(chained, chained(R, t, ln))
        torch.cuda.synchronize()
        _assert_same(a, b, (it, "chained against unchained"))
        if expect_fused is not None:
            assert chained.fused == (expect_fused and it > 0), it
    assert int(p[2][:, 1].min()) > 0 and int(p[2][:, 3].max()) == 0  # every sample has a populated bucket, no NaN


def test_more_than_64_partial_rows(L):
    """16640 triangles = 65 partial rows of 256: the loop path of max |P|^2 beside the one-load path of the small cloud"""
    prs, src, tar = _pairs(2100, 1, 16640, 300)
    _run_steps(L, prs, src, tar, 1100, 2)


def test_unaligned_lines_partial_tile(L):
    prs, src, tar = _pairs(2200, 2, 700, 900)
    _run_steps(L, prs, src, tar, 1500, 3, lines_of=_misaligned)


def _scaled(seed, B, n, m, scale):
    prs, src, tar = _pairs(seed, B, n, m)
    for p in prs:
        p.update(radius=float(p["radius"]) * scale, center=p["center"] * scale, src=p["src"] * scale, tar=p["tar"] * scale)
    return prs, src * scale, tar * scale


def test_unaligned_lines_nan_wide(L):
    prs, src, tar = _scaled(2200, 2, 700, 900, 12.0)
    _run_steps(L, prs, src, tar, 1500, 3, lines_of=_misaligned)


def test_non_finite_target_takes_the_strict_fallback(L):
    """One non-finite coordinate in the target: max |P|^2 of that cloud is not finite, every wavefront of its scan evaluates
    all pairs strictly (the reference's semantics, NaN included) -- through the prepared build (orders taken from the finite
    cloud: any permutation serves) and the cold one; the strict mode agrees on counts, hit lists and the NaN flag."""
    from rrl_hip import ops
    prs, src, tar = _scaled(2200, 2, 700, 900, 12.0)
    ln = _misaligned(_new_lines(L, prs, 1500, 0))
    o1, o2 = ops.cloud_order(src), ops.cloud_order(tar)
    tar = tar.clone()
    tar[1, 5, 4] = float("inf")
    s = ops.loss_forward_raw(src, tar, ln, mode="strict")
    torch.cuda.synchronize()
    assert int(s.status[0]) == 1
    for opts in (None, ops.make_opts(order1=o1, order2=o2)):
        c = ops.loss_forward_raw(src, tar, ln, mode="cull", opts=opts)
        torch.cuda.synchronize()
        assert int(c.status[1]) > 0  # wavefronts did leave the culled walk
        assert int(c.status[0]) == int(s.status[0])
        for w in (1, 2):
            cc, hc = _hits_sorted(c, w)
            cs, hs = _hits_sorted(s, w)
            assert torch.equal(cc, cs) and torch.equal(hc, hs), (opts is not None, w)
        assert torch.equal(c.info, s.info) and _same_bits(c.loss, s.loss)


def test_four_chained_steps(L):
    prs, src, tar = _pairs(2300, 3, 700, 900)
    _run_steps(L, prs, src, tar, 4000, 4, expect_fused=True)
