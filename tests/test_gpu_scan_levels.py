"""The culled scan's levels B and D at their edges (csrc/rrl_cull_scan.h proc_a, proc_c, push_halves, tail_split).

A drain's last pass of level B or D holds fewer than 64 entries; kSplitTail spreads such a pass over 2, 4 or 8 lanes per entry
(8 >> k tests each).  The bar is the strict scan (mode="strict", the reference's arithmetic on every pair): hit COUNTS equal,
hit rows equal as sorted sets (where a line keeps all of its hits: RRL_MAX_HITS), loss / median / info / bucket sums equal
bit for bit -- at shapes with one supergroup and one wavefront, partial supergroups / halves / wavefronts, a tile that holds
one line, on dense clouds whose survivors overflow every queue of the walk, and through the plain, the chained and the fat
(Scan16) launch at the smallest shape each admits.  The in-kernel counters (ops.make_opts(counters=...), one row per
wavefront) say which passes ran: every non-final pass of a level takes exactly 64 entries, so a wavefront's last pass of level
B holds (row[1] / 8) % 64 entries and its last pass of level D row[2] % 64.
"""
import numpy as np
import pytest
import torch

from test_gpu_chain import _assert_same, _new_lines, _poses, _snapshot
from test_gpu_parity import cu
from test_gpu_prepared import _lines, _pairs, _same_evaluation, _with_fat

pytestmark = pytest.mark.gpu

WC_CAP = 128   # parked candidates per wavefront (csrc/rrl_cull_scan.h, both variants)
DENSE = 0.15   # _dense: the clouds' extent against synth.make_pair's


@pytest.fixture(scope="module")
def L():
    import loss
    from rrl_hip import _lib
    _lib.load()
    assert torch.cuda.is_available()
    return loss


def _table():
    return torch.zeros(1 << 14, 16, dtype=torch.int64, device="cuda")


def _split_classes(tab):
    """Which split factors k the wavefronts' last passes ran with, per level: {0, 1, 2, 3} when all four occurred."""
    rows = tab[(tab[:, 5] > 0) & (tab[:, 6] == 0)]
    out = []
    for rem in ((rows[:, 1] // 8) % 64, rows[:, 2] % 64):
        rem = rem[rem > 0].cpu().numpy()
        out.append({int(k) for k in np.select([rem <= 8, rem <= 16, rem <= 32], [3, 2, 1], 0)})
    return out


@pytest.mark.parametrize("B,n,m,nl", [(2, 64, 64, 128),      # one supergroup, one wavefront of lines
                                      (1, 70, 130, 129),     # partial supergroup, partial half, partial wavefront
                                      (3, 512, 512, 1025)])  # two tiles, the second holds ONE line; n % 8 != 0 is the case above
@pytest.mark.parametrize("prepared", [False, True])
def test_levels_equal_the_strict_scan(L, B, n, m, nl, prepared):
    from rrl_hip import ops
    prs, t1, t2 = _pairs(1300, B, n, m)
    ln = _lines(L, prs, nl)
    strict = ops.loss_forward_raw(t1, t2, ln, mode="strict")
    tab = _table()
    o = dict(order1=ops.cloud_order(t1), order2=ops.cloud_order(t2)) if prepared else {}
    cull = ops.loss_forward_raw(t1, t2, ln, mode="cull", opts=ops.make_opts(**o) if o else None)
    counted = ops.loss_forward_raw(t1, t2, ln, mode="cull", opts=ops.make_opts(counters=tab, **o))
    torch.cuda.synchronize()
    _same_evaluation(strict, cull)
    _same_evaluation(strict, counted)
    assert int(cull.status[1]) == 0 and int(tab[:, 6].sum()) == 0  # no wavefront left the culled path
    kb, kd = _split_classes(tab)
    if nl == 1025:  # 54 wavefronts with lines, every fill level: all four split factors at both levels, a lone line among them
        assert kb == {0, 1, 2, 3} and kd == {0, 1, 2, 3}, (kb, kd)
        assert int(tab[tab[:, 5] > 0, 0].min()) <= 8  # the tile of one line: 1 line x the slice's supergroups
    else:  # (one supergroup: every line may pass level A, and 128 pairs leave no partial pass)
        assert int(tab[:, 1].sum()) > 0 and int(tab[:, 3].sum()) > 0 and int(tab[:, 4].sum()) > 0, "the walk reached levels B and D"
    print(f"[levels] {B},{n},{m},{nl} prepared={prepared}: last-pass split factors B {sorted(kb)} D {sorted(kd)}")


def _dense(seed, B, n):
    """synth.make_pair with every triangle moved towards the cloud's centre (its size kept): tiny, overlapping clouds -- a
    line through them passes within the threshold of many triangles."""
    from rrl_hip import synth
    prs = [synth.make_pair(seed + b, n, n) for b in range(B)]
    for p in prs:
        for key in ("src", "tar"):
            tri = p[key + "_tri"].reshape(-1, 3, 3)
            c = tri.mean(1, keepdims=True)
            p[key + "_tri"] = (tri - (1.0 - DENSE) * c).reshape(-1, 9).astype(np.float32)
            p[key] = (p[key] * DENSE).astype(np.float32)
        p["radius"] = np.float32(DENSE * float(p["radius"]))
        p["center"] = (DENSE * p["center"]).astype(np.float32)
    return prs, cu(np.stack([p["src_tri"] for p in prs])), cu(np.stack([p["tar_tri"] for p in prs]))


@pytest.mark.parametrize("fat,B,n,nl", [("1", 1, 1024, 1000),     # 16 supergroups > 8: RRL_CULL_FAT=1 is honoured, one fat slice per cloud
                                        ("0", 16, 512, 24576)])   # the lean variant keeps its 8-supergroup slices from 768 workgroups on:
def test_dense_clouds_overflow_every_queue(L, fat, B, n, nl):     # 2 clouds x 16 samples x 24 line tiles x 1 slice (cull_geometry)
    """Most lines hit five triangles or more: level A leaves more pairs than queue A holds (the supergroup-by-supergroup path
    with level B in between), level B more halves than queue C holds (level D runs in between, and a pass that does not fit goes
    half by half), and the parked candidates exceed their buffer (flushes inside level D, the lean variant's inline resolution)."""
    from rrl_hip import ops
    prs, t1, t2 = _dense(1400, B, n)
    ln = _lines(L, prs, nl)
    strict = ops.loss_forward_raw(t1, t2, ln, mode="strict")
    torch.cuda.synchronize()
    dense1, dense2 = float((strict.count1 >= 5).float().mean()), float((strict.count2 >= 5).float().mean())
    print(f"[dense] lines with >= 5 hits: {dense1:.2f} / {dense2:.2f}, mean count {float(strict.count1.float().mean()):.1f}")
    assert dense1 > 0.5 and dense2 > 0.5
    o1, o2 = ops.cloud_order(t1), ops.cloud_order(t2)
    tab = torch.zeros(1 << 15, 16, dtype=torch.int64, device="cuda")
    cull = _with_fat(fat, lambda: ops.loss_forward_raw(t1, t2, ln, mode="cull", opts=ops.make_opts(order1=o1, order2=o2)))
    _with_fat(fat, lambda: ops.loss_forward_raw(t1, t2, ln, mode="cull", opts=ops.make_opts(order1=o1, order2=o2, counters=tab)))
    _same_evaluation(strict, cull)
    assert int(cull.status[1]) == 0 and int(tab[:, 6].sum()) == 0
    waves = int(tab[:, 5].sum())
    pairs, halves, cands = tab[:, 1] // 8, tab[:, 2], tab[:, 4]
    print(f"[dense] fat={fat}: {waves} wavefronts, max per wavefront: pairs {int(pairs.max())}, halves {int(halves.max())}, candidates {int(cands.max())}")
    assert waves == 2 * B * ((n + 63) // 64 // (16 if fat == "1" else 8)) * ((nl + 127) // 128)  # slices of 16 / 8 supergroups ran
    # beyond the capacities: queue A 384 / 256 pairs, queue C 256 halves, 128 parked candidates (csrc/rrl_cull_scan.h)
    assert int(pairs.max()) > (384 if fat == "1" else 256) and int(halves.max()) > 256 and int(cands.max()) > WC_CAP


def test_chained_and_fat_launches_at_their_smallest_shapes(L):
    """cull_scan_build_kernel of both variants against the STRICT step at B = 2, N = 1200, M = 1000.  Fat: L = 2500 is the shape
    test_gpu_chain.py forces its fused launch at (19 supergroups > 8; 20 wavefronts of lines: full workgroups).  Lean: the
    slices thin out to one supergroup there and full 8-wavefront workgroups need 2 x 2 x tiles x 19 >= 256 workgroups
    (cull_geometry): four line tiles, L = 3100.  Second and third call: the chained launch."""
    from rrl_hip import ops
    B, n, m = 2, 1200, 1000
    prs, src, tar = _pairs(1500, B, n, m)
    for fat, nl in (("0", 3100), ("1", 2500)):
        strict = ops.LossStep(src, tar, nl, mode="strict", chain=False)
        chained = ops.LossStep(src, tar, nl)
        for it in range(3):
            ln = _new_lines(L, prs, nl, it)
            R, t = _poses(B, it)
            a = _snapshot(strict, strict(R, t, ln))
            b = _with_fat(fat, lambda: _snapshot(chained, chained(R, t, ln)))
            _assert_same(a, b, (fat, it))
            assert chained.fused is (it > 0), (fat, it)
        assert int(b["info"][:, 1].min()) > 0 and int(b["info"][:, 3].max()) == 0
