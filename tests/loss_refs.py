"""The float64 twin of the stages behind the scan (tests/test_gpu_loss_stages.py, tests/test_loss_refs_host.py).

The scan stays the definition of what is selected: the twin takes, per cloud, the oracle's `count`, ascending `hit_idx` and
float32 `hit_w` (oracle.scan(..., cap=8)) and evaluates everything behind them -- intersection points q, the k x j blocks D,
the lower median, the Welsch terms, the row / column minima, the bucket means, the loss and its gradient -- in float64 (the
reference) or, with dtype=float32, the same formulas in float32 (the yardstick: what a plain float32 implementation of this
arithmetic loses against float64 on these inputs).  Written from oracle/torch_eager.py's sparse stage and SURVEY.md
Appendix A; nothing here is taken from the code under test.

    q[a]      = ((w0 P0 + w1 P1) + w2 P2) / 3          P = the hit triangle's three points, w its float32 weights
    D[a][b]   = (dx dx + dy dy) + dz dz                 d = q1[a] - q2[b]
    med       = the value of rank (n - 1) // 2 among all n valid D (pooled call: among the LAST sample's)
    Wl[a][b]  = 1 - exp(-(D / med) / 2)
    loss      = 1 / C  sum over the C populated (k, j) buckets of  exp(-|k - j| / 2) (rows / (S k) + cols / (S j))
                rows = sum over the bucket's S lines and a of min_b Wl, cols = sum over lines and b of min_a Wl
    dL/dD     = gl exp(-|k - j| / 2) / C  exp(-D / (2 med)) / (2 med)  ([b = argmin_b(a)] / (S k) + [a = argmin_a(b)] / (S j))
    dL/dP1[f_a][kk] += w_kk / 3 * 2 (q1[a] - q2[b]) dL/dD      (dL/dP2 with the opposite sign); med, weights, labels: constants

THE BOUNDS of Q and D (u = 2^-24, derived from the number of roundings, not measured).  A float32 evaluation of q rounds
every term w_i P_i at most five times -- the product, two additions, and the division by 3 either once or, as a product
with the rounded constant 1/3, twice -- and a fused multiply-add only removes roundings, so per component
    |q32 - q| <= Eq = 5 u (|w0 P0| + |w1 P1| + |w2 P2|) / 3        (<= 5 u max|P| / 3, the weights being positive with sum 1).
The difference d = q1 - q2 of the rounded points is rounded once: |d32 - d| <= e = Eq1 + Eq2 + u |d|.  Its square is off
by at most 2 |d| e + e^2, and each of the three squares passes through at most three more roundings (the product and two
additions; all terms are non-negative):
    |D32 - D| <= ED = (1 + 3 u) sum_c (2 |d_c| e_c + e_c^2) + 3 u D,
which is 2^-24 (|q1 - q2| max|P| + D) up to the constants, plus the squared term e^2 that takes over where q1 and q2 coincide.
An order statistic moves by no more than its elements do: the library's median lies between the rank-(n - 1) // 2 values of
D - ED and of D + ED.
"""
import numpy as np

from pose_refs import U32, rigid_reference

NEAR_TIE = 2.0 ** -18   # two Welsch terms closer than this (relative) may legitimately swap their order in float32
TINY = 2.0 ** -126      # a gradient row whose sum of |contributions| is below this may be flushed to zero


def _as_list(x, pool):
    return list(x) if pool else [x]


def select(scan1, scan2, rng):
    """{(k, j): ascending line indices} of the lines with k hits in cloud 1 and j in cloud 2, inside the range."""
    s_m, s_n, e_m, e_n = (int(v) for v in rng)
    c1, c2 = np.asarray(scan1["count"]), np.asarray(scan2["count"])
    out = {}
    for k in range(s_m, e_m):
        for j in range(s_n, e_n):
            out[(k, j)] = np.nonzero((c1 == k) & (c2 == j))[0]
    return out


def _points(tri, scan, sel, k, dtype, alt=False):
    """q (S, k, 3), its bound Eq (S, k, 3) (float64), the hit triangles f (S, k) and their weights w (S, k, 3) as `dtype`.
    alt: the same point as (w0 P0 + (w1 P1 + w2 P2)) * (1 / 3) -- another association and a reciprocal instead of the
    division, both inside the five roundings of Eq: a second, equally correct evaluation in `dtype`."""
    f = np.asarray(scan["hit_idx"])[sel, :k].astype(np.int64)
    w = np.asarray(scan["hit_w"], np.float32)[sel, :k].astype(dtype)
    P = np.asarray(tri, np.float32).reshape(-1, 3, 3)[f].astype(dtype)          # (S, k, point, xyz)
    t = w[..., None] * P
    q = (t[:, :, 0] + (t[:, :, 1] + t[:, :, 2])) * (dtype(1) / dtype(3)) if alt else ((t[:, :, 0] + t[:, :, 1]) + t[:, :, 2]) / dtype(3)
    Eq = 5.0 * U32 * np.abs(t.astype(np.float64)).sum(2) / 3.0
    return q, Eq, f, w


def _same_points(tri, fa, fb):
    a, b = np.asarray(tri, np.float32)[fa].reshape(3, 3), np.asarray(tri, np.float32)[fb].reshape(3, 3)
    return sorted(map(tuple, a.tolist())) == sorted(map(tuple, b.tolist()))


def _near_ties(Wl, tri_other, f_other, axis):
    """(S,) bool: a row (axis = 2: over cloud 2's hits) or column (axis = 1) of Wl (S, k, j) whose two smallest terms
    differ by less than NEAR_TIE relative and belong to pseudo-triangles with different point sets."""
    S = Wl.shape[0]
    flag = np.zeros(S, bool)
    if Wl.shape[axis] < 2:
        return flag
    W64 = np.asarray(Wl, np.float64)
    order = np.argsort(W64, axis=axis, kind="stable")
    lo = np.take(order, 0, axis=axis)          # (S, other extent)
    hi = np.take(order, 1, axis=axis)
    srt = np.sort(W64, axis=axis)
    a0, a1 = np.take(srt, 0, axis=axis), np.take(srt, 1, axis=axis)
    close = (a1 - a0) < NEAR_TIE * np.maximum(np.abs(a1), TINY)
    for s, r in zip(*np.nonzero(close)):
        if not _same_points(tri_other, f_other[s, lo[s, r]], f_other[s, hi[s, r]]):
            flag[s] = True
    return flag


def post_scan_ref(tri1, tri2, scan1, scan2, rng, grad_out=1.0, dtype=np.float64, pool=False, alt=False):
    """The stages behind the scan for one sample -- or, with pool=True, for a list of samples pooled the way the reference
    treats B > 1 (tests/golden/loss_b2_quirk.npz, SURVEY.md Q2: the lines of all samples in one set of (k, j) buckets,
    the LAST sample's median, one loss).  tri1 (N, 9), tri2 (M, 9) float32; scan1 / scan2: oracle.scan(..., cap=8) of
    them.  Returns None when no bucket is populated, else a dict:
      blocks    per sample {(k, j): dict(lines (S,), f1 (S, k), f2 (S, j), q1 (S, k, 3), q2 (S, j, 3), D (S, k, j),
                Eq1, Eq2, ED: the bounds of the module docstring (float64), tie (S,) bool: the near-tie flag)}
      values    all valid D of the group whose median counts (1-D, bucket-major, then line), EDvalues their bounds
      med, n_values, n_selected, n_buckets (C), bcnt {(k, j): S}, rows / cols {(k, j): sum of the row / column minima}
      loss
      g1, g2    per sample dL/dtri1 (N, 9), dL/dtri2 (M, 9) for the upstream gradient grad_out, float64 accumulation of
                contributions evaluated in `dtype`
      a1, a2    per sample the sum of |contributions| to every gradient element;  k1, k2: their number
      tie_lines per sample the selected lines that hold a near tie;  n_tie, tie_share
    With pool=False the per-sample entries are the sample's own (no list).  alt (with dtype=float32): a second correct
    float32 evaluation, see _points."""
    dtype = np.dtype(dtype).type
    t1s, t2s, s1s, s2s = (_as_list(x, pool) for x in (tri1, tri2, scan1, scan2))
    ns = len(t1s)
    blocks = []
    for b in range(ns):
        blk = {}
        for (k, j), sel in select(s1s[b], s2s[b], rng).items():
            if len(sel) == 0:
                continue
            q1, Eq1, f1, w1 = _points(t1s[b], s1s[b], sel, k, dtype, alt)
            q2, Eq2, f2, w2 = _points(t2s[b], s2s[b], sel, j, dtype, alt)
            d = q1[:, :, None, :] - q2[:, None, :, :]
            D = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            d64 = np.abs(d.astype(np.float64))
            e = Eq1[:, :, None, :] + Eq2[:, None, :, :] + U32 * d64
            ED = (1 + 3 * U32) * (2 * d64 * e + e * e).sum(-1) + 3 * U32 * D.astype(np.float64)
            blk[(k, j)] = dict(lines=sel, f1=f1, f2=f2, w1=w1, w2=w2, q1=q1, q2=q2, D=D, d=d, Eq1=Eq1, Eq2=Eq2, ED=ED)
        blocks.append(blk)
    keys = sorted({kj for blk in blocks for kj in blk})
    if not keys:
        return None
    last = blocks[-1]
    if not last:
        raise ValueError("pooled call whose last sample selects nothing: the reference divides by an empty median")
    values = np.concatenate([last[kj]["D"].reshape(-1) for kj in sorted(last)])
    EDvalues = np.concatenate([last[kj]["ED"].reshape(-1) for kj in sorted(last)])
    med = np.sort(values)[(len(values) - 1) // 2]
    C = len(keys)
    two, one = dtype(2), dtype(1)
    gl = dtype(grad_out)
    out = dict(blocks=blocks, values=values, EDvalues=EDvalues, med=med, n_values=len(values), n_buckets=C,
               n_selected=sum(len(v["lines"]) for v in last.values()), bcnt={}, rows={}, cols={})
    N, M = [np.asarray(t).reshape(-1, 9).shape[0] for t in t1s], [np.asarray(t).reshape(-1, 9).shape[0] for t in t2s]
    acc = {n: [np.zeros(sz[b] * 9) for b in range(ns)] for n, sz in (("g1", N), ("g2", M), ("a1", N), ("a2", M))}
    cnt = {n: [np.zeros(sz[b] * 9, np.int64) for b in range(ns)] for n, sz in (("k1", N), ("k2", M))}
    tie_lines = [[] for _ in range(ns)]
    loss = dtype(0)
    for (k, j) in keys:
        S = sum(len(blk[(k, j)]["lines"]) for blk in blocks if (k, j) in blk)
        wkj = dtype(np.exp(dtype(-0.5) * dtype(abs(k - j))))
        rows = cols = dtype(0)
        for b, blk in enumerate(blocks):
            v = blk.get((k, j))
            if v is None:
                continue
            ex = np.exp(-(v["D"] / med) / two)
            Wl = one - ex
            amin_b, amin_a = Wl.argmin(2), Wl.argmin(1)          # first occurrence, like torch.min on the CPU
            rows = rows + Wl.min(2).sum(dtype=dtype)
            cols = cols + Wl.min(1).sum(dtype=dtype)
            v["Wl"] = Wl
            v["tie"] = _near_ties(Wl, t2s[b], v["f2"], 2) | _near_ties(Wl, t1s[b], v["f1"], 1)
            tie_lines[b].append(v["lines"][v["tie"]])
            # ---- the backward, contribution by contribution
            is_row = np.arange(j)[None, None, :] == amin_b[:, :, None]
            is_col = np.arange(k)[None, :, None] == amin_a[:, None, :]
            sw = is_row * (one / (dtype(S) * dtype(k))) + is_col * (one / (dtype(S) * dtype(j)))
            gD = (gl * wkj / dtype(C)) * sw * ex / (two * med)                    # (S, k, j)
            gq = two * v["d"] * gD[..., None]                                      # (S, k, j, 3) = dL/dq1[a] via (a, b)
            live = (sw != 0)
            for side, (w, f, names) in enumerate(((v["w1"], v["f1"], ("g1", "a1", "k1")), (v["w2"], v["f2"], ("g2", "a2", "k2")))):
                wk = w / dtype(3)                                                   # (S, h, 3)
                if side == 0:
                    c = wk[:, :, None, :, None] * gq[:, :, :, None, :]             # (S, k, j, kk, xyz)
                    fi = np.broadcast_to(f[:, :, None, None, None], c.shape)
                else:
                    c = -(wk[:, None, :, :, None] * gq[:, :, :, None, :])
                    fi = np.broadcast_to(f[:, None, :, None, None], c.shape)
                slot = np.broadcast_to((3 * np.arange(3)[:, None] + np.arange(3)[None, :])[None, None, None], c.shape)
                lv = np.broadcast_to(live[..., None, None], c.shape)
                idx = (fi * 9 + slot)[lv]
                cc = c[lv].astype(np.float64)
                np.add.at(acc[names[0]][b], idx, cc)
                np.add.at(acc[names[1]][b], idx, np.abs(cc))
                np.add.at(cnt[names[2]][b], idx, 1)
        out["bcnt"][(k, j)], out["rows"][(k, j)], out["cols"][(k, j)] = S, rows, cols
        loss = loss + wkj * (rows / (dtype(S) * dtype(k)) + cols / (dtype(S) * dtype(j)))
    out["loss"] = loss / dtype(C)
    tie_lines = [np.sort(np.concatenate(t)) if t else np.zeros(0, np.int64) for t in tie_lines]
    nsel_all = sum(len(v["lines"]) for blk in blocks for v in blk.values())
    out.update(n_selected_all=nsel_all, n_tie=sum(len(t) for t in tie_lines))
    out["tie_share"] = out["n_tie"] / max(nsel_all, 1)
    per = {n: [a.reshape(-1, 9) for a in v] for n, v in list(acc.items()) + list(cnt.items())}
    per["tie_lines"] = tie_lines
    for n, v in per.items():
        out[n] = v if pool else v[0]
    if not pool:
        out["blocks"] = blocks[0]
    return out


def post_scan_torch(tri1, tri2, ref, rng, grad_out=1.0):
    """torch float64 autograd of the twin's forward with the median and the labels frozen at `ref`'s (one sample, a
    post_scan_ref result): (loss, dL/dtri1, dL/dtri2) as float / float64 arrays.  tri1 / tri2 may be float64 (the finite
    difference perturbs them)."""
    import torch
    t1 = torch.tensor(np.asarray(tri1, np.float64).reshape(-1, 3, 3), requires_grad=True)
    t2 = torch.tensor(np.asarray(tri2, np.float64).reshape(-1, 3, 3), requires_grad=True)
    med, C, total = float(ref["med"]), ref["n_buckets"], 0.0
    for (k, j), v in sorted(ref["blocks"].items()):
        q1 = (torch.from_numpy(v["w1"].astype(np.float64))[..., None] * t1[torch.from_numpy(v["f1"])]).sum(2) / 3
        q2 = (torch.from_numpy(v["w2"].astype(np.float64))[..., None] * t2[torch.from_numpy(v["f2"])]).sum(2) / 3
        D = ((q1[:, :, None, :] - q2[:, None, :, :]) ** 2).sum(-1)
        Wl = 1 - torch.exp(-(D / med) / 2.0)
        total = total + float(np.exp(-0.5 * abs(k - j))) * (Wl.min(2)[0].mean() + Wl.min(1)[0].mean())
    total = total / C
    (total * grad_out).backward()
    return float(total.detach()), t1.grad.numpy().reshape(-1, 9), t2.grad.numpy().reshape(-1, 9)


def rigid_grads_ref(src, R, t, g_points, transpose_r):
    """float64 dL/dR (3, 3, in R's layout) and dL/dt (3,) of y = src m + t (m = R^T with transpose_r, else R) from the
    gradient g_points with respect to the moved points; src and g_points (N, 9) or (n, 3)."""
    c = dict(x=np.asarray(src, np.float64).reshape(1, -1, 3), R=np.asarray(R, np.float64).reshape(1, 3, 3),
             t=np.asarray(t, np.float64).reshape(1, 3), gy=np.asarray(g_points, np.float64).reshape(1, -1, 3))
    r = rigid_reference(c, transpose_r, np.float64)
    return r["gR"][0], r["gt"][0]


def rigid_abs_sums(src, a_points, transpose_r):
    """The sums of |contributions| behind rigid_grads_ref's 12 outputs -- |src_i| a_j for dR, a_j for dt, with a_points the
    per-element sums of |contributions| of the point gradient: (aR (3, 3), at (3,))."""
    return rigid_grads_ref(np.abs(np.asarray(src, np.float64)), np.eye(3), np.zeros(3), a_points, transpose_r)


# ------------------------------------------------------------------------------------------------------------- the bounds
FACTOR, FLOOR_UNITS = 4.0, 8.0   # the margin of a device evaluation over a host float32 one (tests/pose_refs.py: SE3_*)


def scalar_bound(x64, x32, extra=0.0):
    """Loss, payload, bucket sums: 4 |x32 - x64| + 8 u |x64| (+ extra: a fixed-point unit where one applies)."""
    return FACTOR * abs(float(x32) - float(x64)) + FLOOR_UNITS * U32 * abs(float(x64)) + extra


FIX_UNIT = 2.0 ** -40  # BSUM's fixed point


def bucket_sum_bounds(r64, r32, kj, key):
    """(x64, the bound used, the bound in the plain form) for the row ('rows') or column ('cols') sum of bucket kj of one
    sample or a pooled group.  Plain form: scalar_bound on the two sums, 4 |x32 - x64| + 8 u |x64|, plus one fixed-point
    unit per term.  Used: the same with the float32 twin's error taken TERM BY TERM, 4 sum |W32 - W64| over the minima.
    1 - exp(-y) loses up to 1e-6 relative where D is small against the median, the errors of one float32 evaluation
    partly cancel in the sum, and those of another correct evaluation need not cancel alike:
    tests/test_loss_refs_host.py shows a second float32 evaluation of the same twin (`alt`) at 1.6 x the plain form and
    inside the term-by-term one."""
    k, j = kj
    ax, n = (2, k) if key == "rows" else (1, j)
    b64s, b32s = (r["blocks"] if isinstance(r["blocks"], list) else [r["blocks"]] for r in (r64, r32))
    terms = sum(float(np.abs(b32[kj]["Wl"].min(ax).astype(np.float64) - b64[kj]["Wl"].min(ax)).sum())
                for b64, b32 in zip(b64s, b32s) if kj in b64)
    x64, units = float(r64[key][kj]), r64["bcnt"][kj] * n * FIX_UNIT
    return x64, FACTOR * terms + FLOOR_UNITS * U32 * abs(x64) + units, scalar_bound(x64, r32[key][kj], units)


def normalised(err, a):
    """|err| / a where a > 0, else 0 (an element nothing contributes to must be exactly zero: checked apart)."""
    err, a = np.abs(np.asarray(err, np.float64)), np.asarray(a, np.float64)
    return np.divide(err, a, out=np.zeros_like(err), where=a > 0)


def grad_bound(g64, g32, a, k, keep=None):
    """The allowed normalised error of every gradient element: 4 x the float32 twin's largest normalised error over the
    set (its kept elements) plus (k + 3) u for the k-term sum (the Chamfer backward's form).
    Returns (bound like k, the float32 twin's largest normalised error)."""
    n32 = normalised(np.asarray(g32, np.float64) - g64, a)
    if keep is not None:
        n32 = n32[keep]
    worst32 = float(n32.max()) if n32.size else 0.0
    return FACTOR * worst32 + (np.asarray(k, np.float64) + 3.0) * U32, worst32


def det_extra(k, gl, C, med):
    """Deterministic mode's absolute allowance per element: k 2^-37 1.62 |gl| / (C sqrt(med)) -- every contribution is
    rounded to a fixed-point unit no coarser than 2^-38 of the largest possible contribution."""
    return np.asarray(k, np.float64) * 2.0 ** -37 * 1.62 * abs(float(gl)) / (C * np.sqrt(float(med)))


def tie_points(tri1, tri2, ref_blocks):
    """The 3-D points (as rows of float32 triples) of every pseudo-triangle hit by a near-tie line, per cloud."""
    p1, p2 = [np.zeros((0, 3), np.float32)], [np.zeros((0, 3), np.float32)]
    for v in ref_blocks.values():
        t = v["tie"]
        if t.any():
            p1.append(np.asarray(tri1, np.float32)[v["f1"][t].reshape(-1)].reshape(-1, 3))
            p2.append(np.asarray(tri2, np.float32)[v["f2"][t].reshape(-1)].reshape(-1, 3))
    return np.concatenate(p1), np.concatenate(p2)


def point_mask(tri, excluded):
    """(unique points of tri, in merge_by_point's order,) -> bool mask: True where the point is NOT one of `excluded`."""
    keys = np.unique(np.asarray(tri, np.float32).reshape(-1, 3), axis=0)
    if len(excluded) == 0:
        return np.ones(len(keys), bool)
    ex = {tuple(r) for r in np.asarray(excluded, np.float32).tolist()}
    return np.array([tuple(r) not in ex for r in keys.tolist()], bool)


def check_grad(name, tri, got, ref64, ref32, key, merge, excluded=(), extra_abs=None, scale=1.0):
    """Hold a (N, 9) gradient to the twin per point.  ref64 / ref32: post_scan_ref results (float64 / float32) for ONE
    sample at upstream gradient 1; `scale` the call's upstream gradient (the twin's figures scale with it exactly when
    it is a power of two, and to one rounding otherwise); key '1' or '2'.  Returns (worst ratio, text)."""
    g64, g32 = merge(tri, ref64["g" + key]) * scale, merge(tri, ref32["g" + key]) * scale
    a, k = merge(tri, ref64["a" + key]) * abs(scale), merge(tri, ref64["k" + key])
    mine = merge(tri, got)
    keep = point_mask(tri, excluded)[:, None] & np.ones(3, bool)[None]
    if scale == 0.0:
        assert not np.any(mine), f"{name}: a zero upstream gradient must give an exactly zero gradient"
        return 0.0, f"{name}: exactly zero"
    bound, worst32 = grad_bound(g64, g32, a, k, keep)
    allowed = bound * a + (0.0 if extra_abs is None else extra_abs(k))
    err = np.abs(mine - g64)
    assert np.isfinite(mine).all(), f"{name}: non-finite gradient"
    # rows without any contribution are exactly zero; rows with one are non-zero unless it is below the subnormal range
    assert not np.any(mine[a == 0]), f"{name}: gradient where the twin has no contribution"
    # (deterministic mode rounds every contribution to its fixed-point unit: a row below that allowance may vanish too)
    floor = TINY if extra_abs is None else np.maximum(TINY, extra_abs(k).sum(1))
    rows_mine, rows_ref = np.abs(mine).sum(1) > 0, a.sum(1) >= floor
    big = rows_ref & keep[:, 0]
    assert np.array_equal(rows_mine[big], rows_ref[big]), f"{name}: the non-zero rows differ from the twin's"
    ratio = np.divide(err, allowed, out=np.zeros_like(err), where=allowed > 0)[keep]
    worst = float(ratio.max()) if ratio.size else 0.0
    dev = float(normalised(err, a)[keep].max()) if ratio.size else 0.0
    text = (f"{name}: normalised error device {dev:.3e}, float32 host {worst32:.3e}, worst error / bound {worst:.3f}, "
            f"points left out {int((~keep[:, 0]).sum())} of {len(keep)}")
    return worst, text
