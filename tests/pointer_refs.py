"""Host twins of the softmax pointer (include/rrl.h rrl_pointer_fwd / rrl_pointer_bwd), numpy only.

The scores restate the header's rule bit for bit: one float32 fmaf chain per score over the channels ascending, then one
float32 multiplication by sc = float32(1 / sqrt(double(C))).  numpy has no fmaf, so fmaf32 builds one: the product of two
float32 values is exact in float64 (48 significant bits), TwoSum adds the accumulator to it with its exact residual, and the
float64 sum is rounded to float32 -- correctly, except where that sum is exactly a float32 tie while the residual is not
zero: then the residual decides the direction (double rounding is innocuous everywhere else).

Everything behind the scores is float64 from those float32 z: the softmax weights, corr and the three gradients by the
header's formulas, together with the sums of magnitudes the GPU tests' bounds are made of.  `exact` is the plain float64
function (exact scores) that torch autograd of the reference formulation is compared with.
"""
import numpy as np

F32, F64 = np.float32, np.float64
U24, U23, U22 = 2.0 ** -24, 2.0 ** -23, 2.0 ** -22


def fmaf32(a, b, c):
    """float32(a * b + c) with ONE rounding, elementwise on float32 arrays (finite values)."""
    a, b, c = (np.asarray(v, F32) for v in (a, b, c))
    p = a.astype(F64) * b.astype(F64)          # exact
    cd = c.astype(F64)
    s = p + cd                                 # TwoSum: s + e == p + cd exactly
    bb = s - p
    e = (p - (s - bb)) + (cd - bb)
    with np.errstate(over="ignore", invalid="ignore"):
        r = s.astype(F32)
        up, dn = np.nextafter(r, F32(np.inf)), np.nextafter(r, F32(-np.inf))
        rd = r.astype(F64)
        tie_up = (s == (rd + up.astype(F64)) / 2) & np.isfinite(up)    # exact in float64: neighbours of one binade pair
        tie_dn = (s == (rd + dn.astype(F64)) / 2) & np.isfinite(dn)
    # round-to-even kept r at the tie; a residual pointing past the midpoint moves the result to the other neighbour
    r = np.where(tie_up & (e > 0), up, r)
    r = np.where(tie_dn & (e < 0), dn, r)
    return r.astype(F32)


def scale(C):
    return F32(1.0 / np.sqrt(F64(C)))


def chains(src_emb, tgt_emb):
    """chain (N, M) float32 of one sample: src_emb (C, N), tgt_emb (C, M)."""
    C, N = src_emb.shape
    acc = np.zeros((N, tgt_emb.shape[1]), F32)
    for c in range(C):
        acc = fmaf32(src_emb[c][:, None], tgt_emb[c][None, :], acc)
    return acc


def scores(src_emb, tgt_emb):
    """z (N, M) float32 of one sample, the header's steps 1 and 2."""
    return (chains(src_emb, tgt_emb) * scale(src_emb.shape[0])).astype(F32)


def head(z, x, ns=None, nt=None, g=None, src_emb=None, tgt_emb=None, sc=None):
    """The float64 head of one sample from float32 scores z (N, M) and x (3, M): dict with
         w (N, M) softmax weights over the first nt columns (0 elsewhere and on rows >= ns), rowmax (N,), corr (3, N),
         eps (N, M) = 2^-22 + 2^-23 |z - rowmax| (the per-term error of two expf's and their arguments' roundings),
         corr_bound (3, N) = 2 sum_k w eps |x_k - corr| + 2^-24 |corr|,
       and with g (3, N), src_emb (C, N), tgt_emb (C, M) the gradients d_src_emb, d_tgt_emb, d_tgt with abs_* = the same sums
       with every term replaced by its magnitude (ds's own two terms, g . x and delta, included: their difference cancels).
       z may also be float64 (exact scores) and sc the exact 1 / sqrt(C): the plain float64 function's gradients."""
    N, M = z.shape
    ns, nt = N if ns is None else ns, M if nt is None else nt
    zd = z.astype(F64)
    w = np.zeros((N, M))
    rowmax = np.zeros(N)
    if ns and nt:
        rowmax[:ns] = zd[:ns, :nt].max(1)
        e = np.exp(zd[:ns, :nt] - rowmax[:ns, None])
        w[:ns, :nt] = e / e.sum(1, keepdims=True)
    xd = x.astype(F64)
    corr = xd @ w.T                                             # (3, N)
    eps = U22 + U23 * np.abs(zd - rowmax[:, None])
    eps[w == 0] = 0.0
    dev = np.abs(xd[:, None, :] - corr[:, :, None])             # (3, N, M)
    out = dict(w=w, rowmax=rowmax, corr=corr, eps=eps, corr_bound=2 * (w * eps * dev).sum(2) + U24 * np.abs(corr))
    if g is None:
        return out
    gd, se, te = g.astype(F64), src_emb.astype(F64), tgt_emb.astype(F64)
    sc = F64(scale(se.shape[0])) if sc is None else F64(sc)
    delta = (gd * corr).sum(0)                                  # (N,)
    gx = gd.T @ xd                                              # (N, M)
    ds = w * (gx - delta[:, None]) * sc
    ads = w * (np.abs(gd).T @ np.abs(xd) + (np.abs(gd) * np.abs(corr)).sum(0)[:, None]) * sc
    out.update(ds=ds, d_tgt=gd @ w, abs_d_tgt=np.abs(gd) @ w, d_src_emb=te @ ds.T, abs_d_src_emb=np.abs(te) @ ads.T,
               d_tgt_emb=se @ ds, abs_d_tgt_emb=np.abs(se) @ ads, eps_max=float(eps.max()) if eps.size else 0.0)
    return out


def grad_bound(tw, name, n, terms=0, other=1.0):
    """The GPU tests' bound of one gradient: (1.001 n 2^-24 + max eps + 2^-22) sum|terms| + 2^-24 |entry|, n the length of the
    float32 chain the rule states for it (0 for d_tgt, a double sum) -- plus float32's underflow, which no relative bound
    covers: below 2^-126 an expf, a ds or a chain's partial sum is rounded to a multiple of 2^-149 (an expf below 2^-150 is
    0 where the float64 twin still holds 1e-188), so each of the `terms` terms of the sum may be off by 2^-148 times the
    largest magnitude `other` of its other factor, and by 2^-148 once more inside the chain: (terms + 1) 2^-148 max(1, other).
    That is 1e-42 for the shapes of the tests."""
    return ((1.001 * n * U24 + tw["eps_max"] + U22) * tw["abs_" + name] + U24 * np.abs(tw[name])
            + (terms + 1) * 2.0 ** -148 * max(1.0, float(other)))


def exact(src_emb, tgt_emb, x):
    """corr (3, N) of one sample in plain float64: exact scores, no float32 anywhere."""
    zd = src_emb.astype(F64).T @ tgt_emb.astype(F64) / np.sqrt(F64(src_emb.shape[0]))
    e = np.exp(zd - zd.max(1, keepdims=True))
    return x.astype(F64) @ (e / e.sum(1, keepdims=True)).T


KINDS = ("random", "ascending", "one_hot", "equal")


def make_case(C, N, M, B=1, sigma=1.0, kind="random", seed=0):
    """src_emb (B, C, N), tgt_emb (B, C, M), tgt (B, 3, M), g (B, 3, N), all float32.  sigma: the scale of the embeddings
    (scores of about sigma^2).  random: normal embeddings.  ascending: a row's scores rise with k (the maximum rises in every
    tile).  one_hot: one column per row dominates the others by more than 100.  equal: all scores identical."""
    rs = np.random.default_rng([seed, C, N, M, B, KINDS.index(kind)])
    se = (sigma * rs.standard_normal((B, C, N))).astype(F32)
    te = (sigma * rs.standard_normal((B, C, M))).astype(F32)
    if kind == "ascending":   # channel 0 carries a ramp over k that outgrows the noise of the others
        se[:, 0, :] = F32(sigma) * (1.0 + rs.uniform(0.0, 1.0, (B, N))).astype(F32)
        te *= F32(0.01 / np.sqrt(C))
        te[:, 0, :] = (sigma * np.sqrt(C) * np.arange(M) / 8.0).astype(F32)[None]
    elif kind == "one_hot":   # channel 0 gives column (2 M) // 3 a score of 150 .. 300 in every row, the others stay near 0
        se[:, 0, :] = F32(sigma) * (1.0 + rs.uniform(0.0, 1.0, (B, N))).astype(F32)
        te *= F32(0.01 / np.sqrt(C))
        te[:, 0, :] = 0.0
        te[:, 0, (2 * M) // 3] = F32(150.0 * np.sqrt(C) / sigma)
    elif kind == "equal":
        se = np.full((B, C, N), F32(sigma * 0.5))
        te = np.full((B, C, M), F32(sigma * 0.25))
    x = rs.uniform(-1.0, 1.0, (B, 3, M)).astype(F32)
    g = rs.standard_normal((B, 3, N)).astype(F32)
    return se, te, x, g
