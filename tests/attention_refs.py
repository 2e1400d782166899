"""Host twins of the attention node (include/rrl.h rrl_attention_fwd / rrl_attention_bwd), numpy only.

`scores` restates the header's step 1 bit for bit with pointer_refs' exact fmaf: one float32 chain per score over a head's
channels ascending, then one float32 multiplication by sc = float32(1 / sqrt(double(DK))).  `forward_rule` restates steps 2 and
3 in the rule's own arithmetic (float32 p, the column chain of o by the same fmaf, L in double, one final rounding), with
numpy's float32 exp in the place of the device's expf -- the one operation the two do not share bit for bit, so its results
are compared within `evaluate`'s bounds, not as bits.  `evaluate` is the float64 evaluation of the same z: softmax weights,
out and the three gradients by the header's formulas, each with the bound the GPU tests hold the device to.

The bounds (u = 2^-24; w the float64 weights of a row, z and M its float32 scores and their maximum; every sum over the
valid columns or rows only):
  eps_k     = 2^-23 + u |z_k - M|: one expf within an ulp (2^-23 of its value) of the exponential of its float32 argument,
              and that argument z_k - M rounded once (u |z_k - M| absolute, so as much relative in the exponential).
  out       p_k = e_k (1 + e), |e| <= eps_k, gives weights w_k (1 + e_k) / (1 + ebar), ebar = sum w e: as sum w_k (v_k - out) = 0
              the mean drops out and |out' - out| <= 1.001 sum_k w_k eps_k |v_kc - out_c|.  The column chain rounds nt times, each
              within u of a partial sum that sum_k p_k |v_kc| bounds: 1.001 nt u sum_k w_k |v_kc| after the division.  L is a
              double sum of float32 terms (nt 2^-53: nothing).  The final rounding: u |out|.
  Pn        = float32(expf() / L): relative eP_k = eps_k + ebar_j + u, ebar_j = sum_k w_k eps_k the error of L.
  delta_j   uses the DEVICE's out: |delta' - delta| <= D_j = sum_c |g_jc| out_bound_jc.
  dP        a float32 chain of DK terms: 1.001 DK u sum_c |g_jc v_kc|.
  ds        = float32(Pn (dP - delta) sc); with A_jk = sc w_jk (sum_c |g v| + sum_c |g out|) -- the two terms of the difference
              by their magnitudes, it cancels --: |ds' - ds| <= A_jk (eP_jk + 1.001 DK u + u) + sc w_jk D_j.
  d_v[k][c] the chain over j of g Pn: 1.001 nq u sum_j |g_jc| w_jk (1 + eP_jk) + sum_j |g_jc| w_jk eP_jk.
  d_q[j][c] the chain over k of ds k, |ds'| <= A + |ds' - ds|: 1.001 nt u sum_k (A_jk + |ds' - ds|) |k_kc| + sum_k |ds' - ds| |k_kc|;
            d_k[k][c] likewise over j with q and nq.
  underflow no relative bound covers float32 below 2^-126: an expf, a Pn, a ds or a chain's partial sum there is rounded to a
              multiple of 2^-149 (pointer_refs.grad_bound): (terms + 1) 2^-148 max(1, other factor) is added to every bound.
"""
import numpy as np

import pointer_refs as PR

F32, F64 = np.float32, np.float64
U = 2.0 ** -24


def scale(DK):
    return F32(1.0 / np.sqrt(F64(DK)))


def heads(x, H):
    """(T, H DK) token-major -> (H, T, DK)."""
    T, D = x.shape
    return np.ascontiguousarray(x.reshape(T, H, D // H).transpose(1, 0, 2))


def merge(x):
    """(H, T, DK) -> (T, H DK)."""
    H, T, DK = x.shape
    return np.ascontiguousarray(x.transpose(1, 0, 2).reshape(T, H * DK))


def scores(q, k, H):
    """z (H, N, M) float32 of one sample, the header's step 1: q (N, H DK), k (M, H DK)."""
    qh, kh = heads(q, H), heads(k, H)
    sc = scale(qh.shape[2])
    return np.stack([(PR.chains(np.ascontiguousarray(qh[h].T), np.ascontiguousarray(kh[h].T)) * sc).astype(F32) for h in range(H)])


def forward_rule(z, v, H, nq=None, nt=None):
    """Steps 2 and 3 in the rule's arithmetic, numpy's float32 exp for expf: dict with out (N, H DK) float32, rowmax (H, N)
    float32 (bit for bit the device's kept M_j) and L (H, N) float64."""
    _, N, M = z.shape
    nq, nt = N if nq is None else nq, M if nt is None else nt
    vh = heads(v, H)
    out = np.zeros((H, N, vh.shape[2]), F32)
    rowmax, L = np.zeros((H, N), F32), np.zeros((H, N))
    if nq and nt:
        for h in range(H):
            zz = z[h, :nq, :nt]
            rowmax[h, :nq] = zz.max(1)
            with np.errstate(invalid="ignore"):
                p = np.where(np.isneginf(zz), F32(0), np.exp((zz - rowmax[h, :nq, None]).astype(F32)).astype(F32)).astype(F32)
            half = (np.arange(nt) >> 2) & 1   # the lane half that sums column k: each half ascending, then the two added
            L[h, :nq] = (np.cumsum(p[:, half == 0].astype(F64), axis=1)[:, -1] if (half == 0).any() else 0.0) + \
                        (np.cumsum(p[:, half == 1].astype(F64), axis=1)[:, -1] if (half == 1).any() else 0.0)
            o = PR.chains(np.ascontiguousarray(p.T), np.ascontiguousarray(vh[h, :nt]))          # (nq, DK): the chain over k ascending
            out[h, :nq] = (o.astype(F64) / L[h, :nq, None]).astype(F32)
    return dict(out=merge(out), rowmax=rowmax, L=L)


def evaluate(z, v, H, nq=None, nt=None, g=None, q=None, k=None, sc=None):
    """The float64 evaluation of one sample from scores z (H, N, M) -- the twin's float32 z, or exact float64 scores with sc
    the exact 1 / sqrt(DK) --: dict with w (H, N, M), out (N, H DK), out_bound, and with g (N, H DK), q, k the gradients d_q, d_k,
    d_v with d_q_bound, d_k_bound, d_v_bound (the module docstring derives them)."""
    _, N, M = z.shape
    nq, nt = N if nq is None else nq, M if nt is None else nt
    vh = heads(v, H).astype(F64)
    DK = vh.shape[2]
    zd = z.astype(F64)
    w, eps = np.zeros((H, N, M)), np.zeros((H, N, M))
    if nq and nt:
        zz = zd[:, :nq, :nt]
        mx = zz.max(2, keepdims=True)
        e = np.exp(zz - mx)
        w[:, :nq, :nt] = e / e.sum(2, keepdims=True)
        eps[:, :nq, :nt] = 2.0 ** -23 + U * np.abs(zz - mx)
    out = np.einsum("hjk,hkc->hjc", w, vh)
    spread = np.stack([np.einsum("jk,jkc->jc", (w * eps)[h], np.abs(vh[h][None, :, :] - out[h][:, None, :])) for h in range(H)])
    vmax = float(np.abs(vh[:, :nt]).max()) if nt else 0.0
    floor = (nt + 1) * 2.0 ** -148 * max(1.0, vmax)
    out_bound = (1.001 * spread + 1.001 * nt * U * np.einsum("hjk,hkc->hjc", w, np.abs(vh))
                 + U * np.abs(out) + floor)
    out_bound[:, nq:] = 0.0
    if not nt:
        out_bound[:] = 0.0
    res = dict(w=w, eps=eps, out=merge(out), out_bound=merge(out_bound))
    if g is None:
        return res
    gh, qh, kh = heads(g, H).astype(F64), heads(q, H).astype(F64), heads(k, H).astype(F64)
    gh[:, nq:] = 0.0
    qh[:, nq:] = 0.0
    kh[:, nt:] = 0.0
    vz = vh.copy()
    vz[:, nt:] = 0.0
    sc = F64(scale(DK)) if sc is None else F64(sc)
    ebar = (w * eps).sum(2)                                                                  # (H, N)
    eP = eps + ebar[:, :, None] + U
    delta = (gh * out).sum(2)
    D = (np.abs(gh) * out_bound).sum(2)
    dP = np.einsum("hjc,hkc->hjk", gh, vz)
    mag = np.einsum("hjc,hkc->hjk", np.abs(gh), np.abs(vz)) + (np.abs(gh) * np.abs(out)).sum(2)[:, :, None]
    ds = w * (dP - delta[:, :, None]) * sc
    A = sc * w * mag
    Eds = A * (eP + 1.001 * DK * U + U) + sc * w * D[:, :, None]
    d_v = np.einsum("hjk,hjc->hkc", w, gh)
    d_q = np.einsum("hjk,hkc->hjc", ds, kh)
    d_k = np.einsum("hjk,hjc->hkc", ds, qh)
    big = lambda x: float(np.abs(x).max()) if x.size else 0.0  # noqa: E731
    other = sc * big(mag) * max(big(kh), big(qh), 1.0)
    d_v_bound = (1.001 * nq * U * np.einsum("hjk,hjc->hkc", w * (1 + eP), np.abs(gh)) + np.einsum("hjk,hjc->hkc", w * eP, np.abs(gh))
                 + (nq + 1) * 2.0 ** -148 * max(1.0, big(gh)))
    d_q_bound = (1.001 * nt * U * np.einsum("hjk,hkc->hjc", A + Eds, np.abs(kh)) + np.einsum("hjk,hkc->hjc", Eds, np.abs(kh))
                 + (nt + 1) * 2.0 ** -148 * max(1.0, other))
    d_k_bound = (1.001 * nq * U * np.einsum("hjk,hjc->hkc", A + Eds, np.abs(qh)) + np.einsum("hjk,hjc->hkc", Eds, np.abs(qh))
                 + (nq + 1) * 2.0 ** -148 * max(1.0, other))
    d_q_bound[:, nq:] = 0.0
    d_k_bound[:, nt:] = 0.0
    d_v_bound[:, nt:] = 0.0
    if not (nq and nt):
        d_q_bound[:], d_k_bound[:], d_v_bound[:] = 0.0, 0.0, 0.0
    res.update(ds=ds, d_q=merge(d_q), d_k=merge(d_k), d_v=merge(d_v), d_q_bound=merge(d_q_bound), d_k_bound=merge(d_k_bound),
               d_v_bound=merge(d_v_bound))
    return res


def exact_scores(q, k, H):
    """(H, N, M) float64: exact products and sums, the exact scale."""
    qh, kh = heads(q, H).astype(F64), heads(k, H).astype(F64)
    return np.einsum("hjc,hkc->hjk", qh, kh) / np.sqrt(F64(qh.shape[2]))


def score_bound(q, k, H):
    """|twin z - exact z| <= (1.001 DK u + 2 u) sum_c |q k| / sqrt(DK): the chain, the rounding of sc and the multiplication."""
    qh, kh = heads(q, H).astype(F64), heads(k, H).astype(F64)
    DK = qh.shape[2]
    return (1.001 * DK * U + 2 * U) * np.einsum("hjc,hkc->hjk", np.abs(qh), np.abs(kh)) / np.sqrt(F64(DK))


KINDS = ("random", "one_hot", "equal")


def make_case(B, H, DK, N, M, sigma=1.0, kind="random", seed=0):
    """q (B, N, H DK), k, v (B, M, H DK), g (B, N, H DK), float32.  sigma: the scale of q and k (scores of about sigma^2 in
    spread).  random: normal q and k.  one_hot: one column per row and head dominates the others by more than 100.  equal: all
    scores of a head identical."""
    rs = np.random.default_rng([seed, B, H, DK, N, M, KINDS.index(kind)])
    q = (sigma * rs.standard_normal((B, N, H, DK))).astype(F32)
    k = (sigma * rs.standard_normal((B, M, H, DK))).astype(F32)
    if kind == "one_hot":   # channel 0 of every head gives column (2 M) // 3 a score of 150 .. 300, the others stay near 0
        q[..., 0] = F32(sigma) * (1.0 + rs.uniform(0.0, 1.0, (B, N, H))).astype(F32)
        k *= F32(0.01 / np.sqrt(DK))
        k[..., 0] = 0.0
        k[:, (2 * M) // 3, :, 0] = F32(150.0 * np.sqrt(DK) / sigma)
    elif kind == "equal":
        q = np.full((B, N, H, DK), F32(sigma * 0.5))
        k = np.full((B, M, H, DK), F32(sigma * 0.25))
    v = rs.uniform(-1.0, 1.0, (B, M, H * DK)).astype(F32)
    g = rs.standard_normal((B, N, H * DK)).astype(F32)
    return q.reshape(B, N, H * DK), k.reshape(B, M, H * DK), v, g
