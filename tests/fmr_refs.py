"""Host twins of FMR's inverse-compositional head (include/rrl.h rrl_ic_*), numpy float64 only.

The three rules and their backwards as the header states them -- the same expressions, the sums in plain float64 (the order of
a float64 sum is inside every bound below) --, the open loop (recorded features in, poses out) and a closed loop around a given
encoder callable.  perturb_fwd is the exception: it restates the float32 chain bit for bit with pointer_refs.fmaf32.

Every function that a GPU test holds the device to also returns the sum of the magnitudes of its terms: the bounds are
    final rounding + (number of terms) 2^-53 sum|terms|      (+ kappa(H) times the same where H^-1 enters)
(section 23 derives them); bound() below is that expression.
"""
import numpy as np

from pointer_refs import fmaf32

F32, F64 = np.float32, np.float64
U24, U53 = 2.0 ** -24, 2.0 ** -53
SMALL = 64          # the operations of the 6 x 6 / 4 x 4 algebra behind a sum, counted generously
WS_DOUBLES = 40
TINY = 2.0 ** -149  # float32's underflow quantum


def exp6(x):
    """exp(x) (4, 4) of a twist x = (w, v): rrl_se3_exp's expressions in float64 (the header's rule)."""
    x = np.asarray(x, F64)
    a, b, c = x[0], x[1], x[2]
    n2 = a * a + b * b + c * c
    t = np.sqrt(n2) if n2 > 0.0 else 0.0
    t2 = t * t
    if abs(t) < 0.01:
        s1 = 1.0 - t2 / 6.0 * (1.0 - t2 / 20.0 * (1.0 - t2 / 42.0))
        s2 = 0.5 * (1.0 - t2 / 12.0 * (1.0 - t2 / 30.0 * (1.0 - t2 / 56.0)))
        s3 = (1.0 / 6.0) * (1.0 - t2 / 20.0 * (1.0 - t2 / 42.0 * (1.0 - t2 / 72.0)))
    else:
        sn, cs = np.sin(t), np.cos(t)
        s1, s2, s3 = sn / t, (1.0 - cs) / (t * t), (t - sn) / (t * t * t)
    W = np.array([[0.0, -c, b], [c, 0.0, -a], [-b, a, 0.0]])
    S = W @ W
    E = np.eye(4)
    E[:3, :3] = np.eye(3) + s1 * W + s2 * S
    E[:3, 3] = (np.eye(3) + s2 * W + s3 * S) @ x[3:]
    return E


def genmat():
    """The six generators (6, 4, 4) (se_math/se3.py genmat)."""
    G = np.zeros((6, 4, 4))
    for k in range(3):
        a, b = (k + 1) % 3, (k + 2) % 3
        G[k, b, a], G[k, a, b] = 1.0, -1.0
        G[3 + k, k, 3] = 1.0
    return G


GEN = genmat()


def gen_dot(M, E):
    """q[k] = sum_ij M_ij [gen_k E]_ij and the same sum of magnitudes; M, E (4, 4)."""
    GE = GEN @ E
    return (M[None] * GE).sum((1, 2)), (np.abs(M)[None] * np.abs(GE)).sum((1, 2))


def bound(value, terms, n, kappa=0.0):
    """2^-24 |value| + (n + SMALL) 2^-53 (1 + kappa) sum|terms| + float32's underflow quantum."""
    return U24 * np.abs(value) + (n + SMALL) * U53 * (1.0 + kappa) * terms + TINY


# ---- 1. perturb ------------------------------------------------------------------------------------------------------------
def perturbations(dt):
    """D (6, 4, 4) float64 of one sample: D_i = exp(-dt_i e_i)."""
    return np.stack([exp6(-F64(dt[i]) * np.eye(6)[i]) for i in range(6)])


def perturb_fwd(p0, dt):
    """out (B, 6, N, 3) float32, bit for bit the header's chain: D rounded once, then per point
    out_j = fmaf(p_2, D[j][2], fmaf(p_1, D[j][1], p_0 * D[j][0])) + D[j][3]."""
    B, N = p0.shape[:2]
    out = np.empty((B, 6, N, 3), F32)
    for b in range(B):
        D = perturbations(dt[b]).astype(F32)
        for i in range(6):
            for j in range(3):
                s = (p0[b, :, 0] * D[i, j, 0]).astype(F32)
                s = fmaf32(p0[b, :, 2], np.full(N, D[i, j, 2], F32), fmaf32(p0[b, :, 1], np.full(N, D[i, j, 1], F32), s))
                out[b, i, :, j] = (s + D[i, j, 3]).astype(F32)
    return out


def perturb_exact(p0, dt):
    """out (B, 6, N, 3) in plain float64 (for finite differences)."""
    p, out = p0.astype(F64), []
    for b in range(p0.shape[0]):
        D = perturbations(dt[b])
        out.append(np.einsum("ijk,nk->inj", D[:, :3, :3], p[b]) + D[:, None, :3, 3])
    return np.stack(out)


def perturb_bwd(p0, dt, g_out):
    """g_dt (B, 6) float64 and the sums of magnitudes: -sum_jk M_jk [gen_i D_i]_jk, M = sum_n g_out[n] (x) [p_n; 1]."""
    B, N = p0.shape[:2]
    g_dt, mag = np.zeros((B, 6)), np.zeros((B, 6))
    hom = np.concatenate([p0.astype(F64), np.ones((B, N, 1))], 2)
    for b in range(B):
        D = perturbations(dt[b])
        for i in range(6):
            M, Ma = np.zeros((4, 4)), np.zeros((4, 4))
            M[:3] = g_out[b, i].astype(F64).T @ hom[b]
            Ma[:3] = np.abs(g_out[b, i].astype(F64)).T @ np.abs(hom[b])
            q, _ = gen_dot(M, D[i])
            _, qa = gen_dot(Ma, D[i])
            g_dt[b, i], mag[b, i] = -q[i], qa[i]
    return g_dt, mag


# ---- 2. pinv ---------------------------------------------------------------------------------------------------------------
def chol_inverse(H, tol_rel):
    """(H^-1, ok) by the header's unpivoted Cholesky, column c solved from e_c; ok is False for a pivot p_j that fails
    p_j > tol_rel H_jj, p_j > 0, p_j < inf, or an inverse that is not finite."""
    L, ok = np.zeros((6, 6)), True
    with np.errstate(all="ignore"):
        for j in range(6):
            p = H[j, j]
            for q in range(j):
                p -= L[j, q] * L[j, q]
            if not (p > tol_rel * H[j, j]) or not (p > 0.0) or not (p < np.inf):
                ok, p = False, 1.0
            d = np.sqrt(p)
            L[j, j] = d
            for i in range(j + 1, 6):
                v = H[i, j]
                for q in range(j):
                    v -= L[i, q] * L[j, q]
                L[i, j] = v / d
        Hi = np.zeros((6, 6))
        for c in range(6):
            y, x = np.zeros(6), np.zeros(6)
            for i in range(6):
                v = 1.0 if i == c else 0.0
                for q in range(i):
                    v -= L[i, q] * y[q]
                y[i] = v / L[i, i]
            for i in range(5, -1, -1):
                v = y[i]
                for q in range(i + 1, 6):
                    v -= L[q, i] * x[q]
                x[i] = v / L[i, i]
            Hi[:, c] = x
    return Hi, ok and bool(np.isfinite(Hi).all())


def pinv_fwd(f0, fp, dt):
    """One sample: f0 (K,), fp (6, K), dt (6,) float32 -> dict J (K, 6), H, Hinv, pinv (6, K) float64, flag, kappa = cond_2(H),
    mag (6, K) = sum_j |H^-1_ij| |J_kj|.  A flagged sample has pinv = Hinv = 0."""
    K = f0.shape[0]
    fin = bool(np.isfinite(f0).all() and np.isfinite(fp).all() and np.isfinite(dt).all())
    bad = K < 6 or not fin or bool((dt == 0).any())
    with np.errstate(all="ignore"):
        J = (f0.astype(F64)[:, None] - fp.astype(F64).T) / dt.astype(F64)[None, :]
        H = J.T @ J
        Hi, ok = chol_inverse(H, (K + 6) * 2.0 ** -52)
    if bad or not ok:
        return dict(J=J, H=H, Hinv=np.zeros((6, 6)), pinv=np.zeros((6, K)), flag=1, kappa=np.inf, mag=np.zeros((6, K)))
    return dict(J=J, H=H, Hinv=Hi, pinv=Hi @ J.T, flag=0, kappa=float(np.linalg.cond(H)), mag=np.abs(Hi) @ np.abs(J).T)


def pinv_bwd(tw, dt, G):
    """The header's backward of one sample on pinv_fwd's dict: G (6, K) -> dict d_f0 (K,), d_fp (6, K), d_dt (6,) float64 and
    mag_* the same sums of magnitudes.  Flagged: zeros."""
    K = G.shape[1]
    if tw["flag"]:
        z = np.zeros
        return dict(d_f0=z(K), d_fp=z((6, K)), d_dt=z(6), mag_f0=z(K), mag_fp=z((6, K)), mag_dt=z(6))
    J, Hi, d = tw["J"], tw["Hinv"], dt.astype(F64)
    Gd = G.astype(F64)
    P = Gd @ J
    S = -(Hi @ P) @ Hi
    dJ = Gd.T @ Hi + J @ (S + S.T)                                   # (K, 6)
    Sa = (np.abs(Hi) @ (np.abs(Gd) @ np.abs(J))) @ np.abs(Hi)
    dJa = np.abs(Gd).T @ np.abs(Hi) + np.abs(J) @ (Sa + Sa.T)
    ad = np.abs(d)
    return dict(d_f0=(dJ / d).sum(1), d_fp=-(dJ / d).T, d_dt=-(dJ * J).sum(0) / d,
                mag_f0=(dJa / ad).sum(1), mag_fp=(dJa / ad).T, mag_dt=(dJa * np.abs(J)).sum(0) / ad)


# ---- 3. update -------------------------------------------------------------------------------------------------------------
def update_sums(pinv, f0, f1):
    """r (B, K) float32, dx (B, 6) float64 before its rounding, and mag (B, 6) = sum_k |pinv| |r|."""
    r = (f1.astype(F32) - f0.astype(F32)).astype(F32)
    with np.errstate(all="ignore"):
        dx = -np.einsum("bik,bk->bi", pinv.astype(F64), r.astype(F64))
        mag = np.einsum("bik,bk->bi", np.abs(pinv.astype(F64)), np.abs(r.astype(F64)))
    return r, dx, mag


def step_lengths(dx32):
    """n_b = float32(sqrt(sum_i double(dx_i)^2)), the sum ascending."""
    n2 = np.zeros(dx32.shape[0])
    with np.errstate(all="ignore"):
        for i in range(6):
            n2 = n2 + dx32[:, i].astype(F64) * dx32[:, i].astype(F64)
        return np.sqrt(n2).astype(F32)


def update_pose(dx32, g, xtol, stop):
    """(g_new (B, 4, 4) float64 before its rounding, mag, stopped) from the float32 dx: the batch stops when `stop` is set or
    every step length is < float32(xtol) (a NaN length is not)."""
    with np.errstate(all="ignore"):
        moving = bool((~(step_lengths(dx32) < F32(xtol))).any())
    stopped = 1 if (stop or not moving) else 0
    gd = g.astype(F64)
    if stopped:
        return gd.copy(), np.zeros_like(gd), 1
    with np.errstate(all="ignore"):
        E = np.stack([exp6(dx32[b]) for b in range(g.shape[0])])
        out, mag = E @ gd, np.abs(E) @ np.abs(gd)
    out[:, 3], mag[:, 3] = gd[:, 3], 0.0
    return out, mag, 0


def update_bwd(pinv, r, dx32, g, stopped, Gg=None, Gr=None, Gdx=None):
    """The header's backward on the kept r, dx and decision -> dict d_g (B, 4, 4), d_pinv (B, 6, K), d_f1, d_f0 (B, K)
    float64 and mag_*."""
    B, _, K = pinv.shape
    z = np.zeros
    Gg = z((B, 4, 4)) if Gg is None else Gg.astype(F64)
    Gr = z((B, K)) if Gr is None else Gr.astype(F64)
    Gdx = z((B, 6)) if Gdx is None else Gdx.astype(F64)
    if stopped:
        return dict(d_g=Gg.copy(), d_pinv=z((B, 6, K)), d_f1=Gr.copy(), d_f0=-Gr, mag_g=z((B, 4, 4)), mag_pinv=z((B, 6, K)),
                    mag_f1=z((B, K)), q=z((B, 6)))
    pd, rd, gd = pinv.astype(F64), r.astype(F64), g.astype(F64)
    d_g, mag_g, q, qa = z((B, 4, 4)), z((B, 4, 4)), z((B, 6)), z((B, 6))
    for b in range(B):
        E = exp6(dx32[b])
        d_g[b], mag_g[b] = E.T @ Gg[b], np.abs(E).T @ np.abs(Gg[b])
        M, Ma = Gg[b] @ gd[b].T, np.abs(Gg[b]) @ np.abs(gd[b]).T
        M[3], Ma[3] = 0.0, 0.0
        qb, qab = gen_dot(M, E)
        q[b], qa[b] = qb + Gdx[b], qab + np.abs(Gdx[b])
    d_pinv = -q[:, :, None] * rd[:, None, :]
    d_f1 = Gr - np.einsum("bik,bi->bk", pd, q)
    mag_f1 = np.abs(Gr) + np.einsum("bik,bi->bk", np.abs(pd), qa)
    return dict(d_g=d_g, d_pinv=d_pinv, d_f1=d_f1, d_f0=-d_f1, mag_g=mag_g, mag_pinv=qa[:, :, None] * np.abs(rd)[:, None, :],
                mag_f1=mag_f1, q=q)


# ---- loops -----------------------------------------------------------------------------------------------------------------
def head_pinv(f0, fp, dt):
    """pinv (B, 6, K) float32 and info (B,) of a batch, rounded as the device rounds."""
    tws = [pinv_fwd(f0[b], fp[b], dt[b]) for b in range(f0.shape[0])]
    return np.stack([t["pinv"] for t in tws]).astype(F32), np.array([t["flag"] for t in tws], np.int32), tws


def update_fwd(pinv, f0, f1, g, xtol, stop):
    """One whole update, rounded as the device rounds: r, dx, g_new float32 and the decision."""
    r, dx, _ = update_sums(pinv, f0, f1)
    dx32 = dx.astype(F32)
    g_new, _, stopped = update_pose(dx32, g, xtol, stop)
    return r, dx32, (g.copy() if stopped else g_new.astype(F32)), stopped


def open_loop(f0, fp, dt, f1_series, g_series_in, xtol):
    """The head on recorded features: pinv from (f0, fp, dt), then per iteration one update on the RECORDED f1 and incoming
    pose -> (pinv float32, info, [per iteration (r, dx32, g_new float32, stopped)])."""
    pinv, info, _ = head_pinv(f0, fp, dt)
    out, stop = [], 0
    for f1, g in zip(f1_series, g_series_in):
        step = update_fwd(pinv, f0, f1, g, xtol, stop)
        stop = step[3]
        out.append(step)
    return pinv, info, out


def closed_loop(encoder, p0, p1, dt, maxiter, xtol, g0=None):
    """ic_algo around `encoder` ((n, N, 3) float32 array -> (n, K) float32 array): returns (r, g, g_series (maxiter, B, 4, 4)
    float32, stop, info) with the library's deviation (after the stop the series holds the last pose)."""
    B, N = p0.shape[:2]
    dt = np.broadcast_to(np.asarray(dt, F32).reshape(-1, 6), (B, 6))
    g = np.broadcast_to(np.eye(4, dtype=F32), (B, 4, 4)).copy() if g0 is None else g0.astype(F32)
    f0 = encoder(p0)
    fp = encoder(perturb_fwd(p0, dt).reshape(6 * B, N, 3)).reshape(B, 6, -1)
    pinv, info, _ = head_pinv(f0, fp, dt)
    stop, series, r = 0, [], None
    for _ in range(maxiter):
        p = (np.einsum("bij,bnj->bni", g[:, :3, :3].astype(F64), p1.astype(F64)) + g[:, None, :3, 3]).astype(F32)
        r, _, g, stop = update_fwd(pinv, f0, encoder(p), g, xtol, stop)
        series.append(g)
    return r, g, np.stack(series), stop, info


def ellipsoid_cloud(rng, B, N, axes=(1.0, 0.6, 0.3)):
    """(B, N, 3) float32: points on an ellipsoid's surface, zero-meaned."""
    v = rng.standard_normal((B, N, 3))
    v /= np.linalg.norm(v, axis=2, keepdims=True)
    v = v * np.asarray(axes)
    return (v - v.mean(1, keepdims=True)).astype(F32)


def make_features(K, B=1, seed=0, dt=1e-2):
    """A synthetic well-conditioned head problem: f0 (B, K), fp (B, 6, K), dt (B, 6), f1 (B, K), G (B, 6, K) float32 --
    fp = f0 - dt_i J_i with random J, so cond(H) stays small for K >= 6."""
    rs = np.random.default_rng([seed, K, B])
    f0 = rs.standard_normal((B, K)).astype(F32)
    J = rs.standard_normal((B, 6, K))
    dts = np.full((B, 6), dt, F32) if np.isscalar(dt) else np.broadcast_to(np.asarray(dt, F32), (B, 6)).copy()
    fp = (f0[:, None, :] - dts[:, :, None].astype(F64) * J).astype(F32)
    f1 = (f0 + 0.05 * rs.standard_normal((B, K))).astype(F32)
    G = rs.standard_normal((B, 6, K)).astype(F32)
    return f0, fp, dts, f1, G
