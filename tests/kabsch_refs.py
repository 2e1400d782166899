"""Float64 twins of the closed-form rigid fit and the ICP loop around it (include/rrl.h rrl_kabsch_fwd, rrl_kabsch_bwd,
rrl_icp_step_batch, rrl_icp_epoch).  numpy for the values, torch float64 for autograd; nothing here
touches a GPU or the library.

Row convention: x -> x R + T.  wn = w / (sum w + eps), abar = sum wn a, bbar = sum wn b, H = sum wn (a - abar)^T (b - bbar)
= U S V^T, delta = det(U V^T), R = U diag(1, 1, delta) V^T, T = bbar - abar R.
"""
import numpy as np
import torch

FIT_OK, FIT_FEW, FIT_DEGENERATE, ICP_DONE = 0, 1, 2, 3
ALL_ONES = 0xFFFFFFFFFFFFFFFF


def select_pairs(a, b, w=None, keys=None, count_a=None, count_b=None, gate_sq=None):
    """The pairs of ONE sample as the kernel selects them: (a rows, b rows, w, key distance words, skipped).  a (n, >= 3),
    b (m, >= 3) float32; keys (n,) uint64 or None (b[i] pairs with a[i])."""
    n, m = a.shape[0], b.shape[0]
    ca = n if count_a is None else min(max(int(count_a), 0), n)
    cb = m if count_b is None else min(max(int(count_b), 0), m)
    rows, cols, dist, skipped = [], [], [], 0
    for i in range(n):
        if i >= ca:
            skipped += 1
            continue
        if keys is not None:
            key = int(keys[i])
            idx, d = key & 0xFFFFFFFF, np.array([key >> 32], np.uint32).view(np.float32)[0]
            if key == ALL_ONES or idx >= m or idx >= cb:
                skipped += 1
                continue
            if gate_sq is not None and d > np.float32(gate_sq):
                continue
        else:
            idx, d = i, np.float32(0.0)
            if i >= cb:
                skipped += 1
                continue
        rows.append(i); cols.append(idx); dist.append(d)
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    ww = np.ones(len(rows)) if w is None else np.asarray(w, np.float64)[rows]
    return (np.asarray(a, np.float64)[rows, :3], np.asarray(b, np.float64)[cols, :3], ww, np.asarray(dist, np.float64), skipped)


def fit_pairs(pa, pb, w, dist=None, eps=0.0, rank_tol=1e-6, transpose_r=False, skipped=0):
    """The fit of selected pairs pa, pb (k, 3), w (k,) in float64 with numpy's SVD -> dict(R, T, W, abar, bbar, S, delta, H,
    res_after, key_mean, info = [pairs, status, reflected, skipped], gap, terms).  terms: sum |term| of every moment, for the
    bounds ((k + 2) 2^-52 sum|terms|): W, abar, bbar (3 each) and H (3 x 3; its singular values move by at most |dH|_F)."""
    k = len(w)
    W = float(w.sum())
    out = dict(W=W, info=[k, FIT_OK, 0, skipped], R=np.eye(3), T=np.zeros(3), abar=np.zeros(3), bbar=np.zeros(3), S=np.zeros(3),
               delta=0.0, res_after=0.0, key_mean=0.0, gap=0.0, H=np.zeros((3, 3)))
    if k < 3 or not W > 0.0:
        out["info"][1] = FIT_FEW
        return out
    wn = w / (W + eps)
    abar, bbar = (wn[:, None] * pa).sum(0), (wn[:, None] * pb).sum(0)
    ac, bc = pa - abar, pb - bbar
    H = ac.T @ (bc * wn[:, None])
    U, S, Vt = np.linalg.svd(H)
    delta = 1.0 if np.linalg.det(U @ Vt) > 0 else -1.0
    R = U @ np.diag([1.0, 1.0, delta]) @ Vt
    T = bbar - abar @ R
    gap = S[1] + delta * S[2]
    m2 = float((wn * (ac ** 2).sum(1)).sum() + (wn * (bc ** 2).sum(1)).sum())
    res = max(m2 - 2.0 * (S[0] + gap), 0.0)
    c = float(wn.sum())
    terms = dict(W=float(np.abs(w).sum()), abar=(np.abs(wn)[:, None] * np.abs(pa)).sum(0), bbar=(np.abs(wn)[:, None] * np.abs(pb)).sum(0),
                 H=np.abs(pa).T @ (np.abs(pb) * np.abs(wn)[:, None]) + (2.0 + c) * np.abs(abar)[:, None] * np.abs(bbar)[None, :],
                 # res_after combines second moments, each at most sum wn (|a|^2 + |b|^2) (|a_j b_k| <= (a_j^2 + b_k^2) / 2)
                 res=4.0 * float((np.abs(wn) * ((pa ** 2).sum(1) + (pb ** 2).sum(1))).sum()),
                 key=float((np.abs(wn) * np.abs(dist)).sum()) if dist is not None else 0.0)
    out.update(R=R.T if transpose_r else R, T=T, abar=abar, bbar=bbar, S=S, delta=delta, H=H, gap=gap, res_after=res, terms=terms,
               key_mean=float((wn * dist).sum()) if dist is not None else 0.0, U=U, V=Vt.T)
    out["info"][1] = FIT_DEGENERATE if gap <= rank_tol * S[0] else FIT_OK
    out["info"][2] = int(delta < 0)
    return out


def fit(a, b, w=None, keys=None, count_a=None, count_b=None, gate_sq=None, eps=0.0, rank_tol=1e-6, transpose_r=False):
    """One sample, from the kernel's inputs."""
    pa, pb, ww, dist, skipped = select_pairs(a, b, w, keys, count_a, count_b, gate_sq)
    return fit_pairs(pa, pb, ww, dist, eps, rank_tol, transpose_r, skipped)


def residual_direct(pa, pb, w, R, T, eps=0.0):
    """sum wn |a R + T - b|^2, evaluated pair by pair (R in the row convention)."""
    wn = w / (w.sum() + eps)
    return float((wn * ((pa @ R + T - pb) ** 2).sum(1)).sum())


def fit_torch(a, b, w, eps=0.0, transpose_r=False):
    """The dense fit of a batch in torch float64, differentiable: a, b (B, n, 3), w (B, n) -> R (B, 3, 3), T (B, 3).  DCP's
    SVDHead (dcp/model.py:405-455) is the w = 1, eps = 0 case of it with R^T and channel-first clouds; RPM's
    compute_rigid_transform (rpm/models/rpmnet.py:121-157) the eps = 1e-5 case."""
    wn = w / (w.sum(1, keepdim=True) + eps)
    abar, bbar = (wn[..., None] * a).sum(1), (wn[..., None] * b).sum(1)
    H = (a - abar[:, None]).transpose(1, 2) @ ((b - bbar[:, None]) * wn[..., None])
    U, S, Vh = torch.linalg.svd(H)
    delta = torch.where(torch.linalg.det(U @ Vh) > 0, 1.0, -1.0).to(H.dtype)
    D = torch.diag_embed(torch.stack([torch.ones_like(delta), torch.ones_like(delta), delta], -1))
    R = U @ D @ Vh
    T = bbar - (abar[:, None] @ R)[:, 0]
    return (R.transpose(1, 2) if transpose_r else R), T


def rpm_transform(a, b, w):
    """(B, 3, 4) as rpm's compute_rigid_transform returns it: [R^T | T]."""
    R, T = fit_torch(a, b, w, eps=1e-5, transpose_r=True)
    return torch.cat([R, T[..., None]], 2)


def dcp_head(src, src_corr):
    """DCP's SVDHead on channel-first clouds (B, 3, n): (R (B, 3, 3) moving column vectors, t (B, 3))."""
    a, b = src.transpose(1, 2), src_corr.transpose(1, 2)
    return fit_torch(a, b, torch.ones(a.shape[:2], dtype=a.dtype), eps=0.0, transpose_r=True)


def grads_torch(a, b, w, gR, gT, eps=0.0, transpose_r=False):
    """float64 autograd of <gR, R> + <gT, T> with respect to a, b, w (numpy in, numpy out)."""
    ta, tb, tw = (torch.tensor(np.asarray(x, np.float64), requires_grad=True) for x in (a, b, w))
    R, T = fit_torch(ta, tb, tw, eps, transpose_r)
    ((R * torch.tensor(np.asarray(gR, np.float64))).sum() + (T * torch.tensor(np.asarray(gT, np.float64))).sum()).backward()
    return ta.grad.numpy(), tb.grad.numpy(), tw.grad.numpy()


def rotation_angle(R0, R1):
    E = R0.T @ R1
    v = np.array([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]])
    return float(np.arctan2(0.5 * np.linalg.norm(v), 0.5 * (np.trace(E) - 1.0)))


def step_lengths(Rk, Tk, abar, R, T):
    """(angle, centroid motion) in float64, the additions in the kernel's order."""
    Rk, Tk, R, T, ab = (np.asarray(x, np.float64) for x in (Rk, Tk, R, T, abar))
    E = np.empty((3, 3))
    for i in range(3):
        for j in range(3):
            E[i, j] = (R[0, i] * Rk[0, j] + R[1, i] * Rk[1, j]) + R[2, i] * Rk[2, j]
    vx, vy, vz = E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]
    ang = np.arctan2(0.5 * np.sqrt((vx * vx + vy * vy) + vz * vz), 0.5 * (((E[0, 0] + E[1, 1]) + E[2, 2]) - 1.0))
    mv2 = 0.0
    for k in range(3):
        now = ((ab[0] * Rk[0, k] + ab[1] * Rk[1, k]) + ab[2] * Rk[2, k]) + Tk[k]
        was = ((ab[0] * R[0, k] + ab[1] * R[1, k]) + ab[2] * R[2, k]) + T[k]
        mv2 += (now - was) * (now - was)
    return float(ang), float(np.sqrt(mv2))


def icp_step(Rk, Tk, status, abar, R, T, state, tol_rot, tol_trans, patience):
    """The step rule of rrl_icp_step_batch for one pair, float64: -> (R, T, last_step or None, state).  state = [epochs, calm
    epochs, done epoch or -1, what this call did]."""
    epochs, done_at = state[0] + 1, state[2]
    if done_at >= 0:
        return R, T, None, [epochs, state[1], done_at, ICP_DONE]
    if status != FIT_OK or not (np.isfinite(Rk).all() and np.isfinite(Tk).all()):
        return R, T, None, [epochs, 0, -1, status if status != FIT_OK else FIT_DEGENERATE]
    ang, mv = step_lengths(Rk, Tk, abar, R, T)
    calm = state[1] + 1 if (patience > 0 and np.float32(ang) < np.float32(tol_rot) and np.float32(mv) < np.float32(tol_trans)) else 0
    done = epochs if (patience > 0 and calm >= patience) else -1
    return Rk, Tk, (ang, mv), [epochs, calm, done, FIT_OK]


def stepped_fit(R, T, ang, mv):
    """(Rk, Tk) float32: the pose (R, T) turned by `ang` about z and shifted by `mv` along x.  With abar = 0 the two step
    lengths the rule measures from it are (ang, mv), up to the float32 rounding of the entries (1e-7)."""
    c, s = np.cos(ang), np.sin(ang)
    Rz = np.array([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]])
    return (np.asarray(R, np.float64) @ Rz).astype(np.float32), (np.asarray(T, np.float64) + [mv, 0.0, 0.0]).astype(np.float32)


def icp_epoch_from_keys(src, tar, keys, R, T, state, count1=None, count2=None, gate_sq=None, tol_rot=0.0, tol_trans=0.0, patience=0):
    """The host ICP epoch of one pair from GIVEN keys (those the walk left for the moved source): fit of the source as given
    against the keyed targets, then the step rule -> (fit dict, R, T, last_step, state)."""
    f = fit(src, tar, None, keys, count1, count2, gate_sq)
    Rn, Tn, last, st = icp_step(f["R"].astype(np.float32), f["T"].astype(np.float32), f["info"][1], f["abar"], R, T, state, tol_rot,
                                tol_trans, patience)
    return f, Rn, Tn, last, st
