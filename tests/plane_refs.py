"""Float64 numpy twins of the point-to-plane entries (include/rrl.h rrl_idx_normals, rrl_plane_normal_eq,
rrl_plane_step_batch) and a float64 restatement of both ICP loops on the host (scipy cKDTree pairing)."""
import math

import numpy as np

import group_refs as GR

ALL_ONES = 0xFFFFFFFFFFFFFFFF
FIT_OK, FIT_FEW = 0, 1
STEPPED, FEW, FAILED, DONE = 0, 1, 2, 3
H0, G0, W_, RES, KEYMEAN, USED, SKIPPED, DOUBLES = 0, 21, 27, 28, 29, 30, 31, 32
RANK_TOL = float(np.float32(1e-10))  # neighbors.NORMAL_RANK_TOL as the kernel receives it: a float32


# ---- rule 1: normals --------------------------------------------------------------------------------------------------------
def jacobi_eigh(C):
    """Eigenvalues (as found on the diagonal, unsorted) and eigenvectors (columns) of a symmetric 3 x 3 matrix by cyclic Jacobi
    rotations in the order (0, 1), (0, 2), (1, 2): the kernel's method, in Python floats."""
    A = [[float(C[i][j]) for j in range(3)] for i in range(3)]
    V = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    floor = 1e-22 * ((abs(A[0][0]) + abs(A[1][1])) + abs(A[2][2]))
    for _ in range(16):
        turned = False
        for p, q in ((0, 1), (0, 2), (1, 2)):
            apq = A[p][q]
            if apq == 0.0 or not abs(apq) > floor:
                continue
            turned = True
            r = 3 - p - q
            theta = (A[q][q] - A[p][p]) / (2.0 * apq)
            t = math.copysign(1.0, theta) / (abs(theta) + math.sqrt(1.0 + theta * theta))
            c = 1.0 / math.sqrt(1.0 + t * t)
            s = c * t
            app, aqq, arp, arq = A[p][p], A[q][q], A[r][p], A[r][q]
            A[p][p], A[q][q] = app - t * apq, aqq + t * apq
            A[p][q] = A[q][p] = 0.0
            A[r][p] = A[p][r] = c * arp - s * arq
            A[r][q] = A[q][r] = s * arp + c * arq
            for i in range(3):
                vp, vq = V[i][p], V[i][q]
                V[i][p], V[i][q] = c * vp - s * vq, s * vp + c * vq
        if not turned:
            break
    return [A[0][0], A[1][1], A[2][2]], V


def scatter(members):
    """(k, 3) float64 member points -> C = sum d d^T - k m m^T about the first member."""
    d = members - members[0]
    k = float(len(d))
    m = d.sum(0) / k
    return d.T @ d - k * np.outer(m, m)


def normal_of(C, rank_tol=RANK_TOL):
    """(normal (3,) float64, quality, (l0, l1, l2)) of one scatter matrix by rule 1; a zero normal where there is no plane."""
    zero = (np.zeros(3), 0.0, (0.0, 0.0, 0.0))
    if not np.isfinite(C).all():
        return zero
    lam, V = jacobi_eigh(C)
    c0 = 0
    if lam[1] < lam[c0]:
        c0 = 1
    if lam[2] < lam[c0]:
        c0 = 2
    rest = [lam[i] for i in range(3) if i != c0]
    l0, l1, l2 = lam[c0], min(rest), max(rest)
    if not l1 > rank_tol * l2:
        return zero
    e = np.array([V[0][c0], V[1][c0], V[2][c0]])
    big = e[0]
    if abs(e[1]) > abs(big):
        big = e[1]
    if abs(e[2]) > abs(big):
        big = e[2]
    return (-e if big < 0.0 else e), (l1 - l0) / l2, (l0, l1, l2)


def idx_normals(points, idx, found, counts=None, rank_tol=RANK_TOL):
    """points (B, n, >= 3) float32, idx (B, S, nsample), found (B, S) -> dict(normals (B, S, 3) float64, quality (B, S))."""
    points = np.asarray(points, np.float32)
    B, n = points.shape[:2]
    S, nsample = idx.shape[1], idx.shape[2]
    normals, quality = np.zeros((B, S, 3)), np.zeros((B, S))
    for b in range(B):
        nb = n if counts is None else min(max(int(counts[b]), 0), n)
        x = points[b, :, :3].astype(np.float64)
        for i in range(S):
            f = min(max(int(found[b, i]), 0), nsample)
            mem = [int(j) for j in idx[b, i, :f] if 0 <= int(j) < nb]
            if len(mem) < 3:
                continue
            normals[b, i], quality[b, i], _ = normal_of(scatter(x[mem]), rank_tol)
    return dict(normals=normals, quality=quality)


def estimate_normals(points, radius, nsample=64, counts=None, rank_tol=RANK_TOL):
    """neighbors.estimate_normals on the host: the ball groups of tests/group_refs.py (the query among its members), then rule 1.
    Also returns idx, found and border (rows with a member within rounding of the radius)."""
    g = GR.ball_group(points, None, radius, nsample, counts=counts, exclude_self=False)
    out = idx_normals(points, g["idx"], g["found"], counts, rank_tol)
    out.update(idx=g["idx"], found=g["found"], border=g["border"])
    return out


# ---- rule 2: the sums ---------------------------------------------------------------------------------------------------------
def select_pairs(moved, tar, normals, keys=None, count1=None, count2=None, gate_sq=None):
    """The pairs of ONE sample as the kernel selects them: (rows, partner rows, key distance words, skipped)."""
    n, m = moved.shape[0], tar.shape[0]
    c1 = n if count1 is None else min(max(int(count1), 0), n)
    c2 = m if count2 is None else min(max(int(count2), 0), m)
    rows, cols, dist, skipped = [], [], [], 0
    for i in range(n):
        if i >= c1:
            skipped += 1
            continue
        if keys is not None:
            key = int(keys[i])
            j, d = key & 0xFFFFFFFF, np.array([key >> 32], np.uint32).view(np.float32)[0]
            if key == ALL_ONES or j >= m or j >= c2:
                skipped += 1
                continue
            if gate_sq is not None and d > np.float32(gate_sq):
                continue
        else:
            j, d = i, np.float32(0.0)
            if i >= c2:
                skipped += 1
                continue
        nr = normals[j]
        if not np.isfinite(nr).all() or not nr.any():
            continue
        rows.append(i); cols.append(j); dist.append(d)
    return np.asarray(rows, np.int64), np.asarray(cols, np.int64), np.asarray(dist, np.float64), skipped


def normal_eq(moved, tar, normals, keys=None, count1=None, count2=None, w=None, gate_sq=None, pivot=None):
    """One sample -> dict(neq (32,), info [used, status, 0, skipped], sums (32,) before the division, terms (32,) = sum |term|
    of every sum, H (6, 6), g (6,))."""
    moved, tar, normals = np.asarray(moved, np.float32), np.asarray(tar, np.float32), np.asarray(normals, np.float32)
    rows, cols, dist, skipped = select_pairs(moved, tar, normals, keys, count1, count2, gate_sq)
    c = np.zeros(3) if pivot is None else np.asarray(pivot, np.float32).astype(np.float64)
    y, bt, nn = moved[rows, :3].astype(np.float64), tar[cols, :3].astype(np.float64), normals[cols].astype(np.float64)
    ww = np.ones(len(rows)) if w is None else np.asarray(w, np.float32).astype(np.float64)[rows]
    p, e = y - c, y - bt
    r = (e[:, 0] * nn[:, 0] + e[:, 1] * nn[:, 1]) + e[:, 2] * nn[:, 2]
    J = np.concatenate([np.cross(p, nn), nn], axis=1)
    sums, terms = np.zeros(DOUBLES), np.zeros(DOUBLES)
    at = 0
    for u in range(6):
        for v in range(u, 6):
            t = ww * J[:, u] * J[:, v]
            sums[H0 + at], terms[H0 + at] = t.sum(), np.abs(t).sum()
            at += 1
        t = ww * J[:, u] * r
        sums[G0 + u], terms[G0 + u] = t.sum(), np.abs(t).sum()
    sums[W_], terms[W_] = ww.sum(), np.abs(ww).sum()
    sums[RES], terms[RES] = (ww * (r * r)).sum(), np.abs(ww * (r * r)).sum()
    sums[KEYMEAN], terms[KEYMEAN] = (ww * dist).sum(), np.abs(ww * dist).sum()
    sums[USED], sums[SKIPPED] = len(rows), skipped
    W = sums[W_]
    few = len(rows) < 6 or not W > 0.0
    neq = sums.copy()
    for q in list(range(W_)) + [RES, KEYMEAN]:
        neq[q] = 0.0 if few else sums[q] / W
    H, g = unpack(neq)
    return dict(neq=neq, info=[len(rows), FIT_FEW if few else FIT_OK, 0, skipped], sums=sums, terms=terms, H=H, g=g)


def unpack(neq):
    """(H (6, 6), g (6,)) of a neq row."""
    H = np.zeros((6, 6))
    at = 0
    for u in range(6):
        for v in range(u, 6):
            H[u, v] = H[v, u] = neq[H0 + at]
            at += 1
    return H, np.asarray(neq[G0:G0 + 6], np.float64).copy()


# ---- rule 3: the step ---------------------------------------------------------------------------------------------------------
def rodrigues(w):
    th2 = float(w @ w)
    th = math.sqrt(th2)
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-4:
        A, Bc = 1.0 - th2 / 6.0 * (1.0 - th2 / 20.0), 0.5 - th2 / 24.0 * (1.0 - th2 / 30.0)
    else:
        A, Bc = math.sin(th) / th, (1.0 - math.cos(th)) / th2
    return np.eye(3) + A * K + Bc * (K @ K)


def solve(H, g, damping, eps):
    """(H + damping diag(H) + eps I) x = -g by Cholesky; None where a pivot does not exceed eps or something is not finite."""
    A = H + damping * np.diag(np.diag(H)) + eps * np.eye(6)
    L = np.zeros((6, 6))
    for j in range(6):
        p = A[j, j] - (L[j, :j] ** 2).sum()
        if not (p > eps and p < np.inf):
            return None
        L[j, j] = math.sqrt(p)
        for i in range(j + 1, 6):
            L[i, j] = (A[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
    x = np.linalg.solve(L.T, np.linalg.solve(L, -g))
    return x if np.isfinite(x).all() else None


def step(neq, info, R, T, state, pivot=None, damping=1e-2, step_scale=1.0, max_rot=0.2, max_trans=np.inf, eps=1e-12,
         tol_rot=0.0, tol_trans=0.0, patience=0):
    """rrl_plane_step_batch for one pair, float64 and unrounded: -> (R, T, last_step or None, state).  R, T float32 in;
    state = [epochs, calm epochs, done epoch or -1, what this call did]."""
    R, T = np.asarray(R, np.float32).astype(np.float64).reshape(3, 3), np.asarray(T, np.float32).astype(np.float64)
    epochs, calm_was, done_at = state[0] + 1, state[1], state[2]
    if done_at >= 0:
        return R, T, None, [epochs, calm_was, done_at, DONE]
    if info[1] != FIT_OK:
        return R, T, None, [epochs, 0, done_at, FEW]
    H, g = unpack(neq)
    x = solve(H, g, float(np.float32(damping)), eps)
    if x is None:
        return R, T, None, [epochs, 0, done_at, FAILED]
    sc = float(np.float32(step_scale))
    w, v = sc * x[:3], sc * x[3:]
    nw, nv = math.sqrt(w @ w), math.sqrt(v @ v)
    mr, mt = float(np.float32(max_rot)), float(np.float32(max_trans))
    if nw > mr:
        w, nw = w * (mr / nw), mr
    if nv > mt:
        v, nv = v * (mt / nv), mt
    Rot = rodrigues(w)
    c = np.zeros(3) if pivot is None else np.asarray(pivot, np.float32).astype(np.float64)
    Rn, Tn = R @ Rot.T, (T - c) @ Rot.T + c + v
    for i in range(3):
        for p in range(i):
            Rn[i] -= (Rn[i] @ Rn[p]) * Rn[p]
        Rn[i] /= math.sqrt(Rn[i] @ Rn[i])
    if not (np.isfinite(Rn).all() and np.isfinite(Tn).all()):
        return R, T, None, [epochs, 0, done_at, FAILED]
    calm, done = 0, done_at
    if patience > 0:
        calm = calm_was + 1 if (np.float32(nw) < np.float32(tol_rot) and np.float32(nv) < np.float32(tol_trans)) else 0
        if calm >= patience:
            done = epochs
    return Rn, Tn, (nw, nv), [epochs, calm, done, STEPPED]


# ---- the loops, restated in float64 on the host ---------------------------------------------------------------------------------
def rotation_error_deg(R, R_true):
    """The angle between two rotations (row convention), degrees."""
    E = np.asarray(R, np.float64).T @ np.asarray(R_true, np.float64)
    v = np.array([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]])
    return math.degrees(math.atan2(0.5 * math.sqrt(v @ v), 0.5 * (np.trace(E) - 1.0)))


def pair_with_rotation(seed, n, m, deg=20.0):
    """synth.make_pair(seed, n, m, rot_deg=deg) and the row-convention rotation that generated its target (src R ~ tar)."""
    from rrl_hip import synth
    pr = synth.make_pair(seed, n, m, rot_deg=deg)
    rs = np.random.default_rng(seed)  # make_pair's own stream: two surfaces, then the axis
    synth._surface(rs, n), synth._surface(rs, m)
    return pr, synth._rotation(rs.standard_normal(3), deg).T


def box_centre(tar):
    return (0.5 * (tar.min(0) + tar.max(0))).astype(np.float32)


def plane_loop(src, tar, normals, n_epoch, damping=1e-2, max_rot=0.2, max_trans_frac=0.1, eps=1e-12, round_pose=False):
    """Point-to-plane ICP of one pair on the host: float64 nearest neighbours (scipy cKDTree), rules 2 and 3.  round_pose: the
    pose is rounded to float32 after every step, as the device holds it.  -> (R, T)."""
    from scipy.spatial import cKDTree
    src, tar = np.asarray(src, np.float32), np.asarray(tar, np.float32)
    tree = cKDTree(tar.astype(np.float64))
    diag = float(np.linalg.norm(tar.max(0).astype(np.float64) - tar.min(0).astype(np.float64)))
    pivot = box_centre(tar)
    R, T, state = np.eye(3), np.zeros(3), [0, 0, -1, 0]
    for _ in range(n_epoch):
        moved = src.astype(np.float64) @ R + T
        if round_pose:
            moved = moved.astype(np.float32).astype(np.float64)
        _, j = tree.query(moved)
        ne = _normal_eq64(moved, tar[j].astype(np.float64), np.asarray(normals, np.float64)[j], pivot)
        R, T, _, state = _step64(ne, R, T, state, pivot, damping, max_rot, max_trans_frac * diag, eps)
        if round_pose:
            R, T = R.astype(np.float32).astype(np.float64), T.astype(np.float32).astype(np.float64)
    return R, T


def _normal_eq64(y, bt, nn, pivot):
    """rule 2 on float64 moved points (the loop's own; normal_eq rounds its inputs to float32 like the kernel's)."""
    keep = np.isfinite(nn).all(1) & nn.any(1)
    y, bt, nn = y[keep], bt[keep], nn[keep]
    p, e = y - pivot.astype(np.float64), y - bt
    r = (e * nn).sum(1)
    J = np.concatenate([np.cross(p, nn), nn], axis=1)
    W = float(len(r))
    return dict(H=J.T @ J / max(W, 1.0), g=J.T @ r / max(W, 1.0), info=[len(r), FIT_FEW if len(r) < 6 else FIT_OK, 0, 0])


def _step64(ne, R, T, state, pivot, damping, max_rot, max_trans, eps):
    neq = np.zeros(DOUBLES)
    at = 0
    for u in range(6):
        for v in range(u, 6):
            neq[H0 + at] = ne["H"][u, v]
            at += 1
    neq[G0:G0 + 6] = ne["g"]
    # (step() rounds R, T and the controls to float32 on entry: the float64 loop calls its body on float64 poses)
    H, g = unpack(neq)
    x = solve(H, g, float(np.float32(damping)), eps) if ne["info"][1] == FIT_OK else None
    if x is None:
        return R, T, None, state
    w, v = x[:3].copy(), x[3:].copy()
    nw, nv = math.sqrt(w @ w), math.sqrt(v @ v)
    if nw > max_rot:
        w *= max_rot / nw
    if nv > max_trans:
        v *= max_trans / nv
    Rot = rodrigues(w)
    c = pivot.astype(np.float64)
    Rn, Tn = R @ Rot.T, (T - c) @ Rot.T + c + v
    for i in range(3):
        for p in range(i):
            Rn[i] -= (Rn[i] @ Rn[p]) * Rn[p]
        Rn[i] /= math.sqrt(Rn[i] @ Rn[i])
    return Rn, Tn, (nw, nv), state


def point_loop(src, tar, n_epoch):
    """Point-to-point ICP of one pair on the host, float64: nearest neighbours, the closed-form fit of the source as given."""
    from scipy.spatial import cKDTree
    a, b = np.asarray(src, np.float64), np.asarray(tar, np.float64)
    tree = cKDTree(b)
    R, T = np.eye(3), np.zeros(3)
    for _ in range(n_epoch):
        _, j = tree.query(a @ R + T)
        q = b[j]
        abar, bbar = a.mean(0), q.mean(0)
        U, _, Vt = np.linalg.svd((a - abar).T @ (q - bbar))
        D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
        R = U @ D @ Vt
        T = bbar - abar @ R
    return R, T
