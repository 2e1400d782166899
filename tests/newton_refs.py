"""The float64 twin of the second-order pose path (include/rrl.h rrl_pose_normal_eq / rrl_se3_newton_step_batch; DESIGN.md
section 15), for tests/test_newton_refs_host.py (CPU) and tests/test_gpu_newton.py.

From the fields a registration forward leaves in its workspace, for ONE sample as numpy arrays --
    kj (L,) uint8 = k | j << 4 (0: not selected), w1 (L, 4, 3), Q1 / Q2 (L, 4, 4) = (xyz, 0), D (L, 16): the k x j block with
    row stride j, med (), bcnt (16,) at (k - 1) 4 + (j - 1), info (4,) with info[0] = C, the populated buckets
-- it recomputes the selected pairs (line, source hit h, target hit o), their weights
    a = exp(-|k - j| / 2) / C * ([o = argmin_o(h)] / (S k) + [h = argmin_h(o)] / (S j)) * exp(-D / (2 med)) / (2 med)
(the backward's dL/dD at upstream gradient 1; first-occurrence minima of the Welsch terms), and with Q = Q1[h], e = Q1[h] -
Q2[o], s = (w_0 + w_1 + w_2) / 3 the sixteen sums
    S_QQ = sum 2a Q Q^T (xx, xy, xz, yy, yz, zz), S_sQ = sum 2a s Q, S_ss = sum 2a s^2, g_w = sum 2a Q x e, g_v = sum 2a s e
together with the sums of the ABSOLUTE values of their terms (for Q x e the two products of a component are two terms).
It also holds what the pose step does with them: H and g, the damped solve, the clamps, the composition and the stopping
rule, all in float64.  Written from the formulas of the issue and DESIGN.md section 15; nothing is taken from the kernels.

The minima are taken on the Welsch terms evaluated in float32, as every implementation of the loss does (far from the
median 1 - exp(-x) saturates at 1 and the FIRST of the saturated entries wins); the weights are float64."""
import numpy as np

NSUMS = 16
STEPPED, GATED, FAILED, DONE = 0, 1, 2, 3   # include/rrl.h RRL_NEWTON_*


def selected_pairs(f, min_dtype=np.float32):
    """dict of flat arrays over the pairs that carry weight: a (float64), Q (n, 3), e (n, 3), s, line, h, o.  min_dtype: the
    precision in which the Welsch terms are compared (float64: the minima of tests/loss_refs.py's float64 twin)."""
    kj = np.asarray(f["kj"])
    C = int(np.asarray(f["info"]).reshape(-1)[0])
    out = dict(a=[], Q=[], e=[], s=[], line=[], h=[], o=[])
    if C > 0:
        med = float(f["med"])
        mt = np.dtype(min_dtype).type
        bcnt = np.asarray(f["bcnt"]).reshape(-1)
        D_all, Q1, Q2 = np.asarray(f["D"], np.float64), np.asarray(f["Q1"], np.float64), np.asarray(f["Q2"], np.float64)
        w1 = np.asarray(f["w1"], np.float64)
        for l in np.nonzero(kj)[0]:
            k, j = int(kj[l]) & 15, int(kj[l]) >> 4
            S = int(bcnt[(k - 1) * 4 + (j - 1)])
            D = D_all[l, :k * j].reshape(k, j)
            with np.errstate(over="ignore", under="ignore"):
                W32 = mt(1) - np.exp(-(D.astype(mt) / mt(med)) / mt(2))
            er = np.exp(-(D / med) / 2.0)
            amin_o, amin_h = W32.argmin(1), W32.argmin(0)   # first occurrence
            wkj = np.exp(-0.5 * abs(k - j))
            for h in range(k):
                for o in range(j):
                    sw = (1.0 / (S * k) if amin_o[h] == o else 0.0) + (1.0 / (S * j) if amin_h[o] == h else 0.0)
                    if sw == 0.0:
                        continue
                    Q = Q1[l, h, :3]
                    out["a"].append(wkj / C * sw * er[h, o] / (2.0 * med))
                    out["Q"].append(Q)
                    out["e"].append(Q - Q2[l, o, :3])
                    out["s"].append(w1[l, h].sum() / 3.0)
                    out["line"].append(l); out["h"].append(h); out["o"].append(o)
    n = len(out["a"])
    return dict(a=np.array(out["a"], np.float64), Q=np.array(out["Q"], np.float64).reshape(n, 3),
                e=np.array(out["e"], np.float64).reshape(n, 3), s=np.array(out["s"], np.float64),
                line=np.array(out["line"], np.int64), h=np.array(out["h"], np.int64), o=np.array(out["o"], np.int64))


def normal_sums(f, min_dtype=np.float32):
    """(sums (16,), abs_sums (16,), number of pairs) of one sample: the sums and the sums of |terms|."""
    p = selected_pairs(f, min_dtype)
    a2, Q, e, s = 2.0 * p["a"], p["Q"], p["e"], p["s"]
    x, y, z = Q[:, 0], Q[:, 1], Q[:, 2]
    ex, ey, ez = e[:, 0], e[:, 1], e[:, 2]
    plus = [a2 * x * x, a2 * x * y, a2 * x * z, a2 * y * y, a2 * y * z, a2 * z * z, a2 * s * x, a2 * s * y, a2 * s * z, a2 * s * s,
            a2 * y * ez, a2 * z * ex, a2 * x * ey, a2 * s * ex, a2 * s * ey, a2 * s * ez]
    minus = {10: a2 * z * ey, 11: a2 * x * ez, 12: a2 * y * ex}
    sums, abs_sums = np.zeros(NSUMS), np.zeros(NSUMS)
    for q in range(NSUMS):
        sums[q] = plus[q].sum() - (minus[q].sum() if q in minus else 0.0)
        abs_sums[q] = np.abs(plus[q]).sum() + (np.abs(minus[q]).sum() if q in minus else 0.0)
    return sums, abs_sums, len(a2)


def skew(q):
    return np.array([[0.0, -q[2], q[1]], [q[2], 0.0, -q[0]], [-q[1], q[0], 0.0]])


def assemble(sums):
    """H (6, 6), g (6,) from the sixteen sums: H_ww = tr(S_QQ) I - S_QQ, H_wv = [S_sQ]x, H_vv = S_ss I."""
    S = np.asarray(sums, np.float64)
    SQQ = np.array([[S[0], S[1], S[2]], [S[1], S[3], S[4]], [S[2], S[4], S[5]]])
    H = np.zeros((6, 6))
    H[:3, :3] = np.trace(SQQ) * np.eye(3) - SQQ
    H[:3, 3:] = skew(S[6:9])
    H[3:, :3] = H[:3, 3:].T
    H[3:, 3:] = S[9] * np.eye(3)
    return H, S[10:16].copy()


def damped(H, damping, eps):
    return H + damping * np.diag(np.diag(H)) + eps * np.eye(6)


def solve(H, g, damping, eps):
    """x with (H + damping diag(H) + eps I) x = -g by Cholesky, or None: a pivot that does not exceed eps or is not
    finite, or a non-finite solution."""
    A = damped(np.asarray(H, np.float64), float(damping), float(eps))
    Lm = np.zeros((6, 6))
    for j in range(6):
        p = A[j, j] - (Lm[j, :j] ** 2).sum()
        if not (p > eps) or not np.isfinite(p):
            return None
        Lm[j, j] = np.sqrt(p)
        for i in range(j + 1, 6):
            Lm[i, j] = (A[i, j] - (Lm[i, :j] * Lm[j, :j]).sum()) / Lm[j, j]
    y = np.zeros(6)
    for i in range(6):
        y[i] = (-g[i] - (Lm[i, :i] * y[:i]).sum()) / Lm[i, i]
    x = np.zeros(6)
    for i in range(5, -1, -1):
        x[i] = (y[i] - (Lm[i + 1:, i] * x[i + 1:]).sum()) / Lm[i, i]
    return x if np.isfinite(x).all() else None


def clamp(x, step, max_rot, max_trans):
    """(omega, v, |omega|, |v|) as applied: step x, each half scaled down to its maximum norm."""
    w, v = step * np.asarray(x[:3], np.float64), step * np.asarray(x[3:], np.float64)
    nw, nv = np.linalg.norm(w), np.linalg.norm(v)
    if nw > max_rot:
        w, nw = w * (max_rot / nw), float(max_rot)
    if nv > max_trans:
        v, nv = v * (max_trans / nv), float(max_trans)
    return w, v, nw, nv


def rodrigues(w):
    """exp([w]x), the column-convention rotation."""
    th = np.linalg.norm(w)
    K = skew(w)
    if th < 1e-8:
        return np.eye(3) + K + 0.5 * K @ K
    return np.eye(3) + np.sin(th) / th * K + (1.0 - np.cos(th)) / th ** 2 * K @ K


def compose(R, T, w, v):
    """The pose after the twist (w, v): R Rot^T re-orthonormalised by one Gram-Schmidt pass over its rows, T Rot^T + v."""
    Rot = rodrigues(w)
    Rn = np.asarray(R, np.float64).reshape(3, 3) @ Rot.T
    Tn = np.asarray(T, np.float64).reshape(3) @ Rot.T + v
    for i in range(3):
        for p in range(i):
            Rn[i] -= (Rn[i] @ Rn[p]) * Rn[p]
        Rn[i] /= np.linalg.norm(Rn[i])
    return Rn, Tn


def step(neq, gate, R, T, state, damping, step_scale, max_rot, max_trans, tol_rot, tol_trans, patience, eps):
    """One sample of rrl_se3_newton_step_batch: returns (R, T, state (4,), delta or None, last_step or None).  state =
    (epochs, calm, done epoch or -1, status)."""
    epochs, calm0, done_at = int(state[0]) + 1, int(state[1]), int(state[2])
    R, T = np.asarray(R, np.float64).reshape(3, 3), np.asarray(T, np.float64).reshape(3)
    if done_at >= 0:
        return R, T, np.array([epochs, calm0, done_at, DONE]), None, None
    if gate <= 0:
        return R, T, np.array([epochs, 0, -1, GATED]), None, None
    H, g = assemble(neq)
    x = solve(H, g, damping, eps) if np.isfinite(np.asarray(neq, np.float64)).all() else None
    if x is None:
        return R, T, np.array([epochs, 0, -1, FAILED]), None, None
    w, v, nw, nv = clamp(x, step_scale, max_rot, max_trans)
    Rn, Tn = compose(R, T, w, v)
    calm = calm0 + 1 if (patience > 0 and np.float32(nw) < np.float32(tol_rot) and np.float32(nv) < np.float32(tol_trans)) else 0
    done = epochs if (patience > 0 and calm >= patience) else -1
    return Rn, Tn, np.array([epochs, calm, done, STEPPED]), x, np.array([nw, nv])


def diagonal_neq(nw, nv):
    """Sixteen sums whose undamped system is the identity (S_QQ = I / 2, S_sQ = 0, S_ss = 1) and whose gradient is
    -(nw, 0, 0, nv, 0, 0): with damping 0 and step 1 the solved twist is (nw, 0, 0), (nv, 0, 0) up to the eps term, so the two
    step lengths are the two numbers given."""
    S = np.zeros(NSUMS, np.float32)
    S[0] = S[3] = S[5] = 0.5
    S[9], S[10], S[13] = 1.0, -nw, -nv
    return S


def chain_rule_gradient(gR, gt, R, T):
    """(g_w, g_v) of the twist (omega, v) at 0 from dL/dR (3, 3) and dL/dT (3,) of y = x R + T: dy = omega x y + v, so
    g_v = dL/dT and g_w = sum y x g_y = vee(A - A^T) + T x dL/dT with A = R^T dL/dR."""
    gR, gt = np.asarray(gR, np.float64).reshape(3, 3), np.asarray(gt, np.float64).reshape(3)
    R, T = np.asarray(R, np.float64).reshape(3, 3), np.asarray(T, np.float64).reshape(3)
    A = R.T @ gR
    return np.array([A[1, 2] - A[2, 1], A[2, 0] - A[0, 2], A[0, 1] - A[1, 0]]) + np.cross(T, gt), gt


def chain_rule_abs(aR, at, R, T):
    """The sums of |terms| behind chain_rule_gradient from those behind dL/dR, dL/dT (aR (3, 3), at (3,))."""
    aR, at = np.asarray(aR, np.float64).reshape(3, 3), np.asarray(at, np.float64).reshape(3)
    A = np.abs(np.asarray(R, np.float64).reshape(3, 3)).T @ aR
    Ta = np.abs(np.asarray(T, np.float64).reshape(3))
    cr = np.array([Ta[1] * at[2] + Ta[2] * at[1], Ta[2] * at[0] + Ta[0] * at[2], Ta[0] * at[1] + Ta[1] * at[0]])
    return np.array([A[1, 2] + A[2, 1], A[2, 0] + A[0, 2], A[0, 1] + A[1, 0]]) + cr, at


def fields_from_ref(ref, L, dtype=np.float64):
    """The workspace fields of one sample from a tests/loss_refs.py post_scan_ref result (its blocks, median and bucket
    counts), laid out as the library lays them out."""
    kj = np.zeros(L, np.uint8)
    w1, Q1, Q2, D = np.zeros((L, 4, 3), dtype), np.zeros((L, 4, 4), dtype), np.zeros((L, 4, 4), dtype), np.zeros((L, 16), dtype)
    bcnt = np.zeros(16, np.int64)
    for (k, j), v in ref["blocks"].items():
        if k > 4 or j > 4:
            continue
        ln = v["lines"]
        kj[ln] = k | (j << 4)
        w1[ln, :k] = v["w1"]
        Q1[ln, :k, :3] = v["q1"]
        Q2[ln, :j, :3] = v["q2"]
        D[ln, :k * j] = v["D"].reshape(len(ln), k * j)
        bcnt[(k - 1) * 4 + (j - 1)] = len(ln)
    return dict(kj=kj, w1=w1, Q1=Q1, Q2=Q2, D=D, med=float(ref["med"]), bcnt=bcnt,
                info=np.array([ref["n_buckets"], ref["n_selected"], ref["n_values"], 0]))
