"""Exact and float64 twins of the robust ICP loop (include/rrl.h rrl_key_median, rrl_welsch_weights, rrl_robust_step_batch,
rrl_robust_icp_epoch), and the acceptance pairs.  numpy only; nothing here touches a GPU or the library.

A VALID row is one rrl_kabsch_fwd would not skip: below count_a, its key not all ones, its key's index < m and < count_b.
"""
import numpy as np

import kabsch_refs as KR

ALL_ONES = KR.ALL_ONES
TOL_ROT, TOL_TRANS, PATIENCE = 1e-4, 1e-5, 3           # IcpRegistration's stopping rule
NU_START, ANNEAL, LEVEL_CAP = 3.0, 0.5, 10             # RobustIcpRegistration's defaults
SHIFT = np.array([0.05, -0.03, 0.02])


def pack_keys(d2, idx):
    """(float32 distance words << 32 | index) as uint64."""
    words = np.ascontiguousarray(d2, np.float32).view(np.uint32).astype(np.uint64)
    return (words << np.uint64(32)) | np.asarray(idx, np.uint64)


def key_words(keys):
    return (np.asarray(keys, np.uint64) >> np.uint64(32)).astype(np.uint32)


def valid_rows(keys, m, count_a=None, count_b=None):
    """Boolean mask over the rows of ONE sample's keys (n,) uint64."""
    keys = np.asarray(keys, np.uint64)
    n = keys.shape[0]
    ca = n if count_a is None else min(max(int(count_a), 0), n)
    cb = m if count_b is None else min(max(int(count_b), 0), m)
    idx = keys & np.uint64(0xFFFFFFFF)
    return (np.arange(n) < ca) & (keys != np.uint64(ALL_ONES)) & (idx < np.uint64(m)) & (idx < np.uint64(cb))


def key_median_ref(keys, m, count_a=None, count_b=None):
    """(med_sq float32, k): the word of rank (k - 1) // 2 among the valid rows' distance words sorted as uint32; (0, 0) without one."""
    words = np.sort(key_words(keys)[valid_rows(keys, m, count_a, count_b)])
    k = int(words.shape[0])
    if k == 0:
        return np.float32(0.0), 0
    return words[(k - 1) // 2: (k - 1) // 2 + 1].view(np.float32)[0], k


def nu_start_ref(med_sq, nu_scale, nu_end):
    """float32: max(float32(nu_scale sqrt(double(med_sq))), nu_end), nu_end when the left side is NaN."""
    with np.errstate(over="ignore", invalid="ignore"):
        start = np.float32(np.float64(nu_scale) * np.sqrt(np.float64(np.float32(med_sq))))
    end = np.float32(nu_end)
    return start if start > end else end


def welsch_weights_ref(keys, nu, m, count_a=None, count_b=None):
    """(n,) float32 weights of ONE sample; double arithmetic, rounded once."""
    keys = np.asarray(keys, np.uint64)
    w = np.zeros(keys.shape[0], np.float32)
    nu = np.float32(nu)
    if not (nu > 0 and np.isfinite(nu)):
        return w
    ok = valid_rows(keys, m, count_a, count_b)
    d2 = key_words(keys).view(np.float32).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        e = np.exp(-d2 / (2.0 * np.float64(nu) * np.float64(nu)))
    e = np.where(np.isnan(e), 0.0, e)
    w[ok] = e[ok].astype(np.float32)
    return w


def robust_step_rule_ref(Rk, Tk, status, abar, R, T, state, level, nu, nu_end, tol_rot, tol_trans, patience, anneal, level_cap):
    """rrl_robust_step_batch for one pair, the integer and float32 state machine exactly: KR.icp_step up to its calm count, then
    the annealing rule where that one declares a pair done:
    -> (R, T, last_step (float32, float32) or None, state [4], level [2], nu float32)."""
    nu, nu_end = np.float32(nu), np.float32(nu_end)
    R, T, last, (epochs, calm, done, out) = KR.icp_step(Rk, Tk, status, abar, R, T, state, tol_rot, tol_trans, patience)
    if state[2] >= 0:
        return R, T, None, [epochs, calm, done, out], list(level), nu
    if last is not None:
        last = (np.float32(last[0]), np.float32(last[1]))
    at_nu, levels, done = level[0] + 1, level[1], -1
    if (patience > 0 and calm >= patience) or (level_cap > 0 and at_nu >= level_cap):
        if nu > nu_end:
            nxt = np.float32(nu * np.float32(anneal))
            nu = nxt if nxt > nu_end else nu_end
            calm, at_nu, levels = 0, 0, levels + 1
        else:
            done = epochs
    return R, T, last, [epochs, calm, done, out], [at_nu, levels], nu


def nearest_keys(moved, tar):
    """Brute-force nearest neighbours in float64, the smallest index among equals -> keys (n,) uint64 whose distance words are
    the squared distances rounded to float32."""
    d2 = ((np.asarray(moved, np.float64)[:, None, :] - np.asarray(tar, np.float64)[None, :, :]) ** 2).sum(-1)
    idx = d2.argmin(1)
    return pack_keys(d2[np.arange(d2.shape[0]), idx].astype(np.float32), idx)


def nu_end_ref(tar):
    """The lower median distance from a target point to its nearest OTHER target point, over 3 sqrt(3)."""
    t = np.asarray(tar, np.float64)
    d2 = ((t[:, None, :] - t[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d2, np.inf)
    near = np.sort(np.sqrt(d2.min(1)))
    return float(near[(len(near) - 1) // 2] / (3.0 * np.sqrt(3.0)))


def robust_epoch_from_keys(src, tar, keys, R, T, state, level, nu, nu_end, init, count1=None, count2=None, nu_scale=NU_START,
                           anneal=ANNEAL, level_cap=LEVEL_CAP, tol_rot=0.0, tol_trans=0.0, patience=0):
    """One epoch of one pair from GIVEN keys -> (fit dict, w, R, T, last_step, state, level, nu)."""
    m = tar.shape[0]
    if init:
        med, _ = key_median_ref(keys, m, count1, count2)
        nu = nu_start_ref(med, nu_scale, nu_end)
    w = welsch_weights_ref(keys, nu, m, count1, count2)
    f = KR.fit(src, tar, w, keys, count1, count2)
    Rn, Tn, last, st, lv, nu = robust_step_rule_ref(f["R"].astype(np.float32), f["T"].astype(np.float32), f["info"][1], f["abar"], R, T,
                                                    state, level, nu, nu_end, tol_rot, tol_trans, patience, anneal, level_cap)
    return f, w, Rn, Tn, last, st, lv, nu


def robust_icp_ref(src, tar, n_epoch=60, robust=True, nu_end=None, nu_scale=NU_START, anneal=ANNEAL, level_cap=LEVEL_CAP,
                   tol_rot=TOL_ROT, tol_trans=TOL_TRANS, patience=PATIENCE):
    """The whole loop for one pair, float64 (poses held as float32, as the device holds them), from the identity.
    robust=False: the plain twin -- all weights 1, the same tolerances, rrl_icp_step_batch's rule.
    -> dict(R, T, state, level, nu, epochs run)."""
    src, tar = np.asarray(src, np.float32), np.asarray(tar, np.float32)
    diag = float(np.linalg.norm(tar.max(0).astype(np.float64) - tar.min(0).astype(np.float64)))
    tol_t = np.float32(np.float32(tol_trans) * np.float32(diag))
    nu_end = np.float32(nu_end_ref(tar) if nu_end is None else nu_end)
    R, T = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    state, level, nu, e = [0, 0, -1, 0], [0, 0], np.float32(0.0), 0
    for e in range(1, n_epoch + 1):
        moved = src.astype(np.float64) @ R.astype(np.float64) + T.astype(np.float64)
        keys = nearest_keys(moved, tar)
        if robust:
            _, _, R, T, _, state, level, nu = robust_epoch_from_keys(src, tar, keys, R, T, state, level, nu, nu_end, e == 1, None, None,
                                                                     nu_scale, anneal, level_cap, tol_rot, tol_t, patience)
        else:
            _, R, T, _, state = KR.icp_epoch_from_keys(src, tar, keys, R, T, state, tol_rot=tol_rot, tol_trans=tol_t, patience=patience)
        if state[2] >= 0:
            break
    return dict(R=np.asarray(R), T=np.asarray(T), state=state, level=level, nu=nu, nu_end=nu_end, epochs=e)


def surface(rng, n):
    """rrl_hip.synth's bumpy ellipsoid."""
    u = rng.standard_normal((n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    rad = 1.0 + 0.25 * np.sin(3.0 * u[:, 0]) * np.cos(2.0 * u[:, 1])
    return (u * rad[:, None]) * np.array([1.0, 0.7, 0.5])


def rotation(axis, deg):
    """rrl_hip.synth's Rodrigues matrix (moves column vectors)."""
    axis = axis / np.linalg.norm(axis)
    a = np.deg2rad(deg)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


def outlier_pair(seed, n, rot_deg, frac):
    """(src (n, 3) float32, tar (n, 3) float32, R (3, 3) float64 with tar = clean src R + shift, in the row convention).
    One stream draws, in this order: the surface, the rotation axis, the permutation, the outlier rows, the outlier
    coordinates.  The target is the clean surface rotated, shifted and permuted; then a fraction `frac` of the source rows is
    replaced by uniform points in 1.5 x the source's box (about its centre)."""
    rng = np.random.default_rng(seed)
    src = surface(rng, n)
    Rg = rotation(rng.standard_normal(3), rot_deg).T
    tar = (src @ Rg + SHIFT)[rng.permutation(n)]
    rows = rng.choice(n, int(round(frac * n)), replace=False)
    lo, hi = src.min(0), src.max(0)
    centre, half = 0.5 * (lo + hi), 0.75 * (hi - lo)
    src[rows] = rng.uniform(centre - half, centre + half, (len(rows), 3))
    return src.astype(np.float32), tar.astype(np.float32), Rg


def rot_err_deg(R, Rg):
    return float(np.degrees(KR.rotation_angle(np.asarray(R, np.float64), np.asarray(Rg, np.float64))))
