"""Host twin of rrl_ball_group (include/rrl.h "ball-query grouping") in numpy: the rule restated, not
the kernel's loop.  Membership is float64 in the stated order -- (dx dx + dy dy) + dz dz from the float64 differences of the
float32 coordinates, compared with float64(float32(radius ** 2)) --, dxyz is the float32 subtraction, the angles and the norm
are float64 (the kernel rounds them once to float32)."""
import numpy as np

FEATURES = ("xyz", "dxyz", "ppf")
SIZES = {"xyz": 3, "dxyz": 3, "ppf": 4}
ANGLE_TOL = 2.0 ** -20      # rad: an angle of the kernel (or of the float32 reference) against this twin
NORM_RTOL = 3 * 2.0 ** -24  # |d| against itself
BORDER = 2.0 ** -20         # a pair is borderline when |d2 - r2| <= BORDER (|x_i|^2 + |x_j|^2)


def r2_of(radius):
    """float32(radius ** 2): the Python double squared, then rounded -- what torch compares its float32 matrix against."""
    return np.float32(float(radius) ** 2)


def dist2(xq, x):
    """(Q, 3), (n, 3) float32 -> (Q, n) float64 squared distances in the rule's order."""
    d = xq.astype(np.float64)[:, None, :] - x.astype(np.float64)[None, :, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def angle(a, b):
    """atan2(|a x b|, a . b) over the last axis, float64 (rpm/models/pointnet_util.py:173-194)."""
    a, b = np.broadcast_arrays(a.astype(np.float64), b.astype(np.float64))
    cx = a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1]
    cy = a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2]
    cz = a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]
    cn = np.sqrt((cx * cx + cy * cy) + cz * cz)
    dot = ((0.0 + a[..., 0] * b[..., 0]) + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]  # summed from +0 like torch.sum: never -0
    return np.arctan2(cn, dot)


def ball_group(points, normals, radius, nsample, features=(), query_idx=None, counts=None, qcounts=None, exclude_self=True):
    """numpy (B, n, 3) float32 -> dict(idx (B, S, nsample) int32, found (B, S) int32, feat (B, S, nsample, C) float64 or None,
    dxyz (B, S, nsample, 3) float32 -- bit-exact --, border (B, S) bool: the row has a borderline pair)."""
    points = np.asarray(points, np.float32)
    B, n, _ = points.shape
    S = n if query_idx is None else np.asarray(query_idx).shape[1]
    r2 = np.float64(r2_of(radius))
    feats = [f for f in FEATURES if f in features]
    C = sum(SIZES[f] for f in feats)
    idx = np.zeros((B, S, nsample), np.int32)
    found = np.zeros((B, S), np.int32)
    feat = np.zeros((B, S, nsample, C), np.float64) if C else None
    dxyz = np.zeros((B, S, nsample, 3), np.float32)
    border = np.zeros((B, S), bool)
    for b in range(B):
        nb = n if counts is None else min(max(int(counts[b]), 0), n)
        Sb = (S if qcounts is None else min(max(int(qcounts[b]), 0), S)) if nb > 0 else 0
        if query_idx is None:
            Sb = min(Sb, nb)
        if Sb == 0:
            continue
        x = points[b, :nb]
        qi = np.arange(Sb) if query_idx is None else np.clip(np.asarray(query_idx)[b, :Sb].astype(np.int64), 0, nb - 1)
        with np.errstate(invalid="ignore", over="ignore"):
            d2 = dist2(x[qi], x)
            member = d2 <= r2  # (a NaN distance compares false)
            sq = (x.astype(np.float64) ** 2).sum(-1)
            border[b, :Sb] = (np.abs(d2 - r2) <= BORDER * (sq[qi][:, None] + sq[None, :])).any(1)
        if exclude_self:
            member[np.arange(Sb), qi] = False
        rank = np.cumsum(member, axis=1) - 1
        keep = member & (rank < nsample)
        cnt = np.minimum(member.sum(1), nsample)
        first = np.where(cnt > 0, np.argmax(member, axis=1), qi)
        pad = qi if exclude_self else first
        rows = np.repeat(pad[:, None], nsample, axis=1)
        r, c = np.nonzero(keep)
        rows[r, rank[r, c]] = c
        idx[b, :Sb], found[b, :Sb] = rows, cnt
        with np.errstate(invalid="ignore"):
            d = x[rows] - x[qi][:, None, :]  # float32
        dxyz[b, :Sb] = d
        if C:
            parts = []
            if "xyz" in feats:
                parts.append(np.repeat(x[qi][:, None, :].astype(np.float64), nsample, axis=1))
            if "dxyz" in feats:
                parts.append(d.astype(np.float64))
            if "ppf" in feats:
                nr = np.asarray(normals, np.float32)[b, :nb]
                ni, nj = nr[qi][:, None, :], nr[rows]
                d64 = d.astype(np.float64)
                with np.errstate(invalid="ignore"):
                    norm = np.sqrt((d64[..., 0] * d64[..., 0] + d64[..., 1] * d64[..., 1]) + d64[..., 2] * d64[..., 2])
                    parts.append(np.stack([angle(ni, d), angle(nj, d), angle(ni, nj), norm], -1))
            feat[b, :Sb] = np.concatenate(parts, -1)
    return dict(idx=idx, found=found, feat=feat, dxyz=dxyz, border=border)


def ppf_errors(got, want, ppf_at):
    """(worst angle error in rad, worst relative |d| error) of got against the float64 `want`, ppf starting at channel ppf_at."""
    g, w = np.asarray(got, np.float64)[..., ppf_at:ppf_at + 4], np.asarray(want, np.float64)[..., ppf_at:ppf_at + 4]
    ang = np.abs(g[..., :3] - w[..., :3]).max() if g.size else 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(w[..., 3] > 0, np.abs(g[..., 3] - w[..., 3]) / w[..., 3], np.abs(g[..., 3]))
    return float(ang), float(rel.max() if rel.size else 0.0)


def make_cloud(seed, B, N, kind):
    """The golden file's inputs: torch.Generator().manual_seed(seed), x = rand(B, N, 3) * 2 - 1 (unit length for "sphere"),
    then normals drawn the same way and normalised."""
    import torch
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, N, 3, generator=g) * 2 - 1
    if kind == "sphere":
        x = x / x.norm(dim=-1, keepdim=True)
    nr = torch.rand(B, N, 3, generator=g) * 2 - 1
    nr = nr / nr.norm(dim=-1, keepdim=True)
    return x, nr
