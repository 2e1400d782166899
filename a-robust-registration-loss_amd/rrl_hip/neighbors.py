"""Pseudo-triangle builder on the GPU (reference: Sample_neighs, code/loss.py:473-485 with
utils.farthest_point_sample, code/utils.py:275-296, and sklearn's KDTree).  SURVEY.md §8f row 1."""
import numpy as np
import torch

from . import _lib
from . import ops as _ops
from .ops import _home, _p, _run


def _check_index(idx, n, name, shape):
    """The kernels follow these indices into the cloud unchecked: refuse one outside [0, n) on the host, before any launch
    (preprocessing: reading a GPU-resident index tensor back synchronises, once per cloud)."""
    if not isinstance(idx, torch.Tensor) or idx.dtype.is_floating_point or idx.dtype == torch.bool:
        raise ValueError(f"{name} must be an integer tensor")
    if tuple(idx.shape) != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)}, got {tuple(idx.shape)}")
    if idx.numel() and bool(((idx < 0) | (idx >= n)).any()):
        raise ValueError(f"{name} holds an index outside [0, {n})")


def fps(points, num_sample, start=None):
    """points (B, n, 3) tensor -> (B, S) int32 indices in farthest-point order.  `start` (B,)
    defaults to torch.randint(0, n, (B,)) from the CPU generator, like the reference; a given start
    outside [0, n) is a ValueError."""
    B, n, _ = points.shape
    if start is None:
        start = torch.randint(0, n, (B,), dtype=torch.long)
    else:
        _check_index(start, n, "start", (B,))
    dev = _home(points)
    pts = points.detach().to(device=dev, dtype=torch.float32).contiguous()
    S = min(int(num_sample), n)
    st = start.to(device=dev, dtype=torch.int32).contiguous()
    out = torch.empty(B, S, dtype=torch.int32, device=dev)
    scratch = torch.empty(B, n, dtype=torch.float32, device=dev)
    _run(dev, "rrl_fps", _p(pts), _p(st), _p(out), _p(scratch), B, n, S)
    return out


def knn3(points, query_idx):
    """points (B, n, 3), query_idx (B, S) -> (B, S, 3) int32: the 3 nearest of the cloud's n points to each query point,
    the query itself and its duplicates included, ascending distance, the lowest index among equals (so a query comes first
    unless a duplicate of it has a lower index).  ValueError for n < 3 or a query index outside [0, n)."""
    B, n, _ = points.shape
    if n < 3:
        raise ValueError(f"knn3 needs at least 3 points per cloud, got {n}")
    if query_idx.dim() != 2:
        raise ValueError(f"query_idx must have shape (B, S), got {tuple(query_idx.shape)}")
    _check_index(query_idx, n, "query_idx", (B, query_idx.shape[1]))
    dev = _home(points, query_idx)
    pts = points.detach().to(device=dev, dtype=torch.float32).contiguous()
    qi = query_idx.to(device=dev, dtype=torch.int32).contiguous()
    S = qi.shape[1]
    nn = torch.empty(B, S, 3, dtype=torch.int32, device=dev)
    _run(dev, "rrl_knn3", _p(pts), _p(qi), _p(nn), B, n, S)
    return nn


def sample_neighs(points, num_sample=5000, num_neigh=3):
    """numpy (n, 3) -> numpy (3 S, 3): rows [p, nn1, nn2] of the S farthest-point samples
    (S = min(num_sample, n)), the row layout every caller reshapes to (S, 9)."""
    if num_neigh != 3:
        raise ValueError("the loss uses pseudo-triangles: num_neigh must be 3")
    pts_np = np.asarray(points)
    if pts_np.ndim != 2 or pts_np.shape[0] < 3:
        raise ValueError(f"sample_neighs needs at least 3 points, got an array of shape {pts_np.shape}")
    pts = torch.from_numpy(np.ascontiguousarray(pts_np, dtype=np.float32))[None]
    idx = fps(pts, num_sample)
    nn = knn3(pts, idx)[0].long().cpu().numpy()
    out = pts_np[nn.reshape(-1)]  # gathers from the caller's array: keeps its dtype
    return out.reshape(-1, 3)


# ---- pseudo-triangles on the device: batched, ragged, tree 3-NN (include/rrl.h) -------------------
METHODS = ("auto", "brute", "tree")
# method="auto" takes the tree for the all-points form from this many points per cloud (the capacity n): the smallest
# measured size from which the tree was faster than brute force on BOTH cloud kinds (a volume and a surface), at B = 1 and
# B = 8 -- profiles/pseudo_triangles_timing.json, written by tools/pseudo_triangles_timing.py: 1024 is the smallest size measured,
# and the tree won there and at every larger one (72 .. 109 us against 122 at n = 1024, 0.4 .. 0.8 ms against 37 at 262144).
# None: never.
TREE_MIN_POINTS = 1024


def _use_tree(method, n):
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}, got {method!r}")
    if method == "auto":
        return TREE_MIN_POINTS is not None and TREE_MIN_POINTS <= n <= _ops.sort_capacity()
    return method == "tree"


def _points3(points):
    if not isinstance(points, torch.Tensor) or points.dim() != 3 or points.shape[-1] != 3:
        raise ValueError("points must be a (B, n, 3) tensor")
    return points.shape[0], points.shape[1]


def _host_counts(counts, B, n, name):
    """Host-side counts validated before any device is touched (ops.check_counts_host) as int64; None: none, or device data."""
    host = _ops.check_counts_host(counts, B, n, name)
    return None if host is None else host.to(torch.int64)


def _check_index_counted(idx, hcounts, n, name, shape):
    """_check_index against each sample's own count where the counts are known on the host (an empty sample admits 0)."""
    _check_index(idx, n, name, shape)
    if hcounts is not None and idx.numel():
        lim = hcounts.clamp(min=1).reshape((-1,) + (1,) * (idx.dim() - 1))
        if bool((idx.to(torch.int64) >= lim).any()):
            raise ValueError(f"{name} holds an index outside its sample's count")


def knn3_self(points, counts=None, method="auto"):
    """points (B, n, 3) -> (B, n, 3) int32: the 3 nearest points of EVERY point among its cloud's points, as knn3 orders them
    (ascending float64 distance, the lowest index among equals, the point itself and its duplicates included).
    method="tree" walks the sorted layout (include/rrl.h rrl_knn3_self; n <= ops.sort_capacity()), "brute" is knn3's loop,
    "auto" picks by TREE_MIN_POINTS; the result is the same, bit for bit.  counts: (B,) int32 on the GPU (read by the kernels
    only: clamped to [0, n], never validated on the host), or a list / CPU tensor (validated, ValueError).  Rows beyond a
    count, and every row of a sample with fewer than three points, are zero.  ValueError for n < 3."""
    return _neighbours(points, None, counts, None, method, False)[2]


def knn3_counted(points, query_idx, counts=None, qcounts=None):
    """knn3 for ragged batches (include/rrl.h rrl_knn3_counted; brute force: the tool for S << n): sample b's first qcounts[b]
    queries among its first counts[b] points; rows beyond are zero.  Device-resident indices and counts are not validated
    on the host (the kernel clamps them); host-side ones are, as knn3 validates (ValueError before any launch)."""
    B, n = _points3(points)
    if n < 3:
        raise ValueError(f"knn3 needs at least 3 points per cloud, got {n}")
    if not isinstance(query_idx, torch.Tensor) or query_idx.dim() != 2:
        raise ValueError("query_idx must be a (B, S) tensor")
    S = query_idx.shape[1]
    hc, hq = _host_counts(counts, B, n, "counts"), _host_counts(qcounts, B, S, "qcounts")
    if not query_idx.is_cuda:
        _check_index_counted(query_idx, hc, n, "query_idx", (B, S))
    elif tuple(query_idx.shape) != (B, S) or query_idx.dtype.is_floating_point:
        raise ValueError(f"query_idx must be an integer tensor of shape {(B, S)}")
    dev = _home(points, query_idx, counts)
    pts = _ops._prep(points, "points", 3, dev)
    qi = query_idx.to(device=dev, dtype=torch.int32).contiguous()
    cnt = _ops.check_counts(counts if hc is None else hc, B, n, dev, "counts")
    qcnt = _ops.check_counts(qcounts if hq is None else hq, B, S, dev, "qcounts")
    nn = torch.empty(B, S, 3, dtype=torch.int32, device=dev)
    _run(dev, "rrl_knn3_counted", _p(pts), _p(cnt), _p(qi), _p(qcnt), _p(nn), None, None, B, n, S)
    return nn


# ---- ball-query grouping and raw point-pair features (include/rrl.h rrl_ball_group) ----------------
FEATURES = ("xyz", "dxyz", "ppf")  # the reference's order (rpm/models/feature_nets.py _raw_features_order), 3 + 3 + 4 channels
FEATURE_SIZES = {"xyz": 3, "dxyz": 3, "ppf": 4}
MAX_NSAMPLE = _lib.GROUP_MAX_SAMPLE


def _channel_mask(features):
    if isinstance(features, str):
        features = (features,)
    features = tuple(features)
    if not features or len(set(features)) != len(features) or any(f not in FEATURES for f in features):
        raise ValueError(f"features must be distinct names out of {FEATURES}, got {features!r}")
    return sum(1 << FEATURES.index(f) for f in features), sum(FEATURE_SIZES[f] for f in features)


def _ball(points, normals, radius, nsample, mask, C, query_idx, counts, qcounts, exclude_self):
    """Every host-side refusal, then the one launch: (feat or None, idx, found)."""
    B, n = _points3(points)
    if isinstance(nsample, bool) or int(nsample) != nsample or not 1 <= int(nsample) <= MAX_NSAMPLE:
        raise ValueError(f"nsample must be an integer in [1, {MAX_NSAMPLE}], got {nsample!r}")
    nsample = int(nsample)
    radius = float(radius)
    if not radius >= 0.0:
        raise ValueError(f"radius must not be negative or NaN, got {radius}")
    try:  # the Python double squared, then rounded: what torch compares its float32 matrix against
        r2 = float(np.float32(radius ** 2))
    except OverflowError:
        r2 = float("inf")
    if not 1 <= B <= 32767 or n < 1:
        raise ValueError(f"ball_query serves 1 .. 32767 clouds of at least one point, got {B} of {n}")
    if n > _ops.sort_capacity():
        raise ValueError(f"ball_query serves clouds up to {_ops.sort_capacity()} points, got {n}")
    if mask & _lib.GROUP_PPF:
        if normals is None:
            raise ValueError('the "ppf" feature needs normals')
        if not isinstance(normals, torch.Tensor) or tuple(normals.shape) != tuple(points.shape):
            raise ValueError(f"normals must be a tensor of the points' shape {tuple(points.shape)}")
    hc = _host_counts(counts, B, n, "counts")
    if query_idx is None:
        S = n
    else:
        if not isinstance(query_idx, torch.Tensor) or query_idx.dim() != 2:
            raise ValueError("query_idx must be a (B, S) tensor")
        S = query_idx.shape[1]
        if not query_idx.is_cuda:
            _check_index_counted(query_idx, hc, n, "query_idx", (B, S))
        elif tuple(query_idx.shape) != (B, S) or query_idx.dtype.is_floating_point:
            raise ValueError(f"query_idx must be an integer tensor of shape {(B, S)}")
    hq = _host_counts(qcounts, B, S, "qcounts")
    dev = _home(points, query_idx, counts)
    pts = _ops._prep(points, "points", 3, dev)
    nrm = _ops._prep(normals, "normals", 3, dev) if mask & _lib.GROUP_PPF else None
    qi = None if query_idx is None else query_idx.to(device=dev, dtype=torch.int32).contiguous()
    cnt = _ops.check_counts(counts if hc is None else hc, B, n, dev, "counts")
    qcnt = _ops.check_counts(qcounts if hq is None else hq, B, S, dev, "qcounts")
    idx = torch.empty(B, S, nsample, dtype=torch.int32, device=dev)
    found = torch.empty(B, S, dtype=torch.int32, device=dev)
    feat = torch.empty(B, S, nsample, C, dtype=torch.float32, device=dev) if mask else None
    _run(dev, "rrl_ball_group", _p(pts), _p(nrm), _p(cnt), _p(qi), _p(qcnt), r2, nsample, int(bool(exclude_self)), mask,
         _p(idx), _p(found), _p(feat), B, n, S)
    return feat, idx, found


def ball_query(points, radius, nsample, *, query_idx=None, counts=None, qcounts=None, exclude_self=True):
    """points (B, n, 3) -> (idx (B, S, nsample) int32, found (B, S) int32): for every query the `nsample` lowest indices j of
    its cloud with |x_j - x_i|^2 <= float32(radius ** 2), ascending -- the reference's query_ball_point
    (rpm/models/pointnet_util.py:96-131) without its (B, S, n) index tensor, distance matrix and row sort.  The distance is
    the float64 sum of rrl_knn3 (the reference's is the expanded float32 matmul: pairs within a few float32 roundings of
    the radius can differ).  found counts the slots that hold a member; the rest hold the pad index.
    exclude_self=True is the reference with `itself_indices` (sample_and_group_multi): the query itself is no member, and it
    is the pad; False is `itself_indices=None` (sample_and_group): the pad is the first member.
    query_idx (B, S) integers (default: every point, S = n), counts / qcounts (B,): as knn3_counted takes them -- on the
    GPU they are read by the kernel only and clamped, on the host they are validated (ValueError before any launch).  Rows
    beyond a count are zero.  Nothing synchronises with device-side arguments: the call can be captured in a graph."""
    return _ball(points, None, radius, nsample, 0, 0, query_idx, counts, qcounts, exclude_self)[1:]


def ball_group(points, normals, radius, nsample, *, features=FEATURES, query_idx=None, counts=None, qcounts=None,
               exclude_self=True):
    """ball_query plus the raw features of its groups in the same launch: (feat (B, S, nsample, C) float32, idx, found) with
    the chosen channels in the reference's order whatever the order of `features`: "xyz" (3) the query's coordinates on
    every slot, "dxyz" (3) x_j - x_i, "ppf" (4) angle(n_i, d), angle(n_j, d), angle(n_i, n_j), |d| with angle(a, b) =
    atan2(|a x b|, a . b) (pointnet_util.py:173-244).  normals (B, n, 3) may be None without "ppf".  A pad slot with
    exclude_self has d = 0: its dxyz and ppf values are exactly 0.  No gradient flows (the reference feeds detached clouds)."""
    mask, C = _channel_mask(features)
    return _ball(points, normals, radius, nsample, mask, C, query_idx, counts, qcounts, exclude_self)


# ---- unit normals from ball groups (include/rrl.h rrl_idx_normals) -----------------------------------
# l1 <= NORMAL_RANK_TOL l2 on the EIGENVALUES of a group's scatter matrix (squared lengths): the members are collinear or
# coincident and have no plane.  Collinear float32 points leave l1 / l2 near 2^-48; 1e-10 is 1e-5 on the lengths themselves.
NORMAL_RANK_TOL = 1e-10


def normals_from_groups(points, idx, found, *, counts=None, return_quality=False):
    """The kernel behind estimate_normals on given index lists: points (B, n, 3), idx (B, S, nsample) int32 and found (B, S)
    int32 as ball_query returns them -> normals (B, S, 3) float32 [, quality (B, S)]."""
    B, n = _points3(points)
    if not (isinstance(idx, torch.Tensor) and isinstance(found, torch.Tensor)) or idx.dim() != 3 or idx.dtype != torch.int32 or \
            found.dtype != torch.int32 or idx.shape[0] != B or tuple(found.shape) != tuple(idx.shape[:2]):
        raise ValueError("idx must be an int32 (B, S, nsample) tensor and found an int32 (B, S) tensor, as ball_query returns them")
    S, nsample = idx.shape[1], idx.shape[2]
    if not 1 <= nsample <= MAX_NSAMPLE:
        raise ValueError(f"nsample must lie in [1, {MAX_NSAMPLE}], got {nsample}")
    if not 1 <= B <= 32767 or not 1 <= n <= _ops.sort_capacity():
        raise ValueError(f"normals are served for 1 .. 32767 clouds of 1 .. {_ops.sort_capacity()} points, got {B} of {n}")
    hc = _host_counts(counts, B, n, "counts")
    dev = _home(points, idx, counts)
    pts = _ops._prep(points, "points", 3, dev)
    cnt = _ops.check_counts(counts if hc is None else hc, B, n, dev, "counts")
    ix, fd = idx.to(device=dev).contiguous(), found.to(device=dev).contiguous()
    normals = torch.empty(B, S, 3, dtype=torch.float32, device=dev)
    quality = torch.empty(B, S, dtype=torch.float32, device=dev) if return_quality else None
    _run(dev, "rrl_idx_normals", _p(pts), 3, _p(ix), _p(fd), _p(cnt), nsample, NORMAL_RANK_TOL, _p(normals), _p(quality), B, n, S)
    return (normals, quality) if return_quality else normals


def estimate_normals(points, radius, nsample=64, *, counts=None, return_quality=False):
    """points (B, n, 3) -> unit normals (B, n, 3) float32: for every point the direction of least variance of its ball group --
    the first `nsample` points (in index order, the point itself among them: ball_query(exclude_self=False)) within `radius`
    --, as the eigenvector of the smallest eigenvalue of the group's scatter matrix (double sums and a double Jacobi
    eigen-decomposition on the device, rounded once).  The normals are NOT oriented: the sign is fixed by a convention (the
    component of largest magnitude is positive), not by an inside or an outside -- enough for point-to-plane residuals, which
    do not see the sign.  A point whose group has fewer than three members, collinear or coincident members, or a non-finite
    member gets the normal (0, 0, 0); so do the rows beyond a count.  counts: as ball_query takes them.
    return_quality=True appends quality (B, n) = (l1 - l0) / l2 of the eigenvalues l0 <= l1 <= l2 (0 for a zero normal): near
    0 where the group does not determine a plane.  Two launches, no read-back: the call can be captured in a graph."""
    idx, found = ball_query(points, radius, nsample, counts=counts, exclude_self=False)
    return normals_from_groups(points, idx, found, counts=counts, return_quality=return_quality)


# ---- k nearest neighbours, any k up to 32, and DCP's graph features (include/rrl.h rrl_knn) ---------
KNN_FEATURES = ("nbr", "dxyz", "ctr")  # the kernel's channel order: x_j, x_j - x_i, x_i; 3 channels each
MAX_K = _lib.CONSTANTS["RRL_KNN_MAX_K"]
# method="auto" takes the tree from this many reference points per cloud (the capacity n): the smallest measured size from
# which the tree was faster than brute force on BOTH cloud kinds (a volume and a surface), at k = 20 and k = 3, at B = 1 and
# B = 8 -- profiles/knn_timing.json, written by tools/knn_timing.py: 256 is the smallest size measured, and the tree won
# there and at every larger one (k = 20: 280 .. 322 us against 364 .. 368 at n = 256, 447 .. 539 against 1230 .. 1253 at 1024,
# 2.3 .. 17.9 ms against 108 .. 661 at 262144; k = 3: 77 .. 84 against 89 .. 96 at n = 256).  None: never.
KNN_TREE_MIN_POINTS = 256


def _knn_channel_mask(features):
    if isinstance(features, str):
        features = (features,)
    features = tuple(features)
    if not features or len(set(features)) != len(features) or any(f not in KNN_FEATURES for f in features):
        raise ValueError(f"features must be distinct names out of {KNN_FEATURES}, got {features!r}")
    return sum(1 << KNN_FEATURES.index(f) for f in features), 3 * len(features)


def _knn(points, k, query, counts, qcounts, exclude_self, want_dist, method, mask, C, channel_first):
    """Every host-side refusal, then the launches of rrl_knn: (feat or None, idx, found, dist2 or None)."""
    B, n = _points3(points)
    if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= MAX_K:
        raise ValueError(f"k must be an integer in [1, {MAX_K}], got {k!r}")
    k = int(k)
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}, got {method!r}")
    if not 1 <= B <= 32767 or n < 1:
        raise ValueError(f"knn serves 1 .. 32767 clouds of at least one point, got {B} of {n}")
    if query is None:
        if qcounts is not None:
            raise ValueError("qcounts belongs to query: the self form's queries are the points, counted by counts")
        S = n
    else:
        if _points3(query)[0] != B:
            raise ValueError(f"query must be a ({B}, S, 3) tensor, got {tuple(query.shape)}")
        if exclude_self:
            raise ValueError("exclude_self belongs to the self form (query=None): a query cloud has no row of its own")
        S = query.shape[1]
    cap = _ops.sort_capacity()
    if method == "tree" and max(n, S) > cap:
        raise ValueError(f"the tree serves clouds up to {cap} points, got {max(n, S)}")
    tree = method == "tree" or (method == "auto" and KNN_TREE_MIN_POINTS is not None and KNN_TREE_MIN_POINTS <= n and max(n, S) <= cap)
    hc = _host_counts(counts, B, n, "counts")
    hq = _host_counts(qcounts, B, S, "qcounts")
    dev = _home(points, query, counts, qcounts)
    pts = _ops._prep(points, "points", 3, dev)
    qry = None if query is None else _ops._prep(query, "query", 3, dev)
    cnt = _ops.check_counts(counts if hc is None else hc, B, n, dev, "counts")
    qcnt = _ops.check_counts(qcounts if hq is None else hq, B, S, dev, "qcounts")
    flags = (_lib.CONSTANTS["RRL_KNN_EXCLUDE_SELF"] if exclude_self else 0) | (_lib.CONSTANTS["RRL_KNN_CHANNEL_FIRST"] if channel_first else 0) | \
        (0 if tree else _lib.CONSTANTS["RRL_KNN_BRUTE"])
    idx = torch.empty(B, S, k, dtype=torch.int32, device=dev)
    found = torch.empty(B, S, dtype=torch.int32, device=dev)
    dist2 = torch.empty(B, S, k, dtype=torch.float32, device=dev) if want_dist else None
    feat = torch.empty((B, C, S, k) if channel_first else (B, S, k, C), dtype=torch.float32, device=dev) if mask else None
    ws = torch.empty(_ops._scratch_size("rrl_knn_workspace_bytes", B, n, S), dtype=torch.uint8, device=dev)
    _run(dev, "rrl_knn", _p(pts), _p(cnt), _p(qry), _p(qcnt), k, flags, mask, _p(ws), ws.numel(), _p(idx), _p(found), _p(dist2),
         _p(feat), B, n, S)
    return feat, idx, found, dist2


def knn(points, k, *, query=None, counts=None, qcounts=None, exclude_self=False, return_dist=False, method="auto"):
    """points (B, n, 3) -> (idx (B, S, k) int32, found (B, S) int32[, dist2 (B, S, k) float32]): for every query the k nearest
    points of its cloud -- the k smallest keys (d, j), d the float64 squared distance (dx dx + dy dy) + dz dz from the float32
    coordinates, j the row: ascending distance, the lowest index among equal distances (include/rrl.h rrl_knn).  A pair whose
    distance is NaN or infinite is no neighbour.  found = min(k, neighbours): k > n is legal.  The slots beyond found repeat
    slot 0; a row without any neighbour (an empty cloud, a NaN query, a row beyond a count) is zero.

    query=None: every point is a query (S = n) and finds itself first at d = 0 -- unless a duplicate has a lower index --;
    exclude_self=True removes the row's own index, not its duplicates.  query (B, S, 3): another cloud's points, with qcounts.
    counts / qcounts (B,): as ball_query takes them -- on the GPU read by the kernels only and clamped, on the host validated
    (ValueError before any launch).  method: "brute", "tree" (both clouds within ops.sort_capacity()) or "auto"
    (KNN_TREE_MIN_POINTS); the same bits.  dist2 is d rounded once.  Nothing synchronises: the call can be captured in a graph."""
    _, idx, found, dist2 = _knn(points, k, query, counts, qcounts, exclude_self, return_dist, method, 0, 0, False)
    return (idx, found, dist2) if return_dist else (idx, found)


def knn_group(points, k, *, features=("nbr", "ctr"), channel_first=False, query=None, counts=None, qcounts=None,
              exclude_self=False, method="auto"):
    """knn plus the features of its groups from the same kernel: (feat, idx, found) with feat (B, S, k, C) float32 -- or
    (B, C, S, k) with channel_first, the layout DCP's get_graph_feature ends in -- and the chosen channels in the kernel's
    order whatever the order of `features`: "nbr" (3) x_j, "dxyz" (3) x_j - x_i (the float32 subtraction), "ctr" (3) x_i on
    every slot.  Pad slots repeat slot 0, rows without a neighbour are zero.  No gradient flows."""
    mask, C = _knn_channel_mask(features)
    return _knn(points, k, query, counts, qcounts, exclude_self, False, method, mask, C, bool(channel_first))[:3]


def estimate_normals_knn(points, k, *, counts=None, return_quality=False):
    """estimate_normals with "the k nearest" in place of a radius ball, which needs no radius tuned to the data's scale:
    points (B, n, 3) -> unit normals (B, n, 3) float32 [, quality (B, n)] from every point's k nearest points (itself among
    them: knn(exclude_self=False)) by normals_from_groups -- same scatter matrix, same eigenvector, same sign convention, same
    zero rows (fewer than three members, collinear or coincident members).  k <= MAX_K.  The k-NN launches plus one, no
    read-back: the call can be captured in a graph."""
    idx, found = knn(points, k, counts=counts)
    return normals_from_groups(points, idx, found, counts=counts, return_quality=return_quality)


def _neighbours(points, num_sample, counts, start, method, want_tri):
    """The launches of pseudo_triangles / knn3_self after every host-side refusal: (sample_idx or None, tri or None, nn,
    tri_counts)."""
    B, n = _points3(points)
    tree = _use_tree(method, n)
    if n < 3:
        raise ValueError(f"pseudo-triangles need at least 3 points per cloud, got {n}")
    hc = _host_counts(counts, B, n, "counts")
    device_counts = counts is not None and hc is None
    if num_sample is None:
        if start is not None:
            raise ValueError("start belongs to the farthest-point sampler: give num_sample with it")
        if method == "tree" and n > _ops.sort_capacity():
            raise ValueError(f"the tree serves clouds up to {_ops.sort_capacity()} points, got {n}")
        S = n
    else:
        if method == "tree":
            raise ValueError('method="tree" serves the all-points form (num_sample=None); given queries take brute force')
        S = min(int(num_sample), n)
        if S < 0:
            raise ValueError(f"num_sample must not be negative, got {num_sample}")
        if start is not None and not (isinstance(start, torch.Tensor) and start.is_cuda):
            start = torch.as_tensor(start)
            _check_index_counted(start, hc, n, "start", (B,))
        elif start is not None and (tuple(start.shape) != (B,) or start.dtype.is_floating_point):
            raise ValueError(f"start must be an integer tensor of shape {(B,)}")
    dev = _home(points, counts, start)
    pts = _ops._prep(points, "points", 3, dev)
    cnt = _ops.check_counts(counts if hc is None else hc, B, n, dev, "counts")
    nn = torch.empty(B, S, 3, dtype=torch.int32, device=dev)
    tri = torch.empty(B, S, 9, dtype=torch.float32, device=dev) if want_tri else None
    tric = torch.empty(B, dtype=torch.int32, device=dev) if want_tri else None
    if num_sample is None:
        if tree and n <= _ops.sort_capacity():
            ws = torch.empty(_ops._scratch_size("rrl_knn3_self_workspace_bytes", B, n), dtype=torch.uint8, device=dev)
            _run(dev, "rrl_knn3_self", _p(pts), _p(cnt), _p(ws), ws.numel(), _p(nn), _p(tri), _p(tric), B, n)
        else:
            _run(dev, "rrl_knn3_counted", _p(pts), _p(cnt), None, _p(cnt), _p(nn), _p(tri), _p(tric), B, n, S)
        return None, tri, nn, tric
    if start is None:
        if device_counts:  # drawn on the device and reduced modulo the count: no read-back
            start = torch.randint(0, n, (B,), device=dev) % cnt.clamp(1, n).to(torch.int64)
        else:  # like the reference (and fps): the CPU generator; with counts all equal to n the uniform call's draw
            start = torch.randint(0, n, (B,), dtype=torch.long)
            if hc is not None:
                start = start % hc.clamp(min=1)
    st = start.to(device=dev, dtype=torch.int32).contiguous()
    idx = torch.empty(B, S, dtype=torch.int32, device=dev)
    qcnt = torch.empty(B, dtype=torch.int32, device=dev)
    scratch = torch.empty(B, n, dtype=torch.float32, device=dev)
    _run(dev, "rrl_fps_counted", _p(pts), _p(cnt), _p(st), _p(idx), _p(qcnt), _p(scratch), B, n, S)
    _run(dev, "rrl_knn3_counted", _p(pts), _p(cnt), _p(idx), _p(qcnt), _p(nn), _p(tri), _p(tric), B, n, S)
    return idx, tri, nn, tric


def pseudo_triangles(points, num_sample=None, *, counts=None, start=None, method="auto", order=False, return_index=False):
    """The pseudo-triangles of a batch of clouds, built on the device: points (B, n, 3) -> tri (B, S, 9) float32, rows
    [p, nn1, nn2] as loss.Sample_neighs lays them out (the rows points[nn0], points[nn1], points[nn2]), and tri_counts.

    num_sample=None: every point gets a triangle, in row order (S = n, no sampling).  num_sample given: the counted
    farthest-point sampler first (S = min(num_sample, n); sample b emits min(S, counts[b]) points, exactly fps's sequence
    on its own points), then the three neighbours of the samples by brute force.
    counts: the points each sample really has -- (B,) int32 on the GPU, read by the kernels only, or a list / CPU tensor,
    validated (ops.check_counts) and uploaded.  points[b, counts[b]:] is never read.  tri_counts (B,) int32 on the GPU holds
    each sample's triangles (0 for a sample of fewer than three points: three neighbours do not exist) and feeds counts1= /
    counts2= of the loss and counts= of ops.cloud_order directly; None without counts.  Rows beyond a count are zero.
    start (B,): the sampler's first index per sample.  By default drawn like the reference's, torch.randint on the CPU
    generator (torch.manual_seed reproduces loss.Sample_neighs), when counts are absent or host-side; with device counts
    it is drawn on the device and reduced modulo the count, with no read-back.
    method: "brute", "tree" (the all-points form only: the sorted layout's sphere tree, n <= ops.sort_capacity()) or
    "auto" (TREE_MIN_POINTS).  Same result, bit for bit.
    order=True appends ops.cloud_order(tri, counts=tri_counts); return_index=True appends (sample_idx (B, S) int32 -- the
    row numbers when nothing was sampled --, nn (B, S, 3) int32), so that a caller can gather differentiably: the output
    itself carries no grad_fn, like the reference's numpy.

    Device-resident counts and start are NOT validated on the host: the kernels clamp them (counts into [0, n], start into
    [0, count)).  Host-side ones are validated as fps / knn3 validate, and refused with ValueError before any launch, as
    are n < 3 and an unknown method.  With device counts and a given start nothing synchronises and the call can be
    captured in a graph (one plain chain of launches)."""
    idx, tri, nn, tric = _neighbours(points, num_sample, counts, start, method, True)
    out = [tri, tric if counts is not None else None]
    if order:
        out.append(_ops.cloud_order(tri, counts=out[1]))
    if return_index:
        if idx is None:
            idx = torch.arange(tri.shape[1], dtype=torch.int32, device=tri.device).expand(tri.shape[0], -1)
        out += [idx, nn]
    return tuple(out)
