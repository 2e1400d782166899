"""Inputs of tests/test_gpu_ragged_chamfer.py (the ragged Chamfer distance: include/rrl.h rrl_chamfer_tree_fwd_counted), shown
sound on the CPU by tests/test_ragged_chamfer_host.py.

Shapes: the smallest that cross the structures' edges -- patch / supergroup 64, leaf 16, partial block 256, the in-kernel
sort's 4096.  Every float case is standard normal float32, seeded.  FILLERS decide what the rows beyond a count hold:
NaN, zeros, or DECOYS -- the absent rows of x are copies of present rows of y and vice versa, so that any read of an absent
row as a point makes a zero-distance minimum."""
import numpy as np

FILLERS = ("nan", "zero", "decoy")

# name -> (seed, B, N, M, counts_x, counts_y)
FLOAT_CASES = {
    "edges": (101, 4, 130, 200, [130, 1, 64, 65], [200, 63, 17, 129]),
    "zero_counts": (102, 3, 70, 70, [0, 70, 5], [70, 0, 5]),
    "full": (103, 2, 300, 257, [300, 300], [257, 257]),
    "wide_sort": (104, 2, 4097, 4200, [4097, 300], [257, 4200]),
    "prepared": (105, 2, 300, 257, [300, 65], [64, 257]),
    "nan": (106, 2, 200, 150, [200, 100], [150, 90]),
    "device_counts": (107, 3, 130, 200, [130, 64, 17], [100, 200, 65]),
    "device_counts_after": (107, 3, 130, 200, [1, 129, 130], [200, 16, 0]),  # the same clouds, the counts written in place
    "backward_float": (108, 3, 300, 257, [300, 1, 129], [257, 200, 64]),
}
BACKWARD_INT = (109, 3, 256, 256, [100, 256, 1], [156, 256, 255])  # pose_refs.chamfer_int_case; cx + cy = 256, 512, 256
BACKWARD_INT_UPSTREAM = [4.0, -0.5, 2.0]  # per-sample route
BACKWARD_INT_SCALAR = 4.0                 # scalar route: sum of the counts = 1024, every scale a power of two
BACKWARD_FLOAT_UPSTREAM = [-2.5, 1.5, 0.75]


def fill(x, y, cx, cy, filler):
    """Copies of x (B, N, 3), y (B, M, 3) whose rows beyond the counts hold the filler."""
    x, y = x.copy(), y.copy()
    for b in range(len(cx)):
        nx, ny = x.shape[1] - cx[b], y.shape[1] - cy[b]
        if filler == "nan":
            x[b, cx[b]:], y[b, cy[b]:] = np.nan, np.nan
        elif filler == "zero" or cx[b] == 0 or cy[b] == 0:  # (no present row to copy: zeros)
            x[b, cx[b]:], y[b, cy[b]:] = 0.0, 0.0
        else:
            assert filler == "decoy"
            px, py = x[b, :cx[b]].copy(), y[b, :cy[b]].copy()
            x[b, cx[b]:] = py[np.arange(nx) % cy[b]]
            y[b, cy[b]:] = px[np.arange(ny) % cx[b]]
    return x, y


def float_case(name, filler="decoy"):
    """(x (B, N, 3), y (B, M, 3), counts_x, counts_y) of FLOAT_CASES[name]; the present rows do not depend on the filler."""
    seed, B, N, M, cx, cy = FLOAT_CASES[name]
    g = np.random.default_rng(seed)
    x, y = g.standard_normal((B, N, 3)).astype(np.float32), g.standard_normal((B, M, 3)).astype(np.float32)
    x, y = fill(x, y, cx, cy, filler)
    return x, y, list(cx), list(cy)


def nan_case():
    """The "nan" case with zeros beyond the counts, then: a NaN in the PRESENT row x[1, 17] (sample 1's target cloud of the
    y -> x direction, and a query of the other), and NaNs in absent rows -- x[1, 100] and y[1, 90], the first rows beyond
    their counts, x[1, 150] and y[1, 149] further out.  Sample 0 (counts = capacities, no absent row) stays finite."""
    x, y, cx, cy = float_case("nan", "zero")
    x[1, 17, 1] = np.nan
    x[1, 100, 0] = x[1, 150, 2] = np.nan
    y[1, 90, 1] = y[1, 149, 0] = np.nan
    return x, y, cx, cy


def reference(oracle, x, y, cx, cy):
    """Per sample, from oracle.chamfer_parts on the truncated pair: [(min_x, arg_x, min_y, arg_y) or None for a sample with an
    empty cloud], values (B,) float32 = the float64 mean of the sample's minima rounded (0 without minima), value float32 =
    the float64 mean over all present minima."""
    parts, vals, allmin = [], [], []
    for b in range(len(cx)):
        if cx[b] == 0 or cy[b] == 0:
            parts.append(None)
            vals.append(np.float32(0.0))
            continue
        p = oracle.chamfer_parts(x[b, :cx[b]], y[b, :cy[b]])
        parts.append(p)
        m = np.concatenate([p[0], p[2]]).astype(np.float64)
        vals.append(np.float32(m.mean()))
        allmin.append(m)
    value = np.float32(np.concatenate(allmin).mean()) if allmin else np.float32(0.0)
    return parts, np.asarray(vals, np.float32), value


def expected_keys(part, count, cap):
    """int64 (cap,): distance bits << 32 | argmin for the present rows, -1 beyond the count."""
    out = np.full(cap, -1, np.int64)
    if part is not None:
        mins, args = part
        out[:count] = ((mins.view(np.uint32).astype(np.uint64) << np.uint64(32)) | args.astype(np.uint64)).view(np.int64)
    return out
