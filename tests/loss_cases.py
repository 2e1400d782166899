"""The input sets of tests/test_gpu_loss_stages.py, built on the host from seeds (numpy, the CPU oracle's sampler) so that
tests/test_loss_refs_host.py can show for every one of them, without a GPU, that the oracle's NaN flag is clear, that at
least 64 lines are selected, that at most TIE_CAP of the selected lines hold a near tie and that the C oracle (a correct
float32 implementation) stays inside every bound the GPU test applies.  A sample is dict(tri1 (N, 9), tri2 (M, 9),
lines (L, 6)) float32; `empty` marks a sample whose lines hit nothing on purpose."""
import numpy as np

TIE_CAP = 0.005
SCALES = [1.0, 12.0, 300.0, 5000.0]
OFFSET = np.array([3.0, -2.0, 1.5], np.float32)
# The line streams (seeds of synth.uniform_streams) of every set, searched on the moved clouds with the twin alone so that the
# oracle's NaN flag is clear and the share of selected lines that hold a near tie stays under TIE_CAP (the search kept a margin:
# it took the first stream at or below 0.4 %; tests/test_loss_refs_host.py asserts the flag and the cap).  Most near ties on
# these clouds are pairs of SATURATED Welsch terms (D > 25 med: 1 - exp(-D / 2 med) equals 1 to seven digits), a few per
# thousand selected lines; with ~130 selected lines a set must have none.
SCALE_STREAMS = {(1.0, False): 3, (1.0, True): 19, (12.0, False): 3, (12.0, True): 29, (300.0, False): 62, (300.0, True): 62,
                 (5000.0, False): 25, (5000.0, True): 70, (0.01, False): 3}
ROUTE_STREAMS = {(600, True): (12, 13, 2), (600, False): (3, 13, 2), (900, True): (15, 22, 17), (1000, True): (12, 7, 14),
                 (1000, False): (3, 4, 8), (4500, True): (21, 376, 23), (4500, False): (9, 13, 14), (3000, True): (42, 61, 35)}
XCHG_STREAMS = (0, 1, 2, 3)
BIG_STREAM = 17
_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _pair_with_lines(oracle, seed, n, m, nl, stream, scale=1.0, far=False):
    from rrl_hip import synth
    p = synth.make_pair(seed, n, m)
    sc = np.float32(scale)
    off = OFFSET * sc if far else np.zeros(3, np.float32)
    src, tar = p["src"] * sc + off, p["tar"] * sc + off
    lines = oracle.resample_lines(synth.uniform_streams(stream, 10, nl), float(p["radius"]) * scale,
                                  np.asarray(p["center"] * sc + off, np.float32), src, tar, nl)
    return dict(tri1=np.ascontiguousarray(p["src_tri"] * sc + np.tile(off, 3), np.float32),
                tri2=np.ascontiguousarray(p["tar_tri"] * sc + np.tile(off, 3), np.float32),
                lines=np.ascontiguousarray(lines, np.float32))


def scaled_pair(oracle, scale, far):
    """make_pair(77, 1500, 1100) scaled (and moved by OFFSET * scale) with 6000 lines of the reference's sampler."""
    return _cached(("scaled", scale, far), lambda: _pair_with_lines(oracle, 77, 1500, 1100, 6000, SCALE_STREAMS[(scale, far)], scale, far))


def poses(B, seed=2, mag=0.03):
    """B small rigid motions (R (B, 3, 3), t (B, 3) float32) from the host Lie algebra package, seeded."""
    import torch
    from LieAlgebra import se3
    xi = torch.stack([mag * torch.randn(6, generator=torch.Generator().manual_seed(1000 * seed + b)) for b in range(B)])
    Rm, T = se3.exp3(xi)  # (pose b does not depend on B)
    return Rm.contiguous().numpy(), T.contiguous().numpy()


def with_pose(oracle, s, Rm, T, tr):
    """The sample with a pose: `moved` is the source moved on the host (x R^T + t with tr, else x R + t) -- what the entries
    without a pose of their own are given as points1, and what the host file checks the input conditions on (the library
    moves the source itself; its triangles agree with these to a rounding)."""
    moved = oracle.rigid_apply(s["tri1"].reshape(-1, 3), Rm, T, tr).reshape(-1, 9)
    return dict(s, R=np.ascontiguousarray(Rm, np.float32), T=np.ascontiguousarray(T, np.float32), tr=bool(tr), moved=moved)


def route_batch(oracle, nl, tr=True, B=3, n=900, m=800, seed=40, streams=None):
    """make_pair(seed + b, n, m) with nl sampled lines each and a pose per sample: the batch of the route tests."""
    streams = ROUTE_STREAMS[(nl, tr)] if streams is None else streams
    Rm, T = poses(B)
    return _cached(("route", nl, tr, B, n, m, seed), lambda: [
        with_pose(oracle, _pair_with_lines(oracle, seed + b, n, m, nl, streams[b]), Rm[b], T[b], tr) for b in range(B)])


def dense_batch(nl, B=3):
    """Two tiny triangles per cloud, every line through the first: ~nl selected lines in one (1, 1) bucket, k ~ nl
    contributions to one gradient row, near-identical D values (the median's crowded bin), a median of ~1e-5."""
    def make():
        gen = np.random.default_rng(5)
        base = np.array([[0.0, 0.0, 0.0, 0.05, 0.0, 0.0, 0.0, 0.05, 0.0]], np.float32)
        t1 = np.concatenate([base, base + np.float32(3.0)]).astype(np.float32)
        d = np.tile(np.array([[0.0, 0.0, 1.0]]), (nl, 1))
        out = []
        for b in range(B):
            t2 = (t1 + np.array([0.004, -0.003, 0.002] * 3, np.float32) * np.float32(1 + 0.1 * b)).astype(np.float32)
            x0 = np.tile(np.array([[0.012, 0.011, -1.0]]), (nl, 1)) + 1e-5 * (b + 1) * gen.standard_normal((nl, 3))
            out.append(dict(tri1=t1, tri2=t2, lines=np.concatenate([d, x0], 1).astype(np.float32)))
        return out
    return _cached(("dense", nl, B), make)


def empty_sample_batch(oracle, nl=3000):
    def make():
        ss = [dict(s) for s in route_batch(oracle, nl)]
        ss[1]["lines"] = np.tile(np.array([[1.0, 0, 0, 0, 50, 50]], np.float32), (nl, 1))
        ss[1]["empty"] = True
        return ss
    return _cached(("empty", nl), make)


def big_cloud(oracle):
    """N = 65540 source triangles (the dense scan, the rigid backward in a launch of its own), at the demo's scale 12: at
    unit scale so dense a cloud has thresholds below sqrt(2e-4) and nothing ever hits."""
    Rm, T = poses(1)
    return _cached("big", lambda: [with_pose(oracle, _pair_with_lines(oracle, 61, 65540, 300, 1200, BIG_STREAM, 12.0), Rm[0],
                                             T[0] * np.float32(12.0), True)])


def xchg_batch(oracle, B=40):
    """B x tiles > 256: four distinct pairs of 200 / 180 triangles with 8000 lines, repeated along the batch."""
    base = route_batch(oracle, 8000, True, 4, 200, 180, 50, XCHG_STREAMS)
    return [base[b % 4] for b in range(B)]


def golden_sample(name, nl=None):
    from conftest import load_golden
    g = load_golden(name)
    return dict(tri1=g["tri1"], tri2=g["tri2"], lines=g["lines"][:nl] if nl else g["lines"])


NARROW = (1, 1, 5, 5)
HOST_SETS = {
    "routes_600": lambda o: (route_batch(o, 600), NARROW),
    "routes_600_x_R": lambda o: (route_batch(o, 600, False), NARROW),
    "routes_900": lambda o: (route_batch(o, 900), NARROW),
    "routes_1000": lambda o: (route_batch(o, 1000), NARROW),
    "routes_1000_x_R": lambda o: (route_batch(o, 1000, False), NARROW),
    "routes_4500": lambda o: (route_batch(o, 4500), NARROW),
    "routes_4500_x_R": lambda o: (route_batch(o, 4500, False), NARROW),
    "dense_1000": lambda o: (dense_batch(1000), NARROW),
    "dense_2600": lambda o: (dense_batch(2600), NARROW),
    "empty_sample": lambda o: (empty_sample_batch(o), NARROW),
    "big_cloud": lambda o: (big_cloud(o), NARROW),
    "xchg": lambda o: (xchg_batch(o, 4), NARROW),
    "c_is_1": lambda o: ([scaled_pair(o, 1.0, False)], (2, 1, 3, 2)),
    "narrow_1235": lambda o: ([golden_sample("loss_ref_real0.npz")], (1, 2, 3, 5)),
    "wide_1199": lambda o: ([golden_sample("loss_ref_human0.npz")], (1, 1, 9, 9)),
    "pooled": lambda o: ([dict(tri1=a, tri2=b, lines=c) for a, b, c in zip(*(golden_sample("loss_b2_quirk.npz")[k]
                                                                             for k in ("tri1", "tri2", "lines")))], NARROW),
}
