"""Inputs and references of tests/test_gpu_prep_kernels.py: the kernels every trainer runs BEFORE the loss sees a line -- the
farthest-point sampler and the 3-NN of csrc/rrl_neigh.hip, the two AABB kernels of csrc/rrl_geom.hip and the candidate
generation of csrc/rrl_sampler.h with the library's own Philox4x32-10 generator.

Small host twins in numpy, none of them computed from the code under test:
  * EXACT: fps_ref (the reference's loop in float32, no FMA: the index sequence is the reference's), knn3_ref (float64
    distances, stable sort: ties to the lower index), aabb_ref, philox4x32_10 / sampler_uniforms (integers);
  * FLOAT64 with a YARDSTICK: candidate_ref evaluates the chord construction in float64 (the truth) and in float32 (numpy's
    libm, no FMA: the yardstick); the device, with another sincosf, may be CAND_FACTOR times as far from the truth as the
    float32 host evaluation on the same candidates, plus CAND_ULPS ulp of max(radius, |centre|) (candidate_bound).
tests/test_prep_refs_host.py ties the twins to the reference's recorded data (tests/golden/sample_neighs.npz bit for bit,
sampler.npz within the bound) and Philox to the published Random123 known answers."""
import numpy as np

# ----------------------------------------------------------------------------------------------------------------- clouds
FPS_LANES = 1024             # lanes of fps_kernel's one workgroup per cloud: lane t owns points t, t + 1024, ...
FPS_N = [1, 2, 63, 64, 65, 1023, 1024, 1025, 2049]  # 1025: the first n at which a lane owns two points; 2049: three trips
FPS_BATCH = (3, 1500)        # B, n; starts [0, n - 1, 700]: the per-sample stride of pts, start and out
FPS_BATCH_STARTS = [0, 1499, 700]
FPS_LDS_MAX = 8192           # n * 16 bytes <= 128 KiB: points and distances in LDS; beyond: global memory
FPS_SWITCH = [(2, 8192, 1024), (2, 8193, 1024)]  # B, n, S on both sides of the switch
LATTICE_SIDE, LATTICE_COPIES = 12, 300
FAR_N, FAR_S, FAR_SCALE = 1500, 200, 2.0e5
FPS_CAP = np.float32(1e10)   # the reference's initial distance (code/utils.py:286): squared distances above it tie

KNN_LANES = 256
KNN_SHAPES = [(3, 3), (4, 4), (300, 1), (300, 255), (300, 256), (300, 257), (2049, 700)]  # (n, S)
KNN_LATTICE_S = 700

AABB_N = [1, 63, 64, 65, 1023, 1024, 1025, 5000]
AABB_HOT_N = 2500
AABB_HOT_AT = [0, 1, 63, 64, 1023, 1024, 2047, 2048, 2499]  # lane, wave and trip edges of the 1024-lane reduction

CAND_N = [1, 1023, 1024, 1025, 3000]
CAND_B = 3
CAND_RADII = np.array([1.7, 0.6, 12.5], np.float32)
CAND_CENTRES = np.array([[0.0, 0.0, 0.0], [-0.3, 0.2, 0.1], [40.0, -25.0, 17.0]], np.float32)  # one far from the origin
CAND_ROUNDS = 10
CAND_FACTOR, CAND_ULPS = 4.0, 2.0
SHORT_CHORD, SHORT_CHORD_CAP = 0.05, 0.005  # directions of chords below 0.05 rad may be left out: at most 0.5 % of a set

RNG_SEEDS = [1234, 0x123456789ABCDEF0 & 0x7FFFFFFFFFFFFFFF]  # the second puts both key words in use
RNG_PLAIN = (3, 1500)        # B, n of the no-box call
RNG_WIDE = (3, 3000)         # the write pass spans 9 workgroups
RNG_HIGH_CALL = 2 ** 32 + 5  # the high counter word
RNG_ROUNDS_N = 2000


def gaussian_cloud(seed, B, n):
    """(B, n, 3) float32 standard normal: B different clouds."""
    return np.random.default_rng(seed).standard_normal((B, n, 3)).astype(np.float32)


def lattice_cloud(seed):
    """(2028, 3) float32: the 12 x 12 x 12 integer lattice in shuffled order, then 300 copies of lattice points.  Every
    squared distance is an exact integer (<= 363), ties are everywhere, and every copy has a twin at a LOWER index."""
    g = np.random.default_rng(seed)
    a = np.arange(LATTICE_SIDE)
    grid = np.stack(np.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3)
    grid = grid[g.permutation(len(grid))]
    copies = grid[g.integers(0, len(grid), LATTICE_COPIES)]
    return np.concatenate([grid, copies]).astype(np.float32)


def far_cloud(seed):
    """(1500, 3) float32 uniform in [-2e5, 2e5]^3: most squared distances exceed the 1e10 cap."""
    return (np.random.default_rng(seed).uniform(-1.0, 1.0, (FAR_N, 3)) * FAR_SCALE).astype(np.float32)


# ----------------------------------------------------------------------------------------------------------------- FPS, 3-NN
def sq_dist(p, c):
    """(dx dx + dy dy) + dz dz in p's dtype, every product and sum rounded (numpy never fuses)."""
    d = p - c
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def fps_ref(points_f32, S, start, return_dist=False):
    """code/utils.py:275-296 on one cloud (n, 3) in float32: distance = 1e10; S times: emit the current point, distance =
    minimum(distance, squared distance to it), next = argmax (first occurrence).  (S,) int64."""
    p = np.ascontiguousarray(points_f32, np.float32)
    assert p.dtype == np.float32 and p.ndim == 2 and 0 <= int(start) < len(p)
    dist = np.full(len(p), FPS_CAP, np.float32)
    out = np.empty(S, np.int64)
    far = int(start)
    for it in range(S):
        out[it] = far
        s = sq_dist(p, p[far])
        assert s.dtype == np.float32
        dist = np.minimum(dist, s)
        far = int(np.argmax(dist))
    return (out, dist) if return_dist else out


def knn3_ref(points, query_idx):
    """(S, 3) int64: the three nearest points of every query among ALL n points of its cloud (the query itself and its
    duplicates included) by float64 squared distances (dx dx + dy dy) + dz dz, ascending, ties to the lower index."""
    p = np.asarray(points).astype(np.float64)
    q = np.asarray(query_idx).astype(np.int64)
    assert len(p) >= 3
    d = p[q][:, None, :] - p[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    return np.argsort(d2, axis=1, kind="stable")[:, :3]


def aabb_ref(v):
    """(B, n, 3) -> (B, 6) = min xyz, max xyz, exact."""
    v = np.asarray(v)
    return np.concatenate([v.min(1), v.max(1)], axis=1)


# ----------------------------------------------------------------------------------------------------------------- Philox
_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(counter4, key2):
    """Philox4x32 with 10 rounds (Salmon et al., Random123): counter4 = four and key2 = two arrays (or scalars) of 32-bit
    words, broadcast against each other -> (4, ...) uint32."""
    c = [np.asarray(x, np.uint64) & _M32 for x in counter4]
    k = [np.asarray(x, np.uint64) & _M32 for x in key2]
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*c, *k)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0  # 32 x 32 bits: no overflow of uint64
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _M32, (p0 >> _S32) ^ c3 ^ k1, p0 & _M32
        k0 = (k0 + np.uint64(0x9E3779B9)) & _M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & _M32
    return np.stack([c0, c1, c2, c3]).astype(np.uint32)


def sampler_uniforms(seed, call, b, rd, i):
    """The four uniforms of candidate(s) i of round rd of sample b in call number `call` of the library's generator, as
    csrc/rrl_sampler.h documents them: counter (i, rd | b << 16, call & 0xffffffff, call >> 32), key (seed & 0xffffffff,
    seed >> 32), u = (x >> 8) / 2^24.  (4, len(i)) float32 (24-bit values: exact)."""
    seed, call = int(seed), int(call)
    assert 0 <= seed < 1 << 64 and 0 <= call < 1 << 64 and 0 <= int(rd) < 1 << 16 and 0 <= int(b) < 1 << 16
    x = philox4x32_10((np.asarray(i, np.uint64), int(rd) | (int(b) << 16), call & 0xFFFFFFFF, call >> 32),
                      (seed & 0xFFFFFFFF, seed >> 32))
    return ((x >> np.uint32(8)).astype(np.float64) / 2.0 ** 24).astype(np.float32)


# ----------------------------------------------------------------------------------------------------------------- candidates
def candidate_ref(u, rad, centre, dtype):
    """The chord construction of sample_line (code/loss.py:394-411) in `dtype` (np.float64: the truth; np.float32: the
    yardstick) from float32 inputs: u (4, n) uniforms, radius, centre (3,).  pi = float32(3.14159274101257324);
    q = (rad s cos a, rad sin a s, rad v) with a = (u 2) pi, v = u 2 - 1, s = sqrt(1 - v v); direction = (q2 - q1) /
    max(|q2 - q1|, 1e-12), origin = q1 + centre.  Returns (lines (n, 6) in dtype, chord length |q2 - q1| (n,))."""
    u = np.asarray(u)
    assert u.dtype == np.float32 and u.shape[0] == 4
    u = u.astype(dtype)
    rad, centre = dtype(np.float32(rad)), np.asarray(centre, np.float32).astype(dtype)
    pi, one, two = dtype(np.float32(3.14159274101257324)), dtype(1), dtype(2)

    def point(ua, uv):
        al, v = (ua * two) * pi, uv * two - one
        s = np.sqrt(one - v * v)
        return np.stack([(rad * s) * np.cos(al), (rad * np.sin(al)) * s, rad * v], -1)
    q1, q2 = point(u[0], u[1]), point(u[2], u[3])
    d = q2 - q1
    chord = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    lines = np.concatenate([d / np.maximum(chord, dtype(1e-12))[:, None], q1 + centre], axis=1)
    assert lines.dtype == dtype
    return lines, chord


def candidate_bound(u, rad, centre):
    """What a device evaluation of the candidates of u is held to: dict(ref (n, 6) float64, keep (n,) bool -- the candidates
    whose DIRECTION is compared: float64 chord >= 0.05 rad --, host = (direction, origin) largest absolute error of the
    float32 numpy evaluation against float64, bound = (direction, origin) = CAND_FACTOR host + CAND_ULPS ulp of
    max(rad, largest |centre| component)).  Asserts that at most 0.5 % of the set is left out."""
    ref, chord = candidate_ref(u, rad, centre, np.float64)
    host, _ = candidate_ref(u, rad, centre, np.float32)
    keep = chord >= SHORT_CHORD * float(np.float32(rad))
    assert np.count_nonzero(~keep) <= SHORT_CHORD_CAP * len(keep), (np.count_nonzero(~keep), len(keep))
    err = np.abs(host.astype(np.float64) - ref)
    herr = (float(err[keep, :3].max()) if keep.any() else 0.0, float(err[:, 3:].max()))
    floor = CAND_ULPS * float(np.spacing(np.float32(max(float(np.float32(rad)), float(np.abs(np.asarray(centre, np.float32)).max())))))
    return dict(ref=ref, keep=keep, host=herr, bound=(CAND_FACTOR * herr[0] + floor, CAND_FACTOR * herr[1] + floor),
                left_out=float(np.count_nonzero(~keep)) / len(keep))


def candidate_errors(got, cb):
    """(direction, origin) largest absolute error of lines `got` (n, 6) against candidate_bound's float64 reference: the
    directions over the kept candidates, the origins over all."""
    err = np.abs(np.asarray(got, np.float64) - cb["ref"])
    return (float(err[cb["keep"], :3].max()) if cb["keep"].any() else 0.0, float(err[:, 3:].max()))
