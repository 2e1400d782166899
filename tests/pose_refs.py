"""Inputs and references of tests/test_gpu_pose_kernels.py: the pose-side kernels of csrc/rrl_geom.hip (rigid apply forward
and backward, the SE(3) exponential and its dual-number backward, the gated Adam update, the Chamfer backward).

Two kinds of reference, both computed on the host and neither from the code under test:
  * EXACT: inputs on an integer grid (or scaled by a power of two) whose every product and partial sum is a float32 number,
    so the float32 result does not depend on FMA contraction or on the order of a sum and must equal the int64 / float64
    reference bit for bit;
  * FLOAT64 with a YARDSTICK: general floats are compared with a float64 evaluation, and the allowed error is that of a plain
    float32 evaluation of the same reference (a sequential float32 sum; the host LieAlgebra package in float32) -- or is
    derived from the number of roundings (Chamfer).
tests/test_pose_refs_host.py checks on the CPU that the exact cases are exact and that the yardsticks are finite and can be met."""
import numpy as np

U32 = 2.0 ** -24  # unit roundoff of float32: the largest relative error of one rounding

# ----------------------------------------------------------------------------------------------------------------- rigid
RIGID_PTS = 16384            # points per workgroup of rigid_bwd_kernel (one launch up to here, partials + finalize beyond)
RIGID_N = [1, 63, 1024, 1025, 16383, 16384, 16385, 40000]
RIGID_N_GRID_LOOP = 524293   # beyond 2048 * 256 points rigid_fwd_kernel loops over its grid
ONE_HOT_N = 40000
ONE_HOT_AT = [0, 1023, 1024, 16383, 16384, 32767, 32768, ONE_HOT_N - 1]  # lane, wave and workgroup edges of the backward


def rigid_int_case(seed, B, n):
    """x, gy (B, n, 3) and t (B, 3) integers in [-4, 4], R (B, 3, 3) integers in [-2, 2], all float32 (point-major).
    |y|, |gx| <= 28 and every partial sum of gR / gt is an integer of magnitude <= 16 n <= 2^24 (n <= 2^20): exact."""
    assert 16 * n <= 1 << 24
    g = np.random.default_rng(seed)
    x = g.integers(-4, 5, (B, n, 3)).astype(np.float32)
    gy = g.integers(-4, 5, (B, n, 3)).astype(np.float32)
    R = g.integers(-2, 3, (B, 3, 3)).astype(np.float32)
    t = g.integers(-4, 5, (B, 3)).astype(np.float32)
    return dict(x=x, R=R, t=t, gy=gy)


def rigid_one_hot_case(seed, B, n, at):
    """The integer case with gy zero except at point `at`, where gy and x have no zero component."""
    c = rigid_int_case(seed, B, n)
    g = np.random.default_rng(seed + 1)
    nz = lambda: (g.integers(1, 5, (B, 3)) * g.choice([-1, 1], (B, 3))).astype(np.float32)
    hot = nz()
    c["gy"][:] = 0.0
    c["gy"][:, at] = hot
    c["x"][:, at] = nz()
    return c


def rigid_reference(c, transpose_r, dtype=np.int64):
    """y = x m + t, gx = gy m^T, gm = x^T gy, gt = sum gy with m = R^T (transpose_r) or R; gR is gm in R's layout.
    dtype int64 for the integer cases, float64 for general floats."""
    x, R, t, gy = (np.asarray(c[k]).astype(dtype) for k in ("x", "R", "t", "gy"))
    m = R.transpose(0, 2, 1) if transpose_r else R
    y = np.einsum("bni,bij->bnj", x, m) + t[:, None, :]
    gx = np.einsum("bnj,bij->bni", gy, m)
    gm = np.einsum("bni,bnj->bij", x, gy)
    return dict(y=y, gx=gx, gR=gm.transpose(0, 2, 1) if transpose_r else gm, gt=gy.sum(1))


def rigid_float_case(seed, B, n):
    """Standard normal x, gy (B, n, 3), t (B, 3) and an orthonormal R (B, 3, 3), float32."""
    g = np.random.default_rng(seed)
    R = np.stack([np.linalg.qr(g.standard_normal((3, 3)))[0] for _ in range(B)])
    return dict(x=g.standard_normal((B, n, 3)).astype(np.float32), R=R.astype(np.float32),
                t=g.standard_normal((B, 3)).astype(np.float32), gy=g.standard_normal((B, n, 3)).astype(np.float32))


def rigid_sum_terms(c):
    """The 12 B sums of the backward as (B, 12, n) float64 terms: rows 3 i + j hold x_i gy_j (gm[i][j]), rows 9 + j hold gy_j.
    (A product of two float32 numbers is exact in float64.)"""
    x, gy = c["x"].astype(np.float64), c["gy"].astype(np.float64)
    B, n, _ = x.shape
    out = np.empty((B, 12, n))
    for i in range(3):
        for j in range(3):
            out[:, 3 * i + j] = x[:, :, i] * gy[:, :, j]
    out[:, 9:] = gy.transpose(0, 2, 1)
    return out


def outputs_as_sums(gR, gt, transpose_r):
    """(B, 12) in rigid_sum_terms' row order from gR (B, 3, 3) in R's layout and gt (B, 3)."""
    gm = np.asarray(gR).transpose(0, 2, 1) if transpose_r else np.asarray(gR)
    return np.concatenate([gm.reshape(len(gm), 9), np.asarray(gt)], axis=1)


def normalised_error(got, terms):
    """|got - float64 sum| / float64 sum of |terms| per output, (B, 12)."""
    return np.abs(np.asarray(got, np.float64) - terms.sum(-1)) / np.abs(terms).sum(-1)


def sequential_f32_sums(terms):
    """The yardstick: the float32 terms added one after the other in float32, (B, 12)."""
    return np.cumsum(terms.astype(np.float32), axis=-1, dtype=np.float32)[..., -1]


def kernel_order_f32_sums(terms):
    """The summation order of rigid_bwd_kernel emulated in numpy: per workgroup of 16384 points 1024 lanes take 16 points
    each (stride 1024, fused multiply-add: one rounding per term), an adjacent-pair tree over the 64 lanes of a wave, the 16
    waves one after the other; the workgroups in double, rounded once.  (B, 12) float32."""
    B, Q, n = terms.shape
    nblk = -(-n // RIGID_PTS)
    pad = np.zeros((B, Q, nblk * RIGID_PTS))
    pad[..., :n] = terms
    pad = pad.reshape(B, Q, nblk, 16, 1024)
    acc = np.zeros((B, Q, nblk, 1024), np.float32)
    for k in range(16):
        acc = (acc.astype(np.float64) + pad[..., k, :]).astype(np.float32)
    a = acc.reshape(B, Q, nblk, 16, 64)
    while a.shape[-1] > 1:
        a = a[..., 0::2] + a[..., 1::2]
    a = a[..., 0]
    s = np.zeros((B, Q, nblk), np.float32)
    for w in range(16):
        s = s + a[..., w]
    return s[..., 0] if nblk == 1 else s.astype(np.float64).sum(-1).astype(np.float32)


# ----------------------------------------------------------------------------------------------------------------- SE(3)
SE3_MAGS = [0.0, 1e-20, 1e-4, 0.0099, 0.0101, 0.5, 1.0, 3.1405, float(np.float32(np.pi)), 3.6, 6.2822, 6.5, 30.0]
SE3_PER_MAG = 64
SE3_EXACT_MAGS = (0.0, 1e-20)  # the float32 host evaluation of R and T has no error at all here
SE3_CHUNKS = [1, 10, 11, 64, 65]
SE3_FACTOR, SE3_FLOOR_UNITS = 4.0, 8.0


def se3_case(seed=17):
    """xi (832, 6) float32: per magnitude of SE3_MAGS 64 random rotation directions scaled to it (group g = rows 64 g ..
    64 g + 63) and standard normal translations; cR (832, 3, 3), cT (832, 3): the contraction sum cR R + sum cT T."""
    g = np.random.default_rng(seed)
    n = len(SE3_MAGS) * SE3_PER_MAG
    d = g.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    w = d * np.repeat(np.asarray(SE3_MAGS), SE3_PER_MAG)[:, None]
    xi = np.concatenate([w, g.standard_normal((n, 3))], axis=1).astype(np.float32)
    return dict(xi=xi, cR=g.standard_normal((n, 3, 3)).astype(np.float32), cT=g.standard_normal((n, 3)).astype(np.float32))


def se3_host(c, dtype, use_R=True, use_T=True):
    """LieAlgebra.se3.exp3 on the CPU in `dtype` (torch.float64: the reference; torch.float32: the yardstick) and the
    gradient of the contraction by autograd: dict(R, T, gxi) of float64 numpy arrays."""
    import torch
    from LieAlgebra import se3
    x = torch.from_numpy(c["xi"]).to(dtype).requires_grad_(True)
    R, T = se3.exp3(x)
    s = 0
    if use_R:
        s = s + (R * torch.from_numpy(c["cR"]).to(dtype)).sum()
    if use_T:
        s = s + (T * torch.from_numpy(c["cT"]).to(dtype)).sum()
    s.backward()
    return {k: v.detach().double().numpy() for k, v in (("R", R), ("T", T), ("gxi", x.grad))}


def _group_max(a):
    a = np.abs(np.asarray(a, np.float64))
    return a.reshape(len(SE3_MAGS), -1).max(1)


def se3_yardstick(ref64, host32):
    """{output: (host error (13,), allowed error (13,))}: per magnitude group the float32 host evaluation's largest
    absolute error against float64, and SE3_FACTOR times it plus SE3_FLOOR_UNITS float32 roundings of the group's largest
    value of that output."""
    out = {}
    for k in ("R", "T", "gxi"):
        herr = _group_max(host32[k] - ref64[k])
        out[k] = (herr, SE3_FACTOR * herr + SE3_FLOOR_UNITS * U32 * _group_max(ref64[k]))
    return out


def se3_group_errors(got, ref64):
    """{output: largest absolute error per magnitude group (13,)} of dict(R, T, gxi) against the float64 reference."""
    return {k: _group_max(np.asarray(got[k], np.float64) - ref64[k]) for k in ("R", "T", "gxi")}


def se3_table(errs, yard):
    """The per-group table the GPU test prints (DESIGN.md section 6 quotes it)."""
    rows = ["   |w|        " + "".join(f"{k + ' gpu':>11}{k + ' host':>11}{k + ' bound':>11}" for k in ("R", "T", "gxi"))]
    for g, m in enumerate(SE3_MAGS):
        rows.append(f"{m:<12.6g}  " + "".join(f"{errs[k][g]:11.2e}{yard[k][0][g]:11.2e}{yard[k][1][g]:11.2e}" for k in ("R", "T", "gxi")))
    return "\n".join(rows)


# ----------------------------------------------------------------------------------------------------------------- Adam
ADAM_N = [1, 255, 256, 257, 1000]
ADAM_STEPS, ADAM_GATED_OFF, ADAM_LR = 8, (2, 5), {0: 2e-2, 4: 1e-2}  # step -> the learning rate from that step on


def adam_case(n, seed=23):
    """p0 (n,), the gradients of the 8 steps (8, n) float32, the gate (0: skipped) and the learning rate of every step."""
    g = np.random.default_rng(seed)
    p0 = g.standard_normal(n).astype(np.float32)
    grads = (g.standard_normal((ADAM_STEPS, n)) * (0.1 + np.arange(ADAM_STEPS))[:, None]).astype(np.float32)
    lrs, lr = [], None
    for it in range(ADAM_STEPS):
        lr = ADAM_LR.get(it, lr)
        lrs.append(lr)
    return dict(p0=p0, grads=grads, gates=[0 if it in ADAM_GATED_OFF else 3 for it in range(ADAM_STEPS)], lrs=lrs)


def adam_reference(c):
    """The parameter after every step, (8, n) float32, from torch.optim.Adam on the CPU (a gated-off step: no call)."""
    import torch
    ref = torch.nn.Parameter(torch.from_numpy(c["p0"].copy()))
    opt = torch.optim.Adam([ref], lr=c["lrs"][0])
    out = []
    for it in range(ADAM_STEPS):
        opt.param_groups[0]["lr"] = c["lrs"][it]
        if c["gates"][it]:
            ref.grad = torch.from_numpy(c["grads"][it].copy())
            opt.step()
        out.append(ref.detach().numpy().copy())
    return np.stack(out)


# ----------------------------------------------------------------------------------------------------------------- Chamfer
CHAMFER_SHAPES = [(1, 1, 1), (2, 255, 257), (1, 256, 256), (4, 257, 767), (1, 1500, 548)]  # B (N + M) a power of two
CHAMFER_ONE_TARGET = (1, 768, 256)   # every target the same point: N atomics onto one address
CHAMFER_GVALS = [4.0, -0.5]
CHAMFER_FLOAT_SHAPE, CHAMFER_FLOAT_GVAL = (3, 300, 257), -2.5


def chamfer_int_case(seed, B, N, M, one_target=False):
    """x (B, N, 3), y (B, M, 3): integers in [-8, 8] as float32 (ties and duplicates in plenty)."""
    g = np.random.default_rng(seed)
    x = g.integers(-8, 9, (B, N, 3)).astype(np.float32)
    y = g.integers(-8, 9, (B, M, 3)).astype(np.float32)
    if one_target:
        y[:] = y[:, :1]
    return x, y


def chamfer_float_case(seed=29):
    B, N, M = CHAMFER_FLOAT_SHAPE
    g = np.random.default_rng(seed)
    return g.standard_normal((B, N, 3)).astype(np.float32), g.standard_normal((B, M, 3)).astype(np.float32)


def chamfer_nearest(x, y, dtype):
    """(ix (B, N), iy (B, M), value): the first nearest target of every query in both directions with squared distances
    (dx^2 + dy^2) + dz^2 evaluated in `dtype` (int64 for the integer cases, float32 = the kernels' arithmetic, float64), and
    the mean of all B (N + M) minima in float64."""
    a, b = np.asarray(x).astype(dtype), np.asarray(y).astype(dtype)
    d = a[:, :, None, :] - b[:, None, :, :]
    d = d * d
    d2 = (d[..., 0] + d[..., 1]) + d[..., 2]
    value = (d2.min(2).astype(np.float64).sum() + d2.min(1).astype(np.float64).sum()) / (d2.shape[0] * (d2.shape[1] + d2.shape[2]))
    return d2.argmin(2), d2.argmin(1), value


def chamfer_scale(B, N, M, gval):
    return 2.0 * gval / (B * (N + M))


def chamfer_backward_reference(x, y, ix, iy, gval):
    """dict(gx, gy: float64 gradients; ax, ay: the float64 sums of |contributions| per entry; kx, ky: the number of
    contributions per point): every minimum (i, j) adds +-2 gval (x_i - y_j) / (B (N + M)) to x_i and y_j."""
    x64, y64 = np.asarray(x, np.float64), np.asarray(y, np.float64)
    B, N, _ = x64.shape
    M = y64.shape[1]
    sc = chamfer_scale(B, N, M, gval)
    r = {k: np.zeros_like(x64 if k[1] == "x" else y64) for k in ("gx", "gy", "ax", "ay")}
    r["kx"], r["ky"] = np.zeros((B, N), np.int64), np.zeros((B, M), np.int64)
    for b in range(B):
        pi = np.concatenate([np.arange(N), iy[b]])
        pj = np.concatenate([ix[b], np.arange(M)])
        c = (x64[b, pi] - y64[b, pj]) * sc
        np.add.at(r["gx"][b], pi, c)
        np.add.at(r["gy"][b], pj, -c)
        np.add.at(r["ax"][b], pi, np.abs(c))
        np.add.at(r["ay"][b], pj, np.abs(c))
        np.add.at(r["kx"][b], pi, 1)
        np.add.at(r["ky"][b], pj, 1)
    return r
