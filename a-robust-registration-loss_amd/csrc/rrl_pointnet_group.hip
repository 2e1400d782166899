// rrl_pointnet_group.hip -- the grouped PointNet: shared layers Conv2d(., ., 1) + GroupNorm + ReLU over every (point, neighbour
// slot) position and the max over each point's S slots (RPM's FeatExtractionEarlyFusion.prepool and its torch.max(., 2),
// rpm/models/feature_nets.py:118-131, 196-199), rrl_pointnet_group_fwd and rrl_pointnet_group_bwd (include/rrl.h, DESIGN.md
// section 25).  The rule is stated in the header; this file is its device side.  The unit is self-contained: it restates
// rrl_pointnet.hip's layer kernel for positions instead of sharing it through a header, so that unit's code object is untouched.
//
// Forward: pg_layer_kernel + pg_finish_kernel per layer, then pg_out_kernel.
// pg_layer_kernel is rrl_pointnet.hip's pn_layer_kernel over the P = N S positions (the same tile mapping, the same staging, the
// same chain), with two differences.  (1) A chunk is floor(128 / S) WHOLE points, CH = floor(128 / S) S <= 128 positions, so a
// point's slots never leave a workgroup; a chunk's last 32-position tile may reach beyond the chunk, and those lanes take no part.
// (2) The last layer keeps, per (channel, point), the extremum of z = y (gamma >= 0) or -y (gamma < 0) over the point's slots and
// its lowest slot: within a tile a segmented inclusive scan over the 32 lanes that hold the positions (the segment of a lane is
// its point; five shuffle steps at most), the open segment of a tile is carried into the next one, and the lane that holds a
// point's last slot writes ext and arg.  y_L is never stored.
// pg_finish_kernel, grid (B): a channel's chunk partials (lane i of a wavefront the chunks i, i + 64, ..., one fixed tree), then
// per group mu, r and the channels' a and d, as rrl_pointnet.hip.  pg_out_kernel: out = float32(max(0, double(ext) a + d)).
#include <cstddef>
#include <cstdint>
#include <cmath>

#include "rrl_common.h"
#include "rrl_wave_sum_d.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

#define PG_APITCH 68       // floats per row of the weights in LDS (64 steps + 4)
#define PG_MAX_N (1 << 20)
#define PG_MAX_P (1 << 22)
#define PG_MAX_K 1024
#define PG_OCHUNK 1024     // positions per workgroup of the backward's position sums

struct PgArgs {
    int B, N, S, P;           // points, slots, positions P = N S
    int CH, NC;               // positions per chunk, chunks
    int cin, cout, G;
    int first, last;
    double eps;
    const float *in;          // first: x [B][P][cin]; else y_{l-1} of every sample, in_stride floats apart
    size_t in_stride;
    const double *coef_in;
    size_t coef_stride;
    const float *W, *bias, *gamma, *beta;
    float *y;                 // hidden: y_l [cout][P] per sample
    size_t y_stride;
    double *part;             // [B][NC][cout][2]
    double *stat;
    size_t stat_stride;
    double *coef;
    int32_t *flag;
    float *ext, *out;         // last: [B][cout][N]
    int32_t *arg, *info;
};

__device__ __forceinline__ int pg_arow(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// the tile's operand [k][32 positions]: loads unconditional and in bounds (a row at or beyond cin repeats row cin - 1, a position
// at or beyond P position P - 1; the epilogue leaves such positions out); rows cin .. kpad - 1 are zero
template <int IT>
__device__ __forceinline__ void pg_load(const PgArgs &k, int b, int tid, int n0, float (&pre)[IT]) {
    const int q = tid & 31, n = min(n0 + q, k.P - 1);
#pragma unroll
    for (int i = 0; i < IT; ++i) {
        const int kk = min((tid >> 5) + 8 * i, k.cin - 1);
        pre[i] = k.first ? k.in[((size_t)b * k.P + n) * k.cin + kk] : k.in[(size_t)b * k.in_stride + (size_t)kk * k.P + n];
    }
}
template <int IT>
__device__ __forceinline__ void pg_store(const PgArgs &k, int tid, int kpad, const double *__restrict__ cf, const float (&pre)[IT], float *__restrict__ dst) {
    const int q = tid & 31;
#pragma unroll
    for (int i = 0; i < IT; ++i) {
        const int kk = (tid >> 5) + 8 * i;
        if (kk < kpad) {
            float v = 0.f;
            if (kk < k.cin) {
                v = pre[i];
                if (!k.first) {
                    const double t = (double)v * cf[2 * kk] + cf[2 * kk + 1];
                    v = (float)(t < 0.0 ? 0.0 : t);
                }
            }
            dst[kk * 32 + q] = v;
        }
    }
}

template <int ST, bool LAST>
__global__ __launch_bounds__(512) void pg_layer_kernel(const PgArgs k) {
    __shared__ float hs[2][2][128 * 32];
    __shared__ __attribute__((aligned(16))) float as[ST > 0 ? 4 * 64 * PG_APITCH : 4];
    __shared__ double cf[2 * 128];
    __shared__ float bsh[128];
    const int b = blockIdx.z, grp = threadIdx.x >> 8, tid = threadIdx.x & 255, w = tid >> 6, lane = tid & 63, h = lane >> 5, q = lane & 31;
    const int chunk = 2 * blockIdx.x + grp, cbase = blockIdx.y * 128, c0 = cbase + w * 32;
    const bool active = c0 < k.cout && chunk < k.NC;  // (wavefront-uniform)
    const int kpad = (k.cin + 7) & ~7, steps = (k.cin + 1) >> 1;
    if (!k.first) {
        for (int i = threadIdx.x; i < 2 * k.cin; i += 512) cf[i] = k.coef_in[(size_t)b * k.coef_stride * 2 + i];
    }
    if (ST > 0) {
        for (int i0 = threadIdx.x; i0 < 128 * kpad; i0 += 512 * 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = min(i0 + 512 * u, 128 * kpad - 1), cl = i / kpad, kk = i - cl * kpad;
                v[u] = k.W[(size_t)min(cbase + cl, k.cout - 1) * k.cin + min(kk, k.cin - 1)];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = i0 + 512 * u, cl = i / kpad, kk = i - cl * kpad;
                if (i < 128 * kpad)
                    as[((cl >> 5) * 64 + (cl & 31) * 2 + (kk & 1)) * PG_APITCH + (kk >> 1)] = (cbase + cl < k.cout && kk < k.cin) ? v[u] : 0.f;
            }
        }
    }
    unsigned neg = 0;  // bit r: the channel of accumulator r has gamma < 0 and pools its minimum (z = -y)
    if (threadIdx.x < 128) bsh[threadIdx.x] = k.bias[min(cbase + (int)threadIdx.x, k.cout - 1)];
    if (LAST) {
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (k.gamma[min(c0 + pg_arow(r, h), k.cout - 1)] < 0.f) neg |= 1u << r;
    }
    // last layer: the scanned (z, slot) of a tile's lane 31 per (wavefront, channel), the open point's carry into the next tile
    __shared__ float czs[LAST ? 8 * 32 : 1];
    __shared__ int cis[LAST ? 8 * 32 : 1];
    const int cslot = (int)(threadIdx.x >> 6) * 32;
    double sy[16], syy[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        sy[r] = 0.0;
        syy[r] = 0.0;
    }
    const long long beg = (long long)chunk * k.CH;
    const int nbeg = (int)(beg < (long long)k.P ? beg : (long long)k.P), nend = min(k.P, nbeg + k.CH);  // (nend <= nbeg: a group without a chunk)
    const int dmax = min(k.S, 32);          // scan steps d < dmax: no segment of a tile is longer
    const bool carry = (32 % k.S) != 0;     // a point can straddle two tiles
    constexpr int IT = ST > 0 ? ST / 4 : 8;
    float pre[IT];
    if (nbeg < nend) pg_load<IT>(k, b, tid, nbeg, pre);
    __syncthreads();
    if (nbeg < nend) pg_store<IT>(k, tid, kpad, cf, pre, hs[0][grp]);
    __syncthreads();
#pragma unroll 1
    for (int t = 0; t < 4; ++t) {  // CH <= 128: four tiles at most; the same count for both groups (the barrier is the workgroup's)
        const int n0 = nbeg + 32 * t;
        const bool more = n0 + 32 < nend;
        if (more) pg_load<IT>(k, b, tid, n0 + 32, pre);
        if (active && n0 < nend) {
            const float *hb = hs[t & 1][grp];
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = bsh[w * 32 + pg_arow(r, h)];
            if (ST > 0) {
                const float *ap = as + (w * 64 + q * 2 + h) * PG_APITCH;
#pragma unroll 2
                for (int s4 = 0; s4 < ST / 4; ++s4) {
                    if (4 * s4 < steps) {
                        const float4 av = *(const float4 *)(ap + 4 * s4);
                        const float a4[4] = {av.x, av.y, av.z, av.w};
                        float b4[4];
#pragma unroll
                        for (int u = 0; u < 4; ++u) b4[u] = hb[(2 * (4 * s4 + u) + h) * 32 + q];
#pragma unroll
                        for (int u = 0; u < 4; ++u)
                            if (4 * s4 + u < steps) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[u], b4[u], acc, 0, 0, 0);
                    }
                }
            } else {
#pragma unroll 1
                for (int kk = 0; kk < k.cin; ++kk) {
                    const float hv = hb[kk * 32 + q];
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        acc[r] = __builtin_fmaf(k.W[(size_t)min(c0 + pg_arow(r, h), k.cout - 1) * k.cin + kk], hv, acc[r]);
                }
            }
            const int n = n0 + q;
            const bool valid = n < nend;
            if (valid) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float v = acc[r];
                    const double vd = (double)v;
                    sy[r] += vd;
                    syy[r] += vd * vd;
                    if (!LAST && c0 + pg_arow(r, h) < k.cout) k.y[(size_t)b * k.y_stride + (size_t)(c0 + pg_arow(r, h)) * k.P + n] = v;
                }
            }
            if (LAST) {
                // every lane of the wavefront takes part in the shuffles; a lane beyond the chunk holds -inf and ends no point
                const int pt = n / k.S, slot = n - pt * k.S, reach = min(slot, q);  // reach: the lanes below that hold lower slots of this point
                const bool open = carry && q == 0 && slot > 0 && t > 0;             // the point began in the previous tile
                const bool ends = valid && slot == k.S - 1;
                float *eb = k.ext + ((size_t)b * k.cout + c0 + 4 * h) * k.N + pt;     // channel c0 + pg_arow(0, h) of the lane's point
                int32_t *ab = k.arg + ((size_t)b * k.cout + c0 + 4 * h) * k.N + pt;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float z = valid ? ((neg >> r) & 1u ? -acc[r] : acc[r]) : -INFINITY;
                    int iz = slot;
                    if (open) {  // (written by lane 31 before the previous tile's barrier)
                        const float pz = czs[cslot + pg_arow(r, h)];
                        if (pz >= z) {  // a tie keeps the lower slot, the carried one
                            z = pz;
                            iz = cis[cslot + pg_arow(r, h)];
                        }
                    }
#pragma unroll
                    for (int d = 1; d < 32; d <<= 1) {
                        if (d < dmax) {  // (uniform)
                            const float oz = __shfl_up(z, (unsigned)d, 32);
                            const int oi = __shfl_up(iz, (unsigned)d, 32);
                            if (d <= reach && oz >= z) {  // the lower lanes' best: lower slots, so a tie goes to them
                                z = oz;
                                iz = oi;
                            }
                        }
                    }
                    if (carry && q == 31) {
                        czs[cslot + pg_arow(r, h)] = z;
                        cis[cslot + pg_arow(r, h)] = iz;
                    }
                    if (ends && c0 + pg_arow(r, h) < k.cout) {
                        const int o = pg_arow(r, 0) * k.N;  // (< 28 * 2^20; one base per tile: sixteen 64-bit addresses do not fit the registers)
                        eb[o] = (neg >> r) & 1u ? -z : z;
                        ab[o] = iz;
                    }
                    __builtin_amdgcn_sched_barrier(0);  // one row's scan at a time: the kernel sits at the register limit, the rows' temporaries are not to pile up
                }
            }
        }
        if (more) pg_store<IT>(k, tid, kpad, cf, pre, hs[(t + 1) & 1][grp]);
        __syncthreads();
    }
    if (!active) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
#pragma unroll
        for (int m = 16; m >= 1; m >>= 1) {
            sy[r] += __shfl_xor(sy[r], m);
            syy[r] += __shfl_xor(syy[r], m);
        }
        if (q == 0 && c0 + pg_arow(r, h) < k.cout) {
            const size_t o = ((size_t)b * k.NC + chunk) * k.cout + c0 + pg_arow(r, h);
            k.part[2 * o] = sy[r];
            k.part[2 * o + 1] = syy[r];
        }
    }
}

__global__ __launch_bounds__(256) void pg_finish_kernel(const PgArgs k) {
    const int b = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int cpg = k.cout / k.G;
    const double m = (double)cpg * (double)k.P;
    double *stat = k.stat + (size_t)b * k.stat_stride * 4, *coef = k.coef + (size_t)b * k.coef_stride * 2;
    int bad = k.first ? 0 : k.flag[b];
    // a channel's chunks: lane i the chunks i, i + 64, ... ascending, then one fixed tree; parked in the channel's coef slot
    for (int c = w; c < k.cout; c += 4) {  // (wavefront-uniform)
        double s = 0.0, ss = 0.0;
        for (int p = lane; p < k.NC; p += 64) {
            const double2 pp = *(const double2 *)(k.part + 2 * (((size_t)b * k.NC + p) * k.cout + c));
            s += pp.x;
            ss += pp.y;
        }
        s = wave_sum_d(s);
        ss = wave_sum_d(ss);
        if (lane == 0) {
            coef[2 * c] = s;
            coef[2 * c + 1] = ss;
        }
    }
    __syncthreads();
    for (int g = w; g < k.G; g += 4) {  // (wavefront-uniform)
        double s = 0.0, ss = 0.0;
        for (int c = g * cpg + lane; c < (g + 1) * cpg; c += 64) {
            s += coef[2 * c];
            ss += coef[2 * c + 1];
        }
        s = wave_sum_d(s);
        ss = wave_sum_d(ss);
        const double mu = s / m, e2 = ss / m, d = e2 - mu * mu;
        const double var = d > 0.0 ? d : 0.0;
        const double r = 1.0 / sqrt(var + k.eps);
        bad |= !(fabs(s) < INFINITY) || !(fabs(ss) < INFINITY);
        if (lane == 0) {
            stat[4 * g] = s;
            stat[4 * g + 1] = ss;
            stat[4 * g + 2] = mu;
            stat[4 * g + 3] = r;
        }
        for (int c = g * cpg + lane; c < (g + 1) * cpg; c += 64) {
            const double ac = (double)k.gamma[c] * r;
            const double dc = (double)k.beta[c] - mu * ac;
            coef[2 * c] = ac;
            coef[2 * c + 1] = dc;
            bad |= !(fabs(ac) < INFINITY) || !(fabs(dc) < INFINITY);
        }
    }
    bad = __syncthreads_or(bad);
    if (k.last && k.info && threadIdx.x == 0) k.info[b] = bad ? 1 : 0;
    if (threadIdx.x == 0) k.flag[b] = bad ? 1 : 0;
}

// out[b][c][n] = float32(max(0, double(ext) a_c + d_c)), NaN for a flagged sample
__global__ __launch_bounds__(256) void pg_out_kernel(const PgArgs k) {
    const int b = blockIdx.y;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)k.cout * k.N) return;
    const int c = (int)(idx / k.N);
    const double *cf = k.coef + ((size_t)b * k.coef_stride + c) * 2;
    const size_t o = (size_t)b * k.cout * k.N + (size_t)idx;
    const double t = (double)k.ext[o] * cf[0] + cf[1];
    k.out[o] = k.flag[b] ? NAN : (float)(t < 0.0 ? 0.0 : t);
}

// ---- host ------------------------------------------------------------------------------------------------------------
struct PgLayout {
    size_t off[RRL_PG_FIELDS];
    size_t bytes;
    size_t ctot, gtot, hid;
    size_t coff[RRL_PN_MAX_LAYERS], goff[RRL_PN_MAX_LAYERS], yoff[RRL_PN_MAX_LAYERS];
    int P, CH, NC;
};

static bool pg_shape(int B, int N, int S, int c0, int L, const int32_t *widths, const int32_t *groups, PgLayout &lo) {
    if (B < 0 || B > 65535 || N < 1 || N > PG_MAX_N || S < 1 || S > RRL_PG_MAX_S || (long long)N * S > PG_MAX_P || c0 < 1 ||
        c0 > RRL_PG_MAX_C0 || L < 2 || L > RRL_PN_MAX_LAYERS || !widths || !groups)
        return false;
    lo = {};
    lo.P = N * S;
    for (int l = 0; l < L; ++l) {
        const int c = widths[l], g = groups[l];
        if (c < 1 || g < 1 || c % g != 0 || c > (l + 1 < L ? RRL_PN_MAX_HIDDEN : RRL_PG_MAX_K)) return false;
        lo.coff[l] = lo.ctot;
        lo.goff[l] = lo.gtot;
        lo.yoff[l] = lo.hid * (size_t)lo.P;
        lo.ctot += (size_t)c;
        lo.gtot += (size_t)g;
        if (l + 1 < L) lo.hid += (size_t)c;
    }
    const int ppc = 128 / S;
    lo.CH = ppc * S;
    lo.NC = (N + ppc - 1) / ppc;
    const size_t K = (size_t)widths[L - 1], Bz = (size_t)B;
    size_t o = 0;
    lo.off[RRL_PG_STAT] = o;  o += Bz * lo.gtot * 4 * sizeof(double);
    lo.off[RRL_PG_COEF] = o;  o += Bz * lo.ctot * 2 * sizeof(double);
    lo.off[RRL_PG_PART] = o;  o += Bz * lo.NC * lo.ctot * 2 * sizeof(double);
    lo.off[RRL_PG_EXT] = o;   o += Bz * K * (size_t)N * sizeof(float);
    lo.off[RRL_PG_FLAG] = o;  o += Bz * sizeof(int32_t);
    lo.off[RRL_PG_Y] = o;     o += Bz * lo.hid * (size_t)lo.P * sizeof(float);
    lo.bytes = o;
    return true;
}

extern "C" size_t rrl_pointnet_group_workspace_bytes(int B, int N, int S, int c0, int L, const int32_t *widths, const int32_t *groups,
                                                     size_t *offsets) {
    PgLayout lo;
    if (!pg_shape(B, N, S, c0, L, widths, groups, lo)) return 0;
    if (offsets)
        for (int f = 0; f < RRL_PG_FIELDS; ++f) offsets[f] = lo.off[f];
    return lo.bytes;
}

template <bool LAST>
static void pg_launch(const PgArgs &k, hipStream_t st) {
    const dim3 grid((unsigned)((k.NC + 1) / 2), (unsigned)((k.cout + 127) / 128), (unsigned)k.B);
    if (k.cin < 64) hipLaunchKernelGGL((pg_layer_kernel<0, LAST>), grid, dim3(512), 0, st, k);
    else if (k.cin <= 64) hipLaunchKernelGGL((pg_layer_kernel<32, LAST>), grid, dim3(512), 0, st, k);
    else hipLaunchKernelGGL((pg_layer_kernel<64, LAST>), grid, dim3(512), 0, st, k);
    hipLaunchKernelGGL(pg_finish_kernel, dim3((unsigned)k.B), dim3(256), 0, st, k);
}

extern "C" int rrl_pointnet_group_fwd(const float *x, const float **params, const int32_t *widths, const int32_t *groups, double eps,
                                      void *ws, size_t ws_bytes, float *out, int32_t *arg, int32_t *info, int B, int N, int S, int c0,
                                      int L, void *stream) {
    PgLayout lo;
    if (!x || !params || !ws || !out || !arg || !(eps > 0.0) || !pg_shape(B, N, S, c0, L, widths, groups, lo)) return RRL_E_ARG;
    for (int i = 0; i < 4 * L; ++i)
        if (!params[i]) return RRL_E_ARG;
    if ((((uintptr_t)ws) & 15) != 0 || ws_bytes < lo.bytes) return RRL_E_WS;
    if (B == 0) return 0;
    char *base = (char *)ws;
    hipStream_t st = (hipStream_t)stream;
    for (int l = 0; l < L; ++l) {
        PgArgs k = {};
        k.B = B; k.N = N; k.S = S; k.P = lo.P; k.CH = lo.CH; k.NC = lo.NC;
        k.cin = l ? widths[l - 1] : c0; k.cout = widths[l]; k.G = groups[l];
        k.first = l == 0; k.last = l == L - 1;
        k.eps = eps;
        k.in = l ? (const float *)(base + lo.off[RRL_PG_Y]) + lo.yoff[l - 1] : x;
        k.in_stride = lo.hid * (size_t)lo.P;
        k.coef_stride = lo.ctot;
        k.coef_in = l ? (const double *)(base + lo.off[RRL_PG_COEF]) + 2 * lo.coff[l - 1] : nullptr;
        k.W = params[4 * l]; k.bias = params[4 * l + 1]; k.gamma = params[4 * l + 2]; k.beta = params[4 * l + 3];
        k.y = (float *)(base + lo.off[RRL_PG_Y]) + lo.yoff[l];
        k.y_stride = lo.hid * (size_t)lo.P;
        k.part = (double *)(base + lo.off[RRL_PG_PART]) + 2 * (size_t)B * lo.NC * lo.coff[l];
        k.stat = (double *)(base + lo.off[RRL_PG_STAT]) + 4 * lo.goff[l];
        k.stat_stride = lo.gtot;
        k.coef = (double *)(base + lo.off[RRL_PG_COEF]) + 2 * lo.coff[l];
        k.flag = (int32_t *)(base + lo.off[RRL_PG_FLAG]);
        k.ext = (float *)(base + lo.off[RRL_PG_EXT]);
        k.out = out; k.arg = arg; k.info = info;
        if (k.last) {
            pg_launch<true>(k, st);
            hipLaunchKernelGGL(pg_out_kernel, dim3((unsigned)(((long long)k.cout * N + 255) / 256), (unsigned)B), dim3(256), 0, st, k);
        } else {
            pg_launch<false>(k, st);
        }
    }
    RRL_LAUNCH_CHECK();
    return 0;
}

// ---- backward: rrl_pointnet_group_bwd ----------------------------------------------------------------------------------------
// Double arithmetic on what the forward kept, one rounding per output, no atomics.  The position-summed products -- S1 and the
// Gram matrix S2 of h_{L-1}, every hidden dW and db -- are pg_outer: a workgroup takes PG_OCHUNK positions of one sample, stages
// both operands in LDS 32 positions at a time, every thread owns an 8 x 9 register tile of the outputs; the chunk's partial goes
// to bws, and pg_outer_merge adds the partials (sample after sample, chunk after chunk).  The per-position products -- M h and
// W^T dy -- are pg_apply: a workgroup takes 64 positions, stages the operand's columns in LDS, a wavefront owns every fourth
// output row and reads the matrix through wavefront-uniform loads.  The last layer's sparse term is pg_sparse_gate: one wavefront
// per (point, 64 rows of h) holds the point's S columns of dh in LDS and walks the K channels ascending.

struct PgIn {  // an operand h[row][p] of sample b: x (first) or the activation of a kept y with its a, d
    const float *src;
    size_t stride;
    const double *coef;
    size_t coef_stride;
    int first, rows;
};
__device__ __forceinline__ double pg_in(const PgIn &I, int b, int P, int row, int p) {
    if (I.first) return (double)I.src[((size_t)b * P + p) * I.rows + row];
    const double *cf = I.coef + ((size_t)b * I.coef_stride + row) * 2;
    const double t = (double)I.src[(size_t)b * I.stride + (size_t)row * P + p] * cf[0] + cf[1];
    return (double)(float)(t < 0.0 ? 0.0 : t);
}
__device__ __forceinline__ double pg_gate(double h, double v) { return h > 0.0 ? v : (h != h ? h : 0.0); }

struct PgB {
    int B, N, S, P, OC;     // OC: chunks of PG_OCHUNK positions
    int K, H, G;            // the last layer: K channels of H inputs in G groups
    int c, cin;             // the layer in work (pg_outer: the rows of X and of Z)
    PgIn in;                // the input operand h_{l-1} of the layer in work
    const float *W, *bias, *gamma;
    const float *y;
    size_t y_stride;
    const double *stat;
    size_t stat_stride;
    const double *coef;
    size_t coef_stride;
    const float *ext, *g;
    const int32_t *arg, *flag;
    double *dgl, *ab, *s2, *M, *dgb, *pq, *rp, *op, *din, *dout;
    size_t dstride;
    int x_is_in;            // pg_outer: X is the operand itself (the Gram matrix) instead of din
    int per_sample;         // pg_outer_merge: one result per sample (s2) or the sum over the batch (dW, db)
    int to_x;               // pg_apply: write d_x [B][P][cin] instead of the gated buffer
    float *dW, *db, *dgamma, *dbeta, *dx;
};

// s_{c,n} = g_out[c][n] [out[c][n] > 0] (NaN for a flagged sample)
__device__ __forceinline__ double pg_s(const PgB &k, int b, int c, int n, double a, double d, float *e_out) {
    const size_t o = ((size_t)b * k.K + c) * k.N + n;
    const float e = k.ext[o];
    *e_out = e;
    const double t = (double)e * a + d;
    const float f = (float)(t < 0.0 ? 0.0 : t);
    return k.flag[b] ? (double)NAN : (f > 0.f ? (double)k.g[o] : 0.0);
}

// per (sample, channel): dgl = (sum_n s x, sum_n s), lane i the points i, i + 64, ... and one fixed tree; then per group A_g, B_g
__global__ __launch_bounds__(256) void pg_bl_prep(const PgB k) {
    const int b = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63, cpg = k.K / k.G;
    const double m = (double)cpg * (double)k.P;
    for (int c = w; c < k.K; c += 4) {  // (wavefront-uniform)
        const double *st = k.stat + ((size_t)b * k.stat_stride + c / cpg) * 4, *cf = k.coef + ((size_t)b * k.coef_stride + c) * 2;
        double sx = 0.0, ss = 0.0;
        for (int n = lane; n < k.N; n += 64) {
            float e;
            const double s = pg_s(k, b, c, n, cf[0], cf[1], &e);
            sx += s * (((double)e - st[2]) * st[3]);
            ss += s;
        }
        sx = wave_sum_d(sx);
        ss = wave_sum_d(ss);
        if (lane == 0) {
            k.dgl[((size_t)b * k.K + c) * 2] = sx;
            k.dgl[((size_t)b * k.K + c) * 2 + 1] = ss;
        }
    }
    __syncthreads();
    for (int g = threadIdx.x; g < k.G; g += 256) {
        const double *st = k.stat + ((size_t)b * k.stat_stride + g) * 4;
        double Ps = 0.0, Q = 0.0;
        for (int c = g * cpg; c < (g + 1) * cpg; ++c) {
            const double gm = (double)k.gamma[c];
            Q += gm * k.dgl[((size_t)b * k.K + c) * 2];
            Ps += gm * k.dgl[((size_t)b * k.K + c) * 2 + 1];
        }
        const double r = st[3], mu = st[2];
        k.ab[((size_t)b * k.G + g) * 2] = -r * Ps / m + r * r * Q * mu / m;
        k.ab[((size_t)b * k.G + g) * 2 + 1] = -r * r * Q / m;
    }
}

// op[b][chunk][i][j] = sum over the chunk's positions of X[i][p] Z[j][p], i < c, j <= cin, Z[cin] = 1; X = din or the operand.
// 256 threads as 16 x 16; thread (ti, tj) owns i = ti + 16 u (u < 8), j = tj + 16 v (v < 9); positions ascending.
#define PG_OP 33  // doubles per row of a staged operand (32 positions + 1: neighbouring rows two banks apart)
__global__ __launch_bounds__(256) void pg_outer(const PgB k) {
    __shared__ double Xs[128 * PG_OP], Zs[144 * PG_OP];
    const int b = blockIdx.y, chunk = blockIdx.x, ti = threadIdx.x & 15, tj = threadIdx.x >> 4, cz = k.cin + 1;
    const int nu = (k.c + 15) >> 4, nv = (cz + 15) >> 4;
    const int pbeg = chunk * PG_OCHUNK, pend = min(k.P, pbeg + PG_OCHUNK);
    double acc[8][9];
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int v = 0; v < 9; ++v) acc[u][v] = 0.0;
    const int q = threadIdx.x & 31, r0 = threadIdx.x >> 5;
#pragma unroll 1
    for (int p0 = pbeg; p0 < pend; p0 += 32) {
        const int p = p0 + q;
        const bool in = p < pend;
        const int pc = min(p, pend - 1);
        for (int row = r0; row < 16 * nu; row += 8) {
            double v = 0.0;
            if (in && row < k.c) v = k.x_is_in ? pg_in(k.in, b, k.P, row, pc) : k.din[(size_t)b * k.dstride + (size_t)row * k.P + pc];
            Xs[row * PG_OP + q] = v;
        }
        for (int row = r0; row < 16 * nv; row += 8) {
            double v = 0.0;
            if (in && row <= k.cin) v = row < k.cin ? pg_in(k.in, b, k.P, row, pc) : 1.0;
            Zs[row * PG_OP + q] = v;
        }
        __syncthreads();
#pragma unroll 2
        for (int pp = 0; pp < 32; ++pp) {
            double xv[8], zv[9];
#pragma unroll
            for (int u = 0; u < 8; ++u) xv[u] = u < nu ? Xs[(ti + 16 * u) * PG_OP + pp] : 0.0;
#pragma unroll
            for (int v = 0; v < 9; ++v) zv[v] = v < nv ? Zs[(tj + 16 * v) * PG_OP + pp] : 0.0;
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (u < nu) {
#pragma unroll
                    for (int v = 0; v < 9; ++v)
                        if (v < nv) acc[u][v] = __builtin_fma(xv[u], zv[v], acc[u][v]);
                }
        }
        __syncthreads();
    }
    double *o = k.op + ((size_t)b * k.OC + chunk) * (size_t)k.c * cz;
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int v = 0; v < 9; ++v) {
            const int i = ti + 16 * u, j = tj + 16 * v;
            if (i < k.c && j < cz) o[(size_t)i * cz + j] = acc[u][v];
        }
}

// the partials of pg_outer, chunk after chunk (and sample after sample unless per_sample): s2[b][i][j], or dW / db
__global__ __launch_bounds__(256) void pg_outer_merge(const PgB k) {
    const int cz = k.cin + 1, idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= k.c * cz) return;
    const int b0 = k.per_sample ? blockIdx.y : 0, b1 = k.per_sample ? b0 + 1 : k.B;
    double acc = 0.0;
    for (int b = b0; b < b1; ++b)
        for (int ch = 0; ch < k.OC; ++ch) acc += k.op[((size_t)b * k.OC + ch) * (size_t)k.c * cz + idx];
    const int i = idx / cz, j = idx - i * cz;
    if (k.per_sample) k.s2[(size_t)b0 * k.c * cz + idx] = acc;
    else if (j < k.cin) {
        if (k.dW) k.dW[(size_t)i * k.cin + j] = (float)acc;
    } else if (k.db) k.db[i] = (float)acc;
}

// M[k][j] = sum_c B_g W[c][k] W[c][j] (j < H) and M[k][H] = sum_c (A_g + B_g b_c) W[c][k], c ascending; stored as [j][k]
__global__ __launch_bounds__(256) void pg_bl_M(const PgB k) {
    const int b = blockIdx.y, hz = k.H + 1, idx = blockIdx.x * 256 + threadIdx.x, cpg = k.K / k.G;
    if (idx >= k.H * hz) return;
    const int kk = idx / hz, j = idx - kk * hz;
    double acc = 0.0;
    for (int c = 0; c < k.K; ++c) {
        const double *ab = k.ab + ((size_t)b * k.G + c / cpg) * 2;
        const double w = (double)k.W[(size_t)c * k.H + kk];
        acc += j < k.H ? ab[1] * w * (double)k.W[(size_t)c * k.H + j] : (ab[0] + ab[1] * (double)k.bias[c]) * w;
    }
    k.M[((size_t)b * hz + j) * k.H + kk] = acc;  // transposed: pg_apply reads a column of M per step
}

// out[kk][p] = sum_j A[kk][j] X[j][p] (j ascending), kk < nk, 64 positions per workgroup, one position per lane; wavefront w owns
// the rows kk = w + 4 u, u < NU (NU: nk / 4 rounded up to 8, 16, 24 or 32; a row at or beyond nk repeats row nk - 1 and is not
// written).  The matrix arrives through wavefront-uniform loads, NU unconditional ones per step, all in flight together.
// MODE_W = false: A = M[b], kept transposed ([H + 1][H]: row j holds M[.][j], row H the vector v added at the end), X = the operand
// h_{L-1}; written ungated (pg_sparse_gate follows).  MODE_W = true: A[kk][j] = W[j][kk], X = din = dy of the layer; written
// gated by h_{l-1} > 0, or as d_x.
template <int NU, bool MODE_W>
__global__ __launch_bounds__(256) void pg_apply(const PgB k) {
    __shared__ double Xs[128 * 64];
    const int b = blockIdx.y, q = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int p0 = blockIdx.x * 64, p = min(p0 + q, k.P - 1);
    const int nj = MODE_W ? k.c : k.H, nk = MODE_W ? k.cin : k.H;
    for (int j = w; j < nj; j += 4)
        Xs[j * 64 + q] = MODE_W ? k.din[(size_t)b * k.dstride + (size_t)j * k.P + p] : pg_in(k.in, b, k.P, j, p);
    __syncthreads();
    double acc[NU];
    int off[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        acc[u] = 0.0;
        off[u] = min(w + 4 * u, nk - 1);
    }
    const double *Mt = k.M + (size_t)b * k.H * (k.H + 1);
#pragma unroll 1
    for (int j = 0; j < nj; ++j) {
        const double xv = Xs[j * 64 + q];
        double a[NU];
#pragma unroll
        for (int u = 0; u < NU; ++u) a[u] = MODE_W ? (double)k.W[(size_t)j * nk + off[u]] : Mt[(size_t)j * nk + off[u]];
#pragma unroll
        for (int u = 0; u < NU; ++u) acc[u] = __builtin_fma(a[u], xv, acc[u]);
    }
    if (p0 + q >= k.P) return;
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const int kk = w + 4 * u;
        if (kk < nk) {
            if (!MODE_W) k.dout[(size_t)b * k.dstride + (size_t)kk * k.P + p] = acc[u] + Mt[(size_t)k.H * k.H + kk];
            else if (k.to_x) k.dx[((size_t)b * k.P + p) * k.cin + kk] = (float)acc[u];
            else k.dout[(size_t)b * k.dstride + (size_t)kk * k.P + p] = pg_gate(pg_in(k.in, b, k.P, kk, p), acc[u]);
        }
    }
}
template <bool MODE_W>
static void pg_apply_launch(const PgB &k, int nk, hipStream_t st) {
    const dim3 grid((unsigned)((k.P + 63) / 64), (unsigned)k.B);
    if (nk <= 32) hipLaunchKernelGGL((pg_apply<8, MODE_W>), grid, dim3(256), 0, st, k);
    else if (nk <= 64) hipLaunchKernelGGL((pg_apply<16, MODE_W>), grid, dim3(256), 0, st, k);
    else if (nk <= 96) hipLaunchKernelGGL((pg_apply<24, MODE_W>), grid, dim3(256), 0, st, k);
    else hipLaunchKernelGGL((pg_apply<32, MODE_W>), grid, dim3(256), 0, st, k);
}

// dh_{L-1}[kk][n S + arg[c][n]] += t_{c,n} W_L[c][kk], c ascending, then the gate h_{L-1} > 0: one wavefront per (point, 64 rows)
template <int SP>
__global__ __launch_bounds__(64) void pg_sparse_gate(const PgB k) {
    __shared__ double tile[64 * SP];
    const int n = blockIdx.x, k0 = blockIdx.y * 64, b = blockIdx.z, lane = threadIdx.x, cpg = k.K / k.G;
    const int rows = min(64, k.H - k0);
    double *base = k.dout + (size_t)b * k.dstride + (size_t)n * k.S;
    for (int i = lane; i < rows * k.S; i += 64) {
        const int r = i / k.S, s = i - r * k.S;
        tile[r * SP + s] = base[(size_t)(k0 + r) * k.P + s];
    }
    __syncthreads();
    if (lane < rows) {
#pragma unroll 1
        for (int c = 0; c < k.K; ++c) {
            const double *st = k.stat + ((size_t)b * k.stat_stride + c / cpg) * 4, *cf = k.coef + ((size_t)b * k.coef_stride + c) * 2;
            float e;
            const double s = pg_s(k, b, c, n, cf[0], cf[1], &e);
            const double t = st[3] * (double)k.gamma[c] * s;
            const int at = min(max(k.arg[((size_t)b * k.K + c) * k.N + n], 0), k.S - 1);
            tile[lane * SP + at] += t * (double)k.W[(size_t)c * k.H + k0 + lane];
        }
    }
    __syncthreads();
    for (int i = lane; i < rows * k.S; i += 64) {
        const int r = i / k.S, s = i - r * k.S;
        base[(size_t)(k0 + r) * k.P + s] = pg_gate(pg_in(k.in, b, k.P, k0 + r, n * k.S + s), tile[r * SP + s]);
    }
}

// dW_L[c][kk] (kk < H) and db_L[c] (kk = H, where h = 1 and S1 = P), summed over the batch b ascending; dgamma_L, dbeta_L.
// One wavefront per (c, kk): per sample the sparse sum (lane i the points i, i + 64, ...) and W_L[c] . S2[.][kk] (lane i the rows
// i, i + 64, ...), each by one fixed tree.
__global__ __launch_bounds__(256) void pg_bl_dW(const PgB k) {
    const int hz = k.H + 1, cpg = k.K / k.G, lane = threadIdx.x & 63;
    const long long wid = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wid >= (long long)k.K * hz) return;  // (wavefront-uniform)
    const int c = (int)(wid / hz), kk = (int)(wid - (long long)c * hz);
    const double bc = (double)k.bias[c], gm = (double)k.gamma[c];
    double acc = 0.0, dg = 0.0, dbt = 0.0;
    for (int b = 0; b < k.B; ++b) {
        const double *ab = k.ab + ((size_t)b * k.G + c / cpg) * 2, *S = k.s2 + (size_t)b * k.H * hz;
        const double *st = k.stat + ((size_t)b * k.stat_stride + c / cpg) * 4, *cf = k.coef + ((size_t)b * k.coef_stride + c) * 2;
        double sp = 0.0, dot = 0.0;
        for (int n = lane; n < k.N; n += 64) {
            float e;
            const double t = st[3] * gm * pg_s(k, b, c, n, cf[0], cf[1], &e);
            const int at = min(max(k.arg[((size_t)b * k.K + c) * k.N + n], 0), k.S - 1);
            sp += kk < k.H ? t * pg_in(k.in, b, k.P, kk, n * k.S + at) : t;
        }
        for (int j = lane; j < k.H; j += 64) dot += (double)k.W[(size_t)c * k.H + j] * S[(size_t)j * hz + kk];
        sp = wave_sum_d(sp);
        dot = wave_sum_d(dot);
        const double S1k = kk < k.H ? S[(size_t)kk * hz + k.H] : (double)k.P;
        acc += sp + ab[0] * S1k + ab[1] * (dot + bc * S1k);
        dg += k.dgl[((size_t)b * k.K + c) * 2];
        dbt += k.dgl[((size_t)b * k.K + c) * 2 + 1];
    }
    if (lane != 0) return;
    if (kk < k.H) {
        if (k.dW) k.dW[(size_t)c * k.H + kk] = (float)acc;
    } else {
        if (k.db) k.db[c] = (float)acc;
        if (k.dgamma) k.dgamma[c] = (float)dg;
        if (k.dbeta) k.dbeta[c] = (float)dbt;
    }
}

// a hidden layer: rp[b][chunk][ch] = (sum dout xhat, sum dout) over the chunk's positions; one wavefront per channel, lane i the
// positions i, i + 64, ... of the chunk, one fixed tree
__global__ __launch_bounds__(256) void pg_bh_reduce(const PgB k) {
    const int chunk = blockIdx.x, b = blockIdx.z, ch = blockIdx.y * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, cpg = k.c / k.G;
    if (ch >= k.c) return;  // (wavefront-uniform)
    const double *st = k.stat + ((size_t)b * k.stat_stride + ch / cpg) * 4;
    const int pbeg = chunk * PG_OCHUNK, pend = min(k.P, pbeg + PG_OCHUNK);
    double sg = 0.0, sb = 0.0;
    for (int p = pbeg + lane; p < pend; p += 64) {
        const double dv = k.din[(size_t)b * k.dstride + (size_t)ch * k.P + p];
        sg += dv * (((double)k.y[(size_t)b * k.y_stride + (size_t)ch * k.P + p] - st[2]) * st[3]);
        sb += dv;
    }
    sg = wave_sum_d(sg);
    sb = wave_sum_d(sb);
    if (lane == 0) {
        double *o = k.rp + (((size_t)b * k.OC + chunk) * k.c + ch) * 2;
        o[0] = sg;
        o[1] = sb;
    }
}

// dgb[b][ch] = the chunks ascending; then per group P, Q over its channels ascending
__global__ __launch_bounds__(256) void pg_bh_merge(const PgB k) {
    const int b = blockIdx.x, cpg = k.c / k.G;
    for (int ch = threadIdx.x; ch < k.c; ch += 256) {
        double sg = 0.0, sb = 0.0;
        for (int q = 0; q < k.OC; ++q) {
            const double *o = k.rp + (((size_t)b * k.OC + q) * k.c + ch) * 2;
            sg += o[0];
            sb += o[1];
        }
        k.dgb[((size_t)b * k.c + ch) * 2] = sg;
        k.dgb[((size_t)b * k.c + ch) * 2 + 1] = sb;
    }
    __syncthreads();
    for (int g = threadIdx.x; g < k.G; g += 256) {
        double Ps = 0.0, Q = 0.0;
        for (int c = g * cpg; c < (g + 1) * cpg; ++c) {
            const double gm = (double)k.gamma[c];
            Ps += gm * k.dgb[((size_t)b * k.c + c) * 2 + 1];
            Q += gm * k.dgb[((size_t)b * k.c + c) * 2];
        }
        k.pq[((size_t)b * k.G + g) * 2] = Ps;
        k.pq[((size_t)b * k.G + g) * 2 + 1] = Q;
    }
}

// dgamma_l, dbeta_l of a hidden layer: the samples' sums, b ascending
__global__ __launch_bounds__(256) void pg_bh_params(const PgB k) {
    const int ch = blockIdx.x * 256 + threadIdx.x;
    if (ch >= k.c) return;
    double dg = 0.0, dbt = 0.0;
    for (int b = 0; b < k.B; ++b) {
        dg += k.dgb[((size_t)b * k.c + ch) * 2];
        dbt += k.dgb[((size_t)b * k.c + ch) * 2 + 1];
    }
    if (k.dgamma) k.dgamma[ch] = (float)dg;
    if (k.dbeta) k.dbeta[ch] = (float)dbt;
}

// dy = r (gamma dout - P / m - xhat Q / m) in place
__global__ __launch_bounds__(256) void pg_bh_apply(const PgB k) {
    const int b = blockIdx.y, cpg = k.c / k.G;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)k.c * k.P) return;
    const int ch = (int)(idx / k.P), p = (int)(idx - (long long)ch * k.P), g = ch / cpg;
    const double *st = k.stat + ((size_t)b * k.stat_stride + g) * 4, *pq = k.pq + ((size_t)b * k.G + g) * 2;
    const double m = (double)cpg * (double)k.P;
    double *d = k.din + (size_t)b * k.dstride + (size_t)ch * k.P + p;
    const double xh = ((double)k.y[(size_t)b * k.y_stride + (size_t)ch * k.P + p] - st[2]) * st[3];
    *d = st[3] * ((double)k.gamma[ch] * *d - pq[0] / m - xh * pq[1] / m);
}

struct PgBLayout {
    size_t dgl, ab, s2, M, dgb, pq, rp, op, d0, d1, doubles, dstride;
    int OC;
};
static void pg_blayout(int B, int N, int S, int c0, int L, const int32_t *widths, const int32_t *groups, PgBLayout &o) {
    const size_t Bz = (size_t)B, K = (size_t)widths[L - 1], H = (size_t)widths[L - 2], P = (size_t)N * S;
    size_t hmax = 0, gmax = 0, omax = H * (H + 1);
    for (int l = 0; l + 1 < L; ++l) {
        const size_t c = (size_t)widths[l], cin = l ? (size_t)widths[l - 1] : (size_t)c0;
        hmax = hmax > c ? hmax : c;
        gmax = gmax > (size_t)groups[l] ? gmax : (size_t)groups[l];
        omax = omax > c * (cin + 1) ? omax : c * (cin + 1);
    }
    o.OC = (int)((P + PG_OCHUNK - 1) / PG_OCHUNK);
    size_t at = 0;
    o.dgl = at; at += Bz * K * 2;
    o.ab = at;  at += Bz * (size_t)groups[L - 1] * 2;
    o.s2 = at;  at += Bz * H * (H + 1);
    o.M = at;   at += Bz * H * (H + 1);
    o.dgb = at; at += Bz * hmax * 2;
    o.pq = at;  at += Bz * gmax * 2;
    o.rp = at;  at += Bz * (size_t)o.OC * hmax * 2;
    o.op = at;  at += Bz * (size_t)o.OC * omax;
    o.dstride = hmax * P;
    o.d0 = at;  at += Bz * o.dstride;
    o.d1 = at;  at += Bz * o.dstride;
    o.doubles = at;
}

extern "C" size_t rrl_pointnet_group_bwd_workspace_bytes(int B, int N, int S, int c0, int L, const int32_t *widths, const int32_t *groups) {
    PgLayout lo;
    if (!pg_shape(B, N, S, c0, L, widths, groups, lo)) return 0;
    PgBLayout bl;
    pg_blayout(B, N, S, c0, L, widths, groups, bl);
    return bl.doubles * sizeof(double);
}

static unsigned pg_blocks(long long items) { return (unsigned)((items + 255) / 256); }

extern "C" int rrl_pointnet_group_bwd(const float *x, const float **params, const int32_t *widths, const int32_t *groups, const void *ws,
                                      size_t ws_bytes, const int32_t *arg, const float *g_out, void *bws, size_t bws_bytes, float *d_x,
                                      float **d_params, int B, int N, int S, int c0, int L, void *stream) {
    PgLayout lo;
    if (!x || !params || !ws || !arg || !g_out || !bws || !pg_shape(B, N, S, c0, L, widths, groups, lo)) return RRL_E_ARG;
    for (int i = 0; i < 4 * L; ++i)
        if (!params[i]) return RRL_E_ARG;
    PgBLayout bl;
    pg_blayout(B, N, S, c0, L, widths, groups, bl);
    if ((((uintptr_t)ws) & 15) != 0 || ws_bytes < lo.bytes || (((uintptr_t)bws) & 7) != 0 || bws_bytes < bl.doubles * sizeof(double))
        return RRL_E_WS;
    if (B == 0) return 0;
    const char *base = (const char *)ws;
    double *bw = (double *)bws;
    hipStream_t st = (hipStream_t)stream;
    float *none[4] = {nullptr, nullptr, nullptr, nullptr};
    const int P = lo.P;
    auto operand = [&](int l) {  // h_{l-1}, the input of layer l (0-based)
        PgIn I = {};
        if (l == 0) {
            I.src = x; I.first = 1; I.rows = c0;
        } else {
            I.src = (const float *)(base + lo.off[RRL_PG_Y]) + lo.yoff[l - 1];
            I.stride = lo.hid * (size_t)P;
            I.coef = (const double *)(base + lo.off[RRL_PG_COEF]) + 2 * lo.coff[l - 1];
            I.coef_stride = lo.ctot;
            I.rows = widths[l - 1];
        }
        return I;
    };
    PgB k = {};
    k.B = B; k.N = N; k.S = S; k.P = P; k.OC = bl.OC;
    k.K = widths[L - 1]; k.H = widths[L - 2]; k.G = groups[L - 1];
    k.c = k.H; k.cin = k.H;  // (the Gram matrix: pg_outer's shape)
    k.in = operand(L - 1);
    k.W = params[4 * (L - 1)]; k.bias = params[4 * (L - 1) + 1]; k.gamma = params[4 * (L - 1) + 2];
    k.stat = (const double *)(base + lo.off[RRL_PG_STAT]) + 4 * lo.goff[L - 1]; k.stat_stride = lo.gtot;
    k.coef = (const double *)(base + lo.off[RRL_PG_COEF]) + 2 * lo.coff[L - 1]; k.coef_stride = lo.ctot;
    k.ext = (const float *)(base + lo.off[RRL_PG_EXT]); k.flag = (const int32_t *)(base + lo.off[RRL_PG_FLAG]);
    k.arg = arg; k.g = g_out;
    k.dgl = bw + bl.dgl; k.ab = bw + bl.ab; k.s2 = bw + bl.s2; k.M = bw + bl.M; k.dgb = bw + bl.dgb; k.pq = bw + bl.pq;
    k.rp = bw + bl.rp; k.op = bw + bl.op;
    k.dstride = bl.dstride;
    k.dout = bw + bl.d0;
    float **dl = d_params ? d_params + 4 * (L - 1) : none;
    k.dW = dl[0]; k.db = dl[1]; k.dgamma = dl[2]; k.dbeta = dl[3];
    const long long hz = k.H + 1;
    const bool last_params = k.dW || k.db || k.dgamma || k.dbeta;
    hipLaunchKernelGGL(pg_bl_prep, dim3((unsigned)B), dim3(256), 0, st, k);
    if (k.dW || k.db) {  // S1 and S2 serve dW_L and db_L only
        k.x_is_in = 1; k.per_sample = 1;
        hipLaunchKernelGGL(pg_outer, dim3((unsigned)bl.OC, (unsigned)B), dim3(256), 0, st, k);
        hipLaunchKernelGGL(pg_outer_merge, dim3(pg_blocks(k.H * hz), (unsigned)B), dim3(256), 0, st, k);
        k.x_is_in = 0; k.per_sample = 0;
    }
    hipLaunchKernelGGL(pg_bl_M, dim3(pg_blocks(k.H * hz), (unsigned)B), dim3(256), 0, st, k);
    pg_apply_launch<false>(k, k.H, st);
    {
        const dim3 grid((unsigned)N, (unsigned)((k.H + 63) / 64), (unsigned)B);
        if (S <= 64) hipLaunchKernelGGL((pg_sparse_gate<65>), grid, dim3(64), 0, st, k);
        else hipLaunchKernelGGL((pg_sparse_gate<129>), grid, dim3(64), 0, st, k);
    }
    if (last_params) hipLaunchKernelGGL(pg_bl_dW, dim3((unsigned)((k.K * hz + 3) / 4)), dim3(256), 0, st, k);
    double *cur = bw + bl.d0, *other = bw + bl.d1;
    for (int l = L - 2; l >= 0; --l) {
        k.c = widths[l]; k.cin = l ? widths[l - 1] : c0; k.G = groups[l];
        k.in = operand(l);
        k.W = params[4 * l]; k.bias = params[4 * l + 1]; k.gamma = params[4 * l + 2];
        k.y = (const float *)(base + lo.off[RRL_PG_Y]) + lo.yoff[l]; k.y_stride = lo.hid * (size_t)P;
        k.stat = (const double *)(base + lo.off[RRL_PG_STAT]) + 4 * lo.goff[l];
        k.din = cur; k.dout = other;
        dl = d_params ? d_params + 4 * l : none;
        k.dW = dl[0]; k.db = dl[1]; k.dgamma = dl[2]; k.dbeta = dl[3];
        hipLaunchKernelGGL(pg_bh_reduce, dim3((unsigned)bl.OC, (unsigned)((k.c + 3) / 4), (unsigned)B), dim3(256), 0, st, k);
        hipLaunchKernelGGL(pg_bh_merge, dim3((unsigned)B), dim3(256), 0, st, k);
        if (k.dgamma || k.dbeta) hipLaunchKernelGGL(pg_bh_params, dim3(pg_blocks(k.c)), dim3(256), 0, st, k);
        hipLaunchKernelGGL(pg_bh_apply, dim3(pg_blocks((long long)k.c * P), (unsigned)B), dim3(256), 0, st, k);
        if (k.dW || k.db) {
            hipLaunchKernelGGL(pg_outer, dim3((unsigned)bl.OC, (unsigned)B), dim3(256), 0, st, k);
            hipLaunchKernelGGL(pg_outer_merge, dim3(pg_blocks((long long)k.c * (k.cin + 1))), dim3(256), 0, st, k);
        }
        k.to_x = l == 0;
        k.dx = d_x;
        if (l > 0 || d_x) pg_apply_launch<true>(k, k.cin, st);
        double *t = cur; cur = other; other = t;
    }
    RRL_LAUNCH_CHECK();
    return 0;
}
