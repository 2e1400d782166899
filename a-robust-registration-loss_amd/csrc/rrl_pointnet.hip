// rrl_pointnet.hip -- a shared-MLP + GroupNorm + ReLU + max-pool encoder (FMR's PointNet, fmr/model.py:57-126; RPM's
// ParameterPredictionNet.prepool, rpm/models/feature_nets.py:31-52) as a forward and a backward entry, rrl_pointnet_fwd and
// rrl_pointnet_bwd (include/rrl.h).  The rule is stated in the header; this file is its device side.
//
// Forward: one launch of pn_layer_kernel and one of pn_finish_kernel per layer.  (The backward's kernels are described where they
// start, below the forward's host code.)
// pn_layer_kernel, grid (pairs of chunks of PN_CHUNK points, blocks of 128 output channels, B), two groups of four wavefronts,
// one chunk each: wavefront w of a group owns the 32 output channels of tile 4 blockIdx.y + w and walks its chunk's 32-point
// tiles; a SIMD holds one wavefront of each group, so the MFMAs of one overlap the LDS reads and the epilogue of the other.
// The block's weights lie in LDS in operand order, shared by both groups.  A group stages its tile's input operand
// h_{l-1}[k][n] in LDS (two buffers, one barrier per tile; the next tile's loads are issued before this tile's MFMAs) and
// applies the previous layer's activation while it does so: float32(max(0, double(y) a_k + d_k)), and h is never stored.  From
// 64 input channels upward the chain is the f32-input MFMA of rrl_pointer.hip (the same tile mapping: the A operand's 32 rows
// = output channels land in a lane's 16 accumulator registers, the B operand's 32 columns = points on the lanes); below, the
// same 16 x 32 layout by plain fmaf.  The accumulator starts at the bias.  The epilogue stores y (hidden layers), adds the
// lane's values to its per-channel double sums of y and y^2 and -- last layer only -- keeps the running extremum with its
// lowest index; y_L is never stored.  One (sum, sum of squares[, extremum, index]) per (chunk, channel) goes to the workspace.
// pn_finish_kernel, grid (B): per group the chunks and channels merged in index order, mu, r, the channels' a and d; last
// layer: the extrema merged over the chunks, features, arg, info.
#include <cstddef>
#include <cstdint>
#include <cmath>

#include "rrl_common.h"
#include "rrl_wave_sum_d.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

#define PN_CHUNK 128   // points per partial sum: a workgroup takes two chunks
#define PN_APITCH 68   // floats per row of the weights in LDS (64 steps + 4: a lane's 16-byte reads 4 banks from its neighbour's)
#define PN_MAX_N (1 << 20)
#define PN_EPART 2     // words per (chunk, channel) of the last layer: the extremum's z (y, or -y where gamma < 0), its index

// one layer's launch: what pn_layer_kernel and pn_finish_kernel read
struct PnArgs {
    int B, N, P;              // P: chunks
    int cin, cout, G;
    int first, last;
    double eps;
    const float *in;          // first: points [B][N][cin]; else y_{l-1} of every sample, in_stride floats apart
    size_t in_stride;
    const double *coef_in;    // a, d of the previous layer's channels [B][coef_stride][2] (+ its channel offset)
    size_t coef_stride;
    const float *W, *bias, *gamma, *beta;
    float *y;                 // hidden: y_l [cout][N] per sample, y_stride floats apart
    size_t y_stride;
    double *part;             // [B][P][cout][2], the layer's own
    float *epart;             // last: [B][P][cout][PN_EPART]
    double *stat;             // [B][stat_stride][4] (+ the layer's group offset): sum y, sum y^2, mu, r
    size_t stat_stride;
    double *coef;             // [B][coef_stride][2] (+ the layer's channel offset)
    int32_t *flag;            // [B]
    float *ext, *feat;        // last: [B][cout]
    int32_t *arg, *info;
};

__device__ __forceinline__ int pn_arow(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// The tile's operand [k][32 points], in two halves so that the loads' latency hides behind the previous tile's MFMAs:
// pn_load issues the global loads of the next tile into registers (unconditional and in bounds: a row at or beyond cin repeats
// row cin - 1, a point at or beyond N point N - 1; the epilogue leaves such points out), pn_store applies the previous layer's
// activation and writes LDS; rows cin .. kpad - 1 (kpad: cin rounded up to 8, so every 16-byte operand read is of written words) are zero.  IT rows per thread.
template <int IT>
__device__ __forceinline__ void pn_load(const PnArgs &k, int b, int tid, int n0, float (&pre)[IT]) {
    const int q = tid & 31, n = min(n0 + q, k.N - 1);
#pragma unroll
    for (int i = 0; i < IT; ++i) {
        const int kk = min((tid >> 5) + 8 * i, k.cin - 1);
        pre[i] = k.first ? k.in[((size_t)b * k.N + n) * k.cin + kk] : k.in[(size_t)b * k.in_stride + (size_t)kk * k.N + n];
    }
}
template <int IT>
__device__ __forceinline__ void pn_store(const PnArgs &k, int tid, int kpad, const double *__restrict__ cf, const float (&pre)[IT], float *__restrict__ dst) {
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

template <int S, bool LAST>
__global__ __launch_bounds__(512) void pn_layer_kernel(const PnArgs k) {
    __shared__ float hs[2][2][128 * 32];                   // [buffer][group]: the operand tiles
    __shared__ __attribute__((aligned(16))) float as[S > 0 ? 4 * 64 * PN_APITCH : 4];   // the block's weights in MFMA operand order
    __shared__ double cf[2 * 128];
    __shared__ float bsh[128];                             // the block's biases: every chain starts there
    const int b = blockIdx.z, grp = threadIdx.x >> 8, tid = threadIdx.x & 255, w = tid >> 6, lane = tid & 63, h = lane >> 5, q = lane & 31;
    const int chunk = 2 * blockIdx.x + grp, cbase = blockIdx.y * 128, c0 = cbase + w * 32;
    const bool active = c0 < k.cout && chunk < k.P;  // (wavefront-uniform)
    const int kpad = (k.cin + 7) & ~7, steps = (k.cin + 1) >> 1;  // kpad: the operands' rows, zero from cin on, whole 16-byte reads
    if (!k.first) {
        for (int i = threadIdx.x; i < 2 * k.cin; i += 512) cf[i] = k.coef_in[(size_t)b * k.coef_stride * 2 + i];
    }
    // the weights of the workgroup's 128 output channels, once: step s of lane (q, h) of wavefront w takes input channel
    // 2 s + h of output channel cbase + 32 w + q, so a lane's steps lie side by side (rows of PN_APITCH floats: four steps per
    // 16-byte read, the rows 4 banks apart); a channel at or beyond cout and the channel that pads an odd cin are zero
    if (S > 0) {
        for (int i0 = threadIdx.x; i0 < 128 * kpad; i0 += 512 * 8) {  // eight loads in flight (unconditional, clamped), then the writes
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
                    as[((cl >> 5) * 64 + (cl & 31) * 2 + (kk & 1)) * PN_APITCH + (kk >> 1)] = (cbase + cl < k.cout && kk < k.cin) ? v[u] : 0.f;
            }
        }
    }
    // r > 0, so a_c = gamma_c r >= 0 exactly where gamma_c >= 0 (the product of a float32 and r cannot underflow in double): the
    // channel's extremum is the maximum of z = y (gamma_c >= 0) or z = -y (gamma_c < 0; the negation is exact), ONE running
    // maximum with its lowest index per channel; bit r of `neg` marks the second kind
    unsigned neg = 0;
    if (threadIdx.x < 128) bsh[threadIdx.x] = k.bias[min(cbase + (int)threadIdx.x, k.cout - 1)];
    if (LAST) {
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (k.gamma[min(c0 + pn_arow(r, h), k.cout - 1)] < 0.f) neg |= 1u << r;
    }
    double sy[16], syy[16];
    float mx[16];
    int imx[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        sy[r] = 0.0;
        syy[r] = 0.0;
        mx[r] = -INFINITY;
        imx[r] = 0;
    }
    const int nbeg = chunk * PN_CHUNK, nend = min(k.N, nbeg + PN_CHUNK);  // (nend <= nbeg: a group without a chunk)
    constexpr int IT = S > 0 ? S / 4 : 8;  // rows of the operand per thread: kpad <= 2 S (S = 0: cin < 64)
    float pre[IT];
    if (nbeg < nend) pn_load<IT>(k, b, tid, nbeg, pre);
    __syncthreads();
    if (nbeg < nend) pn_store<IT>(k, tid, kpad, cf, pre, hs[0][grp]);
    __syncthreads();
#pragma unroll 1
    for (int t = 0; t < PN_CHUNK / 32; ++t) {  // the same count for both groups: the barrier is the workgroup's
        const int n0 = nbeg + 32 * t;
        const bool more = n0 + 32 < nend;  // (uniform over the group)
        if (more) pn_load<IT>(k, b, tid, n0 + 32, pre);
        if (active && n0 < nend) {
            const float *hb = hs[t & 1][grp];
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = bsh[w * 32 + pn_arow(r, h)];
            if (S > 0) {
                const float *ap = as + (w * 64 + q * 2 + h) * PN_APITCH;
#pragma unroll 2
                for (int s4 = 0; s4 < S / 4; ++s4) {
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
                        acc[r] = __builtin_fmaf(k.W[(size_t)min(c0 + pn_arow(r, h), k.cout - 1) * k.cin + kk], hv, acc[r]);
                }
            }
            const int n = n0 + q;
            if (n < k.N) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float v = acc[r];
                    const double vd = (double)v;
                    sy[r] += vd;
                    syy[r] += vd * vd;
                    if (LAST) {
                        const float z = (neg >> r) & 1u ? -v : v;
                        if (z > mx[r]) {
                            mx[r] = z;
                            imx[r] = n;
                        }
                    } else if (c0 + pn_arow(r, h) < k.cout) {
                        k.y[(size_t)b * k.y_stride + (size_t)(c0 + pn_arow(r, h)) * k.N + n] = v;
                    }
                }
            }
        }
        if (more) pn_store<IT>(k, tid, kpad, cf, pre, hs[(t + 1) & 1][grp]);
        __syncthreads();
    }
    if (!active) return;
    // the 32 lanes of a half-wave hold the 32 points of every tile: one fixed butterfly over them
#pragma unroll
    for (int r = 0; r < 16; ++r) {
#pragma unroll
        for (int m = 16; m >= 1; m >>= 1) {
            sy[r] += __shfl_xor(sy[r], m);
            syy[r] += __shfl_xor(syy[r], m);
            if (LAST) {
                const float ox = __shfl_xor(mx[r], m);
                const int oix = __shfl_xor(imx[r], m);
                if (ox > mx[r] || (ox == mx[r] && oix < imx[r])) {
                    mx[r] = ox;
                    imx[r] = oix;
                }
            }
        }
        if (q == 0 && c0 + pn_arow(r, h) < k.cout) {
            const size_t o = ((size_t)b * k.P + chunk) * k.cout + c0 + pn_arow(r, h);
            k.part[2 * o] = sy[r];
            k.part[2 * o + 1] = syy[r];
            if (LAST) {
                float *e = k.epart + PN_EPART * o;
                e[0] = mx[r];
                e[1] = __int_as_float(imx[r]);
            }
        }
    }
}

template <bool LAST>
__global__ __launch_bounds__(256) void pn_finish_kernel(const PnArgs k) {
    const int b = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int cpg = k.cout / k.G;
    const double m = (double)cpg * (double)k.N;
    double *stat = k.stat + (size_t)b * k.stat_stride * 4, *coef = k.coef + (size_t)b * k.coef_stride * 2;
    int bad = k.first ? 0 : k.flag[b];  // (every lane reads it before the barrier below; lane 0 writes it after)
    // a channel's chunks in index order first (the channels side by side: independent loads), parked in the channel's coef slot
    for (int c = threadIdx.x; c < k.cout; c += 256) {
        double s = 0.0, ss = 0.0;
#pragma unroll 4
        for (int p = 0; p < k.P; ++p) {
            const double2 pp = *(const double2 *)(k.part + 2 * (((size_t)b * k.P + p) * k.cout + c));
            s += pp.x;
            ss += pp.y;
        }
        coef[2 * c] = s;
        coef[2 * c + 1] = ss;
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
    if (LAST) {
        for (int c = threadIdx.x; c < k.cout; c += 256) {
            float mx = -INFINITY;
            int imx = 0;
#pragma unroll 4
            for (int p = 0; p < k.P; ++p) {  // chunks ascending: a tie keeps the lower index (both words in one unconditional load)
                const float2 e = *(const float2 *)(k.epart + PN_EPART * (((size_t)b * k.P + p) * k.cout + c));
                if (e.x > mx) {
                    mx = e.x;
                    imx = __float_as_int(e.y);
                }
            }
            const double ac = coef[2 * c], dc = coef[2 * c + 1];
            const float ext = k.gamma[c] < 0.f ? -mx : mx;
            const double t = (double)ext * ac + dc;
            const size_t o = (size_t)b * k.cout + c;
            k.ext[o] = ext;
            k.arg[o] = imx;
            k.feat[o] = bad ? NAN : (float)(t < 0.0 ? 0.0 : t);
        }
        if (k.info && threadIdx.x == 0) k.info[b] = bad ? 1 : 0;
    }
    if (threadIdx.x == 0) k.flag[b] = bad ? 1 : 0;
}

// ---- host ------------------------------------------------------------------------------------------------------------
struct PnLayout {
    size_t off[RRL_PN_FIELDS];  // bytes
    size_t bytes;
    size_t ctot, gtot, hid;     // channels and groups of all layers, hidden channels
    size_t coff[RRL_PN_MAX_LAYERS], goff[RRL_PN_MAX_LAYERS], yoff[RRL_PN_MAX_LAYERS];
    int P;
};

static bool pn_shape(int B, int N, int c0, int L, const int32_t *widths, const int32_t *groups, PnLayout &lo) {
    if (B < 0 || B > 65535 || N < 1 || N > PN_MAX_N || c0 < 1 || c0 > RRL_PN_MAX_C0 || L < 2 || L > RRL_PN_MAX_LAYERS || !widths || !groups)
        return false;
    lo = {};
    for (int l = 0; l < L; ++l) {
        const int c = widths[l], g = groups[l];
        if (c < 1 || g < 1 || c % g != 0 || c > (l + 1 < L ? RRL_PN_MAX_HIDDEN : RRL_IC_MAX_K)) return false;
        lo.coff[l] = lo.ctot;
        lo.goff[l] = lo.gtot;
        lo.yoff[l] = lo.hid * (size_t)N;
        lo.ctot += (size_t)c;
        lo.gtot += (size_t)g;
        if (l + 1 < L) lo.hid += (size_t)c;
    }
    lo.P = (N + PN_CHUNK - 1) / PN_CHUNK;
    const size_t K = (size_t)widths[L - 1], Bz = (size_t)B;
    size_t o = 0;
    lo.off[RRL_PN_STAT] = o;  o += Bz * lo.gtot * 4 * sizeof(double);
    lo.off[RRL_PN_COEF] = o;  o += Bz * lo.ctot * 2 * sizeof(double);
    lo.off[RRL_PN_PART] = o;  o += Bz * lo.P * lo.ctot * 2 * sizeof(double);
    lo.off[RRL_PN_EPART] = o; o += Bz * lo.P * K * PN_EPART * sizeof(float);
    lo.off[RRL_PN_EXT] = o;   o += Bz * K * sizeof(float);
    lo.off[RRL_PN_FLAG] = o;  o += Bz * sizeof(int32_t);
    lo.off[RRL_PN_Y] = o;     o += Bz * lo.hid * (size_t)N * sizeof(float);
    lo.bytes = o;
    return true;
}

extern "C" size_t rrl_pointnet_workspace_bytes(int B, int N, int c0, int L, const int32_t *widths, const int32_t *groups,
                                               size_t *offsets) {
    PnLayout lo;
    if (!pn_shape(B, N, c0, L, widths, groups, lo)) return 0;
    if (offsets)
        for (int f = 0; f < RRL_PN_FIELDS; ++f) offsets[f] = lo.off[f];
    return lo.bytes;
}

template <bool LAST>
static void pn_launch(const PnArgs &k, hipStream_t st) {
    const dim3 grid((unsigned)((k.P + 1) / 2), (unsigned)((k.cout + 127) / 128), (unsigned)k.B);
    if (k.cin < 64) hipLaunchKernelGGL((pn_layer_kernel<0, LAST>), grid, dim3(512), 0, st, k);
    else if (k.cin <= 64) hipLaunchKernelGGL((pn_layer_kernel<32, LAST>), grid, dim3(512), 0, st, k);
    else hipLaunchKernelGGL((pn_layer_kernel<64, LAST>), grid, dim3(512), 0, st, k);
    hipLaunchKernelGGL((pn_finish_kernel<LAST>), dim3((unsigned)k.B), dim3(256), 0, st, k);
}

extern "C" int rrl_pointnet_fwd(const float *points, const float **params, const int32_t *widths, const int32_t *groups, double eps,
                                void *ws, size_t ws_bytes, float *feat, int32_t *arg, int32_t *info, int B, int N, int c0, int L,
                                void *stream) {
    PnLayout lo;
    if (!points || !params || !ws || !feat || !arg || !(eps > 0.0) || !pn_shape(B, N, c0, L, widths, groups, lo)) return RRL_E_ARG;
    for (int i = 0; i < 4 * L; ++i)
        if (!params[i]) return RRL_E_ARG;
    if ((((uintptr_t)ws) & 15) != 0 || ws_bytes < lo.bytes) return RRL_E_WS;  // (the partials are read 16 bytes at a time)
    if (B == 0) return 0;
    char *base = (char *)ws;
    hipStream_t st = (hipStream_t)stream;
    for (int l = 0; l < L; ++l) {
        PnArgs k = {};
        k.B = B; k.N = N; k.P = lo.P;
        k.cin = l ? widths[l - 1] : c0; k.cout = widths[l]; k.G = groups[l];
        k.first = l == 0; k.last = l == L - 1;
        k.eps = eps;
        k.in = l ? (const float *)(base + lo.off[RRL_PN_Y]) + lo.yoff[l - 1] : points;
        k.in_stride = lo.hid * (size_t)N;
        k.coef_stride = lo.ctot;
        k.coef_in = l ? (const double *)(base + lo.off[RRL_PN_COEF]) + 2 * lo.coff[l - 1] : nullptr;
        k.W = params[4 * l]; k.bias = params[4 * l + 1]; k.gamma = params[4 * l + 2]; k.beta = params[4 * l + 3];
        k.y = (float *)(base + lo.off[RRL_PN_Y]) + lo.yoff[l];
        k.y_stride = lo.hid * (size_t)N;
        k.part = (double *)(base + lo.off[RRL_PN_PART]) + 2 * (size_t)B * lo.P * lo.coff[l];
        k.epart = (float *)(base + lo.off[RRL_PN_EPART]);
        k.stat = (double *)(base + lo.off[RRL_PN_STAT]) + 4 * lo.goff[l];
        k.stat_stride = lo.gtot;
        k.coef = (double *)(base + lo.off[RRL_PN_COEF]) + 2 * lo.coff[l];
        k.flag = (int32_t *)(base + lo.off[RRL_PN_FLAG]);
        k.ext = (float *)(base + lo.off[RRL_PN_EXT]);
        k.feat = feat; k.arg = arg; k.info = info;
        if (k.last) pn_launch<true>(k, st);
        else pn_launch<false>(k, st);
    }
    RRL_LAUNCH_CHECK();
    return 0;
}

// ---- backward: rrl_pointnet_bwd ------------------------------------------------------------------------------------------------
// Everything in double from the forward's kept float32 y_l, its statistics, ext and arg; every sum is one thread's (or one
// wavefront's lanes', then wave_sum_d's fixed tree) over the reduced index ascending; one rounding per output.  The last layer
// costs no N x K work (the header's closed form from S1 and the Gram matrix S2 of h_{L-1}); the hidden layers take the dense
// rule on the kept y_l.  The gradient with respect to a layer's pre-activation travels in a double buffer [c][N] per sample.

struct PnIn {  // an operand h[row][n] of sample b: the points (first) or the activation of a kept y with its a, d
    const float *src;
    size_t stride;
    const double *coef;
    size_t coef_stride;
    int first, rows;
};
__device__ __forceinline__ double pn_in(const PnIn &I, int b, int N, int row, int n) {
    if (I.first) return (double)I.src[((size_t)b * N + n) * I.rows + row];
    const double *cf = I.coef + ((size_t)b * I.coef_stride + row) * 2;
    const double t = (double)I.src[(size_t)b * I.stride + (size_t)row * N + n] * cf[0] + cf[1];
    return (double)(float)(t < 0.0 ? 0.0 : t);
}

// ReLU's gate: the gradient where h > 0, 0 where not -- and h itself where h is NaN (a flagged sample: its gradients are NaN
// throughout, as torch's would be)
__device__ __forceinline__ double pn_gate(double h, double v) { return h > 0.0 ? v : (h != h ? h : 0.0); }

struct PnB {
    int B, N, K, H, G;      // the last layer: K channels of H inputs in G groups
    int c, cin;             // the hidden layer in work: c channels of cin inputs in G groups (G is then that layer's)
    PnIn in;                // the input operand h_{l-1} of the layer in work
    const float *W, *bias, *gamma;
    const float *y;         // the layer's own kept y_l, y_stride floats per sample
    size_t y_stride;
    const double *stat;     // the layer's groups [B][stat_stride][4]
    size_t stat_stride;
    const double *coef;     // the layer's channels [B][coef_stride][2]
    size_t coef_stride;
    const float *ext, *g;
    const int32_t *arg, *flag;
    double *sc, *sx, *tc, *ab, *s2, *M, *dgb, *din, *dout;
    size_t dstride;         // doubles per sample of din / dout
    int per_sample;         // pn_bw_outer: one result per sample (the Gram matrix) or the sum over the batch (dW, db)
    int to_points;          // pn_bh_dh: write d_points [B][N][cin] instead of the gated buffer
    float *dW, *db, *dgamma, *dbeta, *dpts;
};

// s_c = g_f[c] [f[c] > 0] (NaN for a flagged sample), x_c, t_c = r gamma_c s_c; then per group P, Q -> A_g, B_g
__global__ __launch_bounds__(256) void pn_bl_prep(const PnB k) {
    const int b = blockIdx.x, cpg = k.K / k.G;
    const double m = (double)cpg * (double)k.N;
    for (int c = threadIdx.x; c < k.K; c += 256) {
        const double *st = k.stat + ((size_t)b * k.stat_stride + c / cpg) * 4, *cf = k.coef + ((size_t)b * k.coef_stride + c) * 2;
        const size_t o = (size_t)b * k.K + c;
        const float e = k.ext[o];
        const double t = (double)e * cf[0] + cf[1];
        const float f = (float)(t < 0.0 ? 0.0 : t);
        const double s = k.flag[b] ? (double)NAN : (f > 0.f ? (double)k.g[o] : 0.0), x = ((double)e - st[2]) * st[3];
        k.sc[o] = s;
        k.sx[o] = s * x;
        k.tc[o] = st[3] * (double)k.gamma[c] * s;
    }
    __syncthreads();
    for (int g = threadIdx.x; g < k.G; g += 256) {
        const double *st = k.stat + ((size_t)b * k.stat_stride + g) * 4;
        double P = 0.0, Q = 0.0;
        for (int c = g * cpg; c < (g + 1) * cpg; ++c) {
            const double gm = (double)k.gamma[c];
            P += gm * k.sc[(size_t)b * k.K + c];
            Q += gm * k.sx[(size_t)b * k.K + c];
        }
        const double r = st[3], mu = st[2];
        k.ab[((size_t)b * k.G + g) * 2] = -r * P / m + r * r * Q * mu / m;
        k.ab[((size_t)b * k.G + g) * 2 + 1] = -r * r * Q / m;
    }
}

// out[i][j] = sum over n (and over the batch unless per_sample) of X[i][n] Z[j][n], i < c, j <= cin, Z[cin] = 1 (the row sums):
// X = the buffer din (dW, db of a hidden layer) or, without it, the operand `in` itself (S2 and S1 of the last layer's input).
// One wavefront per (i, j): lane l takes n = l, l + 64, ... ascending, sample after sample, then one fixed tree.
__global__ __launch_bounds__(256) void pn_bw_outer(const PnB k) {
    const int cz = k.cin + 1, wid = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (wid >= k.c * cz) return;  // (wavefront-uniform)
    const int i = wid / cz, j = wid - i * cz;
    const int b0 = k.per_sample ? blockIdx.y : 0, b1 = k.per_sample ? b0 + 1 : k.B;
    double acc = 0.0;
    for (int b = b0; b < b1; ++b)
        for (int n = lane; n < k.N; n += 64) {
            const double xv = k.din ? k.din[(size_t)b * k.dstride + (size_t)i * k.N + n] : pn_in(k.in, b, k.N, i, n);
            acc += j < k.cin ? xv * pn_in(k.in, b, k.N, j, n) : xv;
        }
    acc = wave_sum_d(acc);
    if (lane != 0) return;
    if (k.per_sample) k.s2[((size_t)b0 * k.c + i) * cz + j] = acc;
    else if (j < k.cin) {
        if (k.dW) k.dW[(size_t)i * k.cin + j] = (float)acc;
    } else if (k.db) k.db[i] = (float)acc;
}

// M[k][j] = sum_c B_g W[c][k] W[c][j] (j < H) and M[k][H] = sum_c (A_g + B_g b_c) W[c][k], c ascending
__global__ __launch_bounds__(256) void pn_bl_M(const PnB k) {
    const int b = blockIdx.y, hz = k.H + 1, idx = blockIdx.x * 256 + threadIdx.x, cpg = k.K / k.G;
    if (idx >= k.H * hz) return;
    const int kk = idx / hz, j = idx - kk * hz;
    double acc = 0.0;
    for (int c = 0; c < k.K; ++c) {
        const double *ab = k.ab + ((size_t)b * k.G + c / cpg) * 2;
        const double w = (double)k.W[(size_t)c * k.H + kk];
        acc += j < k.H ? ab[1] * w * (double)k.W[(size_t)c * k.H + j] : (ab[0] + ab[1] * (double)k.bias[c]) * w;
    }
    k.M[((size_t)b * k.H + kk) * hz + j] = acc;
}

// dh_{L-1}[k][n] = sum_j M[k][j] h[j][n] + M[k][H] + sum over the channels c ascending with arg_c = n of W[c][k] t_c, gated by h > 0
__global__ __launch_bounds__(256) void pn_bl_dh(const PnB k) {
    const int b = blockIdx.y, hz = k.H + 1;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)k.H * k.N) return;
    const int kk = (int)(idx / k.N), n = (int)(idx - (long long)kk * k.N);
    const double *Mr = k.M + ((size_t)b * k.H + kk) * hz;
    double v = 0.0;
    for (int j = 0; j < k.H; ++j) v += Mr[j] * pn_in(k.in, b, k.N, j, n);
    v += Mr[k.H];
    for (int c = 0; c < k.K; ++c)
        if (k.arg[(size_t)b * k.K + c] == n) v += (double)k.W[(size_t)c * k.H + kk] * k.tc[(size_t)b * k.K + c];
    k.dout[(size_t)b * k.dstride + (size_t)kk * k.N + n] = pn_gate(pn_in(k.in, b, k.N, kk, n), v);
}

// dW_L[c][k] (k < H) and db_L[c] (k = H, where h = 1 and S1 = N), summed over the batch, b ascending; dgamma_L, dbeta_L
__global__ __launch_bounds__(256) void pn_bl_dW(const PnB k) {
    const int hz = k.H + 1, cpg = k.K / k.G;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)k.K * hz) return;
    const int c = (int)(idx / hz), kk = (int)(idx - (long long)c * hz);
    const double bc = (double)k.bias[c];
    double acc = 0.0, dg = 0.0, dbt = 0.0;
    for (int b = 0; b < k.B; ++b) {
        const size_t o = (size_t)b * k.K + c;
        const double *ab = k.ab + ((size_t)b * k.G + c / cpg) * 2, *S = k.s2 + (size_t)b * k.H * hz;
        const int at = min(max(k.arg[o], 0), k.N - 1);
        const double S1k = kk < k.H ? S[(size_t)kk * hz + k.H] : (double)k.N, hk = kk < k.H ? pn_in(k.in, b, k.N, kk, at) : 1.0;
        double dot = 0.0;
        for (int j = 0; j < k.H; ++j) dot += (double)k.W[(size_t)c * k.H + j] * S[(size_t)j * hz + kk];
        acc += k.tc[o] * hk + ab[0] * S1k + ab[1] * (dot + bc * S1k);
        dg += k.sx[o];
        dbt += k.sc[o];
    }
    if (kk < k.H) {
        if (k.dW) k.dW[(size_t)c * k.H + kk] = (float)acc;
    } else {
        if (k.db) k.db[c] = (float)acc;
        if (k.dgamma) k.dgamma[c] = (float)dg;
        if (k.dbeta) k.dbeta[c] = (float)dbt;
    }
}

// a hidden layer's per-sample sums: dgb[b][c] = (sum_n dout xhat, sum_n dout); one wavefront per channel
__global__ __launch_bounds__(256) void pn_bh_reduce(const PnB k) {
    const int b = blockIdx.y, ch = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, cpg = k.c / k.G;
    if (ch >= k.c) return;  // (wavefront-uniform)
    const double *st = k.stat + ((size_t)b * k.stat_stride + ch / cpg) * 4;
    double sg = 0.0, sb = 0.0;
    for (int n = lane; n < k.N; n += 64) {
        const double dv = k.din[(size_t)b * k.dstride + (size_t)ch * k.N + n];
        sg += dv * (((double)k.y[(size_t)b * k.y_stride + (size_t)ch * k.N + n] - st[2]) * st[3]);
        sb += dv;
    }
    sg = wave_sum_d(sg);
    sb = wave_sum_d(sb);
    if (lane == 0) {
        k.dgb[((size_t)b * k.c + ch) * 2] = sg;
        k.dgb[((size_t)b * k.c + ch) * 2 + 1] = sb;
    }
}

// dy = r (gamma dout - P / m - xhat Q / m) in place, P and Q over the group's channels ascending
__global__ __launch_bounds__(256) void pn_bh_apply(const PnB k) {
    const int b = blockIdx.y, cpg = k.c / k.G;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)k.c * k.N) return;
    const int ch = (int)(idx / k.N), n = (int)(idx - (long long)ch * k.N), g = ch / cpg;
    const double *st = k.stat + ((size_t)b * k.stat_stride + g) * 4;
    const double m = (double)cpg * (double)k.N;
    double P = 0.0, Q = 0.0;
    for (int c = g * cpg; c < (g + 1) * cpg; ++c) {
        const double gm = (double)k.gamma[c];
        P += gm * k.dgb[((size_t)b * k.c + c) * 2 + 1];
        Q += gm * k.dgb[((size_t)b * k.c + c) * 2];
    }
    double *p = k.din + (size_t)b * k.dstride + (size_t)ch * k.N + n;
    const double xh = ((double)k.y[(size_t)b * k.y_stride + (size_t)ch * k.N + n] - st[2]) * st[3];
    *p = st[3] * ((double)k.gamma[ch] * *p - P / m - xh * Q / m);
}

// dh_{l-1}[k][n] = sum_c W[c][k] dy[c][n], c ascending: gated by h_{l-1} > 0 into the other buffer, or d_points of layer 1
__global__ __launch_bounds__(256) void pn_bh_dh(const PnB k) {
    const int b = blockIdx.y;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)k.cin * k.N) return;
    const int kk = (int)(idx / k.N), n = (int)(idx - (long long)kk * k.N);
    double v = 0.0;
    for (int c = 0; c < k.c; ++c) v += (double)k.W[(size_t)c * k.cin + kk] * k.din[(size_t)b * k.dstride + (size_t)c * k.N + n];
    if (k.to_points) k.dpts[((size_t)b * k.N + n) * k.cin + kk] = (float)v;
    else k.dout[(size_t)b * k.dstride + (size_t)kk * k.N + n] = pn_gate(pn_in(k.in, b, k.N, kk, n), v);
}

// dgamma_l, dbeta_l of a hidden layer: the samples' sums, b ascending
__global__ __launch_bounds__(256) void pn_bh_merge(const PnB k) {
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

struct PnBLayout {
    size_t sc, sx, tc, ab, s2, M, dgb, d0, d1, doubles, dstride;
};
static void pn_blayout(int B, int N, int L, const int32_t *widths, const int32_t *groups, PnBLayout &o) {
    const size_t Bz = (size_t)B, K = (size_t)widths[L - 1], H = (size_t)widths[L - 2];
    size_t hmax = 0;
    for (int l = 0; l + 1 < L; ++l) hmax = hmax > (size_t)widths[l] ? hmax : (size_t)widths[l];
    size_t at = 0;
    o.sc = at;  at += Bz * K;
    o.sx = at;  at += Bz * K;
    o.tc = at;  at += Bz * K;
    o.ab = at;  at += Bz * (size_t)groups[L - 1] * 2;
    o.s2 = at;  at += Bz * H * (H + 1);
    o.M = at;   at += Bz * H * (H + 1);
    o.dgb = at; at += Bz * hmax * 2;
    o.dstride = hmax * (size_t)N;
    o.d0 = at;  at += Bz * o.dstride;
    o.d1 = at;  at += Bz * o.dstride;
    o.doubles = at;
}

extern "C" size_t rrl_pointnet_bwd_workspace_bytes(int B, int N, int c0, int L, const int32_t *widths, const int32_t *groups) {
    PnLayout lo;
    if (!pn_shape(B, N, c0, L, widths, groups, lo)) return 0;
    PnBLayout bl;
    pn_blayout(B, N, L, widths, groups, bl);
    return bl.doubles * sizeof(double);
}

static unsigned pn_blocks(long long items) { return (unsigned)((items + 255) / 256); }

extern "C" int rrl_pointnet_bwd(const float *points, const float **params, const int32_t *widths, const int32_t *groups, const void *ws,
                                size_t ws_bytes, const int32_t *arg, const float *g_feat, void *bws, size_t bws_bytes, float *d_points,
                                float **d_params, int B, int N, int c0, int L, void *stream) {
    PnLayout lo;
    if (!points || !params || !ws || !arg || !g_feat || !bws || !pn_shape(B, N, c0, L, widths, groups, lo)) return RRL_E_ARG;
    for (int i = 0; i < 4 * L; ++i)
        if (!params[i]) return RRL_E_ARG;
    PnBLayout bl;
    pn_blayout(B, N, L, widths, groups, bl);
    if ((((uintptr_t)ws) & 15) != 0 || ws_bytes < lo.bytes || (((uintptr_t)bws) & 7) != 0 || bws_bytes < bl.doubles * sizeof(double))
        return RRL_E_WS;
    if (B == 0) return 0;
    const char *base = (const char *)ws;
    double *bw = (double *)bws;
    hipStream_t st = (hipStream_t)stream;
    float *none[4] = {nullptr, nullptr, nullptr, nullptr};
    auto operand = [&](int l) {  // h_{l-1}, the input of layer l (0-based)
        PnIn I = {};
        if (l == 0) {
            I.src = points; I.first = 1; I.rows = c0;
        } else {
            I.src = (const float *)(base + lo.off[RRL_PN_Y]) + lo.yoff[l - 1];
            I.stride = lo.hid * (size_t)N;
            I.coef = (const double *)(base + lo.off[RRL_PN_COEF]) + 2 * lo.coff[l - 1];
            I.coef_stride = lo.ctot;
            I.rows = widths[l - 1];
        }
        return I;
    };
    PnB k = {};
    k.B = B; k.N = N; k.K = widths[L - 1]; k.H = widths[L - 2]; k.G = groups[L - 1];
    k.c = k.H; k.cin = k.H;  // (the Gram matrix: pn_bw_outer's shape)
    k.in = operand(L - 1);
    k.W = params[4 * (L - 1)]; k.bias = params[4 * (L - 1) + 1]; k.gamma = params[4 * (L - 1) + 2];
    k.stat = (const double *)(base + lo.off[RRL_PN_STAT]) + 4 * lo.goff[L - 1]; k.stat_stride = lo.gtot;
    k.coef = (const double *)(base + lo.off[RRL_PN_COEF]) + 2 * lo.coff[L - 1]; k.coef_stride = lo.ctot;
    k.ext = (const float *)(base + lo.off[RRL_PN_EXT]); k.flag = (const int32_t *)(base + lo.off[RRL_PN_FLAG]);
    k.arg = arg; k.g = g_feat;
    k.sc = bw + bl.sc; k.sx = bw + bl.sx; k.tc = bw + bl.tc; k.ab = bw + bl.ab; k.s2 = bw + bl.s2; k.M = bw + bl.M; k.dgb = bw + bl.dgb;
    k.dstride = bl.dstride;
    k.dout = bw + bl.d0;
    k.per_sample = 1;
    float **dl = d_params ? d_params + 4 * (L - 1) : none;
    k.dW = dl[0]; k.db = dl[1]; k.dgamma = dl[2]; k.dbeta = dl[3];
    const long long hz = k.H + 1;
    hipLaunchKernelGGL(pn_bl_prep, dim3((unsigned)B), dim3(256), 0, st, k);
    hipLaunchKernelGGL(pn_bw_outer, dim3((unsigned)((k.H * hz + 3) / 4), (unsigned)B), dim3(256), 0, st, k);
    hipLaunchKernelGGL(pn_bl_M, dim3(pn_blocks(k.H * hz), (unsigned)B), dim3(256), 0, st, k);
    hipLaunchKernelGGL(pn_bl_dh, dim3(pn_blocks((long long)k.H * N), (unsigned)B), dim3(256), 0, st, k);
    if (k.dW || k.db || k.dgamma || k.dbeta) hipLaunchKernelGGL(pn_bl_dW, dim3(pn_blocks(k.K * hz)), dim3(256), 0, st, k);
    double *cur = bw + bl.d0, *other = bw + bl.d1;
    for (int l = L - 2; l >= 0; --l) {
        k.c = widths[l]; k.cin = l ? widths[l - 1] : c0; k.G = groups[l];
        k.in = operand(l);
        k.W = params[4 * l]; k.bias = params[4 * l + 1]; k.gamma = params[4 * l + 2];
        k.y = (const float *)(base + lo.off[RRL_PN_Y]) + lo.yoff[l]; k.y_stride = lo.hid * (size_t)N;
        k.stat = (const double *)(base + lo.off[RRL_PN_STAT]) + 4 * lo.goff[l];
        k.din = cur; k.dout = other;
        k.per_sample = 0;
        dl = d_params ? d_params + 4 * l : none;
        k.dW = dl[0]; k.db = dl[1]; k.dgamma = dl[2]; k.dbeta = dl[3];
        hipLaunchKernelGGL(pn_bh_reduce, dim3((unsigned)((k.c + 3) / 4), (unsigned)B), dim3(256), 0, st, k);
        if (k.dgamma || k.dbeta) hipLaunchKernelGGL(pn_bh_merge, dim3(pn_blocks(k.c)), dim3(256), 0, st, k);
        hipLaunchKernelGGL(pn_bh_apply, dim3(pn_blocks((long long)k.c * N), (unsigned)B), dim3(256), 0, st, k);
        if (k.dW || k.db) hipLaunchKernelGGL(pn_bw_outer, dim3((unsigned)(((long long)k.c * (k.cin + 1) + 3) / 4)), dim3(256), 0, st, k);
        k.to_points = l == 0;
        k.dpts = d_points;
        if (l > 0 || d_points) hipLaunchKernelGGL(pn_bh_dh, dim3(pn_blocks((long long)k.cin * N), (unsigned)B), dim3(256), 0, st, k);
        double *t = cur; cur = other; other = t;
    }
    RRL_LAUNCH_CHECK();
    return 0;
}
