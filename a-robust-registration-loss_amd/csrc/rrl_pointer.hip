// rrl_pointer.hip -- DCP's softmax pointer (dcp/model.py:419-425) as two entries, rrl_pointer_fwd / rrl_pointer_bwd
// (include/rrl.h): corr = tgt . softmax(src_emb^T tgt_emb / sqrt(C), dim = 2)^T without the (B, N, M)
// matrix.  The library's first matrix-core unit: gfx950's f32-input MFMA (v_mfma_f32_32x32x2_f32) is bit for bit a
// channel-ordered float32 fmaf chain, so a score is still a result defined by a stated rule (the header states it).
//
// Tile orientation.  One MFMA tile is 32 x 32 chains.  Its A operand's 32 rows land in a lane's 16 accumulator registers
// (row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)), its B operand's 32 columns on the lanes (column = lane & 31).  The forward puts
// the TARGET columns on A and the SOURCE rows on B: a lane then owns one source row and holds 16 of its scores, the row
// softmax is a loop over the lane's own registers, and the two half-waves of a row are merged once per slice.  Both operand
// loads are 32 consecutive floats of one channel row (channel-first storage is already K-major); lanes 0-31 supply channel
// 2 s, lanes 32-63 channel 2 s + 1 of step s, and the accumulator is carried over all steps: ONE chain per score.
//
// Forward, 2 launches: pt_fwd_kernel, grid (column slices of RRL_POINTER_SLICE, ceil(N / 128), B), four wavefronts of 32 rows
// each, two 32-column tiles per pass (they share the source operand and give two independent accumulator chains); a lane
// keeps its scores of the whole slice in registers, so the slice's maximum is known before the first expf; one state
// (m, l, n[3], flag) per (row, slice) into the workspace.  pt_finish_kernel, grid (B): the slices merged in index order,
// corr, the row's (M, L, corr) kept for the backward, info.
// Backward, 1 launch per pass: a workgroup owns 32 source rows (OWN_SRC: d_src_emb) or 32 target columns (d_tgt_emb, d_tgt)
// and walks the other dimension in groups of four 32-wide tiles.  Phase 1: wavefront w recomputes the scores of tile w (the
// same chain, the same bits), turns them into ds and leaves them in LDS [tile][own][reduced].  Phase 2: every wavefront
// multiplies the group's ds with ITS channel tiles (w, w + 4, ...) of the other embedding, 16 accumulator registers per
// channel tile: one fmaf chain per output element over the whole reduced dimension, ascending, never cut.  That product's
// other operand runs ACROSS the channel rows (32 cache lines per load), so each wavefront first copies its 32 channels x 128
// reduced indices into an LDS tile of its own with loads along the rows.  For C <= 512 (pt_bwd_pc_kernel) the two phases
// belong to two sets of four wavefronts, one group apart, over a double-buffered ds; beyond (pt_bwd_kernel) four wavefronts
// take both phases in turn.
#include <cstddef>
#include <cstdint>
#include <cmath>

#include "rrl_common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

#define PT_MAX_DIM 16384
#define PT_STATE 6  // doubles per (row, slice): m, l, n0, n1, n2, flag
#define PT_ROW 5    // doubles per row: M, 1 / L, corr0, corr1, corr2
#define PT_PITCH 33 // floats per LDS row of a ds tile (32 + 1: the lanes of a half-wave read one column)
#define PT_EPITCH 129 // floats per LDS row of an embedding tile of the backward (128 reduced indices + 1)

struct PtArgs {
    int B, C, N, M, S;
    float sc;
    const float *se, *te, *x;
    const int32_t *cs, *ct;
    double *part, *row;
    float *corr, *scores;
    int32_t *info;
    const float *g;
    float *dse, *dte, *dx;
};

// the accumulator register r of lane `lane` holds row pt_arow(r, lane >> 5) of the A operand
__device__ __forceinline__ int pt_arow(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

#define PT_U 4  // MFMA steps per block of the chain loops: the next block's operand loads are issued before this block's MFMAs

// 32 x 32 chains: A's rows a0 .. a0 + 31 of the channel-first matrix A (row length sa, na valid rows, a0 < na), B's likewise.
// A row at or beyond the valid count is zero in the operand (its lane loads the last valid row's address instead, so every
// load is unconditional and in bounds), and the channel that pads an odd C is zero in BOTH operands.
__device__ __forceinline__ f32x16 pt_chain(const float *__restrict__ A, int sa, int a0, int na, const float *__restrict__ Bm,
                                           int sb, int b0, int nb, int C) {
    const int lane = threadIdx.x & 63, h = lane >> 5, q = lane & 31;
    const bool va = a0 + q < na, vb = b0 + q < nb;
    const float *pa = A + (size_t)h * sa + min(a0 + q, na - 1), *pb = Bm + (size_t)h * sb + min(b0 + q, nb - 1);
    f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int Cfull = C - C % (2 * PT_U);
    float a[PT_U] = {}, b[PT_U] = {}, an[PT_U] = {}, bn[PT_U] = {};
    if (Cfull > 0) {
#pragma unroll
        for (int u = 0; u < PT_U; ++u) {
            a[u] = pa[(size_t)(2 * u) * sa];
            b[u] = pb[(size_t)(2 * u) * sb];
        }
    }
    int c2 = 0;
    for (; c2 < Cfull; c2 += 2 * PT_U) {
        if (c2 + 2 * PT_U < Cfull) {
#pragma unroll
            for (int u = 0; u < PT_U; ++u) {
                an[u] = pa[(size_t)(c2 + 2 * PT_U + 2 * u) * sa];
                bn[u] = pb[(size_t)(c2 + 2 * PT_U + 2 * u) * sb];
            }
        }
#pragma unroll
        for (int u = 0; u < PT_U; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(va ? a[u] : 0.f, vb ? b[u] : 0.f, acc, 0, 0, 0);
#pragma unroll
        for (int u = 0; u < PT_U; ++u) {
            a[u] = an[u];
            b[u] = bn[u];
        }
    }
    for (; c2 + 1 < C; c2 += 2) {
        const float av = pa[(size_t)c2 * sa], bv = pb[(size_t)c2 * sb];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(va ? av : 0.f, vb ? bv : 0.f, acc, 0, 0, 0);
    }
    if (c2 < C) {  // odd C: the last channel on lanes 0-31, zeros on lanes 32-63
        const float av = h == 0 ? pa[(size_t)c2 * sa] : 0.f, bv = h == 0 ? pb[(size_t)c2 * sb] : 0.f;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(va ? av : 0.f, vb ? bv : 0.f, acc, 0, 0, 0);
    }
    return acc;
}

// two A tiles (a0 and a0 + 32) against one B tile: the B load is shared, the two chains are independent
__device__ __forceinline__ void pt_chain2(const float *__restrict__ A, int sa, int a0, int na, const float *__restrict__ Bm, int sb,
                                          int b0, int nb, int C, f32x16 &acc0, f32x16 &acc1) {
    const int lane = threadIdx.x & 63, h = lane >> 5, q = lane & 31;
    const bool va0 = a0 + q < na, va1 = a0 + 32 + q < na, vb = b0 + q < nb;
    const float *pa0 = A + (size_t)h * sa + min(a0 + q, na - 1), *pa1 = A + (size_t)h * sa + min(a0 + 32 + q, na - 1);
    const float *pb = Bm + (size_t)h * sb + min(b0 + q, nb - 1);
    const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    acc0 = zero;
    acc1 = zero;
    const int Cfull = C - C % (2 * PT_U);
    float x0[PT_U] = {}, x1[PT_U] = {}, b[PT_U] = {}, x0n[PT_U] = {}, x1n[PT_U] = {}, bn[PT_U] = {};
    if (Cfull > 0) {
#pragma unroll
        for (int u = 0; u < PT_U; ++u) {
            x0[u] = pa0[(size_t)(2 * u) * sa];
            x1[u] = pa1[(size_t)(2 * u) * sa];
            b[u] = pb[(size_t)(2 * u) * sb];
        }
    }
    int c2 = 0;
    for (; c2 < Cfull; c2 += 2 * PT_U) {
        if (c2 + 2 * PT_U < Cfull) {
#pragma unroll
            for (int u = 0; u < PT_U; ++u) {
                x0n[u] = pa0[(size_t)(c2 + 2 * PT_U + 2 * u) * sa];
                x1n[u] = pa1[(size_t)(c2 + 2 * PT_U + 2 * u) * sa];
                bn[u] = pb[(size_t)(c2 + 2 * PT_U + 2 * u) * sb];
            }
        }
#pragma unroll
        for (int u = 0; u < PT_U; ++u) {
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(va0 ? x0[u] : 0.f, vb ? b[u] : 0.f, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(va1 ? x1[u] : 0.f, vb ? b[u] : 0.f, acc1, 0, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < PT_U; ++u) {
            x0[u] = x0n[u];
            x1[u] = x1n[u];
            b[u] = bn[u];
        }
    }
    for (; c2 + 1 < C; c2 += 2) {
        const float v0 = pa0[(size_t)c2 * sa], v1 = pa1[(size_t)c2 * sa], bv = pb[(size_t)c2 * sb];
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(va0 ? v0 : 0.f, vb ? bv : 0.f, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(va1 ? v1 : 0.f, vb ? bv : 0.f, acc1, 0, 0, 0);
    }
    if (c2 < C) {
        const float v0 = h == 0 ? pa0[(size_t)c2 * sa] : 0.f, v1 = h == 0 ? pa1[(size_t)c2 * sa] : 0.f;
        const float bv = h == 0 ? pb[(size_t)c2 * sb] : 0.f;
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(va0 ? v0 : 0.f, vb ? bv : 0.f, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(va1 ? v1 : 0.f, vb ? bv : 0.f, acc1, 0, 0, 0);
    }
}

#define PT_TILES (RRL_POINTER_SLICE / 32)  // 32-column tiles of a slice: a lane keeps its 16 scores of each in registers

// One (row, slice) state: m = the largest score of the row's columns in the slice, l = sum p and n = sum p x in double with
// p = expf(z - m): every term meets ONE expf here and one more when the slices are merged (pt_finish_kernel) -- no running
// maximum, so no term is rescaled a number of times that depends on the data.
__global__ __launch_bounds__(256) void pt_fwd_kernel(const PtArgs k) {
    const int b = blockIdx.z, sl = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63, h = lane >> 5, q = lane & 31;
    const int j0 = (blockIdx.y * 4 + w) * 32;
    if (j0 >= k.N) return;
    const int ns = rrl_rows(k.cs, b, k.N), nt = rrl_rows(k.ct, b, k.M);
    const int j = j0 + q, k0 = sl * RRL_POINTER_SLICE;
    const bool vj = j < ns;
    const float *se = k.se + (size_t)b * k.C * k.N, *te = k.te + (size_t)b * k.C * k.M;
    float z[PT_TILES][16];
#pragma unroll
    for (int pr = 0; pr < PT_TILES / 2; ++pr) {
        const int kt = k0 + 64 * pr;
        f32x16 acc0 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
        if (j0 < ns && kt < nt) pt_chain2(te, k.M, kt, nt, se, k.N, j0, ns, k.C, acc0, acc1);  // (wavefront-uniform)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            z[2 * pr][r] = acc0[r] * k.sc;
            z[2 * pr + 1][r] = acc1[r] * k.sc;
        }
    }
    float m = -INFINITY;
    int flag = 0;
#pragma unroll
    for (int t = 0; t < PT_TILES; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int col = k0 + 32 * t + pt_arow(r, h);
            const bool v = vj && col < nt;
            if (k.scores && j < k.N && col < k.M) k.scores[((size_t)b * k.N + j) * k.M + col] = v ? z[t][r] : -INFINITY;
            if (v) {
                m = fmaxf(m, z[t][r]);
                flag |= !(fabsf(z[t][r]) < INFINITY);
            }
        }
    m = fmaxf(m, __shfl_xor(m, 32));  // the row's two half-waves share the slice maximum: their sums then simply add
    flag |= __shfl_xor(flag, 32);
    const float *x = k.x + (size_t)b * 3 * k.M;
    double l = 0.0, n0 = 0.0, n1 = 0.0, n2 = 0.0;
#pragma unroll
    for (int t = 0; t < PT_TILES; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int col = k0 + 32 * t + pt_arow(r, h);
            if (vj && col < nt) {
                const double p = z[t][r] == -INFINITY ? 0.0 : (double)expf(z[t][r] - m);  // (never -inf - -inf)
                l += p;
                n0 += p * (double)x[col];
                n1 += p * (double)x[k.M + col];
                n2 += p * (double)x[2 * k.M + col];
            }
        }
    const double ol = __shfl_xor(l, 32), o0 = __shfl_xor(n0, 32), o1 = __shfl_xor(n1, 32), o2 = __shfl_xor(n2, 32);
    if (h == 0 && j < k.N) {  // lanes 0-31 first
        double *p = k.part + ((size_t)b * k.S + sl) * PT_STATE * k.N + j;
        p[0] = (double)m;
        p[(size_t)k.N] = l + ol;
        p[(size_t)2 * k.N] = n0 + o0;
        p[(size_t)3 * k.N] = n1 + o1;
        p[(size_t)4 * k.N] = n2 + o2;
        p[(size_t)5 * k.N] = (double)flag;
    }
}

// the slices of a row: M = the largest slice maximum, then l and n as the sums over the slices in index order of
// l_s expf(m_s - M) (one float32 factor per slice) -> corr, the row's (M, L, corr) for the backward, info
__global__ __launch_bounds__(1024) void pt_finish_kernel(const PtArgs k) {
    const int b = blockIdx.x;
    const int ns = rrl_rows(k.cs, b, k.N), nt = rrl_rows(k.ct, b, k.M);
    const int S = min(k.S, (nt + RRL_POINTER_SLICE - 1) / RRL_POINTER_SLICE);  // the slices that hold a valid column
    int flag = 0;
    for (int j = threadIdx.x; j < k.N; j += 1024) {
        const bool v = j < ns && nt > 0;
        const double *p = k.part + (size_t)b * k.S * PT_STATE * k.N + j;
        const size_t st = (size_t)PT_STATE * k.N;
        float M = -INFINITY;
        double l = 0.0, n0 = 0.0, n1 = 0.0, n2 = 0.0;
        if (v) {
            for (int sl = 0; sl < S; ++sl) M = fmaxf(M, (float)p[sl * st]);
            for (int sl = 0; sl < S; ++sl) {
                const double *ps = p + sl * st;
                const float ms = (float)ps[0];
                flag |= ps[(size_t)5 * k.N] != 0.0;
                if (ms == -INFINITY) continue;  // a slice of -inf scores only: p = 0 throughout
                const double f = (double)expf(ms - M);
                l += ps[(size_t)k.N] * f;
                n0 += ps[(size_t)2 * k.N] * f;
                n1 += ps[(size_t)3 * k.N] * f;
                n2 += ps[(size_t)4 * k.N] * f;
            }
        }
        const float c0 = v ? (float)(n0 / l) : 0.f, c1 = v ? (float)(n1 / l) : 0.f, c2 = v ? (float)(n2 / l) : 0.f;
        float *c = k.corr + (size_t)b * 3 * k.N + j;
        c[0] = c0;
        c[k.N] = c1;
        c[2 * k.N] = c2;
        double *rw = k.row + (size_t)b * PT_ROW * k.N + j;
        rw[0] = v ? (double)M : 0.0;
        rw[(size_t)k.N] = v ? 1.0 / l : 0.0;
        rw[(size_t)2 * k.N] = (double)c0;
        rw[(size_t)3 * k.N] = (double)c1;
        rw[(size_t)4 * k.N] = (double)c2;
    }
    flag = __syncthreads_or(flag);
    if (k.info && threadIdx.x == 0) k.info[b] = flag ? 1 : 0;
}

// LDS writes of a wavefront made visible to its own other lanes (the tile is private to the wavefront: no workgroup barrier)
__device__ __forceinline__ void pt_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// what ds needs of source row j: the row's final maximum and the reciprocal of its sum, its upstream gradient and delta = g . corr
struct PtRowQ {
    float M;
    double invL, g0, g1, g2, delta;
};
__device__ __forceinline__ PtRowQ pt_rowq(const PtArgs &k, int b, int j) {
    const double *rw = k.row + (size_t)b * PT_ROW * k.N + j;
    const float *g = k.g + (size_t)b * 3 * k.N + j;
    PtRowQ r;
    r.M = (float)rw[0];
    r.invL = rw[(size_t)k.N];
    r.g0 = (double)g[0];
    r.g1 = (double)g[k.N];
    r.g2 = (double)g[2 * k.N];
    r.delta = (r.g0 * rw[(size_t)2 * k.N] + r.g1 * rw[(size_t)3 * k.N]) + r.g2 * rw[(size_t)4 * k.N];
    return r;
}

// What a backward workgroup knows of its sample.  OWN_SRC: it owns 32 source rows and writes d_src_emb; else 32 target
// columns, d_tgt_emb and d_tgt.  "own" is the owned dimension, "red" the one the chains run over.
struct PtBwd {
    int b, ns, nt, Nown, Nred, no, nr, o0;
    const float *Eo, *Er, *x;
};
template <bool OWN_SRC>
__device__ __forceinline__ PtBwd pt_bwd_ctx(const PtArgs &k) {
    PtBwd c;
    c.b = blockIdx.y;
    c.ns = rrl_rows(k.cs, c.b, k.N);
    c.nt = rrl_rows(k.ct, c.b, k.M);
    c.Nown = OWN_SRC ? k.N : k.M;
    c.Nred = OWN_SRC ? k.M : k.N;
    c.no = OWN_SRC ? c.ns : c.nt;
    c.nr = OWN_SRC ? c.nt : c.ns;
    c.o0 = blockIdx.x * 32;
    c.Eo = (OWN_SRC ? k.se : k.te) + (size_t)c.b * k.C * c.Nown;
    c.Er = (OWN_SRC ? k.te : k.se) + (size_t)c.b * k.C * c.Nred;
    c.x = k.x + (size_t)c.b * 3 * k.M;
    return c;
}

// the per-lane constants of the ds phase: the lane's own row (OWN_SRC) or its own column's point, and the d_tgt sums
struct PtLane {
    PtRowQ rq;
    double x0, x1, x2, dx0, dx1, dx2;
};
template <bool OWN_SRC>
__device__ __forceinline__ PtLane pt_lane_init(const PtArgs &k, const PtBwd &c) {
    PtLane l = {};
    const int oi = c.o0 + (threadIdx.x & 31);
    if (OWN_SRC) {
        if (oi < c.ns) l.rq = pt_rowq(k, c.b, oi);
    } else if (oi < c.nt) {
        l.x0 = (double)c.x[oi]; l.x1 = (double)c.x[k.M + oi]; l.x2 = (double)c.x[2 * k.M + oi];
    }
    return l;
}

// one 32 x 32 score tile recomputed (reduced indices rt .. rt + 31, rt < nr) and turned into ds in the LDS tile [own][reduced]
template <bool OWN_SRC>
__device__ __forceinline__ void pt_ds_tile(const PtArgs &k, const PtBwd &c, int rt, float *tile, PtLane &l) {
    const int lane = threadIdx.x & 63, h = lane >> 5, q = lane & 31, oi = c.o0 + q;
    const double scd = (double)k.sc;
    const f32x16 ch = pt_chain(c.Er, c.Nred, rt, c.nr, c.Eo, c.Nown, c.o0, c.no, k.C);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int rl = pt_arow(r, h), ri = rt + rl;
        float ds = 0.f;
        if (oi < c.no && ri < c.nr) {
            if (OWN_SRC) {
                l.x0 = (double)c.x[ri]; l.x1 = (double)c.x[k.M + ri]; l.x2 = (double)c.x[2 * k.M + ri];
            } else {
                l.rq = pt_rowq(k, c.b, ri);
            }
            const float z = ch[r] * k.sc;
            const double P = (double)expf(z - l.rq.M) * l.rq.invL;
            const double gx = (l.rq.g0 * l.x0 + l.rq.g1 * l.x1) + l.rq.g2 * l.x2;
            ds = (float)(P * (gx - l.rq.delta) * scd);
            if (!OWN_SRC) {
                l.dx0 += P * l.rq.g0; l.dx1 += P * l.rq.g1; l.dx2 += P * l.rq.g2;
            }
        }
        tile[q * PT_PITCH + rl] = ds;
    }
}

// acc += (channels c0 .. c0 + 31 of the other embedding) x (the group's ds tiles): the wavefront copies its 32 channels x 128
// reduced indices into its own LDS tile `est` with loads along the channel rows (coalesced; the MFMA operand is read across
// the channels), then 16 MFMA steps per ds tile, the tiles and the steps ascending
__device__ __forceinline__ void pt_product(const PtArgs &k, const PtBwd &c, int g0, int c0, float *est, const float *ds4, f32x16 &acc) {
    const int lane = threadIdx.x & 63, h = lane >> 5, q = lane & 31;
    pt_wave_sync();
#pragma unroll 8
    for (int rr = 0; rr < 32; ++rr) {
        const float *row = c.Er + (size_t)min(c0 + rr, k.C - 1) * c.Nred;
        const float v0 = row[min(g0 + lane, c.nr - 1)], v1 = row[min(g0 + 64 + lane, c.nr - 1)];
        est[rr * PT_EPITCH + lane] = (c0 + rr < k.C && g0 + lane < c.nr) ? v0 : 0.f;
        est[rr * PT_EPITCH + 64 + lane] = (c0 + rr < k.C && g0 + 64 + lane < c.nr) ? v1 : 0.f;
    }
    pt_wave_sync();
    for (int tt = 0; tt < 4 && g0 + 32 * tt < c.nr; ++tt) {
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const float a = est[q * PT_EPITCH + 32 * tt + 2 * s + h];
            const float bv = ds4[tt * 32 * PT_PITCH + q * PT_PITCH + 2 * s + h];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv, acc, 0, 0, 0);
        }
    }
}

// the accumulators of channel tiles w4 + 4 t to d_src_emb / d_tgt_emb: zero on the owned rows beyond the count
template <int NT>
__device__ __forceinline__ void pt_store_acc(const PtArgs &k, const PtBwd &c, int w4, float *dE, const f32x16 (&acc)[NT]) {
    const int lane = threadIdx.x & 63, h = lane >> 5, oi = c.o0 + (lane & 31);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int c0 = (w4 + 4 * t) * 32;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ch = c0 + pt_arow(r, h);
            if (ch < k.C && oi < c.Nown) dE[((size_t)c.b * k.C + ch) * c.Nown + oi] = oi < c.no ? acc[t][r] : 0.f;
        }
    }
}

// d_tgt of the workgroup's 32 columns: the rows of a column in the order lane halves, then the four ds wavefronts
__device__ __forceinline__ void pt_store_dx(const PtArgs &k, const PtBwd &c, int w, PtLane &l, double (*red)[32][3]) {
    const int lane = threadIdx.x & 63, h = lane >> 5, q = lane & 31, oi = c.o0 + q;
    l.dx0 += __shfl_xor(l.dx0, 32);
    l.dx1 += __shfl_xor(l.dx1, 32);
    l.dx2 += __shfl_xor(l.dx2, 32);
    if (h == 0 && w < 4) {
        red[w][q][0] = l.dx0; red[w][q][1] = l.dx1; red[w][q][2] = l.dx2;
    }
    __syncthreads();
    if (w == 0 && h == 0 && oi < k.M) {
#pragma unroll
        for (int d = 0; d < 3; ++d)
            k.dx[((size_t)c.b * 3 + d) * k.M + oi] = (float)(((red[0][q][d] + red[1][q][d]) + red[2][q][d]) + red[3][q][d]);
    }
}

// Four wavefronts, each both roles in turn: for C > 512, where a wavefront's 8 channel tiles are 128 accumulator registers
// and a second wavefront per SIMD does not fit.  NT: channel tiles per wavefront, 4 NT 32 >= C.
template <bool OWN_SRC, int NT>
__global__ __launch_bounds__(256) void pt_bwd_kernel(const PtArgs k) {
    __shared__ float dsb[4 * 32 * PT_PITCH];
    __shared__ float est[4][32 * PT_EPITCH];
    __shared__ double red[4][32][3];
    const int w = threadIdx.x >> 6;
    const PtBwd c = pt_bwd_ctx<OWN_SRC>(k);
    float *dE = OWN_SRC ? k.dse : k.dte;
    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    PtLane l = pt_lane_init<OWN_SRC>(k, c);
    for (int g0 = 0; c.o0 < c.no && g0 < c.nr; g0 += 128) {  // (workgroup-uniform)
        if (g0 + 32 * w < c.nr) pt_ds_tile<OWN_SRC>(k, c, g0 + 32 * w, dsb + w * 32 * PT_PITCH, l);
        __syncthreads();
        if (dE) {
#pragma unroll
            for (int t = 0; t < NT; ++t)
                if ((w + 4 * t) * 32 < k.C) pt_product(k, c, g0, (w + 4 * t) * 32, est[w], dsb, acc[t]);
        }
        __syncthreads();
    }
    if (dE) pt_store_acc<NT>(k, c, w, dE, acc);
    if (!OWN_SRC && k.dx) pt_store_dx(k, c, w, l, red);
}

// Eight wavefronts in two roles, for C <= 512: wavefronts 0-3 recompute the scores of group i and leave its ds in one of two
// LDS buffers while wavefronts 4-7 multiply group i - 1 from the other buffer with their channel tiles; one barrier per
// group.  A SIMD then always holds one wavefront of each role, and the loads, the double arithmetic and the LDS copy of one
// overlap the MFMAs of the other.  Every chain keeps its order: the groups are still multiplied one after the other.
template <bool OWN_SRC, int NT>
__global__ __launch_bounds__(512) void pt_bwd_pc_kernel(const PtArgs k) {
    __shared__ float dsb[2][4 * 32 * PT_PITCH];
    __shared__ float est[4][32 * PT_EPITCH];
    __shared__ double red[4][32][3];
    const int w = threadIdx.x >> 6, w4 = w & 3;
    const bool producer = w < 4;
    const PtBwd c = pt_bwd_ctx<OWN_SRC>(k);
    float *dE = OWN_SRC ? k.dse : k.dte;
    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    PtLane l = pt_lane_init<OWN_SRC>(k, c);
    const int groups = c.o0 < c.no ? (c.nr + 127) / 128 : 0;  // (workgroup-uniform)
    for (int i = 0; groups && i <= groups; ++i) {
        if (producer) {
            const int rt = 128 * i + 32 * w4;
            if (i < groups && rt < c.nr) pt_ds_tile<OWN_SRC>(k, c, rt, dsb[i & 1] + w4 * 32 * PT_PITCH, l);
        } else if (i >= 1 && dE) {
#pragma unroll
            for (int t = 0; t < NT; ++t)
                if ((w4 + 4 * t) * 32 < k.C) pt_product(k, c, 128 * (i - 1), (w4 + 4 * t) * 32, est[w4], dsb[(i - 1) & 1], acc[t]);
        }
        __syncthreads();
    }
    if (dE && !producer) pt_store_acc<NT>(k, c, w4, dE, acc);
    if (!OWN_SRC && k.dx) pt_store_dx(k, c, w, l, red);
}

static size_t pt_layout(int B, int N, int M, size_t &row_off) {
    const size_t S = ((size_t)M + RRL_POINTER_SLICE - 1) / RRL_POINTER_SLICE;
    row_off = (size_t)B * S * PT_STATE * (size_t)N;
    return (row_off + (size_t)B * PT_ROW * (size_t)N) * sizeof(double);
}

static bool pt_shape_ok(int B, int C, int N, int M) {
    return B >= 0 && B <= 32767 && C >= 1 && C <= RRL_POINTER_MAX_C && N >= 1 && N <= PT_MAX_DIM && M >= 1 && M <= PT_MAX_DIM;
}

extern "C" size_t rrl_pointer_workspace_bytes(int B, int C, int N, int M) {
    if (!pt_shape_ok(B, C, N, M)) return 0;
    size_t row_off;
    return pt_layout(B, N, M, row_off);
}

// the refusals both entries share; 0: `k` is filled
static int pt_check(const float *src_emb, const float *tgt_emb, const float *tgt, const int32_t *count_src, const int32_t *count_tgt,
                    void *ws, size_t ws_bytes, int B, int C, int N, int M, PtArgs &k) {
    if (!src_emb || !tgt_emb || !tgt || !ws || !pt_shape_ok(B, C, N, M)) return RRL_E_ARG;
    size_t row_off;
    if ((((uintptr_t)ws) & 7) != 0 || ws_bytes < pt_layout(B, N, M, row_off)) return RRL_E_WS;
    k = {};
    k.B = B; k.C = C; k.N = N; k.M = M; k.S = (M + RRL_POINTER_SLICE - 1) / RRL_POINTER_SLICE;
    k.sc = (float)(1.0 / sqrt((double)C));
    k.se = src_emb; k.te = tgt_emb; k.x = tgt; k.cs = count_src; k.ct = count_tgt;
    k.part = (double *)ws;
    k.row = (double *)ws + row_off;
    return 0;
}

extern "C" int rrl_pointer_fwd(const float *src_emb, const float *tgt_emb, const float *tgt, const int32_t *count_src,
                               const int32_t *count_tgt, void *ws, size_t ws_bytes, float *corr, float *scores, int32_t *info, int B,
                               int C, int N, int M, void *stream) {
    PtArgs k;
    if (!corr) return RRL_E_ARG;
    if (const int rc = pt_check(src_emb, tgt_emb, tgt, count_src, count_tgt, ws, ws_bytes, B, C, N, M, k)) return rc;
    if (B == 0) return 0;
    k.corr = corr; k.scores = scores; k.info = info;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(pt_fwd_kernel, dim3((unsigned)k.S, (unsigned)((N + 127) / 128), (unsigned)B), dim3(256), 0, st, k);
    hipLaunchKernelGGL(pt_finish_kernel, dim3((unsigned)B), dim3(1024), 0, st, k);
    RRL_LAUNCH_CHECK();
    return 0;
}

template <bool OWN_SRC>
static void pt_bwd_launch(const PtArgs &k, hipStream_t st) {
    const dim3 grid((unsigned)(((OWN_SRC ? k.N : k.M) + 31) / 32), (unsigned)k.B);
    const int ct = (k.C + 31) / 32;
    if (ct <= 4) hipLaunchKernelGGL((pt_bwd_pc_kernel<OWN_SRC, 1>), grid, dim3(512), 0, st, k);
    else if (ct <= 8) hipLaunchKernelGGL((pt_bwd_pc_kernel<OWN_SRC, 2>), grid, dim3(512), 0, st, k);
    else if (ct <= 16) hipLaunchKernelGGL((pt_bwd_pc_kernel<OWN_SRC, 4>), grid, dim3(512), 0, st, k);
    else hipLaunchKernelGGL((pt_bwd_kernel<OWN_SRC, 8>), grid, dim3(256), 0, st, k);
}

extern "C" int rrl_pointer_bwd(const float *src_emb, const float *tgt_emb, const float *tgt, const int32_t *count_src,
                               const int32_t *count_tgt, void *ws, size_t ws_bytes, const float *g_corr, float *d_src_emb,
                               float *d_tgt_emb, float *d_tgt, int B, int C, int N, int M, void *stream) {
    PtArgs k;
    if (!g_corr) return RRL_E_ARG;
    if (const int rc = pt_check(src_emb, tgt_emb, tgt, count_src, count_tgt, ws, ws_bytes, B, C, N, M, k)) return rc;
    if (B == 0) return 0;
    k.g = g_corr; k.dse = d_src_emb; k.dte = d_tgt_emb; k.dx = d_tgt;
    hipStream_t st = (hipStream_t)stream;
    if (d_src_emb) pt_bwd_launch<true>(k, st);
    if (d_tgt_emb || d_tgt) pt_bwd_launch<false>(k, st);
    RRL_LAUNCH_CHECK();
    return 0;
}
