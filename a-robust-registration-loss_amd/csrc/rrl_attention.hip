// rrl_attention.hip -- DCP's multi-head attention (dcp/model.py:27-34, 212-246) as two entries, rrl_attention_fwd /
// rrl_attention_bwd (include/rrl.h): out = softmax(q k^T / sqrt(DK)) v per head, token-major in and out
// ([B][N][H DK]: head h is channels h DK .. (h + 1) DK - 1 of a token's row), without the (B, H, N, M) matrix and without a
// head-major copy.  The library's first kernel that chains two matrix-core products: the weights of a 32 x 32 tile leave the
// accumulator layout of the score product through a wavefront-private LDS tile and come back as the operand of the second.
//
// One v_mfma_f32_32x32x2_f32 tile is 32 x 32 fmaf chains (rrl_pointer.hip states the layout): the A operand's 32 rows land in a
// lane's 16 accumulator registers (row at_arow(r, lane >> 5)), the B operand's 32 columns on the lanes (lane & 31); lanes 0-31
// supply reduction index 2 s, lanes 32-63 index 2 s + 1 of step s, and the accumulator is carried over the steps.
//
// The unit of ownership is the WAVEFRONT: it owns 32 query rows (or, in the column pass of the backward, 32 key columns) of one
// (sample, head) and walks the other dimension in tiles of 32, alone.  A workgroup is four such wavefronts on 128 consecutive
// rows; they share nothing but the cache, so there is no workgroup barrier anywhere.  The owned tokens are the B operand
// of the score product: a lane then owns ONE row and holds 16 of its scores, and the row's softmax is a loop over the lane's
// own registers.  The owned operand (its DK channels, <= 64 steps) stays in registers, or parked in LDS, for the whole walk;
// the walked tile's operand is gathered from the token-major rows with one float4 per two steps where DK % 4 == 0 and the
// tensors are 16-byte aligned (VEC), else with scalar loads.  The second product's A operand runs ALONG a token's channels
// (32 consecutive floats per half-wave: one cache line), its B operand is the tile of weights read back from LDS
// [own][reduced] with pitch AT_PITCH.
//
// Forward, 1 launch, and 1 more when info is asked for: at_fwd_kernel, grid (ceil(N / 128), H, B): walk 1 takes the row
// maximum, walk 2 recomputes the scores, forms p = expf(z - M), sums L in double and carries o (DK / 32 channel tiles of 16
// accumulator registers) over all column tiles; at_info_kernel, grid (B), launched only for a non-NULL info, folds the rows'
// flags (the sign of the kept 1 / L) into it.
// Backward, 1 launch per pass: at_bwd_row_kernel owns rows and writes d_q, at_bwd_col_kernel owns columns and writes d_k and d_v
// (one launch per output in the scalar-gather instantiation of four channel tiles).
// Every kernel exists per number NT = 1, 2, 4 of 32-channel tiles (DK <= 32 NT) so that its channel loops run without a branch.
#include <cstddef>
#include <cstdint>
#include <cmath>
#include <initializer_list>

#include "rrl_common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

#define AT_MAX_DIM 16384
#define AT_STEPS (RRL_ATTENTION_MAX_DK / 2)  // MFMA steps of the longest channel chain
#define AT_CT (RRL_ATTENTION_MAX_DK / 32)    // channel tiles of the second product
#define AT_PITCH 33                          // floats per LDS row of a weight tile (32 + 1: a half-wave reads one column)

struct AtArgs {
    int B, H, DK, N, M, HD;
    float sc;
    const float *q, *k, *v;
    const int32_t *cq, *ckv;
    double *ws;
    float *out, *scores;
    int32_t *info;
    const float *g, *o;
    float *dq, *dk, *dv;
};

// the accumulator register r of lane `lane` holds row at_arow(r, lane >> 5) of the A operand
__device__ __forceinline__ int at_arow(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

__device__ __forceinline__ f32x16 at_zero() {
    const f32x16 z = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    return z;
}

// LDS writes of a wavefront made visible to its own other lanes (the tile is private to the wavefront: no workgroup barrier)
__device__ __forceinline__ void at_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Every kernel is instantiated for NT = 1, 2, 4 channel tiles of 32 (DK <= 32 NT): its loops over the channels have no
// branch, so a gather, a chain or a product is ONE basic block that the compiler can schedule -- loads first, MFMAs behind
// them.  Channels at or beyond DK are zero in BOTH operands (a zero step leaves a chain as it is).

// a value pinned to a register where it stands: the load that made it is issued here, not sunk into the select that uses it
__device__ __forceinline__ void at_pin(float &x) { asm volatile("" : "+v"(x)); }

// The channel-chain operand of one token for this lane: r[s] = channel 2 s + (lane >> 5) of the head's DK channels at token t
// of the head-based X (row length HD: always a readable row, the caller clamps it), 0 where the token is not valid and on
// the channels at or beyond DK (their loads go to a clamped address).
template <bool VEC, int NT>
__device__ __forceinline__ void at_gather(const float *__restrict__ X, int t, int HD, bool valid, int DK, float (&r)[16 * NT]) {
    const int h = (threadIdx.x & 63) >> 5;
    const unsigned off = (unsigned)t * (unsigned)HD;  // (below 2^25: a uniform base and a 32-bit lane offset address every load)
    if (VEC) {
#pragma unroll
        for (int grp = 0; grp < NT; ++grp) {  // eight float4 in flight at a time
            float4 e[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) e[i] = *reinterpret_cast<const float4 *>(X + (off + (unsigned)min(32 * grp + 4 * i, DK - 4)));
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const bool v = valid && 32 * grp + 4 * i < DK;
                at_pin(e[i].x);
                r[16 * grp + 2 * i] = v ? (h ? e[i].y : e[i].x) : 0.f;
                r[16 * grp + 2 * i + 1] = v ? (h ? e[i].w : e[i].z) : 0.f;
            }
        }
    } else {
#pragma unroll
        for (int grp = 0; grp < 2 * NT; ++grp) {  // eight loads in flight at a time
            float e[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) e[i] = X[off + (unsigned)min(16 * grp + 2 * i + h, DK - 1)];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                at_pin(e[i]);
                r[8 * grp + i] = valid && 16 * grp + 2 * i + h < DK ? e[i] : 0.f;
            }
        }
    }
}

// 32 x 32 channel chains: ONE fmaf chain per entry over the channels ascending from +0, never cut
template <int NT>
__device__ __forceinline__ f32x16 at_chain(const float (&a)[16 * NT], const float (&b)[16 * NT]) {
    f32x16 acc = at_zero();
#pragma unroll
    for (int s = 0; s < 16 * NT; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b[s], acc, 0, 0, 0);
    return acc;
}

// The same chains with the B operand parked in LDS: `own` is the lane's own column of a [AT_STEPS][64] array that the lane filled
// itself with at_park (what it reads it wrote: no synchronisation, no bank conflict).  The backward holds two owned operands
// and two sets of accumulators; the second operand lives here so that no instantiation needs scratch memory.
template <int NT>
__device__ __forceinline__ void at_park(const float (&r)[16 * NT], float *own) {
#pragma unroll
    for (int s = 0; s < 16 * NT; ++s) own[64 * s] = r[s];
}
template <int NT>
__device__ __forceinline__ f32x16 at_chain_parked(const float (&a)[16 * NT], const float *own) {
    f32x16 acc = at_zero();
#pragma unroll
    for (int s = 0; s < 16 * NT; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], own[64 * s], acc, 0, 0, 0);
    return acc;
}

// acc[ct][.] += X^T W for one tile: X the token-major rows t0 .. t0 + 31 of a head (row length HD, nr valid rows, t0 < nr),
// W the weight tile in LDS [own][reduced]: entry (channel, own) is continued by the 32 reduced indices ascending.  Rows at
// or beyond nr and channels at or beyond DK are zero in the operand (their lanes load a clamped address).  A channel tile's
// 16 loads are issued together, the next tile's before this tile's MFMAs (AHEAD; behind them where registers are short).
template <int NT, bool AHEAD = true>
__device__ __forceinline__ void at_product(const float *__restrict__ X, int HD, int t0, int nr, int DK, const float *tile,
                                           f32x16 (&acc)[NT]) {
    const int lane = threadIdx.x & 63, h = lane >> 5, q = lane & 31;
    float w[16], x[NT][16];
    unsigned row[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        w[s] = tile[q * AT_PITCH + 2 * s + h];
        row[s] = (unsigned)min(t0 + 2 * s + h, nr - 1) * (unsigned)HD;
    }
#pragma unroll
    for (int s = 0; s < 16; ++s) x[0][s] = X[row[s] + (unsigned)min(q, DK - 1)];
#pragma unroll
    for (int ct = 0; ct < NT; ++ct) {
        if (AHEAD && ct + 1 < NT) {
#pragma unroll
            for (int s = 0; s < 16; ++s) x[ct + 1][s] = X[row[s] + (unsigned)min(32 * (ct + 1) + q, DK - 1)];
        }
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            at_pin(x[ct][s]);
            acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(32 * ct + q < DK && t0 + 2 * s + h < nr ? x[ct][s] : 0.f, w[s], acc[ct], 0, 0, 0);
        }
        if (!AHEAD && ct + 1 < NT) {
#pragma unroll
            for (int s = 0; s < 16; ++s) x[ct + 1][s] = X[row[s] + (unsigned)min(32 * (ct + 1) + q, DK - 1)];
        }
    }
}

// what a wavefront knows of its place: sample, head, the counts, the heads' bases and its own 32 tokens
struct AtCtx {
    int b, hd, nq, nt, own0;
    const float *Q, *K, *V;
    double *ws;  // the head's rows: M_j at [j], +-1 / L_j at [N + j]
};
__device__ __forceinline__ AtCtx at_ctx(const AtArgs &a) {
    AtCtx c;
    c.b = blockIdx.z;
    c.hd = blockIdx.y;
    c.nq = rrl_rows(a.cq, c.b, a.N);
    c.nt = rrl_rows(a.ckv, c.b, a.M);
    c.own0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 32;
    c.Q = a.q + (size_t)c.b * a.N * a.HD + c.hd * a.DK;
    c.K = a.k + (size_t)c.b * a.M * a.HD + c.hd * a.DK;
    c.V = a.v + (size_t)c.b * a.M * a.HD + c.hd * a.DK;
    c.ws = a.ws ? a.ws + ((size_t)c.b * a.H + c.hd) * 2 * a.N : nullptr;
    return c;
}

// the head's DK channels of tokens t0 .. t0 + 31 (those below `cap`) of a token-major output, zeroed by the whole wavefront
__device__ __forceinline__ void at_zero_rows(float *X, int HD, int DK, int t0, int cap) {
    const int lane = threadIdx.x & 63;
    for (int t = t0; t < min(t0 + 32, cap); ++t)
        for (int c = lane; c < DK; c += 64) X[(size_t)t * HD + c] = 0.f;
}

// the accumulators of the second product to a token-major output: the lane's own token, zero where it is not valid
template <int NT>
__device__ __forceinline__ void at_store_acc(float *X, int HD, int DK, int t, bool valid, int cap, const f32x16 (&acc)[NT]) {
    const int h = (threadIdx.x & 63) >> 5;
    if (t >= cap) return;
#pragma unroll
    for (int ct = 0; ct < NT; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int c = 32 * ct + at_arow(r, h);
            if (c < DK) X[(size_t)t * HD + c] = valid ? acc[ct][r] : 0.f;
        }
}

template <bool VEC, int NT>
__global__ __launch_bounds__(256) void at_fwd_kernel(const AtArgs a) {
    __shared__ float tiles[4][32 * AT_PITCH];
    const AtCtx c = at_ctx(a);
    const int lane = threadIdx.x & 63, h = lane >> 5, q = lane & 31, j = c.own0 + q;
    if (c.own0 >= a.N) return;  // (wavefront-uniform, as every return and loop bound below: there is no workgroup barrier)
    float *out = a.out + (size_t)c.b * a.N * a.HD + c.hd * a.DK;
    if (c.own0 >= c.nq || c.nt == 0) {
        at_zero_rows(out, a.HD, a.DK, c.own0, a.N);
        if (h == 0 && j < a.N) {
            c.ws[j] = 0.0;
            c.ws[a.N + j] = 0.0;
        }
        return;
    }
    const bool vj = j < c.nq;
    float *tile = tiles[threadIdx.x >> 6];
    float qr[16 * NT], kr[16 * NT];
    at_gather<VEC, NT>(c.Q, min(j, c.nq - 1), a.HD, vj, a.DK, qr);
    // walk 1: the row's maximum over all its columns, before any term is formed
    float m = -INFINITY;
    int flag = 0;
    at_gather<VEC, NT>(c.K, min(q, c.nt - 1), a.HD, q < c.nt, a.DK, kr);
    for (int kt = 0; kt < c.nt; kt += 32) {
        const f32x16 ch = at_chain<NT>(kr, qr);
        if (kt + 32 < c.nt) at_gather<VEC, NT>(c.K, min(kt + 32 + q, c.nt - 1), a.HD, kt + 32 + q < c.nt, a.DK, kr);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float z = ch[r] * a.sc;
            if (kt + at_arow(r, h) < c.nt) {
                m = fmaxf(m, z);
                flag |= !(fabsf(z) < INFINITY);
            }
        }
    }
    m = fmaxf(m, __shfl_xor(m, 32));
    // walk 2: the same scores again, p = expf(z - M), L in double, o carried over all column tiles
    f32x16 acc[NT];
#pragma unroll
    for (int ct = 0; ct < NT; ++ct) acc[ct] = at_zero();
    double L = 0.0;
    at_gather<VEC, NT>(c.K, min(q, c.nt - 1), a.HD, q < c.nt, a.DK, kr);
    for (int kt = 0; kt < c.nt; kt += 32) {
        const f32x16 ch = at_chain<NT>(kr, qr);
        if (kt + 32 < c.nt) at_gather<VEC, NT>(c.K, min(kt + 32 + q, c.nt - 1), a.HD, kt + 32 + q < c.nt, a.DK, kr);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float z = ch[r] * a.sc;
            const float p = (kt + at_arow(r, h) < c.nt && z != -INFINITY) ? expf(z - m) : 0.f;  // (never -inf - -inf)
            L += (double)p;
            tile[q * AT_PITCH + at_arow(r, h)] = p;
        }
        at_wave_sync();
        at_product<NT>(c.V, a.HD, kt, c.nt, a.DK, tile, acc);
        at_wave_sync();
    }
    L += __shfl_xor(L, 32);  // (the lane halves' sums: a + b == b + a, both halves hold the row's L)
#pragma unroll
    for (int ct = 0; ct < NT; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float o = (float)((double)acc[ct][r] / L);
            if (32 * ct + at_arow(r, h) < a.DK) flag |= !(fabsf(o) < INFINITY);
            acc[ct][r] = o;
        }
    at_store_acc<NT>(out, a.HD, a.DK, j, vj, a.N, acc);
    flag |= __shfl_xor(flag, 32);
    if (h == 0 && j < a.N) {  // the row's flag travels as the sign of 1 / L (L >= 1, or NaN)
        c.ws[j] = vj ? (double)m : 0.0;
        c.ws[a.N + j] = vj ? copysign(1.0 / L, flag ? -1.0 : 1.0) : 0.0;
    }
}

__global__ __launch_bounds__(256) void at_info_kernel(const AtArgs a) {
    const int b = blockIdx.x;
    int flag = 0;
    for (int i = threadIdx.x; i < a.H * a.N; i += 256)
        flag |= signbit(a.ws[((size_t)b * a.H + i / a.N) * 2 * a.N + a.N + i % a.N]) ? 1 : 0;
    flag = __syncthreads_or(flag);
    if (threadIdx.x == 0) a.info[b] = flag ? 1 : 0;
}

// the scaled scores alone, by the same gather and the same chain: [B][H][N][M], -inf at and beyond the counts (tests only)
template <bool VEC, int NT>
__global__ __launch_bounds__(256) void at_scores_kernel(const AtArgs a) {
    const AtCtx c = at_ctx(a);
    const int lane = threadIdx.x & 63, h = lane >> 5, q = lane & 31, j = c.own0 + q;
    if (c.own0 >= a.N) return;
    float *z = a.scores + ((size_t)c.b * a.H + c.hd) * a.N * a.M;
    float qr[16 * NT], kr[16 * NT];
    const bool live = c.own0 < c.nq && c.nt > 0;
    if (live) at_gather<VEC, NT>(c.Q, min(j, c.nq - 1), a.HD, j < c.nq, a.DK, qr);
    for (int kt = 0; kt < a.M; kt += 32) {
        f32x16 ch = at_zero();
        if (live && kt < c.nt) {
            at_gather<VEC, NT>(c.K, min(kt + q, c.nt - 1), a.HD, kt + q < c.nt, a.DK, kr);
            ch = at_chain<NT>(kr, qr);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int col = kt + at_arow(r, h);
            if (j < a.N && col < a.M) z[(size_t)j * a.M + col] = (j < c.nq && col < c.nt) ? ch[r] * a.sc : -INFINITY;
        }
    }
}

// delta = sum_c g[c] out[c] in double, c ascending, of one token's head slice (the products are exact in double)
__device__ __forceinline__ double at_delta(const float *__restrict__ g, const float *__restrict__ o, int DK) {
    double d = 0.0;
    for (int c = 0; c < DK; ++c) d = fma((double)g[c], (double)o[c], d);
    return d;
}

// one weight of the backward: Pn = float32(double(expf(z - M)) (1 / L)), ds = float32(double(Pn) (double(dP) - delta) sc)
__device__ __forceinline__ void at_weights(float ch, float dp, float sc, float m, double invL, double delta, bool valid, float &Pn,
                                           float &ds) {
    const float z = ch * sc;
    const float e = z == -INFINITY ? 0.f : expf(z - m);
    Pn = valid ? (float)((double)e * invL) : 0.f;
    ds = valid ? (float)((double)Pn * ((double)dp - delta) * (double)sc) : 0.f;
}

// owns 32 query rows, walks every column: d_q[j][c] = the chain over k ascending of ds[j][k] k[k][c]
template <bool VEC, int NT>
__global__ __launch_bounds__(256) void at_bwd_row_kernel(const AtArgs a) {
    __shared__ float tiles[4][32 * AT_PITCH];
    __shared__ float parked[4][AT_STEPS * 64];
    const AtCtx c = at_ctx(a);
    const int lane = threadIdx.x & 63, h = lane >> 5, q = lane & 31, j = c.own0 + q;
    if (c.own0 >= a.N) return;
    float *dq = a.dq + (size_t)c.b * a.N * a.HD + c.hd * a.DK;
    if (c.own0 >= c.nq || c.nt == 0) {
        at_zero_rows(dq, a.HD, a.DK, c.own0, a.N);
        return;
    }
    const bool vj = j < c.nq;
    const int jc = min(j, c.nq - 1);
    float *tile = tiles[threadIdx.x >> 6];
    const float *G = a.g + (size_t)c.b * a.N * a.HD + c.hd * a.DK, *O = a.o + (size_t)c.b * a.N * a.HD + c.hd * a.DK;
    float *gr = parked[threadIdx.x >> 6] + lane;
    float qr[16 * NT], xr[16 * NT];
    at_gather<VEC, NT>(G, jc, a.HD, vj, a.DK, xr);
    at_park<NT>(xr, gr);
    at_gather<VEC, NT>(c.Q, jc, a.HD, vj, a.DK, qr);
    const float m = (float)c.ws[jc];
    const double invL = fabs(c.ws[a.N + jc]), delta = at_delta(G + (size_t)jc * a.HD, O + (size_t)jc * a.HD, a.DK);
    f32x16 acc[NT];
#pragma unroll
    for (int ct = 0; ct < NT; ++ct) acc[ct] = at_zero();
    for (int kt = 0; kt < c.nt; kt += 32) {
        at_gather<VEC, NT>(c.K, min(kt + q, c.nt - 1), a.HD, kt + q < c.nt, a.DK, xr);
        const f32x16 ch = at_chain<NT>(xr, qr);
        at_gather<VEC, NT>(c.V, min(kt + q, c.nt - 1), a.HD, kt + q < c.nt, a.DK, xr);
        const f32x16 dp = at_chain_parked<NT>(xr, gr);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float Pn, ds;
            at_weights(ch[r], dp[r], a.sc, m, invL, delta, vj && kt + at_arow(r, h) < c.nt, Pn, ds);
            tile[q * AT_PITCH + at_arow(r, h)] = ds;
        }
        at_wave_sync();
        at_product<NT>(c.K, a.HD, kt, c.nt, a.DK, tile, acc);
        at_wave_sync();
    }
    at_store_acc<NT>(dq, a.HD, a.DK, j, vj, a.N, acc);
}

// owns 32 key columns, walks every row: d_v[k][c] = the chain over j ascending of Pn[j][k] g[j][c], d_k[k][c] of ds[j][k] q[j][c]
// WHICH: 0 both outputs, 1 d_v alone, 2 d_k alone -- the scalar-gather instantiation of four channel tiles holds one set of
// accumulators per launch (two launches, the same chains, the same bits): with both it would need scratch memory
template <bool VEC, int NT, int WHICH>
__global__ __launch_bounds__(256) void at_bwd_col_kernel(const AtArgs a) {
    __shared__ float tiles[4][32 * AT_PITCH];
    __shared__ float parked[4][2][AT_STEPS * 64];
    const AtCtx c = at_ctx(a);
    const int lane = threadIdx.x & 63, h = lane >> 5, q = lane & 31, kc = c.own0 + q;
    if (c.own0 >= a.M) return;
    float *dk = WHICH != 1 && a.dk ? a.dk + (size_t)c.b * a.M * a.HD + c.hd * a.DK : nullptr;
    float *dv = WHICH != 2 && a.dv ? a.dv + (size_t)c.b * a.M * a.HD + c.hd * a.DK : nullptr;
    if (c.own0 >= c.nt || c.nq == 0) {
        if (dk) at_zero_rows(dk, a.HD, a.DK, c.own0, a.M);
        if (dv) at_zero_rows(dv, a.HD, a.DK, c.own0, a.M);
        return;
    }
    const bool vk = kc < c.nt;
    float *tile = tiles[threadIdx.x >> 6];
    const float *G = a.g + (size_t)c.b * a.N * a.HD + c.hd * a.DK, *O = a.o + (size_t)c.b * a.N * a.HD + c.hd * a.DK;
    float *kr = parked[threadIdx.x >> 6][0] + lane, *vr = parked[threadIdx.x >> 6][1] + lane;  // both owned operands are parked
    float xr[16 * NT];
    at_gather<VEC, NT>(c.K, min(kc, c.nt - 1), a.HD, vk, a.DK, xr);
    at_park<NT>(xr, kr);
    if (dk) {
        at_gather<VEC, NT>(c.V, min(kc, c.nt - 1), a.HD, vk, a.DK, xr);
        at_park<NT>(xr, vr);
    }
    f32x16 accv[NT], acck[NT];
#pragma unroll
    for (int ct = 0; ct < NT; ++ct) accv[ct] = acck[ct] = at_zero();
    for (int jt = 0; jt < c.nq; jt += 32) {
        const int jr = min(jt + q, c.nq - 1);  // the row this lane fetches the row quantities of
        at_gather<VEC, NT>(c.Q, jr, a.HD, jt + q < c.nq, a.DK, xr);
        const f32x16 ch = at_chain_parked<NT>(xr, kr);
        f32x16 dp = at_zero();
        double delta_q = 0.0;
        if (dk) {
            at_gather<VEC, NT>(G, jr, a.HD, jt + q < c.nq, a.DK, xr);
            dp = at_chain_parked<NT>(xr, vr);
            delta_q = at_delta(G + (size_t)jr * a.HD, O + (size_t)jr * a.HD, a.DK);
        }
        const float m_q = (float)c.ws[jr];
        const double invL_q = fabs(c.ws[a.N + jr]);
        float ds[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rl = at_arow(r, h);
            const float m = __shfl(m_q, rl);
            const double invL = __shfl(invL_q, rl), delta = __shfl(delta_q, rl);
            float Pn;
            at_weights(ch[r], dp[r], a.sc, m, invL, delta, vk && jt + rl < c.nq, Pn, ds[r]);
            tile[q * AT_PITCH + rl] = Pn;
        }
        at_wave_sync();
        if (dv) at_product<NT, VEC>(G, a.HD, jt, c.nq, a.DK, tile, accv);
        at_wave_sync();
        if (dk) {  // the one tile again, now with ds
#pragma unroll
            for (int r = 0; r < 16; ++r) tile[q * AT_PITCH + at_arow(r, h)] = ds[r];
            at_wave_sync();
            at_product<NT, VEC>(c.Q, a.HD, jt, c.nq, a.DK, tile, acck);
            at_wave_sync();
        }
    }
    if (dv) at_store_acc<NT>(dv, a.HD, a.DK, kc, vk, a.M, accv);
    if (dk) at_store_acc<NT>(dk, a.HD, a.DK, kc, vk, a.M, acck);
}

static bool at_shape_ok(int B, int H, int DK, int N, int M) {
    return B >= 0 && B <= 32767 && H >= 1 && H <= 16 && DK >= 1 && DK <= RRL_ATTENTION_MAX_DK && N >= 1 && N <= AT_MAX_DIM && M >= 1 &&
           M <= AT_MAX_DIM;
}

static size_t at_bytes(int B, int H, int N) { return (size_t)B * H * 2 * (size_t)N * sizeof(double); }

extern "C" size_t rrl_attention_workspace_bytes(int B, int H, int N, int M) {
    return at_shape_ok(B, H, 1, N, M) ? at_bytes(B, H, N) : 0;
}

// one of a kernel's six instantiations: VEC by the alignment, NT by DK
#define AT_LAUNCH(KERNEL, vec, grid, st, a)                                                              \
    do {                                                                                                 \
        const int nt__ = (a).DK <= 32 ? 1 : (a).DK <= 64 ? 2 : 4;                                        \
        if (vec) {                                                                                       \
            if (nt__ == 1) hipLaunchKernelGGL((KERNEL<true, 1>), grid, dim3(256), 0, st, a);             \
            else if (nt__ == 2) hipLaunchKernelGGL((KERNEL<true, 2>), grid, dim3(256), 0, st, a);        \
            else hipLaunchKernelGGL((KERNEL<true, 4>), grid, dim3(256), 0, st, a);                       \
        } else {                                                                                         \
            if (nt__ == 1) hipLaunchKernelGGL((KERNEL<false, 1>), grid, dim3(256), 0, st, a);            \
            else if (nt__ == 2) hipLaunchKernelGGL((KERNEL<false, 2>), grid, dim3(256), 0, st, a);       \
            else hipLaunchKernelGGL((KERNEL<false, 4>), grid, dim3(256), 0, st, a);                      \
        }                                                                                                \
    } while (0)

static bool at_vec(int DK, std::initializer_list<const void *> ptrs) {
    bool ok = DK % 4 == 0;
    for (const void *p : ptrs) ok = ok && (((uintptr_t)p) & 15) == 0;
    return ok;
}

// the refusals the entries share; 0: `k` is filled
static int at_check(const float *q, const float *k, const float *v, const int32_t *count_q, const int32_t *count_kv, void *ws,
                    size_t ws_bytes, int B, int H, int DK, int N, int M, AtArgs &a) {
    if (!q || !k || !v || !ws || !at_shape_ok(B, H, DK, N, M)) return RRL_E_ARG;
    if ((((uintptr_t)ws) & 7) != 0 || ws_bytes < at_bytes(B, H, N)) return RRL_E_WS;
    a = {};
    a.B = B; a.H = H; a.DK = DK; a.N = N; a.M = M; a.HD = H * DK;
    a.sc = (float)(1.0 / sqrt((double)DK));
    a.q = q; a.k = k; a.v = v; a.cq = count_q; a.ckv = count_kv;
    a.ws = (double *)ws;
    return 0;
}

extern "C" int rrl_attention_fwd(const float *q, const float *k, const float *v, const int32_t *count_q, const int32_t *count_kv,
                                 void *ws, size_t ws_bytes, float *out, int32_t *info, int B, int H, int DK, int N, int M,
                                 void *stream) {
    AtArgs a;
    if (!out) return RRL_E_ARG;
    if (const int rc = at_check(q, k, v, count_q, count_kv, ws, ws_bytes, B, H, DK, N, M, a)) return rc;
    if (B == 0) return 0;
    a.out = out; a.info = info;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((N + 127) / 128), (unsigned)H, (unsigned)B);
    AT_LAUNCH(at_fwd_kernel, at_vec(DK, {q, k, v}), grid, st, a);
    if (info) hipLaunchKernelGGL(at_info_kernel, dim3((unsigned)B), dim3(256), 0, st, a);
    RRL_LAUNCH_CHECK();
    return 0;
}

extern "C" int rrl_attention_scores(const float *q, const float *k, const int32_t *count_q, const int32_t *count_kv, float *scores,
                                    int B, int H, int DK, int N, int M, void *stream) {
    if (!q || !k || !scores || !at_shape_ok(B, H, DK, N, M)) return RRL_E_ARG;
    if (B == 0) return 0;
    AtArgs a = {};
    a.B = B; a.H = H; a.DK = DK; a.N = N; a.M = M; a.HD = H * DK;
    a.sc = (float)(1.0 / sqrt((double)DK));
    a.q = q; a.k = k; a.v = k; a.cq = count_q; a.ckv = count_kv; a.scores = scores;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((N + 127) / 128), (unsigned)H, (unsigned)B);
    AT_LAUNCH(at_scores_kernel, at_vec(DK, {q, k}), grid, st, a);
    RRL_LAUNCH_CHECK();
    return 0;
}

extern "C" int rrl_attention_bwd(const float *q, const float *k, const float *v, const int32_t *count_q, const int32_t *count_kv,
                                 void *ws, size_t ws_bytes, const float *out, const float *g_out, float *d_q, float *d_k, float *d_v,
                                 int B, int H, int DK, int N, int M, void *stream) {
    AtArgs a;
    if (!out || !g_out) return RRL_E_ARG;
    if (const int rc = at_check(q, k, v, count_q, count_kv, ws, ws_bytes, B, H, DK, N, M, a)) return rc;
    if (B == 0) return 0;
    a.o = out; a.g = g_out; a.dq = d_q; a.dk = d_k; a.dv = d_v;
    hipStream_t st = (hipStream_t)stream;
    const bool vec = at_vec(DK, {q, k, v, g_out});
    if (d_q) {
        const dim3 grid((unsigned)((N + 127) / 128), (unsigned)H, (unsigned)B);
        AT_LAUNCH(at_bwd_row_kernel, vec, grid, st, a);
    }
    if (d_k || d_v) {
        const dim3 grid((unsigned)((M + 127) / 128), (unsigned)H, (unsigned)B);
        const int nt = DK <= 32 ? 1 : DK <= 64 ? 2 : 4;
        if (vec && nt == 1) hipLaunchKernelGGL((at_bwd_col_kernel<true, 1, 0>), grid, dim3(256), 0, st, a);
        else if (vec && nt == 2) hipLaunchKernelGGL((at_bwd_col_kernel<true, 2, 0>), grid, dim3(256), 0, st, a);
        else if (vec) hipLaunchKernelGGL((at_bwd_col_kernel<true, 4, 0>), grid, dim3(256), 0, st, a);
        else if (nt == 1) hipLaunchKernelGGL((at_bwd_col_kernel<false, 1, 0>), grid, dim3(256), 0, st, a);
        else if (nt == 2) hipLaunchKernelGGL((at_bwd_col_kernel<false, 2, 0>), grid, dim3(256), 0, st, a);
        else {
            if (d_v) hipLaunchKernelGGL((at_bwd_col_kernel<false, 4, 1>), grid, dim3(256), 0, st, a);
            if (d_k) hipLaunchKernelGGL((at_bwd_col_kernel<false, 4, 2>), grid, dim3(256), 0, st, a);
        }
    }
    RRL_LAUNCH_CHECK();
    return 0;
}
