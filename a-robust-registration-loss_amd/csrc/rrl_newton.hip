// rrl_newton.hip -- the second-order pose path (include/rrl.h rrl_pose_normal_eq, rrl_se3_newton_step_batch; DESIGN.md
// section 15): the loss with its weights frozen for one step is a weighted point-to-point problem,
//     sum_i a_i |Q1_i - Q2_i|^2,     a_i = dL/dD_i  (what the backward calls gD, upstream gradient 1),
// over the selected pairs i = (line, source hit h, target hit o), and Q1 = sum_k (w_k / 3)(x_k R + T) is affine in the pose:
// under a world-frame twist (omega, v), dQ1 = omega x Q1 + s v with s = (w_0 + w_1 + w_2) / 3.  Its Gauss-Newton normal
// equations need sixteen sums per pair of clouds,
//     S_QQ (6) = sum 2a Q Q^T,  S_sQ (3) = sum 2a s Q,  S_ss = sum 2a s^2,  g_w (3) = sum 2a Q x e,  g_v (3) = sum 2a s e,
// (e = Q1 - Q2, Q = Q1), which pose_normal_eq_kernel takes from the workspace a registration forward left, and
// se3_newton_step_kernel turns into one damped, clamped step per pose, composed onto (R, T), with the log row, the next
// sampler box and the stopping rule of a registration epoch.
#include <cstddef>
#include <cstdint>

#include "rrl_ws.h"
#include "rrl_pose_tail.h"
#include "rrl_pose_solve.h"
#include "rrl_pair_sums.h"

#define NEQ_LINES 64  // selected lines per 256-lane workgroup (four hit slots each): loss_bwd_rt_kernel's BWD_LINES
#define NEQ_SUBS 16   // workgroups per 1024-line tile: every selected line of a tile has one (64 x 16 = 1024)
#define NEQ_SUMS RRL_NEQ_SUMS

struct NeqArgs {
    const uint8_t *kj;
    const float *w1;
    const float4 *Q1, *Q2;
    const float *D, *med;
    const int32_t *bcnt, *info;
    double *part;  // [B][gridDim.x][NEQ_SUMS]
    int L;
};

// Grid (NEQ_SUBS x line tiles, B), the deterministic direct backward's (loss_bwd_rt_body<true>, rrl_stage_bwd.h): workgroup
// (tile, sub) takes the selected lines of its 1024-line tile with rank 64 sub .. 64 sub + 63 in a FIXED order (round r, then
// thread), found from the tile's KJ bytes -- never from SEL, whose order is that of an atomic.  Four lanes per line, lane h =
// source hit slot h; the Welsch row of a hit travels by quad DPP.  The expressions for er, the first-occurrence argmins, sw and
// gD are bwd_rt_math's, statement for statement: a pair carries weight here exactly when it carries gradient there.  Every term
// is one float32 expression; the sums are double from the lane on.  Each workgroup stores its sixteen sums (zeros when it holds
// no line): nothing to clear, no atomics.
__global__ __launch_bounds__(256) void pose_normal_eq_kernel(const NeqArgs a) {
    __shared__ int s_line[NEQ_LINES];
    __shared__ int s_wc[4][4];
    __shared__ double s_red[4][NEQ_SUMS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int bx = blockIdx.x, b = blockIdx.y, L = a.L;
    const int h = tid & 3;
    const int tile = bx / NEQ_SUBS, sub = bx % NEQ_SUBS;
    const uint8_t *__restrict__ kj = a.kj;
    bool sl[4];
    unsigned long long bm[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int l = tile * 1024 + r * 256 + tid;
        sl[r] = l < L && kj[(size_t)b * L + l] != 0;
        bm[r] = __ballot(sl[r]);
        if (lane == 0) s_wc[r][wave] = __popcll(bm[r]);
    }
    if (tid < NEQ_LINES) s_line[tid] = -1;
    __syncthreads();
    int before = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        int mine = before;
        for (int w = 0; w < 4; ++w) {
            if (w < wave) mine += s_wc[r][w];
            before += s_wc[r][w];
        }
        const int rel = mine + __popcll(bm[r] & ((1ull << lane) - 1ull)) - NEQ_LINES * sub;
        if (sl[r] && rel >= 0 && rel < NEQ_LINES) s_line[rel] = tile * 1024 + r * 256 + tid;
    }
    __syncthreads();
    const int li = s_line[tid >> 2];

    // ---- the line's fields (bwd_rt_line without the source triangle: nothing of a cloud is read)
    const int C = a.info[b * 4];
    const size_t gl = (size_t)b * L + (li >= 0 ? li : 0);
    const unsigned c = (li >= 0 && C > 0) ? kj[gl] : 0u;
    int k = c & 15, j = c >> 4;
    const bool valid = k >= 1 && j >= 1 && k <= RRL_MAX_HITS && j <= RRL_MAX_HITS;  // (a byte the per-line stage cannot write: no line)
    if (!valid) k = j = 0;
    const bool live = valid && h < k;
    const float m = a.med[b];
    float dr[4] = {INFINITY, INFINITY, INFINITY, INFINITY};
    float4 mine = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float qx[4] = {0.0f, 0.0f, 0.0f, 0.0f}, qy[4] = {0.0f, 0.0f, 0.0f, 0.0f}, qz[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    float wq[3] = {0.0f, 0.0f, 0.0f};
    int S = 1;
    if (live) {
#pragma unroll
        for (int o = 0; o < RRL_MAX_HITS; ++o)
            if (o < j) {
                dr[o] = a.D[gl * 16 + h * j + o];
                const float4 t = a.Q2[gl * 4 + o];
                qx[o] = t.x; qy[o] = t.y; qz[o] = t.z;
            }
        S = a.bcnt[b * 16 + (k - 1) * 4 + (j - 1)];
        mine = a.Q1[gl * 4 + h];
        const float *w = a.w1 + (gl * 4 + h) * 3;
#pragma unroll
        for (int q = 0; q < 3; ++q) wq[q] = w[q];
    }

    // ---- the Welsch row, the argmins (bwd_rt_math; all lanes take part in the DPP exchange)
    const int jmax = (int)wave_max((float)j);  // uniform
    float er[4] = {0.0f, 0.0f, 0.0f, 0.0f}, wr[4];
#pragma unroll
    for (int o = 0; o < RRL_MAX_HITS; ++o) {
        wr[o] = INFINITY;
        if (o < jmax) {
            const float e = expf(-(dr[o] / m) / 2.0f);  // == welsch(): 1 - e
            er[o] = e;
            if (dr[o] < INFINITY) wr[o] = 1.0f - e;
        }
    }
    int arg_b_own = 0, arg_a[4];
    {
        float bestw = wr[0];
#pragma unroll
        for (int o = 1; o < RRL_MAX_HITS; ++o)
            if (wr[o] < bestw) { bestw = wr[o]; arg_b_own = o; }
#pragma unroll
        for (int o = 0; o < RRL_MAX_HITS; ++o) {
            const float w0 = quad_bcast<0>(wr[o]), w1_ = quad_bcast<1>(wr[o]), w2_ = quad_bcast<2>(wr[o]), w3 = quad_bcast<3>(wr[o]);
            float best = w0;
            int mm = 0;
            if (w1_ < best) { best = w1_; mm = 1; }
            if (w2_ < best) { best = w2_; mm = 2; }
            if (w3 < best) { best = w3; mm = 3; }
            arg_a[o] = mm;
        }
    }
    double acc[NEQ_SUMS];
#pragma unroll
    for (int q = 0; q < NEQ_SUMS; ++q) acc[q] = 0.0;
    if (live) {
        const float wkj = expf(-0.5f * (float)abs(k - j));
        const float scale = 1.0f * wkj / (float)C;  // (upstream gradient 1)
        const float inv_row = 1.0f / ((float)S * (float)k), inv_col = 1.0f / ((float)S * (float)j);
        const float s = ((wq[0] + wq[1]) + wq[2]) / 3.0f;
        const float Qx = mine.x, Qy = mine.y, Qz = mine.z;
#pragma unroll
        for (int o = 0; o < RRL_MAX_HITS; ++o) {
            if (o >= j) continue;
            float sw = 0.0f;
            if (arg_b_own == o) sw += inv_row;
            if (arg_a[o] == h) sw += inv_col;
            if (sw == 0.0f) continue;
            const float gD = scale * sw * er[o] / (2.0f * m);  // same expressions as loss_bwd_rt_kernel
            const float a2 = 2.0f * gD;
            const float ex = Qx - qx[o], ey = Qy - qy[o], ez = Qz - qz[o];
            const float as = a2 * s;
            acc[0] += (double)((a2 * Qx) * Qx);
            acc[1] += (double)((a2 * Qx) * Qy);
            acc[2] += (double)((a2 * Qx) * Qz);
            acc[3] += (double)((a2 * Qy) * Qy);
            acc[4] += (double)((a2 * Qy) * Qz);
            acc[5] += (double)((a2 * Qz) * Qz);
            acc[6] += (double)(as * Qx);
            acc[7] += (double)(as * Qy);
            acc[8] += (double)(as * Qz);
            acc[9] += (double)(as * s);
            // Q x e: each product is a term of its own (the difference of two rounded products would carry their cancellation)
            acc[10] += (double)((a2 * Qy) * ez); acc[10] -= (double)((a2 * Qz) * ey);
            acc[11] += (double)((a2 * Qz) * ex); acc[11] -= (double)((a2 * Qx) * ez);
            acc[12] += (double)((a2 * Qx) * ey); acc[12] -= (double)((a2 * Qy) * ex);
            acc[13] += (double)(as * ex);
            acc[14] += (double)(as * ey);
            acc[15] += (double)(as * ez);
        }
    }
    block_sum_d(acc, s_red, a.part + ((size_t)b * gridDim.x + bx) * NEQ_SUMS);
}

// The fixed-order tail (a launch of its own, like loss_bwd_rt_finalize_kernel: the stream orders it behind the partials):
// one wavefront per sample, lane (q, r) adds the partials r, r + 4, .. of sum q in index order, the four strides are added
// as (0 + 1) + (2 + 3).  A sample without a populated bucket gets sixteen zeros.
__global__ __launch_bounds__(64) void pose_normal_eq_finish_kernel(const double *__restrict__ part, const int32_t *__restrict__ info,
                                                                   float *__restrict__ neq, int nblk) {
    const int b = blockIdx.x, lane = threadIdx.x, q = lane & 15, r = lane >> 4;
    double s = 0.0;
    for (int kk = r; kk < nblk; kk += 4) s += part[((size_t)b * nblk + kk) * NEQ_SUMS + q];
    const double s1 = __shfl(s, q + 16), s2 = __shfl(s, q + 32), s3 = __shfl(s, q + 48);
    if (lane < NEQ_SUMS) neq[b * NEQ_SUMS + q] = info[b * 4] > 0 ? (float)((s + s1) + (s2 + s3)) : 0.0f;
}

extern "C" size_t rrl_pose_normal_eq_part_bytes(int B, int L) {
    if (B <= 0 || L <= 0) return 0;
    return sizeof(double) * NEQ_SUMS * (size_t)B * NEQ_SUBS * (size_t)((L + 1023) / 1024);
}

extern "C" int rrl_pose_normal_eq(const void *ws, size_t ws_bytes, int B, int N, int M, int L, int s_m, int s_n, int e_m, int e_n,
                                  float *neq, void *part, size_t part_bytes, const rrl_opts *opts, void *stream) {
    if (!ws || !neq || !part || B <= 0 || B > 65535 || N <= 0 || M <= 0 || L <= 0 || L >= (1 << 24)) return RRL_E_ARG;
    if (s_m < 1 || s_n < 1 || e_m > RRL_MAX_HITS + 1 || e_n > RRL_MAX_HITS + 1 || e_m <= s_m || e_n <= s_n) return RRL_E_ARG;  // (the wide path is not served)
    if ((((uintptr_t)part) & 7) != 0) return RRL_E_ARG;
    if (opts && opts->struct_bytes >= (int32_t)(offsetof(rrl_opts, problems) + sizeof(int32_t)) && opts->problems > 0 &&
        opts->problems < B)
        return RRL_E_ARG;  // (multi-pose: B poses of fewer problems)
    const WsLayout w(B, N, M, L);
    if (ws_bytes < w.total || part_bytes < rrl_pose_normal_eq_part_bytes(B, L)) return RRL_E_WS;
    const int nblk = NEQ_SUBS * ((L + 1023) / 1024);
    const NeqArgs a = {w.at<RRL_WS_KJ>(ws), w.at<RRL_WS_W1>(ws), (const float4 *)w.at<RRL_WS_Q1>(ws), (const float4 *)w.at<RRL_WS_Q2>(ws),
                       w.at<RRL_WS_D>(ws), w.at<RRL_WS_MED>(ws), w.at<RRL_WS_BCNT>(ws), w.at<RRL_WS_INFO>(ws), (double *)part, L};
    hipLaunchKernelGGL(pose_normal_eq_kernel, dim3((unsigned)nblk, (unsigned)B), dim3(256), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(pose_normal_eq_finish_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, (const double *)part,
                       a.info, neq, nblk);
    RRL_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------
// The batched Gauss-Newton pose step: one wavefront per pose, grid B (se3_adam_step_kernel<Se3Batch>'s shape).  Lanes 8 .. 13
// reduce the next sampler box from the step's partial rows and lane 0 logs (rrl_pose_tail.h); lane 0 does the pose: H (6 x 6) and g from the
// sixteen sums, then rrl_pose_solve.h: H + damping diag(H) + eps I, Cholesky and both substitutions in double (newton_solve),
// step scale, clamps, the exact Rodrigues rotation, R <- R Rot^T, T <- T Rot^T + v, one Gram-Schmidt pass over R's rows
// (pose_compose<false>: no pivot); the log row, the stopping rule.
// state [B][4] int32: the pose-step state words and their rule, rrl_pose_tail.h (PoseStop); [3] = RRL_NEWTON_*.
// ---------------------------------------------------------------------------------------
struct NewtonArgs {
    const float *neq;
    const int32_t *gate;
    long long gate_stride;
    const float *damping, *step, *max_rot, *max_trans, *tol_rot, *tol_trans;
    int patience;
    double eps;
    float *R, *T;
    const float *loss, *value;
    float *table;
    long long *cursor, nrows;
    float *row;
    const float *aabb_rows;
    long long row_stride;
    const int32_t *count1;
    int N;
    float *box, *delta, *last_step;
    int32_t *state;
    int B;
};

__global__ __launch_bounds__(64) void se3_newton_step_kernel(const NewtonArgs a) {
    const int b = blockIdx.x, k = threadIdx.x;
    if (b >= a.B) return;
    const size_t s = (size_t)b;
    int32_t *__restrict__ st = a.state + s * 4;
    const int raw = a.gate ? a.gate[(long long)b * a.gate_stride] : 1;
    PoseStop stop = pose_stop_load(st);
    const bool open = raw > 0 && !stop.done;  // a done pair's gate is treated as closed: its pose is frozen
    // the shared tail on sample b's slices: column b of the table [nrows][B][3], [0, ceil(count1[b] / 256)) of its partial rows
    const PoseLog plog = pose_log_load(k, a.table ? a.table + s * 3 : nullptr, a.cursor ? a.cursor + s : nullptr,
                                       a.loss ? a.loss + s : nullptr, a.value ? a.value + s : nullptr);
    pose_next_box(k, a.box ? a.box + s * 6 : nullptr, a.aabb_rows + (long long)b * a.row_stride,
                  (rrl_rows(a.count1, b, a.N) + 255) / 256);
    if (k != 0) return;
    int status = stop.done ? RRL_NEWTON_DONE : (raw > 0 ? RRL_NEWTON_STEPPED : RRL_NEWTON_GATED);
    if (open) {
        double S[NEQ_SUMS];
#pragma unroll
        for (int q = 0; q < NEQ_SUMS; ++q) S[q] = (double)a.neq[s * NEQ_SUMS + q];
        // H = [ tr(S_QQ) I - S_QQ   [S_sQ]x ; -[S_sQ]x   S_ss I ],  g = (g_w, g_v)
        const double tr = S[0] + S[3] + S[5];
        double H[6][6];
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = 0; j < 6; ++j) H[i][j] = 0.0;
        H[0][0] = tr - S[0]; H[0][1] = -S[1];     H[0][2] = -S[2];
        H[1][0] = -S[1];     H[1][1] = tr - S[3]; H[1][2] = -S[4];
        H[2][0] = -S[2];     H[2][1] = -S[4];     H[2][2] = tr - S[5];
        H[0][4] = -S[8]; H[0][5] = S[7];
        H[1][3] = S[8];  H[1][5] = -S[6];
        H[2][3] = -S[7]; H[2][4] = S[6];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) H[3 + j][i] = H[i][3 + j];
        H[3][3] = H[4][4] = H[5][5] = S[9];
        const double g[6] = {S[10], S[11], S[12], S[13], S[14], S[15]};
        double x[6];
        const bool solved = newton_solve(H, g, (double)a.damping[s], a.eps, x);
        if (!solved) {
            status = RRL_NEWTON_FAILED;
        } else {
            if (a.delta)
#pragma unroll
                for (int i = 0; i < 6; ++i) a.delta[s * 6 + i] = (float)x[i];
            double nw, nv;
            if (!pose_compose<false>(x, (double)a.step[s], (double)a.max_rot[s], (double)a.max_trans[s], nullptr, a.R + s * 9,
                                     a.T + s * 3, nw, nv))
                status = RRL_NEWTON_FAILED;
            else
                pose_stop_update(stop, s, (float)nw, (float)nv, a.last_step, a.tol_rot, a.tol_trans, a.patience);
        }
    }
    pose_stop_store(stop, status, st);
    pose_log_store(plog, raw > 0, a.table ? a.table + s * 3 : nullptr, 3ll * a.B, a.nrows, a.cursor ? a.cursor + s : nullptr,
                   a.row ? a.row + s * 3 : nullptr);
}

extern "C" int rrl_se3_newton_step_batch(const float *neq, const int32_t *gate, long long gate_stride, const float *damping,
                                         const float *step, const float *max_rot, const float *max_trans, const float *tol_rot,
                                         const float *tol_trans, int patience, double eps, float *R, float *T, const float *loss,
                                         const float *value, float *table, long long *cursor, long long nrows, float *row,
                                         const float *aabb_rows, long long row_stride, const int32_t *count1, int N, float *box,
                                         float *delta, float *last_step, int32_t *state, int B, void *stream) {
    if (B < 0 || !neq || !damping || !step || !max_rot || !max_trans || !R || !T || !state) return RRL_E_ARG;
    if (gate && gate_stride < 0) return RRL_E_ARG;
    if (!(eps >= 0.0) || !pose_stop_args_ok(patience, tol_rot, tol_trans)) return RRL_E_ARG;
    if (box && (!aabb_rows || N <= 0 || row_stride < 8ll * ((N + 255) / 256))) return RRL_E_ARG;
    if (B == 0) return 0;
    const NewtonArgs a = {neq, gate, gate_stride, damping, step, max_rot, max_trans, tol_rot, tol_trans, patience, eps, R, T, loss,
                          value, table, cursor, nrows, row, aabb_rows, row_stride, count1, N, box, delta, last_step, state, B};
    hipLaunchKernelGGL(se3_newton_step_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, a);
    RRL_LAUNCH_CHECK();
    return 0;
}
