// rrl_plane.hip -- point-to-plane ICP on the device (include/rrl.h rrl_idx_normals, rrl_plane_normal_eq, rrl_plane_step_batch,
// rrl_plane_icp_epoch): unit normals from the index lists of rrl_ball_group (the smallest eigenvector of a
// neighbourhood's scatter matrix), the 32 sums of one linearised point-to-plane fit over the keys a Chamfer walk left, the damped
// 6 x 6 pose step about a pivot, and the four entries of an epoch as one C call.
//
// The arithmetic rule is rrl_kabsch.hip's: every sum is a fixed-order double sum of double terms formed from float32 inputs
// (rrl_pair_sums.h: the pair walk, per-lane accumulators, wave_sum_d, four wavefronts, one partial row per workgroup, the
// partial rows in index order, no atomics); everything after the sums is double on one lane, rounded to float32 once.  The
// solver and the pose composition are se3_newton_step_kernel's (rrl_pose_solve.h), the composition in its form about a pivot;
// the epoch's host front is rrl_icp_epoch's (rrl_cloud_epoch.h).
#include <cstddef>
#include <cstdint>

#include "rrl_ws.h"
#include "rrl_pose_tail.h"
#include "rrl_pose_solve.h"
#include "rrl_pair_sums.h"
#include "rrl_cloud_epoch.h"

// ---------------------------------------------------------------------------------------
// 1. Normals.  Grid (ceil(S / 4), B): one wavefront per row, lane = slot of the row's index list, the four waves of a
// workgroup share nothing.  The nine moments about the pivot (the first member kept) are wave sums of doubles; the 3 x 3
// eigenproblem is solved by every lane alike (the same bits in, the same bits out), lane 0 stores.
// ---------------------------------------------------------------------------------------
#define PLN_WAVES 4

// one two-sided Jacobi rotation of the symmetric A in the (P, Q) plane, accumulated into V (columns = eigenvectors);
// false: the entry is zero, negligible against `floor` or not a number
template <int P, int Q>
__device__ __forceinline__ bool sym_jacobi_pair(double (&A)[3][3], double (&V)[3][3], double floor) {
    const double apq = A[P][Q];
    if (apq == 0.0 || !(fabs(apq) > floor)) return false;
    const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
    const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(1.0 + theta * theta));
    const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
    constexpr int R = 3 - P - Q;
    const double app = A[P][P], aqq = A[Q][Q], arp = A[R][P], arq = A[R][Q];
    A[P][P] = app - t * apq;
    A[Q][Q] = aqq + t * apq;
    A[P][Q] = A[Q][P] = 0.0;
    A[R][P] = A[P][R] = c * arp - s * arq;
    A[R][Q] = A[Q][R] = s * arp + c * arq;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double vp = V[i][P], vq = V[i][Q];
        V[i][P] = c * vp - s * vq;
        V[i][Q] = s * vp + c * vq;
    }
    return true;
}

__global__ __launch_bounds__(64 * PLN_WAVES) void idx_normals_kernel(const float *__restrict__ pts, int stride,
                                                                     const int32_t *__restrict__ idx, const int32_t *__restrict__ found,
                                                                     const int32_t *__restrict__ counts, int nsample, double rank_tol,
                                                                     float *__restrict__ normals, float *__restrict__ quality, int ncap,
                                                                     int S) {
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int b = blockIdx.y;
    const int q = (int)blockIdx.x * PLN_WAVES + w;  // wave-uniform
    if (q >= S) return;
    const int n = rrl_rows(counts, b, ncap);
    const size_t row = (size_t)b * S + q;
    const float *__restrict__ p = pts + (size_t)b * ncap * stride;
    const int f = min(max(found[row], 0), nsample);  // nsample <= 64: one slot per lane
    int j = -1;
    if (lane < f) j = idx[row * nsample + lane];
    const bool keep = j >= 0 && j < n;  // a slot whose index is outside the sample's rows is dropped
    const unsigned long long bal = __ballot(keep);
    const int k = __popcll(bal);
    float nx = 0.0f, ny = 0.0f, nz = 0.0f, qual = 0.0f;
    if (k >= 3) {
        const int first = __builtin_amdgcn_readfirstlane((int)__ffsll((long long)bal) - 1);
        const int jp = __shfl(j, first);  // inside [0, n): its lane kept it
        const double px = (double)p[(size_t)jp * stride], py = (double)p[(size_t)jp * stride + 1], pz = (double)p[(size_t)jp * stride + 2];
        double dx = 0.0, dy = 0.0, dz = 0.0;
        if (keep) {
            const float *__restrict__ r = p + (size_t)j * stride;
            dx = (double)r[0] - px; dy = (double)r[1] - py; dz = (double)r[2] - pz;
        }
        const double sx = wave_sum_d(dx), sy = wave_sum_d(dy), sz = wave_sum_d(dz);
        const double sxx = wave_sum_d(dx * dx), sxy = wave_sum_d(dx * dy), sxz = wave_sum_d(dx * dz);
        const double syy = wave_sum_d(dy * dy), syz = wave_sum_d(dy * dz), szz = wave_sum_d(dz * dz);
        const double kd = (double)k, mx = sx / kd, my = sy / kd, mz = sz / kd;
        double A[3][3], V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
        A[0][0] = sxx - kd * mx * mx; A[0][1] = A[1][0] = sxy - kd * mx * my; A[0][2] = A[2][0] = sxz - kd * mx * mz;
        A[1][1] = syy - kd * my * my; A[1][2] = A[2][1] = syz - kd * my * mz; A[2][2] = szz - kd * mz * mz;
        const double scale = (fabs(A[0][0]) + fabs(A[1][1])) + fabs(A[2][2]);
        const bool finite = scale < (double)INFINITY && fabs(A[0][1]) < (double)INFINITY && fabs(A[0][2]) < (double)INFINITY &&
                            fabs(A[1][2]) < (double)INFINITY;
        if (finite) {
            const double floor = 1e-22 * scale;
            for (int sweep = 0; sweep < 16; ++sweep) {
                const bool r01 = sym_jacobi_pair<0, 1>(A, V, floor), r02 = sym_jacobi_pair<0, 2>(A, V, floor),
                           r12 = sym_jacobi_pair<1, 2>(A, V, floor);
                if (!(r01 || r02 || r12)) break;
            }
            // ascending: c0 = the column of the smallest eigenvalue (the lowest index among equals)
            // (selects, not indexed arrays: nothing here may land in scratch memory)
            const double la = A[0][0], lb = A[1][1], lc = A[2][2];
            int c0 = 0;
            double l0 = la;
            if (lb < l0) { c0 = 1; l0 = lb; }
            if (lc < l0) { c0 = 2; l0 = lc; }
            const double ra = c0 == 0 ? lb : la, rb = c0 == 2 ? lb : lc;  // the other two
            const double l1 = fmin(ra, rb), l2 = fmax(ra, rb);
            if (l1 > rank_tol * l2) {  // (collinear or coincident members, or a NaN: no plane)
                const double e0 = c0 == 0 ? V[0][0] : (c0 == 1 ? V[0][1] : V[0][2]);
                const double e1 = c0 == 0 ? V[1][0] : (c0 == 1 ? V[1][1] : V[1][2]);
                const double e2 = c0 == 0 ? V[2][0] : (c0 == 1 ? V[2][1] : V[2][2]);
                double big = e0;  // the component of largest magnitude, the lowest index among equals
                if (fabs(e1) > fabs(big)) big = e1;
                if (fabs(e2) > fabs(big)) big = e2;
                const double sg = big < 0.0 ? -1.0 : 1.0;
                nx = (float)(sg * e0); ny = (float)(sg * e1); nz = (float)(sg * e2);
                qual = (float)((l1 - l0) / l2);
            }
        }
    }
    if (lane == 0) {
        normals[row * 3] = nx; normals[row * 3 + 1] = ny; normals[row * 3 + 2] = nz;
        if (quality) quality[row] = qual;
    }
}

extern "C" int rrl_idx_normals(const float *pts, int stride, const int32_t *idx, const int32_t *found, const int32_t *counts,
                               int nsample, float rank_tol, float *normals, float *quality, int B, int n, int S, void *stream) {
    if (!pts || !idx || !found || !normals) return RRL_E_ARG;
    if (B < 1 || B > 32767 || n < 1 || n > rrl_sort_capacity() || S < 0 || stride < 3) return RRL_E_ARG;
    if (nsample < 1 || nsample > RRL_GROUP_MAX_SAMPLE) return RRL_E_ARG;
    if (!(rank_tol >= 0.0f) || !(rank_tol < 1.0f)) return RRL_E_ARG;  // negative, NaN, or a bound no row can meet
    if (S == 0) return 0;
    const unsigned gx = (unsigned)((S + PLN_WAVES - 1) / PLN_WAVES);
    hipLaunchKernelGGL(idx_normals_kernel, dim3(gx, (unsigned)B), dim3(64 * PLN_WAVES), 0, (hipStream_t)stream, pts, stride, idx, found,
                       counts, nsample, (double)rank_tol, normals, quality, n, S);
    RRL_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------
// 2. The sums of one linearised point-to-plane fit: kabsch_part_kernel's shape with 32 sums per row.
// ---------------------------------------------------------------------------------------
#define PL_ROWS 512  // rows of `moved` per 256-lane workgroup (two rounds)
#define PL_SUMS RRL_PLANE_DOUBLES

struct PlaneArgs {
    int B, N, M, st;
    const float *moved;
    const unsigned long long *keys;
    const float *tar, *normals;
    const int32_t *count1, *count2;
    const float *w, *gate_sq, *pivot;
    double *part, *neq;
    int32_t *info;
};

// lanes q = 0 .. 31 of one wavefront: sample b's neq row from its 32 sums, lane 0 its info
__device__ __forceinline__ void plane_finish(const PlaneArgs &a, int b, const double *s_tot, int q) {
    const double W = s_tot[RRL_PLANE_W];
    const int used = (int)s_tot[RRL_PLANE_USED], skipped = (int)s_tot[RRL_PLANE_SKIPPED];
    const bool few = used < 6 || !(W > 0.0);
    double v = s_tot[q];
    if (q < RRL_PLANE_W || q == RRL_PLANE_RES || q == RRL_PLANE_KEYMEAN) v = few ? 0.0 : v / W;
    a.neq[(size_t)b * PL_SUMS + q] = v;
    if (q == 0) {
        int32_t *__restrict__ info = a.info + (size_t)b * 4;
        info[0] = used;
        info[1] = few ? RRL_FIT_FEW : RRL_FIT_OK;
        info[2] = 0;
        info[3] = skipped;
    }
}

// Grid (ceil(N / PL_ROWS), B).  Lane tid takes rows bx PL_ROWS + tid and + 256 of sample b, in that order; the workgroup's row
// of sums goes to part[b][bx] -- and, when the grid has one workgroup per sample, its first 32 lanes finish in the same launch.
__global__ __launch_bounds__(256) void plane_part_kernel(const PlaneArgs a) {
    __shared__ double s_red[4][PL_SUMS];
    __shared__ double s_tot[PL_SUMS];
    const int tid = threadIdx.x, bx = blockIdx.x, b = blockIdx.y, N = a.N, M = a.M;
    const int c1 = rrl_rows(a.count1, b, N), c2 = rrl_rows(a.count2, b, M);
    const float *__restrict__ Y = a.moved + (size_t)b * N * 3;
    const float *__restrict__ Tp = a.tar + (size_t)b * M * a.st;
    const float *__restrict__ Np = a.normals + (size_t)b * M * 3;
    double c[3] = {0.0, 0.0, 0.0};
    if (a.pivot)
#pragma unroll
        for (int j = 0; j < 3; ++j) c[j] = (double)a.pivot[(size_t)b * 3 + j];
    const float gate = (a.keys && a.gate_sq) ? a.gate_sq[b] : INFINITY;
    double acc[PL_SUMS];
#pragma unroll
    for (int q = 0; q < PL_SUMS; ++q) acc[q] = 0.0;
#pragma unroll
    for (int r = 0; r < PL_ROWS / 256; ++r) {
        const int i = bx * PL_ROWS + r * 256 + tid;
        if (i >= N) continue;
        const PairRow pair = pair_walk(a.keys, b, N, i, c1, M, c2, gate);
        if (pair.skip) {
            acc[RRL_PLANE_SKIPPED] += 1.0;
            continue;
        }
        if (pair.gated) continue;
        const float *__restrict__ nr = Np + (size_t)pair.idx * 3;  // idx < min(M, c2): inside sample b's rows
        const float n0 = nr[0], n1 = nr[1], n2 = nr[2];
        if (!(fabsf(n0) < INFINITY && fabsf(n1) < INFINITY && fabsf(n2) < INFINITY) || (n0 == 0.0f && n1 == 0.0f && n2 == 0.0f))
            continue;  // a partner without a normal: weight 0, neither used nor skipped
        const double w = a.w ? (double)a.w[(size_t)b * N + i] : 1.0;
        const float *__restrict__ yr = Y + (size_t)i * 3;
        const float *__restrict__ br = Tp + (size_t)pair.idx * a.st;
        const double y[3] = {(double)yr[0], (double)yr[1], (double)yr[2]};
        const double nn[3] = {(double)n0, (double)n1, (double)n2};
        const double p[3] = {y[0] - c[0], y[1] - c[1], y[2] - c[2]};
        const double e[3] = {y[0] - (double)br[0], y[1] - (double)br[1], y[2] - (double)br[2]};
        const double res = (e[0] * nn[0] + e[1] * nn[1]) + e[2] * nn[2];
        const double J[6] = {p[1] * nn[2] - p[2] * nn[1], p[2] * nn[0] - p[0] * nn[2], p[0] * nn[1] - p[1] * nn[0], nn[0], nn[1], nn[2]};
        int at = 0;
#pragma unroll
        for (int u = 0; u < 6; ++u) {
            const double wj = w * J[u];
#pragma unroll
            for (int v = u; v < 6; ++v) acc[RRL_PLANE_H + at++] += wj * J[v];
            acc[RRL_PLANE_G + u] += wj * res;
        }
        acc[RRL_PLANE_W] += w;
        acc[RRL_PLANE_RES] += w * (res * res);
        acc[RRL_PLANE_KEYMEAN] += w * (double)pair.dist;
        acc[RRL_PLANE_USED] += 1.0;
    }
    const double tot = block_sum_d(acc, s_red, a.part + ((size_t)b * gridDim.x + bx) * PL_SUMS);
    if (gridDim.x != 1) return;  // (uniform)
    if (tid < PL_SUMS) s_tot[tid] = tot;
    __syncthreads();
    if (tid < PL_SUMS) plane_finish(a, b, s_tot, tid);
}

// One wavefront per sample: lane q adds sum q of the sample's partial rows in index order, then the finish.
__global__ __launch_bounds__(64) void plane_finish_kernel(const PlaneArgs a, int nblk) {
    __shared__ double s_tot[PL_SUMS];
    const int b = blockIdx.x, lane = threadIdx.x;
    if (lane < PL_SUMS) s_tot[lane] = part_rows_total<PL_SUMS>(a.part, b, nblk, lane);
    __syncthreads();
    if (lane < PL_SUMS) plane_finish(a, b, s_tot, lane);
}

extern "C" size_t rrl_plane_part_bytes(int B, int N) {
    if (B <= 0 || N <= 0) return 0;
    return sizeof(double) * PL_SUMS * (size_t)B * (size_t)((N + PL_ROWS - 1) / PL_ROWS);
}

extern "C" int rrl_plane_normal_eq(const rrl_plane_args *p, void *stream) {
    if (!p || p->struct_bytes != (int32_t)sizeof(rrl_plane_args)) return RRL_E_ARG;
    if (p->B < 0 || p->B > 32767 || p->N <= 0 || p->M <= 0 || p->tar_stride < 3) return RRL_E_ARG;
    if (!p->moved || !p->tar || !p->normals || !p->neq || !p->info || !p->part) return RRL_E_ARG;
    if ((((uintptr_t)p->neq) & 7) != 0 || (((uintptr_t)p->part) & 7) != 0) return RRL_E_ARG;
    if ((!p->keys && p->M != p->N) || (p->gate_sq && !p->keys)) return RRL_E_ARG;
    if (p->part_bytes < rrl_plane_part_bytes(p->B, p->N)) return RRL_E_WS;
    if (p->B == 0) return 0;
    const PlaneArgs a = {p->B, p->N, p->M, p->tar_stride, p->moved, (const unsigned long long *)p->keys, p->tar, p->normals, p->count1,
                         p->count2, p->w, p->gate_sq, p->pivot, (double *)p->part, p->neq, p->info};
    const int nblk = (p->N + PL_ROWS - 1) / PL_ROWS;
    hipLaunchKernelGGL(plane_part_kernel, dim3((unsigned)nblk, (unsigned)p->B), dim3(256), 0, (hipStream_t)stream, a);
    if (nblk > 1) hipLaunchKernelGGL(plane_finish_kernel, dim3((unsigned)p->B), dim3(64), 0, (hipStream_t)stream, a, nblk);
    RRL_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------
// 3. The pose step: one wavefront per pair, lane 0 works (icp_step_kernel's lane roles; the state words, the stopping rule
// and the log row are rrl_pose_tail.h's).
// ---------------------------------------------------------------------------------------
struct PlaneStepArgs {
    const double *neq;
    const int32_t *info;
    const float *pivot, *damping, *step, *max_rot, *max_trans, *tol_rot, *tol_trans;
    int patience;
    double eps;
    float *R, *T;
    const float *value;
    float *table;
    long long *cursor, nrows;
    float *row, *last_step;
    int32_t *state;
    int B;
};

__global__ __launch_bounds__(64) void plane_step_kernel(const PlaneStepArgs a) {
    const int b = blockIdx.x;
    if (b >= a.B || threadIdx.x != 0) return;
    const size_t s = (size_t)b;
    int32_t *__restrict__ st = a.state + s * 4;
    const double *__restrict__ S = a.neq + s * PL_SUMS;
    const int fstat = a.info[s * 4 + 1];
    PoseLog plog = {-1, (float)S[RRL_PLANE_RES], a.value ? a.value[s] : 0.0f};
    if (a.table && a.cursor) plog.at = a.cursor[s];
    PoseStop stop = pose_stop_load(st);
    int status = stop.done ? RRL_PLANE_DONE : (fstat == RRL_FIT_OK ? RRL_PLANE_STEPPED : RRL_PLANE_FEW);
    if (!stop.done && fstat == RRL_FIT_OK) {
        double H[6][6], g[6], x[6];
        int at = 0;
#pragma unroll
        for (int u = 0; u < 6; ++u) {
            g[u] = S[RRL_PLANE_G + u];
#pragma unroll
            for (int v = u; v < 6; ++v) {
                const double h = S[RRL_PLANE_H + at++];
                H[u][v] = h;
                H[v][u] = h;
            }
        }
        if (!newton_solve(H, g, (double)a.damping[s], a.eps, x)) {
            status = RRL_PLANE_FAILED;
        } else {
            double nw, nv;
            if (!pose_compose<true>(x, (double)a.step[s], (double)a.max_rot[s], (double)a.max_trans[s],
                                    a.pivot ? a.pivot + s * 3 : nullptr, a.R + s * 9, a.T + s * 3, nw, nv))
                status = RRL_PLANE_FAILED;
            else
                pose_stop_update(stop, s, (float)nw, (float)nv, a.last_step, a.tol_rot, a.tol_trans, a.patience);
        }
    }
    pose_stop_store(stop, status, st);
    pose_log_store(plog, fstat == RRL_FIT_OK, a.table ? a.table + s * 3 : nullptr, 3ll * a.B, a.nrows, a.cursor ? a.cursor + s : nullptr,
                   a.row ? a.row + s * 3 : nullptr);
}

// the step's refusals (host), shared with the epoch
static bool plane_step_args_ok(const double *neq, const int32_t *info, const float *damping, const float *step, const float *max_rot,
                               const float *max_trans, const float *tol_rot, const float *tol_trans, int patience, double eps,
                               const float *R, const float *T, const int32_t *state) {
    if (!neq || !info || !damping || !step || !max_rot || !max_trans || !R || !T || !state) return false;
    if ((((uintptr_t)neq) & 7) != 0) return false;
    return eps >= 0.0 && pose_stop_args_ok(patience, tol_rot, tol_trans);
}

extern "C" int rrl_plane_step_batch(const double *neq, const int32_t *info, const float *pivot, const float *damping, const float *step,
                                    const float *max_rot, const float *max_trans, const float *tol_rot, const float *tol_trans,
                                    int patience, double eps, float *R, float *T, const float *value, float *table, long long *cursor,
                                    long long nrows, float *row, float *last_step, int32_t *state, int B, void *stream) {
    if (B < 0 || !plane_step_args_ok(neq, info, damping, step, max_rot, max_trans, tol_rot, tol_trans, patience, eps, R, T, state))
        return RRL_E_ARG;
    if (B == 0) return 0;
    const PlaneStepArgs a = {neq, info, pivot, damping, step, max_rot, max_trans, tol_rot, tol_trans, patience, eps,
                             R, T, value, table, cursor, nrows, row, last_step, state, B};
    hipLaunchKernelGGL(plane_step_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, a);
    RRL_LAUNCH_CHECK();
    return 0;
}

// One point-to-plane epoch: four public entries back to back, every refusal before the first launch (host code only).
extern "C" int rrl_plane_icp_epoch(const rrl_plane_epoch_args *a, void *stream) {
    if (!cloud_epoch_front_ok(a) || !a->normals) return RRL_E_ARG;
    const int B = a->B, N = a->N, M = a->M;
    if (!plane_step_args_ok(a->neq, a->info, a->damping, a->step, a->max_rot, a->max_trans, a->tol_rot, a->tol_trans, a->patience, a->eps,
                            a->R, a->T, a->state))
        return RRL_E_ARG;
    if (!cloud_epoch_cham_ws_ok(a) || a->part_bytes < rrl_plane_part_bytes(B, N)) return RRL_E_WS;
    int rc = cloud_epoch_pair(a, stream);
    if (rc) return rc;
    rrl_plane_args k = {};
    k.struct_bytes = (int32_t)sizeof(k);
    k.B = B; k.N = N; k.M = M; k.tar_stride = 3;
    k.moved = a->moved; k.keys = a->best_x; k.tar = a->tar; k.normals = a->normals; k.count1 = a->count1; k.count2 = a->count2;
    k.w = a->w; k.gate_sq = a->gate_sq; k.pivot = a->pivot;
    k.part = a->part; k.part_bytes = a->part_bytes; k.neq = a->neq; k.info = a->info;
    rc = rrl_plane_normal_eq(&k, stream);
    if (rc) return rc;
    return rrl_plane_step_batch(a->neq, a->info, a->pivot, a->damping, a->step, a->max_rot, a->max_trans, a->tol_rot, a->tol_trans,
                                a->patience, a->eps, a->R, a->T, a->values, a->table, a->cursor, a->table_rows, a->row, a->last_step,
                                a->state, B, stream);
}
