// rrl_robust.hip -- robust point-to-point ICP on the device (include/rrl.h rrl_key_median, rrl_welsch_weights,
// rrl_robust_step_batch, rrl_robust_icp_epoch): the ICP epoch of rrl_kabsch.hip whose pairs carry the
// Welsch weights exp(-d^2 / 2 nu^2) of the keys' own distance words, with a per-pair scale nu that starts at a multiple of the
// first epoch's median residual and is annealed whenever the pose has settled at the current scale.
//
// Which rows count is rrl_pair_sums.h's pair_walk, the rule of the fit that consumes the weights; the state words and the calm
// count are rrl_pose_tail.h's PoseStop.  Nothing here sums floats: the median is a radix select over integer counts, the
// weights are one double exp per row, the step is one lane per pair.
#include <cstddef>
#include <cstdint>

#include "rrl_ws.h"
#include "rrl_pose_tail.h"
#include "rrl_pair_sums.h"
#include "rrl_cloud_epoch.h"
#include "rrl_icp_step.h"

// the distance word of row i of sample b when the fit would use the row (gate aside), else false
__device__ __forceinline__ bool valid_word(const unsigned long long *__restrict__ keys, int b, int n, int i, int ca, int m, int cb,
                                           unsigned &word) {
    const PairRow pair = pair_walk(keys, b, n, i, ca, m, cb, INFINITY);
    word = __float_as_uint(pair.dist);
    return !pair.skip;
}

struct KeyMedianArgs {
    const unsigned long long *keys;
    const int32_t *count_a, *count_b;
    int n, m;
    float *med_sq;
    int32_t *info;
    float *nu;
    double nu_scale;
    const float *nu_end;
};

// One 256-lane workgroup per pair: four passes, most significant byte first.  A pass counts, among the valid words that agree
// with the bytes decided so far, how many carry each value of its byte (LDS integer atomics: the counts do not depend on the
// order), scans the 256 counts, and the one lane whose bin holds the wanted rank fixes the byte and the rank inside the bin.
__global__ __launch_bounds__(256) void key_median_kernel(const KeyMedianArgs a) {
    __shared__ unsigned s_hist[256], s_scan[256], s_sel[2];
    const int tid = threadIdx.x, b = blockIdx.x, n = a.n, m = a.m;
    const int ca = rrl_rows(a.count_a, b, n), cb = rrl_rows(a.count_b, b, m);
    unsigned prefix = 0u, mask = 0u, rank = 0u, k = 0u;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        s_hist[tid] = 0u;
        __syncthreads();
        for (int i = tid; i < n; i += 256) {
            unsigned word;
            if (valid_word(a.keys, b, n, i, ca, m, cb, word) && (word & mask) == prefix) atomicAdd(&s_hist[(word >> shift) & 255u], 1u);
        }
        __syncthreads();
        const unsigned mine = s_hist[tid];
        s_scan[tid] = mine;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            const unsigned v = tid >= off ? s_scan[tid - off] : 0u;
            __syncthreads();
            s_scan[tid] += v;
            __syncthreads();
        }
        if (pass == 0) {
            k = s_scan[255];  // (uniform)
            if (k == 0u) break;
            rank = (k - 1u) / 2u;
        }
        const unsigned incl = s_scan[tid], excl = incl - mine;
        if (excl <= rank && rank < incl) {  // one lane: the bins partition [0, count)
            s_sel[0] = (unsigned)tid;
            s_sel[1] = rank - excl;
        }
        __syncthreads();
        prefix |= s_sel[0] << shift;
        mask |= 255u << shift;
        rank = s_sel[1];
        __syncthreads();
    }
    if (tid != 0) return;
    const float med = k ? __uint_as_float(prefix) : 0.0f;
    a.med_sq[b] = med;
    a.info[(size_t)b * 2] = (int32_t)k;
    a.info[(size_t)b * 2 + 1] = k == 0u ? 1 : 0;
    if (a.nu) {
        const float start = (float)(a.nu_scale * sqrt((double)med)), end = a.nu_end[b];
        a.nu[b] = start > end ? start : end;
    }
}

static bool keyed_rows_ok(const void *keys, const int32_t *count_a, const int32_t *count_b, int B, int n, int m) {
    return B >= 0 && B <= 32767 && n > 0 && m > 0 && keys && (count_a == nullptr) == (count_b == nullptr);
}

extern "C" int rrl_key_median(const uint64_t *keys, const int32_t *count_a, const int32_t *count_b, int B, int n, int m, float *med_sq,
                              int32_t *info, float *nu, double nu_scale, const float *nu_end, void *stream) {
    if (!keyed_rows_ok(keys, count_a, count_b, B, n, m) || n > rrl_sort_capacity() || !med_sq || !info) return RRL_E_ARG;
    if (nu && (!nu_end || !(nu_scale > 0.0))) return RRL_E_ARG;
    if (B == 0) return 0;
    const KeyMedianArgs a = {(const unsigned long long *)keys, count_a, count_b, n, m, med_sq, info, nu, nu_scale, nu_end};
    hipLaunchKernelGGL(key_median_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, a);
    RRL_LAUNCH_CHECK();
    return 0;
}

// Grid (ceil(n / 256), B): one row per lane.
__global__ __launch_bounds__(256) void welsch_weights_kernel(const unsigned long long *__restrict__ keys, const int32_t *__restrict__ count_a,
                                                             const int32_t *__restrict__ count_b, const float *__restrict__ nu,
                                                             float *__restrict__ w, int n, int m) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float s = nu[b];
    float out = 0.0f;
    unsigned word;
    if (s > 0.0f && s < INFINITY && valid_word(keys, b, n, i, rrl_rows(count_a, b, n), m, rrl_rows(count_b, b, m), word)) {
        const double d2 = (double)__uint_as_float(word), s2 = (double)s * (double)s;
        const double e = exp(-d2 / (2.0 * s2));
        out = e == e ? (float)e : 0.0f;  // (a distance word that is no number weighs nothing)
    }
    w[(size_t)b * n + i] = out;
}

extern "C" int rrl_welsch_weights(const uint64_t *keys, const int32_t *count_a, const int32_t *count_b, const float *nu, float *w, int B,
                                  int n, int m, void *stream) {
    if (!keyed_rows_ok(keys, count_a, count_b, B, n, m) || !nu || !w) return RRL_E_ARG;
    if (B == 0) return 0;
    hipLaunchKernelGGL(welsch_weights_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned long long *)keys, count_a, count_b, nu, w, n, m);
    RRL_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------
// The robust pose step: rrl_icp_step.h's body with the annealing rule where icp_step_kernel (rrl_kabsch.hip) declares a pair
// done, in its own launch.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void robust_step_kernel(const IcpStepArgs a, const IcpAnneal n) { icp_step_one<true>(a, n); }

// RRL_E_ARG of the annealing rule (host)
static bool anneal_args_ok(const float *nu, const float *nu_end, const int32_t *level, float anneal, int level_cap, int patience) {
    if (!nu || !nu_end || !level || !(anneal > 0.0f && anneal < 1.0f) || level_cap < 0) return false;
    return patience > 0 || level_cap > 0;  // (else nothing would ever anneal)
}

extern "C" int rrl_robust_step_batch(const float *Rk, const float *Tk, const int32_t *info, const double *fit, float *R, float *T,
                                     const float *tol_rot, const float *tol_trans, int patience, const float *value, float *table,
                                     long long *cursor, long long nrows, float *row, float *last_step, int32_t *state, float *nu,
                                     const float *nu_end, float anneal, int level_cap, int32_t *level, int B, void *stream) {
    if (B < 0 || !icp_step_args_ok(Rk, Tk, info, fit, R, T, state, patience, tol_rot, tol_trans)) return RRL_E_ARG;
    if (!anneal_args_ok(nu, nu_end, level, anneal, level_cap, patience)) return RRL_E_ARG;
    if (B == 0) return 0;
    const IcpStepArgs a = {Rk, Tk, info, fit, R, T, tol_rot, tol_trans, patience, value, table, cursor, nrows, row, last_step, state, B};
    const IcpAnneal n = {nu, nu_end, anneal, level_cap, level};
    hipLaunchKernelGGL(robust_step_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, a, n);
    RRL_LAUNCH_CHECK();
    return 0;
}

// One robust ICP epoch: the public entries back to back, every refusal before the first launch (host code only).  The struct is
// rrl_icp_epoch's; its w stays NULL, the weights are an output here.
extern "C" int rrl_robust_icp_epoch(const rrl_icp_epoch_args *a, int init, float *w, float *nu, const float *nu_end, float *med_sq,
                                    int32_t *med_info, double nu_scale, float anneal, int level_cap, int32_t *level, void *stream) {
    if (!cloud_epoch_front_ok(a)) return RRL_E_ARG;
    if (!icp_step_args_ok(a->Rk, a->Tk, a->info, a->fit, a->R, a->T, a->state, a->patience, a->tol_rot, a->tol_trans)) return RRL_E_ARG;
    if ((((uintptr_t)a->fit) & 7) != 0 || a->w || !w || !med_sq || !med_info || !(nu_scale > 0.0)) return RRL_E_ARG;
    if (!anneal_args_ok(nu, nu_end, level, anneal, level_cap, a->patience)) return RRL_E_ARG;
    if (!icp_epoch_ws_ok(a)) return RRL_E_WS;
    const int B = a->B, N = a->N, M = a->M;
    int rc = cloud_epoch_pair(a, stream);
    if (rc) return rc;
    if (init) {
        rc = rrl_key_median(a->best_x, a->count1, a->count2, B, N, M, med_sq, med_info, nu, nu_scale, nu_end, stream);
        if (rc) return rc;
    }
    rc = rrl_welsch_weights(a->best_x, a->count1, a->count2, nu, w, B, N, M, stream);
    if (rc) return rc;
    rc = icp_epoch_fit(a, w, stream);
    if (rc) return rc;
    return rrl_robust_step_batch(a->Rk, a->Tk, a->info, a->fit, a->R, a->T, a->tol_rot, a->tol_trans, a->patience, a->values, a->table,
                                 a->cursor, a->table_rows, a->row, a->last_step, a->state, nu, nu_end, anneal, level_cap, level, B, stream);
}
