// rrl_neigh.hip -- pseudo-triangle builder: farthest-point sampling and
// k = 3 nearest neighbours on the GPU, replacing the reference's sequential torch loop
// (code/utils.py:275-296, farthest_point_sample) and sklearn KDTree query (code/loss.py:473-485).
// Preprocessing outside the timed loss path; correctness first, but no host round trips:
// the S sequential FPS iterations run inside ONE workgroup with one barrier per iteration.
#include "rrl_common.h"
#include "rrl_knn3_loop.h"

// (value, index) key: larger distance wins, then the SMALLER index (torch.max's first occurrence)
__device__ __forceinline__ unsigned long long fps_key(float d, int i) {
    return ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)(0xffffffffu - (unsigned)i);
}

__device__ __forceinline__ unsigned long long dpp_u64(unsigned long long v, int ctrl_sel) {
    unsigned lo = (unsigned)v, hi = (unsigned)(v >> 32);
    unsigned plo, phi;
    switch (ctrl_sel) {  // compile-time after unrolling
        case 0: plo = __builtin_amdgcn_update_dpp(lo, lo, 0xB1, 0xf, 0xf, false); phi = __builtin_amdgcn_update_dpp(hi, hi, 0xB1, 0xf, 0xf, false); break;
        case 1: plo = __builtin_amdgcn_update_dpp(lo, lo, 0x4E, 0xf, 0xf, false); phi = __builtin_amdgcn_update_dpp(hi, hi, 0x4E, 0xf, 0xf, false); break;
        case 2: plo = __builtin_amdgcn_update_dpp(lo, lo, 0x141, 0xf, 0xf, false); phi = __builtin_amdgcn_update_dpp(hi, hi, 0x141, 0xf, 0xf, false); break;
        default: plo = __builtin_amdgcn_update_dpp(lo, lo, 0x140, 0xf, 0xf, false); phi = __builtin_amdgcn_update_dpp(hi, hi, 0x140, 0xf, 0xf, false); break;
    }
    return ((unsigned long long)phi << 32) | plo;
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {  // butterfly inside rows of 16 (DPP), then the 4 rows via SGPRs
        unsigned long long p = dpp_u64(v, s);
        v = p > v ? p : v;
    }
    unsigned long long best = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        unsigned lo = __builtin_amdgcn_readlane((unsigned)v, 16 * r);
        unsigned hi = __builtin_amdgcn_readlane((unsigned)(v >> 32), 16 * r);
        unsigned long long x = ((unsigned long long)hi << 32) | lo;
        best = x > best ? x : best;
    }
    return best;
}

// Farthest-point sampling, code/utils.py:275-296: distance = 1e10; repeat S times: emit the
// current point, dist = ((dx^2 + dy^2) + dz^2) to it (fp32, no FMA), distance = min(distance,
// dist), next = argmax(distance) (first occurrence).  One 1024-lane workgroup per cloud; points
// and running distances live in LDS (16 B per point) when they fit, else in global scratch.
// COUNTED (fps_counted_kernel, a ragged batch): the first n_b = clamp(counts[b], 0, ncap) points of sample b (counts == NULL:
// ncap) -- the same arithmetic in the same order, so the S_b = min(S, n_b) indices are those of rrl_fps on pts[b, :n_b]; the
// entries beyond S_b are 0 and the rows beyond n_b are never read.  start[b] is clamped into [0, n_b) (memory safety only).
// out_cnt (optional): S_b.  The other instantiation contains none of this.
template <bool IN_LDS, bool COUNTED>
__device__ __forceinline__ void fps_body(const float *__restrict__ pts, const int32_t *__restrict__ counts,
                                         const int32_t *__restrict__ start, int32_t *__restrict__ out,
                                         int32_t *__restrict__ out_cnt, float *__restrict__ dist_g, int ncap, int S) {
    extern __shared__ __attribute__((aligned(16))) float4 cache[];  // IN_LDS: (x, y, z, distance)
    __shared__ unsigned long long wbest[2][16];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = COUNTED ? rrl_rows(counts, b, ncap) : ncap;  // uniform
    const int Sb = COUNTED ? min(S, n) : S;
    const float *p = pts + (size_t)b * ncap * 3;
    float *dg = dist_g + (size_t)b * ncap;
    if constexpr (COUNTED) {
        for (int i = Sb + tid; i < S; i += 1024) out[(size_t)b * S + i] = 0;
        if (tid == 0 && out_cnt != nullptr) out_cnt[b] = Sb;
        if (Sb == 0) return;  // uniform
    }
    for (int i = tid; i < n; i += 1024) {
        if (IN_LDS) cache[i] = make_float4(p[3 * i], p[3 * i + 1], p[3 * i + 2], 1e10f);
        else dg[i] = 1e10f;
    }
    int far = COUNTED ? min(max(start[b], 0), n - 1) : start[b];
    __syncthreads();
    for (int it = 0; it < Sb; ++it) {
        if (tid == 0) out[(size_t)b * S + it] = far;
        float cx, cy, cz;
        if (IN_LDS) { const float4 c = cache[far]; cx = c.x; cy = c.y; cz = c.z; }
        else { cx = p[3 * far]; cy = p[3 * far + 1]; cz = p[3 * far + 2]; }
        unsigned long long best = 0;
        for (int i = tid; i < n; i += 1024) {
            float x, y, z, d;
            if (IN_LDS) { const float4 q = cache[i]; x = q.x; y = q.y; z = q.z; d = q.w; }
            else { x = p[3 * i]; y = p[3 * i + 1]; z = p[3 * i + 2]; d = dg[i]; }
            const float dx = x - cx, dy = y - cy, dz = z - cz;
            float s = dx * dx;
            s = s + dy * dy;
            s = s + dz * dz;
            if (s < d) {  // distance[mask] = dist[mask]
                d = s;
                if (IN_LDS) cache[i].w = d; else dg[i] = d;
            }
            const unsigned long long k = fps_key(d, i);
            best = k > best ? k : best;
        }
        best = wave_max_u64(best);
        if (lane == 0) wbest[it & 1][wave] = best;
        __syncthreads();
        unsigned long long all = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            const unsigned long long x = wbest[it & 1][w];
            all = x > all ? x : all;
        }
        far = (int)(0xffffffffu - (unsigned)all);
        if constexpr (COUNTED) far = min(far, n - 1);  // (all distances NaN: no key beats 0 -- memory safety only)
    }
}

template <bool IN_LDS>
__global__ __launch_bounds__(1024) void fps_kernel(const float *__restrict__ pts,
                                                   const int32_t *__restrict__ start,
                                                   int32_t *__restrict__ out, float *__restrict__ dist_g,
                                                   int n, int S) {
    fps_body<IN_LDS, false>(pts, nullptr, start, out, nullptr, dist_g, n, S);
}

extern "C" int rrl_fps(const float *pts, const int32_t *start, int32_t *out_idx, float *dist_scratch,
                       int B, int n, int S, void *stream) {
    if (!pts || !start || !out_idx || !dist_scratch || B < 0 || n <= 0 || S < 0 || S > n) return RRL_E_ARG;
    if (B == 0 || S == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    if ((size_t)n * 16 <= 128 * 1024)
        hipLaunchKernelGGL(fps_kernel<true>, dim3((unsigned)B), dim3(1024), (size_t)n * 16, s, pts, start,
                           out_idx, dist_scratch, n, S);
    else
        hipLaunchKernelGGL(fps_kernel<false>, dim3((unsigned)B), dim3(1024), 0, s, pts, start, out_idx,
                           dist_scratch, n, S);
    RRL_LAUNCH_CHECK();
    return 0;
}

// k nearest neighbours (k = 3) of S query points among the n points of their cloud, by brute
// force in double precision (what sklearn's KDTree compares), ties to the lower index.  Lane =
// query, the candidate point is wave-uniform (scalar loads).
__global__ __launch_bounds__(256) void knn3_kernel(const float *__restrict__ pts,
                                                   const int32_t *__restrict__ query_idx,
                                                   int32_t *__restrict__ nn, int n, int S) {
    const int b = blockIdx.y;
    const int q = blockIdx.x * 256 + threadIdx.x;
    const float *p = pts + (size_t)b * n * 3;
    const int qi = q < S ? query_idx[(size_t)b * S + q] : 0;
    const double qx = p[3 * qi], qy = p[3 * qi + 1], qz = p[3 * qi + 2];
    double d0 = 1e300, d1 = 1e300, d2 = 1e300;
    int i0 = 0, i1 = 0, i2 = 0;
    kptr tp = (kptr)(uintptr_t)p;
    for (int j = 0; j < n; ++j, tp += 3) {
        const double dx = qx - (double)tp[0], dy = qy - (double)tp[1], dz = qz - (double)tp[2];
        const double d = (dx * dx + dy * dy) + dz * dz;
        if (d < d2) {
            if (d < d1) {
                d2 = d1; i2 = i1;
                if (d < d0) { d1 = d0; i1 = i0; d0 = d; i0 = j; }
                else { d1 = d; i1 = j; }
            } else { d2 = d; i2 = j; }
        }
    }
    if (q < S) {
        int32_t *o = nn + ((size_t)b * S + q) * 3;
        o[0] = i0; o[1] = i1; o[2] = i2;
    }
}

extern "C" int rrl_knn3(const float *pts, const int32_t *query_idx, int32_t *nn, int B, int n, int S,
                        void *stream) {
    if (!pts || !query_idx || !nn || B < 0 || n <= 0 || S < 0) return RRL_E_ARG;
    if (B == 0 || S == 0) return 0;
    hipLaunchKernelGGL(knn3_kernel, dim3((unsigned)((S + 255) / 256), (unsigned)B), dim3(256), 0,
                       (hipStream_t)stream, pts, query_idx, nn, n, S);
    RRL_LAUNCH_CHECK();
    return 0;
}

// ---- counted entries (include/rrl.h "pseudo-triangles on the device"): ragged batches, no host round trip ----------------
// Kernels of their own, so that fps_kernel and knn3_kernel above keep their code (the FPS pair shares one body template).

// fps_body<IN_LDS, true>: the ragged instantiation, described at the body
template <bool IN_LDS>
__global__ __launch_bounds__(1024) void fps_counted_kernel(const float *__restrict__ pts, const int32_t *__restrict__ counts,
                                                           const int32_t *__restrict__ start, int32_t *__restrict__ out,
                                                           int32_t *__restrict__ out_cnt, float *__restrict__ dist_g,
                                                           int ncap, int S) {
    fps_body<IN_LDS, true>(pts, counts, start, out, out_cnt, dist_g, ncap, S);
}

extern "C" int rrl_fps_counted(const float *pts, const int32_t *counts, const int32_t *start, int32_t *out_idx,
                               int32_t *out_counts, float *dist_scratch, int B, int n, int S, void *stream) {
    if (!pts || !start || !out_idx || !dist_scratch || B < 0 || n <= 0 || S < 0 || S > n) return RRL_E_ARG;
    if (B == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    if ((size_t)n * 16 <= 128 * 1024)
        hipLaunchKernelGGL(fps_counted_kernel<true>, dim3((unsigned)B), dim3(1024), (size_t)n * 16, s, pts, counts, start,
                           out_idx, out_counts, dist_scratch, n, S);
    else
        hipLaunchKernelGGL(fps_counted_kernel<false>, dim3((unsigned)B), dim3(1024), 0, s, pts, counts, start, out_idx,
                           out_counts, dist_scratch, n, S);
    RRL_LAUNCH_CHECK();
    return 0;
}

// knn3_kernel's loop over the first n_b points of sample b for its first S_b = clamp(qcounts[b], 0, S) queries (NULL: S);
// query_idx == NULL: query q is point q.  A sample of fewer than three points has no neighbours: S_b = 0.  Query indices
// are clamped into [0, n_b).  Rows beyond S_b are zero.  tri (optional): [pts[nn0], pts[nn1], pts[nn2]] per query;
// tri_cnt (optional): S_b.
__global__ __launch_bounds__(256) void knn3_counted_kernel(const float *__restrict__ pts, const int32_t *__restrict__ counts,
                                                           const int32_t *__restrict__ query_idx,
                                                           const int32_t *__restrict__ qcounts, int32_t *__restrict__ nn,
                                                           float *__restrict__ tri, int32_t *__restrict__ tri_cnt, int ncap,
                                                           int S) {
    const int b = blockIdx.y;
    const int q = blockIdx.x * 256 + threadIdx.x;
    const int nraw = rrl_rows(counts, b, ncap);  // uniform
    const int n = nraw >= 3 ? nraw : 0;
    const int Sb = n ? rrl_rows(qcounts, b, S) : 0;
    if (blockIdx.x == 0 && threadIdx.x == 0 && tri_cnt != nullptr) tri_cnt[b] = Sb;
    const float *p = pts + (size_t)b * ncap * 3;
    if ((int)blockIdx.x * 256 >= Sb) {  // uniform: nothing but absent rows
        if (q < S) {
            int32_t *o = nn + ((size_t)b * S + q) * 3;
            o[0] = 0; o[1] = 0; o[2] = 0;
            if (tri != nullptr)
                for (int c = 0; c < 9; ++c) tri[((size_t)b * S + q) * 9 + c] = 0.0f;
        }
        return;
    }
    int qi = q < Sb ? (query_idx ? query_idx[(size_t)b * S + q] : q) : 0;
    qi = min(max(qi, 0), n - 1);
    int i0, i1, i2;
    knn3_brute_loop(p, n, qi, i0, i1, i2);
    if (q < S) {
        const bool live = q < Sb;
        int32_t *o = nn + ((size_t)b * S + q) * 3;
        o[0] = live ? i0 : 0; o[1] = live ? i1 : 0; o[2] = live ? i2 : 0;
        if (tri != nullptr) {
            float *t = tri + ((size_t)b * S + q) * 9;
            const int src[3] = {i0, i1, i2};
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int c = 0; c < 3; ++c) t[3 * k + c] = live ? p[3 * src[k] + c] : 0.0f;
        }
    }
}

extern "C" int rrl_knn3_counted(const float *pts, const int32_t *counts, const int32_t *query_idx, const int32_t *qcounts,
                                int32_t *nn, float *tri, int32_t *tri_counts, int B, int n, int S, void *stream) {
    if (!pts || !nn || B < 0 || n <= 0 || S < 0) return RRL_E_ARG;
    if (query_idx == nullptr && S > n) return RRL_E_ARG;  // row order: query q is point q
    if (B == 0) return 0;
    if (S == 0 && tri_counts == nullptr) return 0;
    hipLaunchKernelGGL(knn3_counted_kernel, dim3((unsigned)((S + 255) / 256 > 0 ? (S + 255) / 256 : 1), (unsigned)B), dim3(256), 0,
                       (hipStream_t)stream, pts, counts, query_idx, qcounts, nn, tri, tri_counts, n, S);
    RRL_LAUNCH_CHECK();
    return 0;
}
