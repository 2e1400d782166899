// rrl_group.hip -- ball-query grouping and the raw point-pair features of RPM-Net's feature extractor
// (rpm/models/pointnet_util.py:96-131 query_ball_point, :173-244 angle / sample_and_group_multi) as ONE launch:
// include/rrl.h "ball-query grouping", DESIGN.md section 18.
//
// One wavefront per query, RRL_GROUP_WAVES queries of the same sample per workgroup; the waves of a workgroup share
// nothing (no barrier).  Candidates are visited in ascending tiles of 64 read straight from the cloud (a few KB, cache
// resident): lane = candidate, one float64 distance each -- the 3-NN kernels' (dx dx + dy dy) + dz dz, uncontracted --, a
// 64-bit ballot, slot = found + (members below the lane); slots under nsample go to the wave's list in LDS and the wave
// leaves the loop once the list is full (a wave-uniform test).  The feature phase runs with lane = slot.  No atomics,
// nothing indexed by unclamped data, every value a function of its own sample only: two calls give the same bits, and
// sample b of a ragged batch has the bits of its own B = 1 call.
#include "rrl_common.h"

#define RRL_GROUP_WAVES 4
#define RRL_GROUP_MAX_C 10

// angle(a, b) = atan2(|a x b|, a . b) of pointnet_util.py:173-194, in double from float32 inputs, rounded once by the
// caller.  Uncontracted, a x a is exactly 0, and atan2(0, 0) = 0: a pad slot (d = 0, n_j = n_i) gives exact zeros.  The dot
// product is summed from +0 like torch.sum: three products of -0 (a normal with negative components times d = 0) would
// otherwise add up to -0, and atan2(0, -0) is pi.
__device__ __forceinline__ double group_angle(double ax, double ay, double az, double bx, double by, double bz) {
    const double cx = ay * bz - az * by;
    const double cy = az * bx - ax * bz;
    const double cz = ax * by - ay * bx;
    const double cn = sqrt((cx * cx + cy * cy) + cz * cz);
    const double dot = ((0.0 + ax * bx) + ay * by) + az * bz;
    return atan2(cn, dot);
}

__global__ __launch_bounds__(64 * RRL_GROUP_WAVES) void ball_group_kernel(
    const float *__restrict__ pts, const float *__restrict__ normals, const int32_t *__restrict__ counts,
    const int32_t *__restrict__ query_idx, const int32_t *__restrict__ qcounts, double r2, int nsample, int exclude_self,
    int channels, int32_t *__restrict__ idx, int32_t *__restrict__ found_out, float *__restrict__ feat, int ncap, int S) {
    __shared__ int32_t list[RRL_GROUP_WAVES][64];
    __shared__ float stage[RRL_GROUP_WAVES][64 * RRL_GROUP_MAX_C];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int b = blockIdx.y;
    const int q = (int)blockIdx.x * RRL_GROUP_WAVES + w;  // wave-uniform
    if (q >= S) return;
    const int n = rrl_rows(counts, b, ncap);
    int Sb = n > 0 ? rrl_rows(qcounts, b, S) : 0;
    if (query_idx == nullptr) Sb = min(Sb, n);  // query q is point q: it has to exist
    const int C = ((channels & RRL_GROUP_XYZ) ? 3 : 0) + ((channels & RRL_GROUP_DXYZ) ? 3 : 0) + ((channels & RRL_GROUP_PPF) ? 4 : 0);
    const size_t row = (size_t)b * S + q;
    int32_t *orow = idx + row * nsample;
    float *frow = feat != nullptr ? feat + row * nsample * C : nullptr;
    if (q >= Sb) {  // an absent row: zeros
        if (lane < nsample) orow[lane] = 0;
        if (lane == 0) found_out[row] = 0;
        if (frow != nullptr)
            for (int t = lane; t < nsample * C; t += 64) frow[t] = 0.0f;
        return;
    }
    const float *p = pts + (size_t)b * ncap * 3;
    int qi = query_idx ? query_idx[row] : q;
    qi = __builtin_amdgcn_readfirstlane(min(max(qi, 0), n - 1));
    const float qxf = p[3 * qi], qyf = p[3 * qi + 1], qzf = p[3 * qi + 2];
    const double qx = qxf, qy = qyf, qz = qzf;

    int found = 0;  // wave-uniform
    for (int base = 0; base < n && found < nsample; base += 64) {
        const int j = base + lane;
        bool member = false;
        if (j < n) {
            const double dx = qx - (double)p[3 * j], dy = qy - (double)p[3 * j + 1], dz = qz - (double)p[3 * j + 2];
            const double d = (dx * dx + dy * dy) + dz * dz;
            member = d <= r2 && !(exclude_self && j == qi);  // (a NaN distance compares false)
        }
        const unsigned long long bal = __ballot(member);
        const int below = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
        const int slot = found + below;
        if (member && slot < nsample) list[w][slot] = j;
        found += __popcll(bal);
    }
    found = min(found, nsample);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();  // the list was written and is read by this wavefront alone

    if (lane == 0) found_out[row] = found;
    int j = 0;
    if (lane < nsample) {
        const int pad = exclude_self ? qi : (found > 0 ? list[w][0] : qi);
        j = lane < found ? list[w][lane] : pad;
        orow[lane] = j;
    }
    if (frow == nullptr) return;

    if (lane < nsample) {
        float *o = &stage[w][lane * C];
        const float dxf = p[3 * j] - qxf, dyf = p[3 * j + 1] - qyf, dzf = p[3 * j + 2] - qzf;
        if (channels & RRL_GROUP_XYZ) { o[0] = qxf; o[1] = qyf; o[2] = qzf; o += 3; }
        if (channels & RRL_GROUP_DXYZ) { o[0] = dxf; o[1] = dyf; o[2] = dzf; o += 3; }
        if (channels & RRL_GROUP_PPF) {
            const float *nb = normals + (size_t)b * ncap * 3;
            const double nix = nb[3 * qi], niy = nb[3 * qi + 1], niz = nb[3 * qi + 2];
            const double njx = nb[3 * j], njy = nb[3 * j + 1], njz = nb[3 * j + 2];
            const double dx = dxf, dy = dyf, dz = dzf;
            o[0] = (float)group_angle(nix, niy, niz, dx, dy, dz);
            o[1] = (float)group_angle(njx, njy, njz, dx, dy, dz);
            o[2] = (float)group_angle(nix, niy, niz, njx, njy, njz);
            o[3] = (float)sqrt((dx * dx + dy * dy) + dz * dz);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int t = lane; t < nsample * C; t += 64) frow[t] = stage[w][t];  // whole [nsample][C] rows, coalesced
}

extern "C" int rrl_ball_group(const float *pts, const float *normals, const int32_t *counts, const int32_t *query_idx,
                              const int32_t *qcounts, float r2, int nsample, int exclude_self, int channels, int32_t *idx,
                              int32_t *found, float *feat, int B, int n, int S, void *stream) {
    if (!pts || !idx || !found) return RRL_E_ARG;
    if (B < 1 || B > 32767 || n < 1 || n > rrl_sort_capacity() || S < 0) return RRL_E_ARG;
    if (query_idx == nullptr && S > n) return RRL_E_ARG;  // row order: query q is point q
    if (nsample < 1 || nsample > RRL_GROUP_MAX_SAMPLE) return RRL_E_ARG;
    if (!(r2 >= 0.0f)) return RRL_E_ARG;  // negative or NaN
    if (channels < 0 || channels > (RRL_GROUP_XYZ | RRL_GROUP_DXYZ | RRL_GROUP_PPF)) return RRL_E_ARG;
    if ((channels != 0) != (feat != nullptr)) return RRL_E_ARG;
    if ((channels & RRL_GROUP_PPF) && !normals) return RRL_E_ARG;
    if (S == 0) return 0;
    const unsigned gx = (unsigned)((S + RRL_GROUP_WAVES - 1) / RRL_GROUP_WAVES);
    hipLaunchKernelGGL(ball_group_kernel, dim3(gx, (unsigned)B), dim3(64 * RRL_GROUP_WAVES), 0, (hipStream_t)stream, pts, normals,
                       counts, query_idx, qcounts, (double)r2, nsample, exclude_self ? 1 : 0, channels, idx, found, feat, n, S);
    RRL_LAUNCH_CHECK();
    return 0;
}
