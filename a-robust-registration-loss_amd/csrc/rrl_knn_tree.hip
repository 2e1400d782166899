// rrl_knn_tree.hip -- exact 3 nearest neighbours of EVERY point of a cloud through the sorted layout
// (include/rrl.h rrl_knn3_self): the all-points form of the pseudo-triangle builder (code/loss.py:473-485), where brute
// force (rrl_neigh.hip knn3_kernel) costs n^2 float64 distances per cloud.
//
// Build (reused, nothing new): the Chamfer monitor's build of a point cloud, in a scratch of this entry's own -- up to
// 4096 points tri_sort_kernel<4, true> straight from the points, beyond that pts_records_kernel + the big_* kernels
// (rrl_cull.hip rrl_launch_cloud_sort): (x, y, z, original index) records in 16^3-cell Hilbert order, supergroups of 64
// records with the 13-node sphere tree of rrl_tree.h, max |P|^2 per sample (PMAX; +inf for a NaN, an infinite or an
// overflowing coordinate).  That launcher always builds a pair of clouds; its second cloud is absent here (PairLayout,
// rrl_tree.h) and gets per-sample counts of 0 -- a word row of the scratch, cleared by the launch in front -- so its
// workgroups leave at once.
//
// Walk: rrl_knn_walk.h, with the bound and its proof.  One wavefront owns the 64 consecutive SORTED queries of supergroup
// `sg`, one per lane, each lane with its three best keys (d, original index) in registers (knn3_kernel's formula;
// -ffp-contract=off); the seed is the wavefront's own supergroup.
//
// Exactness.  Result per query: the three smallest keys (d, index) in lexicographic order over ALL points of the sample,
// the query and its duplicates included -- what knn3_kernel's ascending loop with `<` returns (lowest index among equal
// distances).  The walk visits in sorted order, so a key is inserted when d is smaller OR d is equal and the index is
// smaller (knn_push); any visiting order then gives the same three keys.
// Non-finite or huge coordinates: where PMAX of the sample is not <= 1e30 (a NaN, an infinity, |P| > 1e15: float32 squares
// would overflow and finish_sphere caps R at 1e18) the sample is served by knn3_kernel's loop itself -- lane = ORIGINAL row,
// ascending index, `<` -- a workgroup-uniform branch on a word the build left on the device; nothing of the sort is read.
// A sample of fewer than three points has no neighbours: its rows are zero and its triangle count is 0.
#include "rrl_knn_walk.h"
#include "rrl_knn3_loop.h"

// the scratch of rrl_knn3_self (include/rrl.h rrl_knn3_self_workspace_bytes): the pair build of one cloud and the counts of the
// absent second one, which the launch in front of the sort clears together with HISTG
struct KnnLayout : PairLayout {
    size_t zcnt, total;
    __host__ KnnLayout(int B_, int n) : PairLayout(B_, n, -1) {
        zcnt = take(4 * (size_t)B);
        total = end;
    }
};

extern "C" size_t rrl_knn3_self_workspace_bytes(int B, int n) {
    if (B < 0 || n < 0) return 0;
    return KnnLayout(B, n).total;
}

struct Best3 {
    double d0, d1, d2;
    int i0, i1, i2;
};
// insert key (d, j) when it is lexicographically below the third key
__device__ __forceinline__ void knn_push(Best3 &k, double d, int j) {
    if (d < k.d2 || (d == k.d2 && j < k.i2)) {
        if (d < k.d1 || (d == k.d1 && j < k.i1)) {
            k.d2 = k.d1; k.i2 = k.i1;
            if (d < k.d0 || (d == k.d0 && j < k.i0)) { k.d1 = k.d0; k.i1 = k.i0; k.d0 = d; k.i0 = j; }
            else { k.d1 = d; k.i1 = j; }
        } else { k.d2 = d; k.i2 = j; }
    }
}

__global__ __launch_bounds__(64) void knn3_tree_kernel(const float *__restrict__ pts, const int32_t *__restrict__ counts,
                                                       const float4 *__restrict__ p0s, const float4 *__restrict__ grp,
                                                       const uint32_t *__restrict__ pmax, int32_t *__restrict__ nn,
                                                       float *__restrict__ tri, int32_t *__restrict__ tri_cnt, int ncap) {
    const int lane = threadIdx.x, sg = blockIdx.x, b = blockIdx.y;
    const int nraw = rrl_rows(counts, b, ncap);  // uniform
    const int n = nraw >= 3 ? nraw : 0;
    if (sg == 0 && lane == 0 && tri_cnt != nullptr) tri_cnt[b] = n;
    const float *p = pts + (size_t)b * ncap * 3;
    int32_t *onn = nn + (size_t)b * ncap * 3;
    float *otri = tri != nullptr ? tri + (size_t)b * ncap * 9 : nullptr;
    {   // the rows beyond the sample's count: zero (by grid position; the rows below it are written by their queries)
        const int r = sg * SGT + lane;
        if (r >= n && r < ncap) {
            onn[3 * r] = 0; onn[3 * r + 1] = 0; onn[3 * r + 2] = 0;
            if (otri != nullptr)
                for (int c = 0; c < 9; ++c) otri[(size_t)9 * r + c] = 0.0f;
        }
    }
    if (sg * SGT >= n) return;  // uniform
    Best3 k = {1e300, 1e300, 1e300, 0x7fffffff, 0x7fffffff, 0x7fffffff};
    int row;          // the ORIGINAL row of this lane's query
    bool valid;
    if (!(__uint_as_float(pmax[b]) <= 1.0e30f)) {  // uniform: non-finite or huge coordinates -- knn3_kernel's loop, lane = original row
        row = sg * SGT + lane;
        valid = row < n;
        const int qi = valid ? row : 0;
        knn3_brute_loop(p, n, qi, k.i0, k.i1, k.i2);
    } else {
        const int nsg = (n + SGT - 1) / SGT, nsgf = (ncap + SGT - 1) / SGT;
        const float4 *R = p0s + (size_t)b * nsgf * SGT;
        const float4 *T = grp + (size_t)b * nsgf * NODE;
        const int s_ = sg * SGT + lane;
        valid = s_ < n;
        const float4 q = R[s_];  // pad records exist up to the supergroup boundary
        row = min(max(__float_as_int(q.w), 0), n - 1);  // (a permutation of [0, n): the clamp is memory safety only)
        const double qx = q.x, qy = q.y, qz = q.z;
        // `cnt` records from sorted position pos0 for every lane (uniform addresses: scalar loads)
        auto eval = [&](int pos0, int cnt) {
            kptr rp = (kptr)(uintptr_t)(R + pos0);
            for (int t = 0; t < cnt; ++t, rp += 4) {
                const double dx = qx - (double)rp[0], dy = qy - (double)rp[1], dz = qz - (double)rp[2];
                const double d = (dx * dx + dy * dy) + dz * dz;
                knn_push(k, d, __float_as_int(rp[3]));
            }
        };
        eval(sg * SGT, min(SGT, n - sg * SGT));  // own supergroup: the seed (evaluated BEFORE the node load below; that order is the kernel's code)
        kptr qn = (kptr)(uintptr_t)(T + (size_t)sg * NODE);
        const float cqx = qn[0], cqy = qn[1], cqz = qn[2], Rq = qn[3];
        knn_walk_others(T, nsg, n, sg, cqx, cqy, cqz, Rq, q.x, q.y, q.z, valid, lane, [&] { return k.d2; }, eval);
        k.i0 = min(max(k.i0, 0), n - 1); k.i1 = min(max(k.i1, 0), n - 1); k.i2 = min(max(k.i2, 0), n - 1);  // (memory safety only)
    }
    if (valid) {
        onn[3 * row] = k.i0; onn[3 * row + 1] = k.i1; onn[3 * row + 2] = k.i2;
        if (otri != nullptr) {
            float *t = otri + (size_t)9 * row;
            const int src[3] = {k.i0, k.i1, k.i2};
#pragma unroll
            for (int v = 0; v < 3; ++v)
#pragma unroll
                for (int c = 0; c < 3; ++c) t[3 * v + c] = p[3 * src[v] + c];
        }
    }
}

extern "C" int rrl_knn3_self(const float *pts, const int32_t *counts, void *ws, size_t ws_bytes, int32_t *nn, float *tri,
                             int32_t *tri_counts, int B, int n, void *stream) {
    if (!pts || !ws || !nn || B < 0 || n <= 0 || n > rrl_sort_capacity() || B > 32767) return RRL_E_ARG;
    const KnnLayout L(B, n);
    if (ws_bytes < L.total) return RRL_E_WS;
    if (B == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    char *w = (char *)ws;
    int rc;  // up to 4096 points the sort kernel reads the points itself: no records launch
    if (!L.big) rc = rrl_fill(w + L.histg, 0u, L.total - L.histg, s);
    else rc = rrl_launch_pts_records(pts, (float4 *)(w + L.crec[0]), (float *)(w + L.apart), w + L.histg, (L.total - L.histg) / 16, B, n,
                                     L.nblk, counts, s);
    if (rc) return rc;
    rc = rrl_launch_cloud_sort(L, ws, L.big ? nullptr : pts, nullptr, nullptr, 0, counts, (const int32_t *)(w + L.zcnt), s);
    if (rc) return rc;
    hipLaunchKernelGGL(knn3_tree_kernel, dim3((unsigned)((n + SGT - 1) / SGT), (unsigned)B), dim3(64), 0, s, pts, counts,
                       (const float4 *)(w + L.p0s[0]), (const float4 *)(w + L.grp[0]), (const uint32_t *)(w + L.pmax), nn, tri,
                       tri_counts, n);
    RRL_LAUNCH_CHECK();
    return 0;
}
