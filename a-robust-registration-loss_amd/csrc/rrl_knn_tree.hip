// rrl_knn_tree.hip -- exact 3 nearest neighbours of EVERY point of a cloud through the sorted layout
// (include/rrl.h rrl_knn3_self): the all-points form of the pseudo-triangle builder (code/loss.py:473-485), where brute
// force (rrl_neigh.hip knn3_kernel) costs n^2 float64 distances per cloud.
//
// Build (reused, nothing new): the Chamfer monitor's build of a point cloud, in a scratch of this entry's own -- up to
// 4096 points tri_sort_kernel<4, true> straight from the points, beyond that pts_records_kernel + the big_* kernels
// (rrl_cull.hip rrl_launch_cloud_sort): (x, y, z, original index) records in 16^3-cell Hilbert order, supergroups of 64
// records with the 13-node sphere tree of rrl_tree.h, max |P|^2 per sample (PMAX; +inf for a NaN, an infinite or an
// overflowing coordinate).  That launcher always builds a pair of clouds; its second cloud gets per-sample counts of 0 here
// (a word row of the scratch, cleared by the launch in front), so its workgroups leave at once.
//
// Walk (new): one wavefront owns the 64 consecutive SORTED queries of supergroup `sg`, one per lane, each lane with its
// three best keys (d, original index) in registers, d = (dx dx + dy dy) + dz dz in float64 from the float32 coordinates
// (knn3_kernel's formula; -ffp-contract=off).
//   own     the wavefront's own supergroup is evaluated first for all lanes: three neighbours from a compact cell are
//           already a tight bound;
//   flat    the other supergroups j = sg + 1, sg - 1, sg + 2, ... (along the Hilbert curve near means near, so the bounds
//           tighten early), 64 per round, one per lane: lane-parallel test of supergroup j's sphere against the QUERY
//           supergroup's sphere with the largest bound of the wavefront;
//   lane    per surviving supergroup every lane tests its own query with its own current bound against the supergroup
//           sphere, then against each of its four group spheres; a group of 16 records is evaluated -- for the whole
//           wavefront, the records arrive through the scalar cache -- when ANY lane needs it.
// A flat pass costs n / 64 sphere tests per wavefront, n^2 / 4096 in all: at n = 2^20 that is 2.7e8 lane tests, noise
// beside the evaluated pairs, so no level above the supergroups is built.
//
// Exactness.  Result per query: the three smallest keys (d, index) in lexicographic order over ALL points of the sample,
// the query and its duplicates included -- what knn3_kernel's ascending loop with `<` returns (lowest index among equal
// distances).  The walk visits in sorted order, so a key is inserted when d is smaller OR d is equal and the index is
// smaller (knn_push); any visiting order then gives the same three keys.
// Bound.  A node is (c, R) with R >= max |p - c| over its records, conservative (finish_sphere: rho = sqrtf(max e2)
// (1 + 1e-5) + 1e-7, R = rho (1 + 5e-5) + 1e-7, against a relative error of ~3e-7 of e2 in float32).  For a query q with
// third-best distance d3 every record p of the node has |q - p| >= |q - c| - R, so the node holds no key below or EQUAL
// to the third key when |q - c| > sqrt(d3) + R.  Evaluated in float32 so that rounding can only keep a node:
//   left   D = |q - c|^2 from the float32 coordinates (relative error < 4e-7; an underflow makes it smaller), shrunk
//          by LB_SCALE = 0.9999;
//   right  sb = sqrtf(max((float)d3, 1e-30f)) * 1.00001f >= sqrt(d3) (the conversion rounds by 6e-8, the approximate
//          root by 1e-7; the floor keeps a flushed denormal from becoming 0; 1e300 = "no third key yet" becomes +inf),
//          t = sb + R, rounded by 6e-8;
//   skip   iff D * LB_SCALE > t * t, a STRICT comparison with 1e-4 of relative slack in the squares against 1e-6 of error:
//          then |q - c|^2 > (sqrt(d3) + R)^2 (1 + 5e-5), every record of the node is strictly farther than the third key
//          by far more than the 1e-16 of the float64 evaluation, and no tie can hide in it.  Equality never prunes.
//   The wavefront-level test is the same inequality between two spheres: |cq - cj| > sbmax + Rq + Rj with sbmax the
//   largest sb of the wavefront's real queries implies the lane test for every lane.
// Degenerate clouds (identical points, collinear points, far clusters) make radii or bounds useless and cost time only.
// Non-finite or huge coordinates: where PMAX of the sample is not <= 1e30 (a NaN, an infinity, |P| > 1e15: float32 squares
// would overflow and finish_sphere caps R at 1e18) the sample is served by knn3_kernel's loop itself -- lane = ORIGINAL row,
// ascending index, `<` -- a workgroup-uniform branch on a word the build left on the device; nothing of the sort is read.
// A sample of fewer than three points has no neighbours: its rows are zero and its triangle count is 0.
#include "rrl_tree.h"
#include "rrl_chamfer_walk.h"  // LB_SCALE, kptr
#include "rrl_knn3_loop.h"

// the scratch of rrl_knn3_self (include/rrl.h rrl_knn3_self_workspace_bytes)
struct KnnLayout {
    size_t crec, p0s, idx, grp, apart, pmax, zero, histg, zcnt, total;
    int nblk;
    __host__ KnnLayout(int B, int n_) {
        const size_t b = (size_t)B, n = (size_t)n_;
        nblk = (int)((n + 255) / 256);
        size_t o = 0;
        auto take = [&](size_t bytes) { size_t at = o; o += (bytes + 255) & ~(size_t)255; return at; };
        crec = take(n > 4096 ? 16 * b * ((n + 15) / 16) * 16 : 16);
        p0s = take(16 * b * ((n + 63) / 64) * 64);
        idx = take(4 * b * ((n + 63) / 64) * 64);
        grp = take(16 * b * ((n + 63) / 64) * NODE);
        apart = take(4 * 2 * b * 8 * (size_t)nblk);  // (the pair build's rows: cloud 0's are used)
        pmax = take(4 * 2 * b);
        zero = o;                                     // cleared by the launch in front of the sort, up to the end:
        histg = take(n > 4096 ? 4 * 2 * b * 2 * SORT_CELLS : 16);
        zcnt = take(4 * b);                           // the counts of the pair build's absent second cloud
        total = o;
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
// sb of the header: an upper bound of sqrt(d3) in float32
__device__ __forceinline__ float knn_bound(double d3) {
    return __builtin_amdgcn_sqrtf(fmaxf((float)d3, 1e-30f)) * 1.00001f;
}
// may the sphere (cx, cy, cz, R) hold a key not above the bound sb of query (qx, qy, qz)?  (NaN anywhere: yes)
__device__ __forceinline__ bool knn_reach(float qx, float qy, float qz, float cx, float cy, float cz, float R, float sb) {
    const float dx = qx - cx, dy = qy - cy, dz = qz - cz;
    const float D = dx * dx + dy * dy + dz * dz, t = sb + R;
    return !(D * LB_SCALE > t * t);
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
        eval(sg * SGT, min(SGT, n - sg * SGT));  // own supergroup
        kptr qn = (kptr)(uintptr_t)(T + (size_t)sg * NODE);
        const float cqx = qn[0], cqy = qn[1], cqz = qn[2], Rq = qn[3];
        const int kmax = 2 * max(sg, nsg - 1 - sg);  // offsets 1 .. kmax reach every other supergroup
        for (int k0 = 1; k0 <= kmax; k0 += 64) {
            const int kk = k0 + lane;
            const int j = sg + ((kk & 1) ? (kk + 1) / 2 : -(kk / 2));
            const float sbmax = wave_max(valid ? knn_bound(k.d2) : 0.0f);
            bool cand = false;
            if (kk <= kmax && j >= 0 && j < nsg) {
                const float4 c = T[(size_t)j * NODE];
                cand = knn_reach(cqx, cqy, cqz, c.x, c.y, c.z, c.w, sbmax + Rq);
            }
            unsigned long long m = __ballot(cand);
            while (m) {
                const int sl = __ffsll((long long)m) - 1;
                m &= m - 1;
                const int jj = __builtin_amdgcn_readlane(j, sl);
                kptr jn = (kptr)(uintptr_t)(T + (size_t)jj * NODE);
                if (!__any(valid && knn_reach(q.x, q.y, q.z, jn[0], jn[1], jn[2], jn[3], knn_bound(k.d2)))) continue;
                for (int g = 0; g < SGG; ++g) {
                    const int pos0 = jj * SGT + g * GRP, cnt = min(GRP, n - pos0);
                    if (cnt <= 0) break;
                    const bool need = valid && knn_reach(q.x, q.y, q.z, jn[4 * (1 + g)], jn[4 * (1 + g) + 1], jn[4 * (1 + g) + 2],
                                                         jn[4 * (1 + g) + 3], knn_bound(k.d2));
                    if (__any(need)) eval(pos0, cnt);
                }
            }
        }
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
    const bool small = n <= 4096;  // the sort kernel reads the points itself: no records launch
    int rc;
    if (small) rc = rrl_fill(w + L.zero, 0u, L.total - L.zero, s);
    else rc = rrl_launch_pts_records(pts, (float4 *)(w + L.crec), (float *)(w + L.apart), w + L.zero, (L.total - L.zero) / 16, B, n,
                                     L.nblk, counts, s);
    if (rc) return rc;
    // the pair build with an absent second cloud (counts of 0: its pointers are never followed)
    rc = rrl_launch_cloud_sort(small ? pts : nullptr, small ? pts : nullptr, (float4 *)(w + L.crec), (float4 *)(w + L.crec),
                               (float *)(w + L.apart), L.nblk, (float4 *)(w + L.p0s), (float4 *)(w + L.p0s),
                               (int32_t *)(w + L.idx), (int32_t *)(w + L.idx), (float4 *)(w + L.grp), (float4 *)(w + L.grp),
                               (uint32_t *)(w + L.pmax), (unsigned *)(w + L.histg), nullptr, 0, B, n, n, counts,
                               (const int32_t *)(w + L.zcnt), s);
    if (rc) return rc;
    hipLaunchKernelGGL(knn3_tree_kernel, dim3((unsigned)((n + SGT - 1) / SGT), (unsigned)B), dim3(64), 0, s, pts, counts,
                       (const float4 *)(w + L.p0s), (const float4 *)(w + L.grp), (const uint32_t *)(w + L.pmax), nn, tri,
                       tri_counts, n);
    RRL_LAUNCH_CHECK();
    return 0;
}
