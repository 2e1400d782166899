// rrl_knn_walk.h -- the k-nearest-neighbour walk over a cloud in the sorted layout (rrl_tree.h: Hilbert order, supergroups of
// 64 records under a 13-node sphere tree), its bound and the proof that the bound is safe, for knn3_tree_kernel
// (rrl_knn_tree.hip, k = 3, keys in registers) and knn_kernel<true, KU> (rrl_knn.hip, any k, keys in LDS).  Both use the bound;
// knn3_tree_kernel calls knn_walk_others, knn_kernel holds the same loop in its own text (measured slower through the call:
// see there).
//
// One wavefront owns 64 consecutive SORTED queries, one per lane, each with its list of best keys (d, original index),
// d = (dx dx + dy dy) + dz dz in float64 from the float32 coordinates.  The caller evaluates a SEED supergroup of the
// reference for all lanes first (its own in a self search: neighbours from a compact cell are already a tight bound), then
// knn_walk_others visits the rest:
//   flat    the other supergroups j = seed + 1, seed - 1, seed + 2, ... (along the Hilbert curve near means near, so the
//           bounds tighten early), 64 per round, one per lane: lane-parallel test of supergroup j's sphere against the QUERY
//           supergroup's sphere with the largest bound of the wavefront;
//   lane    per surviving supergroup every lane tests its own query with its own current bound against the supergroup
//           sphere, then against each of its four group spheres; a group of 16 records is evaluated -- for the whole
//           wavefront, the records arrive through the scalar cache -- when ANY lane needs it.
// A flat pass costs n / 64 sphere tests per wavefront, n^2 / 4096 in all: at n = 2^20 that is 2.7e8 lane tests, noise
// beside the evaluated pairs, so no level above the supergroups is built.
//
// Bound.  Let dk be the d of the lane's k-th key, 1e300 while fewer than k keys are held (a list that is not full prunes
// nothing).  A node is (c, R) with R >= max |p - c| over its records, conservative (finish_sphere: rho = sqrtf(max e2)
// (1 + 1e-5) + 1e-7, R = rho (1 + 5e-5) + 1e-7, against a relative error of ~3e-7 of e2 in float32).  Every record p of the
// node has |q - p| >= |q - c| - R, so when |q - c| > sqrt(dk) + R every record is STRICTLY farther than the k-th key, cannot
// be lexicographically below it, and cannot enter the list -- now or later, because dk only decreases.  Evaluated in float32
// so that rounding can only keep a node:
//   left   D = |q - c|^2 from the float32 coordinates (relative error < 4e-7; an underflow makes it smaller), shrunk
//          by LB_SCALE = 0.9999;
//   right  sb = sqrtf(max((float)dk, 1e-30f)) * 1.00001f >= sqrt(dk) (knn_bound: the conversion rounds by 6e-8, the
//          approximate root by 1e-7; the floor keeps a flushed denormal from becoming 0; 1e300 becomes +inf),
//          t = sb + R, rounded by 6e-8;
//   skip   iff D * LB_SCALE > t * t, a STRICT comparison with 1e-4 of relative slack in the squares against 1e-6 of error:
//          then |q - c|^2 > (sqrt(dk) + R)^2 (1 + 5e-5), every record of the node is strictly farther than the k-th key
//          by far more than the 1e-16 of the float64 evaluation, and no tie can hide in it.  Equality never prunes, a NaN
//          anywhere keeps the node.
//   The wavefront-level test is the same inequality between two spheres: |cq - cj| > sbmax + Rq + Rj, with (cq, Rq) the
//   query supergroup's sphere and sbmax the largest sb of the wavefront's real queries, implies the lane test for every lane.
// Degenerate clouds (identical points, collinear points, far clusters) make radii or bounds useless and cost time only.
#pragma once
#include "rrl_tree.h"
#include "rrl_chamfer_walk.h"  // LB_SCALE

// sb of the header: an upper bound of sqrt(dk) in float32
__device__ __forceinline__ float knn_bound(double dk) {
    return __builtin_amdgcn_sqrtf(fmaxf((float)dk, 1e-30f)) * 1.00001f;
}
// may the sphere (cx, cy, cz, R) hold a key not above the bound sb of query (qx, qy, qz)?  (NaN anywhere: yes)
__device__ __forceinline__ bool knn_reach(float qx, float qy, float qz, float cx, float cy, float cz, float R, float sb) {
    const float dx = qx - cx, dy = qy - cy, dz = qz - cz;
    const float D = dx * dx + dy * dy + dz * dz, t = sb + R;
    return !(D * LB_SCALE > t * t);
}

// The supergroups of the reference other than `seed` (which the caller has evaluated), for the wavefront's 64 queries:
// T the reference's tree (nsg supergroups, nr records), (cqx, cqy, cqz, Rq) the query supergroup's sphere, (qx, qy, qz)
// the lane's query, valid: the lane holds one.  kth() returns the d of the lane's current k-th key; eval(pos0, cnt) offers
// `cnt` records from sorted position pos0 to every lane.
template <typename Kth, typename Eval>
__device__ __forceinline__ void knn_walk_others(const float4 *__restrict__ T, int nsg, int nr, int seed, float cqx, float cqy,
                                                float cqz, float Rq, float qx, float qy, float qz, bool valid, int lane,
                                                Kth kth, Eval eval) {
    const int kmax = 2 * max(seed, nsg - 1 - seed);  // offsets 1 .. kmax reach every other supergroup
    for (int k0 = 1; k0 <= kmax; k0 += 64) {
        const int kk = k0 + lane;
        const int j = seed + ((kk & 1) ? (kk + 1) / 2 : -(kk / 2));
        const float sbmax = wave_max(valid ? knn_bound(kth()) : 0.0f);
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
            if (!__any(valid && knn_reach(qx, qy, qz, jn[0], jn[1], jn[2], jn[3], knn_bound(kth())))) continue;
            for (int g = 0; g < SGG; ++g) {
                const int pos0 = jj * SGT + g * GRP, cnt = min(GRP, nr - pos0);
                if (cnt <= 0) break;
                const bool need = valid && knn_reach(qx, qy, qz, jn[4 * (1 + g)], jn[4 * (1 + g) + 1], jn[4 * (1 + g) + 2],
                                                     jn[4 * (1 + g) + 3], knn_bound(kth()));
                if (__any(need)) eval(pos0, cnt);
            }
        }
    }
}
