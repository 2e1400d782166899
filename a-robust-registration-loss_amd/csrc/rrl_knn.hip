// rrl_knn.hip -- exact k nearest neighbours, any k up to RRL_KNN_MAX_K, with the graph features of DCP's front end
// (include/rrl.h rrl_knn; dcp/model.py:46-78 knn + get_graph_feature without the (B, N, N) matrix, topk, the index-offset
// tensor, repeat, cat and permute).  DESIGN.md section 21.
//
// The result, defined once.  For query q and the n_b reference points of its sample: the k smallest keys (d, j) in
// lexicographic order, d = (dx dx + dy dy) + dz dz in float64 from the float32 coordinates (knn3_kernel's formula;
// -ffp-contract=off), j the ORIGINAL row -- ascending distance, the lowest index among equal distances.  A pair whose d is NaN
// or +inf is no neighbour (`<` against the 1e300 sentinel, as in knn3_brute_loop).  found = min(k, neighbours); the slots at
// or beyond found repeat slot 0; a row with found == 0 is zero in every output.  Self form (qry == NULL): the queries are the
// reference's own rows, the point itself is a neighbour at d = 0 unless RRL_KNN_EXCLUDE_SELF removes the row's own INDEX (a
// duplicate at another index stays).  Cross form: qry [B][S][3] with its own counts.
//
// Where the k keys live.  A per-lane array indexed by a run-time slot would go to scratch memory.  Each lane's list is
// in LDS instead, laid out [slot][lane] -- doubles and indices in separate arrays, consecutive lanes on consecutive banks --
// and sized by the k of the call: 64 k (8 + 4) bytes per wavefront, 24 KiB at k = 32, 15 KiB at k = 20.  One wavefront per
// workgroup (no barrier anywhere: a lane only ever touches its own column).  The column is UNSORTED; the k-th key -- its
// lexicographic maximum -- and that key's slot are cached in registers, so a candidate that does not enter costs one compare
// and no LDS traffic; one that enters replaces the maximum, and one scan of the column finds the new one.  The epilogue
// emits the column in ascending order by selection.  Any visiting order gives the same set: a key enters when it is
// lexicographically below the k-th key, and every (d, j) is offered exactly once.
//
// Two methods, same bits.
//   brute  one lane per query (original row order), the reference streams through the scalar cache in ascending index.
//   tree   both clouds in 16^3-cell Hilbert order under the sphere tree of rrl_tree.h (rrl_launch_cloud_sort: the pair build;
//          its second cloud is the query cloud, absent -- counts of 0 -- in the self form).  One wavefront owns the 64
//          consecutive SORTED queries of query supergroup sg.  It first evaluates a SEED supergroup of the reference for all
//          lanes -- its own in the self form; in the cross form the one whose centre is nearest the query patch's centre (the
//          Chamfer walk's seed) -- then the others by the walk that rrl_knn_walk.h describes, with that header's bound on
//          the k-th key (knn_bound, knn_reach) and its proof that rounding can only keep a node.
// A sample whose PMAX word (either cloud's) is not <= 1e30 -- a NaN, an infinity, |P| > 1e15 -- takes the brute loop inside the
// same launch: a workgroup-uniform branch on a word the build left on the device.
//
// Launch behaviour: no atomics, nothing read back, one plain chain on the caller's stream (3 launches up to 4096 points, 5
// beyond -- 6 in the cross form --, 1 for brute force); two calls give the same bits.
#include "rrl_knn_walk.h"

#define KNN_NONE 0x7fffffff  // the index of an open slot (its d is 1e300)

// the scratch of rrl_knn (include/rrl.h rrl_knn_workspace_bytes): the pair build of (reference, queries) and the counts of the
// self form's absent second cloud; the launch in front of the sort clears it from PMAX to the end
struct KnnPairLayout : PairLayout {
    size_t zcnt, total;
    bool sorted;  // within the sort capacity: else brute force only, and no scratch to speak of
    __host__ KnnPairLayout(int B_, int n, int S) : PairLayout(B_, n, S) {
        sorted = (n > S ? n : S) <= rrl_sort_capacity();
        zcnt = take(4 * (size_t)B);
        total = sorted ? end : 256;
    }
};

extern "C" size_t rrl_knn_workspace_bytes(int B, int n, int S) {
    if (B < 0 || n < 0 || S < 0) return 0;
    return KnnPairLayout(B, n, S).total;
}

struct KnnArgs {
    const float *ref, *qry;                // [B][n][3], [B][S][3] or NULL (the self form)
    const int32_t *cnt_ref, *cnt_qry;      // [B] or NULL
    const float4 *p0r, *p0q, *grr, *grq;   // the tree method: sorted records and tree nodes of both clouds
    const uint32_t *pmax;                  // [2][B]
    int32_t *idx, *found;
    float *dist2, *feat;
    int B, n, S, k, flags, channels, C;
};

// one lane's view of the wavefront's lists: column `lane` of d [k][64] and i [k][64], UNSORTED, and the lane's k-th key -- the
// lexicographic maximum of its column -- with its slot in registers
struct KnnList {
    double *d;
    int *i;
    int k;
    double dk;
    int ik, ms;
};
// offer key (d, j): it enters when it is lexicographically below the k-th key (a NaN or infinite d never is) -- in that key's
// slot -- and the column is scanned for its new maximum: independent reads in a loop of uniform length.  (A sorted column
// sifted from the end is a chain of dependent LDS round trips that nearly every candidate pays, because among 64 lanes
// some lane takes nearly every candidate.  Brute force at B = 8, n = 1024, k = 20: 2465 us sifted, 1757 us with this scan
// as a rolled loop -- one LDS latency per slot --, 1238 us unrolled as below.)
// KU >= k, a compile-time bound: the scan is unrolled, its KU reads are issued together and cost one LDS latency, not k (a
// slot at or beyond k reads slot k - 1 again, which changes no maximum)
template <int KU>
__device__ __forceinline__ void knn_offer(KnnList &L, double d, int j) {
    if (d < L.dk || (d == L.dk && j < L.ik)) {
        L.d[L.ms * 64] = d; L.i[L.ms * 64] = j;
        double pd[KU];
        int pi[KU];
#pragma unroll
        for (int s = 0; s < KU; ++s) {
            const int t = min(s, L.k - 1);
            pd[s] = L.d[t * 64]; pi[s] = L.i[t * 64];
        }
        double md = -1.0;
        int mi = -1, ms = 0;
#pragma unroll
        for (int s = 0; s < KU; ++s)
            if (pd[s] > md || (pd[s] == md && pi[s] > mi)) { md = pd[s]; mi = pi[s]; ms = min(s, L.k - 1); }
        L.dk = md; L.ik = mi; L.ms = ms;
    }
}

// brute force: the nr points p [nr][3] (wave-uniform: scalar loads) in ascending index, `skip` left out (-1: none)
template <int KU>
__device__ __forceinline__ void knn_brute_rows(const float *__restrict__ p, int nr, double qx, double qy, double qz, int skip,
                                               KnnList &L) {
    kptr tp = (kptr)(uintptr_t)p;
    for (int j = 0; j < nr; ++j, tp += 3) {
        const double dx = qx - (double)tp[0], dy = qy - (double)tp[1], dz = qz - (double)tp[2];
        const double d = (dx * dx + dy * dy) + dz * dz;
        if (j != skip) knn_offer<KU>(L, d, j);
    }
}

// one row of every output from the lane's list (live) or zeros: idx, found, dist2 and the chosen channels of feat.  The
// column is unsorted: slot s of the output is the smallest key above slot s - 1's (keys are distinct: their indices are), found
// by a scan of the column -- k scans of k reads, once per query.
template <int KU>
__device__ __forceinline__ void knn_write_row(const KnnArgs &a, int b, int row, const KnnList &L, bool live, float qx, float qy,
                                              float qz, const float *__restrict__ p, int nr) {
    const int k = a.k, C = a.C;
    const size_t r = (size_t)b * a.S + row;
    int fnd = 0;
    if (live)
        for (int s = 0; s < k; ++s) fnd += L.i[s * 64] != KNN_NONE ? 1 : 0;
    if (a.found != nullptr) a.found[r] = fnd;
    const bool cf = (a.flags & RRL_KNN_CHANNEL_FIRST) != 0;
    const bool gather = a.feat != nullptr && (a.channels & (RRL_KNN_NBR | RRL_KNN_DXYZ)) != 0;
    const float cx = fnd > 0 ? qx : 0.0f, cy = fnd > 0 ? qy : 0.0f, cz = fnd > 0 ? qz : 0.0f;
    double pd = -1.0;  // the key of the slot in front
    int pj = -1;
    int j0 = 0;
    float d0 = 0.0f, nx0 = 0.0f, ny0 = 0.0f, nz0 = 0.0f;  // slot 0's values: those of the slots beyond found
    for (int s = 0; s < k; ++s) {
        int j = j0;
        float d = d0, nx = nx0, ny = ny0, nz = nz0;
        if (__any(s < fnd)) {
            double bd = 2e300;
            int bj = KNN_NONE;
            double td[KU];
            int tj[KU];
#pragma unroll
            for (int t = 0; t < KU; ++t) {
                const int u = min(t, k - 1);
                td[t] = L.d[u * 64]; tj[t] = L.i[u * 64];
            }
#pragma unroll
            for (int t = 0; t < KU; ++t)
                if ((td[t] > pd || (td[t] == pd && tj[t] > pj)) && (td[t] < bd || (td[t] == bd && tj[t] < bj))) { bd = td[t]; bj = tj[t]; }
            if (s < fnd) {
                pd = bd; pj = bj;
                j = min(max(bj, 0), nr - 1);  // (memory safety only)
                d = (float)bd;
                if (gather) { nx = p[3 * j]; ny = p[3 * j + 1]; nz = p[3 * j + 2]; }
                if (s == 0) { j0 = j; d0 = d; nx0 = nx; ny0 = ny; nz0 = nz; }
            }
        }
        a.idx[r * k + s] = j;
        if (a.dist2 != nullptr) a.dist2[r * k + s] = d;
        if (a.feat != nullptr) {
            auto put = [&](int c, float v) {
                const size_t at = cf ? (((size_t)b * C + c) * a.S + row) * k + s : (r * k + s) * C + c;
                a.feat[at] = v;
            };
            int c = 0;
            if (a.channels & RRL_KNN_NBR) { put(c, nx); put(c + 1, ny); put(c + 2, nz); c += 3; }
            if (a.channels & RRL_KNN_DXYZ) { put(c, nx - cx); put(c + 1, ny - cy); put(c + 2, nz - cz); c += 3; }
            if (a.channels & RRL_KNN_CTR) { put(c, cx); put(c + 1, cy); put(c + 2, cz); }
        }
    }
}

// grid (ceil(S / 64), B), one wavefront per workgroup, dynamic LDS 64 k 12 bytes; KU: the unrolled scans' bound, k <= KU
template <bool TREE, int KU>
__global__ __launch_bounds__(64) void knn_kernel(const KnnArgs a) {
    extern __shared__ double knn_lds[];
    const int lane = threadIdx.x, sg = blockIdx.x, b = blockIdx.y;
    const bool self = a.qry == nullptr;
    const int nr = rrl_rows(a.cnt_ref, b, a.n);                     // uniform
    const int nq = self ? nr : rrl_rows(a.cnt_qry, b, a.S);         // uniform
    const float *p = a.ref + (size_t)b * a.n * 3;
    const float *qp = self ? p : a.qry + (size_t)b * a.S * 3;
    KnnList L;
    L.k = a.k;
    L.d = knn_lds + lane;
    L.i = (int *)(knn_lds + 64 * a.k) + lane;
    const int r0 = sg * SGT + lane;
    if (sg * SGT >= nq || nr == 0) {  // uniform: no queries here, or nothing to find
        if (r0 < a.S) knn_write_row<KU>(a, b, r0, L, false, 0.0f, 0.0f, 0.0f, p, nr);
        return;
    }
    for (int s = 0; s < a.k; ++s) { L.d[s * 64] = 1e300; L.i[s * 64] = KNN_NONE; }
    L.dk = 1e300; L.ik = KNN_NONE; L.ms = 0;
    int row;     // the ORIGINAL row of this lane's query
    bool valid;
    float qx, qy, qz;
    bool brute = !TREE;
    if constexpr (TREE) {  // uniform: non-finite or huge coordinates in either cloud -- the brute loop, lane = original row
        brute = !(__uint_as_float(a.pmax[b]) <= 1.0e30f) || (!self && !(__uint_as_float(a.pmax[a.B + b]) <= 1.0e30f));
    }
    if (brute) {
        row = r0;
        valid = row < nq;
        const int qi = valid ? row : 0;
        qx = qp[3 * qi]; qy = qp[3 * qi + 1]; qz = qp[3 * qi + 2];
        if (!valid) L.dk = -1.0;  // (nothing is below it: the lane holds no list)
        knn_brute_rows<KU>(p, nr, (double)qx, (double)qy, (double)qz, self && (a.flags & RRL_KNN_EXCLUDE_SELF) ? row : -1, L);
    } else {
        const int nsg = (nr + SGT - 1) / SGT, nsgf = (a.n + SGT - 1) / SGT, nsgfq = (a.S + SGT - 1) / SGT;
        const float4 *R = a.p0r + (size_t)b * nsgf * SGT;
        const float4 *T = a.grr + (size_t)b * nsgf * NODE;
        const float4 *Q = self ? R : a.p0q + (size_t)b * nsgfq * SGT;
        const float4 *TQ = self ? T : a.grq + (size_t)b * nsgfq * NODE;
        valid = r0 < nq;
        const float4 q = Q[r0];  // pad records exist up to the supergroup boundary
        row = min(max(__float_as_int(q.w), 0), nq - 1);  // (a permutation of [0, nq): the clamp is memory safety only)
        qx = q.x; qy = q.y; qz = q.z;
        if (!valid) L.dk = -1.0;
        const int skip = self && (a.flags & RRL_KNN_EXCLUDE_SELF) ? row : -1;
        const double qxd = qx, qyd = qy, qzd = qz;
        // `cnt` records from sorted position pos0 for every lane (uniform addresses: scalar loads)
        auto eval = [&](int pos0, int cnt) {
            kptr rp = (kptr)(uintptr_t)(R + pos0);
            for (int t = 0; t < cnt; ++t, rp += 4) {
                const double dx = qxd - (double)rp[0], dy = qyd - (double)rp[1], dz = qzd - (double)rp[2];
                const double d = (dx * dx + dy * dy) + dz * dz;
                const int j = __float_as_int(rp[3]);
                if (j != skip) knn_offer<KU>(L, d, j);
            }
        };
        kptr qn = (kptr)(uintptr_t)(TQ + (size_t)sg * NODE);
        const float cqx = qn[0], cqy = qn[1], cqz = qn[2], Rq = qn[3];
        int seed = sg;
        if (!self) {  // the reference supergroup whose centre is nearest the query patch's centre
            float dmin = INFINITY;
            int jmin = 0;
            for (int j = lane; j < nsg; j += 64) {
                const float4 c = T[(size_t)j * NODE];
                const float dx = cqx - c.x, dy = cqy - c.y, dz = cqz - c.z;
                const float d2 = dx * dx + dy * dy + dz * dz;
                if (d2 < dmin) { dmin = d2; jmin = j; }
            }
            const float wmin = wave_min(dmin);
            const unsigned long long who = __ballot(dmin == wmin);
            seed = who ? __builtin_amdgcn_readlane(jmin, __ffsll((long long)who) - 1) : 0;
        }
        seed = min(seed, nsg - 1);  // (the self form: nq == nr, so sg < nsg already)
        eval(seed * SGT, min(SGT, nr - seed * SGT));
        // knn_walk_others (rrl_knn_walk.h) in this kernel's own text: called from here the walk is the same instructions with the
        // scalar address arithmetic in another order and 8 more bytes, and every k >= 8 shape measured 0.2 .. 0.8 % slower than this
        // text, outside the spread of two loads of one library (profiles/nn_walk_timing.json: superseded_rows).  Another place
        // for the query node's load was not measured: the cross form's seed search above needs the centre before the seed is
        // evaluated, so the load cannot follow the seed as it does in knn3_tree_kernel.  A change to the walk or to the visiting
        // order is made in both places; the bound and its tests are shared.
        const int kmax = 2 * max(seed, nsg - 1 - seed);  // offsets 1 .. kmax reach every other supergroup
        for (int k0 = 1; k0 <= kmax; k0 += 64) {
            const int kk = k0 + lane;
            const int j = seed + ((kk & 1) ? (kk + 1) / 2 : -(kk / 2));
            const float sbmax = wave_max(valid ? knn_bound(L.dk) : 0.0f);
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
                if (!__any(valid && knn_reach(qx, qy, qz, jn[0], jn[1], jn[2], jn[3], knn_bound(L.dk)))) continue;
                for (int g = 0; g < SGG; ++g) {
                    const int pos0 = jj * SGT + g * GRP, cnt = min(GRP, nr - pos0);
                    if (cnt <= 0) break;
                    const bool need = valid && knn_reach(qx, qy, qz, jn[4 * (1 + g)], jn[4 * (1 + g) + 1], jn[4 * (1 + g) + 2],
                                                         jn[4 * (1 + g) + 3], knn_bound(L.dk));
                    if (__any(need)) eval(pos0, cnt);
                }
            }
        }
    }
    if (valid) knn_write_row<KU>(a, b, row, L, true, qx, qy, qz, p, nr);
    else if (r0 < a.S) knn_write_row<KU>(a, b, r0, L, false, 0.0f, 0.0f, 0.0f, p, nr);  // a row beyond the sample's queries, by grid position
}

extern "C" int rrl_knn(const float *ref, const int32_t *count_ref, const float *qry, const int32_t *count_qry, int k, int flags,
                       int channels, void *ws, size_t ws_bytes, int32_t *idx, int32_t *found, float *dist2, float *feat, int B,
                       int n, int S, void *stream) {
    const int all_flags = RRL_KNN_EXCLUDE_SELF | RRL_KNN_CHANNEL_FIRST | RRL_KNN_BRUTE;
    const int all_channels = RRL_KNN_NBR | RRL_KNN_DXYZ | RRL_KNN_CTR;
    if (!ref || !idx || !ws || B < 0 || B > 32767 || n < 1 || S < 0 || k < 1 || k > RRL_KNN_MAX_K) return RRL_E_ARG;
    if (!qry && S != n) return RRL_E_ARG;
    if ((flags & ~all_flags) || (channels & ~all_channels) || (channels != 0) != (feat != nullptr)) return RRL_E_ARG;
    KnnPairLayout L(B, n, S);
    if (ws_bytes < L.total) return RRL_E_WS;
    if (B == 0 || S == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    char *w = (char *)ws;
    const bool self = qry == nullptr;
    const bool tree = !(flags & RRL_KNN_BRUTE) && L.sorted;  // beyond the sort capacity: brute force
    KnnArgs a = {};
    a.ref = ref; a.qry = qry;
    a.cnt_ref = count_ref; a.cnt_qry = self ? nullptr : count_qry;
    a.idx = idx; a.found = found; a.dist2 = dist2; a.feat = feat;
    a.B = B; a.n = n; a.S = S; a.k = k; a.flags = flags; a.channels = channels;
    a.C = ((channels & RRL_KNN_NBR) ? 3 : 0) + ((channels & RRL_KNN_DXYZ) ? 3 : 0) + ((channels & RRL_KNN_CTR) ? 3 : 0);
    const dim3 grid((unsigned)((S + SGT - 1) / SGT), (unsigned)B);
    const size_t lds = (size_t)64 * k * (sizeof(double) + sizeof(int));
#define RRL_KNN_LAUNCH(TREE)                                                                        \
    do {                                                                                            \
        if (k <= 4) hipLaunchKernelGGL((knn_kernel<TREE, 4>), grid, dim3(64), lds, s, a);           \
        else if (k <= 8) hipLaunchKernelGGL((knn_kernel<TREE, 8>), grid, dim3(64), lds, s, a);      \
        else if (k <= 16) hipLaunchKernelGGL((knn_kernel<TREE, 16>), grid, dim3(64), lds, s, a);    \
        else if (k <= 24) hipLaunchKernelGGL((knn_kernel<TREE, 24>), grid, dim3(64), lds, s, a);    \
        else hipLaunchKernelGGL((knn_kernel<TREE, 32>), grid, dim3(64), lds, s, a);                 \
    } while (0)
    if (!tree) {
        RRL_KNN_LAUNCH(false);
        RRL_LAUNCH_CHECK();
        return 0;
    }
    if (self) L.drop_second();  // the self form's second cloud is absent: counts of 0 (ZCNT, cleared below)
    int rc;  // up to 4096 points the sort kernel reads the points itself: no records launch
    if (!L.big) rc = rrl_fill(w + L.pmax, 0u, L.total - L.pmax, s);
    else rc = rrl_launch_pts_records(ref, (float4 *)(w + L.crec[0]), (float *)(w + L.apart), w + L.pmax, (L.total - L.pmax) / 16, B, n,
                                     L.nblk, count_ref, s);
    if (rc) return rc;
    if (L.big && !self)  // the query cloud's records and its rows of the partial boxes (cloud 1's: behind cloud 0's B nblk rows)
        rc = rrl_launch_pts_records(qry, (float4 *)(w + L.crec[1]), (float *)(w + L.apart) + (size_t)B * L.nblk * 8, w + L.pmax, 0, B, S,
                                    L.nblk, count_qry, s);
    if (rc) return rc;
    rc = rrl_launch_cloud_sort(L, ws, L.big ? nullptr : ref, L.big ? nullptr : qry, nullptr, 0, count_ref,
                               self ? (const int32_t *)(w + L.zcnt) : count_qry, s);
    if (rc) return rc;
    a.p0r = (const float4 *)(w + L.p0s[0]); a.p0q = (const float4 *)(w + L.p0s[1]);
    a.grr = (const float4 *)(w + L.grp[0]); a.grq = (const float4 *)(w + L.grp[1]);
    a.pmax = (const uint32_t *)(w + L.pmax);
    RRL_KNN_LAUNCH(true);
#undef RRL_KNN_LAUNCH
    RRL_LAUNCH_CHECK();
    return 0;
}
