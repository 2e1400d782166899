// rrl_ws.h -- the host layer's shared types: the layouts of the caller-allocated workspaces (WsLayout, WwLayout: generated from
// the field tables of include/rrl.h), the record of ONE call (RrlCall: options, plan, shape, bucket range, workspace + layout, stream -- set once at
// the top of an extern "C" entry by rrl_begin_call, validated once by rrl_check_call (both rrl_call.hip), then handed to every host function
// below the entry), and the prototypes of the host functions that cross translation units.
// Every field starts on a 256-byte boundary, the fields follow each other in table order.
#pragma once
#include <stdlib.h>

#include "rrl_common.h"

// ---- layouts, generated from include/rrl.h's tables (kind 0: RRL_WS_TABLE, 1: RRL_WW_TABLE) ----
template <class T, class... D>
constexpr size_t rrl_field_bytes(D... d) { return ((sizeof(T) * ... * (size_t)d) + 255) & ~(size_t)255; }
#define RRL_ROW_END_(name, type, ...) *end++ = o += rrl_field_bytes<type>(__VA_ARGS__);
// end[0] = 0, end[i + 1] = where field i ends and field i + 1 starts (g = b: room for every grouping)
template <int KIND>
inline void rrl_place_fields(size_t *end, int B, int N, int M, int L) {
    const size_t b = (size_t)(B > 0 ? B : 0), n = (size_t)(N > 0 ? N : 0), m = (size_t)(M > 0 ? M : 0),
                 l = (size_t)(L > 0 ? L : 0), g = b;
    size_t o = *end++ = 0;
    if constexpr (KIND == 0) { RRL_WS_TABLE(RRL_ROW_END_) } else { (void)n; (void)m; RRL_WW_TABLE(RRL_ROW_END_) }
}
template <int KIND, int F> struct RrlFieldType;  // ::T, the field's element type
#define RRL_WS_TYPE_(name, type, ...) template <> struct RrlFieldType<0, RRL_WS_##name> { typedef type T; };
#define RRL_WW_TYPE_(name, type, ...) template <> struct RrlFieldType<1, RRL_WW_##name> { typedef type T; };
RRL_WS_TABLE(RRL_WS_TYPE_)
RRL_WW_TABLE(RRL_WW_TYPE_)

template <int KIND, int FIELDS>
struct RrlLayout {
    size_t off[FIELDS + 1];  // off[FIELDS] = total
    size_t total;
    RrlLayout() : off{}, total(0) {}  // (a record before rrl_begin_call)
    RrlLayout(int B, int N, int M, int L) { rrl_place_fields<KIND>(off, B, N, M, L); total = off[FIELDS]; }
    // field F of a workspace, as a pointer to the table's element type
    template <int F> typename RrlFieldType<KIND, F>::T *at(void *ws) const {
        return (typename RrlFieldType<KIND, F>::T *)((char *)ws + off[F]);
    }
    template <int F> const typename RrlFieldType<KIND, F>::T *at(const void *ws) const {
        return (const typename RrlFieldType<KIND, F>::T *)((const char *)ws + off[F]);
    }
};

// What the host code knows about the order of the narrow fields beyond their sizes:
static_assert(RRL_WS_STATUS == 0 && RRL_WS_NVALS == 1 && RRL_WS_NSEL == 2 && RRL_WS_PMAX == 3 && RRL_WS_COUNT1 == 4 &&
                  RRL_WS_COUNT2 == 5, "zero_bytes: one fill clears the per-call state, the first six fields");
static_assert(RRL_WS_MCTL == RRL_WS_MHIST + 1 && RRL_WS_MSUM == RRL_WS_MHIST + 2, "state_off / state_bytes span MHIST .. MSUM");
static_assert(RRL_WS_KJC == RRL_WS_GACC + 1, "GACC is cleared up to KJC's offset (rrl_launch_tri_build)");
// ... and about the control words inside MCTL and CHAIN rows (include/rrl.h RRL_MCTL_*, RRL_CHAIN_*), what used to be a
// convention between five files: the rows are the tables' last extents, no two users share a word
template <class... D>
constexpr size_t rrl_last_extent(D... d) { size_t v = 0; ((v = (size_t)d), ...); return v; }
#define RRL_ROW_LAST_(name, type, ...) rrl_last_extent(__VA_ARGS__),
constexpr size_t rrl_ws_last_extent(int field) {
    const size_t b = 1, n = 1, m = 1, l = 1, g = 1;
    const size_t last[] = {RRL_WS_TABLE(RRL_ROW_LAST_)};
    return last[field];
}
constexpr bool rrl_mctl_words_distinct() {
    const int w[] = {RRL_MCTL_CURSOR, RRL_MCTL_TICK1, RRL_MCTL_TICK2, RRL_MCTL_ERR, RRL_MCTL_MEDBITS, RRL_MCTL_MEDRDY, RRL_MCTL_BAD,
                     RRL_MCTL_CHAM_GROUP, RRL_MCTL_CHAM_GROUP + 1, RRL_MCTL_CHAM_TOP, RRL_MCTL_LSUM, RRL_MCTL_LSUM + 1};
    const int nw = (int)(sizeof w / sizeof *w);
    for (int i = 0; i < nw; ++i) {
        if (w[i] < RRL_MCTL_BUCKET0 + 16 || w[i] >= RRL_MCTL_WORDS) return false;  // (the sixteen buckets come first)
        for (int j = 0; j < i; ++j)
            if (w[j] == w[i]) return false;
    }
    return true;
}
static_assert(rrl_ws_last_extent(RRL_WS_MCTL) == RRL_MCTL_WORDS && rrl_ws_last_extent(RRL_WS_CHAIN) == RRL_CHAIN_WORDS,
              "the rows of MCTL and CHAIN as include/rrl.h's table sizes them");
static_assert(rrl_mctl_words_distinct(), "MCTL: behind the buckets, inside the row, no word with two users");
static_assert(RRL_MCTL_LSUM % 2 == 0 && RRL_MCTL_LSUM + 2 <= RRL_MCTL_WORDS, "MCTL: the loss sum is one aligned uint64 inside row 0");
static_assert(RRL_CHAIN_READY == 0 && RRL_CHAIN_NAN == 1 && RRL_CHAIN_FALLBACK == 2 && RRL_CHAIN_TIMEOUT == 3 && RRL_CHAIN_WORDS == 4,
              "CHAIN: one 16-byte row per sample; the fused launch's scan takes [NAN], [FALLBACK] as its STATUS[0], [1]");
struct WsLayout : RrlLayout<0, RRL_WS_FIELDS> {
    size_t zero_bytes;
    size_t state_off, state_bytes;  // MHIST .. MSUM: per-call state of the tiled reduce (cleared by the records kernel)
    WsLayout() : zero_bytes(0), state_off(0), state_bytes(0) {}
    WsLayout(int B, int N, int M, int L)
        : RrlLayout(B, N, M, L), zero_bytes(off[RRL_WS_COUNT2 + 1]), state_off(off[RRL_WS_MHIST]),
          state_bytes(off[RRL_WS_MSUM + 1] - off[RRL_WS_MHIST]) {}
};
static_assert(RRL_WW_STATUS == 0 && RRL_WW_NSEL == 1, "zero_bytes: one fill clears STATUS and NSEL");
struct WwLayout : RrlLayout<1, RRL_WW_FIELDS> {
    size_t zero_bytes;
    WwLayout(int B, int N, int M, int L) : RrlLayout(B, N, M, L), zero_bytes(off[RRL_WW_NSEL + 1]) {}
};

// The options of ONE call, resolved once at its top (include/rrl.h rrl_opts; defaults = what the rrl_set_* setters /
// RRL_* environment variables selected) and handed through its stages by value: no stage reads a process-wide knob.
typedef rrl_chamfer_rider RrlChamRider;  // include/rrl.h: the evaluation's Chamfer walk, carried by the culled scan's launch

// (internal, rrl_demo_epoch) The COUNT pass of the NEXT epoch's line sampler, carried by this evaluation's per-line launch
// (pair_count_kernel): it needs the moved source's box -- the records launch's partial rows -- and the sampler's static
// geometry, not the scan; the per-line stage and the count pass both run 1024-lane workgroups.
struct RrlCountRider {
    const unsigned long long *rng_state;
    const float *r, *centers, *aabb2;
    const float *rows;  // APART rows of cloud 1 (the moved source's partial boxes)
    int n_rows;
    unsigned long long *accept;  // the sampler's ballots (tile_counts)
    int n, rounds;
    int done;
};

// (internal, rrl_demo_epoch) ... and the WRITE pass of the next epoch's sampler, carried by this evaluation's direct-backward
// launch (bwd_write_kernel; 256-lane workgroups): it needs the count pass's ballots (which rode in the per-line launch) and
// overwrites the line buffer, which nothing after the per-line stage reads.
struct RrlWriteRider {
    unsigned long long *rng_state;
    const float *r, *centers;
    const unsigned long long *accept;
    float *lines;
    int32_t *filled;
    int n, rounds;
    int done;
};

struct RrlXform;
// What an entry runs besides the forward (STAGE: one stage entry on its own, no whole forward; SCATTER2: grad_tri2 too);
// the reduce that serves a call (TILE: one tile of lines per sample, per-line stage + reduce + a backward in one launch).
enum { RRL_WANT_NONE = -1, RRL_WANT_STAGE, RRL_WANT_FORWARD, RRL_WANT_SCATTER, RRL_WANT_SCATTER2, RRL_WANT_DIRECT };
enum { RRL_RED_SINGLE, RRL_RED_XCHG, RRL_RED_TAIL, RRL_RED_TILE };
// Which kernels serve ONE call of the narrow pipeline, decided by rrl_plan (rrl_call.hip) before its first launch; the
// launchers read it and derive none of it again.  All zero (rrl_begin_call): nothing rides, nothing chains.
struct RrlPlan {
    int scan_mode;          // cull demoted to auto beyond the sort capacity
    int clouds, build_clouds;  // clouds scanned (1: the target's scan carried over) / built (1: a kept target)
    int lmax_ready;         // the records launch reduced the lines' maxima (no launch of the culled scan's own)
    int reduce, tail_rpl2;  // RRL_RED_*; the tail kernel's <S, 2> instantiation rather than <S, TAIL_RPL>
    int bwd_rides;          // the wanted backward rides in the reduce's launch (single-tile or tail kernel)
    int payload_in_reduce;  // rrl_loss_step_ex: the exchange reduce's last arrivers add payload[0 .. 1]
    int leave_clean;        // include/rrl.h RRL_F_CHAIN: the per-line stage zeroes COUNT1 / COUNT2, the reduce the CHAIN words
    int fused_build;        // RRL_F_CHAINED honoured (only with leave_clean): records + both scans as ONE launch
    int count_rides, write_rides;  // the RrlCountRider rides in the per-line launch, the RrlWriteRider in the backward's
};
// The tail kernel's geometry as far as the plan needs it (rrl_stage_tail.h has the rest): line tiles per sample it serves,
// lanes per workgroup
constexpr int TAIL_MAX_TILES = 32;
constexpr int TAIL_LANES = 512;
struct RrlCall {
    int flags;
    int reduce_mode;    // 0 auto, 1 single, 2 tiled, 3 xchg
    int deterministic;  // 0 / 1
    int sort_parts;     // 0 automatic, k forced
    int scan_variant;   // 0 default, else lines per lane
    const int32_t *order1, *order2;
    unsigned long long *counters;
    long long counter_rows;
    // (internal, not part of rrl_opts) a caller-owned buffer the build step's first launch clears along with the per-call
    // state: the scatter target of rrl_loss_step (grad_tri1), so that no fill launch precedes the step
    void *clear_ptr;
    size_t clear_bytes;  // multiple of 4
    RrlChamRider *rider;  // rrl_opts.chamfer
    RrlCountRider *count_rider;  // (internal) see RrlCountRider
    RrlWriteRider *write_rider;  // (internal) see RrlWriteRider
    int problems;         // rrl_opts.problems (multi-pose evaluation): 0, or Bt < B with B % Bt == 0
    float *payload;       // rrl_opts.payload (rrl_loss_step_ex): [sum of valid losses, #valid, 0 x 12], or NULL
    const void *tar_ws;   // (internal) the workspace that holds cloud 2's records when the target's scan is carried over
                          // (rrl_*_forward_cached: `target_ws`): the riding walk takes the target from there
    int32_t *chain_left;  // rrl_opts.chain_left (host int, or NULL)
    const int32_t *count1, *count2, *nlines;  // rrl_opts: per-sample rows of a RAGGED batch (device int32 [B]), or NULL
    const RrlXform *xf;   // (internal) the source's transform, for the fused build's records body (plan.fused_build) ...
    const float *tri1_in; //   ... and the caller's source rows when there is no transform
    RrlPlan plan;
    // The call itself (rrl_begin_call): shape, bucket range, pool / scan mode / chunk as the entry received them, the
    // workspace with its layout -- built ONCE per call -- and the stream.  No host function below an entry takes any of
    // these as a parameter of its own.
    int B, N, M, L;
    int s_m, s_n, e_m, e_n;
    int pool, mode, chunk;
    void *ws;
    size_t ws_bytes;
    WsLayout w;
    hipStream_t s;
    template <int F> auto at() const { return w.at<F>(ws); }  // field F (RRL_WS_*) of this call's workspace
    // ... and a field of cloud 2 where its scan left it: the carried-over target's workspace (tar_ws), else this one
    template <int F> auto tar_at() const { return w.at<F>(tar_ws ? tar_ws : (const void *)ws); }
    __host__ void set(int sm, int sn, int em, int en, int pool_, int mode_ = RRL_SCAN_CULL, int chunk_ = 0) {
        s_m = sm; s_n = sn; e_m = em; e_n = en; pool = pool_; mode = mode_; chunk = chunk_;
    }
    __host__ bool prepared() const { return order1 != nullptr; }
    __host__ bool target_kept() const { return order1 != nullptr && (flags & RRL_F_TARGET_KEPT); }
    __host__ bool ragged() const { return count1 != nullptr || count2 != nullptr || nlines != nullptr; }
};
// The record of one call (rrl_call.hip): rrl_opts resolved + the shape, the workspace with its layout, the stream; bucket
// range 1 .. 4, pool 0, scan mode cull, chunk 0 until the entry sets what it was given (RrlCall::set)
RrlCall rrl_begin_call(const rrl_opts *opts, int B, int N, int M, int L, void *ws, size_t ws_bytes, void *stream);
// THE validation of a narrow entry, before its first launch, in the order of include/rrl.h ("Refusals"): RRL_E_ARG --
// !pointers (the entry's own null pointers and illegal combinations), the shape, the mode, the plan's refusals
// (rrl_plan(o, want, target_ws, xf); RRL_WANT_NONE: an entry without a forward, no plan) --, RRL_E_RANGE, RRL_E_WS
int rrl_check_call(RrlCall &o, bool pointers, int want, const void *target_ws = nullptr, const RrlXform *xf = nullptr);
// the plan of one call (o.plan; also settles o.problems, the orders, o.tar_ws, o.xf); RRL_E_ARG: an illegal multi-pose call,
// or a ragged one (counts) combined with what does not serve it (include/rrl.h rrl_opts.count1)
int rrl_plan(RrlCall &o, int want, const void *target_ws, const RrlXform *xf);
// include/rrl.h rrl_sort_capacity (rrl_cull.hip): the sorted layout (records kernel, sphere tree, culled scan) serves up to it
inline bool rrl_sorted_layout(int N, int M) { return (N > M ? N : M) <= rrl_sort_capacity(); }
// the sampler's two passes on their own (rrl_geom.hip; rrl_sample_lines_rng = both): rrl_demo_epoch pipelines them
int rrl_sample_count_pass(const uint64_t *rng_state, const float *r, const float *centers, const float *aabb1, const float *aabb2,
                          int32_t *tile_counts, int B, int n, int rounds, void *stream);
int rrl_sample_write_pass(uint64_t *rng_state, const float *r, const float *centers, float *lines, int32_t *filled,
                          int32_t *tile_counts, int B, int n, int rounds, void *stream);
int rrl_sample_prefilter(void);
// rrl_registration_forward_ex on a record that went through rrl_check_call(o, .., RRL_WANT_FORWARD, target_ws, &xf)
// (rrl_sparse.hip; rrl_epoch.hip checks the whole epoch before its first launch)
int rrl_registration_forward_call(RrlCall &o, const float *tri2, const float *line, float *loss);
// rrl_registration_step_ex on a record that went through rrl_check_call(o, .., RRL_WANT_DIRECT, target_ws, &xf)
// (rrl_sparse.hip; rrl_epoch.hip adds its riders before the check)
int rrl_registration_step_call(RrlCall &o, const RrlXform &xf, const float *tri2, const float *line, float *loss,
                               const float *grad_loss, float *gR, float *gt, float *payload);
// The build and the scan of a planned call (rrl_scan.hip; the plan says which clouds and which scan): o.xf != NULL moves the
// source into TRI1; line != NULL: the records launch also reduces the lines' maxima
int rrl_tri_prepare_clouds(const RrlCall &o, const float *tri1, const float *tri2, const float *line);
int rrl_line_tri_scan_clouds(const RrlCall &o, const float *line);
// their launchers on the sorted layout (rrl_cull.hip)
int rrl_launch_tri_build(const RrlCall &o, const float *tri1, const float *tri2, const float *line);
int rrl_launch_cull_scan(const RrlCall &o, const float *line);
int rrl_launch_pmax_from_partials(const RrlCall &o, int clouds);
int rrl_cull_scan_can_fuse(const RrlCall &o);
// (the pair build outside the loss workspace, rrl_launch_cloud_sort: rrl_tree.h, next to its scratch layout)
// the Chamfer path's records launch for one cloud (rrl_chamfer.hip), for the 3-NN tree's build (rrl_knn_tree.hip)
int rrl_launch_pts_records(const float *pts, float4 *crec, float *apart, void *zero, size_t zero_vec4, int B, int n, int nblk,
                           const int32_t *cnt, hipStream_t s);
// the rigid backward behind the scatter (rrl_geom.hip)
int rrl_fused_backward(int B, int N, int M);
int rrl_launch_reg_bwd(const RrlCall &o, const float *src, const float *R, float *grad_src, float *gR, float *gt,
                       float *payload, const float *loss, int transpose_r);  // (G1 -> grad_src, gR, gt; RPART, INFO, STATUS[3])
// Sample b's workgroups on XCD b % 8 (rrl_stage_pair.h xcd_sample_of; the records launch places (cloud, sample) pairs the
// same way).  RRL_XCD_ALIGN=0 turns it off (experimental builds): the one reader of that knob, for every launcher
inline int xcd_align_on() {
    static int v = -1;
    if (v < 0) {
        v = 1;
#ifdef RRL_EXPERIMENT
        if (const char *e = getenv("RRL_XCD_ALIGN")) v = e[0] == '0' ? 0 : 1;
#endif
    }
    return v;
}
// the process-wide defaults, one accessor per translation unit that owns one
bool rrl_default_deterministic(void);                                       // rrl_call.hip (rrl_set_deterministic)
unsigned rrl_default_spin_limit(void);                                      // rrl_call.hip (rrl_set_spin_limit)
int rrl_default_sort_parts(void);                                           // rrl_cull.hip
void rrl_default_scan_counters(unsigned long long **buf, long long *rows);  // rrl_cull.hip
int rrl_default_scan_variant(void);                                         // rrl_scan.hip

// Workgroups of the exchange reduce that are co-resident on the current device: the plan's bound for choosing it
// (rrl_sparse.hip, next to the kernel whose occupancy it queries)
long rrl_xchg_capacity(void);

// Rigid transform of the source cloud folded into the prepare step (the fused training op):
// tri1 = src moved by (R, t) per sample, stored into the workspace field TRI1.
struct RrlXform {
    const float *src, *R, *t;
    int transpose_r;
    int zero_g1;  // also clear GACC, the (dR, dt, payload) accumulator of the direct backward
};
