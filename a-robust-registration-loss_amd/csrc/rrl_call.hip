// rrl_call.hip -- the record and the plan of every call of the narrow pipeline, host code only: rrl_begin_call (rrl_opts and
// the process-wide defaults -> RrlCall), rrl_plan ("which kernels serve this shape": reduce_kind and what rides or chains),
// rrl_check_call (THE validation, in the order of include/rrl.h "Refusals"), the three process-wide knobs those read with
// their setters, and the description of both workspace tables (rrl_workspace_bytes / _layout / _field).  Both scans'
// translation units and rrl_sparse.hip's entries call into it; what the plan needs to know about the stage kernels crosses
// through rrl_ws.h (rrl_xchg_capacity, TAIL_MAX_TILES, TAIL_LANES).  No kernel is defined or launched here.
#define RRL_NO_LAUNCH_UNIT  // (rrl_common.h: not even the fill / copy kernels)
#include <ctype.h>
#include <stdlib.h>
#include <string.h>

#include "rrl_ws.h"

// ---------------------------------------------------------------------------------------
// the process-wide defaults of this unit (a call's rrl_opts overrides them; rrl_begin_call reads them once per call)
// ---------------------------------------------------------------------------------------
// The DEFAULT reduce mode (include/rrl.h rrl_set_reduce_mode; a call's rrl_opts.reduce_mode overrides it): 0 auto, 1 single,
// 2 tiled (the tail kernel wherever legal), 3 xchg (the exchange kernel wherever legal); reduce_kind() below turns a mode
// and a shape into the kernel.  Env RRL_REDUCE=single|tiled|xchg.
static int g_reduce_mode = -1;  // -1: read RRL_REDUCE once
extern "C" int rrl_set_reduce_mode(int mode) {
    if (mode < 0 || mode > 3) return RRL_E_ARG;
    g_reduce_mode = mode;
    return 0;
}
static int default_reduce_mode() {
    if (g_reduce_mode < 0) {
        const char *e = getenv("RRL_REDUCE");
        g_reduce_mode = !e ? 0 : (e[0] == 's' ? 1 : (e[0] == 't' ? 2 : (e[0] == 'x' ? 3 : 0)));
    }
    return g_reduce_mode;
}
// include/rrl.h rrl_set_deterministic.  Env RRL_DETERMINISTIC=1.
static int g_deterministic = -1;  // -1: read RRL_DETERMINISTIC once
extern "C" int rrl_set_deterministic(int on) {
    g_deterministic = on ? 1 : 0;
    return 0;
}
bool rrl_default_deterministic() {
    if (g_deterministic < 0) {
        const char *e = getenv("RRL_DETERMINISTIC");
        g_deterministic = (e && e[0] == '1') ? 1 : 0;
    }
    return g_deterministic == 1;
}
// Test hook: polls a waiting workgroup of the exchange reduce makes before it gives up (default 2^18, ~0.3 s); 0 makes
// every hand-off "time out", so the repair path runs on every sample (tests/test_gpu_stress.py).  Env RRL_SPIN_LIMIT.
static long g_spin_limit = -1;
extern "C" int rrl_set_spin_limit(long long polls) {
    if (polls < 0 || polls > 0xffffffffll) return RRL_E_ARG;
    g_spin_limit = (long)polls;
    return 0;
}
unsigned rrl_default_spin_limit() {
    if (g_spin_limit < 0) {
        const char *e = getenv("RRL_SPIN_LIMIT");
        g_spin_limit = e ? atol(e) : (1l << 18);
        if (g_spin_limit < 0) g_spin_limit = 1l << 18;
    }
    return (unsigned)g_spin_limit;
}

// The record of one call (csrc/rrl_ws.h RrlCall): include/rrl.h rrl_opts -> its options -- fields the caller's struct does
// not reach (struct_bytes), -1 and NULL mean the process-wide default; the internal fields start zero: an empty plan --,
// then the shape, the workspace with its layout and the stream.
RrlCall rrl_begin_call(const rrl_opts *p, int B, int N, int M, int L, void *ws, size_t ws_bytes, void *stream) {
    RrlCall o{};
    rrl_opts v;
    memset(&v, 0, sizeof v);
    v.reduce_mode = v.deterministic = v.sort_parts = v.scan_variant = -1;
    if (p && p->struct_bytes >= 8) memcpy(&v, p, (size_t)p->struct_bytes < sizeof v ? (size_t)p->struct_bytes : sizeof v);
    o.flags = v.flags;
    o.reduce_mode = v.reduce_mode >= 0 && v.reduce_mode <= 3 ? v.reduce_mode : default_reduce_mode();
    o.deterministic = v.deterministic >= 0 ? (v.deterministic ? 1 : 0) : (rrl_default_deterministic() ? 1 : 0);
    o.sort_parts = v.sort_parts >= 0 && v.sort_parts <= 16 ? v.sort_parts : rrl_default_sort_parts();
    const int sv = v.scan_variant;
    o.scan_variant = (sv == 0 || sv == 1 || sv == 2 || sv == 4 || sv == 8) ? sv : rrl_default_scan_variant();
    o.order1 = v.order1;
    o.order2 = v.order2;
    if (v.scan_counters) { o.counters = (unsigned long long *)v.scan_counters; o.counter_rows = v.scan_counter_rows; }
    else rrl_default_scan_counters(&o.counters, &o.counter_rows);
    o.rider = v.chamfer;  // (done is the caller's to clear; the scan's launcher sets it when the walk rides along)
    o.payload = v.payload;
    o.problems = v.problems > 0 ? v.problems : 0;
    o.chain_left = v.chain_left;
    o.count1 = v.count1; o.count2 = v.count2; o.nlines = v.nlines;
    o.B = B; o.N = N; o.M = M; o.L = L;
    o.set(1, 1, RRL_MAX_HITS + 1, RRL_MAX_HITS + 1, 0);
    o.ws = ws; o.ws_bytes = ws_bytes;
    o.w = WsLayout(B, N, M, L);
    o.s = (hipStream_t)stream;
    return o;
}

// (sample, tile) pairs up to which the tail kernel serves a call (experiments: RRL_TAIL_MAX_WG)
static long tail_max_wg() {
    static long v = -1;
    if (v < 0) {
        const char *e = nullptr;
#ifdef RRL_EXPERIMENT
        e = getenv("RRL_TAIL_MAX_WG");
#endif
        v = e ? atol(e) : 256;  // measured at 10 tiles per sample (round 5): B = 16 78.5 -> 77.7, B = 24 98.0 -> 96.7 us per step with the
        if (v < 1) v = 256;     // tail kernel, B = 32 121 -> 128, B = 64 200 -> 213 (the exchange reduce + a backward launch win there)
    }
    return v;
}
// Which reduce kernel (rrl_ws.h RRL_RED_*): one workgroup per sample, tiled with the candidate exchange
// (loss_reduce_tiled_kernel), or the tail kernel (no exchange: every workgroup streams its sample's dense value lists; one
// 512-lane workgroup or two per compute unit, so it serves the small, latency-bound grids: B x tiles <= 256, <= 32 tiles
// per sample).  mode 0 (auto): the tail kernel where the backward rides along (with_bwd: rrl_registration_step -- measured
// -1.9 .. -3.4 us per step at C2 / L = 4096 / C4, round 5b: -6 us at the demo's 20 tiles; as a reduce alone it is within
// +-1 % of the exchange kernel), else the exchange kernel for >= 2 tiles while the grid
// is co-resident, else the single workgroup; 1: single; 2 ("tiled"): the tail kernel wherever it is legal (also forward
// only, also one tile: tests), exchange beyond; 3 ("xchg"): the exchange kernel wherever it is legal.
static int reduce_kind(int mode, int B, int nblk, int pool, bool with_bwd) {
    if (pool || mode == 1) return RRL_RED_SINGLE;
    const bool xchg_ok = (long)B * nblk <= rrl_xchg_capacity();
    if (mode == 3) return xchg_ok && nblk >= 1 ? RRL_RED_XCHG : RRL_RED_SINGLE;
    const bool tail_ok = nblk <= TAIL_MAX_TILES && (long)B * nblk <= tail_max_wg();
    if (mode == 2 && tail_ok && nblk >= 1) return RRL_RED_TAIL;
    // (round 5: up to TAIL_MAX_TILES line tiles, not 16 -- the demo's 20: tail 11.1 us against tiled reduce 10.6 + backward 5.8 / 7.2)
    if (mode == 0 && tail_ok && with_bwd && nblk >= 2) return RRL_RED_TAIL;
    return xchg_ok && nblk >= 2 ? RRL_RED_XCHG : RRL_RED_SINGLE;
}
// The plan of one call (rrl_ws.h RrlPlan).  target_ws != NULL: the target's scan is carried over from it (one cloud scanned);
// xf != NULL: the call moves the source; want: RRL_WANT_*.  A stage entry (RRL_WANT_STAGE) takes the options as given --
// no whole forward, so no single-tile kernel, chain, rider or multi-pose check -- and builds both clouds.
int rrl_plan(RrlCall &o, int want, const void *target_ws, const RrlXform *xf) {
    const int B = o.B, N = o.N, M = o.M, L = o.L, pool = o.pool, mode = o.mode;
    RrlPlan &p = o.plan;
    p = RrlPlan{};
    const bool stage = want == RRL_WANT_STAGE, sorted = rrl_sorted_layout(N, M);
    const int nblk = (L + 1023) / 1024;
    p.scan_mode = mode == RRL_SCAN_CULL && !sorted ? RRL_SCAN_AUTO : mode;
    p.clouds = target_ws ? 1 : 2;
    const bool cull = p.scan_mode == RRL_SCAN_CULL;
    o.tar_ws = target_ws;
    o.xf = xf;
    if (stage) o.flags = 0;
    else if (o.problems >= B) o.problems = 0;
    // multi-pose evaluation (rrl_opts.problems = Bt): the B instances are B / Bt poses of Bt problems; the inputs have Bt
    // entries.  Served by the sorted layout of scan mode cull through the fused entries that move the source (xf)
    if (!stage && o.problems > 0 && (B % o.problems != 0 || !xf || pool || target_ws || !cull || N <= 0 || M <= 0)) return RRL_E_ARG;
    // ragged batches (rrl_opts.count1 / count2 / nlines): independent samples on the sorted layout's builds (every scan mode),
    // each scanning its own target; no rider reads a count
    if (o.ragged() && (pool || o.problems > 0 || o.rider || target_ws || !sorted || o.count_rider || o.write_rider)) return RRL_E_ARG;
    // prepared clouds (include/rrl.h rrl_opts): honoured by the sorted layout of scan mode cull, with the orders of every
    // cloud this call builds; anything else takes the plain path (same results)
    if (o.prepared() && (!cull || (p.clouds == 2 && !o.order2 && !(o.flags & RRL_F_TARGET_KEPT)))) o.order1 = o.order2 = nullptr;
    // a kept target: cloud 2's records / tree / partials stay as the previous call on this workspace left them
    p.build_clouds = o.target_kept() ? 1 : p.clouds;
    // (the records kernel of a forward reduces the lines' maxima whenever it runs: the sorted path)
    p.lmax_ready = !stage && sorted && B > 0 && (p.clouds == 2 && M > N ? M : N) > 0 && L > 0;
    // The reduce, and whether the wanted backward rides in its launch: not deterministic (the fixed-point scatter), not with
    // grad_tri2; the scatter backward rides in the single-tile kernel and, beyond one tile of lines, in the tail kernel
    const bool tile = !stage && L >= 1 && L <= 1024 && !pool && B > 0 && o.reduce_mode < 2;
    const bool ride = (want == RRL_WANT_DIRECT || (want == RRL_WANT_SCATTER && (tile || nblk >= 2))) && B > 0 && L > 0 &&
                      !o.deterministic;
    p.reduce = tile ? RRL_RED_TILE : reduce_kind(o.reduce_mode, B, nblk, pool, ride);
    p.tail_rpl2 = p.reduce == RRL_RED_TAIL && TAIL_LANES / nblk >= 48;  // (see tail_body: groups per lane and round)
    p.bwd_rides = ride && (p.reduce == RRL_RED_TILE || p.reduce == RRL_RED_TAIL);
    // no riding backward, but the exchange reduce serves a step: its last arrivers add the payload (no payload launch)
    p.payload_in_reduce = (want == RRL_WANT_SCATTER || want == RRL_WANT_SCATTER2) && o.payload && !p.bwd_rides && B > 0 &&
                          L > 1024 && p.reduce == RRL_RED_XCHG;
    // Chained steps (include/rrl.h RRL_F_CHAIN / RRL_F_CHAINED).  The chain lives where the per-line stage + the tail kernel or
    // the exchange reduce serve the call: they are the ones that leave COUNT1 / COUNT2 and the CHAIN words cleared ...
    const bool chain_path = B > 0 && L > 1024 && !pool && p.clouds == 2 && !o.problems && cull && N > 0 && M > 0 &&
                            (p.reduce == RRL_RED_XCHG || p.reduce == RRL_RED_TAIL);
    p.leave_clean = (o.flags & RRL_F_CHAIN) && chain_path;
    // ... and a step that FINDS them cleared runs source records + target scan + source scan as ONE launch.  Only a step that
    // also leaves them cleared: the reduce of a fused build writes the CHAIN words it clears (else the plain build serves)
    p.fused_build = p.leave_clean && (o.flags & RRL_F_CHAINED) && o.target_kept() && !o.count_rider && !o.write_rider &&
                    rrl_cull_scan_can_fuse(o);
    // the next epoch's sampler passes (rrl_demo_epoch): the count pass in the per-line launch, the write pass -- with the
    // ballots of THAT count pass -- in the launch that carries the direct backward (nothing after it reads the lines)
    if (const RrlCountRider *cr = o.count_rider)
        p.count_rides = p.reduce != RRL_RED_TILE && B == 1 && L > 0 && cr->rounds > 0 && cr->n > 0 &&
                        (long)((cr->n + 1023) / 1024) * cr->rounds < 512 && cr->rows && cr->n_rows > 0;
    if (const RrlWriteRider *wr = o.write_rider) {
        const long wtiles = (wr->n + 1023) / 1024;
        const bool in_tail = p.bwd_rides && p.reduce == RRL_RED_TAIL, in_bwd = want == RRL_WANT_DIRECT && !p.bwd_rides;
        p.write_rides = (in_tail || in_bwd) && (!o.count_rider || p.count_rides) && B == 1 && L > 0 && wr->n > 0 &&
                        wr->rounds > 0 && wtiles * wr->rounds < 512 &&
                        sizeof(int32_t) * (size_t)wr->rounds * wtiles <= (in_tail ? 32 : 48) * 1024;
    }
    return 0;
}

// The validation of every narrow entry (rrl_ws.h; the order: include/rrl.h "Refusals")
int rrl_check_call(RrlCall &o, bool pointers, int want, const void *target_ws, const RrlXform *xf) {
    if (!pointers || !o.ws || o.B < 0 || o.N < 0 || o.M < 0 || o.L < 0 || o.L >= (1 << 24)) return RRL_E_ARG;  // 24-bit line ids in LDS
    if (o.mode < RRL_SCAN_STRICT || o.mode > RRL_SCAN_CULL || o.chunk < 0 || target_ws == o.ws) return RRL_E_ARG;
    if (want != RRL_WANT_NONE)
        if (const int rc = rrl_plan(o, want, target_ws, xf)) return rc;
    if (o.s_m < 1 || o.s_n < 1 || o.e_m > RRL_MAX_HITS + 1 || o.e_n > RRL_MAX_HITS + 1) return RRL_E_RANGE;
    return o.ws_bytes < o.w.total ? RRL_E_WS : 0;
}

// ---------------------------------------------------------------------------------------
// the workspaces, described from the field tables of include/rrl.h
// ---------------------------------------------------------------------------------------
extern "C" size_t rrl_workspace_bytes(int B, int N, int M, int L) { return WsLayout(B, N, M, L).total; }

extern "C" int rrl_workspace_layout(int B, int N, int M, int L, size_t *offsets) {
    if (!offsets || B < 0 || N < 0 || M < 0 || L < 0) return RRL_E_ARG;
    const WsLayout layout(B, N, M, L);
    for (int i = 0; i < RRL_WS_FIELDS; ++i) offsets[i] = layout.off[i];
    return 0;
}

// include/rrl.h rrl_workspace_field: a row of the two tables (row = field, + RRL_WS_FIELDS for the wide ones), described
template <class T> struct RrlTypeCode;
template <> struct RrlTypeCode<uint8_t> { static const int v = RRL_T_U8; };
template <> struct RrlTypeCode<int32_t> { static const int v = RRL_T_I32; };
template <> struct RrlTypeCode<float> { static const int v = RRL_T_F32; };
template <> struct RrlTypeCode<int64_t> { static const int v = RRL_T_I64; };
struct RrlFieldNames {  // the enumerators' names in lower case
    char s[RRL_WS_FIELDS + RRL_WW_FIELDS][8];
    RrlFieldNames() {
        int i = 0;
#define RRL_ROW_NAME_(name, type, ...)                          \
    static_assert(sizeof(#name) <= sizeof s[0], #name);         \
    for (int k = 0; k < (int)sizeof(#name); ++k) s[i][k] = (char)tolower(#name[k]); \
    ++i;
        RRL_WS_TABLE(RRL_ROW_NAME_)
        RRL_WW_TABLE(RRL_ROW_NAME_)
    }
};
extern "C" int rrl_workspace_field(int kind, int field, int B, int N, int M, int L, int G, const char **name, int *dtype,
                                   long long dims[4]) {
    static const RrlFieldNames names;
    if (kind < 0 || kind > 1) return RRL_E_ARG;
    const int fields = kind ? RRL_WW_FIELDS : RRL_WS_FIELDS;
    if (field == -1) return fields;
    if (field < 0 || field >= fields) return RRL_E_ARG;
    const size_t b = (size_t)(B > 0 ? B : 0), n = (size_t)(N > 0 ? N : 0), m = (size_t)(M > 0 ? M : 0),
                 l = (size_t)(L > 0 ? L : 0), g = (size_t)(G > 0 ? G : 0);
    const int row = field + (kind ? RRL_WS_FIELDS : 0);
    int i = 0, rank = 0;
#define RRL_ROW_DESCRIBE_(name, type, ...)                                \
    if (i++ == row) {                                                     \
        const size_t e[] = {__VA_ARGS__};                                 \
        static_assert(sizeof e / sizeof *e <= 4, #name);                  \
        rank = (int)(sizeof e / sizeof *e);                               \
        for (int k = 0; dims && k < rank; ++k) dims[k] = (long long)e[k]; \
        if (dtype) *dtype = RrlTypeCode<type>::v;                         \
    }
    RRL_WS_TABLE(RRL_ROW_DESCRIBE_)
    RRL_WW_TABLE(RRL_ROW_DESCRIBE_)
    if (name) *name = names.s[row];
    return rank;
}
