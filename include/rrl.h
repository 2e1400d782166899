/*
 * rrl.h -- C ABI of librrl_hip.so: the MI355X (gfx950) implementation of the
 * intersected-line robust registration loss.
 *
 * The reference (Dengzhi-USTC/A-robust-registration-loss) is pure Python and has
 * no FFI; its boundary is the import surface of code/loss.py.  These entry
 * points are what a binding for that path attaches to: each one names the
 * reference lines it replaces.  The Python drop-in
 * (a-robust-registration-loss_amd/loss.py) calls them through ctypes; see
 * INTEGRATION.md for the stub a maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (PyTorch's
 *     allocator); the library allocates no device memory and never
 *     synchronises -- except rrl_loss_forward_info, whose purpose is the drop-in call's one read-back (the optional
 *     scan-timing hook owns a few hipEvents);
 *   - `stream` is a hipStream_t (pass torch's current stream);
 *   - return value: 0 ok, <0 argument error (RRL_E_*), >0 a hipError_t;
 *   - Refusals.  Every entry of the loss pipeline (rrl_tri_prepare .. rrl_loss_step_ex, rrl_demo_epoch's step) validates its
 *     call ONCE, on the host, before its first launch, and reports what it finds in this order: (1) RRL_E_ARG -- a null
 *     pointer, a negative size, L >= 2^24 (line ids have 24 bits), an unknown scan mode, a negative chunk, target_ws == ws,
 *     and every combination of options the entry does not serve (rrl_opts below: multi-pose, ragged batches); (2)
 *     RRL_E_RANGE -- a bucket range outside 1..RRL_MAX_HITS; (3) RRL_E_WS -- a workspace smaller than
 *     rrl_workspace_bytes(B, N, M, L).  A call that is invalid in several ways reports the first of these.  The wide
 *     entries follow the same order with their own limits (B L < 2^31, 1..RRL_WIDE_MAX_HITS, both workspaces).  An empty
 *     batch or line set (B == 0, L == 0) is valid and returns 0 after the checks;
 *   - all floating-point data is fp32, dense and contiguous;
 *   - re-entrant and thread-safe per stream AND per workspace: no entry keeps state between calls except what the
 *     caller's buffers hold, the options of a call are resolved once at its top (rrl_opts below), and two host threads
 *     may drive different streams with different options concurrently (tests/test_gpu_threads.py).  Calls that share
 *     a workspace or an output buffer must be ordered by the caller.  Process-wide state: only the DEFAULTS that the
 *     rrl_set_* setters / RRL_* environment variables choose (read once per call), the rrl_scan_counters /
 *     rrl_chamfer_counters hooks (profiling; use the per-call counter fields / *_ex entries from threads) and the
 *     rrl_scan_timing ring (a profiling hook, not thread-safe);
 *
 * Layouts
 *   tri   [B][N][9]   pseudo-triangles, row = P0 P1 P2 (xyz interleaved)
 *   line  [B][L][6]   dir(3) (unit length, or all zero), x0(3)
 *   ws    one caller-allocated workspace of rrl_workspace_bytes() bytes that
 *         carries every intermediate from forward to backward; field offsets
 *         come from rrl_workspace_layout().
 */
#ifndef RRL_H
#define RRL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RRL_MAX_HITS 4 /* hits kept per line and cloud: callers use buckets 1..4 */
#define RRL_WIDE_MAX_HITS 8 /* ... by the wide pipeline (rrl_loss_forward_wide): buckets 1..8 */
#define RRL_E_ARG (-1)
#define RRL_E_RANGE (-2) /* bucket range outside 1..RRL_MAX_HITS (the wide entries: 1..RRL_WIDE_MAX_HITS) */
#define RRL_E_WS (-3)    /* workspace too small */

/* scan modes */
#define RRL_SCAN_STRICT 0 /* all 3 points of every (line, triangle) are evaluated */
#define RRL_SCAN_LAZY 1   /* points 1,2 only where point 0 passes: same labels; a NaN (negative
                             sqrt argument) is reported only if it occurs in an evaluated pair */
#define RRL_SCAN_AUTO 2   /* per wavefront: lazy where a NaN is provably impossible for its
                             lines (|dir|^2 <= 1+1e-6 and (|x0| + max|P|)^2 <= 100), else strict.
                             Same results AND same NaN detection as strict. */
#define RRL_SCAN_CULL 3   /* default.  Triangles are sorted by grid cell (Hilbert order) under a three-
                             level sphere tree; a line looks only at the halves of 8 whose sphere it can
                             reach, found by a conservative test that is valid at any finite data scale
                             (DESIGN.md "culling bound"); there a conservative FMA prefilter on point 0
                             picks the candidates (~3 %) and the reference's own arithmetic decides on
                             all three points of those: labels, hit lists and the loss equal strict's
                             bit for bit.  NaN detection equals strict's at
                             every scale (round 3): where (|x0| + max|P|)^2 < 111 and |dir|^2 <= 1 + 1e-6 a NaN
                             is provably impossible; lines with |dir|^2 > 1 + 1e-6 or non-finite data send
                             their wavefront of 128 lines through the strict loop (STATUS[1] counts such
                             wavefronts); for unit directions at larger scale (the demo's full-diagonal
                             radius) the walk is widened by every triangle's NaN reach (DEL1 / DEL2), so
                             that each triangle one of whose three points could see a negative sqrt
                             argument is evaluated exactly (csrc/rrl_cull.hip, "NaN").
                             Needs N, M <= rrl_sort_capacity() (2^20), else behaves like AUTO. */

/* ---- workspace fields ---------------------------------------------------------------------------
 * ONE table per workspace: a row X(NAME, element type, extents...) per field, in the order of the field's index.  The
 * extents (one to four, outermost first) are expressions in b, n, m, l -- the call's B, N, M, L, a negative one taken
 * as 0 -- and g, the number of groups (G = 1 pooled, else B; g <= b).  Generated from the table: the enumerators
 * RRL_WS_<NAME> (indices into rrl_workspace_layout's offset array), the layout (a field occupies sizeof(element) x the
 * product of its extents at g = b, rounded up to 256 bytes; fields follow each other in table order), what
 * rrl_workspace_field reports (and the Python views made from it) and the host accessors' pointer types
 * (csrc/rrl_ws.h).  Adding a field is adding one row. */
#define RRL_T_U8 0 /* element types as rrl_workspace_field reports them: uint8_t */
#define RRL_T_I32 1 /* int32_t */
#define RRL_T_F32 2 /* float */
#define RRL_T_I64 3 /* int64_t */

#define RRL_WS_TABLE(X)                                                                                                           \
    X(STATUS, int32_t, 4) /* [0] = NaN seen (reference exit(0), loss.py:89-91); [1] = wavefronts of the
                          culled scan that fell back to the strict loop; [2] = samples whose exchange reduce was repaired
                          by their last workgroup after a hand-off time-out (rrl_set_spin_limit); [3] = internal ticket */        \
    X(NVALS, int32_t, b)  /* (unused since the compact-slot layout; kept for ABI stability) */                                    \
    X(NSEL, int32_t, b)   /* selected lines per sample (length of SEL[b]) */                                                      \
    X(PMAX, float, 2, b)  /* max |P|^2 per cloud and sample (maintained as uint32 bit patterns) */                                \
    X(COUNT1, int32_t, b, l) /* hit count, cloud 1 (loss.py:185) */                                                               \
    X(COUNT2, int32_t, b, l)                                                                                                      \
    X(HIT1, int32_t, b, l, 4) /* unordered hit indices */                                                                         \
    X(HIT2, int32_t, b, l, 4)                                                                                                     \
    X(PTRI1, float, b, n, 12) /* 9 coords, thr2, thr, original triangle index (int): the scans' records.  Rows in
                          original order after a cold build, at the triangles' SORTED positions after a prepared build
                          (rrl_opts.order1 / order2) -- slot 7 of the cloud's first APART row says which (0 / 1)  */              \
    X(PTRI2, float, b, m, 12)                                                                                                     \
    X(P0S1, float, b, (n + 63) / 64 * 64, 4) /* P0 + thr2 in grid-cell (Hilbert curve) order -- clouds of more than 4096
                          triangles: each chunk of 4096 (by original index) in its own order; padded to whole              */     \
    X(P0S2, float, b, (m + 63) / 64 * 64, 4) /* supergroups of 64 sorted triangles; pad records have thr2 = 0 (never hit) */      \
    X(IDX1, int32_t, b, (n + 63) / 64 * 64) /* original triangle index of each sorted position */                                 \
    X(IDX2, int32_t, b, (m + 63) / 64 * 64)                                                                                       \
    X(GRP1, float, b, (n + 63) / 64, 13, 4) /* sphere tree (centre, conservative radius; NaN = empty): per   */                   \
    X(GRP2, float, b, (m + 63) / 64, 13, 4) /* supergroup [0] its own sphere, [1..4] its groups of 16, [5..12] their halves of 8 */ \
    X(CREC1, float, b, (n + 15) / 16 * 16, 4) /* P0 + thr2 in original order (input of the sort) */                               \
    X(CREC2, float, b, (m + 15) / 16 * 16, 4)                                                                                     \
    X(APART, float, 2, b, ((n > m ? n : m) + 255) / 256, 8) /* per-workgroup AABB / max |P|^2 partials (slot 7: PTRI layout) */   \
    X(KJ, uint8_t, b, l)   /* k | j<<4, 0 = line not selected */                                                                  \
    X(SEL, int32_t, b, l)  /* indices of the selected lines, compacted (any order) */                                             \
    X(HS1, int32_t, b, l, 4) /* ascending hit indices (nonzero() order) */                                                        \
    X(HS2, int32_t, b, l, 4)                                                                                                      \
    X(W1, float, b, l, 4, 3) /* weights d / sum d (loss.py:92) */                                                                 \
    X(W2, float, b, l, 4, 3)                                                                                                      \
    X(Q1, float, b, l, 4, 4) /* intersection points q (xyz, 0) (loss.py:155-163) */                                               \
    X(Q2, float, b, l, 4, 4)                                                                                                      \
    X(D, float, b, l, 16)  /* k x j block of |q1-q2|^2 (loss.py:165-166) */                                                       \
    X(VALS, float, b, (l + 1023) / 1024 * 1024, 16) /* canonical 4x4 D tiles (+inf padded) of the selected lines
                          at compact slots: slot = 1024 * x + rank for the x-th 1024-line tile (input of the reduce kernel) */    \
    X(MED, float, g)         /* lower median (loss.py:223-224) */                                                                 \
    X(BCNT, int32_t, g, 16)  /* lines per (k,j) bucket */                                                                         \
    X(BSUM, int64_t, g, 16, 2) /* bucket sums of row / column minima, 2^-40 fixed pt */                                           \
    X(INFO, int32_t, g, 4) /* nbuckets, nselected, nvalues, STATUS[0] (the scan's NaN flag; after a CHAINED step's fused
                          launch: the sample's OWN flag, CHAIN[b][1])  */                                                         \
    X(TRI1, float, b, n, 9) /* transformed source triangles (rrl_registration_*) */                                               \
    X(G1, float, b, n, 9)   /* gradient w.r.t. TRI1 (rrl_registration_backward) */                                                \
    X(RPART, float, b, (3 * n + 1023) / 1024 + 1, 12) /* rigid-apply backward partial sums */                                     \
    X(GACC, float, 12 * b + 16) /* dL/dR [B][9], dL/dt [B][3], shard payload [14]: zeroed by
                          rrl_registration_forward, accumulated by rrl_registration_backward     */                               \
    X(KJC, uint8_t, b, (l + 1023) / 1024 * 1024) /* k | j<<4 at the compact slots */                                              \
    X(BLKCNT, int32_t, b * ((l + 1023) / 1024 + 1)) /* selected lines per 1024-line tile */                                       \
    X(HISTG, int32_t, (n > 4096 || m > 4096) ? 2 * b * 2 * 4096 : 4) /* cell counts and cursors of the wide sort (clouds > 4096) */ \
    X(DEL1, float, b, n) /* NaN reach of a triangle: max(|P1-P0|, |P2-P0|) - thr, clamped at 0, rounded up: how   */              \
    X(DEL2, float, b, m) /* much farther than thr points 1, 2 can sit from point 0 (culled scan, NaN detection);
                          rows laid out like PTRI's (original order / sorted positions)                                  */       \
    X(MHIST, int32_t, b, 2048) /* histogram of the D values' bits 30..20, accumulated by the per-line stage (the
                          median's first radix pass); MHIST, MCTL, MSUM are contiguous and cleared per call                 */    \
    X(MCTL, int32_t, b, 64) /* [0..15] lines per (k,j) bucket (per-line stage); [16] candidate cursor, [17] / [18]
                          arrival counters of the tiled reduce, [19] its error flag (spin time-out), [20] / [21] the median's
                          bits and their ready flag (crowded bin), [22] a non-finite Welsch term; [30], [31] arrival counters
                          of the Chamfer walk on this workspace, per direction; row 0 only: [32] that walk's counter of the
                          groups, [34..35] uint64 fixed-point sum of the valid losses (the step's payload): RRL_MCTL_* below */   \
    X(MSUM, int64_t, b, 32) /* bucket sums of the tiled reduce (2^-40 fixed point, device atomics) */                             \
    X(MCAND, int32_t, b, 2048) /* D values (bit patterns) of the median's bin, gathered by the tiled reduce */                    \
    X(LMAX, float, b, 64, 2) /* (max |dir|^2, max |x0|^2) over 1/64 of a sample's cullable lines: the culled scan's
                          slacks come from their maxima (written by the records kernel, or by the scan entry itself)       */     \
    X(LIDC, int32_t, b, (l + 1023) / 1024 * 1024) /* line index | (k | j<<4) << 24 at the compact slots (the tail kernel's way
                          from a compact slot back to the per-line arrays)                                                 */     \
    X(VLIST, float, b, (l + 1023) / 1024, 16384) /* the valid D values of each 1024-line tile as a dense list (arbitrary order,
                          padded with -1 to a multiple of 4): what the tail kernel streams to find the median                */   \
    X(VLCNT, int32_t, b * ((l + 1023) / 1024 + 1)) /* their number per tile */                                                    \
    X(CHAIN, int32_t, b, 4) /* per-sample words of a CHAINED step (RRL_F_CHAIN / RRL_F_CHAINED, round 6): [0] records
                          workgroups of the sample that have finished in the step's build + scan launch, [1] the scan's NaN
                          flag of the sample, [2] its wavefronts that fell back to the strict loop, [3] wait time-outs; all
                          zero between calls (cleared on exit by the sample's last tail workgroup)                          */    \
    X(GFIX, int64_t, b * (n + m) * 9 + b) /* deterministic scatter backward (rrl_opts.deterministic with rrl_loss_step_ex /
                          rrl_loss_backward): fixed-point accumulators of dL/dpoints1 (and dL/dpoints2), order-independent like
                          MSUM; behind them one non-finite int32 flag per sample and cloud                                  */
#define RRL_WS_ENUM_(name, type, ...) RRL_WS_##name,
enum { RRL_WS_TABLE(RRL_WS_ENUM_) RRL_WS_FIELDS };

/* ---- wide bucket ranges -----------------------------------------------------------------------
 * Every entry above serves bucket ranges within 1..RRL_MAX_HITS (e_m, e_n <= 5: every reference caller's
 * (1, 1, 5, 5)) and returns RRL_E_RANGE beyond.  The reference accepts any range (code/loss.py:170-232; its header,
 * code/loss.py:10-17, names the maximum number of intersections per line as the metric's approximation knob).  The
 * WIDE pipeline serves 1 <= s_m, s_n and e_m, e_n <= RRL_WIDE_MAX_HITS + 1: up to 8 hits per line and cloud.  It runs the
 * scan of any mode into an ordinary loss workspace (ws, rrl_workspace_bytes) and its own stages into a second, WIDE
 * workspace (wws, rrl_wide_workspace_bytes): the lines of the range that have more than 4 hits in a cloud are
 * re-evaluated against all of that cloud's triangles with the scan's strict predicate (hit recovery; the number of hits
 * found must equal the scan's count, else STATUS[0] of the wide workspace is non-zero and the result must not be used),
 * then weights, intersection points, the k x j block of D (<= 64 values), exact lower median, Welsch row / column minima
 * and 2^-40 fixed-point bucket sums over 64 buckets, as the narrow stages do over 16.  Same results as the reference
 * (the forward is deterministic); for a range within 1..4 it gives the narrow entries' loss bits.  Not served by the
 * wide entries: carried-over targets, chained steps, riders, multi-pose evaluation, deterministic gradients, the fused
 * registration steps.  DESIGN.md "Wide bucket ranges". */
#define RRL_WW_TABLE(X) /* rows as in RRL_WS_TABLE */                                                                             \
    X(STATUS, int32_t, 4) /* [0] lines whose recovered hits disagree with the scan's count (must be 0); [1] hit-recovery
                          entries (selected line, cloud with > 4 hits); [2], [3] zero */                                          \
    X(NSEL, int32_t, b)          /* selected lines per sample */                                                                  \
    X(REC, int32_t, 2 * b * l)   /* hit-recovery entries: slot | cloud << 31 */                                                   \
    X(SEL, int32_t, b, l)        /* line index of each selected line, compacted (any order): the SLOT of a line */                \
    X(KJ, uint8_t, b, l)         /* k | j << 4 by slot */                                                                         \
    X(HS1, int32_t, b, l, RRL_WIDE_MAX_HITS) /* ascending hit indices by slot (nonzero() order) */                                \
    X(HS2, int32_t, b, l, RRL_WIDE_MAX_HITS)                                                                                      \
    X(W1, float, b, l, RRL_WIDE_MAX_HITS, 3)     /* weights d / sum d (loss.py:92) */                                             \
    X(W2, float, b, l, RRL_WIDE_MAX_HITS, 3)                                                                                      \
    X(Q1, float, b, l, RRL_WIDE_MAX_HITS, 4)     /* intersection points (xyz, 0) */                                               \
    X(Q2, float, b, l, RRL_WIDE_MAX_HITS, 4)                                                                                      \
    X(D, float, b, l, RRL_WIDE_MAX_HITS, RRL_WIDE_MAX_HITS) /* the k x j block of |q1 - q2|^2 by slot (entries outside it undefined) */ \
    X(MED, float, g)             /* lower median */                                                                               \
    X(BCNT, int32_t, g, RRL_WIDE_MAX_HITS * RRL_WIDE_MAX_HITS) /* lines per (k, j) bucket, index (k - 1) 8 + (j - 1) */           \
    X(BSUM, int64_t, g, RRL_WIDE_MAX_HITS * RRL_WIDE_MAX_HITS, 2) /* bucket sums of row / column minima, 2^-40 fixed point */     \
    X(INFO, int32_t, g, 4)       /* nbuckets, nselected, nvalues, the scan's NaN flag (STATUS[0] of ws) */
#define RRL_WW_ENUM_(name, type, ...) RRL_WW_##name,
enum { RRL_WW_TABLE(RRL_WW_ENUM_) RRL_WW_FIELDS };

/* ---- control words ---------------------------------------------------------------------------
 * The words inside a sample's MCTL and CHAIN rows (RRL_WS_TABLE above) that kernels of different launches hand to each
 * other: ONE map, so that nobody has to find every user to know that they do not overlap (csrc/rrl_ws.h asserts it).
 * Two disciplines (DESIGN.md "What the workspace promises"; tests/test_gpu_workspace.py holds both):
 *   - REWOUND by their last user, so they read zero whenever the stream is idle: CURSOR, TICK1, TICK2, ERR, MEDRDY, BAD,
 *     CHAM_GROUP, CHAM_TOP and every CHAIN word (also MSUM, and STATUS[3], the rigid backward's ticket);
 *   - CLEARED BY THE NEXT CALL's first launch with the rest of MHIST .. MSUM, and left as they are until then: the sixteen
 *     BUCKET words, MEDBITS, LSUM (and MHIST).
 * Neither kind needs the caller's help: the first launch of every call that builds records clears MHIST .. MSUM -- on the
 * sorted layout the CHAIN rows too -- whatever they hold (the chained step's fused launch excepted: RRL_F_CHAINED promises
 * it the workspace as the previous step left it).  A workspace may hold anything before the first call into it. */
enum {
    RRL_MCTL_BUCKET0 = 0,     /* [0..15] lines per (k, j) bucket, index (k - 1) 4 + (j - 1): per-line stage -> reduce */
    RRL_MCTL_CURSOR = 16,     /* exchange reduce: cursor of the sample's candidate list (MCAND) */
    RRL_MCTL_TICK1 = 17,      /* exchange reduce: workgroups that have published their candidates */
    RRL_MCTL_TICK2 = 18,      /* exchange reduce, tail kernel: workgroups whose sums are in MSUM; the last arriver finishes */
    RRL_MCTL_ERR = 19,        /* exchange reduce: a hand-off timed out (rrl_set_spin_limit): the last workgroup repairs */
    RRL_MCTL_MEDBITS = 20,    /* exchange reduce, crowded bin: the median's bit pattern, published by tile 0 ... */
    RRL_MCTL_MEDRDY = 21,     /* ... and its ready flag */
    RRL_MCTL_BAD = 22,        /* exchange reduce, tail kernel: a non-finite Welsch term (median 0): the loss is NaN */
    RRL_MCTL_CHAM_GROUP = 30, /* [30], [31] Chamfer walk on the loss workspace: arrival counter of the sample's direction */
    RRL_MCTL_CHAM_TOP = 32,   /* row 0 only: ... and of the (sample, direction) groups */
    RRL_MCTL_LSUM = 34,       /* row 0 only, [34..35]: uint64 2^-40 fixed-point sum of the valid samples' losses (payload[0]) */
    RRL_MCTL_WORDS = 64       /* the row */
};
enum {
    RRL_CHAIN_READY,    /* records workgroups of the sample that have finished in the chained step's build + scan launch */
    RRL_CHAIN_NAN,      /* that launch's NaN flag of the sample (the plain scan: STATUS[0]) */
    RRL_CHAIN_FALLBACK, /* ... its wavefronts that fell back to the strict loop (STATUS[1]) */
    RRL_CHAIN_TIMEOUT,  /* source workgroups that gave up waiting for their records: the sample's loss is NaN */
    RRL_CHAIN_WORDS     /* the row */
};

const char *rrl_version(void);
/* Largest cloud (triangles of either cloud) that the SORTED layout serves: the per-step cell sort and sphere tree, the
 * culled scan (RRL_SCAN_CULL), prepared orders (rrl_cloud_order, rrl_opts.order1 / order2), multi-pose evaluation
 * (rrl_opts.problems), the Chamfer tree (rrl_chamfer_tree_fwd, rrl_chamfer_from_loss) and its rider.  2^20 = 1048576.
 * Larger clouds take the dense scan: scan mode cull behaves like AUTO there. */
int rrl_sort_capacity(void);

/* ---- per-call options ------------------------------------------------------------------------
 * Every entry point that has an `_ex` twin takes `const rrl_opts *opts` in front of the stream; NULL (and the
 * plain entry) means "the library defaults", i.e. what rrl_set_* / the RRL_* environment variables selected.
 * A field left at -1 / NULL also means "default".  The options are resolved ONCE at the top of a call and travel
 * through all of its stages by value, so a call never observes a setter running in another thread half way
 * through, and two host threads may drive different streams with different options at the same time (the only
 * process-wide state left are the defaults themselves and the rrl_scan_timing ring, a profiling hook).
 * Thread-safety contract: re-entrant; thread-safe per stream and per workspace -- two calls that
 * share a workspace or output buffers must be ordered by the caller (same stream, or events). */
#define RRL_F_TARGET_KEPT 1  /* with order1: cloud 2's prepared records, sphere tree and partials in `ws` are those
                                the PREVIOUS call on this workspace built from the same tri2 -- the target has not moved
                                (code/test_demo_optimized_Lie_Algebra.py:57-62, rpm/Train_RPM.py:207-231 move only the
                                source) -- so nothing of cloud 2 is rebuilt; order2 is not read.  Same results bit for bit. */
/* CHAINED steps (round 6): a loop that calls rrl_loss_step_ex / rrl_registration_step_ex again and again on ONE workspace
 * with a kept target (the demo, code/test_demo_optimized_Lie_Algebra.py:48-62; a trainer's inner iterations).  The target
 * half of the scan (code/loss.py:181-184: the two scans are independent) needs nothing this step's records launch
 * produces -- only cleared hit counts.  RRL_F_CHAIN asks a step to LEAVE them cleared: the per-line stage zeroes
 * COUNT1 / COUNT2 behind its own read, the sample's last tail workgroup zeroes the CHAIN words.  RRL_F_CHAINED tells a
 * step that it FINDS them cleared: records, target scan and source scan then run as ONE launch -- the source records' body
 * in the leading workgroups of the scan's grid, the target-cloud workgroups next, the source-cloud workgroups last, behind
 * the sample's ready word (CHAIN[b][0]); the line slacks come from the scan tile's own lines instead of LMAX.  Three
 * launches instead of four, same labels / hit lists / loss bits.
 *   - *chain_left (rrl_opts, host memory, written when the call is ISSUED): bit 0 = this call leaves the workspace
 *     chain-clean (the shape is served by the per-line stage + tail kernel / exchange reduce and RRL_F_CHAIN was set); bit 1 =
 *     THIS call's build ran fused (RRL_F_CHAINED was honoured);
 *   - RRL_F_CHAINED is valid only when the PREVIOUS call on this workspace reported chain_left bit 0 and nothing else has
 *     written the workspace since; it needs RRL_F_TARGET_KEPT and is ignored (plain 4-launch step) whenever the fused
 *     launch cannot serve the call (rider, counters, multi-pose, other reduce kernels, thin grids); a step without
 *     RRL_F_CHAIN takes the plain build too, for the fused launch only serves a step that leaves the workspace chain-clean;
 *   - after a step with RRL_F_CHAIN COUNT1 / COUNT2 read zero (KJ / HS1 / HS2 hold what the per-line stage read), so its
 *     workspace cannot serve as another call's target_ws; after a step whose build was fused STATUS is not updated:
 *     INFO[b][3] carries each sample's OWN NaN flag (the plain step reports the batch-wide STATUS[0] in every row), and a
 *     source workgroup that gave up waiting for its records (RRL_CHAIN_SPIN polls; CHAIN[b][3]) makes that sample's loss NaN. */
#define RRL_F_CHAIN 2
#define RRL_F_CHAINED 4
/* A Chamfer walk carried by the evaluation's own scan launch (round 4b).  rrl_chamfer_from_loss -- the monitor every caller
 * of the reference computes next to the loss (rpm/Train_RPM.py:223-224, dcp/Train_DCP.py:246, fmr/model.py:293,
 * test_demo_optimized_Lie_Algebra.py:68) -- needs the evaluation's records launch only, not its scan, but launches of one
 * stream never overlap on this stack; handed to an `_ex` forward / step through rrl_opts.chamfer, the walk's workgroups
 * are issued in the culled scan's grid (one launch for both, the walk's time hidden beside the scan's).  Same arithmetic,
 * same keys and value as rrl_chamfer_from_loss after the call.  done: clear it before the call; the call sets it to 1
 * (host side, before it returns) when the walk rode along -- also with a carried-over target (`target_ws`: only the source is
 * scanned, the walk reads the target in the workspace that holds it).  Still 0: it did not (scan mode other than cull,
 * counters, fewer than 1024 lines, clouds beyond the sort capacity, an entry that runs no scan) -- call
 * rrl_chamfer_from_loss as before. */
typedef struct rrl_chamfer_rider {
    void *ws;                  /* Chamfer workspace, rrl_chamfer_workspace_bytes(B, N, M) */
    size_t ws_bytes;
    uint64_t *best_x, *best_y; /* [B][N], [B][M] keys (distance bits << 32 | argmin), as rrl_chamfer_from_loss */
    float *value;              /* [1] the mean */
    int32_t done;              /* out */
} rrl_chamfer_rider;

typedef struct rrl_opts {
    int32_t struct_bytes;    /* sizeof(rrl_opts) of the caller's header (fields beyond it are defaults) */
    int32_t flags;           /* RRL_F_* */
    int32_t reduce_mode;     /* -1 default; 0 auto, 1 single, 2 tiled, 3 xchg (rrl_set_reduce_mode) */
    int32_t deterministic;   /* -1 default; 0 / 1 (rrl_set_deterministic) */
    int32_t sort_parts;      /* -1 default; 0 automatic, 1..16 (rrl_set_sort_parts) */
    int32_t scan_variant;    /* -1 default; 0, 1, 2, 4, 8 (rrl_set_scan_variant) */
    /* Prepared clouds: order [B][64 ceil(n / 64)] from rrl_cloud_order -- sorted position -> triangle, computed ONCE
     * per cloud in any rigid frame of it.  Both given (or order1 + RRL_F_TARGET_KEPT), scan mode cull: the cell sort
     * leaves the step; one wide launch moves the source, writes the records at their sorted positions and refits
     * the sphere tree.  The first n entries of every row MUST be a permutation of [0, n) (the kernels only clamp the
     * index range: a duplicated or missing triangle silently changes labels and loss).  ANY permutation gives the same
     * labels, hit lists and loss (the tree is a conservative filter, the reference's arithmetic decides): an order taken
     * in another pose of the cloud, or a stale one, only costs time. */
    const int32_t *order1, *order2;
    uint64_t *scan_counters;       /* per-call counter table of the culled scan (see rrl_scan_counters) */
    long long scan_counter_rows;
    rrl_chamfer_rider *chamfer;    /* NULL, or the evaluation's Chamfer walk to be carried by its scan launch (above) */
    /* rrl_loss_step_ex only (round 5): NULL, or float[14] that receives the batch-shard payload of the section-8(d) step
     * { sum of the valid losses, #valid, 0 x 12 } -- the buffer a rank contributes to the all-reduce of the scalar loss
     * (points1.grad stays local, so the (dR, dt) slots of rrl_registration_step's payload stay zero).
     * Ideally the workspace's GACC + 12 B floats (cleared by the step's first launch when R, t are given); any other
     * buffer is cleared by a fill launch first.  Written in the reduce's launch where the scatter rides in it, else by
     * one small launch behind the backward. */
    float *payload;
    /* MULTI-POSE evaluation (round 5): 0, or Bt with B % Bt == 0 and Bt < B.  The iterative trainers evaluate several
     * poses of the SAME source against the SAME target along the SAME lines (rpm/Train_RPM.py:207-231 num_iter,
     * fmr/model.py:292-308 the last three estimates), and all poses are known before the first loss call.  With
     * problems = Bt the fused entries that move the source (rrl_registration_forward_ex / _backward_ex / _step_ex,
     * rrl_loss_step_ex with R, t) take src [Bt][N][9], tri2 [Bt][M][9], line [Bt][L][6] and the orders [Bt][..] with
     * R [B][3][3], t [B][3]: instance s = pose (s / Bt) of problem (s % Bt).  Every output (loss [B], gR [B][9], gt [B][3],
     * grad_tri1 [B][N][9], the workspace of B instances) is per instance and bit-identical to evaluating the B / Bt poses one
     * after the other; the target's scan runs ONCE per problem (instances < Bt), the sources' scans side by side in the same
     * launch.  Scan mode cull, clouds within the sort capacity (rrl_sort_capacity), no target_ws, pool = 0; RRL_E_ARG
     * otherwise. */
    int32_t problems;
    int32_t *chain_left;     /* NULL, or a HOST int32 that receives the two bits above at issue time (RRL_F_CHAIN) */
    /* RAGGED batches: NULL (all rows), or DEVICE int32 [B] -- the number of source triangles, target triangles and lines
     * sample b really has.  tri1 [B][N][9], tri2 [B][M][9], line [B][L][6] keep their meaning as capacities and strides;
     * sample b is evaluated as if the call were B = 1 on tri1[b][0 .. count1[b]), tri2[b][0 .. count2[b]),
     * line[b][0 .. nlines[b]): same loss bits, INFO row, median and hit lists.  Rows beyond a count are never interpreted
     * (they may hold NaN, inf, anything): no hit, no tree node, no partial box, no line maximum, no NaN flag, gradient rows
     * exactly zero.  A sample with a zero count has no populated bucket: loss 0, INFO[b][0] = 0.  The counts are read by
     * the kernels (a workgroup-uniform load), never on the host -- a ragged call does not synchronise and can be captured
     * in a graph; a kernel clamps a count to [0, capacity] (memory safety only).  A prepared order of a ragged cloud is
     * [B][64 ceil(N / 64)] whose first count[b] entries are a permutation of [0, count[b]); the rest is not read.  With
     * RRL_F_TARGET_KEPT count2 must hold what it held when the target was built.  A staged entry reads the counts of its
     * OWN call's opts: the build count1 / count2, the scan all three -- the SAME values: the builds write nothing beyond a
     * sample's last supergroup, so a scan with larger counts (or none) walks unwritten records --, the later stages none.
     * For the same reason rrl_chamfer_from_loss must not be run on the workspace of a ragged call.  Workgroups of the builds and
     * scans whose rows, supergroups or lines lie wholly beyond their sample's counts leave before their first load.
     * A call with counts takes the plain four-launch step where a chained one was asked for (same bits), and is refused
     * (RRL_E_ARG, before any launch) together with: pool != 0, problems (multi-pose), the Chamfer rider, target_ws, the
     * wide entries, clouds beyond the sort capacity.  DESIGN.md "Ragged batches". */
    const int32_t *count1, *count2, *nlines;
} rrl_opts;

size_t rrl_workspace_bytes(int B, int N, int M, int L);
/* offsets[RRL_WS_FIELDS] in bytes from the workspace base */
int rrl_workspace_layout(int B, int N, int M, int L, size_t *offsets);
/* field `field` of workspace `kind` (0: RRL_WS_*, 1: RRL_WW_*) at shape (B, N, M, L, G): its lower-case name (static
 * string), element type (RRL_T_U8 / RRL_T_I32 / RRL_T_F32 / RRL_T_I64) and extents; returns the number of extents
 * (1..4), or RRL_E_ARG for an unknown kind / field.  field == -1: returns the number of fields of that kind.  Any output
 * pointer may be NULL. */
int rrl_workspace_field(int kind, int field, int B, int N, int M, int L, int G, const char **name, int *dtype,
                        long long dims[4]);

/* ---- fused entry points (what loss.py calls) ------------------------------------------ */

/* Forward of cal_loss_intersection_batch_whole_median_pts_lines (code/loss.py:170-232) for
 * B samples in 4 launches: prepare -> scan -> per-line distances -> median + Welsch reduce.
 *   loss [G], G = pool ? 1 : B.  pool != 0 reproduces the reference's own B>1 behaviour
 *   (all lines pooled, LAST sample's median: SURVEY.md Q2); pool == 0 gives B independent
 *   losses (what the reference's callers compute by looping B = 1 calls).
 *   loss[g] is 0 and INFO[g][0] == 0 where no (k,j) bucket is populated (the reference
 *   returns (None, None, None), loss.py:231-232).
 * chunk = triangles per workgroup of the scan (0 = default). */
int rrl_loss_forward(const float *tri1, const float *tri2, const float *line, void *ws,
                     size_t ws_bytes, float *loss, int B, int N, int M, int L, int s_m, int s_n,
                     int e_m, int e_n, int pool, int mode, int chunk, void *stream);

/* Closed-form backward (autograd of code/loss.py:170-232).
 * grad_loss [G]; grad_tri1 [B][N][9] is zeroed then accumulated; grad_tri2 may be NULL. */
int rrl_loss_backward(const float *tri1, const float *tri2, const void *ws, size_t ws_bytes,
                      const float *grad_loss, float *grad_tri1, float *grad_tri2, int B, int N,
                      int M, int L, int pool, void *stream);

/* Fused training op (the rigid transform of the call sites + the loss: rpm/Train_RPM.py:205-231,
 * dcp/Train_DCP.py:233-270, fmr/model.py:265-313; code/loss.py:458-463 for the demo): the source
 * pseudo-triangles src [B][N][9] are moved by per-sample (R [B][3][3], t [B][3]) -- x R + t, or
 * x R^T + t when transpose_r -- into the workspace (TRI1) and the loss is evaluated against
 * tri2, all in one call.  The backward returns dL/dR, dL/dt (deterministic reduction), optionally
 * dL/dsrc (may be NULL), and, when payload != NULL, the 14-float batch-shard payload
 * { sum of valid losses, #valid, sum_b dR, sum_b dt } for the all-reduce.  pool must be 0.
 * With grad_src == NULL the gradients are accumulated with float atomics in one launch: pass
 * gR = GACC, gt = GACC + 9 B, payload = GACC + 12 B (the workspace field the forward zeroed) to
 * avoid three extra clearing launches; any other buffers are cleared by the call first. */
int rrl_registration_forward(const float *src, const float *R, const float *t, const float *tri2,
                             const float *line, void *ws, size_t ws_bytes, float *loss, int B,
                             int N, int M, int L, int transpose_r, int s_m, int s_n, int e_m,
                             int e_n, int mode, int chunk, void *stream);
/* The same two forwards with the TARGET's scan carried over: target_ws is a workspace of equal
 * (B, N, M, L) that already ran a forward with the same tri2 and line (RPM and FMR evaluate
 * num_iter source poses against one target and one line set, rpm/Train_RPM.py:204-231,
 * fmr/model.py:295-310).  Only the source cloud is prepared/sorted/scanned; the target's hit
 * counts and lists are READ in target_ws by the per-line stage (round 4b; they used to be copied: two launches) -- so
 * target_ws must be the workspace of the FULL evaluation that scanned the target (not of another carried-over one), and
 * it must stay untouched until this call's kernels have run (same stream, or an event).  COUNT2 / HIT2 of `ws` are not
 * written.  target_ws == NULL: identical to the plain call.  The result is bit-identical to the plain call either way. */
int rrl_loss_forward_cached(const float *tri1, const float *tri2, const float *line, void *ws,
                            size_t ws_bytes, float *loss, int B, int N, int M, int L, int s_m,
                            int s_n, int e_m, int e_n, int pool, int mode, int chunk,
                            const void *target_ws, void *stream);
int rrl_registration_forward_cached(const float *src, const float *R, const float *t,
                                    const float *tri2, const float *line, void *ws, size_t ws_bytes,
                                    float *loss, int B, int N, int M, int L, int transpose_r,
                                    int s_m, int s_n, int e_m, int e_n, int mode, int chunk,
                                    const void *target_ws, void *stream);
/* rrl_loss_forward_cached followed by the read-back the drop-in call needs: INFO (4 int32 per group: nbuckets,
 * nselected, nvalues, NaN flag) is copied to host_info [4 G] (host memory, ideally pinned) and the call waits
 * for the stream.  The reference's callable returns a tensor, None (no populated bucket, code/loss.py:231-232)
 * or exits (NaN, :88-91): a host-side decision per call by contract, so this is the one entry that synchronises. */
int rrl_loss_forward_info(const float *tri1, const float *tri2, const float *line, void *ws,
                          size_t ws_bytes, float *loss, int B, int N, int M, int L, int s_m, int s_n,
                          int e_m, int e_n, int pool, int mode, int chunk, const void *target_ws,
                          int32_t *host_info, void *stream);
/* Opt-in bit-reproducible backward (the reference's CPU autograd is deterministic).  on != 0 (or rrl_opts.deterministic = 1)
 *   - replaces the float atomics of rrl_registration_backward's direct route (grad_src == NULL) by per-workgroup partial
 *     sums added in a fixed order by a second, tiny launch;
 *   - (round 6) makes the SCATTER backward to points1.grad / points2.grad -- rrl_loss_backward, rrl_loss_step_ex, and the
 *     scatter in front of the rigid backward when rrl_registration_backward is asked for grad_src -- accumulate
 *     in 64-bit fixed point (workspace field GFIX; the unit is a power of two derived per sample from |dL/dloss|, the
 *     bucket count and the median, so that 2^24 contributions cannot overflow): integer sums do not depend on the order of the
 *     atomics.  One more launch converts them to fp32; rrl_loss_step_ex then runs forward + backward + conversion instead of
 *     carrying the scatter in its reduce launch.  Every contribution is rounded to the unit (2^-38 .. 2^-61 of the largest
 *     possible one): the result agrees with the float-atomic one to ~1e-6 of the largest entry and reproduces bit for bit.
 * Env RRL_DETERMINISTIC=1 sets the initial state.  The forward is deterministic either way. */
int rrl_set_deterministic(int on);
int rrl_registration_backward(const float *src, const float *R, const float *tri2, void *ws,
                              size_t ws_bytes, const float *loss, const float *grad_loss,
                              float *grad_src, float *gR, float *gt, float *payload, int B, int N,
                              int M, int L, int transpose_r, void *stream);

/* Forward + direct backward of the fused training op in ONE call -- what a training step does when dL/dloss is
 * known up front (grad_loss [B], usually ones): rpm/Train_RPM.py:226-259, dcp/Train_DCP.py:246-270 compute the loss
 * and call backward() right away.  Same arguments and results as rrl_registration_forward_cached followed by
 * rrl_registration_backward(grad_src = NULL); where the tail kernel serves the shape (auto mode: 2 .. 32 line tiles per
 * sample and B x tiles <= 256; not in deterministic mode) the backward rides in the reduce's launch -- 4 launches per
 * step with prepared orders (rrl_opts), 5 without -- and the two kernels' chains of dependent loads overlap; a single
 * tile of lines (L <= 1024) is finished by one workgroup per sample (per-line stage + reduce + backward); every other
 * shape runs the forward and then the backward launch.  gR [B][9], gt [B][3], payload [14] or NULL: ideally the
 * workspace's GACC field. */
int rrl_registration_step(const float *src, const float *R, const float *t, const float *tri2,
                          const float *line, void *ws, size_t ws_bytes, float *loss, const float *grad_loss,
                          float *gR, float *gt, float *payload, int B, int N, int M, int L, int transpose_r,
                          int s_m, int s_n, int e_m, int e_n, int mode, int chunk, const void *target_ws,
                          void *stream);

/* ---- prepared clouds (round 4) ----------------------------------------------------------------
 * The reference itself points at a spatial structure (code/loss.py:260-262), and every caller moves the SAME source
 * rigidly, step after step, against a target that never moves (test_demo_optimized_Lie_Algebra.py:57-62,
 * rpm/Train_RPM.py:207-231).  A rigid motion preserves the spatial order of a cloud, so the order is computed once
 * per cloud (dataset item / demo start) and handed to every later call through rrl_opts.order1 / order2.
 * rrl_cloud_order: order [B][64 ceil(n/64)] int32 = sorted position -> triangle index (positions >= n hold 0) for
 * the clouds tri [B][n][9] in the frame they are given in.  Because it runs once it builds a better order than the
 * per-step cell sort: a full K-D ORDER (csrc/rrl_order.hip) -- positions form an implicit binary tree of aligned
 * power-of-two windows, every window sorted along the longest axis of its records' bounding box, down to halves of
 * 8 -- so the scan's tree nodes (aligned runs of 64 / 16 / 8 positions) are compact k-d cells of the WHOLE cloud
 * (the per-step sort orders clouds beyond 4096 triangles in four or more interleaved chunks).  Only the first point
 * of a row places it.  ws: scratch of rrl_cloud_order_workspace_bytes(B, n) bytes.  n <= rrl_sort_capacity(). */
size_t rrl_cloud_order_workspace_bytes(int B, int n);
int rrl_cloud_order(const float *tri, int32_t *order, void *ws, size_t ws_bytes, int B, int n, void *stream);
/* the same for point clouds pts [B][n][3] (the Chamfer monitor's inputs: rrl_chamfer_tree_fwd_ex); a cloud of
 * pseudo-triangles and the cloud of their first points have the same order */
int rrl_cloud_order_points(const float *pts, int32_t *order, void *ws, size_t ws_bytes, int B, int n, void *stream);
/* rrl_cloud_order for RAGGED clouds tri [B][n][9] (n = capacity): counts [B] device int32 (clamped to [0, n]); the first
 * counts[b] entries of row b are a permutation of [0, counts[b]) -- rows beyond the count are not read --, the rest 0.
 * counts == NULL: rrl_cloud_order. */
int rrl_cloud_order_counted(const float *tri, const int32_t *counts, int32_t *order, void *ws, size_t ws_bytes, int B, int n,
                            void *stream);

/* The fused entries with per-call options (rrl_opts above; NULL = defaults = the plain entries). */
int rrl_loss_forward_ex(const float *tri1, const float *tri2, const float *line, void *ws, size_t ws_bytes,
                        float *loss, int B, int N, int M, int L, int s_m, int s_n, int e_m, int e_n, int pool,
                        int mode, int chunk, const void *target_ws, const rrl_opts *opts, void *stream);
int rrl_registration_forward_ex(const float *src, const float *R, const float *t, const float *tri2,
                                const float *line, void *ws, size_t ws_bytes, float *loss, int B, int N, int M,
                                int L, int transpose_r, int s_m, int s_n, int e_m, int e_n, int mode, int chunk,
                                const void *target_ws, const rrl_opts *opts, void *stream);
int rrl_registration_backward_ex(const float *src, const float *R, const float *tri2, void *ws, size_t ws_bytes,
                                 const float *loss, const float *grad_loss, float *grad_src, float *gR, float *gt,
                                 float *payload, int B, int N, int M, int L, int transpose_r, const rrl_opts *opts,
                                 void *stream);
int rrl_registration_step_ex(const float *src, const float *R, const float *t, const float *tri2,
                             const float *line, void *ws, size_t ws_bytes, float *loss, const float *grad_loss,
                             float *gR, float *gt, float *payload, int B, int N, int M, int L, int transpose_r,
                             int s_m, int s_n, int e_m, int e_n, int mode, int chunk, const void *target_ws,
                             const rrl_opts *opts, void *stream);

/* SURVEY 8(d) by direct issue: forward + backward to points1.grad in ONE call -- what
 * `loss = cal_loss_intersection_batch_whole_median_pts_lines(...); loss.backward()` delivers through autograd
 * (code/loss.py:170-232: points1.grad (B, N, 9)), with the rigid apply of the call sites in front when R, t are given
 * (code/loss.py:458-463, rpm/Train_RPM.py:205-212): points1 = tri1 R + t (x R^T + t when transpose_r), kept in the
 * workspace field TRI1; R == t == NULL: points1 = tri1 as given.  grad_loss [B] = dL/dloss (usually ones),
 * grad_tri1 [B][N][9] = dL/dpoints1 -- cleared by the call's first launch, accumulated by float atomics like
 * rrl_loss_backward --, grad_tri2 [B][M][9] or NULL.  Where the tail kernel serves the shape (2 .. 32 line tiles,
 * B x tiles <= 256) and grad_tri2 == NULL the scatter rides in the reduce's launch: 4 launches per step with prepared
 * orders (opts), 5 without; a single tile of lines (L <= 1024) is finished by one workgroup per sample (per-line stage +
 * reduce + scatter, one launch: 3 / 4 per step); otherwise forward + the scatter kernel of rrl_loss_backward.  Loss, median, bucket sums
 * bit-identical to rrl_loss_forward / rrl_registration_forward; gradients equal rrl_loss_backward's to the rounding of
 * the atomics.  pool semantics: independent samples (pool = 0). */
int rrl_loss_step_ex(const float *tri1, const float *R, const float *t, const float *tri2, const float *line,
                     void *ws, size_t ws_bytes, float *loss, const float *grad_loss, float *grad_tri1,
                     float *grad_tri2, int B, int N, int M, int L, int transpose_r, int s_m, int s_n, int e_m,
                     int e_n, int mode, int chunk, const void *target_ws, const rrl_opts *opts, void *stream);

/* ---- the wide pipeline (RRL_WW_* above: bucket ranges up to RRL_WIDE_MAX_HITS hits per line) ------------------- */
size_t rrl_wide_workspace_bytes(int B, int N, int M, int L);
/* offsets[RRL_WW_FIELDS] in bytes from the wide workspace's base */
int rrl_wide_workspace_layout(int B, int N, int M, int L, size_t *offsets);
/* Forward of code/loss.py:170-232 for any range 1 <= s_m, s_n, e_m, e_n <= 9: scan into ws (any mode; opts: prepared
 * orders and the scan knobs -- flags, riders, payload and multi-pose are ignored), then 4 launches into wws.  loss [G],
 * pool as rrl_loss_forward; INFO of wws as RRL_WS_INFO.  Range inside 1..4 allowed (the same loss bits as the narrow
 * entries).  The caller must check STATUS[0] of wws (hit recovery) before using the result. */
int rrl_loss_forward_wide(const float *tri1, const float *tri2, const float *line, void *ws, size_t ws_bytes, void *wws,
                          size_t wws_bytes, float *loss, int B, int N, int M, int L, int s_m, int s_n, int e_m, int e_n,
                          int pool, int mode, int chunk, const rrl_opts *opts, void *stream);
/* Backward of a wide forward: grad_loss [G]; grad_tri1 [B][N][9] (and grad_tri2 [B][M][9], or NULL) are zeroed and
 * accumulated with float atomics (dL/dD at the first-occurrence argmin entries; median, weights and labels detached). */
int rrl_loss_backward_wide(const void *wws, size_t wws_bytes, const float *grad_loss, float *grad_tri1, float *grad_tri2,
                           int B, int N, int M, int L, int pool, void *stream);

/* ---- the four forward stages, individually (tests, profiling) ------------------------- */

/* K1': prepared triangles for both clouds + zeroing of the per-call state.
 * thr = mean edge * 1.731 / 2 (code/loss.py:94-110); thr2 = the smallest fp32 x with
 * sqrt(x) >= thr, so that "sqrt(x) < thr" (loss.py:107-110) is decided exactly by x < thr2. */
int rrl_tri_prepare(const float *tri1, const float *tri2, void *ws, size_t ws_bytes, int B, int N,
                    int M, int L, void *stream);

/* With options: sort parts; orders (both): the prepared build -- records at their sorted positions + tree refit in one
 * launch, and PMAX completed by a tiny second launch (inside a fused forward the culled scan's prologue does that).
 * rrl_line_tri_scan_ex must then be given the same opts. */
int rrl_tri_prepare_ex(const float *tri1, const float *tri2, void *ws, size_t ws_bytes, int B, int N,
                       int M, int L, const rrl_opts *opts, void *stream);

/* K1: dense line <-> pseudo-triangle scan of both clouds in one launch
 * (code/loss.py:68-112 for points1 and points2, :181-186).  Emits per line the hit count and
 * the (unordered) indices of the first RRL_MAX_HITS hits; nothing of size L*N is written. */
int rrl_line_tri_scan(const float *line, void *ws, size_t ws_bytes, int B, int N, int M, int L,
                      int mode, int chunk, void *stream);

int rrl_line_tri_scan_ex(const float *line, void *ws, size_t ws_bytes, int B, int N, int M, int L,
                         int mode, int chunk, const rrl_opts *opts, void *stream);
/* (K2 below with options: the reduce mode decides whether the dense value lists of the tail kernel are written, so the
 * stage calls of ONE evaluation must be given the same opts) */
int rrl_line_pair_dist_ex(const float *tri1, const float *tri2, const float *line, void *ws,
                          size_t ws_bytes, int B, int N, int M, int L, int s_m, int s_n, int e_m,
                          int e_n, int pool, const rrl_opts *opts, void *stream);

/* K2: per-line sparse stage (code/loss.py:115-167): for lines whose two hit counts fall in
 * [s_m,e_m) x [s_n,e_n): hits sorted ascending (nonzero() order), weights w = d / sum d
 * (loss.py:92), intersection points q = mean_k w_k P_k (loss.py:155-163),
 * D[a][b] = |q1_a - q2_b|^2 (loss.py:165-166), and the D values appended to VALS. */
int rrl_line_pair_dist(const float *tri1, const float *tri2, const float *line, void *ws,
                       size_t ws_bytes, int B, int N, int M, int L, int s_m, int s_n, int e_m,
                       int e_n, int pool, void *stream);

/* K3+K4: lower median (torch.median: sorted[(n-1)/2], loss.py:223-224), Welsch weighting
 * 1 - exp(-(D/med)/2) with symmetric min/mean per bucket (loss.py:20-21, 226-229), bucket
 * weights exp(-|k-j|/2) and the final division by the number of non-empty buckets
 * (loss.py:215-217, 230).  One workgroup per sample; bucket sums in 2^-40 fixed point, so
 * the result does not depend on summation order. */
int rrl_loss_reduce(void *ws, size_t ws_bytes, float *loss, int B, int N, int M, int L, int s_m,
                    int s_n, int e_m, int e_n, int pool, void *stream);

int rrl_loss_reduce_ex(void *ws, size_t ws_bytes, float *loss, int B, int N, int M, int L, int s_m,
                       int s_n, int e_m, int e_n, int pool, const rrl_opts *opts, void *stream);

/* K3 + K4 over caller-supplied rows: rows16 [nrows][16] = canonical 4 x 4 D tiles (+inf outside the k x j block) and
 * kj [nrows] = k | j << 4, i.e. what rrl_line_pair_dist leaves at its compact slots (fields VALS, KJC, BLKCNT) -- the merge
 * step of the line-sharded single-sample mode ("within one sample, lines could also be sharded ... one all-gather
 * of <= 16 S D values"; rrl_hip/dist.py line_sharded_loss): every rank evaluates its share of the lines up to the per-line
 * stage, the rows of all ranks are gathered and reduced here.  Outputs as the fields MED [1], BCNT [16], BSUM [32], INFO [4]
 * (INFO[3] = status[0]) and loss [1]: point them at a rank's own workspace fields and its backward entries use the merged
 * statistics.  blkcnt_scratch: int32 [ceil(nrows / 1024) + 1] device scratch.  Bit-identical to the unsharded loss. */
int rrl_loss_reduce_rows(const float *rows16, const uint8_t *kj, int nrows, int32_t *blkcnt_scratch, float *loss,
                         float *med, int32_t *bcnt, int64_t *bsum, int32_t *info, const int32_t *status, int s_m,
                         int s_n, int e_m, int e_n, void *stream);

/* Which reduce kernel rrl_loss_reduce (and the fused forwards) launch -- the DEFAULT; a call's rrl_opts.reduce_mode
 * overrides it.  Three kernels, bit-identical median, loss and bucket sums (csrc/rrl_call.hip reduce_kind):
 *   single   one 1024-lane workgroup per sample (always legal; the only one for pool != 0);
 *   xchg     loss_reduce_tiled_kernel: one 256-lane workgroup per 1024-line tile; the median's first radix pass comes as a
 *            histogram from the per-line stage, the tiles exchange the values of the median's bin through the workspace
 *            (two tickets, bounded spins; a hand-off that times out is repaired by the sample's last workgroup, see
 *            rrl_set_spin_limit).  Legal while B x tiles <= the number of its workgroups that are co-resident on the
 *            device (compute units x occupancy, queried once per device; 1280 on a whole MI355X);
 *   tail     loss_tail_kernel: no exchange (every workgroup streams its sample's dense D-value lists and selects the
 *            median itself, one ticket, no spin), and the direct / scatter backward can ride in the same launch.
 *            Legal for <= 32 tiles per sample and B x tiles <= 256.
 * mode 0 (auto): tail where a backward rides along (rrl_registration_step, rrl_loss_step), the sample has 2 .. 32 tiles
 *   and B x tiles <= 256; else xchg for >= 2 tiles within its capacity; else single.  A forward alone never takes the
 *   tail kernel in auto mode (as a reduce alone it is within +-1 % of xchg: the per-line stage then writes the value lists).  A single tile of lines (L <= 1024) is
 *   finished by one workgroup per sample together with the per-line stage (and the direct backward).
 * mode 1: single everywhere.  mode 2 ("tiled"): tail wherever it is legal (also forward only, also one tile), xchg
 * beyond, else single.  mode 3 ("xchg"): xchg wherever it is legal (also one tile), else single.
 * Env RRL_REDUCE=single|tiled|xchg sets the initial default. */
int rrl_set_reduce_mode(int mode);

/* Workgroups per cloud of the cell sort + sphere-tree kernel (they share nothing but their input: each owns a range
 * of supergroups): 0 = default (one: more measured no faster, csrc/rrl_cull.hip sort_parts), k = 1..16 forced.  Any value gives the same labels, loss and Chamfer
 * keys; the order of records INSIDE a grid cell may differ.  Env RRL_SORT_PARTS sets the initial state. */
int rrl_set_sort_parts(int parts);

/* Test hooks of the in-launch hand-offs.  rrl_set_spin_limit: polls a waiting workgroup of the exchange reduce makes
 * before it gives up (default 2^18, a fraction of a second; env RRL_SPIN_LIMIT).  A hand-off that times out -- its
 * partners were not co-resident in time: a partitioned device, a CU mask, another process holding the slots -- is
 * REPAIRED inside the same launch by the sample's last workgroup (bit-identical result; STATUS[2] counts the repaired
 * samples); 0 makes every hand-off time out, which is how the tests drive that path.  rrl_debug_occupy: a filler launch
 * of `workgroups` x `lanes` threads that hold their compute-unit slots until the 100 MHz wall clock has advanced by
 * `ticks` (contention tests: a second stream / process that leaves the library only part of the device). */
int rrl_set_spin_limit(long long polls);
int rrl_debug_occupy(int workgroups, int lanes, long long ticks, void *stream);

/* Tuning/testing knobs.  rrl_set_scan_variant: lines per lane of the scan (1 = scalar fp32,
 * 2 / 4 / 8 = one / two / four packed v_pk_*_f32 pairs); 0 = default.  All variants give
 * identical results.  Env RRL_SCAN_VARIANT / RRL_SCAN_CHUNK override the defaults. */
int rrl_set_scan_variant(int lines_per_lane);

/* Profiling hook: enable(k > 0) brackets every k-th scan launch with a hipEvent pair (ring of
 * 1024) recorded on the launch stream; enable(0) turns it off.  collect() synchronises them,
 * writes up to max_n durations in milliseconds and resets the ring.  Returns the number written. */
int rrl_scan_timing_enable(int on);
int rrl_scan_timing_collect(float *ms, int max_n);

/* Profiling hook: executed work of the culled scan.  While dev_counters != NULL every culled scan
 * launches an instrumented instantiation of the same kernel in which every wavefront WRITES one row of 16
 * uint64 (plain stores; row = linear workgroup id x wavefronts per workgroup + wavefront; rows >= `rows`
 * are dropped; the caller clears the buffer and adds the rows up):
 *   [0] level-A sphere tests (line x supergroup)   [1] level-B (line x group)   [2] level-C (line x half)
 *   [3] point-0 prefilter tests (line x record)    [4] candidates resolved exactly (all 3 points)
 *   [5] 1 (the wavefront ran)                      [6] 1 if it took the strict fallback
 *   [7] (line, triangle) pairs evaluated by the fallback   [8], [9] its start / end on the 100 MHz wall clock;
 *   [10..14] phase stamps on the same clock: slice staged, level A done, final drains of levels B / C / D done.
 * NULL switches back to the plain kernel.  bench.py derives the executed flops of a launch from
 * these (12 per sphere test, 11 per prefilter test, 48 per resolved candidate, 48 per fallback pair). */
int rrl_scan_counters(uint64_t *dev_counters, long long rows);

/* Batch-shard payload: out[14] = { sum of valid losses, number of valid
 * samples, sum_b gR[b] (9), sum_b gt[b] (3) } in one launch, fixed summation order; this is
 * the buffer a rank hands to the RCCL all-reduce.  gR / gt may be NULL (zeros). */
int rrl_shard_payload(const float *loss, const void *ws, size_t ws_bytes, const float *gR,
                      const float *gt, float *out, int B, int N, int M, int L, void *stream);

/* ---- rigid apply ----------------------------------------------------------------------- */
/* code/loss.py:460-461; rpm/common/math_torch/se3.py:67-72; code/utils.py:32-37;
 * fmr/se_math/se3.py:110-124.
 *   transpose_r = 0: y = x R + t   (row-vector convention of Reconstruction_point)
 *   transpose_r = 1: y = x R^T + t (= R x + t per point: RPM/DCP/FMR)
 *   channel_first = 0: x,y are [B][n][3];  1: [B][3][n] (DCP)
 * R [B][3][3], t [B][3]. */
int rrl_rigid_apply_fwd(const float *x, const float *R, const float *t, float *y, int B, int n,
                        int transpose_r, int channel_first, void *stream);
/* gx may be NULL.  partial [B][nblk][12] scratch, nblk = rrl_rigid_bwd_blocks(n);
 * gR [B][3][3], gt [B][3] are overwritten (deterministic two-stage reduction). */
int rrl_rigid_bwd_blocks(int n);
int rrl_rigid_apply_bwd(const float *x, const float *R, const float *gy, float *gx, float *gR,
                        float *gt, float *partial, int B, int n, int transpose_r,
                        int channel_first, void *stream);

/* ---- pose kernels of the single-pair demo ------------------------------------------------- */
/* code/loss.py:437-463 (Reconstruction_point.Transform), code/LieAlgebra/se3.py:83-106 (exp3),
 * sinc.py:5-17, 91-103, 120-132.  xi [B][6] = (w, v) -> R [B][3][3] (row-major), T [B][3].
 * rrl_se3_exp_bwd: gxi [B][6] = d<gR, R> + d<gT, T> / dxi (gR or gT may be NULL = zero). */
int rrl_se3_exp(const float *xi, float *R, float *T, int B, void *stream);
int rrl_se3_exp_bwd(const float *xi, const float *gR, const float *gT, float *gxi, int B, void *stream);
/* torch.optim.Adam's step (test_demo_optimized_Lie_Algebra.py:42, 64-66) on p [n] with device-side
 * scalars: state[0] = step count (float), lr[0]; b1, b2, eps are DOUBLES like the Python floats torch.optim.Adam
 * holds (its bias corrections are double arithmetic; in fp32 1 - 0.999^t is 3e-5 off at small t); the update is
 * skipped when gate != NULL and gate[0] <= 0 (the demo's `if loss_di is not None`; gate = INFO[0] of the loss). */
int rrl_adam_gated(float *p, const float *g, float *m, float *v, float *state, const float *lr,
                   const int32_t *gate, int n, double b1, double b2, double eps, void *stream);

/* One row of the demo's per-epoch log (code/test_demo_optimized_Lie_Algebra.py:72-82 prints / logs
 * loss and Chamfer) written on the device, so a captured step needs no host read-back:
 * table[cursor[0]][0..2] = (loss[0], value[0], info[0] > 0 ? 1 : 0), cursor[0] += 1; rows outside
 * [0, nrows) are dropped; row (3 floats, may be NULL) receives a copy. */
int rrl_log_row(const float *loss, const float *value, const int32_t *info, float *table,
                long long *cursor, long long nrows, float *row, void *stream);

/* The pose side of one epoch of the demo loop (code/test_demo_optimized_Lie_Algebra.py:55-82: backward through
 * model.Transform(), optimizer.step(), the next epoch's Transform(), the printed/logged scalars) for ONE pose in one
 * launch: gxi = d/dxi <gR, R(xi)> + <gT, T(xi)> (rrl_se3_exp_bwd), the gated Adam step on xi (rrl_adam_gated),
 * (R, T) = exp(updated xi) (rrl_se3_exp) and, when table and cursor are given, the log row (rrl_log_row with
 * info = gate).  Bit-identical to the four calls.  gxi, loss, value, table, cursor, row may be NULL.
 * box (6 floats, optional): min xyz, max xyz over aabb_rows [n_aabb_rows][8] -- the per-workgroup partial rows (APART
 * field, cloud 1 of sample 0: rows of (min xyz, max xyz, ..)) that the loss step's records launch just wrote for the
 * MOVED source's first points: the next epoch's sampler box (test_demo…:46-51 samples against the previous epoch's moved
 * source) without a rigid-apply + AABB launch of its own. */
int rrl_se3_adam_step(float *xi, const float *gR, const float *gT, float *m, float *v, float *state,
                      const float *lr, const int32_t *gate, double b1, double b2, double eps, float *R, float *T,
                      float *gxi, const float *loss, const float *value, float *table, long long *cursor,
                      long long nrows, float *row, const float *aabb_rows, int n_aabb_rows, float *box, void *stream);

/* rrl_se3_adam_step for a BATCH of B poses in one launch: workgroup b (one wavefront) does for sample b exactly what
 * rrl_se3_adam_step does on that sample's slices -- the same device code, the same bits.  Everything is per sample:
 *   xi, m, v, gxi [B][6]; state, lr, loss, value, cursor [B]; gR, R [B][9]; gT, T [B][3]; row [B][3]; box [B][6];
 *   gate: sample b's word is gate[b * gate_stride] (NULL: every sample steps; stride 4 reads INFO[b][0] of a workspace);
 *   table [nrows][B][3]: sample b writes table[cursor[b]][b] and advances ITS OWN cursor[b] -- no word is read by one
 *     workgroup and written by another within the launch;
 *   box[b] = min xyz, max xyz over the rows aabb_rows + b * row_stride (floats; [..][8]), rows [0, ceil(count1[b] / 256)) --
 *     count1: DEVICE int32 [B], read by the kernel and clamped to [0, N], or NULL: ceil(N / 256) rows.  Rows beyond a
 *     sample's count are never read (a ragged build does not write them); a zero count gives (+inf, -inf) like
 *     rrl_aabb_counted.  With a loss workspace: aabb_rows = the APART field (cloud 1), row_stride = 8 ceil(max(N, M) / 256).
 * gR, gT, gate, gxi, loss, value, table, cursor, row, box (with aabb_rows, count1) may be NULL.  Refusals, before any launch:
 * RRL_E_ARG for B < 0, a NULL required pointer (xi, m, v, state, lr, R, T), a negative gate_stride, and box without rows
 * (aabb_rows NULL, N <= 0, or row_stride < 8 ceil(N / 256)); B == 0 returns 0 without a launch. */
int rrl_se3_adam_step_batch(float *xi, const float *gR, const float *gT, float *m, float *v, float *state, const float *lr,
                            const int32_t *gate, long long gate_stride, double b1, double b2, double eps, float *R, float *T,
                            float *gxi, const float *loss, const float *value, float *table, long long *cursor,
                            long long nrows, float *row, const float *aabb_rows, long long row_stride, const int32_t *count1,
                            int N, float *box, int B, void *stream);

/* One epoch of the single-pair demo (code/test_demo_optimized_Lie_Algebra.py:46-82) as ONE call: line sampler with the
 * library's generator (rrl_sample_lines_rng, against box1 = the previous epoch's moved source) -> fused registration step
 * (rrl_registration_step_ex; pass prepared orders in opts) with the Chamfer walk between the step's own sorted clouds
 * riding in its scan launch (rrl_chamfer_rider; = rrl_chamfer_from_loss: requires the point sets to be the triangles' first
 * points; RRL_DEMO_RIDE=0 in the environment: the separate launch) -> pose step (rrl_se3_adam_step: exp-map backward,
 * gated Adam on xi, (R, T) = exp(updated xi), log row, box1 = the moved source's AABB for the next epoch).  Nothing but
 * the entries' own kernels, 8 launches issued back to back (6 with `pipeline`: the next epoch's sampler passes ride in this
 * epoch's per-line and backward launches): a loop pays one host call per epoch.  One pair
 * (B = 1); every pointer a device pointer as in the four entries; struct_bytes = sizeof(rrl_demo_epoch_args). */
typedef struct rrl_demo_epoch_args {
    int32_t struct_bytes, N, M, L, rounds, transpose_r;
    /* sampler */
    uint64_t *rng_state; const float *radius, *centers; float *box1; const float *box2; float *lines; int32_t *filled, *tile_counts;
    /* loss step: src_tri [N][9], tar_tri [M][9], pose (R [9], T [3]: in / out), workspace of rrl_workspace_bytes(1, N, M, L) */
    const float *src_tri, *tar_tri; float *R, *T; void *ws; size_t ws_bytes; float *loss; const float *grad_loss; float *gR, *gt;
    const rrl_opts *opts;
    /* Chamfer monitor from the loss state: scratch of rrl_chamfer_workspace_bytes(1, N, M) */
    void *cham_ws; size_t cham_ws_bytes; uint64_t *best_x, *best_y; float *cham_value;
    /* pose: xi [6], Adam moments / state / lr on the device, log table [table_rows][3] + cursor, row [3] */
    float *xi, *m, *v, *adam_state; const float *lr; double b1, b2, eps; float *table; long long *cursor; long long table_rows; float *row;
    /* NULL, or one HOST int32 the caller zeroes before the first epoch and then leaves alone: with it the sampler is software-
     * pipelined across epochs -- the COUNT pass of epoch k + 1 (it needs the moved source's box = the partial rows of epoch
     * k's records launch, not box1 from the pose launch) rides in the per-line launch of epoch k, its WRITE pass in the
     * direct-backward launch of epoch k (nothing after the per-line stage reads `lines`); the word remembers what the next
     * call may skip (bit 0: the count pass, bit 1: the write pass too).  radius / centers / box2 / L / rounds must not
     * change while it is non-zero, and `lines` belongs to the library between two calls. */
    int32_t *pipeline;
} rrl_demo_epoch_args;
int rrl_demo_epoch(const rrl_demo_epoch_args *args, void *stream);

/* One epoch of the registration loop for a BATCH of B pairs as ONE call: what rrl_demo_epoch is for one pair, from the
 * batched and ragged entries only, issued back to back on the caller's stream --
 *   1. rrl_sample_lines_rng with B samples against box1 [B][6] (the previous epoch's moved sources) and box2 [B][6];
 *      skipped when rng_state == NULL: `lines` are used as given;
 *   2. the fused registration step (rrl_registration_step_ex) with the caller's opts: prepared orders, count1 / count2 (a
 *      ragged batch), RRL_F_TARGET_KEPT -- the caller switches from its first to its kept options between epochs, as the
 *      demo does.  The chain flags and the Chamfer rider of opts are ignored: no launch here carries another's work;
 *   3. when value != NULL, the monitor: rrl_chamfer_from_loss, then rrl_chamfer_group_means with G = B -> value [B];
 *   4. rrl_se3_adam_step_batch: gate = the workspace's INFO (stride 4), rows = cloud 1 of APART, box output = box1.
 * 7 launches per epoch where the backward rides in the reduce's launch (8 from 512 sampler workgroups on, + 2 with the
 * monitor), for any B.  No host read-back, no environment switch, no pipelining across epochs.  Every pointer a device
 * pointer as in the four entries.
 * Refusals, all before the first launch, in the order of "Refusals" above.  RRL_E_ARG: a NULL or short struct (struct_bytes
 * < sizeof); B, N, M or L <= 0; with rng_state: rounds <= 0 (or > 65535, B > 65535), a NULL radius / centers / box2 /
 * filled / tile_counts, tile_counts not 8-byte aligned; opts->problems or opts->nlines set (one pose per pair; the sampler
 * owns the line set); the monitor together with count1 / count2 -- rrl_chamfer_from_loss must not run on a ragged
 * workspace: call rrl_chamfer_tree_fwd_counted on the first points instead --, with a NULL cham_ws / best_x / best_y /
 * cham_mean, with clouds beyond rrl_sort_capacity() or B > 32767; a NULL xi / m / v / adam_state / lr / box1; and whatever
 * rrl_registration_step_ex refuses.  Then RRL_E_RANGE (never: the range is 1..4), then RRL_E_WS: a short ws or cham_ws. */
typedef struct rrl_register_epoch_args {
    int32_t struct_bytes, B, N, M, L, rounds, transpose_r, reserved;
    /* sampler: rng_state (NULL: keep `lines`), radius [B], centers [B][3], box1 [B][6] (in / out), box2 [B][6],
     * lines [B][L][6], filled [B], tile_counts int32 [B * rounds * ceil(L / 1024) * 32] (8-byte aligned) */
    uint64_t *rng_state; const float *radius, *centers; float *box1; const float *box2; float *lines; int32_t *filled, *tile_counts;
    /* loss step: src_tri [B][N][9], tar_tri [B][M][9], poses (R [B][9], T [B][3]: in / out), workspace of
     * rrl_workspace_bytes(B, N, M, L), loss [B], grad_loss [B], gR [B][9], gt [B][3] (ideally the workspace's GACC field) */
    const float *src_tri, *tar_tri; float *R, *T; void *ws; size_t ws_bytes; float *loss; const float *grad_loss; float *gR, *gt;
    const rrl_opts *opts;
    /* monitor (value == NULL: none): scratch of rrl_chamfer_workspace_bytes(B, N, M), keys [B][N], [B][M], the pooled
     * mean [1] and value [B] = each pair's own Chamfer distance (moved first points against the target's) */
    void *cham_ws; size_t cham_ws_bytes; uint64_t *best_x, *best_y; float *cham_mean, *value;
    /* poses: xi, m, v [B][6], adam_state, lr [B], gxi [B][6] or NULL, log table [table_rows][B][3] + cursor [B], row [B][3] */
    float *xi, *m, *v, *adam_state; const float *lr; double b1, b2, eps; float *gxi; float *table; long long *cursor;
    long long table_rows; float *row;
} rrl_register_epoch_args;
int rrl_register_epoch(const rrl_register_epoch_args *args, void *stream);

/* ---- Gauss-Newton pose steps from the loss's own pairs ---------------------------------
 * With its weights frozen for one step the loss is a weighted point-to-point problem: every selected (line, source hit h,
 * target hit o) that carries gradient in the backward is a pair of points Q1, Q2 of the workspace with the weight
 * a = dL/dD (the backward's gD at upstream gradient 1; weights, median and labels carry no gradient), and
 * Q1 = sum_k (w_k / 3)(x_k R + T) is affine in the pose.  Poses move ROW vectors, y = x R + T (transpose_r = 0).  A step is a
 * world-frame twist (omega, v): y' = y Rot(omega)^T + v with Rot(omega) = exp([omega]x), i.e. R <- R Rot^T, T <- T Rot^T + v.
 * With Q = Q1, e = Q1 - Q2 and s = (w_0 + w_1 + w_2) / 3 of hit h the residual moves by de = omega x Q + s v, and the
 * Gauss-Newton normal equations H (omega, v) = -g are made of sixteen sums per pair of clouds, neq[b][16]:
 *   [0..5]  S_QQ = sum 2a Q Q^T  (xx, xy, xz, yy, yz, zz)      H_ww = tr(S_QQ) I - S_QQ
 *   [6..8]  S_sQ = sum 2a s Q                                   H_wv = [S_sQ]x = -H_vw
 *   [9]     S_ss = sum 2a s^2                                   H_vv = S_ss I
 *   [10..12] g_w = sum 2a Q x e,   [13..15] g_v = sum 2a s e   (g_v = dL/dT; g_w = vee(A - A^T) + T x dL/dT, A = R^T dL/dR)
 * One step of it is one IRLS step of a Welsch-weighted point-to-point fit.
 *
 * rrl_pose_normal_eq: the sixteen sums of every sample from the workspace of ANY registration forward (or step) that ran
 * before it on `ws` with the same B, N, M, L -- scan mode cull or strict, prepared or cold, uniform or ragged: it reads the
 * per-line stage's and the reduce's fields KJ, W1, Q1, Q2, D, MED, BCNT, INFO and nothing of a cloud, a line or a count (an
 * absent line has hit count 0, hence KJ = 0).  A chained step's workspace (RRL_F_CHAIN) keeps these fields too; what such a
 * step clears (COUNT1 / COUNT2, the CHAIN words) is not read here.  Deterministic: the lines of a 1024-line tile go to sixteen
 * workgroups in a fixed order (by rank among the tile's KJ bytes, like the deterministic direct backward), every workgroup
 * stores its sixteen partial sums -- float32 terms accumulated in double -- into `part`, and a second small launch adds them
 * in index order and rounds to float32 once: the same bits on every run.  A sample without a populated bucket
 * (INFO[b][0] == 0) gets sixteen zeros.  part: scratch of rrl_pose_normal_eq_part_bytes(B, L) bytes, 8-byte aligned.
 * opts: NULL, or the forward's options (only `problems` is looked at).
 * Refusals, before any launch: RRL_E_ARG -- a NULL ws / neq / part, B, N, M or L <= 0, B > 65535, L >= 2^24, a misaligned
 * part, a bucket range outside 1..RRL_MAX_HITS hits (s < 1, e > 5: the wide path is not served) or empty, multi-pose
 * `problems` (0 < problems < B) --, then RRL_E_WS: ws_bytes < rrl_workspace_bytes(B, N, M, L) or a short part. */
#define RRL_NEQ_SUMS 16
size_t rrl_pose_normal_eq_part_bytes(int B, int L);
int rrl_pose_normal_eq(const void *ws, size_t ws_bytes, int B, int N, int M, int L, int s_m, int s_n, int e_m, int e_n,
                       float *neq, void *part, size_t part_bytes, const rrl_opts *opts, void *stream);

/* The pose-step state: what the pose steps that stop by themselves (rrl_se3_newton_step_batch, rrl_icp_step_batch) keep per
 * pose, and the one rule both apply.  state [B][4] int32 = { epochs issued, calm epochs, done epoch or -1 (the caller writes
 * -1 before the first call), the pose-step status of this call }.  Every call adds 1 to word 0.  The stopping rule, when
 * patience > 0: word 1 counts the consecutive epochs whose APPLIED step had its rotation length < tol_rot[b] and its
 * translation length < tol_trans[b] (float32 comparisons; any other epoch -- skipped, failed, longer -- resets it); when it
 * reaches `patience`, word 2 = the number of epochs issued so far, this one included.  From then on the pair is done: its pose
 * is frozen, bit for bit, words 1 and 2 are kept and word 3 says RRL_POSE_DONE.  last_step [B][2] (optional) = the two
 * lengths, written only when a step was applied.  Word 3: 0 the step was applied, 1 skipped and 2 failed (the pose keeps its
 * bits; each step names its own reasons: RRL_NEWTON_*, RRL_FIT_*), 3 done. */
#define RRL_POSE_STEPPED 0
#define RRL_POSE_SKIPPED 1
#define RRL_POSE_FAILED 2
#define RRL_POSE_DONE 3

/* One damped Gauss-Newton step for a BATCH of B poses in one launch (one wavefront per pose, like rrl_se3_adam_step_batch;
 * every array per sample: neq [B][16]; damping, step, max_rot, max_trans, tol_rot, tol_trans [B]; R [B][9], T [B][3];
 * loss, value, cursor [B]; table [nrows][B][3]; row [B][3]; box [B][6]; delta [B][6]; last_step [B][2]; state [B][4] int32).
 * Sample b:
 *   1. H (6 x 6), g from neq[b];
 *   2. skipped (RRL_NEWTON_GATED) when its gate word gate[b * gate_stride] <= 0 (NULL: open; a workspace's INFO, stride 4),
 *      or when the pair is done (RRL_NEWTON_DONE, see 9): the pose keeps its bits;
 *   3. (H + damping[b] diag(H) + eps I) x = -g by Cholesky in double.  A pivot that does not exceed eps -- the matrix without
 *      the eps term contributes nothing positive there: a singular H, all-zero sums -- or is not finite (a NaN sum), or a
 *      non-finite solution or pose, leaves the pose unchanged: RRL_NEWTON_FAILED.  delta[b] = x as float32 (optional);
 *   4. (omega, v) = step[b] x, then |omega| <= max_rot[b] and |v| <= max_trans[b] by scaling;
 *   5. R[b] <- R[b] Rot(omega)^T, T[b] <- T[b] Rot(omega)^T + v with the exact Rodrigues rotation in double, then one
 *      Gram-Schmidt pass over the rows of R, then rounded to float32;
 *   6. last_step[b] = (|omega|, |v|) as applied (optional; written only when the sample stepped; a clamped norm IS the clamp);
 *   7. the log row (loss[b], value[b], gate word > 0) into table[cursor[b]][b] and row[b], cursor[b] += 1 -- as the Adam step;
 *   8. box[b] = min xyz, max xyz over the rows aabb_rows + b * row_stride, [0, ceil(count1[b] / 256)) of them -- the contract
 *      of rrl_se3_adam_step_batch (count1 NULL: ceil(N / 256) rows; no rows: (+inf, -inf));
 *   9. the stopping rule of the pose-step state (above) on the lengths (|omega|, |v|) of 6.
 * state[b]: the pose-step state, its status word RRL_NEWTON_* of this call.
 * gate, tol_rot, tol_trans (patience <= 0), loss, value, table, cursor, row, box (with aabb_rows, count1),
 * delta, last_step may be NULL.  Refusals, before any launch: RRL_E_ARG for B < 0, a NULL neq / damping / step / max_rot /
 * max_trans / R / T / state, a negative gate_stride, eps < 0 or NaN, patience > 0 without both tolerances, a box without
 * rows (aabb_rows NULL, N <= 0, or row_stride < 8 ceil(N / 256)); B == 0 returns 0 without a launch. */
#define RRL_NEWTON_STEPPED RRL_POSE_STEPPED
#define RRL_NEWTON_GATED RRL_POSE_SKIPPED
#define RRL_NEWTON_FAILED RRL_POSE_FAILED
#define RRL_NEWTON_DONE RRL_POSE_DONE
int rrl_se3_newton_step_batch(const float *neq, const int32_t *gate, long long gate_stride, const float *damping,
                              const float *step, const float *max_rot, const float *max_trans, const float *tol_rot,
                              const float *tol_trans, int patience, double eps, float *R, float *T, const float *loss,
                              const float *value, float *table, long long *cursor, long long nrows, float *row,
                              const float *aabb_rows, long long row_stride, const int32_t *count1, int N, float *box,
                              float *delta, float *last_step, int32_t *state, int B, void *stream);

/* One Gauss-Newton epoch for a BATCH of B pairs as ONE call: rrl_register_epoch with the second-order pose step, issued
 * back to back on the caller's stream --
 *   1. rrl_sample_lines_rng (skipped when rng_state == NULL: `lines` as given);
 *   2. the registration FORWARD (rrl_registration_forward_ex, range 1..4, scan mode cull, y = x R + T) with the caller's
 *      opts: prepared orders, count1 / count2, RRL_F_TARGET_KEPT after the first epoch.  The point backward is not run.  The
 *      chain flags and the Chamfer rider of opts are dropped;
 *   3. when value != NULL, the monitor exactly as rrl_register_epoch runs it (uniform batches only);
 *   4. rrl_pose_normal_eq -> neq [B][16];
 *   5. rrl_se3_newton_step_batch: gate = the workspace's INFO (stride 4), rows = cloud 1 of APART, box output = box1.
 * No host read-back: the epoch can be captured.  Refusals, all before the first launch, RRL_E_ARG first: a NULL or short
 * struct; B, N, M or L <= 0; B > 65535; the sampler's (rounds, pointers, alignment) as rrl_register_epoch; opts->problems or
 * opts->nlines set; the monitor together with count1 / count2, with a NULL cham_ws / best_x / best_y / cham_mean, with clouds
 * beyond rrl_sort_capacity() or B > 32767; a NULL box1 / neq / part / state or whatever the step (above) refuses; whatever
 * rrl_registration_forward_ex refuses.  Then RRL_E_WS: a short ws, cham_ws or part. */
typedef struct rrl_register_newton_args {
    int32_t struct_bytes, B, N, M, L, rounds, patience, reserved;
    /* sampler, as rrl_register_epoch_args */
    uint64_t *rng_state; const float *radius, *centers; float *box1; const float *box2; float *lines; int32_t *filled, *tile_counts;
    /* forward: src_tri [B][N][9], tar_tri [B][M][9], poses (R [B][9], T [B][3]: in / out), workspace of
     * rrl_workspace_bytes(B, N, M, L), loss [B] */
    const float *src_tri, *tar_tri; float *R, *T; void *ws; size_t ws_bytes; float *loss;
    const rrl_opts *opts;
    /* monitor (value == NULL: none), as rrl_register_epoch_args */
    void *cham_ws; size_t cham_ws_bytes; uint64_t *best_x, *best_y; float *cham_mean, *value;
    /* normal equations: neq [B][16], part of rrl_pose_normal_eq_part_bytes(B, L) bytes */
    float *neq; void *part; size_t part_bytes;
    /* step (rrl_se3_newton_step_batch): per-sample controls [B], eps, delta [B][6] or NULL, last_step [B][2] or NULL,
     * state [B][4]; log table [table_rows][B][3] + cursor [B], row [B][3] */
    const float *damping, *step, *max_rot, *max_trans, *tol_rot, *tol_trans; double eps; float *delta, *last_step; int32_t *state;
    float *table; long long *cursor; long long table_rows; float *row;
} rrl_register_newton_args;
int rrl_register_newton_epoch(const rrl_register_newton_args *args, void *stream);

/* ---- Closed-form rigid fits: batched weighted Kabsch, and an ICP epoch around it ----------
 * In the row convention of the registration loops (x -> x R + T) the fit of sample b is
 *   wn_i = w_i / (sum_i w_i + eps_w),   abar = sum wn_i a_i,   bbar = sum wn_i b_i        (RPM's normalisation: eps_w = 1e-5),
 *   H = sum wn_i (a_i - abar)^T (b_i - bbar) = U S V^T,   delta = det(U V^T),   D = diag(1, 1, delta),
 *   R = U D V^T,   T = bbar - abar R:   the minimiser of sum wn_i |a_i R + T - b_i|^2 (eps_w = 0).
 * transpose_r != 0 returns R^T, the matrix that moves COLUMN vectors: rpm/models/rpmnet.py:121-157 rot_mat for
 * cov = a^T (b wn); dcp/model.py:405-455 r for H.
 * Pairs: without keys the partner of a[b][i] is b[b][i] (m == n); with keys [B][n] -- the u64 keys a Chamfer walk left for the
 * rows of a, (squared distance bits << 32 | index) -- it is b[b][key & 0xffffffff].  No key is followed unchecked: a row at
 * or beyond count_a[b], an all-ones key, a key whose index is >= m or >= count_b[b] (without keys: a row >= count_b[b])
 * contributes NOTHING and is counted in info[b][3].  gate_sq [B] (keys only): a pair whose key distance word exceeds
 * gate_sq[b] gets weight 0 (it is neither used nor skipped).  Counts are device int32 [B], clamped to [0, n] / [0, m] by the
 * kernel, never read on the host; rows beyond a count may hold anything (NaN).  a_stride / b_stride: floats per row (>= 3;
 * 9 reads the first points of pseudo-triangles in place).  w [B][n] or NULL (= 1).
 * Arithmetic: every sum is a fixed-order DOUBLE sum -- per-lane accumulators over the float32 inputs (differences to a
 * per-sample pivot, row 0 of each cloud, taken in double, so that a cloud far from the origin loses nothing), the
 * wavefront's DPP tree, four wavefronts, one partial row per 512-row workgroup in `part`, the partials in index order; no
 * atomics.  H, a one-sided Jacobi SVD of it, delta, R and T are double and rounded to float32 once.  Same bits on every call.
 * Launches: partials (grid ceil(n / 512) x B), then one wavefront per sample; ONE launch when n <= 512.  Nothing synchronises.
 * Outputs: R [B][9], T [B][3]; fit [B][32] double (RRL_FIT_*): W = sum w, abar, bbar, U (row-major), S, V, delta, res_after =
 * sum wn |a R + T - b|^2 from the moments in closed form (clamped at 0), key_mean = sum wn (key distance word) (0 without
 * keys), [31] = 0; info [B][4] int32: pairs used, status, 1 when delta = -1 (the reflection was fixed), pairs skipped.
 * Status: RRL_FIT_OK; RRL_FIT_FEW -- fewer than 3 pairs or sum w <= 0 (or NaN): R = I, T = 0, the rest of fit 0;
 * RRL_FIT_DEGENERATE -- (s1 + delta s2) <= rank_tol s0 (collinear or coincident points): R, T and fit are written (U, V
 * completed to orthonormal bases) but the rotation about the line is not determined.
 * Refusals, before any launch: RRL_E_ARG -- a NULL args / a / b / R / T / fit / info / part, B < 0, n <= 0, m <= 0, a stride
 * below 3, no keys and m != n, gate_sq without keys, B > 32767, struct_bytes != sizeof, a misaligned part or fit --, then
 * RRL_E_WS: part_bytes < rrl_kabsch_part_bytes(B, n).  B == 0 returns 0 without a launch. */
#define RRL_FIT_W 0
#define RRL_FIT_ABAR 1
#define RRL_FIT_BBAR 4
#define RRL_FIT_U 7
#define RRL_FIT_S 16
#define RRL_FIT_V 19
#define RRL_FIT_DELTA 28
#define RRL_FIT_RES 29
#define RRL_FIT_KEYMEAN 30
#define RRL_FIT_DOUBLES 32
#define RRL_FIT_OK 0
#define RRL_FIT_FEW 1
#define RRL_FIT_DEGENERATE 2
typedef struct rrl_kabsch_args {
    int32_t struct_bytes, B, n, m, a_stride, b_stride, transpose_r, reserved;
    const float *a, *b, *w; const uint64_t *keys; const int32_t *count_a, *count_b; const float *gate_sq;
    double eps_w; float rank_tol, reserved_f;
    void *part; size_t part_bytes;
    float *R, *T; double *fit; int32_t *info;
} rrl_kabsch_args;
size_t rrl_kabsch_part_bytes(int B, int n);
int rrl_kabsch_fwd(const rrl_kabsch_args *args, void *stream);
/* Backward of the DENSE fit (args->keys == NULL, else RRL_E_ARG), one launch, double up to the final rounding: from the
 * forward's args (a, b, w, counts, strides, eps_w, transpose_r, fit, info as it left them) and the upstream gR [B][9] (of the
 * matrix as returned), gT [B][3] -- either may be NULL (zero) -- into ga [B][n][3], gb [B][n][3], gw [B][n] (each may be NULL;
 * all rows are written).  With Gt = U^T (gR - abar^T gT) V and s' = (s0, s1, delta s2), d = (1, 1, delta):
 *   gH = U Z V^T,  Z_ii = 0,  Z_ij = (Gt_ij - d_i d_j Gt_ji) / (s'_i + s'_j);
 * then the routes through T, the centroids and wn (eps_w included).  The gradient does not exist where s'_i + s'_j = 0: a
 * sample whose forward status is RRL_FIT_FEW or RRL_FIT_DEGENERATE gets ZERO gradient rows -- its forward info says why --,
 * as do the rows beyond a count. */
int rrl_kabsch_bwd(const rrl_kabsch_args *args, const float *gR, const float *gT, float *ga, float *gb, float *gw, void *stream);

/* The pose step of point-to-point ICP for a batch, one launch, one wavefront per pair: from the fit (Rk [B][9], Tk [B][3],
 * info, fit of rrl_kabsch_fwd on the source AS GIVEN, so that (Rk, Tk) is the total pose) and the current pose R [B][9],
 * T [B][3].  state [B][4] int32: the pose-step state (above), its status word the fit's status RRL_FIT_* (the same three
 * values), or RRL_ICP_DONE.  Pair b, unless done, with status RRL_FIT_OK and a finite (Rk, Tk): in double, the rotation angle
 * between R and Rk and the motion of the weighted source centroid |abar Rk + Tk - abar R - T| are the applied step's two
 * lengths (-> last_step, the stopping rule); (R, T) <- (Rk, Tk), bit for bit.
 * Any other status keeps the pose and resets the calm count (a non-finite fit: RRL_FIT_DEGENERATE).
 * The log row (res_after, value[b], status == RRL_FIT_OK) goes to table[cursor[b]][b] and row[b], cursor[b] += 1, as
 * rrl_se3_adam_step_batch logs.  value, table, cursor, row, last_step, tol_rot / tol_trans (patience <= 0) may be NULL.
 * RRL_E_ARG before the launch: B < 0, a NULL Rk / Tk / info / fit / R / T / state, patience > 0 without both tolerances. */
#define RRL_ICP_DONE RRL_POSE_DONE
int rrl_icp_step_batch(const float *Rk, const float *Tk, const int32_t *info, const double *fit, float *R, float *T,
                       const float *tol_rot, const float *tol_trans, int patience, const float *value, float *table,
                       long long *cursor, long long nrows, float *row, float *last_step, int32_t *state, int B, void *stream);

/* One ICP epoch for a batch of B pairs as ONE call: the existing entries back to back on the caller's stream, nothing else --
 *   1. rrl_rigid_apply_fwd: moved = src R + T                                   (src [B][N][3], transpose_r = 0);
 *   2. rrl_chamfer_tree_fwd_counted on (moved, tar, count1, count2) with the prepared orders -> best_x, best_y, values [B];
 *   3. rrl_kabsch_fwd with a = src (as given, NOT moved), keys = best_x, b = tar, the counts, w, gate_sq -> Rk, Tk, fit, info;
 *   4. rrl_icp_step_batch with value = values (the pair's Chamfer distance, which the walk's other half supplies).
 * Fitting the source as given yields the total pose: nothing is composed, nothing drifts.  No host read-back.  Refusals, all
 * before the first launch: RRL_E_ARG -- a NULL or wrongly sized struct, B <= 0 or > 32767, N or M <= 0 or beyond
 * rrl_sort_capacity(), any NULL pointer among src, tar, R, T, moved, cham_ws, best_x, best_y, values, part, Rk, Tk, fit,
 * info, state, exactly one count or one order, patience > 0 without both tolerances, a misaligned part or fit --, then
 * RRL_E_WS: a short cham_ws or part. */
typedef struct rrl_icp_epoch_args {
    int32_t struct_bytes, B, N, M, patience, reserved;
    const float *src, *tar; const int32_t *count1, *count2; float *R, *T, *moved;
    void *cham_ws; size_t cham_ws_bytes; uint64_t *best_x, *best_y; float *values; const int32_t *order_x, *order_y;
    const float *w, *gate_sq; double eps_w; float rank_tol, reserved_f;
    void *part; size_t part_bytes; float *Rk, *Tk; double *fit; int32_t *info;
    const float *tol_rot, *tol_trans; float *last_step; int32_t *state;
    float *table; long long *cursor; long long table_rows; float *row;
} rrl_icp_epoch_args;
int rrl_icp_epoch(const rrl_icp_epoch_args *args, void *stream);

/* ---- Sinkhorn soft assignment: RPM's match head in front of the Kabsch solve ---------------
 * rpm/models/rpmnet.py:48-118 sinkhorn(log_alpha, n_iters, slack) and the lines 214-222 behind it, as a dual-potential
 * iteration.  With A = log_alpha [B][J][K], x = xyz_ref [B][K][3], sigma = 1 with slack (the padded row and column, never
 * normalised themselves) and 0 without, u^0 = v^0 = 0 and for t = 0 .. n_iters - 1
 *   u^{t+1}[j] = log(sum_k exp(A[j][k] - v^t[k]) + sigma),   v^{t+1}[k] = log(sum_j exp(A[j][k] - u^{t+1}[j]) + sigma):
 *   P = exp(A - u^n - v^n) = exp(sinkhorn(A)),   s[j] = sum_k P,   c[k] = sum_j P,   W[j] = sum_k P x[k] / (s[j] + eps).
 * P is never stored; log_perm [B][J][K] (optional) receives A - u^n - v^n, rounded once, in the output pass.
 * Ragged: count_src / count_ref, device int32 [B] or NULL, clamped to [0, J] / [0, K] by the kernels, never read on the
 * host: rows and columns at or beyond them are never read, get s = 0, W = 0, c = 0 (log_perm -inf) and a zero gradient.
 * Arithmetic: potentials, adjoint vectors and every sum are DOUBLE; a matrix term is the exponential of the double
 * double(A) - u - v, evaluated in double to 2^-36, so nothing is rounded to float32 before the results are; logsumexp runs
 * under a running maximum; lanes, wavefronts and the ceil(J / 128) row slices of a column sum are combined in a fixed
 * order, without atomics: the same bits on every call, and sample b of a batch has the bits of a B = 1 call on its own
 * rows and columns.
 * Non-finite entries: -inf is an entry with P = 0 and gradient 0 (without slack, a row or column of nothing but -inf has no
 * normalisation: its outputs are not finite).  A NaN or +inf entry inside the counts sets info[b] = 1 (else 0); the outputs
 * of that sample are then NaN or inf wherever the entry reaches; nothing is indexed by data.
 * Launches (all on `stream`, no host read-back, capturable): forward 3 n_iters + 2 (a memset of info, per iteration a row
 * pass, a column pass and its finish, then the output row pass; c comes out of the last finish; n_iters = 0: 4); backward
 * 3 n_iters + 2 (n_iters = 0: 4).
 * ws: rrl_sinkhorn_workspace_bytes(B, J, K, n_iters) bytes, 8-byte aligned: the potential history, (n_iters + 1) (J + K)
 * doubles per sample, which the backward reads, the same for the adjoints, s and N in double, and the column partials.  The
 * backward takes the forward's args with ws as the forward left it.
 * Refusals, on the host before any HIP call: RRL_E_ARG -- a NULL args / log_alpha / xyz_ref / ws / W / s / c / info (backward:
 * g_log_alpha), struct_bytes != sizeof, B < 1 or > 32767, J or K < 1 or > 16384, n_iters < 0 or > 64, a misaligned ws --,
 * then RRL_E_WS: ws_bytes below the size above (which is 0 for a shape that is refused). */
typedef struct rrl_sinkhorn_args {
    int32_t struct_bytes, B, J, K, n_iters, slack, reserved0, reserved1;
    const float *log_alpha, *xyz_ref; const int32_t *count_src, *count_ref;
    double eps;
    void *ws; size_t ws_bytes;
    float *W, *s, *c, *log_perm; int32_t *info;
} rrl_sinkhorn_args;
size_t rrl_sinkhorn_workspace_bytes(int B, int J, int K, int n_iters);
int rrl_sinkhorn_fwd(const rrl_sinkhorn_args *args, void *stream);
/* Backward: from upstream gW [B][J][3], gs [B][J], gc [B][K] (each may be NULL: zero) into g_log_alpha [B][J][K] (every
 * entry written) and g_xyz_ref [B][K][3] (may be NULL; the route through W only).  With gN = gW / (s + eps),
 * gs' = gs - (gW . W) / (s + eps) and G[j][k] = gs'[j] + gc[k] + gN[j] . x[k] (rank 5, never stored):
 *   gx[k] = sum_j P gN[j],   ubar^n[j] = -sum_k P G,   vbar^n[k] = -sum_j P G;   for t = n - 1 .. 0, with
 *   Q = exp(A - u^{t+1} - v^{t+1}) and S = exp(A - u^{t+1} - v^t):   ubar^{t+1}[j] -= sum_k vbar^{t+1}[k] Q,
 *   vbar^t[k] = -sum_j ubar^{t+1}[j] S (ubar^t starts from 0);   dA = P G + sum_t (vbar^{t+1}[k] Q + ubar^{t+1}[j] S),
 * 2 n matrix-vector passes that leave vectors only, and one assembly pass: one read of A, one write of dA. */
int rrl_sinkhorn_bwd(const rrl_sinkhorn_args *args, const float *gW, const float *gs, const float *gc, float *g_log_alpha,
                     float *g_xyz_ref, void *stream);

/* ---- Chamfer monitor (code/loss.py:38-52, 236-252) -------------------------------------- */
/* best_x [B][N], best_y [B][M] are u64 keys (dist bits << 32 | argmin), set to all-ones by
 * the call itself.  value[0] = mean of all B*(N+M) minima. */
int rrl_chamfer_fwd(const float *x, const float *y, uint64_t *best_x, uint64_t *best_y,
                    float *value, int B, int N, int M, void *stream);
/* The same result (keys bit-identical, value from a fixed-order sum) through the scan's spatial
 * structures: both clouds in grid-cell (Hilbert) order under the sphere tree, nearest neighbours by a
 * pruned tree walk, the mean folded into the same launch (2 launches for N, M <= 4096).  ws: scratch of
 * rrl_chamfer_workspace_bytes(B, N, M) bytes.  N, M in [1, rrl_sort_capacity()].  best_x / best_y need no
 * initialisation.  A NaN coordinate in a target cloud makes every minimum of that sample NaN and a
 * NaN query its own minimum, as torch.min does. */
size_t rrl_chamfer_workspace_bytes(int B, int N, int M);
int rrl_chamfer_tree_fwd(const float *x, const float *y, void *ws, size_t ws_bytes, uint64_t *best_x,
                         uint64_t *best_y, float *value, int B, int N, int M, void *stream);
/* Chamfer between the two clouds of a LOSS EVALUATION without sorting them again: the loss forward
 * (rrl_loss_forward*, rrl_registration_forward*, or rrl_tri_prepare) left the sorted P0 records, their
 * original indices and the sphere trees of both clouds in its workspace, and the first point of every
 * pseudo-triangle is the point of the cloud it was built from (code/loss.py:473-485: row = [P, neighbour,
 * neighbour]); the fused op's source records are the MOVED source.  This replaces the trainers'
 * chamfer_dist(moved source points, target points) next to the loss (rpm/Train_RPM.py:223-224) when the
 * point sets ARE the triangles' first points: keys and value equal rrl_chamfer_fwd on (P0 of cloud 1,
 * P0 of cloud 2).  ws_src: the evaluation's workspace; ws_tar: the workspace holding cloud 2's records
 * (the same one, or the target_ws the evaluation was carried over from); both of layout (B, N, M, L).
 * ws: scratch of rrl_chamfer_workspace_bytes(B, N, M).  N, M <= rrl_sort_capacity() (larger clouds are not sorted).
 * ONE launch (round 3: the mean is finished by the last workgroups to arrive; their counters are words of ws_src's MCTL
 * field, which is why ws_src is not const).  A non-finite (or overflowing) coordinate anywhere in a cloud gives NaN minima. */
int rrl_chamfer_from_loss(void *ws_src, const void *ws_tar, size_t loss_ws_bytes, int B, int N, int M,
                          int L, void *ws, size_t ws_bytes, uint64_t *best_x, uint64_t *best_y, float *value,
                          void *stream);
/* Profiling hook like rrl_scan_counters: while dev_counters != NULL rrl_chamfer_tree_fwd runs an
 * instrumented instantiation that WRITES one row of 16 uint64 per wavefront of the walk (row index =
 * workgroup * wavefronts per workgroup + wavefront; a full table has 8 * 2 B * ceil(max(N,M)/64) rows; rows >= `rows`
 * are dropped; cleared by the caller): [0] patch-level leaf tests, [1] per-lane leaf tests, [2] (query, leaf)
 * entries evaluated, [3] (query, target) pairs evaluated, [4] 1, [5..7] / [9..14] shader clocks of the phases. */
int rrl_chamfer_counters(uint64_t *dev_counters, long long rows);
/* values[g] = the Chamfer mean (code/loss.py:249-252) over samples [g B / G, (g + 1) B / G) of the evaluation whose walk
 * (rrl_chamfer_from_loss / _ex, or the rider of an `_ex` forward) ran on the Chamfer workspace cham_ws -- the monitor per
 * ITERATION of a multi-pose evaluation (rrl_opts.problems: group g = pose g of every problem; rpm/Train_RPM.py:223-224 logs
 * the distance of every iteration's moved source).  From the per-(sample, direction) sums the walk left in cham_ws. */
int rrl_chamfer_group_means(const void *cham_ws, size_t cham_ws_bytes, float *values, int G, int B, int N, int M,
                            void *stream);
/* The two tree-walk entries with the counter table given PER CALL (NULL: the plain kernel) instead of through the
 * process-wide hook above: two threads / streams can profile independently.  rrl_chamfer_tree_fwd_ex also takes
 * PREPARED clouds: order_x [B][64 ceil(N/64)], order_y [B][64 ceil(M/64)] from rrl_cloud_order on the same clouds in any
 * rigid pose (point clouds: call it on (B, n, 9) rows whose first three floats are the points, or on the pseudo-
 * triangles they are the first points of) -- both given, the per-call sort is replaced by one wide launch that writes
 * the records at their sorted positions and refits the sphere tree; keys and value are the same bits (any permutation
 * gives the same minima and first-occurrence argmins). */
int rrl_chamfer_tree_fwd_ex(const float *x, const float *y, void *ws, size_t ws_bytes, uint64_t *best_x,
                            uint64_t *best_y, float *value, int B, int N, int M, const int32_t *order_x,
                            const int32_t *order_y, uint64_t *counters, long long counter_rows, void *stream);
int rrl_chamfer_from_loss_ex(void *ws_src, const void *ws_tar, size_t loss_ws_bytes, int B, int N, int M,
                             int L, void *ws, size_t ws_bytes, uint64_t *best_x, uint64_t *best_y, float *value,
                             uint64_t *counters, long long counter_rows, void *stream);
/* Backward of either forward from the keys it left: gx [B][N][3], gy [B][M][3] are ACCUMULATED into (zero them first);
 * either may be NULL.  Like the forwards it refuses an empty cloud (N == 0 or M == 0 with B > 0: RRL_E_ARG, no launch). */
int rrl_chamfer_bwd(const float *x, const float *y, const uint64_t *best_x,
                    const uint64_t *best_y, const float *grad_value, float *gx, float *gy, int B,
                    int N, int M, void *stream);
/* RAGGED batches: the Chamfer distance of B pairs whose clouds differ in size, in ONE call (DESIGN.md "Ragged batches").
 * x [B][N][3], y [B][M][3]: N, M are capacities and strides; count_x, count_y: DEVICE int32 [B], clamped by the kernels to
 * [0, N] / [0, M] and never read on the host (no synchronisation; the call can be captured in a graph).  Sample b is the
 * pair x[b][0 .. cx_b), y[b][0 .. cy_b).
 *   absent rows  (beyond a count) are never interpreted: no nearest neighbour, no query, no NaN source, no tree node, no
 *                term of any sum; their key rows best_x[b][cx_b ..], best_y[b][cy_b ..] are written as all-ones by the call.
 *   present rows hold the keys of the uniform entries (distance bits << 32 | original index, first occurrence on ties):
 *                bit-identical to the B = 1 call on the truncated clouds.
 *   values [B]   values[b] = (sum of the sample's cx_b + cy_b minima) / (cx_b + cy_b): chamfer_dist of that pair alone.
 *   value [1]    (may be NULL) the sum of ALL present minima / sum_b (cx_b + cy_b): the mean over the concatenated lists.
 *   empty clouds a sample with cx_b = 0 or cy_b = 0 has no minima: values[b] = 0, all-ones keys, and it is left out of
 *                value's numerator and denominator; if no sample counts, value = 0.
 *   NaN          per sample and over present rows only: a NaN among the present TARGET points makes that direction's
 *                minima NaN, a NaN query its own minimum; a NaN beyond a count is invisible.
 * The sums are the fixed-order double sums of the uniform walk; the denominators are computed on the device by the
 * wavefront that finishes the mean.  count_x == count_y == NULL: the counts are the capacities (keys and value are the bits
 * of rrl_chamfer_tree_fwd, plus values).  order_x / order_y: both or neither; the layout of rrl_cloud_order_counted
 * ([B][64 ceil(N / 64)], the first count[b] entries of a row a permutation of [0, count[b])); same bits as without.
 * ws: rrl_chamfer_workspace_bytes(B, N, M).
 * Who reads which count, and where a workgroup leaves: the records kernels and the sorts take a sample's rows from its own
 * count (workgroups past them leave after the clearing of the histogram / the arrival counters, before their first load;
 * pads sort last, tree nodes only for supergroups [0, ceil(count / 64))); the walk reads both counts of its sample -- two
 * scalar loads --, a patch at or beyond ceil(count / 64) writes its all-ones keys and takes the ticket path with a sum of
 * +0.0 (the grid and the arrival counts stay those of the capacities).
 * Refusals, on the host and before any launch, in this order: RRL_E_ARG -- a NULL required pointer (x, y, ws, best_x,
 * best_y, values), exactly one count pointer NULL, exactly one order given, B <= 0 or a negative size, N == 0 or M == 0,
 * B > 32767, max(N, M) > the sort capacity (there is no counted brute-force kernel) --, then RRL_E_WS (a short workspace). */
int rrl_chamfer_tree_fwd_counted(const float *x, const float *y, const int32_t *count_x, const int32_t *count_y, void *ws,
                                 size_t ws_bytes, uint64_t *best_x, uint64_t *best_y, float *values, float *value, int B,
                                 int N, int M, const int32_t *order_x, const int32_t *order_y, void *stream);
/* Its backward, from the keys it left: accumulates into gx [B][N][3], gy [B][M][3] like rrl_chamfer_bwd (zero them first;
 * either may be NULL).  grad_values [B]: the upstream gradient of values; sample b's minima are scaled by
 * 2 grad_values[b] / (cx_b + cy_b).  (For the scalar value with upstream g: grad_values[b] = g (cx_b + cy_b) / sum.)  The
 * threads of absent rows and of samples with an empty cloud do nothing: those gradient rows stay as they were (zero).
 * RRL_E_ARG as the forward (required: x, y, best_x, best_y, grad_values); B == 0 is a no-op. */
int rrl_chamfer_bwd_counted(const float *x, const float *y, const uint64_t *best_x, const uint64_t *best_y,
                            const float *grad_values, const int32_t *count_x, const int32_t *count_y, float *gx, float *gy,
                            int B, int N, int M, void *stream);

/* ---- dense (line x triangle) tables of code/loss.py:68-112 ------------------------------- */
/* What cal_intersection_batch2_points_with_line returns besides the expanded view of its input:
 * norm_d [B*L][N][3] = d_k / ((d_0 + d_1) + d_2), label [B][L][N] (0/1 bytes), status[0] |= 1 on
 * a NaN distance.  The loss path never materialises these; provided for callers of that public
 * function.  L, B <= 65535. */
int rrl_dense_scan(const float *tri, const float *line, float *norm_d, uint8_t *label,
                   int32_t *status, int B, int N, int L, void *stream);

/* ---- line sampler (code/loss.py:265-432) ------------------------------------------------- */
/* rrl_aabb: per-sample min/max -> aabb [B][6] = min xyz, max xyz (loss.py:325-351).
 * rrl_sample_lines: all `rounds` rejection rounds in two wide launches, slot order == the
 *   reference's candidate order.
 *   rands [rounds][4][B][n] uniform [0,1) draws in the reference's stream order
 *   r [B], centers [B][3], aabb1/aabb2 [B][6] (both NULL: keep every candidate, loss.py:384-412)
 *   lines [B][n][6] (unfilled rows zeroed by the call), filled [B] = accepted (may exceed n)
 *   tile_counts: scratch, 8-byte aligned, int32 [B * rounds * ceil(n/1024) * 32] (one 64-bit accept
 *     ballot per wavefront of every tile of 1024 candidates) */
int rrl_aabb(const float *v, float *aabb, int B, int n, void *stream);
/* ... over the first counts[b] points of sample b only (device int32 [B], clamped to [0, n]; n = capacity and stride):
 * min / max are exact, so the box equals the one of a B = 1 call on the truncated cloud; a zero count gives (+inf, -inf).
 * counts == NULL: every point. */
int rrl_aabb_counted(const float *v, const int32_t *counts, float *aabb, int B, int n, void *stream);
/* y = x R + t (rrl_rigid_apply_fwd, row layout) and aabb [B][6] of y (rrl_aabb) in one launch, one workgroup per
 * sample: for loops whose clouds are small enough that either is launch latency (the demo's epoch). */
int rrl_rigid_apply_aabb(const float *x, const float *R, const float *t, float *y, float *aabb, int B, int n,
                         int transpose_r, void *stream);
/* The resampler's accept test on caller-supplied lines (code/loss.py:265-322, 415-432: label1 * label2):
 * lines [B][n][6], aabb1/aabb2 [B][6] -> mask [B][n] (bit 0: the line crosses >= 1 of the 12 triangles
 * of box 1 by the reference's sub-area test; bit 1: same for box 2 -- accepted == both; bit 2: the
 * sampler's conservative slab pre-test passes) and, when hits != NULL, hits [B][n][2] = the number of
 * box triangles crossed (the reference's label1, label2).  Same device code as rrl_sample_lines. */
int rrl_box_accept(const float *lines, const float *aabb1, const float *aabb2, uint8_t *mask,
                   int32_t *hits, int B, int n, void *stream);
int rrl_sample_lines(const float *rands, const float *r, const float *centers, const float *aabb1,
                     const float *aabb2, float *lines, int32_t *filled, int32_t *tile_counts, int B,
                     int n, int rounds, void *stream);
/* The same with the uniforms drawn INSIDE the kernels by the library's counter-based generator (Philox4x32-10) instead
 * of read from `rands` -- the GPU-side stream for training loops and captured steps (same distribution as torch.rand:
 * 24-bit uniforms in [0, 1); a different stream from both torch generators).  rng_state: 4 uint64 on the device,
 * [0] seed, [1] call counter (every call draws a fresh block and advances it), [2] internal ticket (zero), [3] unused.
 * A captured graph replays correctly: the counter lives on the device. */
int rrl_sample_lines_rng(uint64_t *rng_state, const float *r, const float *centers, const float *aabb1,
                         const float *aabb2, float *lines, int32_t *filled, int32_t *tile_counts, int B,
                         int n, int rounds, void *stream);

/* ---- pseudo-triangle builder (code/loss.py:473-485 + code/utils.py:275-296) --------------- */
/* Farthest-point sampling of S <= n points per cloud, starting at start[b] (the reference draws it
 * with torch.randint; 0 <= start[b] < n is the caller's to guarantee): out_idx [B][S] in selection order.  pts [B][n][3];
 * dist_scratch [B][n].  Distances start at 1e10 like the reference's, so squared distances above it tie; ties go to the
 * lower index; once every distance is 0 the remaining samples are index 0. */
int rrl_fps(const float *pts, const int32_t *start, int32_t *out_idx, float *dist_scratch, int B,
            int n, int S, void *stream);
/* 3 nearest neighbours of the points query_idx [B][S] among ALL n points of their cloud (the query itself and its
 * duplicates included): nn [B][S][3], ascending distance, the lowest index among equals (sklearn KDTree.query, k=3) --
 * a query comes first unless a duplicate of it has a lower index.  n >= 3 and 0 <= query_idx < n are the caller's to
 * guarantee (rrl_hip.neighbors checks both on the host). */
int rrl_knn3(const float *pts, const int32_t *query_idx, int32_t *nn, int B, int n, int S,
             void *stream);

/* ---- pseudo-triangles on the device: batched, ragged, tree 3-NN ---------------------------------
 * What a trainer that augments per step needs: triangles, their counts and (rrl_cloud_order_counted) their orders for a
 * whole batch, built on the device every step.  Plain device pointers, sizes and a stream; nothing is allocated, nothing
 * synchronises, every refusal happens on the host before the first launch (RRL_E_ARG: a NULL pointer that is not marked
 * optional, B < 0, n <= 0, S < 0, S > n where stated, n > rrl_sort_capacity() for the tree; RRL_E_WS: a short scratch).
 * counts [B] (device int32, or NULL = n everywhere): sample b has n_b = clamp(counts[b], 0, n) points, the first n_b rows
 * of pts[b]; the rows beyond are never read (they may hold NaN).  n stays the stride of every array.
 *
 * rrl_fps_counted: sample b emits S_b = min(S, n_b) indices, exactly the sequence rrl_fps gives on pts[b, :n_b] with the
 * same start (NULL counts: rrl_fps's bits); out_idx [B][S], the entries beyond S_b are 0.  start[b] is clamped into
 * [0, n_b) for memory safety only.  out_counts (optional) [B]: S_b.  dist_scratch [B][n].  S <= n. */
int rrl_fps_counted(const float *pts, const int32_t *counts, const int32_t *start, int32_t *out_idx, int32_t *out_counts,
                    float *dist_scratch, int B, int n, int S, void *stream);
/* rrl_knn3_counted: rrl_knn3's brute-force loop for given queries -- the FPS-subsample case, S << n.  query_idx [B][S]
 * (NULL: query q is point q; then S <= n), qcounts [B] (NULL: S): sample b has S_b = clamp(qcounts[b], 0, S) queries
 * among its n_b points; query indices are clamped into [0, n_b).  A sample of fewer than three points has no neighbours:
 * S_b = 0.  nn [B][S][3] as rrl_knn3 writes it, rows beyond S_b zero.  Optional outputs: tri [B][S][9] = the rows
 * pts[nn0], pts[nn1], pts[nn2] (= [p, nn1, nn2] of code/loss.py:473-485; rows beyond S_b zero) and tri_counts [B] = S_b,
 * which feeds rrl_opts.count1 / count2 directly. */
int rrl_knn3_counted(const float *pts, const int32_t *counts, const int32_t *query_idx, const int32_t *qcounts, int32_t *nn,
                     float *tri, int32_t *tri_counts, int B, int n, int S, void *stream);
/* rrl_knn3_self: the three nearest neighbours of EVERY point of its cloud, nn [B][n][3] in the original row order with
 * original indices, bit-equal to rrl_knn3 with query q = point q on every finite cloud -- through the sorted layout
 * (16^3-cell Hilbert sort, supergroups of 64 records, sphere tree) and a pruned walk instead of n^2 distances
 * (csrc/rrl_knn_tree.hip holds the bound's derivation).  A sample with a NaN, an infinite or a huge (|P| > 1e15)
 * coordinate within its count is served by the brute-force loop inside the same launch, with rrl_knn3's result.  Rows
 * beyond n_b, and every row of a sample with n_b < 3, are zero.  Optional outputs: tri [B][n][9] and tri_counts [B]
 * (n_b, or 0 when n_b < 3) as above.  ws: scratch of rrl_knn3_self_workspace_bytes(B, n) bytes.
 * n <= rrl_sort_capacity(), B <= 32767.  3 launches up to 4096 points, 5 beyond. */
size_t rrl_knn3_self_workspace_bytes(int B, int n);
int rrl_knn3_self(const float *pts, const int32_t *counts, void *ws, size_t ws_bytes, int32_t *nn, float *tri,
                  int32_t *tri_counts, int B, int n, void *stream);

/* ---- ball-query grouping and raw point-pair features ----------------------
 * RPM-Net's feature extractor groups every point with "the first nsample in-radius indices, in index order"
 * (rpm/models/pointnet_util.py:96-131 query_ball_point) and builds xyz / dxyz / ppf channels from the groups (:173-244).
 * rrl_ball_group is that as one launch, forward only: plain device pointers, sizes and a stream; nothing is allocated, read
 * back or synchronised, there is no scratch, and every refusal happens on the host before the launch.
 *
 * pts [B][n][3]; normals [B][n][3] (NULL unless RRL_GROUP_PPF is asked for); counts [B] (device int32 or NULL = n): sample b
 * has n_b = clamp(counts[b], 0, n) points, rows beyond are never read.  query_idx [B][S] (device int32, or NULL: query q is
 * point q, then S <= n and a sample has min(S_b, n_b) queries), clamped into [0, n_b); qcounts [B] (or NULL = S): S_b =
 * clamp(qcounts[b], 0, S), and 0 for a sample without points.
 *
 * Membership: candidate j belongs to query i (a point index) iff d2 <= (double)r2, d2 = (dx dx + dy dy) + dz dz in double
 * from the double differences of the float32 coordinates, uncontracted (rrl_knn3's distance) -- a NaN distance never --
 * and, with exclude_self, j != i (a duplicate of the query at another index is a member).
 * Selection: the nsample members of lowest index, ascending, in idx [B][S][nsample]; found [B][S] = how many slots hold a
 * member; the slots beyond hold the pad index: i with exclude_self, else the first member (i when there is none).
 * feat (optional; NULL iff channels == 0) [B][S][nsample][C], the chosen channels in this order:
 *   RRL_GROUP_XYZ  (3) x_i, repeated over the slots;
 *   RRL_GROUP_DXYZ (3) d = x_j - x_i, the float32 subtraction;
 *   RRL_GROUP_PPF  (4) angle(n_i, d), angle(n_j, d), angle(n_i, n_j), |d| with angle(a, b) = atan2(|a x b|, a . b), evaluated
 *                      in double from the float32 d and normals and rounded once.  A pad slot with exclude_self has d = 0 and
 *                      n_j = n_i: its four values are exactly 0.
 * Rows beyond S_b are zero in all three outputs.  Bit-reproducible; sample b of a ragged batch has the bits of its own call.
 *
 * RRL_E_ARG: NULL pts / idx / found; B outside 1..32767; n < 1 or beyond rrl_sort_capacity(); S < 0; S > n with NULL
 * query_idx; nsample outside 1..RRL_GROUP_MAX_SAMPLE; r2 negative or NaN; channels outside the mask, channels without feat
 * or feat without channels; RRL_GROUP_PPF without normals.  S == 0 returns 0 without a launch. */
#define RRL_GROUP_XYZ 1
#define RRL_GROUP_DXYZ 2
#define RRL_GROUP_PPF 4
#define RRL_GROUP_MAX_SAMPLE 64
int rrl_ball_group(const float *pts, const float *normals, const int32_t *counts, const int32_t *query_idx,
                   const int32_t *qcounts, float r2, int nsample, int exclude_self, int channels, int32_t *idx, int32_t *found,
                   float *feat, int B, int n, int S, void *stream);

/* ---- k nearest neighbours, any k up to RRL_KNN_MAX_K, and DCP's graph features ------------
 * DCP's feature extractor starts with get_graph_feature(x, k = 20) (dcp/model.py:46-78): a (B, N, N) float32 distance
 * matrix by matmul, topk, an index-offset tensor, a gather, repeat, cat and permute.  rrl_knn is the exact k-NN behind it with
 * the features written by the same kernel, forward only: plain device pointers, sizes and a stream; nothing is allocated,
 * read back or synchronised, there are no atomics, and every refusal happens on the host before any HIP call.
 *
 * ref [B][n][3]; count_ref [B] (device int32 or NULL = n): sample b has n_b = clamp(count_ref[b], 0, n) reference points, the
 * rows beyond are never read.  Self form, qry == NULL: the queries are the reference's own rows, S must equal n, sample b has
 * n_b queries and count_qry is not read.  Cross form: qry [B][S][3], count_qry [B] (or NULL = S): S_b = clamp(count_qry[b], 0, S).
 *
 * The result: for query q the k smallest keys (d, j) in lexicographic order over the sample's reference points, d =
 * (dx dx + dy dy) + dz dz in double from the double differences of the float32 coordinates, uncontracted (rrl_knn3's distance),
 * j the original row: ascending distance, the lowest index among equal distances.  A pair whose d is NaN or +inf is no
 * neighbour.  In the self form the point itself is a neighbour at d = 0 unless RRL_KNN_EXCLUDE_SELF is set, which removes the
 * row's own index only (a duplicate of it at another index stays); the flag means nothing in the cross form.
 * found [B][S] (optional) = min(k, neighbours); k > n is legal.  idx [B][S][k]; dist2 [B][S][k] (optional) = d rounded once to
 * float32.  The slots at or beyond found repeat slot 0 in every output.  A row with found == 0 -- an empty reference, a NaN
 * query, a row beyond S_b -- is zero in every output.
 * feat (optional; NULL iff channels == 0) [B][S][k][C], the chosen channels always in this order:
 *   RRL_KNN_NBR  (3) x_j;
 *   RRL_KNN_DXYZ (3) x_j - x_i, the float32 subtraction;
 *   RRL_KNN_CTR  (3) x_i, repeated over the slots.
 * With RRL_KNN_CHANNEL_FIRST feat is [B][C][S][k]: the tensor DCP's permute(0, 3, 1, 2) produces, written directly.
 *
 * Method: the sorted layout's sphere tree (16^3-cell Hilbert sort of both clouds, supergroups of 64 records; the walk and
 * its bound for k keys are in csrc/rrl_knn.hip) wherever max(n, S) <= rrl_sort_capacity(), else -- and with RRL_KNN_BRUTE --
 * brute force, one lane per query.  Both give the same bits; a sample with a NaN, an infinite or a huge (|P| > 1e15)
 * coordinate within its counts takes the brute loop inside the tree's launch.  Launches: 1 for brute force; the tree 3 up to
 * 4096 points and 5 beyond (6 in the cross form).  Two calls give the same bits; sample b of a ragged batch has the bits of
 * its own call.  ws: scratch of rrl_knn_workspace_bytes(B, n, S) bytes, needed by either method.
 *
 * RRL_E_ARG: NULL ref / idx / ws; B outside 0..32767; n < 1; S < 0; k outside 1..RRL_KNN_MAX_K; qry == NULL with S != n; flags
 * or channels outside their masks, channels without feat or feat without channels.  Then RRL_E_WS: a short ws.  B == 0 or
 * S == 0 returns 0 without a launch. */
#define RRL_KNN_MAX_K 32
#define RRL_KNN_EXCLUDE_SELF 1
#define RRL_KNN_CHANNEL_FIRST 2
#define RRL_KNN_BRUTE 4 /* force brute force; default: the tree where it serves */
#define RRL_KNN_NBR 1
#define RRL_KNN_DXYZ 2
#define RRL_KNN_CTR 4
size_t rrl_knn_workspace_bytes(int B, int n, int S);
int rrl_knn(const float *ref, const int32_t *count_ref, const float *qry, const int32_t *count_qry, int k, int flags,
            int channels, void *ws, size_t ws_bytes, int32_t *idx, int32_t *found, float *dist2, float *feat,
            int B, int n, int S, void *stream);

/* ---- Point-to-plane ICP: normals from ball groups, the linearised fit, its pose step, an epoch ----
 * The house rules of the closed-form fits hold for all four entries: float32 in, every sum a fixed-order DOUBLE sum
 * (per-lane accumulators, the wavefront's DPP tree, four wavefronts, partial rows in index order), rounded once; no atomics,
 * nothing indexed by unclamped data; counts are device int32 [B], clamped by the kernels, never read on the host; the same
 * bits on every call, and sample b of a ragged batch has the bits of its own B = 1 call; nothing synchronises.
 *
 * rrl_idx_normals: unit normals from neighbour lists, one launch (one wavefront per row, four rows per workgroup).
 * pts [B][n][stride] (stride >= 3 floats per row); idx [B][S][nsample], found [B][S] as rrl_ball_group writes them; counts [B]
 * or NULL (= n).  Row i: its members are the first clamp(found, 0, nsample) slots; a slot whose index is < 0 or >= the sample's
 * count is dropped; k members remain.  Pivot = the point of the first member kept, d_j = double(x_j) - double(pivot),
 * m = sum d_j / k, C = sum d_j d_j^T - k m m^T, all double and uncontracted.  C's eigenvalues l0 <= l1 <= l2 by cyclic Jacobi
 * rotations in double; normal = the eigenvector of l0 (the lowest column among equal eigenvalues), its sign such that the
 * component of largest magnitude (the lowest index among equals) is positive, rounded to float32 once; quality (optional,
 * [B][S]) = (l1 - l0) / l2.  A row with k < 3, a non-finite C, or l1 <= rank_tol l2 (collinear or coincident members) gets
 * the normal (0, 0, 0) and quality 0 -- as does every row beyond a sample's queries, whose found is 0.  The normals are NOT
 * oriented: n and -n describe the same plane, and the point-to-plane residual does not tell them apart.
 * RRL_E_ARG before the launch: NULL pts / idx / found / normals; B outside 1..32767; n < 1 or beyond rrl_sort_capacity();
 * S < 0; stride < 3; nsample outside 1..RRL_GROUP_MAX_SAMPLE; rank_tol negative, NaN or >= 1.  S == 0: no launch. */
int rrl_idx_normals(const float *pts, int stride, const int32_t *idx, const int32_t *found, const int32_t *counts, int nsample,
                    float rank_tol, float *normals, float *quality, int B, int n, int S, void *stream);

/* rrl_plane_normal_eq: the sums of ONE linearised point-to-plane fit of moved [B][N][3] onto the planes (tar [B][M][tar_stride],
 * normals [B][M][3]).  Pairs, skips, weights w [B][N] (NULL = 1) and the gate are rrl_kabsch_fwd's: keys [B][N] are the u64
 * keys a Chamfer walk left for the rows of moved (NULL: partner i <-> i, then M == N); a row at or beyond count1[b], an all-ones
 * key, a key whose index is >= M or >= count2[b] contributes nothing and is counted in info[b][3]; a pair whose key distance
 * word exceeds gate_sq[b] (keys only) gets weight 0.  In addition a partner whose normal is (0, 0, 0) or not finite gets weight
 * 0: it is neither used nor skipped.  Per used pair, in double from the float32 values, with c = pivot[b] ([B][3]; NULL: the
 * origin): p = y - c, e = y - b, r = (e0 n0 + e1 n1) + e2 n2, a = p x n, J = (a, n); the step it linearises is
 * y -> c + Rot(omega)(y - c) + v, so that r changes by J . (omega, v): a rotation about the pivot, which keeps a cloud far from
 * the origin well conditioned.  The 32 sums: w J J^T (upper triangle, row-major, 21), w J r (6), w, w r^2, w (key distance
 * word), pairs used, pairs skipped.  Launches: partials (grid ceil(N / 512) x B) into part, then one wavefront per sample; ONE
 * launch when N <= 512.
 * neq [B][32] double (RRL_PLANE_*): H / W, g / W, W = sum w, the mean squared plane residual, the key mean, used, skipped.
 * info [B][4] int32: pairs used, status, 0, pairs skipped.  Status: RRL_FIT_OK, or RRL_FIT_FEW -- fewer than 6 used pairs, or
 * W <= 0 or NaN: H, g, the residual and the key mean are then 0.
 * Refusals, before any launch: RRL_E_ARG -- a NULL args / moved / tar / normals / neq / info / part, struct_bytes != sizeof,
 * B < 0 or > 32767, N <= 0, M <= 0, tar_stride < 3, a misaligned neq or part, no keys and M != N, gate_sq without keys --, then
 * RRL_E_WS: part_bytes < rrl_plane_part_bytes(B, N).  B == 0 returns 0 without a launch. */
#define RRL_PLANE_H 0
#define RRL_PLANE_G 21
#define RRL_PLANE_W 27
#define RRL_PLANE_RES 28
#define RRL_PLANE_KEYMEAN 29
#define RRL_PLANE_USED 30
#define RRL_PLANE_SKIPPED 31
#define RRL_PLANE_DOUBLES 32
typedef struct rrl_plane_args {
    int32_t struct_bytes, B, N, M, tar_stride, reserved;
    const float *moved; const uint64_t *keys; const float *tar, *normals; const int32_t *count1, *count2;
    const float *w, *gate_sq, *pivot;
    void *part; size_t part_bytes;
    double *neq; int32_t *info;
} rrl_plane_args;
size_t rrl_plane_part_bytes(int B, int N);
int rrl_plane_normal_eq(const rrl_plane_args *args, void *stream);

/* rrl_plane_step_batch: the pose step of point-to-plane ICP for a batch, one launch, one wavefront per pair: from neq and
 * info of rrl_plane_normal_eq and the current pose R [B][9], T [B][3] (x -> x R + T).  Pair b, unless done, with status
 * RRL_FIT_OK: (H + damping[b] diag(H) + eps I) x = -g by Cholesky in double (the solver, the step scale and the two clamps of
 * rrl_se3_newton_step_batch: (omega, v) = step[b] x, |omega| <= max_rot[b], |v| <= max_trans[b]); then with the exact Rodrigues
 * rotation and c = pivot[b] (NULL: the origin)
 *   R <- R Rot^T,   T <- (T - c) Rot^T + c + v,
 * one Gram-Schmidt pass over the rows of R, rounded to float32 once.  last_step[b] = (|omega|, |v|) as applied; the stopping
 * rule, the state words and the log row -- (the mean squared plane residual, value[b], status of the sums == RRL_FIT_OK) into
 * table[cursor[b]][b] and row[b], cursor[b] += 1 -- are the pose-step state's (above).  state[b][3]: RRL_PLANE_STEPPED,
 * RRL_PLANE_FEW (the sums' RRL_FIT_FEW: pose kept), RRL_PLANE_FAILED (a pivot of the factorisation that does not exceed eps --
 * a singular H: all normals parallel --, or a non-finite sum, solution or pose: pose kept) or RRL_PLANE_DONE.
 * pivot, value, table, cursor, row, last_step, tol_rot / tol_trans (patience <= 0) may be NULL.  RRL_E_ARG before the launch:
 * B < 0, a NULL neq / info / damping / step / max_rot / max_trans / R / T / state, a misaligned neq, eps < 0 or NaN,
 * patience > 0 without both tolerances; B == 0 returns 0 without a launch. */
#define RRL_PLANE_STEPPED RRL_POSE_STEPPED
#define RRL_PLANE_FEW RRL_POSE_SKIPPED
#define RRL_PLANE_FAILED RRL_POSE_FAILED
#define RRL_PLANE_DONE RRL_POSE_DONE
int rrl_plane_step_batch(const double *neq, const int32_t *info, const float *pivot, const float *damping, const float *step,
                         const float *max_rot, const float *max_trans, const float *tol_rot, const float *tol_trans, int patience,
                         double eps, float *R, float *T, const float *value, float *table, long long *cursor, long long nrows,
                         float *row, float *last_step, int32_t *state, int B, void *stream);

/* One point-to-plane ICP epoch for a batch of B pairs as ONE call: the entries back to back on the caller's stream, nothing
 * else --
 *   1. rrl_rigid_apply_fwd: moved = src R + T                                   (src [B][N][3], transpose_r = 0);
 *   2. rrl_chamfer_tree_fwd_counted on (moved, tar, count1, count2) with the prepared orders -> best_x, best_y, values [B];
 *   3. rrl_plane_normal_eq with keys = best_x, tar [B][M][3], normals [B][M][3], the counts, w, gate_sq, pivot -> neq, info;
 *   4. rrl_plane_step_batch with value = values (the pair's Chamfer distance, which the walk's other half supplies).
 * No host read-back.  Refusals, all before the first launch: RRL_E_ARG -- a NULL or wrongly sized struct, B <= 0 or > 32767,
 * N or M <= 0 or beyond rrl_sort_capacity(), any NULL pointer among src, tar, normals, R, T, moved, cham_ws, best_x, best_y,
 * values, part, neq, info, damping, step, max_rot, max_trans, state, exactly one count or one order, eps < 0 or NaN,
 * patience > 0 without both tolerances, a misaligned part or neq --, then RRL_E_WS: a short cham_ws or part. */
typedef struct rrl_plane_epoch_args {
    int32_t struct_bytes, B, N, M, patience, reserved;
    const float *src, *tar, *normals; const int32_t *count1, *count2; float *R, *T, *moved;
    void *cham_ws; size_t cham_ws_bytes; uint64_t *best_x, *best_y; float *values; const int32_t *order_x, *order_y;
    const float *w, *gate_sq, *pivot;
    void *part; size_t part_bytes; double *neq; int32_t *info;
    const float *damping, *step, *max_rot, *max_trans, *tol_rot, *tol_trans; double eps; float *last_step; int32_t *state;
    float *table; long long *cursor; long long table_rows; float *row;
} rrl_plane_epoch_args;
int rrl_plane_icp_epoch(const rrl_plane_epoch_args *args, void *stream);

/* ---- Robust ICP: Welsch weights with an annealed scale around the keyed Kabsch fit ----------
 * Point-to-point ICP whose pairs carry the weights w = exp(-d^2 / (2 nu^2)) of the loss's own Welsch function, d^2 the key's
 * distance word, with a per-pair scale nu that starts at a multiple of the first epoch's median residual and is multiplied
 * by `anneal` whenever the pose has settled at the current scale, down to nu_end (Fast-Robust-ICP without its Anderson
 * acceleration).  A VALID row, everywhere below, is a row rrl_kabsch_fwd would not skip: below count_a[b], its key not all
 * ones, its key's index < m and < count_b[b] (counts NULL: n / m; clamped to [0, n] / [0, m] by the kernels).
 *
 * rrl_key_median: for each pair b the exact LOWER median of the distance words (key >> 32) of the valid rows of keys [B][n]:
 * the word of 0-based rank (k - 1) / 2 among the k valid words sorted as uint32 (non-negative floats sort alike; torch.median's
 * rule), bit for bit -> med_sq [B]; info [B][2] = (k, k == 0); med_sq = 0 when k == 0.  With nu != NULL also
 * nu[b] = max(float32(nu_scale * sqrt(double(med_sq[b]))), nu_end[b]) (nu_end[b] when the left side is NaN).  One workgroup
 * per pair, four 8-bit digit passes over an LDS histogram of integer counts: no floating atomics, the same bits on every call.
 * RRL_E_ARG before the launch: B < 0 or > 32767, n <= 0 or beyond rrl_sort_capacity(), m <= 0, a NULL keys / med_sq / info,
 * exactly one count, nu without nu_end or with nu_scale <= 0 (or NaN).  B == 0 returns 0 without a launch. */
int rrl_key_median(const uint64_t *keys, const int32_t *count_a, const int32_t *count_b, int B, int n, int m, float *med_sq,
                   int32_t *info, float *nu, double nu_scale, const float *nu_end, void *stream);

/* w [B][n]: w[b][i] = float32(exp(-double(d^2) / (2 double(nu[b])^2))) for a valid row whose distance word d^2 is a number,
 * exactly 0 for every other row, and 0 on all rows of a pair whose nu[b] is <= 0 or not finite (the fit then reports
 * RRL_FIT_FEW).  Grid (ceil(n / 256), B).  RRL_E_ARG before the launch: B < 0 or > 32767, n <= 0, m <= 0, a NULL keys / nu / w,
 * exactly one count.  B == 0 returns 0 without a launch. */
int rrl_welsch_weights(const uint64_t *keys, const int32_t *count_a, const int32_t *count_b, const float *nu, float *w, int B,
                       int n, int m, void *stream);

/* rrl_icp_step_batch's step -- the same arguments, step lengths, log row and status words -- with the annealing rule in
 * place of its stopping rule.  nu [B] (in / out), nu_end [B], level [B][2] int32 = (epochs at this nu, levels finished).
 * Pair b, unless done: the ICP step updates the pose and the calm count (a failed or skipped fit keeps the pose and nu and
 * resets the calm count); level[b][0] += 1; the level is OVER when patience > 0 and calm >= patience, or when level_cap > 0
 * and level[b][0] >= level_cap.  Over with nu[b] > nu_end[b]: nu[b] = max(nu[b] * anneal, nu_end[b]) in float32, calm = 0,
 * level[b] = (0, level[b][1] + 1), the pair is NOT done.  Over otherwise: the pair is done as rrl_icp_step_batch marks it
 * (state word 2 = the epochs issued; from the next call on the pose, nu and level keep their bits and the status is
 * RRL_POSE_DONE).  RRL_E_ARG before the launch: what rrl_icp_step_batch refuses, a NULL nu / nu_end / level, anneal outside
 * (0, 1), level_cap < 0, patience <= 0 together with level_cap == 0. */
int rrl_robust_step_batch(const float *Rk, const float *Tk, const int32_t *info, const double *fit, float *R, float *T,
                          const float *tol_rot, const float *tol_trans, int patience, const float *value, float *table,
                          long long *cursor, long long nrows, float *row, float *last_step, int32_t *state, float *nu,
                          const float *nu_end, float anneal, int level_cap, int32_t *level, int B, void *stream);

/* One robust ICP epoch for a batch of B pairs as ONE call: the entries back to back on the caller's stream, nothing else --
 *   1. rrl_rigid_apply_fwd: moved = src R + T;
 *   2. rrl_chamfer_tree_fwd_counted on (moved, tar, count1, count2) with the prepared orders -> best_x, best_y, values [B];
 *   3. when init != 0, rrl_key_median on best_x -> med_sq, med_info and the starting nu (nu_scale, nu_end);
 *   4. rrl_welsch_weights -> w [B][N];
 *   5. rrl_kabsch_fwd with a = src (as given), keys = best_x, b = tar, the counts, w, gate_sq -> Rk, Tk, fit, info;
 *   6. rrl_robust_step_batch with value = values.
 * args: rrl_icp_epoch's own argument struct, every field with its meaning there -- the clouds, the walk's buffers, the fit's
 * and the step's -- except w, which must be NULL: the weights are this epoch's OUTPUT and arrive, with everything the
 * annealing adds, as plain arguments (the library keeps one struct per epoch shape; this epoch has rrl_icp_epoch's shape).
 * No host read-back.  Refusals, all before the first launch: RRL_E_ARG -- what rrl_icp_epoch refuses, args->w != NULL, a NULL
 * w / nu / nu_end / level / med_sq / med_info, anneal outside (0, 1), level_cap < 0, nu_scale <= 0, patience <= 0 together with
 * level_cap == 0 --, then RRL_E_WS: a short cham_ws or part. */
int rrl_robust_icp_epoch(const rrl_icp_epoch_args *args, int init, float *w, float *nu, const float *nu_end, float *med_sq,
                         int32_t *med_info, double nu_scale, float anneal, int level_cap, int32_t *level, void *stream);

/* ---- DCP's softmax pointer: the SVD head's correspondences without the score matrix ---------
 * SVDHead.forward (dcp/model.py:419-425): scores = softmax(src_emb^T tgt_emb / sqrt(C), dim = 2), src_corr = tgt scores^T.
 * Channel-first as DCP holds them: src_emb [B][C][N], tgt_emb [B][C][M], tgt [B][3][M], corr and g_corr [B][3][N].
 * count_src / count_tgt: device int32 [B] or NULL (= N / M), clamped by the kernels to [0, N] / [0, M], never read on the host;
 * what lies beyond a count is never read.  Plain device pointers, sizes and a stream: nothing is allocated, read back or
 * synchronised, there are no atomics, nothing is indexed by data, every launch goes to the caller's stream.
 *
 * The rule (the library's first matrix-core kernel: gfx950's f32-input MFMA v_mfma_f32_32x32x2_f32 IS this chain, bit for bit):
 *  1. chain[j][k] starts at +0 and runs over the channels c = 0 .. C - 1 in ascending order, chain = fmaf(src_emb[c][j],
 *     tgt_emb[c][k], chain): ONE chain per score, never split over wavefronts or channel blocks, so a score does not depend on
 *     the tiling.  An odd C is padded with a zero channel in BOTH operands (0 * inf would be NaN).
 *  2. z[j][k] = chain * sc, one float32 multiplication, sc = float32(1 / sqrt(double(C))).
 *  3. A softmax state is (m, l, n[3]), one per row and slice of RRL_POINTER_SLICE columns: m the largest score of the row's
 *     columns in the slice (a lane keeps the slice's scores in registers, so the maximum is final before the first term: the
 *     running maximum of a state rises once, from -inf, and no rescaling factor is ever applied inside a state), l = sum p and
 *     n = sum p x in double, p the float32 expf of the float32 difference z - m; a -inf score and a masked column give p = 0
 *     without forming -inf - (-inf).  A lane sums its columns ascending (columns 4 h .. 4 h + 3 of every eight, h = lane >> 5),
 *     the row's two half-waves are added h = 0 first.  The slices are merged in index order: M = max m_s, L = sum l_s expf(m_s -
 *     M), likewise n: ONE float32 factor per slice, common to l and n.  corr[j] = float32(n / L); a row at or beyond count_src,
 *     and every row when count_tgt[b] == 0, is exactly 0.
 *  4. Backward, on z recomputed by the same chain (the same bits) and the row's final M_j, L_j and corr_j kept in ws:
 *     P = expf(z - M_j) (1 / L_j) (the reciprocal taken once per row, in double), delta_j = g_j . corr_j, ds[j][k] = float32(P (g_j . x_k - delta_j) sc), all in double from the
 *     float32 expf; d_tgt[k] = sum_j P g_j in double (per lane over its rows ascending, then the lane halves, then the four
 *     wavefronts), rounded once; d_src_emb[c][j] = the float32 fmaf chain over k ascending of ds[j][k] tgt_emb[c][k], and
 *     d_tgt_emb[c][k] the chain over j ascending of ds[j][k] src_emb[c][j]: whole chains, never cut (an MFMA again).  Rows and
 *     columns beyond the counts get zero gradient.  Every element of every output is written; nothing is pre-zeroed.
 * Two calls give the same bits; sample b of a ragged batch has the bits of its own B = 1 call.
 *
 * scores (optional) [B][N][M]: z, -inf at and beyond the counts -- detached, for a trainer's endpoints.  info (optional) [B]:
 * 1 where a score inside the counts is NaN or +-inf (the sample's outputs are then NaN where it reaches), else 0.
 * d_src_emb, d_tgt_emb, d_tgt: each may be NULL.
 * ws: rrl_pointer_workspace_bytes(B, C, N, M) bytes, 8-byte aligned: six doubles per (row, slice) and five per row -- no
 * (B, N, M) array in either direction (except scores when asked for).  The backward takes the ws its forward filled.
 * Launches: forward 2 (tiles, then the slices' merge); backward 1 per pass (d_src_emb; d_tgt_emb with d_tgt).
 * Refusals, on the host before any HIP call: RRL_E_ARG -- NULL src_emb / tgt_emb / tgt / ws / corr (backward: g_corr); B outside
 * 0..32767; C outside 1..RRL_POINTER_MAX_C; N or M outside 1..16384 --, then RRL_E_WS: a short or misaligned ws.  B == 0
 * returns 0 without a launch. */
#define RRL_POINTER_MAX_C 1024
#define RRL_POINTER_SLICE 128 /* columns per slice of the forward */
size_t rrl_pointer_workspace_bytes(int B, int C, int N, int M);
int rrl_pointer_fwd(const float *src_emb, const float *tgt_emb, const float *tgt, const int32_t *count_src,
                    const int32_t *count_tgt, void *ws, size_t ws_bytes, float *corr, float *scores, int32_t *info, int B, int C,
                    int N, int M, void *stream);
int rrl_pointer_bwd(const float *src_emb, const float *tgt_emb, const float *tgt, const int32_t *count_src,
                    const int32_t *count_tgt, void *ws, size_t ws_bytes, const float *g_corr, float *d_src_emb, float *d_tgt_emb,
                    float *d_tgt, int B, int C, int N, int M, void *stream);

/* ---- FMR's inverse-compositional solver: the pose head as three pairs of entries -------------
 * SolveRegistration.ic_algo / approx_Jac (fmr/model.py:318-439) with se_math/se3.py:57-80, 133-165 (exp, ExpMap) and
 * se_math/invmat.py:6-13, 83-112 (InvMatrix), everything between the encoder's outputs and the poses; the encoder stays the
 * caller's.  Features f32 [B][K]; perturbed features fp [B][6][K] (the encoder's output on the perturbed clouds viewed as
 * (B, 6, K): no transpose); dt [B][6]; poses 4 x 4 row-major [B][4][4], p' = R p + t, fourth row (0, 0, 0, 1); clouds [B][N][3].
 * Plain device pointers, sizes and a stream: nothing is allocated, read back or synchronised, there are no atomics, every
 * element of every output is written and nothing is pre-zeroed, every launch goes to the caller's stream and is capturable.
 * A sum over K or N is a fixed-order double sum: a workgroup of 256 lanes per sample, lane l takes l, l + 256, ... ascending,
 * the 64 lanes of a wavefront are added by one fixed tree, the four wavefronts in index order.  Two calls give the same bits;
 * sample b of a batch has the bits of its own B = 1 call (rrl_ic_update_fwd: where the stop rule decides alike).
 *
 * exp(x), x = (w, v): rrl_se3_exp's rule in DOUBLE -- t = |w|, W = [w]x, R = I + s1 W + s2 W W, V = I + s2 W + s3 W W, p = V v,
 * s1 = sin t / t, s2 = (1 - cos t) / t^2, s3 = (t - sin t) / t^3, the reference's Taylor polynomials inside |t| < 0.01
 * (se_math/sinc.py) --, rows (R | p) and (0, 0, 0, 1).  gen_k = the k-th generator (se3.py genmat): for k < 3, with a = (k + 1) % 3
 * and b = (k + 2) % 3, row b of gen_k X is row a of X and row a is minus row b; for k >= 3, row k - 3 is X's fourth row.
 *
 * 1. rrl_ic_perturb_fwd: out [B][6][N][3] = D_i applied to p0 [B][N][3], D_i = exp(-dt_i e_i) evaluated in double and rounded
 *    ONCE to float32; a point is the float32 chain of rrl_rigid_apply_fwd in this convention,
 *        out_j = fmaf(p_2, D[j][2], fmaf(p_1, D[j][1], p_0 * D[j][0])) + D[j][3].                                One launch.
 *    rrl_ic_perturb_bwd: to dt only (p0 carries no gradient in the reference).  M = sum_n g_out[b][i][n] (x) [p_n; 1], twelve
 *    double sums over n; g_dt[b][i] = float32(-sum_jk M_jk [gen_i D_i]_jk), D_i in double (not rounded).  For a single-axis
 *    twist ExpMap's rule IS the derivative.                                                                      One launch.
 * 2. rrl_ic_pinv_fwd: all in double.  J[k][i] = (double(f0[k]) - double(fp[i][k])) / double(dt[i]); H = the 21 sums sum_k
 *    J_ki J_kj; H^-1 by the unpivoted, undamped Cholesky (the loops of the pose steps' solver), column c solved from e_c;
 *    pinv[i][k] = float32(sum_j H^-1_ij J_kj), j ascending.  info[b] = 1 (info may be NULL) and that sample's pinv is exactly 0
 *    -- its pose will not move -- when a pivot p_j fails p_j > (K + 6) 2^-52 H_jj (the rounding of H's own sums: below it a
 *    pivot is not told from 0), is not finite, or an entry of H^-1 is not finite; when an input of the sample (f0, fp, dt) is
 *    NaN or +-inf; when a dt_i is 0; when K < 6.  This replaces the reference's `except RuntimeError`.
 *    ws: RRL_IC_WS_DOUBLES doubles per sample, 8-byte aligned -- H^-1 (36, zeros when flagged), the flag, padding; J is not
 *    kept: the backward recomputes it by the same expression.                                                    One launch.
 *    rrl_ic_pinv_bwd, G = g_pinv: P = G J (36 double sums over k); S = -(H^-1 P) H^-1; dJ[k][i] = sum_j G[j][k] H^-1_ji + sum_j
 *    J[k][j] (S + S^T)_ji; d_f0[k] = float32(sum_i dJ_ki / dt_i); d_fp[i][k] = float32(-(dJ_ki / dt_i)); d_dt[i] =
 *    float32(-(sum_k dJ_ki J_ki) / dt_i).  InvMatrix.backward composed with the two bmm's.  A flagged sample gets zeros.
 *    d_f0, d_fp, d_dt: each may be NULL.                                                                         One launch.
 * 3. rrl_ic_update_fwd: r = f1 - f0 (one float32 subtraction); dx_i = float32(-sum_k double(pinv[i][k]) double(r[k])); a
 *    sample's step length n_b = float32(sqrt(sum_i double(dx_i)^2)).  The batch-wide rule of the reference (check = max_b n_b,
 *    stop when check < xtol; a NaN n_b makes check NaN, which is not < xtol): the batch stops when `stop` (a device int32 the
 *    caller zeroes once per loop) is already set or EVERY n_b < xtol.  Then stop = 1 and g_new = g bit for bit for every sample;
 *    else stop = 0 and g_new = float32(exp(dx) g), exponential and product in double (rows 0..2: sum over m ascending of
 *    exp_im g_mj; the fourth row is g's).  A NaN dx therefore does not stop: that sample's pose becomes NaN.  `stopped` (int32,
 *    one word per CALL) receives this call's decision for its backward.  Deviation from the reference: after the stop its
 *    g_series_gpu keeps zeros; here the later poses hold the last pose and `stop` lets a caller put the zeros back.
 *    ws: rrl_ic_update_workspace_bytes(B), 8-byte aligned (the n_b).   Two launches: per-sample sums, then one workgroup.
 *    rrl_ic_update_bwd, on the r, dx and `stopped` the forward left; G' = g_g_new, Gr = g_r, Gdx = g_dx (each may be NULL = 0).
 *    Stopped: d_g = G', d_f1 = Gr, d_f0 = -Gr, d_pinv = 0.  Else d_g = exp(dx)^T G'; q_k = sum_ij (G' g^T)_ij [gen_k exp(dx)]_ij
 *    + Gdx_k -- ExpMap.backward's rule word for word: for a general twist NOT the exact derivative of exp --; d_pinv[i][k] =
 *    float32(-(q_i r_k)); d_f1[k] = float32(Gr_k - sum_i pinv[i][k] q_i); d_f0 = -d_f1.  d_g, d_pinv, d_f0, d_f1: each may be
 *    NULL.                                                                                                       One launch.
 * Refusals, on the host before any HIP call: RRL_E_ARG -- a NULL pointer that is not marked optional, B outside 0..65535,
 * N < 1, K outside 1..RRL_IC_MAX_K --, then RRL_E_WS: a short or misaligned ws.  B == 0 returns 0 without a launch. */
#define RRL_IC_MAX_K 16384
#define RRL_IC_WS_DOUBLES 40 /* per sample: H^-1 [36], the flag, padding */
int rrl_ic_perturb_fwd(const float *p0, const float *dt, float *out, int B, int N, void *stream);
int rrl_ic_perturb_bwd(const float *p0, const float *dt, const float *g_out, float *g_dt, int B, int N, void *stream);
size_t rrl_ic_pinv_workspace_bytes(int B, int K);
int rrl_ic_pinv_fwd(const float *f0, const float *fp, const float *dt, void *ws, size_t ws_bytes, float *pinv, int32_t *info,
                    int B, int K, void *stream);
int rrl_ic_pinv_bwd(const float *f0, const float *fp, const float *dt, const void *ws, size_t ws_bytes, const float *g_pinv,
                    float *d_f0, float *d_fp, float *d_dt, int B, int K, void *stream);
size_t rrl_ic_update_workspace_bytes(int B);
int rrl_ic_update_fwd(const float *pinv, const float *f0, const float *f1, const float *g, float xtol, int32_t *stop, void *ws,
                      size_t ws_bytes, float *r, float *dx, float *g_new, int32_t *stopped, int B, int K, void *stream);
int rrl_ic_update_bwd(const float *pinv, const float *r, const float *dx, const float *g, const int32_t *stopped,
                      const float *g_g_new, const float *g_r, const float *g_dx, float *d_g, float *d_pinv, float *d_f0,
                      float *d_f1, int B, int K, void *stream);

/* ---- A shared-MLP + GroupNorm + ReLU + max-pool encoder: FMR's PointNet, RPM's prepool ---------
 * fmr/model.py:57-126 PointNet (3 -> 64 -> 64 -> 64 -> 128 -> K, GroupNorm(8, .)) and rpm/models/feature_nets.py:31-52
 * ParameterPredictionNet.prepool (4 -> 64 -> 64 -> 64 -> 128 -> 1024, 8 / 8 / 8 / 8 / 16 groups), followed by the max over the
 * points.  points f32 [B][N][c0], 1 <= c0 <= RRL_PN_MAX_C0; layers l = 1 .. L, 2 <= L <= RRL_PN_MAX_LAYERS, widths[l - 1] = c_l
 * a multiple of groups[l - 1] = G_l, hidden widths <= RRL_PN_MAX_HIDDEN, the last K = c_L <= RRL_IC_MAX_K.  widths and groups
 * are HOST arrays of L ints; params is a HOST array of 4 L DEVICE pointers, params[4 (l - 1) + 0 .. 3] = W_l [c_l][c_{l-1}] (a
 * Conv1d weight as torch holds it), b_l, gamma_l, beta_l [c_l]: they reach the kernels as arguments -- nothing is allocated,
 * copied, read back or synchronised, there are no atomics, every launch goes to the caller's stream and is capturable.
 *
 * The rule:
 *  1. y_l[c][n] is ONE float32 fmaf chain that starts at b_l[c] and runs over the input channels k ascending,
 *     y = fmaf(W_l[c][k], h_{l-1}[k][n], y), h_0 = the points; never split over wavefronts or tiles.  From 64 input channels
 *     upward it is gfx950's f32-input MFMA (bit for bit this chain, as for rrl_pointer_fwd; an odd count is padded with a zero
 *     channel in both operands), below plain fmaf.
 *  2. Per (sample, layer, group), over the m = (c_l / G_l) N values of the group: sum y and sum y^2 are fixed-order double
 *     sums (a lane over its points ascending, one butterfly over the 32 lanes of a tile, one partial per chunk of 128 points
 *     and channel in ws; then a channel's chunks ascending, per group lane i of a wavefront adds the channels i, i + 64, ...
 *     ascending, and the lanes are added by one fixed tree).  mu = sum y / m, var = max(0, sum y^2 / m - mu^2), r = 1 /
 *     sqrt(var + eps), in double.
 *  3. h_l[c][n] = float32(max(0, double(y) a_c + d_c)), a_c = double(gamma_c) r, d_c = double(beta_c) - mu a_c: a double
 *     multiplication, a double addition (not fused), one rounding to float32; max(0, t) is 0 where t < 0, else t (a NaN stays).
 *  4. y_L is never stored.  The map of 3 is monotone, so max_n h_L[c][n] is 3 at ext_c = max_n y_L[c][n] where a_c >= 0 and
 *     min_n y_L[c][n] where a_c < 0: feat[b][c] = float32(max(0, double(ext_c) a_c + d_c)), arg[b][c] = the LOWEST n that
 *     attains ext_c.  Deviation: where several points tie (or gamma_c = 0) torch's max-pool picks its own index among equal
 *     values; where feat = 0 no gradient flows either way.
 *  5. info[b] = 1 (info may be NULL) and feat[b][.] is NaN when a sum y or sum y^2, or an a_c or d_c, of ANY layer of the
 *     sample is not finite (a NaN or +-inf among the sample's points poisons that sample only, one in a parameter every
 *     sample); else info = 0.
 * ws: rrl_pointnet_workspace_bytes(...) bytes, 16-byte aligned; every byte is written by the forward.  offsets (optional):
 * RRL_PN_FIELDS byte offsets of its fields --
 *   RRL_PN_STAT  f64 [B][sum G_l][4]: sum y, sum y^2, mu, r per group, the layers' groups one after the other;
 *   RRL_PN_COEF  f64 [B][sum c_l][2]: a_c, d_c, the layers' channels one after the other;
 *   RRL_PN_PART  f64, per layer [B][chunks][c_l][2]: the per-chunk partial sums;
 *   RRL_PN_EPART per (sample, chunk, channel of the last layer): the chunk's extremum as z = y (gamma_c >= 0) or -y (gamma_c <
 *                0) f32, its lowest index int32 (r > 0, so a_c >= 0 exactly where gamma_c >= 0);
 *   RRL_PN_EXT   f32 [B][K]: ext_c;   RRL_PN_FLAG int32 [B]: info;
 *   RRL_PN_Y     f32 [B][sum hidden c_l][N]: y_1 .. y_{L-1} channel-first -- 4 sum hidden c_l bytes per point (1280 for FMR),
 *                nothing K wide per point.
 * Two calls give the same bits; sample b of a batch has the bits of its own B = 1 call.  Launches: two per layer.
 * Refusals, on the host before any HIP call: RRL_E_ARG -- a NULL points / params / params[i] / widths / groups / ws / feat /
 * arg, B outside 0..65535, N outside 1..2^20, c0, L, a width or a group count outside the limits above, eps <= 0 --, then
 * RRL_E_WS: a short or misaligned ws (rrl_pointnet_workspace_bytes is 0 for a shape that is refused).  B == 0 returns 0
 * without a launch. */
#define RRL_PN_MAX_C0 8
#define RRL_PN_MAX_LAYERS 8
#define RRL_PN_MAX_HIDDEN 128
enum { RRL_PN_STAT, RRL_PN_COEF, RRL_PN_PART, RRL_PN_EPART, RRL_PN_EXT, RRL_PN_FLAG, RRL_PN_Y, RRL_PN_FIELDS };
size_t rrl_pointnet_workspace_bytes(int B, int N, int c0, int L, const int32_t *widths, const int32_t *groups, size_t *offsets);
int rrl_pointnet_fwd(const float *points, const float **params, const int32_t *widths, const int32_t *groups, double eps,
                     void *ws, size_t ws_bytes, float *feat, int32_t *arg, int32_t *info, int B, int N, int c0, int L,
                     void *stream);
/* The backward of rrl_pointnet_fwd, on the ws its forward filled (16-byte aligned) and the forward's arg: from g_feat [B][K] to
 * d_points [B][N][c0] and, through d_params -- a HOST array of 4 L device pointers in params' order, or NULL --, dW_l, db_l,
 * dgamma_l, dbeta_l.  d_points, d_params and every entry of d_params may be NULL; what is asked for is written in full, nothing
 * is pre-zeroed.  All arithmetic is double on the kept float32 y_l, mu, r, a, d, ext and arg, one rounding per output; every sum
 * runs over its reduced index ascending in one thread, or lane l of a wavefront over n = l, l + 64, ... (sample after sample
 * where the batch is summed) and then one fixed tree; parameter gradients sum the samples b ascending.  No atomics.
 *  Per layer GroupNorm's rule with xhat = (y - mu) r, dxhat = gamma dout: dgamma_c = sum_n dout xhat, dbeta_c = sum_n dout,
 *  dy = r (dxhat - P / m - xhat Q / m), P = sum_group gamma dbeta, Q = sum_group gamma dgamma; dW = sum_{b,n} dy (x) h_{l-1},
 *  db = sum dy, dh_{l-1} = W^T dy (c ascending) gated by h_{l-1} > 0.
 *  The last layer needs no N x K work: dout is s_c = g_feat[c] [feat[c] > 0] at (c, arg_c) only, so with x_c = (ext_c - mu) r,
 *  t_c = r gamma_c s_c, A_g = -r P / m + r^2 Q mu / m, B_g = -r^2 Q / m, S1 = sum_n h_{L-1}[n] and S2 = sum_n h h^T (per sample):
 *  dW_L[c] = t_c h[arg_c] + A_g S1 + B_g (W_L[c] S2 + b_c S1), db_L[c] = t_c + N A_g + B_g (W_L[c] . S1 + N b_c), dgamma_c = s_c x_c,
 *  dbeta_c = s_c, dh_{L-1}[n] = M h[n] + v + sum over the channels c ascending with arg_c = n of t_c W_L[c], M = sum_c B_g W_L[c]^T
 *  W_L[c], v = sum_c (A_g + B_g b_c) W_L[c].  A sample the forward flagged has s_c = NaN: its d_points and every parameter
 *  gradient become NaN, as torch's would.
 * bws: rrl_pointnet_bwd_workspace_bytes(...) bytes, 8-byte aligned: 3 K + 2 G_L + 2 H (H + 1) + 2 hmax doubles per sample (H =
 * c_{L-1}, hmax the widest hidden layer) and two buffers of hmax N doubles per sample -- nothing K wide per point.
 * Refusals as the forward's (NULL arg / g_feat / bws: RRL_E_ARG; a short or misaligned ws or bws: RRL_E_WS); B == 0 returns 0. */
size_t rrl_pointnet_bwd_workspace_bytes(int B, int N, int c0, int L, const int32_t *widths, const int32_t *groups);
int rrl_pointnet_bwd(const float *points, const float **params, const int32_t *widths, const int32_t *groups, const void *ws,
                     size_t ws_bytes, const int32_t *arg, const float *g_feat, void *bws, size_t bws_bytes, float *d_points,
                     float **d_params, int B, int N, int c0, int L, void *stream);

/* ---- The grouped PointNet: shared layers over every (point, neighbour slot) position, max over each point's slots -------------
 * RPM's FeatExtractionEarlyFusion.prepool followed by torch.max(new_feat, 2)[0] (rpm/models/feature_nets.py:118-131, 196-199;
 * DESIGN.md section 25).  x f32 [B][N][S][c0], the layout rrl_ball_group writes: N points of S slots, 1 <= S <= RRL_PG_MAX_S, 1 <=
 * c0 <= RRL_PG_MAX_C0, N <= 2^20, N S <= 2^22.  Layers, widths, groups, params and the conventions as rrl_pointnet_fwd (2 <= L <=
 * RRL_PN_MAX_LAYERS, hidden widths <= RRL_PN_MAX_HIDDEN); the last width K <= RRL_PG_MAX_K.  Position p = n S + s takes the place
 * of rrl_pointnet_fwd's point: rules 1 and 3 hold as stated there over the P = N S positions, and
 *  2. per (sample, layer, group), over the m = (c_l / G_l) N S values of the group, sum y and sum y^2 are fixed-order double sums:
 *     a chunk is floor(128 / S) whole points (its positions in 32-position tiles from the chunk's start); a lane adds its
 *     positions of the chunk ascending (lane q those at offsets q, q + 32, ...), one butterfly over the 32 lanes, one partial per
 *     (chunk, channel) in ws; then per channel lane i of a wavefront adds the chunks i, i + 64, ... ascending and the lanes are
 *     added by one fixed tree; per group lane i adds the channels i, i + 64, ... and the same tree.  mu, var, r as there.
 *  4. y_L is never stored and h_L is never formed per position.  out[b][c][n] = float32(max(0, double(ext) a_c + d_c)), f32
 *     channel-first (B, K, N), with ext = max_s y_L[c][n S + s] where gamma_c >= 0 and min_s where gamma_c < 0; arg[b][c][n]
 *     int32 is the LOWEST slot s that attains it.  A point's slots are pooled inside one workgroup, never by atomics.
 *     Deviation: rrl_ball_group pads a short group with repeated slots, equal slots give exactly equal y, so ties are the normal
 *     case; torch's max picks its own index among equal values, arg is the lowest.  Parameter gradients do not depend on the choice.
 *  5. info[b] = 1 (info may be NULL) and out[b] is NaN throughout when a sum or coefficient of ANY layer of the sample is not finite.
 * ws: rrl_pointnet_group_workspace_bytes(...) bytes, 16-byte aligned, every byte written by the forward; offsets (optional):
 * RRL_PG_FIELDS byte offsets --
 *   RRL_PG_STAT f64 [B][sum G_l][4]; RRL_PG_COEF f64 [B][sum c_l][2]; RRL_PG_PART f64 per layer [B][chunks][c_l][2];
 *   RRL_PG_EXT f32 [B][K][N]: ext; RRL_PG_FLAG int32 [B]; RRL_PG_Y f32 [B][sum hidden c_l][N S]: y_1 .. y_{L-1} channel-first over
 *   the positions.  Nothing K wide per position is kept.
 * Two calls give the same bits; sample b of a batch has the bits of its own B = 1 call.  Launches: two per layer and one.
 * Refusals, on the host before any HIP call: RRL_E_ARG -- a NULL x / params / params[i] / widths / groups / ws / out / arg, B
 * outside 0..65535, N, S, N S, c0, L, a width or a group count outside the limits above, eps <= 0 --, then RRL_E_WS: a short or
 * misaligned ws (the size is 0 for a shape that is refused).  B == 0 returns 0 without a launch. */
#define RRL_PG_MAX_C0 16
#define RRL_PG_MAX_S 128
#define RRL_PG_MAX_K 1024
enum { RRL_PG_STAT, RRL_PG_COEF, RRL_PG_PART, RRL_PG_EXT, RRL_PG_FLAG, RRL_PG_Y, RRL_PG_FIELDS };
size_t rrl_pointnet_group_workspace_bytes(int B, int N, int S, int c0, int L, const int32_t *widths, const int32_t *groups,
                                          size_t *offsets);
int rrl_pointnet_group_fwd(const float *x, const float **params, const int32_t *widths, const int32_t *groups, double eps, void *ws,
                           size_t ws_bytes, float *out, int32_t *arg, int32_t *info, int B, int N, int S, int c0, int L,
                           void *stream);
/* The backward of rrl_pointnet_group_fwd on the ws its forward filled and the forward's arg: from g_out [B][K][N] to d_x
 * [B][N][S][c0] and, through d_params (a HOST array of 4 L device pointers, or NULL), dW_l, db_l, dgamma_l, dbeta_l.  d_x,
 * d_params and every entry of it may be NULL; what is asked for is written in full.  Double arithmetic on the kept float32 y_l,
 * mu, r, a, d, ext and arg, one rounding per output, no atomics; rrl_pointnet_bwd's rule 5 with P = N S for N and the last
 * layer's sparse term per point: s_{c,n} = g_out[c][n] [out[c][n] > 0] sits at position n S + arg[c][n];
 *  dbeta_c = sum_n s_{c,n}, dgamma_c = sum_n s_{c,n} x_{c,n}, x = (ext - mu) r, t_{c,n} = r gamma_c s_{c,n};
 *  dW_L[c] = sum_n t_{c,n} h[n S + arg_{c,n}] + A_g S1 + B_g (W_L[c] S2 + b_c S1), db_L[c] = sum_n t_{c,n} + P A_g + B_g (W_L[c] . S1
 *  + P b_c), dh_{L-1}[p] = M h[p] + v + sum over the channels c ASCENDING with arg[c][n(p)] = s(p) of t_{c,n(p)} W_L[c].
 * Order of the sums: a sum over a point's or a sample's points is lane i of a wavefront over n = i, i + 64, ... and one fixed
 * tree; the position-summed products (S1, S2, every hidden dW and db, the hidden layers' dgamma and dbeta) are formed per chunk
 * of 1024 positions (positions ascending inside a thread, or lane i the positions i, i + 64, ... and the tree) as double partials
 * in bws and added chunk after chunk, sample after sample by a second launch; sums over channels run c ascending.
 * bws: rrl_pointnet_group_bwd_workspace_bytes(...) bytes, 8-byte aligned: two buffers of hmax N S doubles per sample, the chunk
 * partials and O(K + H^2) doubles per sample -- nothing K wide per position.  Refusals as the forward's (NULL arg / g_out / bws:
 * RRL_E_ARG; a short or misaligned ws or bws: RRL_E_WS); B == 0 returns 0. */
size_t rrl_pointnet_group_bwd_workspace_bytes(int B, int N, int S, int c0, int L, const int32_t *widths, const int32_t *groups);
int rrl_pointnet_group_bwd(const float *x, const float **params, const int32_t *widths, const int32_t *groups, const void *ws,
                           size_t ws_bytes, const int32_t *arg, const float *g_out, void *bws, size_t bws_bytes, float *d_x,
                           float **d_params, int B, int N, int S, int c0, int L, void *stream);

/* ---- DCP's multi-head attention: the transformer's core without the score matrix -------------
 * attention() inside MultiHeadedAttention.forward (dcp/model.py:27-34, 212-246): out = softmax(q k^T / sqrt(DK), dim = -1) v per
 * head.  Token-major, exactly as the nn.Linear projections leave it: q, out, g_out, d_q [B][N][H DK]; k, v, d_k, d_v
 * [B][M][H DK]; head h is channels h DK .. (h + 1) DK - 1 of a token's row -- the entries absorb the reference's
 * view(...).transpose(1, 2).contiguous() on the way in and out, no head-major copy exists.  count_q / count_kv: device int32
 * [B] or NULL (= N / M), clamped by the kernels to [0, N] / [0, M], never read on the host; rows and columns beyond them are
 * never read.  Plain device pointers, sizes and a stream: nothing is allocated, read back or synchronised, there are no
 * atomics, nothing is indexed by data, every launch goes to the caller's stream.
 *
 * The rule (v_mfma_f32_32x32x2_f32 is a float32 fmaf chain over its reduction index, bit for bit, as for rrl_pointer_fwd):
 *  1. z[j][k] = chain * sc: chain starts at +0 and runs over the head's channels c ascending, chain = fmaf(q[j][c], k[k][c],
 *     chain), ONE chain per score, never split over wavefronts or channel blocks; sc = float32(1 / sqrt(double(DK))), one
 *     float32 multiplication.  DK is padded with zero channels in BOTH operands up to 32, 64 or 128, the kernel's block (a
 *     zero step leaves a chain as it is, but for the sign of a zero).
 *  2. M_j = max_k z[j][k] over the columns below count_kv, taken in a first walk over ALL columns before any term is formed
 *     (fmaxf: a NaN score does not enter).  p[j][k] = expf(z - M_j), float32 from the float32 difference; a -inf score gives
 *     0 without forming -inf - (-inf).  L_j = sum_k p in double: a lane sums its columns ascending (columns 4 h .. 4 h + 3 of
 *     every eight, h = 0, 1), the two halves are then added.
 *  3. o[j][c] starts at +0 and runs over k = 0 .. count_kv - 1 ascending, o = fmaf(v[k][c], p[j][k], o): whole, the wavefront
 *     that owns row j walks every column and carries the accumulator; the columns that pad the last tile of 32 are zero in
 *     BOTH operands.  out[j][c] = float32(double(o) / L_j).  The score product therefore runs twice in the forward.  Rows at
 *     or beyond count_q, and every row when count_kv[b] == 0, are exactly 0.
 *  4. Backward, on z recomputed by the same chain (the same bits) and M_j, 1 / L_j (the reciprocal taken once per row, in
 *     double) kept in ws: delta_j = sum_c g[j][c] out[j][c] in double, c ascending; Pn = float32(double(expf(z - M_j)) (1 / L_j));
 *     dP[j][k] = the float32 chain over c ascending of g[j][c] v[k][c]; ds[j][k] = float32(double(Pn) (double(dP) - delta_j)
 *     double(sc)); d_v[k][c] = the chain over j ascending of g[j][c] Pn[j][k], d_q[j][c] the chain over k ascending of k[k][c]
 *     ds[j][k], d_k[k][c] the chain over j ascending of q[j][c] ds[j][k]: whole chains (one pass owns rows and writes d_q,
 *     one owns columns and writes d_k and d_v, each walks the other dimension entirely).  Rows and columns beyond the counts
 *     get zero gradient.  Every element of every output is written; nothing is pre-zeroed.
 * Two calls give the same bits; sample b of a ragged batch has the bits of its own B = 1 call.
 *
 * info (optional) [B]: 1 where a score or an output entry inside the counts is NaN or +-inf, else 0.  d_q, d_k, d_v: each may
 * be NULL; a pass that serves only NULL outputs is not launched.  The backward takes the forward's out.
 * ws: rrl_attention_workspace_bytes(B, H, N, M) bytes, 8-byte aligned: two doubles per (sample, head, row) -- M_j and
 * 1 / L_j, whose SIGN carries the row's info flag (L >= 1 or NaN; the backward takes the magnitude) --, independent of M and DK;
 * no array of size N M in either direction.  The backward takes the ws its forward filled.
 * Launches: forward 1, and 1 more when info is asked for; backward 1 per pass (the column pass 1 per output where DK > 64 is
 * odd or a tensor is not 16-byte aligned).
 * Refusals, on the host before any HIP call: RRL_E_ARG -- NULL q / k / v / ws / out (backward also g_out); B outside 0..32767;
 * H outside 1..16; DK outside 1..RRL_ATTENTION_MAX_DK; N or M outside 1..16384 --, then RRL_E_WS: a short or misaligned ws.
 * B == 0 returns 0 without a launch.
 * rrl_attention_scores writes z alone, [B][H][N][M], -inf at and beyond the counts, by the same chain: for tests and
 * endpoints, it is the only (B, H, N, M) array and nothing else reads it. */
#define RRL_ATTENTION_MAX_DK 128
size_t rrl_attention_workspace_bytes(int B, int H, int N, int M);
int rrl_attention_fwd(const float *q, const float *k, const float *v, const int32_t *count_q, const int32_t *count_kv, void *ws,
                      size_t ws_bytes, float *out, int32_t *info, int B, int H, int DK, int N, int M, void *stream);
int rrl_attention_bwd(const float *q, const float *k, const float *v, const int32_t *count_q, const int32_t *count_kv, void *ws,
                      size_t ws_bytes, const float *out, const float *g_out, float *d_q, float *d_k, float *d_v, int B, int H,
                      int DK, int N, int M, void *stream);
int rrl_attention_scores(const float *q, const float *k, const int32_t *count_q, const int32_t *count_kv, float *scores, int B,
                         int H, int DK, int N, int M, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RRL_H */
