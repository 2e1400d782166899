// rrl_stage_args.h -- the kernel argument structs of the stages behind the scan, next to each other: what rrl_sparse.hip's
// argument fillers fill and the kernels of rrl_stage_{pair,reduce,tail,bwd}.h take by value.  Plain data, no code.
#pragma once
#include "rrl_common.h"

// K2, the per-line stage (rrl_stage_pair.h: line_pair_dist_kernel, pair_count_kernel, the single-tile kernels)
struct PairArgs {
    const float *tri1, *tri2, *line;  // the triangles of both clouds (raw 36-byte rows: st1 = st2 = 9), the lines
    const int32_t *count1, *hit1, *count2, *hit2;
    uint8_t *kj;
    int32_t *sel_out, *nsel, *hs1, *hs2;
    float *w1, *w2;
    float4 *Q1, *Q2;
    float *D, *dc;
    uint8_t *kjc;
    uint32_t *lidc;          // line | kj << 24 at the compact slot (or NULL)
    float *vlist;            // [B][ntile][16384] dense list of the tile's valid D values (with mhist; or NULL)
    int32_t *vlcnt;
    int32_t *blkcnt;
    uint32_t *mhist, *mctl;  // tiled reduce: per-sample histogram of the D values' top 11 bits, bucket counts (or NULL)
    int B, N, M, L, s_m, s_n, e_m, e_n, st1, st2;
    int Bt;  // multi-pose evaluation (rrl_opts.problems): tri2, line and cloud 2's scan (count2, hit2) of instance b are those
             // of problem b % Bt; 0: every instance has its own
    int xcd_align;  // line_pair_dist_kernel: sample b's workgroups on XCD b % 8 (xcd_sample_of; B % 8 == 0)
    int32_t *zc1, *zc2;  // chained steps (include/rrl.h RRL_F_CHAIN): COUNT1 / COUNT2 again, writable -- every lane zeroes its
                         // line's two counts behind its own read, so that the NEXT step's scan finds them cleared; or NULL
};

// the count pass of the next epoch's line sampler, riding in the per-line launch (pair_count_kernel; rrl_ws.h RrlCountRider)
struct CountKArgs {
    const unsigned long long *rng_state;
    const float *r, *centers, *aabb2, *rows;
    unsigned long long *accept;
    int n_rows, n, rounds, prefilter, gx, gy;
};

// K3 + K4 by one workgroup per sample (rrl_stage_reduce.h: loss_reduce_kernel, the single-tile kernels)
struct ReduceArgs {
    const uint8_t *kjc;
    const float *dc;
    const int32_t *blkcnt;
    float *med_out;
    int32_t *bcnt_out;
    int64_t *bsum_out;
    int32_t *info;
    float *loss;
    const int32_t *status;
    int B, nblk, s_m, s_n, e_m, e_n, pool;
};

// K3 + K4 by the exchange reduce (rrl_stage_reduce.h: loss_reduce_tiled_kernel)
struct TiledArgs {
    const uint8_t *kjc;
    const float *dc;
    const int32_t *blkcnt;
    uint32_t *mhist, *mctl, *mcand;
    unsigned long long *msum;
    float *med_out;
    int32_t *bcnt_out;
    int64_t *bsum_out;
    int32_t *info;
    float *loss;
    int32_t *status;      // [0] the scan's NaN flag (read); [2] += samples repaired after a hand-off time-out
    int B, nblk, s_m, s_n, e_m, e_n;
    unsigned spin_limit;  // polls before a waiting workgroup gives up (rrl_set_spin_limit: tests set 0)
    int xcd_align;        // sample b's workgroups on XCD b % 8 (xcd_sample_of; B % 8 == 0): its in-launch hand-offs stay in one L2
    float *payload;       // != NULL (rrl_loss_step_ex): the sample's last workgroup adds its loss to payload[0 .. 1] (tail_payload)
    uint32_t *chain;      // chained steps (include/rrl.h RRL_F_CHAIN), as TailArgs: the CHAIN words the sample's last workgroup zeroes
    int chain_flags;      //   (or NULL); != 0: this step's scan ran in the fused launch -- NaN flag / time-outs are CHAIN[b][NAN], [TIMEOUT]
};

// K3 + K4 (+ K5) by the tail kernel (rrl_stage_tail.h: loss_tail_kernel, tail_write_kernel)
struct TailArgs {
    const uint32_t *lidc;
    const float *dc;
    const float *vlist;
    const int32_t *vlcnt;
    const int32_t *blkcnt;
    const uint32_t *mhist;
    uint32_t *mctl;
    unsigned long long *msum;
    float *med_out;
    int32_t *bcnt_out;
    int64_t *bsum_out;
    int32_t *info;
    float *loss;
    const int32_t *status;
    int B, nblk, s_m, s_n, e_m, e_n;
    int do_bwd, N, L, transpose_r;
    const int32_t *hs1;
    const float *w1;
    const float4 *Q1, *Q2;
    const float *grad_loss, *src;
    float *gR, *gt, *payload;
    float *grad_tri1;  // != NULL: the backward SCATTERS dL/dpoints1 [B][N][9] (rrl_loss_step) instead of summing (dR, dt)
    int Bt;            // multi-pose (rrl_opts.problems): src has Bt entries, instance b is a pose of entry b % Bt; 0: its own
    int xcd_align;     // sample b's workgroups on XCD b % 8 (xcd_sample_of; B % 8 == 0)
    // chained steps (include/rrl.h RRL_F_CHAIN): the CHAIN words [B][RRL_CHAIN_WORDS], which the sample's last workgroup zeroes
    // on exit (or NULL); chain_flags != 0: this step's scan ran in the fused launch -- its NaN flag and time-outs are
    // CHAIN[b][RRL_CHAIN_NAN], CHAIN[b][RRL_CHAIN_TIMEOUT], not STATUS[0]
    uint32_t *chain;
    int chain_flags;
};

// the write pass of the next epoch's line sampler, riding in the tail kernel's or the direct backward's launch
// (tail_write_kernel, bwd_write_kernel; rrl_ws.h RrlWriteRider)
struct WriteKArgs {
    unsigned long long *rng_state;
    const float *r, *centers;
    const unsigned long long *accept;
    float *lines;
    int32_t *filled;
    int n, rounds, gx, gy;
};

// K5, the scatter backward to the points (rrl_stage_bwd.h: loss_bwd_kernel, scatter_fix_to_float_kernel, pair_reduce_scatter_kernel)
struct ScatArgs {
    const uint32_t *lidc;
    const int32_t *blkcnt, *hs1, *hs2, *bcnt, *info;
    const float *w1, *w2, *D, *med, *grad_loss;
    const float4 *Q1, *Q2;
    float *g1, *g2;
    int N, M, L;
    unsigned long long *fx;  // deterministic mode: GFIX -- [B][N + M][9] fixed-point accumulators, then int32 [B][2] non-finite flags; or NULL
    int fxbits;              // ... fractional bits below the sample's bound exponent (scat_unit_exp)
    int fxB;                 // ... samples (the flags sit behind the B accumulators)
};

// K5', the direct backward to (dR, dt) with the sampler's write pass riding along (rrl_stage_bwd.h: bwd_write_kernel)
struct BwdKArgs {
    const uint8_t *kj;
    const int32_t *sel, *nsel, *hs1;
    const float *w1;
    const float4 *Q1, *Q2;
    const float *D, *med;
    const int32_t *bcnt, *info;
    const float *grad_loss, *src;
    float *gR, *gt, *payload;
    const float *loss;
    int B, N, L, transpose_r;
    float *part;
    int gx;
};

// ... and riding in the single-tile kernel's launch (rrl_stage_bwd.h: pair_reduce_bwd_kernel)
struct SoloBwd {
    const uint8_t *kj;
    const int32_t *sel, *nsel, *hs1, *bcnt, *info;
    const float *w1, *D, *med, *grad_loss, *src, *loss;
    const float4 *Q1, *Q2;
    float *gR, *gt, *payload;
    uint32_t *mctl;
    int B, N, L, transpose_r;
    int Bt;  // multi-pose (rrl_opts.problems)
};
