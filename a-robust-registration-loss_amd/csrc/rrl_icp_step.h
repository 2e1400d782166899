// rrl_icp_step.h -- what the two point-to-point ICP loops share (rrl_icp_step_batch, rrl_icp_epoch, rrl_kabsch.hip;
// rrl_robust_step_batch, rrl_robust_icp_epoch, rrl_robust.hip; DESIGN.md sections 16 and 20): the pose step's one body, with
// the annealing rule of the robust loop as its compile-time variant, and, host code only, the step's refusals and the front
// of the epoch on include/rrl.h's rrl_icp_epoch_args.  Include after rrl_ws.h, rrl_pose_tail.h and rrl_cloud_epoch.h.
#pragma once

struct IcpStepArgs {
    const float *Rk, *Tk;
    const int32_t *info;
    const double *fit;
    float *R, *T;
    const float *tol_rot, *tol_trans;
    int patience;
    const float *value;
    float *table;
    long long *cursor, nrows;
    float *row, *last_step;
    int32_t *state;
    int B;
};

// what rrl_robust_step_batch adds: the per-pair scale and its end, the factor of a level's end, the cap of epochs at one
// scale, level [B][2] = (epochs at this scale, levels finished)
struct IcpAnneal {
    float *nu;
    const float *nu_end;
    float anneal;
    int level_cap;
    int32_t *level;
};

// The ICP pose step of pair blockIdx.x: one wavefront per pair, lane 0 works (se3_newton_step_kernel's shape; the state words
// and the stopping rule are rrl_pose_tail.h's PoseStop, [3] = the fit's status or RRL_POSE_DONE).  ANNEAL: the calm count ends
// a LEVEL of the scale nu, and the pair is done when a level ends at nu_end.
template <bool ANNEAL>
__device__ __forceinline__ void icp_step_one(const IcpStepArgs &a, const IcpAnneal &n) {
    const int b = blockIdx.x;
    if (b >= a.B || threadIdx.x != 0) return;
    const size_t s = (size_t)b;
    int32_t *__restrict__ st = a.state + s * 4;
    const double *__restrict__ fit = a.fit + s * RRL_FIT_DOUBLES;
    const int fstat = a.info[s * 4 + 1];
    PoseLog plog = {-1, (float)fit[RRL_FIT_RES], a.value ? a.value[s] : 0.0f};
    if (a.table && a.cursor) plog.at = a.cursor[s];
    PoseStop stop = pose_stop_load(st);
    int status = stop.done ? RRL_POSE_DONE : fstat;
    if (!stop.done && fstat == RRL_FIT_OK) {
        double Rk[3][3], Ro[3][3], Tk[3], To[3], ab[3];
        bool finite = true;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            Tk[i] = (double)a.Tk[s * 3 + i];
            To[i] = (double)a.T[s * 3 + i];
            ab[i] = fit[RRL_FIT_ABAR + i];
            finite = finite && fabs(Tk[i]) < (double)INFINITY;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                Rk[i][j] = (double)a.Rk[s * 9 + 3 * i + j];
                Ro[i][j] = (double)a.R[s * 9 + 3 * i + j];
                finite = finite && fabs(Rk[i][j]) < (double)INFINITY;
            }
        }
        if (!finite) {
            status = RRL_FIT_DEGENERATE;
        } else {
            // E = R^T Rk: the rotation from the old pose to the new; angle = atan2(|vee(E - E^T)| / 2, (tr E - 1) / 2)
            double E[3][3];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) E[i][j] = (Ro[0][i] * Rk[0][j] + Ro[1][i] * Rk[1][j]) + Ro[2][i] * Rk[2][j];
            const double vx = E[2][1] - E[1][2], vy = E[0][2] - E[2][0], vz = E[1][0] - E[0][1];
            const double ang = atan2(0.5 * sqrt((vx * vx + vy * vy) + vz * vz), 0.5 * (((E[0][0] + E[1][1]) + E[2][2]) - 1.0));
            double mv2 = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double now = ((ab[0] * Rk[0][k] + ab[1] * Rk[1][k]) + ab[2] * Rk[2][k]) + Tk[k];
                const double was = ((ab[0] * Ro[0][k] + ab[1] * Ro[1][k]) + ab[2] * Ro[2][k]) + To[k];
                mv2 += (now - was) * (now - was);
            }
            const double mv = sqrt(mv2);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                a.T[s * 3 + i] = a.Tk[s * 3 + i];
#pragma unroll
                for (int j = 0; j < 3; ++j) a.R[s * 9 + 3 * i + j] = a.Rk[s * 9 + 3 * i + j];
            }
            pose_stop_update(stop, s, (float)ang, (float)mv, a.last_step, a.tol_rot, a.tol_trans, a.patience);
        }
    }
    if (ANNEAL && !stop.done) {  // the annealing rule decides what the calm count means
        int32_t *__restrict__ lv = n.level + s * 2;
        int at_nu = lv[0] + 1, levels = lv[1];
        stop.done_new = -1;
        if ((a.patience > 0 && stop.calm >= a.patience) || (n.level_cap > 0 && at_nu >= n.level_cap)) {
            const float nu = n.nu[s], end = n.nu_end[s];
            if (nu > end) {
                const float next = nu * n.anneal;
                n.nu[s] = next > end ? next : end;
                stop.calm = 0;
                at_nu = 0;
                levels += 1;
            } else {
                stop.done_new = stop.epochs;
            }
        }
        lv[0] = at_nu;
        lv[1] = levels;
    }
    pose_stop_store(stop, status, st);
    pose_log_store(plog, fstat == RRL_FIT_OK, a.table ? a.table + s * 3 : nullptr, 3ll * a.B, a.nrows, a.cursor ? a.cursor + s : nullptr,
                   a.row ? a.row + s * 3 : nullptr);
}

// ---------------------------------------------------------------------------------------
// Host code only.  An epoch asks cloud_epoch_front_ok, icp_step_args_ok with its fit's alignment and its own RRL_E_ARG checks,
// then icp_epoch_ws_ok, and only then launches: every refusal before the first launch, RRL_E_ARG first.
// ---------------------------------------------------------------------------------------
// the step's refusals, shared with the epochs
static inline bool icp_step_args_ok(const float *Rk, const float *Tk, const int32_t *info, const double *fit, const float *R, const float *T,
                                    const int32_t *state, int patience, const float *tol_rot, const float *tol_trans) {
    if (!Rk || !Tk || !info || !fit || !R || !T || !state) return false;
    return pose_stop_args_ok(patience, tol_rot, tol_trans);
}

// RRL_E_WS: the Chamfer walk's scratch and the fit's partial rows
static inline bool icp_epoch_ws_ok(const rrl_icp_epoch_args *a) {
    return cloud_epoch_cham_ws_ok(a) && a->part_bytes >= rrl_kabsch_part_bytes(a->B, a->N);
}

// the fit of the source as given onto its keyed partners, weights w (NULL: all 1), into (Rk, Tk, fit, info)
static inline int icp_epoch_fit(const rrl_icp_epoch_args *a, const float *w, void *stream) {
    rrl_kabsch_args k = {};
    k.struct_bytes = (int32_t)sizeof(k);
    k.B = a->B; k.n = a->N; k.m = a->M; k.a_stride = 3; k.b_stride = 3; k.transpose_r = 0;
    k.a = a->src; k.b = a->tar; k.w = w; k.keys = a->best_x; k.count_a = a->count1; k.count_b = a->count2; k.gate_sq = a->gate_sq;
    k.eps_w = a->eps_w; k.rank_tol = a->rank_tol;
    k.part = a->part; k.part_bytes = a->part_bytes; k.R = a->Rk; k.T = a->Tk; k.fit = a->fit; k.info = a->info;
    return rrl_kabsch_fwd(&k, stream);
}
