#!/usr/bin/env python3
"""bench.py -- BASELINE.json's metric on MI355X: point-pairs/sec for the intersected-line loss
fwd+bwd at B=8, N=M=4096 (L=10000 lines, the RPM call-site default), per GPU.

One "step" (the timed one) = SURVEY.md section 8(d)'s definition, exactly: rigid apply of the source
pseudo-triangles -> S (line<->triangle scan of both clouds) -> P (per-line distances) -> median +
Welsch reduce -> backward to points1.grad (B, N, 9) -- what code/loss.py:170-232 + autograd delivers --
issued as ONE C call per step (ops.LossStep -> rrl_loss_step_ex; four launches with prepared orders,
five cold), followed by one all-reduce of the 14-float shard payload [loss sum, valid count, 0 x 12]
over the ranks (points1.grad stays local).  Inputs are resident in HBM before the timed
region.  pairs per step = B * L * 3 * (N + M) per GPU -- DENSE-EQUIVALENT pairs: the culled scan
decides every one of them exactly but evaluates ~1 %; value = all ranks' pairs / max time over ranks.

`config.workload` says whether the step is PREPARED (default: the k-d order of each cloud was computed
once, outside the timed region -- rrl_cloud_order, config.prepare_us -- as a training loop does per
dataset item; a target that has not moved keeps its records) or COLD (--cold: records + cell sort +
tree of both clouds in every step).  With --full, whichever one is timed, the other is measured right after
on the same inputs and printed at top level (`value_cold` / `ms_per_step_cold`, or `value_prepared` / ...):
round-over-round comparisons of rounds 1-3 must use the cold number.

A plain run does only what the headline needs: it makes the workload, warms up, times the K steps, writes
the last timed step's outputs if --dump-outputs DIR is given, and prints the line.  Its `extras` hold the
timed step's own payload (`loss_sum`, `valid`) and nothing that takes a run of its own.

--dump-outputs DIR: after the timed steps, what the last one computed -- what a caller of ops.LossStep
receives -- as DIR/<name>.npy (float32 / float64): loss (B,), points1_grad (B, N, 9), info (B, 4) and the
all-reduced payload (14,); with more than one rank every rank writes its own shard as <name>.rank<r>.npy.
A points1_grad beyond DUMP_GRAD_BYTES is written as a seeded sample of its rows (points1_grad_rows.npy).
The inputs are seeded: the same arguments give the same inputs in every run.

With --full, measured in the same run, outside the timed region, in the same JSON line:
  * `variants.fused_dRdT`: the fused TRAINING op (ops.RegistrationStep: backward straight to (dR, dT),
    the headline of rounds 3-4); `variants.points1_grad_autograd`: section 8(d) through the drop-in
    callables chained by autograd (hipGraph replay); `variants.dropin_loop`: the reference trainers'
    LITERAL per-sample loop (rpm/Train_RPM.py:226-231), eager, one host read-back per call;
  * `roofline`: the DOMINANT KERNEL OF THE TIMED STEP, cull_scan_kernel: launch time by HIP events on
    the launch stream (this run) AND rocprof's average of the committed profile of this build
    (`launch_ms_rocprof`, `frac_rocprof`), the arithmetic it EXECUTED (in-kernel counters) against the
    non-FMA fp32 VALU peak, issue-side fraction and HBM traffic from the committed PMC pass;
    `roofline.at_B64` = the same figures at a CHIP-FILLING shape (BASELINE configs[2] as one batch on
    one GPU); `roofline.dense_reference` = the strict scan (all 18 counted flops per pair);
  * `cpu_baseline`: the reference-equivalent torch-eager formulation on the host cores (SURVEY 8(d)'s
    stated baseline), the C/OpenMP port nested as `c_port`; bounded samples of the same workload.
Weak scaling by default (B = 8 per GPU); --global-batch 64 fixes the total (BASELINE configs[2]).

    python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...
"""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(ROOT, "a-robust-registration-loss_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

FLOPS_PER_PAIR = 18          # 3 sub, 3+3+1 mul, 2+2+1 add, 1 sub, 1 sqrt-class
VALU_PEAK_TFLOPS = 78.6      # 157.3 TFLOP/s fp32 vector peak counts FMA as 2 flops; this path is
                             # contraction-off mul/add (one flop per lane-op) -> half of it
HBM_PEAK_GBS = 8000.0
# arithmetic of one test of the culled scan, in lane-ops (an FMA counted once, like every VALU op):
# sphere test = 3 sub + 3 (dot) + 3 (|a|^2) + 2 fma + add + mul = 12 (compares excluded); exact test = dist_sq's 16;
# a resolved candidate = points 1 and 2; a fallback pair = 3 points
OPS_SPHERE, OPS_EXACT, OPS_CAND, OPS_FALLBACK = 12, 11, 48, 48  # level-D prefilter: 10 FMA-chain ops + sign; candidate: 3 exact points
# --dump-outputs stays under 64 MB over all ranks: points1_grad beyond this is sampled by rows (their float64 indices: 2/9 more)
DUMP_GRAD_BYTES = 48 << 20


def csrc_sha():
    """Hash of the kernel sources: profile-derived numbers (HBM traffic from PMC passes) are only
    attached to the line when they were collected for exactly this build."""
    h = hashlib.sha256()
    d = os.path.join(PKG, "csrc")
    for f in sorted(x for x in os.listdir(d) if x.endswith((".hip", ".h", ".inc"))) + ["../../include/rrl.h"]:
        h.update(open(os.path.join(d, f), "rb").read())
    try:  # an experimental build (RRL_HIPCC_FLAGS) names its flags in the version string: another hash
        from rrl_hip import _lib
        ver = _lib.load().rrl_version()
        if b"[" in ver:
            h.update(ver)
    except Exception:
        pass
    return h.hexdigest()[:16]


def make_workload(B, N, M, L, rank, dev):
    import loss as Lmod
    from rrl_hip import synth
    tri1, tri2, src, tar, rad, ctr = [], [], [], [], [], []
    for b in range(B):
        pr = synth.make_pair(1000 * rank + b, N, M)
        tri1.append(pr["src_tri"]); tri2.append(pr["tar_tri"]); src.append(pr["src"])
        tar.append(pr["tar"]); rad.append(pr["radius"]); ctr.append(pr["center"])
    to = lambda a: torch.from_numpy(np.stack(a)).to(dev)  # noqa: E731
    w = dict(tri1=to(tri1), tri2=to(tri2), src=to(src), tar=to(tar))
    w["radius"], w["center"] = torch.tensor(rad).reshape(B, 1), torch.from_numpy(np.stack(ctr))
    torch.manual_seed(1000 * rank)  # CPU seed selects the sampler's uniform streams
    t0 = time.perf_counter()
    w["lines"] = Lmod.Random_uniform_distribution_lines_batch_efficient_resample(
        w["radius"], w["center"], L, w["src"], w["tar"], dev)
    torch.cuda.synchronize()
    w["sample_s"] = time.perf_counter() - t0
    # per-sample "predicted" transforms (what RPM/DCP/FMR hand to the loss): small rotations
    gen = torch.Generator().manual_seed(7 + rank)
    from LieAlgebra import se3
    R, T = se3.exp3(0.05 * torch.randn(B, 6, generator=gen))
    w["R"], w["T"] = R.to(dev).requires_grad_(True), T.to(dev).requires_grad_(True)
    return w


def cpu_baseline(N, M, L, budget_s=12.0, eager_budget_s=8.0):
    """Two CPU legs on bounded samples of the same workload, host cores of this box:
    (top level) oracle/torch_eager.py: the reference's own op sequence (materialised (L, N, 3, 3)
        temporaries, per-bucket gathers, autograd backward; code/loss.py:68-232) in torch CPU ops on a line
        subset of one sample sized to ~eager_budget_s -- SURVEY 8(d)'s stated baseline;
    (`c_port`) oracle/rrl_oracle.c (C, OpenMP over lines): whole samples of N=M, L lines, fwd+bwd, until
        ~budget_s seconds are spent."""
    from oracle import rrl_oracle, torch_eager
    from rrl_hip import synth
    rrl_oracle.build()
    cores = os.cpu_count() or 1
    pr = synth.make_pair(500, N, M)
    rands = synth.uniform_streams(0, 3, L)
    lines = rrl_oracle.resample_lines(rands, pr["radius"], pr["center"], pr["src"], pr["tar"], L)
    done, spent = 0, 0.0
    while spent < budget_s:
        t0 = time.perf_counter()
        ref = rrl_oracle.loss(pr["src_tri"], pr["tar_tri"], lines, want_grad=True)
        spent += time.perf_counter() - t0
        done += 1
    pairs = done * L * 3 * (N + M)
    c_port = {"value": pairs / spent, "unit": "point-pairs/s", "cores": cores, "kind": "port",
              "formulation": "oracle/rrl_oracle.c: fused C restatement (nothing of size L x N materialised), OpenMP over lines",
              "sample": f"{done} evaluation(s) of one N=M={N}, L={L} sample, loss fwd+bwd, oracle/rrl_oracle.c "
                        f"(fused C restatement) with OpenMP on {cores} threads, {spent:.1f} s"}
    try:
        # torch's intra-op pool degrades badly beyond a few dozen threads on these small per-chunk ops
        # (profiles/r02_torch_eager_threads.txt: 256 lines take 0.02 s on 32 threads, 0.2 s on 128, 29 s on 256)
        eth = min(cores, 32)
        torch.set_num_threads(eth)
        t2 = torch.from_numpy(pr["tar_tri"])
        ln = torch.from_numpy(lines)

        def run(nl):
            t1 = torch.from_numpy(pr["src_tri"]).clone().requires_grad_(True)
            t0 = time.perf_counter()
            val = torch_eager.loss(t1, t2, ln[:nl], max_lines=64)
            if val is not None:
                val.backward()
            return time.perf_counter() - t0, val
        probe = min(L, 256)
        tp, _ = run(probe)
        nl = int(max(probe, min(L, probe * eager_budget_s / max(tp, 1e-3))))
        te, val = run(nl)
        return {"value": nl * 3 * (N + M) / te, "unit": "point-pairs/s", "cores": eth, "kind": "port",
                "formulation": "torch-eager: the reference's own op sequence (code/loss.py:68-232) in torch CPU ops + autograd, "
                               "evaluated in CHUNKS of 64 lines (cache-resident temporaries; the reference materialises the whole "
                               "(L, N, 3, 3) tensors at once and is slower: BASELINE.md ~14 s per sample on 8 cores) -- the chunking "
                               "errs in the CPU's favour",
                "chunk_lines": 64,
                "sample": f"one N=M={N} sample, first {nl} of its {L} lines, loss fwd+bwd by autograd, "
                          f"oracle/torch_eager.py (the reference's materialising op sequence, code/loss.py:68-232) "
                          f"with torch.set_num_threads({eth}) (of {cores} host threads), {te:.1f} s",
                "loss_full_sample_c_port": float(ref["loss"]) if ref["loss"] is not None else None,
                "c_port": c_port}
    except Exception as exc:  # the C leg stands on its own
        out = dict(c_port)
        out["torch_eager_error"] = f"{type(exc).__name__}: {exc}"
        out["c_port"] = c_port
        return out


def parity_in_run(w, Rd, Td, moved_gpu, loss, grad, info, samples):
    """The TIMED object against the oracle on the TIMED workload, for the given samples:
    (W, G on identical inputs) the oracle evaluates code/loss.py:170-232 + the closed-form gradient on the triangles the timed
        step itself moved (its TRI1 field): loss (rel 1e-5), the selected-line / D-value / bucket counts (EXACT: every label of
        the 2 x L x N scan enters them), points1.grad per POINT (1e-4; sums over the rows that hold the same 3-D point:
        independent of tie-breaks between duplicate pseudo-triangles, SURVEY hard part 3);
    (T) the step's moved triangles against the oracle's own rigid apply x R^T + t (unfused mul/add; the kernel uses FMAs):
        max abs difference relative to the cloud's extent (a few 1e-8: one rounding);
    (end to end, reported, not gated) the oracle on ITS OWN moved triangles: a 1-ulp different input flips the few labels that
        sit on a threshold (fragments 2e-4).
    Checker only: outside the timed region."""
    from oracle import rrl_oracle
    rrl_oracle.build()
    out = {"samples": list(samples), "loss_rel_max": 0.0, "grad_per_point_rel_max": 0.0, "labels_equal": True,
           "rigid_apply_rel_max": 0.0, "per_sample": []}
    t0 = time.perf_counter()
    for b in samples:
        src = w["tri1"][b].cpu().numpy()
        tar, lines = w["tri2"][b].cpu().numpy(), w["lines"][b].cpu().numpy()
        moved = moved_gpu[b].cpu().numpy().reshape(-1, 9)
        ref = rrl_oracle.loss(moved, tar, lines, want_grad=True)
        mine_loss, mine_info = float(loss[b]), [int(v) for v in info[b].tolist()]
        rel = abs(mine_loss - float(ref["loss"])) / max(abs(float(ref["loss"])), 1e-30) if ref["loss"] is not None else float("nan")
        same = mine_info[:3] == [ref["n_buckets"], ref["n_selected"], ref["n_values"]] and bool(mine_info[3]) == bool(ref["nan"])
        _, inv = np.unique(moved.reshape(-1, 3), axis=0, return_inverse=True)
        a_, b_ = np.zeros((inv.max() + 1, 3)), np.zeros((inv.max() + 1, 3))
        np.add.at(a_, inv.reshape(-1), grad[b].cpu().numpy().astype(np.float64).reshape(-1, 3))
        np.add.at(b_, inv.reshape(-1), np.asarray(ref["grad1"], np.float64).reshape(-1, 3))
        grel = float(np.abs(a_ - b_).max() / max(np.abs(b_).max(), 1e-30))
        moved_o = rrl_oracle.rigid_apply(src.reshape(-1, 3), Rd[b].cpu().numpy(), Td[b].cpu().numpy(), transpose_r=True).reshape(-1, 9)
        trel = float(np.abs(moved_o - moved).max() / max(np.abs(moved_o).max(), 1e-30))
        e2e = rrl_oracle.loss(moved_o, tar, lines, want_grad=False)
        out["loss_rel_max"] = max(out["loss_rel_max"], rel)
        out["grad_per_point_rel_max"] = max(out["grad_per_point_rel_max"], grel)
        out["rigid_apply_rel_max"] = max(out["rigid_apply_rel_max"], trel)
        out["labels_equal"] = out["labels_equal"] and same
        out["per_sample"].append({"sample": b, "loss": mine_loss, "oracle_loss": float(ref["loss"]), "info": mine_info,
                                  "oracle_counts": [ref["n_buckets"], ref["n_selected"], ref["n_values"], int(ref["nan"])],
                                  "end_to_end": {"oracle_loss_on_its_own_rigid_apply": float(e2e["loss"]) if e2e["loss"] is not None else None,
                                                 "counts": [e2e["n_buckets"], e2e["n_selected"], e2e["n_values"]],
                                                 "loss_rel": abs(mine_loss - float(e2e["loss"])) / abs(float(e2e["loss"])) if e2e["loss"] else None}})
    out["seconds"] = time.perf_counter() - t0
    out["tolerances"] = {"loss_rel": 1e-5, "grad_per_point_rel": 1e-4, "counts": "exact", "rigid_apply_rel": 1e-6}
    out["ok"] = bool(out["labels_equal"] and out["loss_rel_max"] <= 1e-5 and out["grad_per_point_rel_max"] <= 1e-4 and
                     out["rigid_apply_rel_max"] <= 1e-6)
    out["what"] = ("oracle/rrl_oracle.c (pinned to the reference's fixtures, tests/test_oracle_golden.py) on samples of the TIMED "
                   "workload: W + G on the triangles the timed step moved (identical inputs: counts exact, loss 1e-5, per-point "
                   "gradient 1e-4), T against the oracle's unfused rigid apply (1e-6 of the extent), and -- reported -- the oracle "
                   "end to end on its own moved triangles")
    return out


def scan_roofline(ops, run_step, B, N, M, L, launches=20, counters=True):
    """Figures of the culled scan's launch inside `run_step()` (a callable that issues one step directly on the current
    stream): HIP-event launch time on the launch stream (mean over `launches`, first two dropped), and -- from the
    instrumented instantiation of the kernel, one extra launch -- the arithmetic it executed."""
    ops.scan_timing(1)
    for _ in range(launches):
        run_step()
    torch.cuda.synchronize()
    t = ops.scan_timing_collect()
    ops.scan_timing(0)
    ms = float(np.mean(t[2:] if len(t) > 4 else t))
    out = {"launch_ms": ms, "launches_timed": len(t)}
    dense_flops = FLOPS_PER_PAIR * B * L * 3 * (N + M)
    if counters:
        ops.scan_counters(True)
        run_step()  # one launch: every wavefront writes its row of counters
        torch.cuda.synchronize()
        c = ops.scan_counters(False).cpu().numpy().astype(np.float64)
        exe = OPS_SPHERE * (c[0] + c[1]) + OPS_EXACT * c[3] + OPS_CAND * c[4] + OPS_FALLBACK * c[7]  # c[2] counts survivors, not tests
        out.update({
            "executed_flops": exe, "achieved": exe / (ms * 1e-3) / 1e12,
            "frac": exe / (ms * 1e-3) / 1e12 / VALU_PEAK_TFLOPS,
            "work_ratio": dense_flops / exe,
            "dense_equivalent_tflops": dense_flops / (ms * 1e-3) / 1e12,
            "counters_per_launch": {"sphere_tests_A": c[0], "half_sphere_tests_B": c[1], "halves_passed": c[2],
                                    "point0_prefilter_tests": c[3], "candidates_resolved": c[4], "wavefronts": c[5],
                                    "fallback_wavefronts": c[6], "fallback_pairs": c[7]}})
    return out


def attach_pmc(roof, B, N, L, mode):
    """PMC-derived figures (HBM bytes, VALU instructions, rocprof's average duration per launch) -- only when the committed
    pass (profiles/scan_hbm_traffic.json) was collected for exactly this build."""
    pmc = None
    pmc_file = os.path.join(ROOT, "profiles", "scan_hbm_traffic.json")
    if os.path.exists(pmc_file):
        rec = json.load(open(pmc_file))
        ent = rec.get(f"B{B}_N{N}_L{L}_{mode}")
        if ent and rec.get("csrc_sha") == csrc_sha():
            pmc = ent
    roof["traffic"] = pmc.get("bytes") if pmc else None
    roof["traffic_detail"] = pmc
    s_ = roof["launch_ms"] * 1e-3
    if pmc and pmc.get("sq_insts_valu"):
        roof["issue_frac"] = pmc["sq_insts_valu"] * 64 / s_ / 1e12 / VALU_PEAK_TFLOPS
        roof["pmc"] = {k: pmc[k] for k in pmc if k.startswith("sq_") or k == "rocprof_avg_us"}
    else:
        roof["issue_frac"] = None
    # the same fraction against rocprof's own average duration of the kernel (the HIP-event figure brackets the launch on
    # the stream: it includes the launch's start-up; rocprof times the kernel's execution)
    avg_us = pmc.get("rocprof_avg_us") if pmc else None
    roof["launch_ms_rocprof"] = avg_us * 1e-3 if avg_us else None
    if avg_us and roof.get("executed_flops"):
        roof["frac_rocprof"] = roof["executed_flops"] / (avg_us * 1e-6) / 1e12 / VALU_PEAK_TFLOPS
        if pmc.get("sq_insts_valu"):
            roof["issue_frac_rocprof"] = pmc["sq_insts_valu"] * 64 / (avg_us * 1e-6) / 1e12 / VALU_PEAK_TFLOPS
    else:
        roof["frac_rocprof"] = None
    return roof


def main():
    # ONE JSON line on stdout is the contract: RCCL prints a version banner to fd 1 when a communicator
    # comes up (and libraries may print whatever they like), so everything but the final line goes to stderr
    real_stdout = os.dup(1)
    os.dup2(2, 1)
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=300)  # ~65 us each: the closing fence costs ~3 us/step at 30
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=8, help="samples per GPU (weak scaling)")
    ap.add_argument("--global-batch", type=int, default=0,
                    help="total samples over all GPUs (strong scaling, BASELINE configs[2]: 64); overrides --batch")
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--lines", type=int, default=10000)
    ap.add_argument("--mode", default=os.environ.get("RRL_SCAN_MODE", "cull"))
    ap.add_argument("--reducer", default=os.environ.get("RRL_REDUCER", "auto"),
                    choices=["auto", "inline", "overlap", "torch"],
                    help="all-reduce of the shard payload: a node of the step's stream (inline), overlapped "
                         "with the next step on a second stream (overlap), torch.distributed (torch); auto "
                         "measures inline vs overlap during warm-up when there is more than one rank")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-parity", action="store_true", help="skip parity_in_run (the oracle's check of the timed workload)")
    ap.add_argument("--no-graph", action="store_true", help="never replay a hipGraph")
    ap.add_argument("--issue", choices=["auto", "graph", "direct"], default="auto",
                    help="how the step's launches are issued: the C call of ops.LossStep on the stream (direct), or one "
                         "hipGraph replay of it; auto measures both in warm-up")
    ap.add_argument("--no-extras", action="store_true", help="skip the variant / strict / counter / B=64 passes")
    ap.add_argument("--no-fresh", action="store_true", help="skip variants.fresh_lines / fresh_clouds_cold")
    ap.add_argument("--no-other", action="store_true",
                    help="skip the other build of the step (value_cold / value_prepared): profiling passes want the timed "
                         "step's kernels only")
    ap.add_argument("--no-b64", action="store_true", help="skip roofline.at_B64 (64 synthetic pairs take ~20 s to make)")
    ap.add_argument("--cold", action="store_true",
                    help="time the COLD step: no prepared orders, every step sorts both clouds (records + cell sort + tree)")
    ap.add_argument("--no-dist", action="store_true",
                    help="single process without a process group (default: even a plain 1-GPU run creates a 1-rank "
                         "RCCL group, so that the timed step carries the same all-reduce as N > 1)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also run every auxiliary measurement and check (host time, parity_in_run, "
                         "the other build, fresh-input loops, roofline, variants, extras, B=64, CPU baseline); the --no-* "
                         "options above select among them")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed as DIR/<name>.npy (loss, points1_grad, info, payload)")
    args = ap.parse_args()
    if "RANK" not in os.environ and not args.no_dist and args.gpus == 1:
        # not under torchrun: a standalone 1-rank group on a free local port
        import socket
        with socket.socket() as so:
            so.bind(("127.0.0.1", 0))
            port = so.getsockname()[1]
        os.environ.update(RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))

    from rrl_hip import dist as rdist, ops
    import loss as Lmod
    try:
        rank, world, local = rdist.init_from_env()
    except Exception as exc:  # no usable RCCL / rendezvous for the standalone group: measure without one
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise
        print(f"[bench] process group unavailable ({type(exc).__name__}: {exc}); running without one", file=sys.stderr)
        rank, world, local = 0, 1, 0
    if world != args.gpus and world > 1:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    strong = args.global_batch > 0
    if strong:
        lo, hi = rdist.shard_bounds(args.global_batch, rank, world)
        B = hi - lo
        if B <= 0:
            raise SystemExit("--global-batch smaller than the number of ranks")
    else:
        B = args.batch
    N, M, L = args.points, args.points, args.lines
    w = make_workload(B, N, M, L, rank, dev)
    Rd, Td = w["R"].detach(), w["T"].detach()
    ones = torch.ones(B, device=dev)
    # Prepared clouds (include/rrl.h rrl_cloud_order): the spatial order of each cloud is computed ONCE, outside the
    # timed region -- as a training loop does per dataset item and the demo at its start (the reference's callers move
    # the same source against a fixed target, rpm/Train_RPM.py:207-231) -- and every step runs the prepared build.
    can_prepare = args.mode == "cull"
    prepared = can_prepare and not args.cold
    order1 = order2 = None
    prepare_us = None
    if can_prepare and not args.full:
        order1, order2 = ops.cloud_order(w["tri1"]), ops.cloud_order(w["tri2"])
    elif can_prepare:
        ops.cloud_order(w["tri1"])  # (first call: scratch allocation, code load)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(5):
            order1, order2 = ops.cloud_order(w["tri1"]), ops.cloud_order(w["tri2"])
        torch.cuda.synchronize()
        prepare_us = (time.perf_counter() - t0) / 5 / 2 * 1e6  # per call = per B clouds of N triangles

    def loss_step(prep):
        """SURVEY 8(d) by direct issue: ops.LossStep (rigid apply + loss + backward to points1.grad, one C call) with the
        shard payload [loss sum, valid count, 0 x 12] in its workspace."""
        return ops.LossStep(w["tri1"], w["tri2"], L, transpose_r=True, mode=args.mode, prepared=prep,
                            src_order=order1 if prep else None, tar_order=order2 if prep else None, want_payload=True)

    ls = loss_step(prepared)

    def direct_step():
        ls(Rd, Td, w["lines"])
        return ls.payload

    from rrl_hip import rccl as rrccl
    if args.reducer == "torch":
        os.environ["RRL_DIRECT_RCCL"] = "0"
    reducer = rrccl.make_reducer(dev)   # collective: the same class on every rank
    direct = hasattr(reducer, "allreduce_inline")
    evidence = reducer.evidence() if direct else None
    print(f"[bench] rank {rank}/{world} local {local}: reducer {type(reducer).__name__} rccl {evidence}", file=sys.stderr)

    from rrl_hip.graph import GraphedStep

    def build(inline, issue):
        """(graph or None, callable step, finish) for one all-reduce placement and one way of issuing; capture success is
        agreed on by all ranks, so nobody replays a graph with a collective the others do not have."""
        last = [None]
        if issue == "direct":
            if inline:
                def step():
                    last[0] = reducer.allreduce_inline(direct_step())
                return None, step, (lambda: last[0])

            def step():
                reducer.submit(direct_step())
            return None, step, reducer.finish
        g, err = None, None
        try:
            g = GraphedStep((lambda: reducer.allreduce_inline(direct_step())) if inline else direct_step)
        except Exception as exc:
            err = exc
        if not rrccl.agree(g is not None, dev):
            if rank == 0:
                print(f"[bench] graph capture failed on some rank ({err}); direct issue only", file=sys.stderr)
            return None
        if inline:
            def step():
                last[0] = g()
            return g, step, (lambda: last[0])

        def step():
            reducer.submit(g())
        return g, step, reducer.finish

    def fence():
        torch.cuda.synchronize()
        if dist.is_initialized():
            dist.barrier()
        torch.cuda.synchronize()

    def timed(step, n):
        fence()
        t0 = time.perf_counter()
        for _ in range(n):
            step()
        return t0

    # ---- choose how the step is issued and where the all-reduce sits (identically on every rank)
    choice_note = None
    cands = []
    issues = ["direct", "graph"] if args.issue == "auto" and not args.no_graph else \
        [args.issue if args.issue != "auto" else "direct"]
    for issue in issues:
        have = False
        if direct and args.reducer in ("auto", "inline"):
            c = build(True, issue)
            if c is not None:
                cands.append(("inline/" + issue, c))
                have = True
        if args.reducer in ("overlap", "torch") or (args.reducer == "auto" and world > 1) or not have:
            c = build(False, issue)
            if c is not None:
                cands.append(("overlap/" + issue, c))
    if not cands:
        raise SystemExit("no way to issue the step (graph capture failed and --issue graph was forced)")
    if len(cands) > 1:  # measure all during warm-up; max over ranks -> the same decision everywhere
        probe = {}
        for trial in range(3):  # the smallest of three short trials per candidate: one host hiccup during a 1 ms probe
            for name, (g, step, finish) in cands:  # must not decide how the timed region is issued
                for _ in range(5):
                    step()
                t0 = timed(step, 40)
                finish()
                fence()
                tt = torch.tensor([time.perf_counter() - t0], device=dev, dtype=torch.float64)
                if dist.is_initialized():
                    dist.all_reduce(tt, op=dist.ReduceOp.MAX)
                probe[name] = min(probe.get(name, float("inf")), float(tt.item()) / 40 * 1e3)
        best = min(probe, key=probe.get)
        choice_note = {k: round(v, 4) for k, v in probe.items()}
        cands = [(n, c) for n, c in cands if n == best]
    (placement, issued), (graphed, step, finish) = cands[0][0].split("/"), cands[0][1]

    for _ in range(args.warmup):
        step()
    finish()
    t0 = timed(step, args.steps)  # barrier + synchronize, then the clock
    payload = finish()  # the last reduction is inside the timed region
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0  # this rank's K steps, from the common start to its own completion
    fence()  # closing barrier + synchronize; the MAX over the ranks' elapsed times below is the job's time (the
    #          barrier's own ~60-90 us of host/NCCL latency is not part of any step and stays outside the clock)
    tmax = torch.tensor([dt], device=dev, dtype=torch.float64)
    if dist.is_initialized():
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    dt = float(tmax.item())
    payload = payload.clone()
    if args.dump_outputs:  # the last timed step's results, as its caller receives them (ops.LossStep's outputs + the reduced payload)
        os.makedirs(args.dump_outputs, exist_ok=True)
        sfx = f".rank{rank}" if world > 1 else ""
        for name, t in (("loss", ls.st.loss), ("points1_grad", ls.grad), ("info", ls.st.info), ("payload", payload)):
            a = t.detach().cpu().numpy()
            if name == "points1_grad" and a.nbytes > DUMP_GRAD_BYTES // world:  # a fixed, seeded sample of the B * N rows
                a = a.reshape(-1, 9)
                rows = np.sort(np.random.default_rng(0).choice(len(a), DUMP_GRAD_BYTES // world // (9 * 4), replace=False))
                np.save(os.path.join(args.dump_outputs, f"points1_grad_rows{sfx}.npy"), rows.astype(np.float64))
                a = a[rows]
            np.save(os.path.join(args.dump_outputs, f"{name}{sfx}.npy"),
                    a.astype(np.float32 if a.dtype == np.float32 else np.float64))

    # ---- everything below is outside the timed region (rank 0 only, no collectives: the other ranks wait at the end)
    def time_loop(fn, n, warm=10):
        """ms per call of fn over n calls -- as the SMALLEST of three blocks of n / 3: these are the line's auxiliary figures
        (variants, extras), measured once each, and one host or box hiccup (a 90 ms stall was seen once in 300 cold steps) must
        not become the published value.  (The headline's timed region above is exactly K steps, unfiltered, as the contract says.)"""
        for _ in range(warm):
            out = fn()
        nb = max(n // 3, 1)
        best = float("inf")
        for _ in range(3):
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(nb):
                out = fn()
            torch.cuda.synchronize()
            best = min(best, (time.perf_counter() - t1) / nb * 1e3)
        return best, out

    extras, variants, roofline = {}, {}, None
    pairs_step = B * L * 3 * (N + M)
    dense_flops = FLOPS_PER_PAIR * pairs_step
    do_extras = rank == 0 and args.full and not args.no_extras
    other = None
    # ---- host time per step: what the CPU spends inside the calls that issue one step (the C call of
    # ops.LossStep + the reducer), measured while the GPU works through them asynchronously -- the step is GPU-bound as long as
    # this stays below ms_per_step; every rank measures (no collective inside), rank 0 reports
    host_us = None
    if graphed is None and args.full:
        torch.cuda.synchronize()
        acc_h, nh = 0.0, 100
        for _ in range(nh):
            th = time.perf_counter()
            step()
            acc_h += time.perf_counter() - th
        finish()
        torch.cuda.synchronize()
        host_us = acc_h / nh * 1e6
    parity = None
    if rank == 0:
        loss_default = ls.st.loss.clone()
        grad_default = ls.grad.clone()
        info_default = ls.st.info.clone()
        chained_step = bool(getattr(ls, "fused", False))  # the library's own word: the timed calls' records + scans were ONE launch
    if rank == 0 and args.full:
        if not args.no_parity:
            try:
                parity = parity_in_run(w, Rd, Td, ls.st.tri1t.clone(), loss_default, grad_default, info_default, sorted({0, B - 1}))
            except Exception as exc:
                parity = {"ok": False, "error": f"{type(exc).__name__}: {exc}"}
        # the OTHER build of the same step, always measured (round-over-round comparisons use the cold number): this rank's
        # step without the all-reduce
        if can_prepare and not args.no_other:
            lo_ = loss_step(not prepared)
            oms, oout = time_loop(lambda: lo_(Rd, Td, w["lines"]), args.steps)
            other = {"ms_per_step": oms, "value": pairs_step / (oms * 1e-3), "unit": "point-pairs/s (this rank, no all-reduce)",
                     "loss_bit_identical_to_timed_step": bool(torch.equal(oout[0], loss_default)),
                     "what": ("the section-8(d) step with NO prepared order: records + cell sort + sphere tree of both clouds in "
                              "every step (ops.LossStep(prepared=False), one C call, 5 launches) -- what a loop pays whose clouds "
                              "are new in every step; rounds 1-3 timed this build") if prepared else
                             "the section-8(d) step with prepared orders (ops.LossStep, 4 launches)"}
            variants["loss_step_cold" if prepared else "loss_step_prepared"] = other
            del lo_
        # ---- loops whose inputs CHANGE the way the callers' do: the timed region replays one (R, t, lines,
        # clouds); these rotate pre-made inputs per step (made outside the loops, resident in HBM like the timed step's)
        if not args.no_fresh and args.mode == "cull":
            from LieAlgebra import se3 as _se3f
            K = 8
            gen_f = torch.Generator().manual_seed(1234 + rank)
            lines_k, R_k, T_k = [], [], []
            for k in range(K):
                wk = w if k == 0 else None
                if wk is None:
                    torch.manual_seed(5000 + 17 * k + rank)  # (the CPU seed selects the sampler's uniform streams)
                    lk = Lmod.Random_uniform_distribution_lines_batch_efficient_resample(
                        w["radius"], w["center"], L, w["src"], w["tar"], dev)
                else:
                    lk = w["lines"]
                Rk_, Tk_ = _se3f.exp3(0.05 * torch.randn(B, 6, generator=gen_f))
                lines_k.append(lk); R_k.append(Rk_.to(dev).contiguous()); T_k.append(Tk_.to(dev).contiguous())
            torch.cuda.synchronize()
            if prepared:
                lf = loss_step(True)
                it = [0]

                def fresh_lines_step():
                    k = it[0] % K
                    it[0] += 1
                    return lf(R_k[k], T_k[k], lines_k[k])
                fms, _ = time_loop(fresh_lines_step, max(args.steps, 4 * K), warm=2 * K)
                variants["fresh_lines"] = {
                    "ms_per_step": fms, "value": pairs_step / (fms * 1e-3), "unit": "point-pairs/s (this rank, no all-reduce)",
                    "sets": K, "chained": bool(lf.fused),
                    "what": f"the timed step (prepared orders, kept target) with NEW lines and a NEW pose in every step: {K} pre-sampled "
                            "line sets and poses rotated per step -- the demo's loop (code/test_demo_optimized_Lie_Algebra.py:48-57: "
                            "lines re-sampled and the pose updated every epoch, the target never moves)"}
                del lf
            # ... and new CLOUDS in every step, through the cold build (a trainer's new batch: rpm/Train_RPM.py:45-81)
            Kc = 4
            clouds_k = [(w["tri1"], w["tri2"])]
            for k in range(1, Kc):
                wk = make_workload(B, N, M, 1, 100 + 10 * k + rank, dev)  # (one line: only the clouds are taken)
                clouds_k.append((wk["tri1"], wk["tri2"]))
            lcold = loss_step(False)
            itc = [0]

            def fresh_clouds_step():
                k = itc[0] % Kc
                itc[0] += 1
                lcold.src, lcold.tar = clouds_k[k]
                return lcold(R_k[k], T_k[k], lines_k[k])
            cms, _ = time_loop(fresh_clouds_step, max(args.steps, 4 * Kc), warm=2 * Kc)
            variants["fresh_clouds_cold"] = {
                "ms_per_step": cms, "value": pairs_step / (cms * 1e-3), "unit": "point-pairs/s (this rank, no all-reduce)", "sets": Kc,
                "what": f"the COLD step (records + cell sort + tree of both clouds every step) on {Kc} different cloud pairs rotated "
                        "per step, with new lines and poses too -- a trainer whose every batch brings new clouds that are evaluated "
                        "once (rpm/Train_RPM.py:45-81, RPM-Net's own re-cropping); (the lines of pairs 1.. were sampled for pair 0's "
                        "geometry: same shapes and hit statistics, synthetic either way)"}
            del lcold, clouds_k
        roofline = scan_roofline(ops, lambda: ls(Rd, Td, w["lines"]), B, N, M, L, launches=min(args.steps, 20),
                                 counters=do_extras and args.mode == "cull")
        if chained_step and "executed_flops" in roofline:
            # the scan ALONE, as a launch of its own (the plain step: chain off), for the same executed arithmetic: the chained
            # launch's fraction is taken over records + scan, this one over the scan kernel -- round 5's figure, like for like
            lpl = loss_step(prepared)
            lpl.chain = False
            rpl = scan_roofline(ops, lambda: lpl(Rd, Td, w["lines"]), B, N, M, L, launches=min(args.steps, 20), counters=False)
            roofline["plain_scan"] = {
                "kernel": "cull_scan_kernel<false> of the PLAIN step (ops.LossStep(chain=False): records launch + this scan launch)",
                "launch_ms": rpl["launch_ms"], "launches_timed": rpl["launches_timed"],
                "frac": roofline["executed_flops"] / (rpl["launch_ms"] * 1e-3) / 1e12 / VALU_PEAK_TFLOPS,
                "loss_bit_identical_to_timed_step": bool(torch.equal(lpl.st.loss, loss_default))}
            del lpl
    if do_extras:
        # ---- the fused TRAINING op (rounds 3-4's headline): backward straight to (dR, dT), 14-float payload with the sums
        rs = ops.RegistrationStep(w["tri1"], w["tri2"], L, transpose_r=True, mode=args.mode, want_payload=True,
                                  prepared=prepared, src_order=order1 if prepared else None,
                                  tar_order=order2 if prepared else None, chain=True)
        fms, fout = time_loop(lambda: rs(Rd, Td, w["lines"]), args.steps)
        fused_gR = fout[1].clone()
        variants["fused_dRdT"] = {
            "ms_per_step": fms, "value": pairs_step / (fms * 1e-3), "unit": "point-pairs/s (this rank, no all-reduce)",
            "what": "ops.RegistrationStep(chain=True) -> rrl_registration_step: rigid apply + loss + backward straight to (dR, dT) "
                    "(no points1.grad), one C call per step, chained like the timed step -- what a trainer whose pose comes out "
                    "of a network needs",
            "chained": bool(rs.fused),
            "loss_bit_identical_to_timed_step": bool(torch.equal(fout[0], loss_default))}
        del rs

        # ---- bit-reproducible points1.grad on request: the scatter in 64-bit fixed point + a conversion launch
        ldet = ops.LossStep(w["tri1"], w["tri2"], L, transpose_r=True, mode=args.mode, prepared=prepared,
                            src_order=order1 if prepared else None, tar_order=order2 if prepared else None, deterministic=True)
        dms_, dout = time_loop(lambda: ldet(Rd, Td, w["lines"]), args.steps)
        gdet = dout[1].clone()
        ldet(Rd, Td, w["lines"])
        variants["deterministic_grad"] = {
            "ms_per_step": dms_, "value": pairs_step / (dms_ * 1e-3), "unit": "point-pairs/s (this rank, no all-reduce)",
            "what": "ops.LossStep(deterministic=True): the same step with points1.grad accumulated in 64-bit fixed point (workspace "
                    "field GFIX; integer atomics commute) and converted by one more launch -- forward + scatter + conversion, no "
                    "chain, no riding backward; the reference's CPU autograd is deterministic",
            "loss_bit_identical_to_timed_step": bool(torch.equal(dout[0], loss_default)),
            "grad_bit_identical_between_calls": bool(torch.equal(ldet.grad, gdet)),
            "grad_max_rel_diff_vs_timed_step": float((gdet - grad_default).abs().max() / grad_default.abs().max())}
        del ldet

        # ---- the kernel that performs ALL counted flops: the strict scan of the same step
        lstrict = ops.LossStep(w["tri1"], w["tri2"], L, transpose_r=True, mode="strict")
        sroof = scan_roofline(ops, lambda: lstrict(Rd, Td, w["lines"]), B, N, M, L, launches=20, counters=False)
        same = bool(torch.equal(lstrict.st.loss, loss_default))
        s_ = sroof["launch_ms"] * 1e-3
        roofline["dense_reference"] = {
            "kernel": "scan_kernel<v2f,2> (scan mode strict: every (line, point) pair evaluated -- the kernel that performs "
                      "all 18 counted flops per pair; NOT part of the timed step; HIP events on the launch stream, this run)",
            "achieved": dense_flops / s_ / 1e12, "frac": dense_flops / s_ / 1e12 / VALU_PEAK_TFLOPS,
            "launch_ms": sroof["launch_ms"], "launches_timed": sroof["launches_timed"],
            "algorithmic_flops_per_launch": dense_flops, "loss_bit_identical_to_default_mode": same}
        del lstrict

        # ---- SURVEY 8(d) through the drop-in callables: T-apply -> loss -> backward to points1.grad (and on through the
        # rigid apply to dR, dT), chained by autograd
        keep = {}

        def dropin_step():
            w["R"].grad = w["T"].grad = None
            tri1 = ops.rigid_apply(w["tri1"].reshape(B, 3 * N, 3), w["R"], w["T"], transpose_r=True).reshape(B, N, 9)
            tri1.retain_grad()
            loss, info, _ = ops.intersection_loss(tri1, w["tri2"], w["lines"], (1, 1, 5, 5), mode=args.mode,
                                                  order1=order1 if prepared else None, order2=order2 if prepared else None)
            torch.autograd.backward([loss], [ones])
            keep["g"], keep["loss"] = tri1.grad, loss
            return tri1.grad
        try:
            gd = GraphedStep(dropin_step) if not args.no_graph else dropin_step
        except Exception as exc:
            print(f"[bench] drop-in capture failed ({type(exc).__name__}: {exc}); eager", file=sys.stderr)
            gd = dropin_step
        dms, _ = time_loop(gd, args.steps)
        g1 = keep["g"]
        variants["points1_grad_autograd"] = {
            "ms_per_step": dms, "value": pairs_step / (dms * 1e-3), "unit": "point-pairs/s (this rank)",
            "what": "ops.rigid_apply -> ops.intersection_loss (what loss.cal_loss_intersection_batch_whole_median_"
                    "pts_lines calls) -> backward to points1.grad (B,N,9), then rigid-apply backward to dR, dT; "
                    + ("hipGraph replay" if gd is not dropin_step else "eager launches"),
            "points1_grad_nonzero_rows": int((g1.abs().sum(-1) > 0).sum()),
            "loss_sum": float(keep["loss"].detach().sum()),
            "loss_bit_identical_to_timed_step": bool(torch.equal(keep["loss"].detach(), loss_default)),
            "points1_grad_max_rel_diff_vs_timed_step": float((grad_default - g1).abs().max() / g1.abs().max()),
            "dR_max_rel_diff_vs_fused": float((w["R"].grad - fused_gR).abs().max() / fused_gR.abs().max())}
        extras["points1_grad_nonzero_rows"] = int((grad_default.abs().sum(-1) > 0).sum())

        # ---- the reference trainers' literal call pattern (rpm/Train_RPM.py:204-231, dcp/Train_DCP.py:266-270,
        # fmr/model.py:302-306): transform once, then one reference-signature call per sample, summed in Python,
        # one backward.  Eager by nature: every call reads its flags back (None / NaN are host-side decisions).
        def loop_step():
            w["R"].grad = w["T"].grad = None
            tri1 = ops.rigid_apply(w["tri1"].reshape(B, 3 * N, 3), w["R"], w["T"], transpose_r=True).reshape(B, N, 9)
            total = 0
            for j in range(B):
                one = Lmod.cal_loss_intersection_batch_whole_median_pts_lines(
                    1, 1, 5, 5, tri1[j:j + 1], w["tri2"][j:j + 1], w["lines"][j:j + 1], dev)
                if one is not None:
                    total = total + one
            total.backward()
            return total
        lms, tot = time_loop(loop_step, max(10, min(args.steps, 50)), warm=5)
        variants["dropin_loop"] = {
            "ms_per_step": lms, "ms_per_call": lms / B, "value": pairs_step / (lms * 1e-3),
            "unit": "point-pairs/s (this rank)",
            "what": f"for j in range({B}): loss += loss.cal_loss_intersection_batch_whole_median_pts_lines(1, 1, 5, 5, "
                    "p1[j:j+1], p2[j:j+1], line[j:j+1]) on the moved triangles, then loss.backward() to (dR, dT) -- the "
                    "reference trainers' literal pattern, eager, one host read-back per call",
            "loss_sum": float(tot.detach().sum()),
            "dR_max_rel_diff_vs_fused": float((w["R"].grad - fused_gR).abs().max() / fused_gR.abs().max())}

        # ---- Chamfer monitor (every caller evaluates it next to the loss): device time per call
        def time_call(fn, n=50):
            """ms per call of fn, issued eagerly and as a hipGraph replay: (best, how, last result, both)"""
            out = {}
            for how in (["eager"] if args.no_graph else ["eager", "graph"]):
                gc = GraphedStep(fn) if how == "graph" else fn
                ms, res = time_loop(gc, n, warm=5)
                out[how] = (ms, res)
            how = min(out, key=lambda k: out[k][0])
            return out[how][0], how, out[how][1], {k: round(v[0], 5) for k, v in out.items()}

        def chamfer_ms(tree):
            ops.CHAMFER_TREE = tree
            try:
                ms, how, cd, both = time_call(lambda: Lmod.chamfer_dist(w["src"], w["tar"]))
                return ms, float(cd), how, both
            finally:
                ops.CHAMFER_TREE = True
        cms, cd, chow, cboth = chamfer_ms(True)
        bms, cdb, _, _ = chamfer_ms(False)
        if prepared:  # with PREPARED point clouds (the orders of the loss's clouds serve their first points): no sort in the call
            pms, phow, pcd, pboth = time_call(lambda: ops.chamfer(w["src"], w["tar"], order_x=order1, order_y=order2))
            extras.update({"chamfer_prepared_ms": pms, "chamfer_prepared_issue": phow, "chamfer_prepared_ms_by_issue": pboth,
                           "chamfer_prepared_equals_chamfer": float(pcd) == cd})
        extras.update({"chamfer_ms": cms, "chamfer_issue": chow, "chamfer_ms_by_issue": cboth,
                       "chamfer_pairs_per_s": B * N * M / (cms * 1e-3), "chamfer": cd,
                       "chamfer_brute_force_ms": bms, "chamfer_values_equal": cd == cdb,
                       "chamfer_note": "both directions, B x N x M dense-equivalent pairs; sorted clouds + sphere tree "
                                       "(rrl_chamfer.hip) vs the all-pairs kernel"})
        # the monitor INSIDE the step: the walk needs the step's records launch only, and launches of one stream never
        # overlap on this stack, so ops.ChamferRide issues its workgroups in the culled scan's grid
        if prepared and args.mode == "cull":
            ride_ms = {}
            for name, kw in (("step_then_chamfer_from_state", {}), ("step_with_the_walk_riding", {"chamfer": True})):
                rs = ops.LossStep(w["tri1"], w["tri2"], L, transpose_r=True, mode=args.mode, src_order=order1,
                                  tar_order=order2, **kw)

                def monitored():
                    rs(Rd, Td, w["lines"])
                    return rs.chamfer_value if kw else ops.chamfer_from_state(rs.st)
                ride_ms[name], cv = time_loop(monitored, args.steps)
                ride_ms[name + "_value"] = float(cv)
            extras["step_with_chamfer_monitor_ms"] = ride_ms

        # ---- the iterative trainers (RPM num_iter = 2, rpm/Train_RPM.py:207-231): both poses as ONE multi-pose evaluation
        # (rrl_opts.problems) against pose after pose with the target's scan carried over, and one pose alone -- the fused
        # training op forward + backward through its autograd front end, as hipGraph replays (device time)
        if prepared and args.mode == "cull" and not args.no_graph:
            try:
                g2 = torch.Generator().manual_seed(11 + rank)
                from LieAlgebra import se3 as _se3
                R2, T2 = _se3.exp3(0.05 * torch.randn(B, 6, generator=g2))
                Rk = torch.cat([w["R"].detach(), R2.to(dev)]).requires_grad_(True)
                Tk = torch.cat([w["T"].detach(), T2.to(dev)]).requires_grad_(True)
                ones2 = torch.ones(2 * B, device=dev)
                kept = {}

                def multi():
                    Rk.grad = Tk.grad = None
                    l, _, _ = ops.registration_loss(w["tri1"], Rk, Tk, w["tri2"], w["lines"], order1=order1, order2=order2)
                    torch.autograd.backward([l], [ones2])
                    kept["m"] = l
                    return l

                def loop():
                    Rk.grad = Tk.grad = None
                    la, _, _ = ops.registration_loss(w["tri1"], Rk[:B], Tk[:B], w["tri2"], w["lines"], order1=order1, order2=order2)
                    first = ops.last_state()
                    lb, _, _ = ops.registration_loss(w["tri1"], Rk[B:], Tk[B:], w["tri2"], w["lines"], order1=order1, order2=order2,
                                                     target_from=first)
                    torch.autograd.backward([la, lb], [ones, ones])
                    kept["l"] = (la, lb)
                    return la

                def single():
                    Rk.grad = Tk.grad = None
                    la, _, _ = ops.registration_loss(w["tri1"], Rk[:B], Tk[:B], w["tri2"], w["lines"], order1=order1, order2=order2)
                    torch.autograd.backward([la], [ones])
                    return la
                mp = {}
                for name, fn in (("two_poses_one_evaluation", multi), ("two_poses_one_after_the_other", loop), ("one_pose", single)):
                    mp[name + "_ms"], _ = time_loop(GraphedStep(fn), max(50, args.steps // 2))
                mp["loss_bits_equal"] = bool(torch.equal(kept["m"].detach(), torch.cat([x.detach() for x in kept["l"]])))
                mp["ratio_to_one_pose"] = mp["two_poses_one_evaluation_ms"] / mp["one_pose_ms"]
                mp["what"] = ("ops.registration_loss forward + backward to (dR, dT) at the timed shape, hipGraph replays: k = 2 poses of every "
                              "problem evaluated as 2 B instances in one set of launches (target scanned once per problem) / as two "
                              "evaluations, the second with the target's scan carried over (round 4) / one pose")
                extras["multi_pose"] = mp
            except Exception as exc:
                extras["multi_pose"] = {"error": f"{type(exc).__name__}: {exc}"}

        # ---- a CHIP-FILLING shape: BASELINE configs[2] (B = 64) as one batch on this GPU -- separates the kernel's quality
        # from "B = 8 fills under half of the 256 CUs"
        if not args.no_b64 and args.mode == "cull" and B < 64:
            B64 = 64
            w64 = make_workload(B64, N, M, L, 7 + rank, dev)
            o1, o2 = ops.cloud_order(w64["tri1"]), ops.cloud_order(w64["tri2"])
            l64 = ops.LossStep(w64["tri1"], w64["tri2"], L, transpose_r=True, mode=args.mode, src_order=o1, tar_order=o2)
            R64, T64 = w64["R"].detach(), w64["T"].detach()
            ms64, out64 = time_loop(lambda: l64(R64, T64, w64["lines"]), max(20, args.steps // 4))
            r64 = scan_roofline(ops, lambda: l64(R64, T64, w64["lines"]), B64, N, M, L, launches=20)
            r64 = attach_pmc(r64, B64, N, L, args.mode)
            r64.update({"workload": f"B={B64} on ONE GPU, N=M={N}, L={L} (BASELINE configs[2] as one batch), the same section-8(d) "
                                    "step, prepared orders, direct issue, no all-reduce",
                        "ms_per_step": ms64, "value": B64 * L * 3 * (N + M) / (ms64 * 1e-3), "unit_value": "point-pairs/s",
                        "ms_per_8_samples": ms64 / (B64 / 8), "valid_samples": int((out64[2][:, 0] > 0).sum()),
                        "scan_share_of_step": r64["launch_ms"] / ms64})
            roofline["at_B64"] = r64
            del l64, w64

    if rank == 0:
        value = sum_pairs(world, B, args, L, N, M) * args.steps / dt
        ms_step = dt / args.steps * 1e3
        if args.full:  # the roofline of the timed step's dominant launch, measured above
            alg_bytes = B * (N + M) * 48 + B * L * 24 + 2 * B * L * 4  # ptri + lines + counts
            if chained_step:  # + the records body of the same launch: raw row in; record, (P0, thr2), index, NaN reach, moved row, tree out; clearing
                alg_bytes += int(B * N * (36 + 48 + 16 + 4 + 4 + 36 + 13 * 16 / 64 + 36))
            cull_ms = roofline["launch_ms"]
            cull_s = cull_ms * 1e-3
            if "frac" not in roofline:
                if args.mode != "cull":  # a dense mode was asked for: the timed kernel does evaluate every pair
                    roofline.update({"achieved": dense_flops / cull_s / 1e12, "frac": dense_flops / cull_s / 1e12 / VALU_PEAK_TFLOPS})
                else:
                    roofline.update({"achieved": None, "frac": None})
            attach_pmc(roofline, B, N, L, args.mode)
            roofline.update({
                "bound": "valu",
                "note": "fp32 VALU / latency-bound, not HBM- or MFMA-bound (no FMA allowed where labels are decided; O(L (N+M)) "
                        "elementwise geometry).  peak = 157.3 / 2 TFLOP/s (one flop per lane-op: 256 CU x 4 SIMD-32 x 2.4 GHz).  "
                        "achieved / frac = arithmetic the kernel EXECUTED (in-kernel counters, this run: sphere tests x 12 + "
                        "point-0 prefilter x 11 + resolved candidates x 48 lane-ops; queue / ballot / bookkeeping instructions not "
                        "counted) / its launch time by HIP events on the launch stream (this run); frac_rocprof = the same / "
                        "rocprof's average kernel duration of the committed profile of exactly this build; issue_frac = "
                        "SQ_INSTS_VALU x 64 of the committed PMC pass / launch time; the dense work this kernel decides "
                        "(18 flops per pair) is work_ratio x executed.",
                "peak": VALU_PEAK_TFLOPS, "unit": "TFLOP/s",
                "kernel": (("cull_scan_build_kernel (the CHAINED step's launch: the source's records body in its leading workgroups + the "
                            "culled scan of both clouds; launch time = the whole launch, executed flops = the scan's, counted by the "
                            "instrumented plain scan of the same step)") if chained_step else
                           "cull_scan_kernel<false> (scan mode cull: the dominant kernel of the timed step)") if args.mode == "cull"
                          else f"scan_kernel (scan mode {args.mode})",
                "ops_per_test": {"sphere": OPS_SPHERE, "point0_prefilter": OPS_EXACT, "candidate": OPS_CAND,
                                 "fallback_pair": OPS_FALLBACK},
                "csrc_sha": csrc_sha(),
                "hbm": {"algorithmic_bytes": alg_bytes, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "achieved": alg_bytes / cull_s / 1e9, "frac": alg_bytes / cull_s / 1e9 / HBM_PEAK_GBS,
                        "kernel": "scan launch of the timed step"}})
        extras.update({"loss_sum": float(payload[0]), "valid": float(payload[1]),
                       "line_sampling_s": w["sample_s"]})
        if args.full:
            extras.update({"scan_launch_ms": cull_ms,
                           "scan_share_of_step": cull_ms / ms_step,
                           "host_us_per_step": host_us,
                           "host_margin": (1.0 - host_us / (ms_step * 1e3)) if host_us else None,
                           "host_note": "CPU time inside the calls that issue one step (ops.LossStep's C call: 3 launches chained, + "
                                        "the reducer), 100 steps issued asynchronously behind the timed region; host_margin = 1 - "
                                        "host / ms_per_step: the step is GPU-bound while it is positive (a slower host moves the "
                                        "crossover; a hipGraph replay costs ~8 us + 1.5 us per node on this stack and is measured "
                                        "in warm-up: config.allreduce.warmup_ms_per_step)"})
        out = {
            "metric": "point-pairs/sec for loss fwd+bwd at B=8, N=M=4096",
            "value": value, "unit": "point-pairs/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": ms_step,
            "higher_is_better": True, "scaling": "strong" if strong else "weak", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "config": {"workload": (f"B={B}/GPU" if not strong else f"global B={args.global_batch} sharded over {world}")
                                   + f", N=M={N} pseudo-triangles, L={L} lines, fp32 loss fwd+bwd "
                                   f"(BASELINE.json configs[{2 if strong else 1}]); SURVEY 8(d) step: rigid apply of the source + "
                                   f"S + P + median + Welsch + backward to points1.grad (B,N,9) (code/loss.py:170-232 + autograd), "
                                   f"one C call per step (ops.LossStep -> rrl_loss_step_ex), then the all-reduce of "
                                   f"[loss sum, valid count]; scan mode {args.mode}; "
                                   + ("PREPARED: k-d order of each cloud computed once outside the timed region "
                                      "(rrl_cloud_order: prepare_us), target records kept while it does not move"
                                      + ("; CHAINED (round 6): source records + target scan + source scan as ONE launch, 3 launches per step; "
                                         if chained_step else "; 4 launches; ")
                                      + "applies to loops that evaluate many poses / line sets per cloud pair (the demo: 1000 epochs per "
                                        "pair -- variants.fresh_lines --, RPM / FMR inner iterations, datasets that cache the orders: "
                                        "pre_dataloader.kd_order); a trainer whose clouds are new in every step and evaluated once gets "
                                        "value_cold / variants.fresh_clouds_cold (config.break_even_steps); "
                                      if prepared else "COLD: records + cell sort + sphere tree of both clouds every step; 5 launches; ")
                                   + ("hipGraph replay" if graphed is not None else "direct issue on the stream")
                                   + "; value counts dense-equivalent pairs",
                       "step": "loss_step (SURVEY 8(d): points1.grad)",
                       "issue": issued, "prepared_order": prepared, "chained": chained_step, "prepare_us": prepare_us,
                       "break_even_steps": (2.0 * prepare_us / max((other["ms_per_step"] - ms_step) * 1e3, 1e-9)
                                            if (prepared and other is not None and prepare_us and other["ms_per_step"] > ms_step) else None),
                       "break_even_note": "steps per cloud pair from which computing both orders in-stream (2 x prepare_us) pays for "
                                          "itself: 2 prepare_us / (ms_per_step_cold - ms_per_step)",
                       "prepare_note": "rrl_cloud_order of B clouds of N triangles, once per cloud (dataset item / demo start); a "
                                       "rigid motion keeps the order, so it serves every pose of the cloud",
                       "global_batch": args.global_batch if strong else B * world,
                       "parallelism": f"batch-shard dp{world}",
                       "allreduce": {"reducer": type(reducer).__name__, "placement": placement,
                                     "in_graph": placement == "inline" and graphed is not None,
                                     "rccl": evidence, "process_group": dist.is_initialized(),
                                     "backend": dist.get_backend() if dist.is_initialized() else None,
                                     "warmup_ms_per_step": choice_note}},
            "value_is": "SURVEY section 8(d) as defined: rigid apply + loss forward + backward to points1.grad (B, N, 9), "
                        "dense-equivalent pairs, " + ("prepared orders" if prepared else "cold build")
                        + ("; the other build of the same step is value_" + ("cold" if prepared else "prepared")
                           + " (this rank, no all-reduce); round-over-round comparisons with rounds 1-3 must use the cold number; "
                             "variants.fused_dRdT = the fused training op (rounds 3-4's headline)" if args.full else ""),
            **({"roofline": roofline, "parity_in_run": parity, "variants": variants} if args.full else {}),
            "extras": extras,
        }
        if other is not None:
            out["value_" + ("cold" if prepared else "prepared")] = other["value"]
            out["ms_per_step_" + ("cold" if prepared else "prepared")] = other["ms_per_step"]
        if world == 1 and args.full and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(N, M, L)
        sys.stdout.flush()
        os.write(real_stdout, (json.dumps(out) + "\n").encode())
    if hasattr(reducer, "close"):
        reducer.close()
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


def sum_pairs(world, B, args, L, N, M):
    """Dense-equivalent pairs of one step over ALL ranks."""
    total_b = args.global_batch if args.global_batch > 0 else B * world
    return total_b * L * 3 * (N + M)


if __name__ == "__main__":
    main()
