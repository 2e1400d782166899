"""Timing of the ball-query grouping and raw features (rrl_hip/neighbors.py ball_group) against the
reference's formulation in eager torch on the same GPU, in the same process.

  sizes         B = 8 surface clouds (synth.surface_cloud, unit normals) at N = 1024 and N = 1433 (the RPM trainer's 2048 points
                at 0.7 crop), radius 0.3, nsample 64, the three channels xyz, dxyz, ppf
  baseline      rpm/models/pointnet_util.py:96-131, 173-244 and feature_nets.py:184-193 restated below in torch: the (B, N, N)
                int64 index tensor, the matmul distance matrix, two masks, the row sort, four gathers, three atan2 passes,
                expand and cat
  per call      us per call through Python (callsites.rpm_raw_features): device events around a window of --steps calls, the
                two paths' windows interleaved, median of --rounds windows with min ... max
  device        the C entry called directly on buffers allocated once (rrl_ball_group): the stream stays full and the window
                measures the device.  Also with no channel (indices and found only): the distance loop without the feature phase
  kernel        with --trace DIR: the kernel's own time from a kernel trace (rocprofv3 --kernel-trace, a run of its own, of
                `--kernel-calls K`: K calls per size with the three channels, then K per size with none), median of each group

Writes --out (default profiles/ball_query_timing.json) and prints it.  With --parent DIR (a checkout of the parent commit with its
library built): `python bench.py` in this tree and in DIR, alternating (and alternating which of the two goes first),
--bench-rounds times each."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "a-robust-registration-loss_amd"))

B, RADIUS, NSAMPLE = 8, 0.3, 64
SIZES = (1024, 1433)
LAUNCHES = 1


def torch_angle(a, b):
    import torch
    cross = torch.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                         a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], dim=-1)
    return torch.atan2(torch.norm(cross, dim=-1), torch.sum(a * b, dim=-1))


def torch_gather(t, idx):
    import torch
    return t[torch.arange(t.shape[0], device=t.device).view(-1, 1, 1), idx]


def torch_raw_features(xyz, normals, radius=RADIUS, nsample=NSAMPLE):
    """The reference's formulation of the (B, N, nsample, 10) tensor, eager torch."""
    import torch
    Bn, N, _ = xyz.shape
    own = torch.arange(N, device=xyz.device)
    group = own.view(1, 1, N).repeat(Bn, N, 1)
    d2 = -2 * torch.matmul(xyz, xyz.transpose(1, 2))
    d2 += torch.sum(xyz ** 2, -1)[:, :, None]
    d2 += torch.sum(xyz ** 2, -1)[:, None, :]
    group[:, own, own] = N
    group[d2 > radius ** 2] = N
    group = group.sort(dim=-1)[0][:, :, :nsample]
    first = own.view(1, N, 1).repeat(Bn, 1, nsample)
    mask = group == N
    group[mask] = first[mask]
    d = torch_gather(xyz, group) - xyz.view(Bn, N, 1, 3)
    nj, ni = torch_gather(normals, group), normals[:, :, None, :]
    ppf = torch.stack([torch_angle(ni, d), torch_angle(nj, d), torch_angle(ni, nj), torch.norm(d, dim=-1)], dim=-1)
    return torch.cat([xyz[:, :, None, :].expand(-1, -1, nsample, -1), d, ppf], -1)


def summary(v):
    return {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)}


def interleaved(fns, steps, warmup, rounds):
    """us per call of each fn: their windows alternate, round after round."""
    import torch
    for fn in fns:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(steps):
                fn()
            t1.record()
            torch.cuda.synchronize()
            out[i].append(t0.elapsed_time(t1) * 1e3 / steps)
    return [summary(v) for v in out]


def inputs(n):
    import numpy as np
    import torch
    from rrl_hip import synth
    x = np.stack([synth.surface_cloud(1000 + n + b, n) for b in range(B)])
    nr = x / np.linalg.norm(x, axis=-1, keepdims=True)
    return torch.from_numpy(x).cuda(), torch.from_numpy(nr.astype(np.float32)).cuda()


def device_calls(x, nr, n):
    """(all channels, no channel): closures around the C entry on buffers allocated once (kept alive by the closures)."""
    import numpy as np
    import torch
    from rrl_hip import ops
    idx = torch.empty(B, n, NSAMPLE, dtype=torch.int32, device="cuda")
    found = torch.empty(B, n, dtype=torch.int32, device="cuda")
    feat = torch.empty(B, n, NSAMPLE, 10, dtype=torch.float32, device="cuda")
    r2 = float(np.float32(RADIUS ** 2))

    def full():
        ops._run(x.device, "rrl_ball_group", ops._p(x), ops._p(nr), None, None, None, r2, NSAMPLE, 1, 7, ops._p(idx), ops._p(found),
                 ops._p(feat), B, n, n)

    def index_only():
        ops._run(x.device, "rrl_ball_group", ops._p(x), None, None, None, None, r2, NSAMPLE, 1, 0, ops._p(idx), ops._p(found), None, B, n, n)
    return full, index_only


def rows(a):
    import torch
    from rrl_hip import callsites
    out = []
    for n in SIZES:
        x, nr = inputs(n)

        def new():
            return callsites.rpm_raw_features(x, nr, ("xyz", "dxyz", "ppf"), RADIUS, NSAMPLE)

        def ref():
            return torch_raw_features(x, nr)
        mine, theirs = new(), ref()
        found = (mine[..., 3:6] != 0).any(-1).sum(-1)  # (a member is another point: d != 0)
        same = ((mine[..., 3:6] - theirs[..., 3:6]).abs().amax((-1, -2)) == 0)
        row = {"B": B, "N": n, "radius": RADIUS, "nsample": NSAMPLE, "channels": 10, "launches": LAUNCHES,
               "output_megabytes": mine.numel() * 4 / 1e6, "members_mean": float(found.float().mean()),
               "rows_truncated": float((found == NSAMPLE).float().mean()),
               "agreement": {"rows_with_equal_dxyz": float(same.float().mean()),
                             "ppf_max_abs_on_those_rows": float((mine[..., 6:] - theirs[..., 6:]).abs()[same].max())}}
        for name, r in zip(("per_call", "torch_per_call"), interleaved([new, ref], a.steps, a.warmup, a.rounds)):
            row[name] = r
        full, index_only = device_calls(x, nr, n)
        for name, r in zip(("device", "device_indices_only"), interleaved([full, index_only], a.steps, a.warmup, a.rounds)):
            row[name] = r
        row["speedup_per_call"] = row["torch_per_call"]["median_us"] / row["per_call"]["median_us"]
        row["speedup_device"] = row["torch_per_call"]["median_us"] / row["device"]["median_us"]
        row["faster_in_both"] = row["speedup_per_call"] > 1.0 and row["speedup_device"] > 1.0
        row["feature_phase_share_of_device"] = 1.0 - row["device_indices_only"]["median_us"] / row["device"]["median_us"]
        out.append(row)
        del mine, theirs
        torch.cuda.empty_cache()
    return out


def kernel_calls(k):
    """The run a kernel trace is taken of: k calls per size with the three channels, then k per size with none."""
    import torch
    calls = [device_calls(*inputs(n), n) for n in SIZES]
    for which in (0, 1):
        for pair in calls:
            for _ in range(k):
                pair[which]()
    torch.cuda.synchronize()


def kernel_rows(trace_dir, k):
    """Median duration of each group of k dispatches of the kernel, in trace order."""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {trace_dir}")
    spans = []
    for f in files:
        for r in csv.DictReader(open(f)):
            if "ball_group_kernel" in r.get("Kernel_Name", ""):
                spans.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    spans.sort()
    if len(spans) != 2 * len(SIZES) * k:
        raise SystemExit(f"expected {2 * len(SIZES) * k} dispatches of the kernel, found {len(spans)}")
    out = []
    for g, (what, n) in enumerate((w, n) for w in ("three channels", "indices only") for n in SIZES):
        us = [(e - s) / 1e3 for s, e in spans[g * k:(g + 1) * k]]
        out.append({"N": n, "what": what, "calls": k, "launches_per_call": LAUNCHES, **summary(us)})
    return out


def bench_series(parent, rounds):
    def one(cwd):
        res = subprocess.run([sys.executable, "bench.py"], cwd=cwd, capture_output=True, text=True, check=True).stdout
        value = json.loads(res.strip().splitlines()[-1])["value"]
        print("bench.py in", cwd, value, file=sys.stderr, flush=True)
        return value
    mine, theirs = [], []
    for i in range(rounds):  # the pair's order alternates: whichever runs second in a pair follows a process that just left the GPU
        for cwd in ((ROOT, parent) if i % 2 == 0 else (parent, ROOT)):
            (mine if cwd == ROOT else theirs).append(one(cwd))
    return {"command": "python bench.py", "rounds": rounds, "order": "alternating pairs, this tree first in the even ones",
            "this_tree": mine, "parent_library": theirs,
            "this_tree_median": statistics.median(mine), "parent_min": min(theirs), "parent_max": max(theirs),
            "inside_parent_spread": min(theirs) <= statistics.median(mine) <= max(theirs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--kernel-calls", type=int, default=0, help="only issue this many calls per group (the run to trace), write nothing")
    ap.add_argument("--trace", help="directory of a kernel trace of a --kernel-calls run: adds the kernel's own time")
    ap.add_argument("--trace-calls", type=int, default=20, help="the --kernel-calls of the traced run")
    ap.add_argument("--parent", help="checkout of the parent commit with its library built")
    ap.add_argument("--bench-rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ball_query_timing.json"))
    a = ap.parse_args()
    import torch
    if a.kernel_calls:
        kernel_calls(a.kernel_calls)
        return
    doc = {"what": "ball-query grouping and raw features against the reference's formulation in eager torch on one MI355X: device "
                   "events around windows of %d calls, the paths' windows interleaved, median of %d windows" % (a.steps, a.rounds),
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "ball_group": rows(a)}
    torch.cuda.synchronize()
    if a.trace:
        doc["kernel"] = {"what": "ball_group_kernel's own time (rocprofv3 --kernel-trace, a run of its own)", "rows": kernel_rows(a.trace, a.trace_calls)}
    if a.parent:
        doc["bench"] = bench_series(os.path.abspath(a.parent), a.bench_rounds)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
