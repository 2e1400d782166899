"""The ragged Chamfer distance against what a caller with mixed sizes has WITHOUT it (DESIGN.md "Ragged batches").

B = 8 pairs, capacities 4096 / 4096, per-sample counts spread evenly between 1024 and 4096 (both clouds of sample b have
COUNTS[b] points), forward alone and forward + backward to x.grad and y.grad:

  ragged_fwd / ragged_fwdbwd        this tree, ops.chamfer(x, y, counts_x=, counts_y=): ONE call (+ one backward call)
  ragged_full_fwd                   this tree, counts equal to the capacities (what reading the counts costs)
  uniform_fwd / uniform_fwdbwd      this tree, ops.chamfer(x, y) at B = 8, N = M = 4096: the uniform path
  loop8_fwd / loop8_fwdbwd          the PARENT commit's library: eight B = 1 ops.chamfer calls on the truncated clouds --
                                    the only correct alternative there
  uniform_parent_fwd / _fwdbwd      the PARENT commit's library: the uniform call (must keep its speed)

The parent's numbers come from a CHILD process that imports the package of a checkout of the parent commit (--parent DIR:
`git worktree add DIR HEAD~1`, then build its library there) -- two builds of one library cannot live in one process.
Rounds alternate between the two processes in one session; every timed window ends in a device synchronisation.  Writes
--out (default profiles/ragged_chamfer_timing.json) and prints it.  Kernel averages: run --steps-only VARIANT under
`rocprofv3 --kernel-trace --stats` in a run of its own."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

B, CAP = 8, 4096
COUNTS = [CAP // 4 + (CAP - CAP // 4) * b // (B - 1) for b in range(B)]  # 1024 .. 4096


def workload(pkg_root):
    """(x, y) (B, CAP, 3) on the GPU, seeded: the same tensors in both processes."""
    sys.path.insert(0, os.path.join(pkg_root, "a-robust-registration-loss_amd"))
    import numpy as np
    import torch
    from rrl_hip import synth
    prs = [synth.make_pair(1000 + b, CAP, CAP) for b in range(B)]
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    return cu(np.stack([p["src"] for p in prs])), cu(np.stack([p["tar"] for p in prs]))


def timed(fn, steps):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / steps


def _fwd(ops, x, y, **kw):
    return lambda: ops.chamfer(x, y, **kw)


def _fwdbwd(ops, x, y, **kw):
    xg, yg = x.clone().requires_grad_(True), y.clone().requires_grad_(True)

    def step():
        xg.grad = yg.grad = None
        ops.chamfer(xg, yg, **kw).backward()
    return step


def parent_variants(root):
    x, y = workload(root)
    from rrl_hip import ops
    ones = [(x[b:b + 1, :COUNTS[b]].contiguous(), y[b:b + 1, :COUNTS[b]].contiguous()) for b in range(B)]  # the exact sizes
    fw = [_fwd(ops, a, c) for a, c in ones]
    fb = [_fwdbwd(ops, a, c) for a, c in ones]
    return {"loop8_fwd": lambda: [f() for f in fw], "loop8_fwdbwd": lambda: [f() for f in fb],
            "uniform_parent_fwd": _fwd(ops, x, y), "uniform_parent_fwdbwd": _fwdbwd(ops, x, y)}


def own_variants():
    x, y = workload(ROOT)
    import torch
    from rrl_hip import ops
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")  # noqa: E731
    cnt, full = i32(COUNTS), i32([CAP] * B)
    out = {"ragged_fwd": _fwd(ops, x, y, counts_x=cnt, counts_y=cnt), "ragged_fwdbwd": _fwdbwd(ops, x, y, counts_x=cnt, counts_y=cnt),
           "ragged_full_fwd": _fwd(ops, x, y, counts_x=full, counts_y=full),
           "uniform_fwd": _fwd(ops, x, y), "uniform_fwdbwd": _fwdbwd(ops, x, y)}
    return out, (x, y, cnt, full)


def child(root, steps, warmup):
    """Serve rounds over stdin / stdout: 'round' -> one JSON line of us per step for every parent variant; 'quit'."""
    v = parent_variants(root)
    for fn in v.values():
        timed(fn, warmup)
    print(json.dumps({"ready": sorted(v)}), flush=True)
    for line in sys.stdin:
        if line.strip() != "round":
            break
        print(json.dumps({k: timed(fn, steps) for k, fn in v.items()}), flush=True)


def read_json(proc):
    """The child's next JSON line (anything else it prints is passed on)."""
    while True:
        line = proc.stdout.readline()
        if not line:
            raise RuntimeError("the parent-library child process ended early")
        if line.startswith("{"):
            return json.loads(line)
        sys.stderr.write(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="checkout of the parent commit with its library built")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--steps-only", metavar="VARIANT", help="run only this variant's steps (kernel traces)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_chamfer_timing.json"))
    a = ap.parse_args()
    if a.child:
        return child(a.parent, a.steps, a.warmup)
    import torch
    own, (x, y, cnt, full) = own_variants()
    if a.steps_only:
        timed(own[a.steps_only], a.warmup)
        print(a.steps_only, round(timed(own[a.steps_only], a.steps), 2), "us per step")
        return
    for fn in own.values():
        timed(fn, a.warmup)
    from rrl_hip import ops
    # what the ragged call computes: with the counts at the capacities, the uniform call's bits; with COUNTS, per sample the
    # B = 1 call's on the truncated clouds
    same_full = torch.equal(ops.chamfer(x, y, counts_x=full, counts_y=full), ops.chamfer(x, y))
    vals = ops.chamfer(x, y, counts_x=cnt, counts_y=cnt, per_sample=True)
    same_each = all(torch.equal(vals[b], ops.chamfer(x[b:b + 1, :COUNTS[b]].contiguous(), y[b:b + 1, :COUNTS[b]].contiguous())) for b in range(B))
    res = {k: [] for k in own}
    proc = None
    if a.parent:
        proc = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", "--parent", os.path.abspath(a.parent),
                                 "--steps", str(a.steps), "--warmup", str(a.warmup)], stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                                text=True, cwd=os.path.abspath(a.parent))
        ready = read_json(proc)
        res.update({k: [] for k in ready["ready"]})
    for _ in range(a.rounds):  # alternate: this process, then the parent's
        for k, fn in own.items():
            res[k].append(timed(fn, a.steps))
        if proc:
            proc.stdin.write("round\n")
            proc.stdin.flush()
            for k, v in read_json(proc).items():
                res[k].append(v)
    if proc:
        proc.stdin.write("quit\n")
        proc.stdin.close()
        proc.wait(timeout=60)
    rows = {k: {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2), "n": len(v)}
            for k, v in res.items()}
    doc = {"what": "us per call of the Chamfer distance (forward; forward + backward to x.grad and y.grad), B = 8, capacities 4096 / 4096, "
                   "one MI355X; rounds alternate between this tree and a child process on the parent commit's library",
           "device": torch.cuda.get_device_name(0), "counts": COUNTS, "rounds": a.rounds, "steps_per_round": a.steps,
           "full_counts_equal_uniform_bits": bool(same_full), "values_equal_the_b1_calls_bits": bool(same_each), "us_per_call": rows}
    if proc:
        med = lambda k: rows[k]["median_us"]  # noqa: E731
        doc["ratios"] = {f"loop8_over_ragged_{g}": round(med(f"loop8_{g}") / med(f"ragged_{g}"), 2) for g in ("fwd", "fwdbwd")}
        doc["ragged_faster_than_the_loop"] = all(med(f"ragged_{g}") < med(f"loop8_{g}") for g in ("fwd", "fwdbwd"))
        # (b) the uniform path keeps its speed: this tree's median within the spread of the parent's own rounds
        doc["uniform_within_parent_spread"] = {g: bool(med(f"uniform_{g}") <= rows[f"uniform_parent_{g}"]["max_us"]) for g in ("fwd", "fwdbwd")}
        doc["ratios"].update({f"uniform_over_uniform_parent_{g}": round(med(f"uniform_{g}") / med(f"uniform_parent_{g}"), 3) for g in ("fwd", "fwdbwd")})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
