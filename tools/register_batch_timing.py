"""One epoch of B = 8 registrations: PairRegistration.epoch (ONE call, rrl_register_epoch) against the loop of eight
rrl_demo_epoch calls -- the only one-call form before it.

Sizes: the demo's (BASELINE.json configs[0]: N = M = 1024 triangles, L = 20000 lines), eight synthetic pairs.

  batch_uniform          this tree, all rows, no monitor
  batch_uniform_monitor  this tree, all rows, each pair's Chamfer distance per epoch (what the demo's epoch also computes)
  batch_ragged           this tree, counts spread evenly from a quarter of the capacity up to all of it (no monitor: refused)
  loop8_uniform          the PARENT commit's library: eight rrl_demo_epoch calls per epoch, pipelined as the demo runs them
  loop8_ragged           ... on eight pairs of the exact ragged sizes

The parent's numbers come from a CHILD process that imports the package of a checkout of the parent commit (--parent DIR:
`git worktree add DIR HEAD~1`, then build its library there) -- two builds of one library cannot live in one process.
Rounds alternate between the two processes; every timed window ends in a device synchronisation; medians are reported.
Writes --out (default profiles/register_batch_timing.json) and prints it.  Kernel averages: run --steps-only VARIANT under
`rocprofv3 --kernel-trace --stats` in a run of its own."""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

B, CAP, LINES = 8, 1024, 20000
COUNTS = [CAP // 4 + (CAP - CAP // 4) * b // (B - 1) for b in range(B)]  # 256 .. 1024
LR = 1e-2


def pairs(root, counts):
    sys.path.insert(0, os.path.join(root, "a-robust-registration-loss_amd"))
    from rrl_hip import synth
    return [synth.make_pair(2000 + b, counts[b], counts[b]) for b in range(B)]


def timed(fn, steps):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / steps


def demo_loop(root, counts):
    """epoch() = eight rrl_demo_epoch calls, one per pair, each with the demo's own buffers and its sampler pipeline."""
    prs = pairs(root, counts)
    import numpy as np
    import torch
    import loss as LS
    from rrl_hip import ops
    demo = importlib.import_module("test_demo_optimized_Lie_Algebra")
    dev = torch.device("cuda:0")
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    calls, alive, rows = [], [], 16
    for p in prs:
        src, tar = cu(p["src"]), cu(p["tar"])
        src_tri, tar_tri = cu(p["src_tri"]).reshape(1, -1, 9), cu(p["tar_tri"]).reshape(1, -1, 9)
        bbox = LS.generate_bbox(tar[None])[0].to(dev)
        radius = (bbox[0, :] - bbox[-1, :]).norm(p=2).reshape(1)
        draw = demo._default_lines(radius, tar.mean(0), LINES, tar, dev, True)
        xi = torch.nn.Parameter(torch.zeros(6, device=dev))
        opt = demo._GatedAdam(xi, LR)
        reg = ops.RegistrationStep(src_tri, tar_tri, LINES, transpose_r=False)
        Rb, Tb = torch.empty(1, 3, 3, device=dev), torch.empty(1, 3, device=dev)
        ops._run(dev, "rrl_se3_exp", ops._p(xi.data), ops._p(Rb), ops._p(Tb), 1)
        lines = torch.zeros(1, LINES, 6, device=dev)
        box1 = ops.aabb(src.reshape(1, -1, 3))
        trace, slot, row = torch.zeros(rows, 3, device=dev), torch.zeros(1, dtype=torch.long, device=dev), torch.zeros(3, device=dev)
        call = demo._one_call_epoch(draw, reg, lines, box1, xi, opt, Rb, Tb, trace, slot, row, rows)
        # every pair its own generator state (the demo's is one per process; a pipelined count pass must find the counter
        # its write pass will read), and everything the call points into stays alive with it
        rng = ops.sampler_rng(dev).clone()
        call.keep[1].rng_state = ops._p(rng)
        calls.append(call)
        alive.append((p, src, tar, src_tri, tar_tri, draw, xi, opt, reg, Rb, Tb, lines, box1, trace, slot, row, rng))
    state = {"epoch": 0, "alive": alive}

    def epoch():
        for call in calls:
            call(state["epoch"])
        state["epoch"] += 1
    return epoch


def batch_epochs():
    import numpy as np
    import torch
    out, keep = {}, []
    for name, counts, monitor in (("batch_uniform", None, False), ("batch_uniform_monitor", None, True), ("batch_ragged", COUNTS, False)):
        prs = pairs(ROOT, counts or [CAP] * B)
        from rrl_hip import register
        src, tar = np.full((B, CAP, 9), np.nan, np.float32), np.full((B, CAP, 9), np.nan, np.float32)
        for b, p in enumerate(prs):
            src[b, :len(p["src_tri"])], tar[b, :len(p["tar_tri"])] = p["src_tri"], p["tar_tri"]
        reg = register.PairRegistration(torch.from_numpy(src).cuda(), torch.from_numpy(tar).cuda(), LINES, counts1=counts, counts2=counts,
                                        lr=LR, seed=17, monitor=monitor, table_rows=16)
        out[name] = reg.epoch
        keep.append(reg)
    return out, keep


def child(root, steps, warmup):
    """Serve rounds over stdin / stdout: 'round' -> one JSON line of us per epoch for both loops; anything else: quit."""
    v = {"loop8_uniform": demo_loop(root, [CAP] * B), "loop8_ragged": demo_loop(root, COUNTS)}
    for fn in v.values():
        timed(fn, warmup)
    print(json.dumps({"ready": sorted(v)}), flush=True)
    for line in sys.stdin:
        if line.strip() != "round":
            break
        print(json.dumps({k: timed(fn, steps) for k, fn in v.items()}), flush=True)


def read_json(proc):
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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--steps-only", metavar="VARIANT", help="run only this variant's epochs (kernel traces)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "register_batch_timing.json"))
    a = ap.parse_args()
    if a.child:
        return child(a.parent, a.steps, a.warmup)
    import torch
    own, keep = batch_epochs()
    if a.steps_only:
        timed(own[a.steps_only], a.warmup)
        print(a.steps_only, round(timed(own[a.steps_only], a.steps), 2), "us per epoch")
        return
    for fn in own.values():
        timed(fn, a.warmup)
    res = {k: [] for k in own}
    proc = None
    if a.parent:
        proc = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", "--parent", os.path.abspath(a.parent),
                                 "--steps", str(a.steps), "--warmup", str(a.warmup)], stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                                text=True, cwd=os.path.abspath(a.parent))
        res.update({k: [] for k in read_json(proc)["ready"]})
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
    valid = {k: [int(x) for x in (r.step.st.info[:, 0] > 0).tolist()] for k, r in zip(own, keep)}
    doc = {"what": "us per epoch of B = 8 registrations (N = M = 1024, L = 20000), one MI355X: PairRegistration.epoch (one call) "
                   "against eight rrl_demo_epoch calls in a child process on the parent commit's library; alternating rounds",
           "device": torch.cuda.get_device_name(0), "counts": COUNTS, "rounds": a.rounds, "epochs_per_round": a.steps,
           "pairs_with_a_populated_bucket_in_the_last_epoch": valid, "us_per_epoch": rows}
    if proc:
        med = lambda k: rows[k]["median_us"]  # noqa: E731
        doc["ratios"] = {"loop8_uniform_over_batch_uniform": round(med("loop8_uniform") / med("batch_uniform"), 2),
                         "loop8_uniform_over_batch_uniform_monitor": round(med("loop8_uniform") / med("batch_uniform_monitor"), 2),
                         "loop8_ragged_over_batch_ragged": round(med("loop8_ragged") / med("batch_ragged"), 2)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
