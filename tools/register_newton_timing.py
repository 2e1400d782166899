"""One epoch of B = 8 registrations: NewtonRegistration.epoch (rrl_register_newton_epoch: forward + normal equations + Gauss-
Newton step) against PairRegistration.epoch (rrl_register_epoch: fused step + Adam) on the PARENT commit's library, and the
epochs and wall time either loop needs to the same Chamfer level.

Sizes: the demo's (N = M = 1024 triangles, L = 20000 lines), eight synthetic pairs (synth.make_pair(2000 + b), 20 degrees).

  newton_uniform / newton_uniform_monitor    this tree, without / with each pair's Chamfer distance per epoch
  adam_uniform / adam_uniform_monitor        the parent commit's library, PairRegistration.epoch, the same pairs

The parent's numbers come from a CHILD process that imports the package of a checkout of the parent commit (--parent DIR: a
checkout of HEAD~1 with its library built) -- two builds of one library cannot live in one process.  Rounds alternate between
the two processes; every timed window ends in a device synchronisation; medians are reported.  No ratio is fixed in advance.

Convergence (this process): PairRegistration.run(1000) with the monitor gives each pair's level (the Chamfer distance of its
last epoch) and the wall time of the existing loop; NewtonRegistration with the monitor and no stopping rule gives the first
epoch at which each pair reaches its level; a third object runs with the default stopping rule and check_every = 10.
Writes --out (default profiles/register_newton_timing.json) and prints it."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

B, CAP, LINES, SEED = 8, 1024, 20000, 17


def clouds(root):
    sys.path.insert(0, os.path.join(root, "a-robust-registration-loss_amd"))
    import numpy as np
    import torch
    from rrl_hip import synth
    prs = [synth.make_pair(2000 + b, CAP, CAP) for b in range(B)]
    return (torch.from_numpy(np.stack([p["src_tri"] for p in prs])).cuda(), torch.from_numpy(np.stack([p["tar_tri"] for p in prs])).cuda())


def timed(fn, steps):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / steps


def child(root, steps, warmup):
    """Serve rounds over stdin / stdout: 'round' -> one JSON line of us per epoch; anything else: quit."""
    src, tar = clouds(root)
    from rrl_hip import register
    regs = {"adam_uniform": register.PairRegistration(src, tar, LINES, lr=1e-2, seed=SEED, table_rows=16),
            "adam_uniform_monitor": register.PairRegistration(src, tar, LINES, lr=1e-2, seed=SEED, monitor=True, table_rows=16)}
    v = {k: r.epoch for k, r in regs.items()}
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


def convergence(src, tar, newton_epochs):
    import torch
    from rrl_hip import newton, ops, register
    tp = tar[:, :, :3].contiguous()
    base = register.PairRegistration(src, tar, LINES, seed=SEED, monitor=True, table_rows=1000)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    base.run(1000)
    torch.cuda.synchronize()
    adam_ms = (time.perf_counter() - t0) * 1e3
    level = [h[-1][2] for h in base.history()]
    reg = newton.NewtonRegistration(src, tar, LINES, seed=SEED, monitor=True, table_rows=newton_epochs, patience=0)
    reg.run(newton_epochs)
    reached = [next((e + 1 for e, h in enumerate(hh) if h[2] is not None and h[2] <= level[b]), None) for b, hh in enumerate(reg.history())]
    need = max([r for r in reached if r is not None], default=None)
    wall = None
    if need is not None:
        again = newton.NewtonRegistration(src, tar, LINES, seed=SEED, monitor=True, table_rows=16, patience=0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        again.run(need)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
    stop = newton.NewtonRegistration(src, tar, LINES, seed=SEED, table_rows=16)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    stop.run(1000, check_every=10)
    torch.cuda.synchronize()
    stop_ms = (time.perf_counter() - t0) * 1e3
    end = ops.chamfer(stop.moved_points().contiguous(), tp, per_sample=True).tolist()
    return {"adam_1000_epochs_wall_ms": round(adam_ms, 2), "adam_chamfer_after_1000": level,
            "newton_epochs_to_that_level": reached, "newton_wall_ms_to_the_last_pair": None if wall is None else round(wall, 2),
            "newton_epochs_run": newton_epochs,
            "stopping_rule": {"check_every": 10, "epochs_issued": stop.epochs, "done_epoch": stop.done_epoch.tolist(),
                              "wall_ms": round(stop_ms, 2), "chamfer_of_the_last_moved_points": end}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="checkout of the parent commit with its library built")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--newton-epochs", type=int, default=300)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "register_newton_timing.json"))
    a = ap.parse_args()
    if a.child:
        return child(a.parent, a.steps, a.warmup)
    import torch
    src, tar = clouds(ROOT)
    from rrl_hip import newton
    regs = {"newton_uniform": newton.NewtonRegistration(src, tar, LINES, seed=SEED, table_rows=16, patience=0),
            "newton_uniform_monitor": newton.NewtonRegistration(src, tar, LINES, seed=SEED, monitor=True, table_rows=16, patience=0)}
    own = {k: r.epoch for k, r in regs.items()}
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
    doc = {"what": "us per epoch of B = 8 registrations (N = M = 1024, L = 20000), one MI355X: NewtonRegistration.epoch against "
                   "PairRegistration.epoch in a child process on the parent commit's library, alternating rounds; and epochs / wall "
                   "time to the Chamfer level PairRegistration.run(1000) ends at",
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "epochs_per_round": a.steps, "us_per_epoch": rows,
           "convergence": convergence(src, tar, a.newton_epochs)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
