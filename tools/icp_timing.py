"""Timing and convergence of the closed-form fit and the ICP epoch (rrl_hip/kabsch.py, rrl_hip/icp.py).

  kabsch        us per kabsch forward, and per forward + backward, at B = 8 and n = 1024 and 4096 (random rigid pairs, weights)
  icp_epoch     us per IcpRegistration.epoch at B = 8, N = M = 1024: uniform, and ragged (counts 256 ... 1024); launches per epoch
                (counted from the entries the epoch issues: include/rrl.h states each one's launches)
  convergence   eight synth.make_pair pairs at 20 degrees, N = M = 1024: epochs until the default stopping rule ends each pair,
                the pose error there against the generating rotation (degrees) and translation, and the steps of the last epochs
                (what the default tolerances are read from)
  bench         with --parent DIR (a checkout of the parent commit with its library built): `python bench.py` in this tree and
                in DIR, alternating, --bench-rounds times each; both series of the headline value

Every time is device events around a window of --steps calls after a warm-up, the median of --rounds windows.  Writes --out
(default profiles/icp_timing.json) and prints it."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "a-robust-registration-loss_amd"))

B, N = 8, 1024


def window_us(fn, steps, warmup, rounds):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(steps):
            fn()
        t1.record()
        torch.cuda.synchronize()
        out.append(t0.elapsed_time(t1) * 1e3 / steps)
    return {"median_us": statistics.median(out), "min_us": min(out), "max_us": max(out)}


def kabsch_rows(a):
    import torch
    from rrl_hip import kabsch
    rows = []
    for n in (1024, 4096):
        g = torch.Generator().manual_seed(n)
        x = torch.rand(B, n, 3, generator=g)
        y = (x @ torch.linalg.qr(torch.randn(3, 3, generator=g))[0] + 0.01 * torch.randn(B, n, 3, generator=g)).cuda()
        x, w = x.cuda(), torch.rand(B, n, generator=g).cuda()
        xg, yg, wg = (t.clone().requires_grad_(True) for t in (x, y, w))

        def fwd():
            kabsch.kabsch(x, y, w)

        def both():
            R, T = kabsch.kabsch(xg, yg, wg)
            torch.autograd.backward((R, T), (torch.ones_like(R), torch.ones_like(T)))
            xg.grad = yg.grad = wg.grad = None
        rows.append({"B": B, "n": n, "forward": window_us(fwd, a.steps, a.warmup, a.rounds),
                     "forward_backward": window_us(both, a.steps, a.warmup, a.rounds),
                     "launches_forward": 1 if n <= 512 else 2, "launches_backward": 1})
    return rows


def pairs(deg, seeds, counts=None):
    import numpy as np
    import torch
    from rrl_hip import synth
    src, tar, rots = np.full((len(seeds), N, 3), np.nan, np.float32), np.full((len(seeds), N, 3), np.nan, np.float32), []
    for b, s in enumerate(seeds):
        c = N if counts is None else counts[b]
        pr = synth.make_pair(s, c, c, rot_deg=deg)
        src[b, :c], tar[b, :c] = pr["src"], pr["tar"]
        rs = np.random.default_rng(s)  # make_pair's own stream: the axis is its third draw
        synth._surface(rs, c), synth._surface(rs, c)
        rots.append(synth._rotation(rs.standard_normal(3), deg))
    return torch.from_numpy(src).cuda(), torch.from_numpy(tar).cuda(), rots


def icp_rows(a):
    from rrl_hip import icp
    rows = []
    for name, counts in (("uniform", None), ("ragged", [256, 384, 512, 640, 768, 896, 960, 1024])):
        src, tar, _ = pairs(20.0, range(900, 900 + B), counts)
        reg = icp.IcpRegistration(src, tar, counts1=counts, counts2=counts, patience=0)
        rows.append({"batch": name, "B": B, "N": N, "M": N, "counts": counts, "epoch": window_us(reg.epoch, a.steps, a.warmup, a.rounds),
                     # rigid apply 1, counted Chamfer walk with prepared orders 2 (records + walk), fit 2 (n > 512), pose step 1
                     "launches_per_epoch": 1 + 2 + 2 + 1})
    return rows


def convergence(a):
    import numpy as np
    from rrl_hip import icp
    src, tar, rots = pairs(20.0, range(700, 700 + B))
    reg = icp.IcpRegistration(src, tar, table_rows=a.max_epochs)
    steps = []
    for e in range(a.max_epochs):
        reg.epoch()
        steps.append((reg.last_step.cpu().numpy() / np.stack([np.ones(B, np.float32), reg.radius.cpu().numpy()], 1)).tolist())
        if bool((reg.done_epoch >= 0).all()):
            break
    R, T, done = reg.R.double().cpu().numpy(), reg.T.double().cpu().numpy(), reg.done_epoch.tolist()
    rows = []
    for b in range(B):
        # make_pair: tar = surface Rgen^T + t (then centred): in the row convention the generating rotation is Rgen^T
        E = R[b].T @ rots[b].T
        ang = float(np.degrees(np.arccos(np.clip((np.trace(E) - 1) / 2, -1, 1))))
        rows.append({"pair": b, "done_epoch": done[b], "rotation_error_deg": ang, "chamfer_first": reg.history()[b][0][2],
                     "chamfer_last": reg.history()[b][-1][2], "residual_last": reg.history()[b][-1][1],
                     "last_steps_rot_rad": [s[b][0] for s in steps[-6:]], "last_steps_trans_of_diagonal": [s[b][1] for s in steps[-6:]]})
    return {"rot_deg": 20.0, "N": N, "M": N, "tol_rot": icp.TOL_ROT, "tol_trans": icp.TOL_TRANS, "patience": icp.PATIENCE,
            "epochs_run": len(steps), "pairs": rows}


def bench_series(parent, rounds):
    def one(cwd):
        out = subprocess.run([sys.executable, "bench.py"], cwd=cwd, capture_output=True, text=True, check=True).stdout
        return json.loads(out.strip().splitlines()[-1])["value"]
    mine, theirs = [], []
    for _ in range(rounds):
        mine.append(one(ROOT))
        theirs.append(one(parent))
    return {"command": "python bench.py", "rounds": rounds, "this_tree": mine, "parent_library": theirs,
            "this_tree_median": statistics.median(mine), "parent_min": min(theirs), "parent_max": max(theirs),
            "inside_parent_spread": min(theirs) <= statistics.median(mine) <= max(theirs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--max-epochs", type=int, default=200)
    ap.add_argument("--parent", help="checkout of the parent commit with its library built")
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_timing.json"))
    a = ap.parse_args()
    import torch
    doc = {"what": "closed-form fit and ICP epoch on one MI355X: device events around windows of %d calls, median of %d windows"
                   % (a.steps, a.rounds), "device": torch.cuda.get_device_name(0),
           "kabsch": kabsch_rows(a), "icp_epoch": icp_rows(a), "convergence": convergence(a)}
    torch.cuda.synchronize()
    if a.parent:
        doc["bench"] = bench_series(os.path.abspath(a.parent), a.bench_rounds)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
