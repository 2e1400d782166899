"""Timing and convergence of robust ICP next to point-to-point ICP (rrl_hip/icp.py RobustIcpRegistration / IcpRegistration;
DESIGN.md section 20).

  epoch          us per .epoch() at B = 8, N = M = 1024, uniform and ragged (counts 256 ... 1024): IcpRegistration's epoch, the
                 robust loop's steady epoch and its init epoch (the one that also takes the median); the windows of the three
                 alternate, medians with min ... max; launches per epoch (counted from the entries an epoch issues: include/rrl.h
                 states each one's launches)
  acceptance     the pairs of tests/robust_refs.py outlier_pair(seed, 1024, 20 degrees, 20 % outliers), seeds 0 .. 7, as one batch
                 under the defaults: epochs to done, levels and final rotation error of the robust loop, and what IcpRegistration
                 ends at on the same batch
  bench          with --parent DIR (a checkout of the parent commit with its library built): `python bench.py` in this tree and
                 in DIR, alternating, in both orders, --bench-rounds times each

Every time is device events around a window of --steps calls after a warm-up.  Writes --out (default
profiles/robust_icp_timing.json) and prints it."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "a-robust-registration-loss_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))  # robust_refs: the acceptance pairs' recipe, stated once

B, N = 8, 1024
RAGGED = [256, 384, 512, 640, 768, 896, 960, 1024]


def window(fn, steps):
    import torch
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / steps


def summary(xs):
    return {"median_us": statistics.median(xs), "min_us": min(xs), "max_us": max(xs)}


def interleaved(fns, steps, warmup, rounds):
    """{name: summary}: the windows of the functions alternate, so that a drift of the machine meets all of them alike."""
    import torch
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            out[k].append(window(fn, steps))
    return {k: summary(v) for k, v in out.items()}


def outlier_batch(n, deg, counts=None):
    import numpy as np
    import torch
    import robust_refs as RR
    src, tar, rots = np.full((B, n, 3), np.nan, np.float32), np.full((B, n, 3), np.nan, np.float32), []
    for b in range(B):
        c = n if counts is None else counts[b]
        s, t, Rg = RR.outlier_pair(b, c, deg, 0.2)
        src[b, :c], tar[b, :c] = s, t
        rots.append(Rg)
    return torch.from_numpy(src).cuda(), torch.from_numpy(tar).cuda(), rots


def epoch_rows(a):
    from rrl_hip import icp
    rows = []
    for name, counts in (("uniform", None), ("ragged", RAGGED)):
        src, tar, _ = outlier_batch(N, 20.0, counts)
        point = icp.IcpRegistration(src, tar, counts1=counts, counts2=counts, patience=0)
        steady = icp.RobustIcpRegistration(src, tar, counts1=counts, counts2=counts, patience=0, level_cap=1 << 30)
        first = icp.RobustIcpRegistration(src, tar, counts1=counts, counts2=counts, patience=0, level_cap=1 << 30)
        steady.epoch()

        def init_epoch():
            first.epochs = 0  # (.epoch() passes init = 1 while no epoch has been issued)
            first.epoch()
        t = interleaved({"point": point.epoch, "steady": steady.epoch, "init": init_epoch}, a.steps, a.warmup, a.rounds)
        # rigid apply 1, counted Chamfer walk with prepared orders 2 (records + walk), sums 2 (N > 512), pose step 1; the robust
        # epoch adds the weights 1, its init epoch the median 1
        rows.append({"batch": name, "B": B, "N": N, "M": N, "counts": counts, "point_epoch": t["point"], "robust_steady_epoch": t["steady"],
                     "robust_init_epoch": t["init"], "steady_over_point": t["steady"]["median_us"] / t["point"]["median_us"],
                     "launches_per_epoch": {"point": 1 + 2 + 2 + 1, "robust_steady": 1 + 2 + 1 + 2 + 1, "robust_init": 1 + 2 + 1 + 1 + 2 + 1}})
    return rows


def acceptance(a):
    import robust_refs as RR
    from rrl_hip import icp
    src, tar, rots = outlier_batch(N, 20.0)
    rob = icp.RobustIcpRegistration(src, tar, table_rows=a.max_epochs).run(a.max_epochs, check_every=1)
    plain = icp.IcpRegistration(src, tar, table_rows=a.max_epochs).run(a.max_epochs, check_every=1)
    Rr, Rp = rob.R.double().cpu().numpy(), plain.R.double().cpu().numpy()
    rows = [{"pair": b, "robust_done_epoch": rob.done_epoch[b].item(), "robust_levels": rob.levels[b].item(),
             "robust_rotation_error_deg": RR.rot_err_deg(Rr[b], rots[b]), "nu_start": 3.0 * float(rob.med_sq[b].sqrt()), "nu_end": rob.nu_end[b].item(),
             "point_done_epoch": plain.done_epoch[b].item(), "point_rotation_error_deg": RR.rot_err_deg(Rp[b], rots[b])} for b in range(B)]
    return {"pairs_of": "tests/robust_refs.py outlier_pair(seed, 1024, 20.0, 0.2), seeds 0 .. 7", "nu_start": icp.NU_START, "anneal": icp.ANNEAL,
            "level_cap": icp.LEVEL_CAP, "tol_rot": icp.TOL_ROT, "tol_trans": icp.TOL_TRANS, "patience": icp.PATIENCE, "pairs": rows}


def bench_series(parent, rounds):
    def one(cwd):
        out = subprocess.run([sys.executable, "bench.py"], cwd=cwd, capture_output=True, text=True, check=True).stdout
        return json.loads(out.strip().splitlines()[-1])["value"]
    mine, theirs = [], []
    for r in range(rounds):  # both orders
        for who in (("mine", "theirs") if r % 2 == 0 else ("theirs", "mine")):
            (mine if who == "mine" else theirs).append(one(ROOT if who == "mine" else parent))
            print("bench", r, who, (mine if who == "mine" else theirs)[-1], file=sys.stderr, flush=True)
    return {"command": "python bench.py", "rounds": rounds, "this_tree": mine, "parent_library": theirs,
            "this_tree_median": statistics.median(mine), "parent_median": statistics.median(theirs), "parent_min": min(theirs),
            "parent_max": max(theirs), "inside_parent_spread": min(theirs) <= statistics.median(mine) <= max(theirs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--max-epochs", type=int, default=200)
    ap.add_argument("--parent", help="checkout of the parent commit with its library built")
    ap.add_argument("--bench-rounds", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "robust_icp_timing.json"))
    a = ap.parse_args()
    import torch
    doc = {"what": "robust ICP next to point-to-point ICP on one MI355X: device events around windows of %d calls, %d alternating "
                   "windows each" % (a.steps, a.rounds), "device": torch.cuda.get_device_name(0)}
    doc["epoch"] = epoch_rows(a)
    doc["acceptance"] = acceptance(a)
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
