"""Timing and convergence of point-to-plane ICP next to point-to-point ICP (rrl_hip/icp.py PlaneIcpRegistration /
IcpRegistration, rrl_hip/neighbors.py estimate_normals).

  epoch          us per .epoch() of both loops at B = 8, N = M = 1024, uniform and ragged (counts 256 ... 1024): the windows of the
                 two loops alternate, medians with min ... max; launches per epoch (counted from the entries an epoch issues:
                 include/rrl.h states each one's launches)
  normals        us per estimate_normals (ball query + normals, two launches) at B = 8, n = 1024 and 1433, radius 0.25, 64 members
  to_accuracy    eight synth.make_pair pairs at 20 degrees, N = M = 1024: IcpRegistration under its default stopping rule -> the
                 epochs it takes and the rotation error it ends at; then the epochs PlaneIcpRegistration takes to be at or below
                 that error, per pair, and both as wall time (epochs x the measured epoch time, the normals included once)
  convergence    PlaneIcpRegistration under its own default rule on the same pairs: done epoch, rotation error there, the last
                 steps (what the default tolerances are confirmed from)
  bench          with --parent DIR (a checkout of the parent commit with its library built): `python bench.py` in this tree and
                 in DIR, alternating, in both orders, --bench-rounds times each

Every time is device events around a window of --steps calls after a warm-up.  Writes --out (default
profiles/plane_icp_timing.json) and prints it."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "a-robust-registration-loss_amd"))

B, N = 8, 1024
RADIUS, NSAMPLE = 0.25, 64
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
        rots.append(synth._rotation(rs.standard_normal(3), deg).T)  # the row-convention rotation: src R ~ tar
    return torch.from_numpy(src).cuda(), torch.from_numpy(tar).cuda(), rots


def rot_err_deg(R, Rt):
    import numpy as np
    E = R.T @ Rt
    return float(np.degrees(np.arccos(np.clip((np.trace(E) - 1) / 2, -1, 1))))


def epoch_rows(a):
    from rrl_hip import icp
    rows = []
    for name, counts in (("uniform", None), ("ragged", RAGGED)):
        src, tar, _ = pairs(20.0, range(900, 900 + B), counts)
        point = icp.IcpRegistration(src, tar, counts1=counts, counts2=counts, patience=0)
        plane = icp.PlaneIcpRegistration(src, tar, normal_radius=RADIUS, nsample=NSAMPLE, counts1=counts, counts2=counts, patience=0)
        t = interleaved({"point": point.epoch, "plane": plane.epoch}, a.steps, a.warmup, a.rounds)
        # rigid apply 1, counted Chamfer walk with prepared orders 2 (records + walk), sums 2 (N > 512), pose step 1 -- both loops
        rows.append({"batch": name, "B": B, "N": N, "M": N, "counts": counts, "point_epoch": t["point"], "plane_epoch": t["plane"],
                     "launches_per_epoch": {"point": 1 + 2 + 2 + 1, "plane": 1 + 2 + 2 + 1}})
    return rows


def normals_rows(a):
    import torch
    from rrl_hip import neighbors, synth
    import numpy as np
    rows = []
    for n in (1024, 1433):
        x = torch.from_numpy(np.stack([synth.surface_cloud(300 + b, n) for b in range(B)])).cuda()
        t = interleaved({"normals": lambda: neighbors.estimate_normals(x, RADIUS, NSAMPLE)}, a.steps, a.warmup, a.rounds)
        nrm, q = neighbors.estimate_normals(x, RADIUS, NSAMPLE, return_quality=True)
        rows.append({"B": B, "n": n, "radius": RADIUS, "nsample": NSAMPLE, "estimate_normals": t["normals"], "launches": 2,
                     "zero_normals": int((~nrm.any(-1)).sum()), "least_quality_of_the_rest": float(q[nrm.any(-1)].min())})
    return rows


def to_accuracy(a, epoch_us, normals_us):
    import numpy as np
    from rrl_hip import icp
    src, tar, rots = pairs(20.0, range(700, 700 + B))
    point = icp.IcpRegistration(src, tar, table_rows=a.max_epochs).run(a.max_epochs, check_every=1)
    Rq, done_q = point.R.double().cpu().numpy(), point.done_epoch.tolist()
    target = [rot_err_deg(Rq[b], rots[b]) for b in range(B)]
    plane = icp.PlaneIcpRegistration(src, tar, normal_radius=RADIUS, nsample=NSAMPLE, patience=0)
    reached, errs = [None] * B, []
    for e in range(a.plane_epochs):
        plane.epoch()
        Rp = plane.R.double().cpu().numpy()
        errs.append([rot_err_deg(Rp[b], rots[b]) for b in range(B)])
        for b in range(B):
            if reached[b] is None and errs[-1][b] <= target[b]:
                reached[b] = e + 1
    rows = []
    for b in range(B):
        ep = done_q[b] if done_q[b] >= 0 else a.max_epochs
        rows.append({"pair": b, "point_epochs": ep, "point_rotation_error_deg": target[b], "point_wall_us": ep * epoch_us["point"],
                     "plane_epochs_to_that_error": reached[b],
                     "plane_wall_us": None if reached[b] is None else reached[b] * epoch_us["plane"] + normals_us,
                     "plane_rotation_error_deg_after": {str(k): errs[k - 1][b] for k in (5, 10, a.plane_epochs) if k <= len(errs)}})
    return {"rot_deg": 20.0, "N": N, "M": N, "normal_radius": RADIUS, "nsample": NSAMPLE, "epoch_us_used": epoch_us,
            "normals_us_used": normals_us, "pairs": rows}


def convergence(a):
    import numpy as np
    from rrl_hip import icp
    src, tar, rots = pairs(20.0, range(700, 700 + B))
    reg = icp.PlaneIcpRegistration(src, tar, normal_radius=RADIUS, nsample=NSAMPLE, table_rows=a.max_epochs)
    steps = []
    for e in range(a.max_epochs):
        reg.epoch()
        steps.append((reg.last_step.cpu().numpy() / np.stack([np.ones(B, np.float32), reg.radius.cpu().numpy()], 1)).tolist())
        if bool((reg.done_epoch >= 0).all()):
            break
    R, done, hist = reg.R.double().cpu().numpy(), reg.done_epoch.tolist(), reg.history()
    rows = [{"pair": b, "done_epoch": done[b], "rotation_error_deg": rot_err_deg(R[b], rots[b]), "chamfer_first": hist[b][0][2],
             "chamfer_last": hist[b][-1][2], "plane_residual_last": hist[b][-1][1],
             "steps_rot_rad": [s[b][0] for s in steps[:12]], "steps_trans_of_diagonal": [s[b][1] for s in steps[:12]]} for b in range(B)]
    return {"tol_rot": icp.PLANE_TOL_ROT, "tol_trans": icp.PLANE_TOL_TRANS, "patience": icp.PATIENCE, "epochs_run": len(steps), "pairs": rows}


def bench_series(parent, rounds):
    def one(cwd):
        out = subprocess.run([sys.executable, "bench.py"], cwd=cwd, capture_output=True, text=True, check=True).stdout
        return json.loads(out.strip().splitlines()[-1])["value"]
    mine, theirs = [], []
    for r in range(rounds):  # both orders
        for who in (("mine", "theirs") if r % 2 == 0 else ("theirs", "mine")):
            (mine if who == "mine" else theirs).append(one(ROOT if who == "mine" else parent))
    return {"command": "python bench.py", "rounds": rounds, "this_tree": mine, "parent_library": theirs,
            "this_tree_median": statistics.median(mine), "parent_median": statistics.median(theirs), "parent_min": min(theirs),
            "parent_max": max(theirs), "inside_parent_spread": min(theirs) <= statistics.median(mine) <= max(theirs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--max-epochs", type=int, default=200)
    ap.add_argument("--plane-epochs", type=int, default=30)
    ap.add_argument("--parent", help="checkout of the parent commit with its library built")
    ap.add_argument("--bench-rounds", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plane_icp_timing.json"))
    a = ap.parse_args()
    import torch
    doc = {"what": "point-to-plane ICP next to point-to-point ICP on one MI355X: device events around windows of %d calls, %d "
                   "alternating windows each" % (a.steps, a.rounds), "device": torch.cuda.get_device_name(0)}
    doc["epoch"] = epoch_rows(a)
    doc["normals"] = normals_rows(a)
    uniform = doc["epoch"][0]
    doc["to_accuracy"] = to_accuracy(a, {"point": uniform["point_epoch"]["median_us"], "plane": uniform["plane_epoch"]["median_us"]},
                                     doc["normals"][0]["estimate_normals"]["median_us"])
    doc["convergence"] = convergence(a)
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
