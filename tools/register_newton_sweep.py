"""The sweep behind NewtonRegistration's defaults (rrl_hip/newton.py): damping in {0, 1e-3, 1e-2, 1e-1} x
step in {0.5, 1} on the demo's shape (N = M = 1024, L = 20000), synth.make_pair at 10, 20 and 30 degrees, with and without crop.

Per pair: the BASELINE is the existing loop, PairRegistration.run(1000) with the monitor, on the same pair and sampler seed; its
level is the Chamfer distance of its last epoch.  The eight settings then run side by side as ONE batch of eight copies of the
pair (per-pair damping and step; no stopping rule) for --epochs epochs; a setting's figure is the first epoch (counted from 1) at
which its Chamfer distance reaches the baseline's level, or null.  Also recorded, for the tolerances of the stopping rule: the
median and the largest applied step (|omega|; |v| as a fraction of the sampler radius) over the last quarter of the epochs,
where the pose only follows the line sets' noise.  Writes --out (default profiles/register_newton_sweep.json) and prints it."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "a-robust-registration-loss_amd"))

N, LINES, SEED = 1024, 20000, 31
DAMPINGS, STEPS = (0.0, 1e-3, 1e-2, 1e-1), (0.5, 1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--baseline-epochs", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "register_newton_sweep.json"))
    a = ap.parse_args()
    import torch
    from rrl_hip import newton, register, synth
    settings = [(d, s) for d in DAMPINGS for s in STEPS]
    B = len(settings)
    rows = []
    for deg in (10.0, 20.0, 30.0):
        for crop in (False, True):
            pr = synth.make_pair(3000 + int(deg) + int(crop), N, N, crop=crop, rot_deg=deg)
            src = torch.from_numpy(pr["src_tri"]).cuda().reshape(1, N, 9)
            tar = torch.from_numpy(pr["tar_tri"]).cuda().reshape(1, N, 9)
            base = register.PairRegistration(src, tar, LINES, seed=SEED, monitor=True, table_rows=a.baseline_epochs)
            base.run(a.baseline_epochs)
            hist = base.history()[0]
            level, start = hist[-1][2], hist[0][2]
            reg = newton.NewtonRegistration(src.expand(B, N, 9).contiguous(), tar.expand(B, N, 9).contiguous(), LINES, seed=SEED,
                                            monitor=True, table_rows=a.epochs, patience=0,
                                            damping=torch.tensor([d for d, _ in settings]), step=torch.tensor([s for _, s in settings]))
            tail = []
            for e in range(a.epochs):
                reg.epoch()
                if e >= a.epochs - a.epochs // 4:
                    tail.append((reg.last_step / torch.stack([torch.ones_like(reg.radius), reg.radius], 1)).cpu())
            tail = torch.stack(tail)  # (epochs, B, 2)
            out = []
            for b, (d, s) in enumerate(settings):
                cf = [h[2] for h in reg.history()[b]]
                reached = next((e + 1 for e, v in enumerate(cf) if v is not None and v <= level), None)
                out.append({"damping": d, "step": s, "epochs_to_baseline_level": reached, "chamfer_best": min(v for v in cf if v is not None),
                            "chamfer_last": cf[-1], "tail_rot_median": float(tail[:, b, 0].median()), "tail_rot_max": float(tail[:, b, 0].max()),
                            "tail_trans_median": float(tail[:, b, 1].median()), "tail_trans_max": float(tail[:, b, 1].max()),
                            "failed_last": int(reg.failed[b])})
            rows.append({"rot_deg": deg, "crop": crop, "chamfer_start": start, "baseline_chamfer_after_%d" % a.baseline_epochs: level,
                         "baseline_chamfer_best": min(h[2] for h in hist if h[2] is not None), "settings": out})
            print(json.dumps(rows[-1]), flush=True)
    summary = []
    for b, (d, s) in enumerate(settings):
        got = [r["settings"][b]["epochs_to_baseline_level"] for r in rows]
        summary.append({"damping": d, "step": s, "pairs_reached": sum(g is not None for g in got), "epochs": got,
                        "median_epochs_of_reached": statistics.median([g for g in got if g is not None]) if any(g is not None for g in got) else None})
    doc = {"what": "epochs until NewtonRegistration's Chamfer distance first reaches what PairRegistration.run(%d) ends at, same pair "
                   "and sampler seed; N = M = %d, L = %d, max_rot %g rad, max_trans %g of the radius, one MI355X"
                   % (a.baseline_epochs, N, LINES, newton.MAX_ROT, newton.MAX_TRANS),
           "device": torch.cuda.get_device_name(0), "newton_epochs": a.epochs, "pairs": rows, "summary": summary}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc["summary"]))


if __name__ == "__main__":
    main()
