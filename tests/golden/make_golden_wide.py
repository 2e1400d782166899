#!/usr/bin/env python3
"""Generate tests/golden/loss_wide.npz -- the reference's loss at WIDE bucket ranges (up to 8 hits per line) -- by
RUNNING THE REFERENCE, with the helpers of make_golden.py (same stubs, same reference import).

Run in the build container only (needs the reference checkout, see make_golden.py):

    python tests/golden/make_golden_wide.py

Inputs are the committed loss fixtures (12 pairs of the reference's own sample data, two synthetic pairs); the output
file holds only their names and the reference's outputs: per fixture and range the loss, points1.grad, the D values in
the reference's concatenation order and their lower median, plus points2.grad of one pair (a second backward with
points2 requiring grad).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (registers the stubs and imports the reference)

# the 12 pairs of the reference's sample data (demo_scale: its challenge pair) and the two synthetic pairs
FIXTURES = ("ref_airplane0", "ref_airplane1", "ref_airplane2", "ref_airplane3", "ref_airplane4", "ref_human0", "ref_human1",
            "ref_human2", "ref_real0", "ref_real1", "ref_real2", "demo_scale", "synth_s0", "synth_s1")
RANGES = ((1, 1, 9, 9), (2, 3, 8, 9), (1, 1, 7, 5), (5, 5, 9, 9))
GRAD2_PAIR, GRAD2_RANGE = "ref_human0", (1, 1, 9, 9)


def ref_grad2(tri1, tri2, lines, rng):
    p1 = MG.t(tri1)[None].clone().requires_grad_(True)
    p2 = MG.t(tri2)[None].clone().requires_grad_(True)
    out = MG.RL.cal_loss_intersection_batch_whole_median_pts_lines(*rng, p1, p2, MG.t(lines)[None], "cpu")
    out.backward()
    return np.float32(out.item()), p1.grad[0].numpy().copy(), p2.grad[0].numpy().copy()


def main():
    kw = dict(fixtures=np.array(FIXTURES), ranges=np.array(RANGES, np.int32))
    for name in FIXTURES:
        g = np.load(os.path.join(HERE, f"loss_{name}.npz"))
        for i, rng in enumerate(RANGES):
            res = MG.ref_loss_case(g["tri1"], g["tri2"], g["lines"], rng)
            kw[f"{name}_r{i}_empty"] = np.bool_(res["empty"])
            kw[f"{name}_r{i}_loss"] = res["loss"]
            if not res["empty"]:
                kw[f"{name}_r{i}_grad1"] = res["grad1"].astype(np.float32)
                kw[f"{name}_r{i}_D"] = res["D"]
                kw[f"{name}_r{i}_median"] = res["median"]
            print(f"{name} {rng}: loss {res['loss']} nD {len(res.get('D', []))}")
    g = np.load(os.path.join(HERE, f"loss_{GRAD2_PAIR}.npz"))
    lv, g1, g2 = ref_grad2(g["tri1"], g["tri2"], g["lines"], GRAD2_RANGE)
    kw.update(grad2_pair=np.array(GRAD2_PAIR), grad2_range=np.array(GRAD2_RANGE, np.int32), grad2_loss=lv, grad2_grad1=g1,
              grad2_grad2=g2)
    MG.save("loss_wide.npz", **kw)


if __name__ == "__main__":
    main()
