"""Clouds beyond 65536 triangles on the sorted layout: one LossStep (rigid apply + loss + backward to points1.grad, one C
call) in scan mode cull against the same step in strict mode (the dense scan every cloud above 65536 triangles took before
the sort capacity was raised to 2^20), ops.chamfer with and without the tree, and ops.cloud_order -- at B = 1, L = 10000,
N = M in {65537, 131072, 307200, 2^20} (--sizes).  Clouds are scaled with their density so that lines hit them (see
tests/test_gpu_large_clouds.py).  Cull and strict run in interleaved rounds in ONE process; every timed call is followed by
a device synchronisation.  Writes --out (default profiles/large_clouds.json) and prints it."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "a-robust-registration-loss_amd"))


def scaled_pair(seed, n, L):
    import loss as LS
    from rrl_hip import synth
    s = np.float32(10.0 * math.sqrt(n / 65536.0))
    p = synth.make_pair(seed, n, n)
    p = {k: (v * s if isinstance(v, np.ndarray) or k == "radius" else v) for k, v in p.items()}
    torch.manual_seed(seed)
    ln = LS.Random_uniform_distribution_lines_batch_efficient_resample(
        torch.tensor([[float(p["radius"])]]), torch.from_numpy(p["center"]).reshape(1, 3), L,
        torch.from_numpy(p["src"]).cuda()[None], torch.from_numpy(p["tar"]).cuda()[None], "cuda")
    cu = lambda k: torch.from_numpy(np.ascontiguousarray(p[k])).cuda()[None]  # noqa: E731
    return cu("src_tri"), cu("tar_tri"), ln.contiguous(), cu("src"), cu("tar")


def timed(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6)
    return out


def stats(us):
    return {"median_us": round(statistics.median(us), 1), "min_us": round(min(us), 1), "n": len(us)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="65537,131072,307200,1048576")
    ap.add_argument("--L", type=int, default=10000)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "large_clouds.json"))
    a = ap.parse_args()
    from rrl_hip import ops
    R = torch.eye(3, device="cuda")[None].contiguous()
    t = torch.full((1, 3), 0.01, device="cuda")
    rows = []
    for n in [int(v) for v in a.sizes.split(",")]:
        src, tar, ln, xs, ys = scaled_pair(900 + n % 89, n, a.L)
        steps = {m: ops.LossStep(src, tar, a.L, mode=m) for m in ("cull", "strict")}
        res = {m: [] for m in steps}
        out = {}
        for m, st in steps.items():
            for _ in range(a.warmup):
                st(R, t, ln)
        for _ in range(a.rounds):  # interleaved: same clocks for both modes
            for m, st in steps.items():
                res[m] += timed(lambda: st(R, t, ln), 1)
        for m, st in steps.items():
            loss, _, info = st(R, t, ln)
            torch.cuda.synchronize()
            out[m] = (loss.clone(), info.clone())
        same = torch.equal(out["cull"][0].view(torch.int32), out["strict"][0].view(torch.int32))
        row = {"N": n, "M": n, "B": 1, "L": a.L, "prepared": steps["cull"].prepared,
               "step_cull": stats(res["cull"]), "step_strict": stats(res["strict"]),
               "strict_over_cull": round(statistics.median(res["strict"]) / statistics.median(res["cull"]), 2),
               "loss_bit_equal": bool(same), "selected": int(out["cull"][1][0, 1])}
        cham = {}
        for tree in (True, False):
            ops.CHAMFER_TREE = tree
            try:
                ops.chamfer(xs, ys)
                cham[tree] = timed(lambda: ops.chamfer(xs, ys), max(3, a.rounds // 2))
            finally:
                ops.CHAMFER_TREE = True
        row["chamfer_tree"], row["chamfer_brute"] = stats(cham[True]), stats(cham[False])
        ops.cloud_order(src)
        row["cloud_order"] = stats(timed(lambda: ops.cloud_order(src), max(3, a.rounds // 2)))
        rows.append(row)
        print(json.dumps(row), flush=True)
        del steps
        torch.cuda.empty_cache()
    doc = {"what": "LossStep cull vs strict, ops.chamfer tree vs brute force, ops.cloud_order; B = 1, one MI355X",
           "device": torch.cuda.get_device_name(0), "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
