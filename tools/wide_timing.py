"""Forward + backward of ops.intersection_loss at the C2 shape (B = 8, N = M = 4096, L = 10000) for the narrow range
(1, 1, 5, 5) and the wide range (1, 1, 9, 9), in interleaved rounds in ONE process (same clocks, same allocator state
for both).  Each timed call is forward + loss.sum().backward() + a device synchronisation (the wide forward synchronises
once anyway: its hit-recovery check).  Prints one JSON line: median / min milliseconds per range and their ratio."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "a-robust-registration-loss_amd"))


def c2_batch(B, N, M, L, seed=700):
    import loss as LS
    from rrl_hip import synth
    prs = [synth.make_pair(seed + b, N, M) for b in range(B)]
    ln = []
    for b, p in enumerate(prs):
        torch.manual_seed(seed + b)
        ln.append(LS.Random_uniform_distribution_lines_batch_efficient_resample(
            torch.tensor([[float(p["radius"])]]), torch.from_numpy(p["center"]).reshape(1, 3), L,
            torch.from_numpy(p["src"]).cuda()[None], torch.from_numpy(p["tar"]).cuda()[None], "cuda")[0])
    t = lambda k: torch.from_numpy(np.stack([p[k] for p in prs])).cuda()  # noqa: E731
    return t("src_tri"), t("tar_tri"), torch.stack(ln).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--N", type=int, default=4096)
    ap.add_argument("--L", type=int, default=10000)
    a = ap.parse_args()
    from rrl_hip import ops
    tri1, tri2, lines = c2_batch(a.B, a.N, a.N, a.L)
    ranges = {"narrow_1_1_5_5": (1, 1, 5, 5), "wide_1_1_9_9": (1, 1, 9, 9)}
    times = {k: [] for k in ranges}
    info = {}

    def step(rng):
        p1 = tri1.detach().requires_grad_(True)
        lv, inf, _ = ops.intersection_loss(p1, tri2, lines, rng)
        lv.sum().backward()
        return inf

    for r in range(a.warmup + a.rounds):
        for k, rng in ranges.items():  # interleaved: both ranges see the same machine state round by round
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            inf = step(rng)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            if r >= a.warmup:
                times[k].append(dt)
            info[k] = inf.sum(0).tolist()
    st = ops.last_state()
    out = {"shape": {"B": a.B, "N": a.N, "M": a.N, "L": a.L}, "rounds": a.rounds, "warmup": a.warmup,
           "recovered_entries": int(st.status[1]), "recovery_mismatches": int(st.status[0])}
    for k in ranges:
        out[k] = {"median_ms": round(statistics.median(times[k]), 4), "min_ms": round(min(times[k]), 4),
                  "info_sum_nbuckets_nselected_nvalues_nan": info[k]}
    out["ratio_median"] = round(out["wide_1_1_9_9"]["median_ms"] / out["narrow_1_1_5_5"]["median_ms"], 3)
    out["ratio_min"] = round(out["wide_1_1_9_9"]["min_ms"] / out["narrow_1_1_5_5"]["min_ms"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
