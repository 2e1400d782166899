"""The device-side pseudo-triangle builder, measured (writes profiles/pseudo_triangles_timing.json).

  knn3_self      the tree entry (rrl_knn3_self: build + walk, its scratch allocated once) against the brute-force kernel
                 that was there before (rrl_knn3 with query q = point q), at B = 1 for n = 1024 .. 262144 and at B = 8 for
                 n = 1024 and 4096, on two cloud kinds: `volume` (uniform in a cube) and `surface` (rrl_hip.synth's bumpy
                 ellipsoid).  n = 2^20: the tree only, with brute force's time extrapolated from 262144 (x 16); below that brute
                 force is not run either where the extrapolation from n / 4 exceeds BRUTE_LIMIT_S.
  whole          neighbors.pseudo_triangles(points, counts=device counts, order=True) at the trainers' shape, B = 8,
                 n = 1024 and 4096, per method; the Python call as a trainer makes it, allocations included.
  fps            rrl_fps_counted at the same shapes, S = 256: the time per sequential round.

Rounds alternate between the variants of one shape; every timed window ends in a device synchronisation; the figure is
the median of the rounds.  The crossover -- the smallest measured n from which the tree is faster on BOTH kinds at B = 1
and, where measured, at B = 8 -- is what neighbors.TREE_MIN_POINTS must hold.

Kernel split of the whole call: run `--steps-only whole_tree_4096` (any key of `whole`) under
`rocprofv3 --kernel-trace --stats` in a run of its own, then fold the CSV in with --kernel-stats CSV --label KEY."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "a-robust-registration-loss_amd"))

SIZES_B1 = [1024, 4096, 16384, 65536, 262144]
SIZES_B8 = [1024, 4096]
TREE_ONLY = 1 << 20
BRUTE_LIMIT_S = 3.0
KINDS = ("volume", "surface")
FPS_S = 256


def cloud(kind, seed, B, n):
    import numpy as np
    from rrl_hip import synth
    g = np.random.default_rng(seed)
    if kind == "volume":
        return g.uniform(-1.0, 1.0, (B, n, 3)).astype(np.float32)
    return np.stack([synth.surface_cloud(seed + 1000 * b, n) for b in range(B)])


def timed(fn, steps):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / steps


def knn_variants(kind, B, n, brute=True):
    import torch
    from rrl_hip import ops
    from rrl_hip.ops import _p, _run
    pts = torch.from_numpy(cloud(kind, 7 * n + B, B, n)).cuda()
    dev = pts.device
    nn_t = torch.empty(B, n, 3, dtype=torch.int32, device=dev)
    nn_b = torch.empty(B, n, 3, dtype=torch.int32, device=dev)
    ws = torch.empty(ops._scratch_size("rrl_knn3_self_workspace_bytes", B, n), dtype=torch.uint8, device=dev)
    q = torch.arange(n, dtype=torch.int32, device=dev).expand(B, -1).contiguous()
    v = {"tree": lambda: _run(dev, "rrl_knn3_self", _p(pts), None, _p(ws), ws.numel(), _p(nn_t), None, None, B, n)}
    if brute:
        v["brute"] = lambda: _run(dev, "rrl_knn3", _p(pts), _p(q), _p(nn_b), B, n, n)
    return v, (nn_t, nn_b)


def whole_variants(B, n):
    import torch
    from rrl_hip import neighbors
    from rrl_hip.ops import _p, _run
    pts = torch.from_numpy(cloud("surface", 99 + n, B, n)).cuda()
    cnt = torch.full((B,), n, dtype=torch.int32, device="cuda")
    st = torch.zeros(B, dtype=torch.int32, device="cuda")
    idx = torch.empty(B, FPS_S, dtype=torch.int32, device="cuda")
    scratch = torch.empty(B, n, dtype=torch.float32, device="cuda")
    v = {f"whole_{m}_{n}": (lambda m=m: neighbors.pseudo_triangles(pts, counts=cnt, method=m, order=True)) for m in ("tree", "brute")}
    v[f"fps{FPS_S}_{n}"] = lambda: _run(pts.device, "rrl_fps_counted", _p(pts), _p(cnt), _p(st), _p(idx), None, _p(scratch), B, n, FPS_S)
    return v


def steps_for(us):
    return max(2, min(200, int(2.0e5 / max(us, 1.0))))


def measure(variants, rounds):
    """{name: median us} over alternating rounds; the step count of a variant follows its first (warm-up) timing."""
    steps = {}
    for k, fn in variants.items():
        timed(fn, 1)
        steps[k] = steps_for(timed(fn, 2))
    rows = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            rows[k].append(timed(fn, steps[k]))
    return {k: statistics.median(r) for k, r in rows.items()}, steps


def fold_kernel_stats(out_path, csv_path, label):
    with open(out_path) as f:
        doc = json.load(f)
    rows = []
    with open(csv_path) as f:
        for r in csv.DictReader(f):
            rows.append({"kernel": r.get("Name") or r.get("KernelName"), "calls": int(r["Calls"]),
                         "avg_us": float(r["AverageNs"]) / 1e3, "percent": float(r["Percentage"])})
    doc.setdefault("kernel_split", {})[label] = rows
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps-only", metavar="KEY", help="run only this `whole` variant, 20 times (kernel traces)")
    ap.add_argument("--kernel-stats", metavar="CSV", help="fold a rocprofv3 --stats kernel CSV into --out under --label")
    ap.add_argument("--label")
    ap.add_argument("--max-n", type=int, default=TREE_ONLY)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pseudo_triangles_timing.json"))
    a = ap.parse_args()
    if a.kernel_stats:
        fold_kernel_stats(a.out, a.kernel_stats, a.label or os.path.basename(a.kernel_stats))
        return
    import torch
    from rrl_hip import neighbors, ops
    if a.steps_only:
        n = int(a.steps_only.rsplit("_", 1)[1])
        fn = whole_variants(8, n)[a.steps_only]
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        return
    doc = {"device": torch.cuda.get_device_name(0), "library": ops.version() if hasattr(ops, "version") else None,
           "rounds": a.rounds, "unit": "us per call, median of alternating rounds", "knn3_self": [], "whole": {}}
    faster = {}
    for B, sizes in ((1, SIZES_B1 + [TREE_ONLY]), (8, SIZES_B8)):
        for n in sizes:
            if n > a.max_n:
                continue
            for kind in KINDS:
                prev = next((r for r in doc["knn3_self"] if r["B"] == B and r["kind"] == kind and r["n"] * 4 == n and "brute_us" in r), None)
                est = prev["brute_us"] * 16 / 1e6 if prev else 0.0
                run_brute = n != TREE_ONLY and est <= BRUTE_LIMIT_S
                v, (nn_t, nn_b) = knn_variants(kind, B, n, run_brute)
                med, steps = measure(v, a.rounds)
                row = {"B": B, "n": n, "kind": kind, "tree_us": round(med["tree"], 1), "steps": steps}
                if run_brute:
                    row["brute_us"] = round(med["brute"], 1)
                    row["equal"] = bool(torch.equal(nn_t, nn_b))
                    faster.setdefault(n, []).append(med["tree"] < med["brute"])
                else:
                    prev4 = next((r for r in doc["knn3_self"] if r["B"] == B and r["kind"] == kind and r["n"] * 4 == n and "brute_us" in r), None)
                    row["brute_not_run"] = (f"extrapolated from n = {n // 4}: {prev4['brute_us'] * 16 / 1e6:.1f} s per call" if prev4
                                            else "not run")
                doc["knn3_self"].append(row)
                print(json.dumps(row), flush=True)
                del v, nn_t, nn_b
                torch.cuda.empty_cache()
    for n in SIZES_B8:
        med, steps = measure(whole_variants(8, n), a.rounds)
        for k, us in med.items():
            doc["whole"][k] = round(us, 1)
        doc["whole"][f"fps_us_per_round_{n}"] = round(med[f"fps{FPS_S}_{n}"] / FPS_S, 2)
        print(json.dumps({k: round(us, 1) for k, us in med.items()}), flush=True)
    sizes = sorted(faster)
    cross = None
    for n in reversed(sizes):  # the smallest n from which the tree wins everywhere measured, at that size and every larger one
        if all(faster[n]):
            cross = n
        else:
            break
    doc["crossover_n"] = cross
    doc["tree_min_points_in_library"] = neighbors.TREE_MIN_POINTS
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"crossover_n": cross, "out": a.out}))


if __name__ == "__main__":
    main()
