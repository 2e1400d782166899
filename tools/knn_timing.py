"""Timing of the k-nearest-neighbour entry (include/rrl.h rrl_knn; rrl_hip/neighbors.py knn, knn_group, estimate_normals_knn;
rrl_hip/callsites.py dcp_graph_feature) on one MI355X, everything in one process.

  method        device events around a window of calls, the windows of the paths that are compared interleaved round after
                round, median of --rounds windows with min ... max.  The calls per window follow from a first timed call so
                that a window lasts about --window-ms (at least 1 call, at most --steps)
  (a) dcp       B = 8, k = 20, N = 1024 and 2048: callsites.dcp_graph_feature against the reference's formulation
                (dcp/model.py:46-78, restated below) in eager torch -- per call through Python -- and the C entry on
                buffers allocated once (the stream stays full: device time)
  (b) tree      tree against brute force, self form, k = 20 and k = 3, B = 1 and B = 8, n = 256 ... 262144 (x 4), on a
                `volume` cloud (uniform in a cube) and a `surface` cloud (rrl_hip.synth's bumpy sphere); C entry, preallocated.
                At k = 3 also rrl_knn3_self: what the general kernel costs over the specialised one.
                tree_min_points = the smallest measured n from which the tree wins on both kinds, both batch sizes and both
                k, at that n and at every larger one; null if there is none
  (c) cross     the cross form, S = n = 1024, 4096, 16384, B = 8, k = 20: tree and brute force
  (d) normals   estimate_normals_knn(k = 20) against estimate_normals(radius 0.3, 64) at n = 1024, B = 8
  (e) bench     with --parent DIR (a checkout of the parent commit with its library built): `python bench.py` in this tree and
                in DIR, alternating, --bench-rounds times each

Writes --out (default profiles/knn_timing.json) and prints it."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "a-robust-registration-loss_amd"))

KINDS = ("volume", "surface")
TREE_SIZES = (256, 1024, 4096, 16384, 65536, 262144)
BRUTE = 4  # RRL_KNN_BRUTE


def cloud(kind, seed, B, n):
    import numpy as np
    import torch
    from rrl_hip import synth
    if kind == "volume":
        x = np.random.default_rng(seed).uniform(-1, 1, (B, n, 3)).astype(np.float32)
    else:
        x = np.stack([synth.surface_cloud(seed + 1000 * b, n) for b in range(B)])
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()


def torch_graph_feature(x, k):
    """dcp/model.py:46-78 restated: x (B, 3, N) -> (B, 6, N, k), eager torch."""
    import torch
    inner = -2 * torch.matmul(x.transpose(2, 1).contiguous(), x)
    xx = torch.sum(x ** 2, dim=1, keepdim=True)
    idx = (-xx - inner - xx.transpose(2, 1).contiguous()).topk(k=k, dim=-1)[1]
    B, N, _ = idx.shape
    idx = (idx + torch.arange(0, B, device=x.device).view(-1, 1, 1) * N).view(-1)
    xt = x.transpose(2, 1).contiguous()
    feature = xt.view(B * N, -1)[idx, :].view(B, N, k, 3)
    xr = xt.view(B, N, 1, 3).repeat(1, 1, k, 1)
    return torch.cat((feature, xr), dim=3).permute(0, 3, 1, 2)


def summary(v):
    return {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)}


def timed(fn, steps):
    import torch
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / steps


def interleaved(fns, a):
    """{name: summary} of us per call: a warm-up call, a timed call that sizes the window, then the windows alternate."""
    steps = {}
    for name, fn in fns.items():
        fn()
        steps[name] = max(1, min(a.steps, int(a.window_ms * 1e3 / max(timed(fn, 1), 1.0))))
    out = {name: [] for name in fns}
    for _ in range(a.rounds):
        for name, fn in fns.items():
            out[name].append(timed(fn, steps[name]))
    return {name: dict(summary(v), calls_per_window=steps[name]) for name, v in out.items()}


def c_entry(x, k, flags=0, query=None, channels=0):
    """A closure around rrl_knn on buffers allocated once (kept alive by the closure)."""
    import torch
    from rrl_hip import ops
    B, n = x.shape[:2]
    S = n if query is None else query.shape[1]
    idx = torch.empty(B, S, k, dtype=torch.int32, device="cuda")
    found = torch.empty(B, S, dtype=torch.int32, device="cuda")
    C = 3 * bin(channels).count("1")
    feat = torch.empty(B, max(C, 1), S, k, device="cuda") if channels else None
    ws = torch.empty(ops._scratch_size("rrl_knn_workspace_bytes", B, n, S), dtype=torch.uint8, device="cuda")

    def call():
        ops._run(x.device, "rrl_knn", ops._p(x), None, ops._p(query), None, k, flags, channels, ops._p(ws), ws.numel(), ops._p(idx),
                 ops._p(found), None, ops._p(feat), B, n, S)
    call.outputs = (idx, found, feat)
    return call


def knn3_entry(x):
    import torch
    from rrl_hip import ops
    B, n = x.shape[:2]
    nn = torch.empty(B, n, 3, dtype=torch.int32, device="cuda")
    ws = torch.empty(ops._scratch_size("rrl_knn3_self_workspace_bytes", B, n), dtype=torch.uint8, device="cuda")

    def call():
        ops._run(x.device, "rrl_knn3_self", ops._p(x), None, ops._p(ws), ws.numel(), ops._p(nn), None, None, B, n)
    call.outputs = (nn,)
    return call


def dcp_rows(a):
    import torch
    from rrl_hip import callsites
    out = []
    for n in (1024, 2048):
        x = cloud("surface", 500 + n, 8, n)
        xc = x.transpose(2, 1).contiguous()
        mine, theirs = callsites.dcp_graph_feature(xc, 20), torch_graph_feature(xc, 20)
        same = (mine == theirs).all(1).all(-1)  # (B, N): rows whose 20 neighbours agree, in order
        tree, brute = c_entry(x, 20, 2, channels=5), c_entry(x, 20, 2 | BRUTE, channels=5)
        tree(), brute()
        torch.cuda.synchronize()
        row = {"B": 8, "N": n, "k": 20, "output_megabytes": mine.numel() * 4 / 1e6, "rows_equal_to_the_matmul_form": float(same.float().mean()),
               "tree_equals_brute": all(torch.equal(u, v) for u, v in zip(tree.outputs, brute.outputs))}
        row.update(interleaved({"per_call": lambda: callsites.dcp_graph_feature(xc, 20), "torch_per_call": lambda: torch_graph_feature(xc, 20)}, a))
        row.update(interleaved({"device_tree": tree, "device_brute": brute}, a))
        row["speedup_per_call"] = row["torch_per_call"]["median_us"] / row["per_call"]["median_us"]
        row["speedup_device"] = row["torch_per_call"]["median_us"] / min(row["device_tree"]["median_us"], row["device_brute"]["median_us"])
        out.append(row)
        del mine, theirs
        torch.cuda.empty_cache()
    return out


def tree_rows(a):
    import torch
    out = []
    for n in TREE_SIZES:
        for B in (1, 8):
            for kind in KINDS:
                x = cloud(kind, 70 + n, B, n)
                for k in (20, 3):
                    fns = {"tree": c_entry(x, k), "brute": c_entry(x, k, BRUTE)}
                    if k == 3:
                        fns["knn3_self"] = knn3_entry(x)
                    row = {"n": n, "B": B, "kind": kind, "k": k}
                    row.update(interleaved(fns, a))
                    row["tree_equals_brute"] = all(torch.equal(u, v) for u, v in zip(fns["tree"].outputs[:2], fns["brute"].outputs[:2]))
                    if k == 3:
                        row["equals_knn3_self"] = torch.equal(fns["tree"].outputs[0], fns["knn3_self"].outputs[0])
                        row["general_over_knn3_self"] = row["tree"]["median_us"] / row["knn3_self"]["median_us"]
                    row["tree_wins"] = row["tree"]["median_us"] < row["brute"]["median_us"]
                    out.append(row)
                    print(json.dumps(row), file=sys.stderr, flush=True)
                    del fns
                del x
                torch.cuda.empty_cache()
    wins = {n: all(r["tree_wins"] for r in out if r["n"] == n) for n in TREE_SIZES}
    best = None
    for n in reversed(TREE_SIZES):  # the smallest n from which the tree wins there and at every larger size
        if not wins[n]:
            break
        best = n
    return out, best


def cross_rows(a):
    import torch
    out = []
    for n in (1024, 4096, 16384):
        x, q = cloud("surface", 900 + n, 8, n), cloud("volume", 901 + n, 8, n) * 0.8
        fns = {"tree": c_entry(x, 20, 0, query=q), "brute": c_entry(x, 20, BRUTE, query=q)}
        row = {"n": n, "S": n, "B": 8, "k": 20}
        row.update(interleaved(fns, a))
        row["tree_equals_brute"] = all(torch.equal(u, v) for u, v in zip(fns["tree"].outputs[:2], fns["brute"].outputs[:2]))
        out.append(row)
        del fns, x, q
        torch.cuda.empty_cache()
    return out


def normals_row(a):
    from rrl_hip import neighbors
    x = cloud("surface", 333, 8, 1024)
    row = {"n": 1024, "B": 8, "k": 20, "radius": 0.3, "nsample": 64}
    row.update(interleaved({"estimate_normals_knn": lambda: neighbors.estimate_normals_knn(x, 20),
                            "estimate_normals": lambda: neighbors.estimate_normals(x, 0.3, 64)}, a))
    return row


def bench_series(parent, rounds):
    def one(cwd):
        res = subprocess.run([sys.executable, "bench.py"], cwd=cwd, capture_output=True, text=True, check=True).stdout
        value = json.loads(res.strip().splitlines()[-1])["value"]
        print("bench.py in", cwd, value, file=sys.stderr, flush=True)
        return value
    mine, theirs = [], []
    for i in range(rounds):  # the pair's order alternates: whichever runs second in a pair follows a process that just left the GPU
        for cwd in ((ROOT, parent) if i % 2 == 0 else (parent, ROOT)):
            (mine if cwd == ROOT else theirs).append(one(cwd))
    return {"command": "python bench.py", "rounds": rounds, "order": "alternating pairs, this tree first in the even ones",
            "this_tree": mine, "parent_library": theirs,
            "this_tree_median": statistics.median(mine), "parent_min": min(theirs), "parent_max": max(theirs),
            "inside_parent_spread": min(theirs) <= statistics.median(mine) <= max(theirs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50, help="most calls per window")
    ap.add_argument("--window-ms", type=float, default=20.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parts", default="abcd", help="which of (a) .. (d) to run")
    ap.add_argument("--parent", help="checkout of the parent commit with its library built: adds (e)")
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_timing.json"))
    a = ap.parse_args()
    import torch
    doc = {"what": "rrl_knn on one MI355X: device events around windows of about %g ms (at most %d calls), the compared paths' windows "
                   "interleaved, median of %d windows with min ... max" % (a.window_ms, a.steps, a.rounds),
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__}
    if "a" in a.parts:
        doc["dcp_graph_feature"] = dcp_rows(a)
    if "b" in a.parts:
        doc["tree_against_brute"], doc["tree_min_points"] = tree_rows(a)
    if "c" in a.parts:
        doc["cross_form"] = cross_rows(a)
    if "d" in a.parts:
        doc["normals"] = normals_row(a)
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
