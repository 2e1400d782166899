"""Timing of the grouped PointNet (rrl_hip/pointnet.py encode_grouped, callsites.rpm_feat_prepool_pool)
against the reference's formulation as eager torch modules (Conv2d, GroupNorm, ReLU, torch.max over the slots) on the same GPU,
in the same process, with the same weights.

  shapes        B = 8 and B = 2 (two clouds per call) at N = 1024 and 717, S = 64, c0 = 10, widths 96 / 96 / 192
  per row       forward and forward + backward to the input and every parameter: us per call (device events around a window of
                --steps calls, the paths' windows interleaved, median of --rounds windows with min ... max;
                tools/fmr_head_timing.py's helpers) and torch.cuda.max_memory_allocated of either path
  --kernels     instead: --steps forward + backward calls of the library path at B = 8, N = 1024 and nothing else, the program
                to run under `rocprofv3 --kernel-trace --stats` (a run of its own)

Writes --out (default profiles/pointnet_group_timing.json) and prints it.  With --parent DIR (a checkout of the parent commit
with its library built): `python bench.py` in this tree and in DIR, alternating, --bench-rounds times each."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "a-robust-registration-loss_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fmr_head_timing as FH  # noqa: E402  (the interleaved windows, the bench series)
from pointnet_timing import peak  # noqa: E402

S, C0, FEATURE_DIM = 64, 10, 96
SHAPES = ((8, 1024), (2, 1024), (8, 717), (2, 717))


def raw_features(B, N, seed):
    """Standard-normal raw features with ball-query's padding: the slots from a per-point count on repeat the first slot."""
    import torch
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, N, S, C0, generator=gen)
    count = torch.randint(8, S + 1, (B, N, 1, 1), generator=gen)
    pad = torch.arange(S).reshape(1, 1, S, 1) >= count
    return torch.where(pad, x[:, :, :1], x).cuda().contiguous()


def paths(B, N):
    import torch
    from rrl_hip import pointnet
    torch.manual_seed(0)
    mine = pointnet.GroupedEncoder.rpm_feat_prepool(C0, FEATURE_DIM).cuda()
    ref = mine.prepool                       # the same torch modules: the reference's get_prepool stack
    x = raw_features(B, N, B + N).requires_grad_(True)
    leaves = [x] + list(mine.parameters())

    def torch_out():
        return torch.max(ref(x.permute(0, 3, 2, 1)), 2)[0]

    def lib_fwd():
        with torch.no_grad():
            return mine(x)

    def torch_fwd():
        with torch.no_grad():
            return torch_out()

    def lib_both():
        return torch.autograd.grad(mine(x).sum(), leaves)

    def torch_both():
        return torch.autograd.grad(torch_out().sum(), leaves)
    names = ["grouped_forward", "torch_forward", "grouped_forward_backward", "torch_forward_backward"]
    return names, [lib_fwd, torch_fwd, lib_both, torch_both]


def rows(a):
    out = []
    for B, N in SHAPES:
        names, fns = paths(B, N)
        row = {"B": B, "N": N, "S": S, "c0": C0, "widths": [FEATURE_DIM, FEATURE_DIM, 2 * FEATURE_DIM]}
        row["max_abs_difference_of_the_outputs"] = float((fns[0]() - fns[1]()).abs().max())
        both = list(zip(fns[2](), fns[3]()))
        row["max_abs_difference_of_the_gradients"] = max(float((p - q).abs().max()) for p, q in both)
        row["max_abs_gradient"] = max(float(q.abs().max()) for _, q in both)
        del both
        for name, r in zip(names, FH.interleaved(fns, a.steps, a.warmup, a.rounds)):
            row[name] = r
        row["speedup_forward"] = row["torch_forward"]["median_us"] / row["grouped_forward"]["median_us"]
        row["speedup_forward_backward"] = row["torch_forward_backward"]["median_us"] / row["grouped_forward_backward"]["median_us"]
        row["peak_bytes"] = {n: peak(f) for n, f in zip(names, fns)}
        row["launches"] = {n: FH.launches(f) for n, f in zip(names, fns)}
        out.append(row)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--kernels", action="store_true", help="only --steps forward + backward calls at B = 8, N = 1024 (for rocprofv3)")
    ap.add_argument("--parent", help="checkout of the parent commit with its library built")
    ap.add_argument("--bench-rounds", type=int, default=5)
    ap.add_argument("--bench-only", action="store_true", help="with --parent: only the bench series, written to --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pointnet_group_timing.json"))
    a = ap.parse_args()
    import torch
    if a.kernels:
        _, fns = paths(8, 1024)
        for _ in range(a.steps):
            fns[2]()
        torch.cuda.synchronize()
        return
    if a.bench_only:
        doc = {"bench": FH.bench_series(os.path.abspath(a.parent), a.bench_rounds)}
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        print(json.dumps(doc))
        return
    doc = {"what": "the grouped PointNet against the reference's formulation as eager torch modules on one MI355X: device events "
                   "around windows of %d calls, the paths' windows interleaved, median of %d windows" % (a.steps, a.rounds),
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "rows": rows(a)}
    torch.cuda.synchronize()
    if a.parent:
        doc["bench"] = FH.bench_series(os.path.abspath(a.parent), a.bench_rounds)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
