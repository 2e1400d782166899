"""Timing of the Sinkhorn soft assignment (rrl_hip/sinkhorn.py) against the reference's formulation in
eager torch on the same GPU, in the same process.

  sizes         B = 8 at J = K = 1024 and at J = K = 1433 (the RPM trainer's 2048 points at 0.7 crop), n_iters = 5, slack on;
                and ragged at J = K = 1024 with counts 512 ... 1024 (the new path only: the torch formulation has no counts)
  baseline      rpm/models/rpmnet.py:48-118 and 214-222 restated below in torch (padded matrix, two logsumexp, two cat per
                iteration; exp, matmul, two sums), forward, and forward + autograd backward of sum(W gW) + sum(s gs) + sum(c gc)
  per call      us per call through Python: device events around a window of --steps calls, the two paths' windows
                interleaved, median of --rounds windows with min ... max
  device        the C entries called directly on buffers allocated once (rrl_sinkhorn_fwd; rrl_sinkhorn_fwd + rrl_sinkhorn_bwd): the
                host then issues a call in a fraction of its device time, the stream stays full, and the window measures the device.
                The baseline's eager windows are device-bound as they are (every one of its launches moves the whole matrix)
  launches      launches per forward / backward of the new path, from include/rrl.h (3 n + 2 each)

Writes --out (default profiles/sinkhorn_timing.json) and prints it.  With --parent DIR (a checkout of the parent commit with its
library built): `python bench.py` in this tree and in DIR, alternating, --bench-rounds times each."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "a-robust-registration-loss_amd"))

B, N_ITERS = 8, 5


def torch_head(log_alpha, xyz_ref, n_iters=N_ITERS, eps=1e-5):
    """The reference's formulation (slack on), eager torch."""
    import torch
    la = torch.nn.functional.pad(log_alpha, (0, 1, 0, 1))
    for _ in range(n_iters):
        la = torch.cat((la[:, :-1, :] - torch.logsumexp(la[:, :-1, :], dim=2, keepdim=True), la[:, -1:, :]), dim=1)
        la = torch.cat((la[:, :, :-1] - torch.logsumexp(la[:, :, :-1], dim=1, keepdim=True), la[:, :, -1:]), dim=2)
    perm = torch.exp(la[:, :-1, :-1])
    s = perm.sum(2)
    return perm @ xyz_ref / (s[..., None] + eps), s, perm.sum(1)


def summary(v):
    return {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)}


def interleaved(fns, steps, warmup, rounds):
    """us per call of each fn: their windows alternate, round after round."""
    import torch
    for fn in fns:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(steps):
                fn()
            t1.record()
            torch.cuda.synchronize()
            out[i].append(t0.elapsed_time(t1) * 1e3 / steps)
    return [summary(v) for v in out]


def rows(a):
    import torch
    from rrl_hip import ops, sinkhorn
    out = []
    for J, counts in ((1024, None), (1433, None), (1024, [512, 585, 658, 731, 804, 877, 950, 1024])):
        g = torch.Generator().manual_seed(J)
        A = (10.0 * torch.randn(B, J, J, generator=g)).cuda()
        x = torch.rand(B, J, 3, generator=g).cuda()
        gW, gs, gc = torch.randn(B, J, 3, generator=g).cuda(), torch.randn(B, J, generator=g).cuda(), torch.randn(B, J, generator=g).cuda()
        Ag, xg = A.clone().requires_grad_(True), x.clone().requires_grad_(True)
        cnt = torch.tensor(counts, dtype=torch.int32).cuda() if counts else None

        def new_fwd():
            return sinkhorn.soft_assign(A, x, n_iters=N_ITERS, counts_src=cnt, counts_ref=cnt)

        def new_both():
            W, s, c = sinkhorn.soft_assign(Ag, xg, n_iters=N_ITERS, counts_src=cnt, counts_ref=cnt)
            return torch.autograd.grad((W * gW).sum() + (s * gs).sum() + (c * gc).sum(), (Ag, xg))

        def ref_fwd():
            with torch.no_grad():
                return torch_head(A, x)

        def ref_both():
            W, s, c = torch_head(Ag, xg)
            return torch.autograd.grad((W * gW).sum() + (s * gs).sum() + (c * gc).sum(), (Ag, xg))
        row = {"B": B, "J": J, "K": J, "n_iters": N_ITERS, "slack": True, "counts": counts,
               "launches_forward": 3 * N_ITERS + 2, "launches_backward": 3 * N_ITERS + 2}
        if counts is None:
            W, s, c = new_fwd()
            Wr, sr, cr = ref_fwd()
            row["agreement_max_abs"] = {"W": float((W - Wr).abs().max()), "s": float((s - sr).abs().max()), "c": float((c - cr).abs().max())}
            fns = [new_fwd, ref_fwd, new_both, ref_both]
            names = ["forward", "torch_forward", "forward_backward", "torch_forward_backward"]
        else:
            fns, names = [new_fwd, new_both], ["forward", "forward_backward"]
        for name, r in zip(names, interleaved(fns, a.steps, a.warmup, a.rounds)):
            row[name] = r
        k = sinkhorn._call(A, x, N_ITERS, True, 1e-5, cnt, cnt, False)  # (the tuple keeps the buffers alive)
        gA, gx = torch.empty_like(A), torch.empty_like(x)

        def dev_fwd():
            ops._run(A.device, "rrl_sinkhorn_fwd", ctypes.byref(k[0]))

        def dev_both():
            dev_fwd()
            ops._run(A.device, "rrl_sinkhorn_bwd", ctypes.byref(k[0]), ops._p(gW), ops._p(gs), ops._p(gc), ops._p(gA), ops._p(gx))
        for name, r in zip(("device_forward", "device_forward_backward"), interleaved([dev_fwd, dev_both], a.steps, a.warmup, a.rounds)):
            row[name] = r
        if counts is None:
            row["speedup_forward"] = row["torch_forward"]["median_us"] / row["forward"]["median_us"]
            row["speedup_forward_backward"] = row["torch_forward_backward"]["median_us"] / row["forward_backward"]["median_us"]
            row["faster_in_both"] = row["speedup_forward"] > 1.0 and row["speedup_forward_backward"] > 1.0
        out.append(row)
    return out


def bench_series(parent, rounds):
    def one(cwd):
        res = subprocess.run([sys.executable, "bench.py"], cwd=cwd, capture_output=True, text=True, check=True).stdout
        return json.loads(res.strip().splitlines()[-1])["value"]
    mine, theirs = [], []
    for _ in range(rounds):
        mine.append(one(ROOT))
        theirs.append(one(parent))
    return {"command": "python bench.py", "rounds": rounds, "this_tree": mine, "parent_library": theirs,
            "this_tree_median": statistics.median(mine), "parent_min": min(theirs), "parent_max": max(theirs),
            "inside_parent_spread": min(theirs) <= statistics.median(mine) <= max(theirs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent", help="checkout of the parent commit with its library built")
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sinkhorn_timing.json"))
    a = ap.parse_args()
    import torch
    doc = {"what": "Sinkhorn soft assignment against the reference's formulation in eager torch on one MI355X: device events around "
                   "windows of %d calls, the paths' windows interleaved, median of %d windows" % (a.steps, a.rounds),
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "sinkhorn": rows(a)}
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
