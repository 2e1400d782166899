"""Timing of the softmax pointer (rrl_hip/pointer.py) against the reference's formulation in eager torch
on the same GPU, in the same process.

  sizes         B = 8, C = 512 at N = M = 1024 and at N = M = 2048; and ragged at N = M = 1024 with counts 512 ... 1024 (the new
                path only: the torch formulation has no counts)
  baseline      dcp/model.py:419-425 restated below in torch (matmul, division, softmax, transpose().contiguous(), matmul),
                forward, and forward + autograd backward of sum(corr g)
  per call      us per call through Python: device events around a window of --steps calls, the two paths' windows
                interleaved, median of --rounds windows with min ... max
  device        the C entries called directly on buffers allocated once (rrl_pointer_fwd; rrl_pointer_fwd + rrl_pointer_bwd)
  memory        torch.cuda.max_memory_allocated over one forward + backward of either path at N = M = 2048, above what the
                inputs occupy
  accuracy      max |corr - float64| of both paths against the same formulation in float64 on the GPU, and their ratio
  matrix peak   the forward's 2 B C N M flop over its device time, as a share of --peak-tflops (157.3: the f32 matrix peak)

Writes --out (default profiles/pointer_timing.json) and prints it.  With --parent DIR (a checkout of the parent commit with its
library built): `python bench.py` in this tree and in DIR, alternating, --bench-rounds times each."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "a-robust-registration-loss_amd"))

B, C = 8, 512


def torch_head(src_emb, tgt_emb, tgt):
    """The reference's formulation, eager torch."""
    import torch
    scores = torch.matmul(src_emb.transpose(2, 1).contiguous(), tgt_emb) / math.sqrt(src_emb.size(1))
    scores = torch.softmax(scores, dim=2)
    return torch.matmul(tgt, scores.transpose(2, 1).contiguous())


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


def peak_bytes(fn):
    """Peak allocation of one call of fn above what is allocated before it."""
    import torch
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return int(peak)


def rows(a):
    import torch
    from rrl_hip import _lib, ops, pointer
    lib = _lib.load()
    out = []
    for N, counts in ((1024, None), (2048, None), (1024, [512, 585, 658, 731, 804, 877, 950, 1024])):
        gen = torch.Generator().manual_seed(N)
        se, te = torch.randn(B, C, N, generator=gen).cuda(), torch.randn(B, C, N, generator=gen).cuda()
        x, g = (torch.rand(B, 3, N, generator=gen) * 2 - 1).cuda(), torch.randn(B, 3, N, generator=gen).cuda()
        seg, teg, xg = (t.clone().requires_grad_(True) for t in (se, te, x))
        cnt = torch.tensor(counts, dtype=torch.int32).cuda() if counts else None

        def new_fwd():
            return pointer.soft_pointer(se, te, x, counts_src=cnt, counts_tgt=cnt)

        def new_both():
            return torch.autograd.grad((pointer.soft_pointer(seg, teg, xg, counts_src=cnt, counts_tgt=cnt) * g).sum(), (seg, teg, xg))

        def ref_fwd():
            with torch.no_grad():
                return torch_head(se, te, x)

        def ref_both():
            return torch.autograd.grad((torch_head(seg, teg, xg) * g).sum(), (seg, teg, xg))
        ws_bytes = int(lib.rrl_pointer_workspace_bytes(B, C, N, N))
        row = {"B": B, "C": C, "N": N, "M": N, "counts": counts, "launches_forward": 2, "launches_backward": 2,
               "workspace_bytes": ws_bytes, "score_matrix_bytes": B * N * N * 4}
        if counts is None:
            want = torch_head(se.double(), te.double(), x.double())
            mine, theirs = float((new_fwd().double() - want).abs().max()), float((ref_fwd().double() - want).abs().max())
            row["error_vs_float64"] = {"pointer": mine, "torch_float32": theirs, "ratio": mine / theirs if theirs else None}
            del want
            fns = [new_fwd, ref_fwd, new_both, ref_both]
            names = ["forward", "torch_forward", "forward_backward", "torch_forward_backward"]
        else:
            fns, names = [new_fwd, new_both], ["forward", "forward_backward"]
        for name, r in zip(names, interleaved(fns, a.steps, a.warmup, a.rounds)):
            row[name] = r
        ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=se.device)
        corr, info = torch.empty(B, 3, N, device=se.device), torch.empty(B, dtype=torch.int32, device=se.device)
        d = [torch.empty_like(t) for t in (se, te, x)]
        P = ops._p
        head = (P(se), P(te), P(x), P(cnt), P(cnt), P(ws), ws_bytes)

        def dev_fwd():
            ops._run(se.device, "rrl_pointer_fwd", *head, P(corr), None, P(info), B, C, N, N)

        def dev_both():
            dev_fwd()
            ops._run(se.device, "rrl_pointer_bwd", *head, P(g), P(d[0]), P(d[1]), P(d[2]), B, C, N, N)
        for name, r in zip(("device_forward", "device_forward_backward"), interleaved([dev_fwd, dev_both], a.steps, a.warmup, a.rounds)):
            row[name] = r
        if counts is None:
            row["speedup_forward"] = row["torch_forward"]["median_us"] / row["forward"]["median_us"]
            row["speedup_forward_backward"] = row["torch_forward_backward"]["median_us"] / row["forward_backward"]["median_us"]
            flop = 2.0 * B * C * N * N
            row["forward_share_of_f32_matrix_peak"] = flop / (row["device_forward"]["median_us"] * 1e-6) / (a.peak_tflops * 1e12)
            if N == 2048:
                row["peak_bytes_forward_backward"] = {"pointer": peak_bytes(new_both), "torch": peak_bytes(ref_both)}
        out.append(row)
    return out


def kernel_trace_workload(calls, N=1024):
    import torch
    from rrl_hip import _lib, ops
    gen = torch.Generator().manual_seed(N)
    se, te = torch.randn(B, C, N, generator=gen).cuda(), torch.randn(B, C, N, generator=gen).cuda()
    x, g = (torch.rand(B, 3, N, generator=gen) * 2 - 1).cuda(), torch.randn(B, 3, N, generator=gen).cuda()
    ws_bytes = int(_lib.load().rrl_pointer_workspace_bytes(B, C, N, N))
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=se.device)
    corr, d = torch.empty(B, 3, N, device=se.device), [torch.empty_like(t) for t in (se, te, x)]
    P = ops._p
    head = (P(se), P(te), P(x), None, None, P(ws), ws_bytes)
    for _ in range(calls):
        ops._run(se.device, "rrl_pointer_fwd", *head, P(corr), None, None, B, C, N, N)
        ops._run(se.device, "rrl_pointer_bwd", *head, P(g), P(d[0]), P(d[1]), P(d[2]), B, C, N, N)
    torch.cuda.synchronize()


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
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--peak-tflops", type=float, default=157.3)
    ap.add_argument("--parent", help="checkout of the parent commit with its library built")
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pointer_timing.json"))
    ap.add_argument("--calls", type=int, default=0, help="only issue this many forward + backward calls at N = M = 1024 through "
                    "the C entries and exit: the workload for `rocprofv3 --kernel-trace --stats`")
    a = ap.parse_args()
    import torch
    if a.calls:
        return kernel_trace_workload(a.calls)
    doc = {"what": "softmax pointer against the reference's formulation in eager torch on one MI355X: device events around "
                   "windows of %d calls, the paths' windows interleaved, median of %d windows" % (a.steps, a.rounds),
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "pointer": rows(a)}
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
