"""Timing of the attention node (rrl_hip/attention.py) against the reference's formulation in eager torch
on the same GPU, in the same process.

  sizes         B = 8, H = 4, DK = 128 at N = M = 1024 and at N = M = 2048; and ragged at N = M = 1024 with counts 512 ... 1024
                (the new path only: the torch formulation has no counts)
  baseline      dcp/model.py:27-34, 232-245 restated below in torch on the projections: three view().transpose(1, 2).contiguous(),
                matmul, division, softmax, matmul, transpose(1, 2).contiguous().view() -- the four copies the node absorbs
                included --, forward, and forward + autograd backward of sum(out g)
  sdpa          torch.nn.functional.scaled_dot_product_attention on the same head-major copies, where this torch build runs it
                on the device: an additional row, not the reference's formulation
  per call      us per call through Python: device events around a window of --steps calls, the paths' windows interleaved,
                median of --rounds windows with min ... max
  device        the C entries called directly on buffers allocated once (rrl_attention_fwd; rrl_attention_fwd + rrl_attention_bwd)
  memory        torch.cuda.max_memory_allocated over one forward + backward of either path, above what the inputs occupy
  accuracy      max |out - float64| of both paths against the same formulation in float64 on the GPU, and their ratio
  matrix peak   the flop of the matrix-core products a kernel issues (forward 3, row pass 3, column pass 4 products of
                2 B H DK N M) over its device time, as a share of --peak-tflops (157.3: the f32 matrix peak)
  transformer   one callsites.dcp_transformer call (emb_dims 512, 4 heads, ff_dims 1024, 1 block: DCP's defaults) against the same
                module with the torch formulation in the place of the node, forward and forward + backward

Writes --out (default profiles/attention_timing.json) and prints it.  With --parent DIR (a checkout of the parent commit with its
library built): `python bench.py` in this tree and in DIR, alternating, --bench-rounds times each -- once with this tree first in
every pair and once with the parent first, since the second process of a pair meets a warmer device."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "a-robust-registration-loss_amd"))

B, H, DK = 8, 4, 128


def torch_attend(q, k, v, n_heads, *_):
    """The reference's formulation, eager torch, on token-major projections."""
    import torch
    nb, d_k = q.size(0), q.size(2) // n_heads
    qh, kh, vh = (x.view(nb, -1, n_heads, d_k).transpose(1, 2).contiguous() for x in (q, k, v))
    scores = torch.matmul(qh, kh.transpose(-2, -1).contiguous()) / math.sqrt(d_k)
    x = torch.matmul(torch.softmax(scores, dim=-1), vh)
    return x.transpose(1, 2).contiguous().view(nb, -1, n_heads * d_k)


def sdpa_attend(q, k, v, n_heads):
    import torch
    nb, d_k = q.size(0), q.size(2) // n_heads
    qh, kh, vh = (x.view(nb, -1, n_heads, d_k).transpose(1, 2).contiguous() for x in (q, k, v))
    x = torch.nn.functional.scaled_dot_product_attention(qh, kh, vh)
    return x.transpose(1, 2).contiguous().view(nb, -1, n_heads * d_k)


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
    import gc
    import torch
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return int(peak)


def inputs(N, requires_grad=False):
    import torch
    gen = torch.Generator().manual_seed(N)
    ts = [torch.randn(B, N, H * DK, generator=gen).cuda() for _ in range(4)]
    return [t.requires_grad_(True) for t in ts[:3]] + ts[3:] if requires_grad else ts


def rows(a):
    import torch
    from rrl_hip import _lib, attention, ops
    lib = _lib.load()
    out = []
    for N, counts in ((1024, None), (2048, None), (1024, [512, 585, 658, 731, 804, 877, 950, 1024])):
        q, k, v, g = inputs(N)
        qg, kg, vg = (t.clone().requires_grad_(True) for t in (q, k, v))
        cnt = torch.tensor(counts, dtype=torch.int32).cuda() if counts else None

        def fwd(fn, *extra):
            def call():
                with torch.no_grad():
                    return fn(q, k, v, H, *extra)
            return call

        def both(fn, *extra):
            return lambda: torch.autograd.grad((fn(qg, kg, vg, H, *extra) * g).sum(), (qg, kg, vg))
        ws_bytes = int(lib.rrl_attention_workspace_bytes(B, H, N, N))
        row = {"B": B, "H": H, "DK": DK, "N": N, "M": N, "counts": counts, "launches_forward": 1, "launches_backward": 2,
               "workspace_bytes": ws_bytes, "score_matrix_bytes": B * H * N * N * 4}
        fns = {"forward": fwd(attention.attend, cnt, cnt), "forward_backward": both(attention.attend, cnt, cnt)}
        if counts is None:
            want = torch_attend(q.double(), k.double(), v.double(), H)
            mine, theirs = (float((f().double() - want).abs().max()) for f in (fns["forward"], fwd(torch_attend)))
            row["error_vs_float64"] = {"attention": mine, "torch_float32": theirs, "ratio": mine / theirs if theirs else None}
            del want
            fns.update(torch_forward=fwd(torch_attend), torch_forward_backward=both(torch_attend))
            try:
                fwd(sdpa_attend)()
                both(sdpa_attend)()
                fns.update(sdpa_forward=fwd(sdpa_attend), sdpa_forward_backward=both(sdpa_attend))
            except Exception as e:  # this torch build does not run it on the device
                row["sdpa"] = "not run: " + type(e).__name__
        for name, r in zip(fns, interleaved(list(fns.values()), a.steps, a.warmup, a.rounds)):
            row[name] = r
        ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=q.device)
        o = torch.empty_like(q)
        d = [torch.empty_like(t) for t in (q, k, v)]
        P = ops._p
        head = (P(q), P(k), P(v), P(cnt), P(cnt), P(ws), ws_bytes)

        def dev_fwd():
            ops._run(q.device, "rrl_attention_fwd", *head, P(o), None, B, H, DK, N, N)

        def dev_row():
            ops._run(q.device, "rrl_attention_bwd", *head, P(o), P(g), P(d[0]), None, None, B, H, DK, N, N)

        def dev_col():
            ops._run(q.device, "rrl_attention_bwd", *head, P(o), P(g), None, P(d[1]), P(d[2]), B, H, DK, N, N)

        def dev_both():
            dev_fwd()
            ops._run(q.device, "rrl_attention_bwd", *head, P(o), P(g), P(d[0]), P(d[1]), P(d[2]), B, H, DK, N, N)
        names = ("device_forward", "device_backward_rows", "device_backward_columns", "device_forward_backward")
        for name, r in zip(names, interleaved([dev_fwd, dev_row, dev_col, dev_both], a.steps, a.warmup, a.rounds)):
            row[name] = r
        if counts is None:
            row["speedup_forward"] = row["torch_forward"]["median_us"] / row["forward"]["median_us"]
            row["speedup_forward_backward"] = row["torch_forward_backward"]["median_us"] / row["forward_backward"]["median_us"]
            product = 2.0 * B * H * DK * N * N
            row["share_of_f32_matrix_peak"] = {name: n * product / (row[key]["median_us"] * 1e-6) / (a.peak_tflops * 1e12) for name, key, n in
                                               (("forward", "device_forward", 3), ("backward_rows", "device_backward_rows", 3),
                                                ("backward_columns", "device_backward_columns", 4))}
            row["peak_bytes_forward_backward"] = {"attention": peak_bytes(fns["forward_backward"]), "torch": peak_bytes(fns["torch_forward_backward"])}
        out.append(row)
    return out


def transformer_row(a, N=1024):
    """DCP's default pointer on (B, 512, N) embeddings: the module with the node, and with the torch formulation in its place."""
    import torch
    from rrl_hip import attention, callsites
    torch.manual_seed(0)
    module = attention.Transformer(H * DK, H, 1024, 1).cuda()
    gen = torch.Generator().manual_seed(1)
    src, tgt = (torch.randn(B, H * DK, N, generator=gen).cuda().requires_grad_(True) for _ in range(2))
    node = attention.attend

    def run(attend, grad):
        def call():
            attention.attend = attend
            try:
                if not grad:
                    with torch.no_grad():
                        return callsites.dcp_transformer(module, src, tgt)
                s, t = callsites.dcp_transformer(module, src, tgt)
                return torch.autograd.grad(s.sum() + t.sum(), (src, tgt))
            finally:
                attention.attend = node
        return call
    fns = {"forward": run(node, False), "torch_forward": run(torch_attend, False), "forward_backward": run(node, True),
           "torch_forward_backward": run(torch_attend, True)}
    row = {"emb_dims": H * DK, "n_heads": H, "ff_dims": 1024, "n_blocks": 1, "B": B, "N": N, "M": N}
    a32, b32 = fns["forward"](), fns["torch_forward"]()
    row["max_difference_between_the_paths"] = float(max((x - y).abs().max() for x, y in zip(a32, b32)))
    for name, r in zip(fns, interleaved(list(fns.values()), max(a.steps // 4, 2), a.warmup, a.rounds)):
        row[name] = r
    row["speedup_forward"] = row["torch_forward"]["median_us"] / row["forward"]["median_us"]
    row["speedup_forward_backward"] = row["torch_forward_backward"]["median_us"] / row["forward_backward"]["median_us"]
    row["peak_bytes_forward_backward"] = {"attention": peak_bytes(fns["forward_backward"]), "torch": peak_bytes(fns["torch_forward_backward"])}
    return row


def kernel_trace_workload(calls, N=1024):
    import torch
    from rrl_hip import _lib, ops
    q, k, v, g = inputs(N)
    ws_bytes = int(_lib.load().rrl_attention_workspace_bytes(B, H, N, N))
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=q.device)
    o, d = torch.empty_like(q), [torch.empty_like(t) for t in (q, k, v)]
    P = ops._p
    head = (P(q), P(k), P(v), None, None, P(ws), ws_bytes)
    for _ in range(calls):
        ops._run(q.device, "rrl_attention_fwd", *head, P(o), None, B, H, DK, N, N)
        ops._run(q.device, "rrl_attention_bwd", *head, P(o), P(g), P(d[0]), P(d[1]), P(d[2]), B, H, DK, N, N)
    torch.cuda.synchronize()


def bench_series(parent, rounds, parent_first=False):
    def one(cwd):
        res = subprocess.run([sys.executable, "bench.py"], cwd=cwd, capture_output=True, text=True, check=True).stdout
        return json.loads(res.strip().splitlines()[-1])["value"]
    mine, theirs = [], []
    for _ in range(rounds):
        if parent_first:
            theirs.append(one(parent))
        mine.append(one(ROOT))
        if not parent_first:
            theirs.append(one(parent))
    return {"command": "python bench.py", "rounds": rounds, "first_of_each_pair": "parent" if parent_first else "this tree",
            "this_tree": mine, "parent_library": theirs,
            "this_tree_median": statistics.median(mine), "parent_min": min(theirs), "parent_max": max(theirs),
            "inside_parent_spread": min(theirs) <= statistics.median(mine) <= max(theirs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--peak-tflops", type=float, default=157.3)
    ap.add_argument("--parent", help="checkout of the parent commit with its library built")
    ap.add_argument("--bench-rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attention_timing.json"))
    ap.add_argument("--calls", type=int, default=0, help="only issue this many forward + backward calls at N = M = 1024 through "
                    "the C entries and exit: the workload for `rocprofv3 --kernel-trace --stats`")
    a = ap.parse_args()
    import torch
    if a.calls:
        return kernel_trace_workload(a.calls)
    doc = {"what": "attention node against the reference's formulation in eager torch on one MI355X: device events around "
                   "windows of %d calls, the paths' windows interleaved, median of %d windows" % (a.steps, a.rounds),
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "attention": rows(a), "transformer": transformer_row(a)}
    torch.cuda.synchronize()
    if a.parent:
        doc["bench"] = bench_series(os.path.abspath(a.parent), a.bench_rounds)
        doc["bench_parent_first"] = bench_series(os.path.abspath(a.parent), a.bench_rounds, parent_first=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
