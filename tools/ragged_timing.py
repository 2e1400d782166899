"""Ragged batches against the alternatives a caller with mixed sizes has WITHOUT them (DESIGN.md "Ragged batches").

One step = rigid apply + loss + backward to points1.grad (ops.LossStep, one C call) of a B = 8 batch with capacities
4096 / 4096 / 10000 and per-sample counts spread evenly between a quarter of the capacity and the capacity:

  ragged        this tree, counts1 / counts2 / nlines (cold and prepared builds)
  ragged_full   this tree, counts equal to the capacities (what reading the counts costs)
  uniform       this tree, no counts, all rows (for reference)
  loop8         the PARENT commit's library: eight B = 1 steps on the exact sizes -- the only correct alternative there
  uniform_parent  the PARENT commit's library: the uniform step at the capacities (the ragged step does a subset of its work)

The parent's numbers come from a CHILD process that imports the package of a checkout of the parent commit (--parent DIR:
`git worktree add DIR HEAD~1`, then build its library there) -- two builds of one library cannot live in one process.
Rounds alternate between the two processes in one session; every timed window ends in a device synchronisation.  Writes
--out (default profiles/ragged_timing.json) and prints it.  Kernel averages: run this file's --steps-only mode under
`rocprofv3 --kernel-trace --stats` (tools/kt.sh) in a run of its own."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

B, CAP, LCAP = 8, 4096, 10000
COUNTS = [CAP // 4 + (CAP - CAP // 4) * b // (B - 1) for b in range(B)]      # 1024 .. 4096
NLINES = [LCAP // 4 + (LCAP - LCAP // 4) * b // (B - 1) for b in range(B)]   # 2500 .. 10000


def workload(pkg_root):
    """(src, tar, lines, R, t) at the capacities, seeded: the same tensors in both processes."""
    sys.path.insert(0, os.path.join(pkg_root, "a-robust-registration-loss_amd"))
    import numpy as np
    import torch
    import loss as LS
    from LieAlgebra import se3
    from rrl_hip import synth
    prs = [synth.make_pair(1000 + b, CAP, CAP) for b in range(B)]
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    src, tar = cu(np.stack([p["src_tri"] for p in prs])), cu(np.stack([p["tar_tri"] for p in prs]))
    lines = []
    for b, p in enumerate(prs):
        torch.manual_seed(50 + b)
        lines.append(LS.Random_uniform_distribution_lines_batch_efficient_resample(
            torch.tensor([[float(p["radius"])]]), torch.from_numpy(p["center"]).reshape(1, 3), LCAP, cu(p["src"])[None],
            cu(p["tar"])[None], "cuda")[0])
    R, t = (x.cuda().contiguous() for x in se3.exp3(0.03 * torch.randn(B, 6, generator=torch.Generator().manual_seed(3))))
    return src, tar, torch.stack(lines).contiguous(), R, t


def timed(fn, steps):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / steps


def parent_variants(root):
    src, tar, ln, R, t = workload(root)
    from rrl_hip import ops
    out = {}
    for prepared in (False, True):
        tag = "prepared" if prepared else "cold"
        uni = ops.LossStep(src, tar, LCAP, prepared=prepared)
        out["uniform_parent_" + tag] = lambda uni=uni: uni(R, t, ln)
        ones = []
        for b in range(B):  # the exact sizes, contiguous tensors of their own
            s1, s2, l1 = src[b:b + 1, :COUNTS[b]].contiguous(), tar[b:b + 1, :COUNTS[b]].contiguous(), ln[b:b + 1, :NLINES[b]].contiguous()
            ones.append((ops.LossStep(s1, s2, NLINES[b], prepared=prepared), R[b:b + 1].contiguous(), t[b:b + 1].contiguous(), l1))

        def loop8(ones=ones):
            for st, Rb, tb, lb in ones:
                st(Rb, tb, lb)
        out["loop8_" + tag] = loop8
    return out


def own_variants():
    src, tar, ln, R, t = workload(ROOT)
    import torch
    from rrl_hip import ops
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")  # noqa: E731
    out, keep = {}, {}
    for prepared in (False, True):
        tag = "prepared" if prepared else "cold"
        rag = ops.LossStep(src, tar, LCAP, prepared=prepared, counts1=i32(COUNTS), counts2=i32(COUNTS), nlines=i32(NLINES))
        full = ops.LossStep(src, tar, LCAP, prepared=prepared, counts1=i32([CAP] * B), counts2=i32([CAP] * B), nlines=i32([LCAP] * B))
        uni = ops.LossStep(src, tar, LCAP, prepared=prepared)
        out["ragged_" + tag] = lambda s=rag: s(R, t, ln)
        out["ragged_full_" + tag] = lambda s=full: s(R, t, ln)
        out["uniform_" + tag] = lambda s=uni: s(R, t, ln)
        keep[tag] = (rag, full, uni)
    return out, keep, (src, tar, ln, R, t)


def child(root, steps, warmup):
    """Serve rounds over stdin / stdout: 'round' -> one JSON line of us per step for every parent variant; 'quit'."""
    v = parent_variants(root)
    for fn in v.values():
        timed(fn, warmup)
    print(json.dumps({"ready": sorted(v)}), flush=True)
    for line in sys.stdin:
        if line.strip() != "round":
            break
        print(json.dumps({k: timed(fn, steps) for k, fn in v.items()}), flush=True)


def read_json(proc):
    """The child's next JSON line (anything else it prints is passed on)."""
    while True:
        line = proc.stdout.readline()
        if not line:
            raise RuntimeError("the parent-library child process ended early")
        if line.startswith("{"):
            return json.loads(line)
        sys.stderr.write(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="checkout of the parent commit with its library built")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--steps-only", metavar="VARIANT", help="run only this variant's steps (kernel traces)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_timing.json"))
    a = ap.parse_args()
    if a.child:
        return child(a.parent, a.steps, a.warmup)
    import torch
    own, keep, data = own_variants()
    if a.steps_only:
        timed(own[a.steps_only], a.warmup)
        print(a.steps_only, round(timed(own[a.steps_only], a.steps), 2), "us per step")
        return
    for fn in own.values():
        timed(fn, a.warmup)
    # what the ragged step computes: bit-identical per sample to the uniform step where the counts are the capacities
    rag, full, uni = keep["prepared"]
    same_full = torch.equal(full.st.loss, uni.st.loss) and torch.equal(full.st.info, uni.st.info)
    res = {k: [] for k in own}
    proc = None
    if a.parent:
        proc = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", "--parent", os.path.abspath(a.parent),
                                 "--steps", str(a.steps), "--warmup", str(a.warmup)], stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                                text=True, cwd=os.path.abspath(a.parent))
        ready = read_json(proc)
        res.update({k: [] for k in ready["ready"]})
    for _ in range(a.rounds):  # alternate: this process, then the parent's
        for k, fn in own.items():
            res[k].append(timed(fn, a.steps))
        if proc:
            proc.stdin.write("round\n")
            proc.stdin.flush()
            for k, v in read_json(proc).items():
                res[k].append(v)
    if proc:
        proc.stdin.write("quit\n")
        proc.stdin.close()
        proc.wait(timeout=60)
    rows = {k: {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2), "n": len(v)}
            for k, v in res.items()}
    doc = {"what": "us per LossStep (rigid apply + loss + backward to points1.grad), B = 8, capacities 4096 / 4096 / 10000, one MI355X; "
                   "rounds alternate between this tree and a child process on the parent commit's library",
           "device": torch.cuda.get_device_name(0), "counts": COUNTS, "nlines": NLINES, "rounds": a.rounds, "steps_per_round": a.steps,
           "full_counts_equal_uniform_bits": bool(same_full), "us_per_step": rows}
    if proc:
        med = lambda k: rows[k]["median_us"]  # noqa: E731
        doc["ratios"] = {f"loop8_over_ragged_{g}": round(med(f"loop8_{g}") / med(f"ragged_{g}"), 2) for g in ("cold", "prepared")}
        doc["ratios"].update({f"ragged_over_uniform_parent_{g}": round(med(f"ragged_{g}") / med(f"uniform_parent_{g}"), 3) for g in ("cold", "prepared")})
        doc["ratios"].update({f"ragged_full_over_uniform_parent_{g}": round(med(f"ragged_full_{g}") / med(f"uniform_parent_{g}"), 3) for g in ("cold", "prepared")})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
