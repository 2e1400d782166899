"""Timing of FMR's inverse-compositional head (rrl_hip/fmr.py, callsites.fmr_ic_algo) against the
reference's formulation restated in eager torch on the same GPU, in the same process.

  shapes        B = 8, N = 1024, K = 1024; maxiter 5 (the trainer) and 10 (the evaluation)
  baseline      fmr/model.py:318-439 with se_math's exp / ExpMap / InvMatrix restated below in torch: the Python loop over the
                batch in approx_Jac and InvMatrix, and the `float(check) < xtol` read-back of every iteration, as the reference has them
  (a) head      perturb + pinv + maxiter updates on fixed features (no encoder): forward, and forward + backward
  (b) whole     one ic_algo around the reference's PointNet, forward and forward + backward to the encoder's parameters, and
                the head's share of it ((a) over (b), either path)
  launches      device kernels per call of each path (torch.profiler; None where the profiler is not available)
  graph         whether the captured callsites.fmr_ic_algo replays with the bits of the eager call, and its time per replay
  per call      us per call through Python: device events around a window of --steps calls, the paths' windows interleaved,
                median of --rounds windows with min ... max

Writes --out (default profiles/fmr_head_timing.json) and prints it.  With --parent DIR (a checkout of the parent commit with its
library built): `python bench.py` in this tree and in DIR, alternating, --bench-rounds times each."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "a-robust-registration-loss_amd"))

B, N, K = 8, 1024, 1024
XTOL = 1.0e-7


def build_reference():
    """The reference's pieces in torch (restated; nothing is imported from it)."""
    import torch

    def mlp(widths):
        layers = []
        for a, b in zip(widths[:-1], widths[1:]):
            layers += [torch.nn.Conv1d(a, b, 1), torch.nn.GroupNorm(8, b), torch.nn.ReLU()]
        return torch.nn.Sequential(*layers)

    class PointNet(torch.nn.Module):  # fmr/model.py:57-126
        def __init__(self, dim_k):
            super().__init__()
            self.h1, self.h2 = mlp([3, 64, 64]), mlp([64, 64, 128, dim_k])

        def forward(self, points):
            x = self.h2(self.h1(points.transpose(1, 2)))
            return torch.nn.functional.max_pool1d(x, x.size(-1)).flatten(1)

    gen = torch.zeros(6, 4, 4)
    for k in range(3):
        a, b = (k + 1) % 3, (k + 2) % 3
        gen[k, b, a], gen[k, a, b], gen[3 + k, k, 3] = 1.0, -1.0, 1.0

    def exp(x):  # se_math/se3.py:57-80 with sinc.py's branches
        w, v = x[:, :3], x[:, 3:]
        t = w.norm(dim=1).view(-1, 1, 1)
        O = torch.zeros_like(w[:, 0])
        W = torch.stack((torch.stack((O, -w[:, 2], w[:, 1]), 1), torch.stack((w[:, 2], O, -w[:, 0]), 1), torch.stack((-w[:, 1], w[:, 0], O), 1)), 1)
        S = W.bmm(W)
        small = t.abs() < 0.01
        ts = torch.where(small, torch.ones_like(t), t)
        t2 = t * t
        s1 = torch.where(small, 1 - t2 / 6 * (1 - t2 / 20 * (1 - t2 / 42)), torch.sin(ts) / ts)
        s2 = torch.where(small, 0.5 * (1 - t2 / 12 * (1 - t2 / 30 * (1 - t2 / 56))), (1 - torch.cos(ts)) / (ts * ts))
        s3 = torch.where(small, 1 / 6 * (1 - t2 / 20 * (1 - t2 / 42 * (1 - t2 / 72))), (ts - torch.sin(ts)) / (ts ** 3))
        eye = torch.eye(3).to(x)
        R = eye + s1 * W + s2 * S
        p = (eye + s2 * W + s3 * S).bmm(v.reshape(-1, 3, 1))
        bottom = torch.tensor([0.0, 0.0, 0.0, 1.0]).to(x).view(1, 1, 4).repeat(x.shape[0], 1, 1)
        return torch.cat((torch.cat((R, p), 2), bottom), 1)

    class Exp(torch.autograd.Function):  # se_math/se3.py:133-165
        @staticmethod
        def forward(ctx, x):
            ctx.save_for_backward(x)
            return exp(x)

        @staticmethod
        def backward(ctx, go):
            x, = ctx.saved_tensors
            return (go[:, None] * (gen.to(x)[None] @ exp(x)[:, None])).sum((-1, -2))

    class Inv(torch.autograd.Function):  # se_math/invmat.py:6-13, 83-112
        @staticmethod
        def forward(ctx, x):
            y = torch.zeros_like(x)
            for i in range(x.shape[0]):
                y[i] = x[i].inverse()
            ctx.save_for_backward(y)
            return y

        @staticmethod
        def backward(ctx, go):
            y, = ctx.saved_tensors
            return -(y.transpose(1, 2) @ go @ y.transpose(1, 2))

    def perturb(p0, dt):  # approx_Jac's loop over the batch (fmr/model.py:416-424)
        transf = torch.zeros(p0.shape[0], 6, 4, 4).to(p0)
        for b in range(p0.shape[0]):
            transf[b] = Exp.apply(-torch.diag(dt[b]))
        transf = transf.unsqueeze(2).contiguous()
        return (transf[..., :3, :3] @ p0[:, None, :, :, None]).squeeze(-1) + transf[..., :3, 3]

    def pinv_of(f0, fp, dt):
        J = (f0.unsqueeze(-1) - fp.transpose(1, 2)) / dt.unsqueeze(1)
        Jt = J.transpose(1, 2)
        return Inv.apply(Jt.bmm(J)).bmm(Jt)

    def update(pinv, f0, f1, g, xtol):
        r = f1 - f0
        dx = -pinv.bmm(r.unsqueeze(-1)).view(-1, 6)
        if float(dx.norm(p=2, dim=1, keepdim=True).max()) < xtol:
            return r, None
        return r, Exp.apply(dx).matmul(g)

    def ic_algo(enc, p0, p1, dt, maxiter, xtol):
        f0 = enc(p0)
        fp = enc(perturb(p0, dt).view(-1, p0.shape[1], 3)).view(p0.shape[0], 6, -1)
        pinv = pinv_of(f0, fp, dt)
        g = torch.eye(4).to(p0).expand(p0.shape[0], 4, 4).contiguous()
        series, r = [], None
        for _ in range(maxiter):
            p = (g[:, None, :3, :3] @ p1[..., None]).squeeze(-1) + g[:, None, :3, 3]
            r, g_new = update(pinv, f0, enc(p), g, xtol)
            if g_new is None:
                break
            g = g_new
            series.append(g)
        return r, g, series
    return PointNet, perturb, pinv_of, update, ic_algo, exp


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


def launches(fn):
    """Device kernels of one call of fn; without a working profiler the exception's text (a report, never a silent None)."""
    import torch
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if getattr(e, "device_type", None) is not None and "cuda" in str(e.device_type).lower()
                and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
        return n if n else "profiler reported no device kernel"
    except Exception as e:  # noqa: BLE001  (the count is a report, not a check: the text says why it is missing)
        return "profiler failed: " + repr(e)[:200]


def rows(a):
    import torch
    from rrl_hip import callsites, fmr
    from rrl_hip.graph import GraphedStep
    PointNet, ref_perturb, ref_pinv, ref_update, ref_ic_algo, ref_exp = build_reference()
    out = []
    gen = torch.Generator().manual_seed(1)
    v = torch.randn(B, N, 3, generator=gen)
    v = v / v.norm(dim=2, keepdim=True) * torch.tensor([1.0, 0.6, 0.3])
    p0 = (v - v.mean(1, keepdim=True)).cuda()
    twist = torch.randn(B, 6, generator=gen) * torch.tensor([0.05] * 3 + [0.02] * 3)
    torch.manual_seed(0)
    net = PointNet(K).cuda()
    dt = torch.full((B, 6), 1.0e-2).cuda()
    f0 = torch.randn(B, K, generator=gen).cuda()
    fp = (f0[:, None, :] - 1.0e-2 * torch.randn(B, 6, K, generator=gen).cuda()).contiguous()
    for maxiter in (5, 10):
        f1s = [(f0 + 0.05 * torch.randn(B, K, generator=gen).cuda()) for _ in range(maxiter)]
        leaves = [t.clone().requires_grad_(True) for t in (f0, fp, dt)]
        g0 = torch.eye(4).expand(B, 4, 4).contiguous().cuda()

        def new_head(a0=f0, ap=fp, ad=dt):
            pert = fmr.ic_perturb(p0, ad)
            pinv = fmr.ic_pinv(a0, ap, ad)
            g, stop, r = g0, fmr.new_stop(p0.device), None
            for f1 in f1s:
                r, _, g, stop = fmr.ic_update(pinv, a0, f1, g, stop, XTOL)
            return pert, r, g

        def ref_head(a0=f0, ap=fp, ad=dt):
            pert = ref_perturb(p0, ad)
            pinv = ref_pinv(a0, ap, ad)
            g, r = g0, None
            for f1 in f1s:
                r, g_new = ref_update(pinv, a0, f1, g, XTOL)
                if g_new is None:
                    break
                g = g_new
            return pert, r, g

        def both(head):
            def run():
                pert, r, g = head(*leaves)
                return torch.autograd.grad(pert.sum() + r.sum() + g.sum(), leaves)
            return run

        def fwd(head):
            def run():
                with torch.no_grad():
                    return head()
            return run
        row = {"B": B, "N": N, "K": K, "maxiter": maxiter}
        fns = [fwd(new_head), fwd(ref_head), both(new_head), both(ref_head)]
        names = ["head_forward", "torch_head_forward", "head_forward_backward", "torch_head_forward_backward"]
        for name, r in zip(names, interleaved(fns, a.steps, a.warmup, a.rounds)):
            row[name] = r
        row["launches"] = {n: launches(f) for n, f in zip(names, fns)}
        # (b) the whole call around the encoder
        R = ref_exp(twist)
        p1 = (p0 @ R[:, :3, :3].transpose(1, 2).cuda() + R[:, None, :3, 3].cuda()).contiguous()
        params = list(net.parameters())

        def new_algo():
            r, g, series, _, _ = callsites.fmr_ic_algo(net, p0, p1, maxiter=maxiter, xtol=XTOL, dt=dt)
            return r, g, series

        def ref_algo():
            r, g, series = ref_ic_algo(net, p0, p1, dt, maxiter, XTOL)
            return r, g, torch.stack(series)

        def both_algo(algo):
            def run():
                r, g, series = algo()
                return torch.autograd.grad(series.sum() + r.sum(), params)
            return run

        def fwd_algo(algo):
            def run():
                with torch.no_grad():
                    return algo()
            return run
        fns = [fwd_algo(new_algo), fwd_algo(ref_algo), both_algo(new_algo), both_algo(ref_algo)]
        names = ["ic_algo_forward", "torch_ic_algo_forward", "ic_algo_forward_backward", "torch_ic_algo_forward_backward"]
        for name, r in zip(names, interleaved(fns, a.steps, a.warmup, a.rounds)):
            row[name] = r
        row["launches"].update({n: launches(f) for n, f in zip(names, fns)})
        for mode in ("forward", "forward_backward"):
            row["head_share_" + mode] = {"library": row["head_" + mode]["median_us"] / row["ic_algo_" + mode]["median_us"],
                                         "torch": row["torch_head_" + mode]["median_us"] / row["torch_ic_algo_" + mode]["median_us"]}
            row["speedup_head_" + mode] = row["torch_head_" + mode]["median_us"] / row["head_" + mode]["median_us"]
            row["speedup_ic_algo_" + mode] = row["torch_ic_algo_" + mode]["median_us"] / row["ic_algo_" + mode]["median_us"]
        # the captured loop
        try:
            with torch.no_grad():
                eager = new_algo()[2].clone()
                step = GraphedStep(lambda: new_algo()[2])
                same = bool(torch.equal(step(), eager))
                row["graph"] = {"replays": True, "same_bits_as_eager": same, **interleaved([step], a.steps, a.warmup, a.rounds)[0]}
        except Exception as e:  # noqa: BLE001
            row["graph"] = {"replays": False, "error": repr(e)[:200]}
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
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent", help="checkout of the parent commit with its library built")
    ap.add_argument("--bench-rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fmr_head_timing.json"))
    a = ap.parse_args()
    import torch
    doc = {"what": "FMR's inverse-compositional head against the reference's formulation in eager torch on one MI355X: device "
                   "events around windows of %d calls, the paths' windows interleaved, median of %d windows" % (a.steps, a.rounds),
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "rows": rows(a)}
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
