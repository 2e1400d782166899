"""Timing of the PointNet encoder (rrl_hip/pointnet.py, callsites.fmr_encoder) against the reference's
formulation as eager torch modules (Conv1d, GroupNorm, ReLU, max_pool1d) on the same GPU, in the same process, with the same
weights.

  encoder       clouds = 8 and 48 at N = 1024, K = 1024, forward and forward + backward to every parameter: us per call and
                torch.cuda.max_memory_allocated of either path
  ic_algo       a whole callsites.fmr_ic_algo at B = 8, N = K = 1024 with either encoder, maxiter 5 and 10: forward eager and captured,
                and forward + backward to the encoder's parameters
  per call      us per call through Python: device events around a window of --steps calls, the paths' windows interleaved,
                median of --rounds windows with min ... max (tools/fmr_head_timing.py's helpers)

Writes --out (default profiles/pointnet_timing.json) and prints it.  With --parent DIR (a checkout of the parent commit with its
library built): `python bench.py` in this tree and in DIR, alternating, --bench-rounds times each."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "a-robust-registration-loss_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fmr_head_timing as FH  # noqa: E402  (the restated reference, the interleaved windows, the bench series)

N, K = 1024, 1024
XTOL = 1.0e-7


def clouds(B, seed):
    import torch
    gen = torch.Generator().manual_seed(seed)
    v = torch.randn(B, N, 3, generator=gen)
    v = v / v.norm(dim=2, keepdim=True) * torch.tensor([1.0, 0.6, 0.3])
    return (v - v.mean(1, keepdim=True)).cuda()


def peak(fn):
    import torch
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    del out
    return torch.cuda.max_memory_allocated() - base


def rows(a):
    import torch
    from rrl_hip import callsites
    from rrl_hip.graph import GraphedStep
    PointNet, _, _, _, ref_ic_algo, ref_exp = FH.build_reference()
    torch.manual_seed(0)
    ref = PointNet(K).cuda()
    mine = callsites.fmr_encoder(K, state_dict={k: v.detach().cpu() for k, v in ref.state_dict().items()})
    params, my_params = list(ref.parameters()), list(mine.parameters())
    out = {"encoder": [], "ic_algo": []}
    for B in (8, 48):
        p = clouds(B, B)

        def lib_fwd():
            with torch.no_grad():
                return mine(p)

        def torch_fwd():
            with torch.no_grad():
                return ref(p)

        def torch_both():
            return torch.autograd.grad(ref(p).sum(), params)

        def lib_both():
            return torch.autograd.grad(mine(p).sum(), my_params)
        with torch.no_grad():
            gap = float((mine(p) - ref(p)).abs().max())
        row = {"clouds": B, "N": N, "K": K, "max_abs_difference_of_the_features": gap}
        names = ["encoder_forward", "torch_encoder_forward", "encoder_forward_backward", "torch_encoder_forward_backward"]
        fns = [lib_fwd, torch_fwd, lib_both, torch_both]
        row["max_abs_difference_of_the_gradients"] = max(float((a - b).abs().max()) for a, b in zip(lib_both(), torch_both()))
        row["max_abs_gradient"] = max(float(b.abs().max()) for b in torch_both())
        for name, r in zip(names, FH.interleaved(fns, a.steps, a.warmup, a.rounds)):
            row[name] = r
        row["speedup_forward"] = row["torch_encoder_forward"]["median_us"] / row["encoder_forward"]["median_us"]
        row["speedup_forward_backward"] = row["torch_encoder_forward_backward"]["median_us"] / row["encoder_forward_backward"]["median_us"]
        row["peak_bytes"] = {n: peak(f) for n, f in zip(names, fns)}
        row["launches"] = {n: FH.launches(f) for n, f in zip(names[:2], fns[:2])}
        out["encoder"].append(row)
    B = 8
    p0 = clouds(B, 1)
    gen = torch.Generator().manual_seed(2)
    twist = torch.randn(B, 6, generator=gen) * torch.tensor([0.05] * 3 + [0.02] * 3)
    R = ref_exp(twist)
    p1 = (p0 @ R[:, :3, :3].transpose(1, 2).cuda() + R[:, None, :3, 3].cuda()).contiguous()
    dt = torch.full((B, 6), 1.0e-2).cuda()
    for maxiter in (5, 10):
        def algo(enc):
            def run():
                with torch.no_grad():
                    return callsites.fmr_ic_algo(enc, p0, p1, maxiter=maxiter, xtol=XTOL, dt=dt)[2]
            return run

        def all_torch():
            with torch.no_grad():
                return ref_ic_algo(ref, p0, p1, dt, maxiter, XTOL)[1]
        row = {"B": B, "N": N, "K": K, "maxiter": maxiter}

        def both(enc, prm):
            def run():
                r, _, series, _, _ = callsites.fmr_ic_algo(enc, p0, p1, maxiter=maxiter, xtol=XTOL, dt=dt)
                return torch.autograd.grad(series.sum() + r.sum(), prm)
            return run
        names = ["ic_algo_library_encoder", "ic_algo_torch_encoder", "torch_ic_algo", "ic_algo_forward_backward_library_encoder",
                 "ic_algo_forward_backward_torch_encoder"]
        fns = [algo(mine), algo(ref), all_torch, both(mine, my_params), both(ref, params)]
        for name, r in zip(names, FH.interleaved(fns, a.steps, a.warmup, a.rounds)):
            row[name] = r
        row["pose_difference_between_the_encoders"] = float((fns[0]() - fns[1]()).abs().max())
        for name, enc in (("library_encoder", mine), ("torch_encoder", ref)):
            try:
                eager = algo(enc)().clone()
                step = GraphedStep(algo(enc))
                same = bool(torch.equal(step(), eager))
                row["graph_" + name] = {"replays": True, "same_bits_as_eager": same, **FH.interleaved([step], a.steps, a.warmup, a.rounds)[0]}
            except Exception as e:  # noqa: BLE001
                row["graph_" + name] = {"replays": False, "error": repr(e)[:200]}
        out["ic_algo"].append(row)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent", help="checkout of the parent commit with its library built")
    ap.add_argument("--bench-rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pointnet_timing.json"))
    a = ap.parse_args()
    import torch
    doc = {"what": "the PointNet encoder against the reference's formulation as eager torch modules on one MI355X: device "
                   "events around windows of %d calls, the paths' windows interleaved, median of %d windows" % (a.steps, a.rounds),
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, **rows(a)}
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
