#!/usr/bin/env python3
"""Generate tests/golden/pointnet.npz and tests/golden/pointnet_grads.npz (two files: a committed file stays below 1 MiB) -- FMR's
feature extractor on a few small clouds -- by RUNNING THE REFERENCE's PointNet
(fmr/model.py:105-126) on the CPU at random initialisation, in float32 and, on float64 copies of the same weights, in float64,
with the helpers of make_golden.py and make_golden_fmr_ic.py (same stubs, same reference checkout).

Run in the build container only (needs the reference checkout, see make_golden.py):

    python tests/golden/make_golden_pointnet.py

Clouds: fmr_refs.ellipsoid_cloud (semi-axes 1 / 0.6 / 0.3, zero-meaned).  Per case NAME = b<B>_n<N>_k<K>:
    NAME_p (B, N, 3) float32, NAME_w_<key> the state_dict, NAME_f32 (B, K) and NAME_f64 (B, K) the features of the two runs,
    NAME_dist = max |f32 - f64|, NAME_arg (B, K) the index the float64 run pools (argmax over the points of its last activation),
    NAME_gap the smallest relative gap between the best and the second-best activation over the channels with f > 0.
For the first two cases pointnet_grads.npz holds, of the scalar sum(f * g) for a recorded g: NAME_g (B, K) float32, NAME_d32_<key>
and NAME_d64_<key> the parameter gradients of the float32 and the float64 run, NAME_d32_p and NAME_d64_p (B, N, 3) the input
gradients.
A draw of the first two cases is kept only when the float32 and the float64 run pool the same point for every channel with
f > 0 and that gap is >= 1e-3: there the pooled index is no near-tie, and a test may hold `arg` to the recording outright and no near-tie hides behind a gradient tolerance.  The
two larger cases carry no such condition (no draw among the first twenty meets both there).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402  (registers the stubs, names the reference checkout)
import make_golden_fmr_ic as MF  # noqa: E402

import torch  # noqa: E402

import fmr_refs as FR  # noqa: E402

# (B, N, K, drawn without near-ties)
CASES = ((2, 64, 32, True), (3, 33, 64, True), (2, 130, 64, False), (1, 257, 1024, False))
GAP_MIN = 1.0e-3


def pooled(net, p, dtype):
    """One run of the reference -> (features, the last activation (B, K, N))."""
    last = []
    hook = net.h2.register_forward_hook(lambda m, i, o: last.append(o))
    f = net(p.to(dtype))
    hook.remove()
    return f, last[0]


def main():
    ref = MF.reference_module()
    fwd, grads, names = {}, {}, []
    for ci, (B, N, K, strict) in enumerate(CASES):
        name = f"b{B}_n{N}_k{K}"
        names.append(name)
        for attempt in range(50):
            seed = 7000 + 100 * ci + attempt
            rng = np.random.default_rng(seed)
            torch.manual_seed(seed)
            p = torch.from_numpy(FR.ellipsoid_cloud(rng, B, N))
            g = torch.from_numpy(np.random.default_rng(seed + 50000).standard_normal((B, K)).astype(np.float32))
            net = ref.PointNet(dim_k=K).eval()
            state = {k: v.clone() for k, v in net.state_dict().items()}
            p32 = p.clone().requires_grad_(True)
            f32, h32 = pooled(net, p32, torch.float32)
            d32 = torch.autograd.grad((f32 * g).sum(), [p32] + list(net.parameters())) if strict else None
            net.double()
            p64 = p.double().requires_grad_(True)
            f64, h64 = pooled(net, p64, torch.float64)
            d64 = torch.autograd.grad((f64 * g.double()).sum(), [p64] + list(net.parameters())) if strict else None
            a32, a64 = h32.argmax(2), h64.argmax(2)
            top = h64.detach().topk(min(2, N), dim=2).values
            on = f64.detach() > 0
            gap = float(((top[..., 0] - top[..., -1]) / top[..., 0].clamp_min(1e-300))[on].min()) if on.any() else np.inf
            if not strict or (bool((a32 == a64)[on].all()) and gap >= GAP_MIN):
                break
        else:
            raise RuntimeError(f"{name}: no draw within the conditions")
        dist = float((f32.detach().double() - f64.detach()).abs().max())
        fwd.update({f"{name}_p": p.numpy(), f"{name}_f32": f32.detach().numpy(), f"{name}_f64": f64.detach().numpy(),
                    f"{name}_dist": np.array(dist), f"{name}_arg": a64.numpy().astype(np.int32), f"{name}_gap": np.array(gap)})
        fwd.update({f"{name}_w_{k}": v.numpy() for k, v in state.items()})
        if strict:
            keys = ["p"] + [k for k, _ in net.named_parameters()]
            grads[f"{name}_g"] = g.numpy()
            grads.update({f"{name}_d32_{k}": v.numpy() for k, v in zip(keys, d32)})
            grads.update({f"{name}_d64_{k}": v.numpy() for k, v in zip(keys, d64)})
        print(name, "attempt", attempt, "dist %.2e of max|f| %.2e" % (dist, float(f64.abs().max())), "gap %.2e" % gap)
    MG.save("pointnet.npz", cases=np.array(names), **fwd)
    MG.save("pointnet_grads.npz", cases=np.array(names[:2]), **grads)


if __name__ == "__main__":
    main()
