#!/usr/bin/env python3
"""Generate tests/golden/pointnet_group.npz and tests/golden/pointnet_group_grads.npz -- RPM's per-point neighbourhood features --
by RUNNING THE REFERENCE's get_prepool stack (rpm/models/feature_nets.py:118-131) followed by torch.max(., 2)[0] (:199) on the
CPU at random initialisation, in float32 and, on float64 copies of the same weights, in float64, with the helpers and stubs of
make_golden.py, like make_golden_pointnet.py.

Run in the build container only (needs the reference checkout, see make_golden.py):

    python tests/golden/make_golden_pointnet_group.py

pointnet_group.npz, the forward-only case `rpm130`: the input is NOT stored, it is the recorded raw features of
ball_query_rpm.npz sphere_b2_130 (xyz + r030_k16 dxyz + ppf: 10 channels, S = 16, with repeated slots;
pointnet_group_refs.rpm_raw_case builds it), through get_prepool(10, 192).  rpm130_w_<key> the state_dict, rpm130_keys its key
list, rpm130_f32 / rpm130_f64 (B, 192, N) the pooled features of the two runs, rpm130_dist = max |f32 - f64|.
pointnet_group_grads.npz, per case NAME = b<B>_n<N>_s<S>_f<feature_dim>, (B, N, S, c0, feature_dim) = (2, 5, 20, 10, 96) and
(2, 7, 64, 10, 32): NAME_x (B, N, S, 10) float32 standard normal (no two slots are equal), NAME_w_<key>, NAME_f32, NAME_f64,
NAME_dist, NAME_arg (B, K, N) the slot the float64 run pools, NAME_gap, NAME_g (B, K, N) float32, and of sum(out * g):
NAME_d32_<key> / NAME_d64_<key> the parameter gradients of the two runs, NAME_d32_x / NAME_d64_x the input gradients.
A draw is kept only if the float32 and the float64 run pool the same slot wherever out > 0 and the relative gap between the best
and the second-best activation is >= 1e-3 there (the condition and constant of make_golden_pointnet.py).  Both shapes meet it
within 50 draws at the N the issue names; N was not shrunk.
"""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402  (registers the stubs, names the reference checkout)

import torch  # noqa: E402

import pointnet_group_refs as GP  # noqa: E402

# (B, N, S, c0, feature_dim)
GRAD_CASES = ((2, 5, 20, 10, 96), (2, 7, 64, 10, 32))
GAP_MIN = 1.0e-3


def reference_module():
    sys.path.insert(0, os.path.join(MG.REF, "exps_deep_learning", "rpm"))
    return importlib.import_module("models.feature_nets")


def run(net, x, dtype):
    """The reference's lines 196-199 on x (B, N, S, C) -> (pooled (B, K, N), the last activation (B, K, S, N))."""
    new_feat = net(x.to(dtype).permute(0, 3, 2, 1))
    return torch.max(new_feat, 2)[0], new_feat


def main():
    ref = reference_module()
    # ---- forward only, on the recorded raw features ----
    bq = np.load(os.path.join(HERE, "ball_query_rpm.npz"), allow_pickle=False)
    x = torch.from_numpy(GP.rpm_raw_case(bq))
    torch.manual_seed(8100)
    fe = ref.FeatExtractionEarlyFusion(["xyz", "dxyz", "ppf"], 96, 0.3, 64).eval()   # its prepool is get_prepool(10, 192)
    net = fe.prepool
    state = {k: v.clone() for k, v in fe.state_dict().items() if k.startswith("prepool.")}
    with torch.no_grad():
        f32 = run(net, x, torch.float32)[0]
        f64 = run(net.double(), x, torch.float64)[0]
    dist = float((f32.double() - f64).abs().max())
    fwd = {"rpm130_f32": f32.numpy(), "rpm130_f64": f64.numpy(), "rpm130_dist": np.array(dist), "rpm130_keys": np.array(list(state))}
    fwd.update({f"rpm130_w_{k}": v.numpy() for k, v in state.items()})
    print("rpm130 dist %.2e of max|f| %.2e" % (dist, float(f64.abs().max())))
    MG.save("pointnet_group.npz", cases=np.array(["rpm130"]), **fwd)
    # ---- gradients ----
    grads, names = {}, []
    for ci, (B, N, S, c0, fd) in enumerate(GRAD_CASES):
        name = f"b{B}_n{N}_s{S}_f{fd}"
        names.append(name)
        K = 2 * fd
        for attempt in range(50):
            seed = 8200 + 100 * ci + attempt
            torch.manual_seed(seed)
            x = torch.from_numpy(np.random.default_rng(seed).standard_normal((B, N, S, c0)).astype(np.float32))
            g = torch.from_numpy(np.random.default_rng(seed + 50000).standard_normal((B, K, N)).astype(np.float32))
            net = ref.get_prepool(c0, K).eval()
            state = {f"prepool.{k}": v.clone() for k, v in net.state_dict().items()}   # the keys FeatExtractionEarlyFusion gives them
            x32 = x.clone().requires_grad_(True)
            f32, h32 = run(net, x32, torch.float32)
            d32 = torch.autograd.grad((f32 * g).sum(), [x32] + list(net.parameters()))
            net.double()
            x64 = x.double().requires_grad_(True)
            f64, h64 = run(net, x64, torch.float64)
            d64 = torch.autograd.grad((f64 * g.double()).sum(), [x64] + list(net.parameters()))
            a32, a64 = h32.argmax(2), h64.argmax(2)
            top = h64.detach().topk(2, dim=2).values
            on = f64.detach() > 0
            gap = float(((top[:, :, 0] - top[:, :, 1]) / top[:, :, 0].clamp_min(1e-300))[on].min()) if on.any() else np.inf
            if bool((a32 == a64)[on].all()) and gap >= GAP_MIN:
                break
        else:
            raise RuntimeError(f"{name}: no draw within the conditions")
        dist = float((f32.detach().double() - f64.detach()).abs().max())
        keys = ["x"] + [f"prepool.{k}" for k, _ in net.named_parameters()]
        grads.update({f"{name}_x": x.numpy(), f"{name}_f32": f32.detach().numpy(), f"{name}_f64": f64.detach().numpy(),
                      f"{name}_dist": np.array(dist), f"{name}_arg": a64.numpy().astype(np.int8), f"{name}_gap": np.array(gap),
                      f"{name}_g": g.numpy()})
        grads.update({f"{name}_w_{k}": v.numpy() for k, v in state.items()})
        grads.update({f"{name}_d32_{k}": v.numpy() for k, v in zip(keys, d32)})
        grads.update({f"{name}_d64_{k}": v.numpy() for k, v in zip(keys, d64)})
        print(name, "attempt", attempt, "dist %.2e" % dist, "gap %.2e" % gap)
    MG.save("pointnet_group_grads.npz", cases=np.array(names), **grads)


if __name__ == "__main__":
    main()
