#!/usr/bin/env python3
"""Generate tests/golden/sinkhorn_rpm.npz -- RPM-Net's match head on a few small cases -- by RUNNING THE REFERENCE's sinkhorn
(rpm/models/rpmnet.py:48-118) and the lines 214-222 behind it (exp, the weighted reference points, compute_rigid_transform)
on the CPU in float64, with the helpers of make_golden.py (same stubs, same reference checkout).

Run in the build container only (needs the reference checkout, see make_golden.py):

    python tests/golden/make_golden_sinkhorn.py

Per case: the inputs log_alpha (B, J, K), xyz_src (B, J, 3), xyz_ref (B, K, 3), stored as float32 (the GPU path reads exactly
these numbers); log_perm, W, s, c and the (B, 3, 4) transform in float64; the autograd gradients of the fixed contraction
sum(W C_W) + sum(s C_s) + sum(c C_c) with respect to log_alpha and xyz_ref, the three C recorded too; and the relative gap
(s1 + delta s2) / s0 of every sample's Kabsch solve, which the script requires to be >= 1e-3 wherever a rotation exists
(J >= 3): the transform is only compared where it is determined.
"""
import importlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402  (registers the stubs, names the reference checkout)

import torch  # noqa: E402

import kabsch_refs as KR  # noqa: E402

GAP_MIN = 1e-3


def reference_module():
    rpm = os.path.join(MG.REF, "exps_deep_learning", "rpm")
    sys.path.insert(0, rpm)
    for _ in range(8):  # modules the file imports for its network, not for the head: stubbed when absent here
        try:
            return importlib.import_module("models.rpmnet")
        except ModuleNotFoundError as e:
            if e.name.split(".")[0] in ("models", "common"):
                raise
            sys.modules[e.name] = types.ModuleType(e.name)
    raise RuntimeError("could not import the reference's rpmnet")


# name -> (B, J, K, slack, n_iters, entry scale)
CASES = {
    "slack_b2_5x7": (2, 5, 7, True, 5, 3.0),
    "noslack_b1_9x4": (1, 9, 4, False, 3, 10.0),
    "slack_b2_33x48": (2, 33, 48, True, 5, 30.0),
    "noiter_b1_6x6": (1, 6, 6, True, 0, 3.0),
    "single_b1_1x1": (1, 1, 1, True, 2, 3.0),
}


def make_case(seed, B, J, K, scale):
    rs = np.random.default_rng(seed)
    f32 = lambda v: v.astype(np.float32)  # noqa: E731
    A = f32(scale * rs.standard_normal((B, J, K)))
    src, ref = f32(rs.uniform(-1.0, 1.0, (B, J, 3))), f32(rs.uniform(-1.0, 1.0, (B, K, 3)))
    C = [f32(rs.standard_normal(s)) for s in ((B, J, 3), (B, J), (B, K))]
    return A, src, ref, C


def main():
    ref = reference_module()
    kw = dict(cases=np.array(list(CASES)))
    for i, (name, (B, J, K, slack, n, scale)) in enumerate(CASES.items()):
        for attempt in range(50):  # a draw whose solve is well determined
            A, src, xr, C = make_case(1000 * i + attempt, B, J, K, scale)
            ta, tx = (torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (A, xr))
            log_perm = ref.sinkhorn(ta, n_iters=n, slack=slack)
            perm = torch.exp(log_perm)
            W = perm @ tx / (torch.sum(perm, dim=2, keepdim=True) + 1e-5)
            s, c = torch.sum(perm, dim=2), torch.sum(perm, dim=1)
            Wn, sn = W.detach().numpy(), s.detach().numpy()
            fits = [KR.fit(src[b], Wn[b].astype(np.float32), sn[b].astype(np.float32), eps=1e-5) for b in range(B)]
            gaps = np.array([f["gap"] / f["S"][0] if f["S"][0] > 0 else 0.0 for f in fits])
            if J < 3 or (gaps >= 10 * GAP_MIN).all():
                break
        else:
            raise RuntimeError(f"{name}: no draw with a determined rotation")
        transform = ref.compute_rigid_transform(torch.tensor(src, dtype=torch.float64), W, weights=s)
        CW, Cs, Cc = (torch.tensor(v, dtype=torch.float64) for v in C)
        ((W * CW).sum() + (s * Cs).sum() + (c * Cc).sum()).backward()
        kw.update({f"{name}_log_alpha": A, f"{name}_xyz_src": src, f"{name}_xyz_ref": xr, f"{name}_CW": C[0], f"{name}_Cs": C[1],
                   f"{name}_Cc": C[2], f"{name}_spec": np.array([int(slack), n]), f"{name}_log_perm": log_perm.detach().numpy(),
                   f"{name}_W": Wn, f"{name}_s": sn, f"{name}_c": c.detach().numpy(), f"{name}_transform": transform.detach().numpy(),
                   f"{name}_gA": ta.grad.numpy(), f"{name}_gx": tx.grad.numpy(), f"{name}_gap": gaps})
        print(name, "attempt", attempt, "gaps", gaps.round(4).tolist(), "s", sn[0, :3].round(4).tolist())
    MG.save("sinkhorn_rpm.npz", **kw)


if __name__ == "__main__":
    main()
