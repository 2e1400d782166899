#!/usr/bin/env python3
"""Generate tests/golden/kabsch_rpm.npz -- RPM-Net's weighted Kabsch solve on a few small cases -- by RUNNING THE REFERENCE's
compute_rigid_transform (rpm/models/rpmnet.py:121-157) on the CPU in float64, with the helpers of make_golden.py (same stubs,
same reference checkout).

Run in the build container only (needs the reference checkout, see make_golden.py):

    python tests/golden/make_golden_kabsch.py

Per case: inputs a, b (B, n, 3) and weights (B, n); the (B, 3, 4) transform; the autograd gradients of the fixed contraction
sum(transform * C) with respect to a, b and the weights, C (B, 3, 4) recorded too.  n <= 64: a few kilobytes.  DCP's SVDHead
(dcp/model.py:405-455) needs h5py to import; it is the weights = 1, eps = 0 case of the same formula and is restated in
tests/kabsch_refs.py.
"""
import importlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (registers the stubs, names the reference checkout)

import torch  # noqa: E402


def reference_solver():
    rpm = os.path.join(MG.REF, "exps_deep_learning", "rpm")
    sys.path.insert(0, rpm)
    for _ in range(8):  # modules the file imports for its network, not for the solve: stubbed when absent here
        try:
            return importlib.import_module("models.rpmnet").compute_rigid_transform
        except ModuleNotFoundError as e:
            if e.name.split(".")[0] in ("models", "common"):
                raise
            sys.modules[e.name] = types.ModuleType(e.name)
    raise RuntimeError("could not import the reference's rpmnet")


# name -> (B, n, rotation angle in degrees, noise, offset of the clouds from the origin, weight pattern)
CASES = {
    "rigid_b2_n64": (2, 64, 35.0, 0.0, 0.0, "uniform"),
    "noisy_b3_n33": (3, 33, 80.0, 0.05, 0.0, "random"),
    "offset_b2_n17": (2, 17, 15.0, 0.01, 30.0, "random"),
    "sparse_b2_n8": (2, 8, 120.0, 0.02, 0.0, "zeros"),
}


def make_case(seed, B, n, angle, noise, offset, weights):
    rs = np.random.default_rng(seed)
    a = rs.uniform(-1.0, 1.0, (B, n, 3)) + offset
    b = np.empty_like(a)
    for i in range(B):
        ax = rs.standard_normal(3)
        ax /= np.linalg.norm(ax)
        th = np.deg2rad(angle)
        K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        Rc = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
        b[i] = a[i] @ Rc.T + rs.uniform(-0.5, 0.5, 3) + noise * rs.standard_normal((n, 3))
    w = np.ones((B, n)) if weights == "uniform" else rs.uniform(0.05, 1.0, (B, n))
    if weights == "zeros":
        w[:, ::2] = 0.0
    # float32-representable inputs: the GPU path reads exactly these numbers
    return (x.astype(np.float32).astype(np.float64) for x in (a, b, w, rs.standard_normal((B, 3, 4))))


def main():
    solve = reference_solver()
    kw = dict(cases=np.array(list(CASES)))
    for i, (name, spec) in enumerate(CASES.items()):
        a, b, w, C = make_case(100 + i, *spec)
        ta, tb, tw = (torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in (a, b, w))
        out = solve(ta, tb, tw)
        (out * torch.tensor(C)).sum().backward()
        kw.update({f"{name}_a": a, f"{name}_b": b, f"{name}_w": w, f"{name}_C": C, f"{name}_transform": out.detach().numpy(),
                   f"{name}_ga": ta.grad.numpy(), f"{name}_gb": tb.grad.numpy(), f"{name}_gw": tw.grad.numpy()})
        print(name, out.detach().numpy()[0].round(4).tolist())
    MG.save("kabsch_rpm.npz", **kw)


if __name__ == "__main__":
    main()
