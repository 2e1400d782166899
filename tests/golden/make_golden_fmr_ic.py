#!/usr/bin/env python3
"""Generate tests/golden/fmr_ic.npz -- FMR's inverse-compositional head on a few small cases -- by RUNNING THE REFERENCE's
SolveRegistration.approx_Jac and ic_algo (fmr/model.py:318-439) on the CPU in float32 around its own PointNet at random
initialisation, with the helpers of make_golden.py (same stubs, same reference checkout).

Run in the build container only (needs the reference checkout, see make_golden.py):

    python tests/golden/make_golden_fmr_ic.py

The reference module imports igl and plyfile and its se_math package imports its mesh and transforms modules for the data
loaders; the head uses none of them, so empty stand-ins are registered first (as h5py for DCP).

Clouds: points on the surface of an ellipsoid with semi-axes 1 / 0.6 / 0.3, zero-meaned; p1 is p0 under a pose of about 0.14 rad
(the stop case: p1 = p0, so r = 0 at iteration 0 and the reference breaks there).  dt = 1e-2.  Per case NAME, recorded from the
reference's run (the encoder's outputs through a forward hook, J from approx_Jac's return, g and dx from the arguments of
`update`; pinv, and dx of an iteration that breaks, by the same three torch lines of ic_algo on the recorded tensors):
    NAME_p0, _p1 (B, N, 3), _dt (B, 6), _f0 (B, K), _fp (B, 6, K), _J (B, K, 6), _pinv (B, 6, K),
    NAME_f1 (n, B, K), _r (n, B, K), _dx (n, B, 6), _g_in (n, B, 4, 4), _g_out (n, B, 4, 4) for the n iterations the reference
    ran (g_out = g_in where it broke), NAME_moved (n,) = 0 where it broke, NAME_g (B, 4, 4) the final pose, NAME_maxiter,
    NAME_xtol, NAME_cond (B,) cond_2(H);
the float32 head's own distance from a float64 evaluation (the reference's own functions on float64 copies) of the SAME
recorded float32 features:
    NAME_pinv64_dist, NAME_dx64_dist (n,), NAME_g64_dist (n,)   (max abs over the batch);
and the same loop from an all-float64 run of the same weights: NAME_g64 (n, B, 4, 4) with NAME_loop_dist = max |g_out - g64|.
For the case WEIGHTS the encoder's state_dict is stored as WEIGHTS_w_<name>.  A draw is kept only when every sample has
cond_2(H) <= 1e4 and, for WEIGHTS, loop_dist <= 1e-3 (no max-pool argmax cascade behind the closed-loop bound).
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

import fmr_refs as FR  # noqa: E402

# name -> (B, N, K, maxiter, stop case)
CASES = {
    "b2_n64_k32": (2, 64, 32, 5, False),
    "b2_n130_k64": (2, 130, 64, 5, False),
    "b1_n257_k1024": (1, 257, 1024, 5, False),
    "b3_n33_k64_it10": (3, 33, 64, 10, False),
    "b2_n64_k32_stop": (2, 64, 32, 5, True),
}
WEIGHTS = "b2_n64_k32"
XTOL = 1.0e-7
COND_MAX, LOOP_MAX = 1.0e4, 1.0e-3


def reference_module():
    for name in ("igl", "plyfile", "se_math.mesh", "se_math.transforms"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.path.insert(0, os.path.join(MG.REF, "exps_deep_learning", "fmr"))
    return importlib.import_module("model")


def run(ref, net, p0, p1, maxiter, dtype):
    """One ic_algo of the reference in `dtype` -> dict of what it computed (numpy, in `dtype`)."""
    solver = ref.SolveRegistration(net).to(dtype)
    solver.device = torch.device("cpu")
    feats, steps, jac = [], [], []
    hook = net.register_forward_hook(lambda m, i, o: feats.append(o.detach().clone()))
    update, approx = solver.update, solver.approx_Jac
    solver.update = lambda g, dx: (steps.append((g.detach().clone(), dx.detach().clone())), update(g, dx))[1]
    solver.approx_Jac = lambda a, f, d: (jac.append(approx(a, f, d)), jac[-1])[1]
    tp0, tp1 = torch.from_numpy(p0).to(dtype), torch.from_numpy(p1).to(dtype)
    g0 = torch.eye(4, dtype=dtype).view(1, 4, 4).expand(p0.shape[0], 4, 4).contiguous()
    with torch.no_grad():
        r, g, _ = solver.ic_algo(g0, tp0, tp1, maxiter, XTOL)
        hook.remove()
        assert solver.last_err in (None, 0), solver.last_err
        B = p0.shape[0]
        # the encoder's calls in ic_algo's order: f0, f1 (lines 340-341), f0 again (363), the perturbed clouds, then one per iteration
        f0, fp, f1s = feats[2], feats[3].view(B, 6, -1), feats[4:]
        J = jac[0].detach()
        Jt = J.transpose(1, 2)
        H = Jt.bmm(J)
        pinv = solver.inverse(H).bmm(Jt)
        n = len(f1s)
        g_in = [s[0] for s in steps] + ([g] if len(steps) < n else [])
        rs = [f1 - f0 for f1 in f1s]
        dxs = [-pinv.bmm(rr.unsqueeze(-1)).view(B, 6) for rr in rs]
        for (_, dx), mine in zip(steps, dxs):
            assert torch.equal(dx, mine)  # the three lines above ARE the run's
        g_out = [solver.g_series[i + 1] for i in range(len(steps))] + ([g] if len(steps) < n else [])
        moved = np.array([1] * len(steps) + [0] * (n - len(steps)), np.int32)
    num = lambda t: t.detach().numpy()  # noqa: E731
    return dict(f0=num(f0), fp=num(fp), J=num(J), H=num(H), pinv=num(pinv), f1=np.stack([num(f) for f in f1s]),
                r=np.stack([num(x) for x in rs]), dx=np.stack([num(x) for x in dxs]), g_in=np.stack([num(x) for x in g_in]),
                g_out=np.stack([num(x) for x in g_out]), moved=moved, g=num(g), solver=solver)


def head64(ref, solver32, rec, dt):
    """The reference's head functions in float64 on the RECORDED float32 features -> (pinv64, dx64 (n, B, 6), g64 (n, B, 4, 4))."""
    d = torch.float64
    f0, fp = torch.from_numpy(rec["f0"]).to(d), torch.from_numpy(rec["fp"]).to(d)
    J = (f0.unsqueeze(-1) - fp.transpose(1, 2)) / torch.from_numpy(dt).to(d).unsqueeze(1)
    Jt = J.transpose(1, 2)
    pinv = solver32.inverse(Jt.bmm(J)).bmm(Jt)
    dxs, gs = [], []
    for i in range(rec["f1"].shape[0]):
        r = torch.from_numpy(rec["r"][i]).to(d)
        dx = -pinv.bmm(r.unsqueeze(-1)).view(-1, 6)
        g_in = torch.from_numpy(rec["g_in"][i]).to(d)
        dxs.append(dx.numpy())
        gs.append(solver32.update(g_in, dx).numpy() if rec["moved"][i] else g_in.numpy())
    return pinv.numpy(), np.stack(dxs), np.stack(gs)


def main():
    ref = reference_module()
    kw = dict(cases=np.array(list(CASES)), weights=np.array(WEIGHTS))
    for ci, (name, (B, N, K, maxiter, stop)) in enumerate(CASES.items()):
        for attempt in range(50):
            seed = 1000 * ci + attempt
            rng = np.random.default_rng(seed)
            torch.manual_seed(seed)
            p0 = FR.ellipsoid_cloud(rng, B, N)
            twist = rng.standard_normal((B, 6))
            twist[:, :3] *= 0.14 / np.linalg.norm(twist[:, :3], axis=1, keepdims=True)
            twist[:, 3:] *= 0.03
            T = np.stack([FR.exp6(x) for x in twist])
            p1 = p0.copy() if stop else (np.einsum("bij,bnj->bni", T[:, :3, :3], p0.astype(np.float64)) + T[:, None, :3, 3]).astype(np.float32)
            net = ref.PointNet(dim_k=K).eval()
            rec = run(ref, net, p0, p1, maxiter, torch.float32)
            state = {k: v.clone() for k, v in net.state_dict().items()}
            rec64 = run(ref, net.double(), p0, p1, maxiter, torch.float64)
            net.float()
            cond = np.array([np.linalg.cond(h.astype(np.float64)) for h in rec["H"]])
            n = rec["f1"].shape[0]
            same = rec64["f1"].shape[0] == n
            loop = float(np.abs(rec["g_out"] - rec64["g_out"]).max()) if same else np.inf
            if (cond <= COND_MAX).all() and same and (name != WEIGHTS or loop <= LOOP_MAX):
                break
        else:
            raise RuntimeError(f"{name}: no draw within the conditions")
        assert (n == 1 and not rec["moved"].any()) if stop else (n == maxiter and rec["moved"].all()), (name, rec["moved"])
        dt = np.full((B, 6), 1.0e-2, np.float32)
        assert np.array_equal(dt[:1], rec["solver"].dt.detach().numpy())
        pinv64, dx64, g64h = head64(ref, rec["solver"], rec, dt)
        for key in ("f0", "fp", "J", "pinv", "f1", "r", "dx", "g_in", "g_out", "moved", "g"):
            kw[f"{name}_{key}"] = rec[key]
        kw.update({f"{name}_p0": p0, f"{name}_p1": p1, f"{name}_dt": dt, f"{name}_maxiter": np.array(maxiter),
                   f"{name}_xtol": np.array(XTOL), f"{name}_cond": cond,
                   f"{name}_pinv64_dist": np.array(np.abs(rec["pinv"] - pinv64).max()),
                   f"{name}_dx64_dist": np.abs(rec["dx"] - dx64).reshape(n, -1).max(1),
                   f"{name}_g64_dist": np.abs(rec["g_out"] - g64h).reshape(n, -1).max(1),
                   f"{name}_g64": rec64["g_out"], f"{name}_loop_dist": np.array(loop)})
        if name == WEIGHTS:
            kw.update({f"{name}_w_{k}": v.numpy() for k, v in state.items()})
        print(name, "attempt", attempt, "cond", cond.round(1).tolist(), "loop_dist %.2e" % loop, "pinv64_dist %.2e" % kw[f"{name}_pinv64_dist"],
              "iterations", n)
    MG.save("fmr_ic.npz", **kw)


if __name__ == "__main__":
    main()
