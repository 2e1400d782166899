#!/usr/bin/env python3
"""Generate tests/golden/pointer_dcp.npz -- DCP's SVD head on a few small cases -- by RUNNING THE REFERENCE's SVDHead.forward
(dcp/model.py:405-459) on the CPU in float32, with the helpers of make_golden.py (same stubs, same reference checkout).

Run in the build container only (needs the reference checkout, see make_golden.py):

    python tests/golden/make_golden_pointer_dcp.py

Per case of pointer_refs-style (B, C, N, M, sigma): the inputs src_emb (B, C, N), tgt_emb (B, C, M), src (B, 3, N), tgt
(B, 3, M) as float32 (the GPU path reads exactly these numbers), the head's R (B, 3, 3) and t (B, 3), and src_corr (B, 3, N),
which the head does not return: recomputed here by the three lines of its forward (model.py:419-425).  The reference module
imports h5py for its data loaders; the head does not use it, so an empty stand-in is registered first.  A draw is kept only
when every sample's rotation is well determined (the Kabsch twin's gap (s1 + delta s2) / s0 >= 1e-2).
"""
import importlib
import math
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
import pointer_refs as PR  # noqa: E402

# name -> (B, C, N, M, sigma)
CASES = {
    "b2_c64_65x70": (2, 64, 65, 70, 1.0),
    "b1_c512_33x40": (1, 512, 33, 40, 1.0),
    "b2_c33_64x64_s4": (2, 33, 64, 64, 4.0),
}
GAP_MIN = 1e-2


def reference_module():
    sys.modules.setdefault("h5py", types.ModuleType("h5py"))
    sys.path.insert(0, os.path.join(MG.REF, "exps_deep_learning", "dcp"))
    return importlib.import_module("model")


def main():
    ref = reference_module()
    kw = dict(cases=np.array(list(CASES)))
    for i, (name, (B, C, N, M, sigma)) in enumerate(CASES.items()):
        head = ref.SVDHead(types.SimpleNamespace(emb_dims=C))
        for attempt in range(50):
            se, te, tgt, _ = PR.make_case(C, N, M, B, sigma, "random", seed=1000 * i + attempt)
            src = np.random.default_rng(77 + 1000 * i + attempt).uniform(-1.0, 1.0, (B, 3, N)).astype(np.float32)
            tse, tte, tsrc, ttgt = (torch.from_numpy(v) for v in (se, te, src, tgt))
            with torch.no_grad():
                R, t = head(tse, tte, tsrc, ttgt)
                sc = torch.softmax(torch.matmul(tse.transpose(2, 1).contiguous(), tte) / math.sqrt(tse.size(1)), dim=2)
                corr = torch.matmul(ttgt, sc.transpose(2, 1).contiguous())
            fits = [KR.fit(src[b].T, corr[b].numpy().T) for b in range(B)]
            gaps = np.array([f["gap"] / f["S"][0] for f in fits])
            if (gaps >= GAP_MIN).all():
                break
        else:
            raise RuntimeError(f"{name}: no draw with a determined rotation")
        kw.update({f"{name}_src_emb": se, f"{name}_tgt_emb": te, f"{name}_src": src, f"{name}_tgt": tgt, f"{name}_R": R.numpy(),
                   f"{name}_t": t.numpy(), f"{name}_src_corr": corr.numpy(), f"{name}_gap": gaps})
        print(name, "attempt", attempt, "gaps", gaps.round(4).tolist())
    MG.save("pointer_dcp.npz", **kw)


if __name__ == "__main__":
    main()
