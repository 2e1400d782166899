#!/usr/bin/env python3
"""Generate tests/golden/knn_dcp.npz -- DCP's k-NN graph on a few small clouds -- by RUNNING THE REFERENCE's knn
(dcp/model.py:46-52) on the CPU in float32, with the helpers of make_golden.py (same reference checkout).

Run in the build container only (needs the reference checkout, see make_golden.py):

    python tests/golden/make_golden_knn_dcp.py

Per case of knn_refs.DCP_CASES: the cloud xyz (B, N, 3) float32 as drawn by group_refs.make_cloud (the GPU path reads exactly
these numbers) and, per k of knn_refs.DCP_KS, the reference's indices (B, N, k) as int16.  The reference module imports h5py
for its data loaders; knn does not use it and it is not installed here, so an empty stand-in is registered first.
"""
import importlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402  (names the reference checkout)

import torch  # noqa: E402

import knn_refs as KR  # noqa: E402


def reference_module():
    sys.modules.setdefault("h5py", types.ModuleType("h5py"))
    sys.path.insert(0, os.path.join(MG.REF, "exps_deep_learning", "dcp"))
    return importlib.import_module("model")


def main():
    ref = reference_module()
    kw = dict(cases=np.array(list(KR.DCP_CASES)), ks=np.array(KR.DCP_KS, np.int32))
    for name, (seed, B, N, kind) in KR.DCP_CASES.items():
        x = torch.from_numpy(KR.dcp_cloud(name))
        kw[f"{name}_xyz"] = x.numpy()
        for k in KR.DCP_KS:
            idx = ref.knn(x.transpose(2, 1).contiguous(), k)
            assert tuple(idx.shape) == (B, N, k) and int(idx.min()) >= 0 and int(idx.max()) < N
            kw[f"{name}_k{k}_idx"] = idx.numpy().astype(np.int16)
        print(name, KR.DCP_KS)
    MG.save("knn_dcp.npz", **kw)


if __name__ == "__main__":
    main()
