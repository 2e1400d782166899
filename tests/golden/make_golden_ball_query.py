#!/usr/bin/env python3
"""Generate tests/golden/ball_query_rpm.npz -- RPM-Net's grouping on a few small clouds -- by RUNNING THE REFERENCE's
query_ball_point (rpm/models/pointnet_util.py:96-131) and sample_and_group_multi (:197-244) on the CPU in float32, with the
helpers of make_golden.py (same reference checkout).

Run in the build container only (needs the reference checkout, see make_golden.py):

    python tests/golden/make_golden_ball_query.py

Per case: the cloud xyz (B, N, 3) float32 as drawn by group_refs.make_cloud (the GPU path reads exactly these numbers), and
per (radius, nsample) the indices of query_ball_point with itself_indices = every point's own index (what
sample_and_group_multi passes), as int16.  The two small cases are also recorded at nsample 64 and with itself_indices = None
(sample_and_group's form); a row without any member holds N there, recorded as it is.  The 130-point case carries its
normals and the dxyz and ppf tensors of sample_and_group_multi.
"""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402  (names the reference checkout)

import torch  # noqa: E402

import group_refs as GR  # noqa: E402

# name -> (seed, B, N, kind)
CASES = {
    "cube_b4_1024": (0, 4, 1024, "cube"),
    "sphere_b4_1024": (1, 4, 1024, "sphere"),
    "sphere_b2_717": (2, 2, 717, "sphere"),
    "cube_b3_257": (3, 3, 257, "cube"),
    "sphere_b2_130": (4, 2, 130, "sphere"),
}
SETTINGS = [(0.3, 16), (0.1, 8)]
SMALL = [(0.3, 64)]  # ... and for the clouds of at most 257 points
FEATURE_CASE = "sphere_b2_130"


def reference_module():
    sys.path.insert(0, os.path.join(MG.REF, "exps_deep_learning", "rpm"))
    return importlib.import_module("models.pointnet_util")


def tag(radius, nsample):
    return f"r{int(round(radius * 100)):03d}_k{nsample}"


def main():
    ref = reference_module()
    kw = dict(cases=np.array(list(CASES)))
    for name, (seed, B, N, kind) in CASES.items():
        x, nr = GR.make_cloud(seed, B, N, kind)
        own = torch.arange(N)[None].repeat(B, 1)
        kw[f"{name}_xyz"] = x.numpy()
        settings = SETTINGS + (SMALL if N <= 257 else [])
        kw[f"{name}_settings"] = np.array(settings, np.float64)
        for radius, nsample in settings:
            idx = ref.query_ball_point(radius, nsample, x, x, own)
            assert int(idx.min()) >= 0 and int(idx.max()) < N
            kw[f"{name}_{tag(radius, nsample)}_idx"] = idx.numpy().astype(np.int16)
            if N <= 257:
                idx0 = ref.query_ball_point(radius, nsample, x, x)
                kw[f"{name}_{tag(radius, nsample)}_idx_noself"] = idx0.numpy().astype(np.int16)
            if name == FEATURE_CASE:
                out = ref.sample_and_group_multi(-1, radius, nsample, x, nr)
                assert torch.equal(out["xyz"], x)
                kw[f"{name}_{tag(radius, nsample)}_dxyz"] = out["dxyz"].numpy()
                kw[f"{name}_{tag(radius, nsample)}_ppf"] = out["ppf"].numpy()
        if name == FEATURE_CASE:
            kw[f"{name}_normals"] = nr.numpy()
        print(name, [tag(*s) for s in settings])
    MG.save("ball_query_rpm.npz", **kw)


if __name__ == "__main__":
    main()
