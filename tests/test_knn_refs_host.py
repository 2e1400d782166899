"""The numpy twin of rrl_knn (tests/knn_refs.py) against what it must reproduce, and every Python-side refusal of
rrl_hip.neighbors.knn / knn_group / estimate_normals_knn and the DCP call sites.  No GPU, no GPU call.

- the fixture tests/golden/knn_dcp.npz (the reference's own knn, dcp/model.py:46-52, recorded on the CPU): per case at most
  2 % of the rows are borderline -- two consecutive keys among the first k + 1 within 2^-20 (|x_i|^2 + |x_j|^2), where the
  reference's float32 matmul expansion may order them either way -- and every other row equals the recorded indices, in order;
- k = 3 against prep_refs' 3-NN twin;
- the found, pad and zero-row rules on hand-made clouds."""
import numpy as np
import pytest
import torch

import knn_refs as KR
import prep_refs as PR
from conftest import load_golden


@pytest.mark.parametrize("k", KR.DCP_KS)
@pytest.mark.parametrize("name", list(KR.DCP_CASES))
def test_twin_against_the_recorded_reference(name, k):
    g = load_golden("knn_dcp.npz")
    x = g[f"{name}_xyz"]
    assert x.dtype == np.float32 and np.array_equal(x, KR.dcp_cloud(name))  # the GPU tests draw the same numbers
    want = g[f"{name}_k{k}_idx"].astype(np.int32)
    twin = KR.knn(x, k)
    share = twin["border"].mean()
    exact = (twin["idx"] == want).all(-1)
    print(f"{name} k={k}: borderline share {100 * share:.2f} %, rows that differ {int((~exact).sum())}")
    assert share <= KR.BORDER_SHARE_MAX, (name, k, share)
    assert exact[~twin["border"]].all(), (name, k, int((~exact & ~twin["border"]).sum()))
    assert (twin["found"] == k).all()


def test_twin_at_k3_is_the_3nn_twin():
    for seed, n in ((1, 3), (2, 64), (3, 300)):
        x = PR.gaussian_cloud(seed, 2, n)
        twin = KR.knn(x, 3)
        for b in range(2):
            assert np.array_equal(twin["idx"][b], PR.knn3_ref(x[b], np.arange(n)))
    lat = PR.lattice_cloud(5)[:700]  # equal distances everywhere, copies with a twin at a lower index
    assert np.array_equal(KR.knn(lat[None], 3)["idx"][0], PR.knn3_ref(lat, np.arange(len(lat))))


def test_twin_rules_on_hand_made_clouds():
    # n < k: found says what exists, the open slots repeat slot 0
    x = np.array([[[0, 0, 0], [1, 0, 0], [3, 0, 0]]], np.float32)
    t = KR.knn(x, 5)
    assert t["found"].tolist() == [[3, 3, 3]]
    assert t["idx"][0].tolist() == [[0, 1, 2, 0, 0], [1, 0, 2, 1, 1], [2, 1, 0, 2, 2]]
    assert t["d"][0, 2].tolist() == [0.0, 4.0, 9.0, 0.0, 0.0]
    t = KR.knn(x, 5, exclude_self=True)
    assert t["found"].tolist() == [[2, 2, 2]] and t["idx"][0, 1].tolist() == [0, 2, 0, 0, 0]
    # duplicates: the lowest index first; exclude_self removes the own row only
    dup = np.array([[[1, 1, 1]] * 3 + [[2, 1, 1]]], np.float32)
    assert KR.knn(dup, 2)["idx"][0].tolist() == [[0, 1], [0, 1], [0, 1], [3, 0]]
    assert KR.knn(dup, 2, exclude_self=True)["idx"][0].tolist() == [[1, 2], [0, 2], [0, 1], [0, 1]]
    # a NaN point: a neighbour of nobody, and its own row is zero
    bad = x.copy()
    bad[0, 1, 1] = np.nan
    t = KR.knn(bad, 2)
    assert t["found"].tolist() == [[2, 0, 2]] and t["idx"][0].tolist() == [[0, 2], [0, 0], [2, 0]]
    assert not KR.features(bad, t, ("nbr", "dxyz", "ctr"))[0, 1].any()
    # an empty sample and rows beyond a count: zero; the cross form with its own counts
    t = KR.knn(np.concatenate([x, x]), 2, counts=[0, 2])
    assert not t["idx"][0].any() and not t["found"][0].any() and t["found"][1].tolist() == [2, 2, 0]
    q = np.array([[[0.9, 0, 0], [5, 0, 0]]], np.float32)
    t = KR.knn(x, 2, query=q, qcounts=[1])
    assert t["idx"][0].tolist() == [[1, 0], [0, 0]] and t["found"].tolist() == [[2, 0]]
    f = KR.features(x, t, ("ctr", "nbr"), query=q, channel_first=True)  # the kernel's order, whatever the order given
    assert f.shape == (1, 6, 2, 2) and f[0, :3, 0, 0].tolist() == [1, 0, 0] and np.allclose(f[0, 3:, 0, 1], [0.9, 0, 0]) and not f[0, :, 1].any()
    # the borderline mask: equal keys are borderline, well separated ones are not
    assert KR.knn(dup, 1)["border"][0].tolist() == [True, True, True, False]
    assert not KR.knn(x, 2)["border"].any()


def test_python_refusals_need_no_device():
    from rrl_hip import callsites, neighbors
    x = torch.zeros(2, 5, 3)
    for k in (0, 33, 2.5, True, -1):
        with pytest.raises(ValueError, match="k must be"):
            neighbors.knn(x, k)
    with pytest.raises(ValueError, match="method"):
        neighbors.knn(x, 3, method="kd")
    with pytest.raises(ValueError, match="points"):
        neighbors.knn(torch.zeros(5, 3), 3)
    with pytest.raises(ValueError, match="at least one point"):
        neighbors.knn(torch.zeros(2, 0, 3), 3)
    with pytest.raises(ValueError, match="at least one point"):
        neighbors.knn(torch.zeros(0, 5, 3), 3)
    with pytest.raises(ValueError, match="query"):
        neighbors.knn(x, 3, query=torch.zeros(3, 4, 3))
    with pytest.raises(ValueError, match="points"):
        neighbors.knn(x, 3, query=torch.zeros(2, 4))
    with pytest.raises(ValueError, match="exclude_self"):
        neighbors.knn(x, 3, query=torch.zeros(2, 4, 3), exclude_self=True)
    with pytest.raises(ValueError, match="qcounts"):
        neighbors.knn(x, 3, qcounts=[1, 1])
    for kw, match in ((dict(counts=[1, 6]), r"\[0, 5\]"), (dict(counts=[1]), "one per sample"), (dict(counts=[1.0, 2.0]), "integers"),
                      (dict(query=torch.zeros(2, 4, 3), qcounts=[5, 0]), r"\[0, 4\]")):
        with pytest.raises(ValueError, match=match):
            neighbors.knn(x, 3, **kw)
    big = torch.zeros(1, 1, 3).expand(1, (1 << 20) + 1, 3)  # (no memory behind it)
    with pytest.raises(ValueError, match="tree serves"):
        neighbors.knn(big, 3, method="tree")
    with pytest.raises(ValueError, match="tree serves"):
        neighbors.knn(x, 3, query=big.expand(2, -1, -1), method="tree")
    for bad in ((), ("nbr", "nbr"), ("xyz",)):
        with pytest.raises(ValueError, match="features"):
            neighbors.knn_group(x, 3, features=bad)
    with pytest.raises(ValueError, match="k must be"):
        neighbors.estimate_normals_knn(x, 40)
    for fn in (callsites.dcp_knn, callsites.dcp_graph_feature):
        with pytest.raises(ValueError, match="out of range"):
            fn(torch.zeros(2, 3, 5), 6)
        with pytest.raises(ValueError, match=r"\(B, 3, N\)"):
            fn(torch.zeros(2, 5, 3), 2)
        with pytest.raises(ValueError, match="k must be"):
            fn(torch.zeros(2, 3, 50), 33)
        with pytest.raises(ValueError, match="positive integer"):
            fn(torch.zeros(2, 3, 50), 0)
    assert neighbors.MAX_K == 32 and neighbors.KNN_FEATURES == KR.FEATURES
    assert neighbors.KNN_TREE_MIN_POINTS is None or neighbors.KNN_TREE_MIN_POINTS >= 1


# (B, n[, S]) -> bytes at the commit before the three scratches shared one layout (PairLayout, csrc/rrl_tree.h): a caller who
# sized a buffer with that library must still fit, so a size may shrink and never grow
SCRATCH_BYTES_BEFORE = {
    "rrl_chamfer_workspace_bytes": {(1, 3): 5376, (3, 64): 17664, (3, 65): 27904, (2, 4096): 648960, (2, 4097): 787200,
                                    (1, 1 << 20): 82904320, (2, 4097, 130): 475648, (2, 130, 4097): 475648},
    "rrl_knn3_self_workspace_bytes": {(1, 3): 2816, (3, 64): 5888, (3, 65): 10240, (2, 4096): 193536, (2, 4097): 459008,
                                      (1, 1 << 20): 41484800},
    "rrl_knn_workspace_bytes": {(1, 3): 4608, (3, 64): 10752, (3, 65): 19456, (2, 4096): 384256, (2, 4097): 784128,
                                (1, 1 << 20): 82641408, (2, 4097, 130): 472576, (2, 130, 4097): 472576},
}


@pytest.mark.parametrize("entry", list(SCRATCH_BYTES_BEFORE))
def test_scratch_sizes_never_grow(entry):
    """The size functions of the entries that build the sorted layout in their own scratch (the Chamfer walk, the all-points 3-NN,
    the any-k k-NN): positive, at most what they returned before, 0 for a negative dimension.  No GPU needed."""
    from rrl_hip import build, _lib
    build.build_lib()
    fn = getattr(_lib.load(), entry)
    pair = entry != "rrl_knn3_self_workspace_bytes"
    for shape, before in SCRATCH_BYTES_BEFORE[entry].items():
        dims = shape if len(shape) == 3 or not pair else shape + shape[1:]  # (B, n): both clouds of n points
        now = int(fn(*dims))
        print(entry, dims, now, "before", before)
        assert 0 < now <= before, (entry, dims, now, before)
        assert now % 256 == 0
        for at in range(len(dims)):
            bad = list(dims)
            bad[at] = -1
            assert fn(*bad) == 0, (entry, bad)
    # an empty batch and empty clouds are legal sizes, and were no larger either: 768, 512, 768 bytes
    empty = int(fn(*([0] * (3 if pair else 2))))
    before = {"rrl_chamfer_workspace_bytes": 768, "rrl_knn3_self_workspace_bytes": 512, "rrl_knn_workspace_bytes": 768}[entry]
    assert 0 < empty <= before and empty % 256 == 0, (entry, empty, before)
