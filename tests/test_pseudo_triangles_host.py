"""CPU-side checks of the device-side pseudo-triangle builder (include/rrl.h rrl_fps_counted, rrl_knn3_counted, rrl_knn3_self;
rrl_hip.neighbors.pseudo_triangles / knn3_self): the symbols exist, every entry refuses bad arguments on the host with the
documented code (fake pointers: nothing is launched), the Python layer refuses host-side mistakes before any launch, and
the numpy twin of the counted semantics (tests/neigh_refs.py) reproduces the reference's recorded Sample_neighs rows."""
import ctypes

import numpy as np
import pytest
import torch

import neigh_refs as NR
import prep_refs as PF
from conftest import load_golden

FAKE = ctypes.c_void_p(256)
BIG = 1 << 50
E_ARG, E_WS = -1, -3


@pytest.fixture(scope="module")
def lib():
    from rrl_hip import _lib
    return _lib.load()


def test_new_symbols_are_exported_and_declared(lib):
    from rrl_hip import neighbors
    import loss
    for name in ("pseudo_triangles", "knn3_self"):
        assert callable(getattr(neighbors, name)) and callable(getattr(loss, name))
    assert neighbors.TREE_MIN_POINTS is None or neighbors.TREE_MIN_POINTS >= 3
    assert int(lib.rrl_knn3_self_workspace_bytes(2, 1000)) > 0
    assert int(lib.rrl_knn3_self_workspace_bytes(2, 5000)) > int(lib.rrl_knn3_self_workspace_bytes(2, 1000))


# entry -> argument names in order (stream is always NULL); one valid call each, rows override
BASE = dict(pts=FAKE, counts=None, start=FAKE, out=FAKE, out_counts=None, scratch=FAKE, query=FAKE, qcounts=None, nn=FAKE,
            tri=None, tri_counts=None, ws=FAKE, ws_bytes=BIG, B=2, n=1000, S=100)
ARGS = {
    "rrl_fps_counted": ("pts", "counts", "start", "out", "out_counts", "scratch", "B", "n", "S"),
    "rrl_knn3_counted": ("pts", "counts", "query", "qcounts", "nn", "tri", "tri_counts", "B", "n", "S"),
    "rrl_knn3_self": ("pts", "counts", "ws", "ws_bytes", "nn", "tri", "tri_counts", "B", "n"),
}
CAP1 = "sort capacity + 1"
REFUSALS = [
    ("rrl_fps_counted", dict(pts=None), E_ARG), ("rrl_fps_counted", dict(start=None), E_ARG),
    ("rrl_fps_counted", dict(out=None), E_ARG), ("rrl_fps_counted", dict(scratch=None), E_ARG),
    ("rrl_fps_counted", dict(B=-1), E_ARG), ("rrl_fps_counted", dict(n=0), E_ARG), ("rrl_fps_counted", dict(n=-5), E_ARG),
    ("rrl_fps_counted", dict(S=-1), E_ARG), ("rrl_fps_counted", dict(S=1001), E_ARG),
    ("rrl_knn3_counted", dict(pts=None), E_ARG), ("rrl_knn3_counted", dict(nn=None), E_ARG),
    ("rrl_knn3_counted", dict(B=-1), E_ARG), ("rrl_knn3_counted", dict(n=0), E_ARG), ("rrl_knn3_counted", dict(S=-1), E_ARG),
    ("rrl_knn3_counted", dict(query=None, S=1001), E_ARG),  # row order: query q is point q
    ("rrl_knn3_self", dict(pts=None), E_ARG), ("rrl_knn3_self", dict(ws=None), E_ARG), ("rrl_knn3_self", dict(nn=None), E_ARG),
    ("rrl_knn3_self", dict(B=-1), E_ARG), ("rrl_knn3_self", dict(n=0), E_ARG), ("rrl_knn3_self", dict(n=-1), E_ARG),
    ("rrl_knn3_self", dict(n=CAP1), E_ARG), ("rrl_knn3_self", dict(ws_bytes=0), E_WS),
    ("rrl_knn3_self", dict(ws_bytes="one short"), E_WS), ("rrl_knn3_self", dict(n=5000, ws_bytes="one short"), E_WS),
]


@pytest.mark.parametrize("entry, over, code", REFUSALS, ids=[f"{e}-{'-'.join(f'{k}={v}' for k, v in o.items())}" for e, o, _ in REFUSALS])
def test_entries_refuse_on_the_host(lib, entry, over, code):
    """Fake pointers: a call that got past its validation would fault the process, so the code alone proves no launch."""
    a = dict(BASE, **over)
    if a["n"] == CAP1:
        a["n"] = int(lib.rrl_sort_capacity()) + 1
    if a["ws_bytes"] == "one short":
        a["ws_bytes"] = int(lib.rrl_knn3_self_workspace_bytes(a["B"], a["n"])) - 1
    assert getattr(lib, entry)(*[a[k] for k in ARGS[entry]], None) == code


def test_empty_calls_launch_nothing(lib):
    """B = 0 is a valid, empty call of every entry (fake pointers: it must not launch)."""
    for entry in ARGS:
        a = dict(BASE, B=0)
        assert getattr(lib, entry)(*[a[k] for k in ARGS[entry]], None) == 0


# ----------------------------------------------------------------------------------------------------------------- Python
@pytest.fixture
def no_launch(monkeypatch):
    """rrl_hip.neighbors with its launcher replaced: reaching it fails the test (test_prep_refs_host.py's fixture)."""
    from rrl_hip import neighbors

    def reached(*a, **k):
        pytest.fail(f"a launch was reached: {a[1] if len(a) > 1 else a}")
    monkeypatch.setattr(neighbors, "_run", reached)
    return neighbors


@pytest.mark.parametrize("start", [[-1, 0], [0, 50], [2 ** 31, 0], [0], [0, 1, 2]])
def test_pseudo_triangles_refuses_a_host_start_outside_the_cloud(no_launch, start):
    with pytest.raises(ValueError, match="start"):
        no_launch.pseudo_triangles(torch.zeros(2, 50, 3), 10, start=torch.tensor(start))


def test_pseudo_triangles_refuses_a_host_start_outside_its_samples_count(no_launch):
    with pytest.raises(ValueError, match="start"):
        no_launch.pseudo_triangles(torch.zeros(2, 50, 3), 10, counts=[50, 20], start=torch.tensor([49, 20]))


@pytest.mark.parametrize("counts", [[51, 3], [-1, 3], [3], [3.0, 4.0], [[3, 4]]])
def test_host_counts_outside_the_capacity_are_refused(no_launch, counts):
    pts = torch.zeros(2, 50, 3)
    with pytest.raises(ValueError, match="counts"):
        no_launch.pseudo_triangles(pts, counts=counts)
    with pytest.raises(ValueError, match="counts"):
        no_launch.pseudo_triangles(pts, 10, counts=counts)
    with pytest.raises(ValueError, match="counts"):
        no_launch.knn3_self(pts, counts=counts)


@pytest.mark.parametrize("query", [[[0, 50]], [[-1, 3]], [[2 ** 31 + 1, 3]]])
def test_knn3_counted_refuses_a_host_query_outside_the_cloud(no_launch, query):
    with pytest.raises(ValueError, match="query_idx"):
        no_launch.knn3_counted(torch.zeros(1, 50, 3), torch.tensor(query))


def test_knn3_counted_refuses_a_host_query_outside_its_samples_count(no_launch):
    with pytest.raises(ValueError, match="query_idx"):
        no_launch.knn3_counted(torch.zeros(1, 50, 3), torch.tensor([[0, 20]]), counts=[20])


@pytest.mark.parametrize("n", [1, 2])
def test_fewer_than_three_points_are_refused(no_launch, n):
    pts = torch.zeros(1, n, 3)
    for call in (lambda: no_launch.pseudo_triangles(pts), lambda: no_launch.pseudo_triangles(pts, 1),
                 lambda: no_launch.knn3_self(pts), lambda: no_launch.knn3_self(pts, method="tree")):
        with pytest.raises(ValueError, match="3 points"):
            call()


def test_unknown_method_and_misplaced_arguments_are_refused(no_launch):
    pts = torch.zeros(1, 50, 3)
    with pytest.raises(ValueError, match="method"):
        no_launch.pseudo_triangles(pts, method="kdtree")
    with pytest.raises(ValueError, match="method"):
        no_launch.knn3_self(pts, method="")
    with pytest.raises(ValueError, match="tree"):
        no_launch.pseudo_triangles(pts, 10, method="tree")  # given queries take brute force
    with pytest.raises(ValueError, match="start"):
        no_launch.pseudo_triangles(pts, start=torch.tensor([0]))
    with pytest.raises(ValueError, match="points"):
        no_launch.pseudo_triangles(torch.zeros(50, 3))


# ----------------------------------------------------------------------------------------------------------------- the twin
@pytest.mark.parametrize("seed, S, key", [(77, 900, "full"), (78, 300, "sub")])
def test_counted_twin_reproduces_the_reference_sample_neighs(seed, S, key):
    """tests/golden/sample_neighs.npz with counts = the full size, the seeds of test_prep_refs_host.py: the same rows, bit
    for bit -- and the same again when the cloud sits inside a larger capacity whose tail is NaN."""
    g = load_golden("sample_neighs.npz")
    pts = g["points"]
    torch.manual_seed(seed)
    start = [int(torch.randint(0, len(pts), (1,)))]
    r = NR.pseudo_triangles_ref(pts[None], counts=[len(pts)], num_sample=S, start=start)
    assert r["tri_counts"].tolist() == [S] and r["tri"].shape == (1, S, 9)
    np.testing.assert_array_equal(r["tri"].reshape(-1, 3).view(np.uint32), g[key].view(np.uint32))
    cap = np.full((1, len(pts) + 37, 3), np.nan, np.float32)
    cap[0, :len(pts)] = pts
    r2 = NR.pseudo_triangles_ref(cap, counts=[len(pts)], num_sample=S, start=start)
    np.testing.assert_array_equal(r2["tri"].view(np.uint32), r["tri"].view(np.uint32))
    np.testing.assert_array_equal(r2["idx"], r["idx"])


def test_counted_twin_semantics():
    """S_b = min(S, n_b), zero rows beyond, tri_counts 0 below three points; without a sampler every row in row order."""
    pts = PF.gaussian_cloud(5, 4, 40)
    counts = [40, 7, 3, 2]
    r = NR.pseudo_triangles_ref(pts, counts=counts, num_sample=10, start=[3, 6, 0, 1])
    assert r["fps_counts"].tolist() == [10, 7, 3, 2] and r["tri_counts"].tolist() == [10, 7, 3, 0]
    for b, (nb, sb) in enumerate(zip(counts, r["tri_counts"])):
        assert not r["tri"][b, sb:].any() and not r["nn"][b, sb:].any() and not r["idx"][b, r["fps_counts"][b]:].any()
        if sb:
            assert r["nn"][b, :sb].max() < nb
            np.testing.assert_array_equal(r["nn"][b, :sb], PF.knn3_ref(pts[b, :nb], r["idx"][b, :sb]))
    assert sorted(r["nn"][2, 0].tolist()) == [0, 1, 2]
    full = NR.pseudo_triangles_ref(pts, counts=counts)
    assert full["tri_counts"].tolist() == [40, 7, 3, 0] and full["tri"].shape == (4, 40, 9)
    np.testing.assert_array_equal(full["nn"][1, :7], PF.knn3_ref(pts[1, :7], np.arange(7)))
    np.testing.assert_array_equal(full["tri"][1, :7, :3], pts[1, :7])  # no duplicates: every point is its own nearest
    assert not full["tri"][1, 7:].any() and not full["tri"][3].any()
