"""CPU-side checks of the ragged Chamfer distance (include/rrl.h rrl_chamfer_tree_fwd_counted / rrl_chamfer_bwd_counted):
what the two entries refuse and with which code -- on the host, with fake pointers that are never dereferenced --, the
ValueErrors of the Python layer before anything touches a GPU, rrl_hip.ragged.pack_points, and that the inputs of
tests/test_gpu_ragged_chamfer.py (tests/ragged_chamfer_cases.py) have unambiguous first-occurrence minima."""
import ctypes

import numpy as np
import pytest
import torch

import pose_refs as PR
import ragged_chamfer_cases as CC

FAKE = ctypes.c_void_p(256)
BIG = 1 << 50
E_ARG, E_WS = -1, -3


@pytest.fixture(scope="module")
def lib():
    from rrl_hip import _lib, build
    build.build_lib()
    return _lib.load()


FWD_ARGS = ("x", "y", "count_x", "count_y", "ws", "ws_bytes", "best_x", "best_y", "values", "value", "B", "N", "M", "order_x", "order_y")
BWD_ARGS = ("x", "y", "best_x", "best_y", "grad_values", "count_x", "count_y", "gx", "gy", "B", "N", "M")
BASE = dict(x=FAKE, y=FAKE, count_x=FAKE, count_y=FAKE, ws=FAKE, ws_bytes=BIG, best_x=FAKE, best_y=FAKE, values=FAKE, value=FAKE,
            grad_values=FAKE, gx=FAKE, gy=FAKE, B=2, N=130, M=200, order_x=None, order_y=None)
CAP1 = "sort capacity + 1"

# (entry, what is wrong, overrides, code)
REFUSALS = [("fwd", f"null {k}", {k: None}, E_ARG) for k in ("x", "y", "ws", "best_x", "best_y", "values")]
REFUSALS += [
    ("fwd", "only count_x", dict(count_y=None), E_ARG),
    ("fwd", "only count_y", dict(count_x=None), E_ARG),
    ("fwd", "only order_x", dict(order_x=FAKE), E_ARG),
    ("fwd", "only order_y", dict(order_y=FAKE), E_ARG),
    ("fwd", "B = 0 (the backward: a no-op, below)", dict(B=0), E_ARG),
    ("fwd", "negative B", dict(B=-1), E_ARG),
    ("fwd", "negative N", dict(N=-5), E_ARG),
    ("fwd", "negative M", dict(M=-1), E_ARG),
    ("fwd", "B > 32767", dict(B=32768), E_ARG),
    ("fwd", "N = 0", dict(N=0), E_ARG),
    ("fwd", "M = 0", dict(M=0), E_ARG),
    ("fwd", "N beyond the sort capacity", dict(N=CAP1), E_ARG),
    ("fwd", "M beyond the sort capacity", dict(M=CAP1), E_ARG),
    ("fwd", "short workspace", dict(ws_bytes=4096), E_WS),
    ("fwd", "short workspace (0)", dict(ws_bytes=0), E_WS),
    # two at once: RRL_E_ARG before RRL_E_WS
    ("fwd", "null x + short workspace", dict(x=None, ws_bytes=0), E_ARG),
    ("fwd", "one count + short workspace", dict(count_x=None, ws_bytes=0), E_ARG),
    ("fwd", "one order + short workspace", dict(order_y=FAKE, ws_bytes=0), E_ARG),
    ("fwd", "capacity + short workspace", dict(M=CAP1, ws_bytes=0), E_ARG),
    ("fwd", "B > 32767 + short workspace", dict(B=40000, ws_bytes=0), E_ARG),
]
REFUSALS += [("bwd", f"null {k}", {k: None}, E_ARG) for k in ("x", "y", "best_x", "best_y", "grad_values")]
REFUSALS += [
    ("bwd", "only count_x", dict(count_y=None), E_ARG),
    ("bwd", "only count_y", dict(count_x=None), E_ARG),
    ("bwd", "negative B", dict(B=-1), E_ARG),
    ("bwd", "negative N", dict(N=-1), E_ARG),
    ("bwd", "negative M", dict(M=-7), E_ARG),
    ("bwd", "B > 32767", dict(B=32768), E_ARG),
    ("bwd", "N = 0", dict(N=0), E_ARG),
    ("bwd", "M = 0", dict(M=0), E_ARG),
    ("bwd", "N beyond the sort capacity", dict(N=CAP1), E_ARG),
    ("bwd", "M beyond the sort capacity", dict(M=CAP1), E_ARG),
]


def _call(lib, entry, over):
    kw = dict(BASE, **over)
    for k in ("N", "M"):
        if kw[k] == CAP1:
            kw[k] = lib.rrl_sort_capacity() + 1
    if entry == "fwd":
        return lib.rrl_chamfer_tree_fwd_counted(*[kw[k] for k in FWD_ARGS], None)
    return lib.rrl_chamfer_bwd_counted(*[kw[k] for k in BWD_ARGS], None)


@pytest.mark.parametrize("entry,what,over,code", REFUSALS, ids=[f"{e}-{w}" for e, w, _, _ in REFUSALS])
def test_refusals_before_any_launch(lib, entry, what, over, code):
    assert _call(lib, entry, over) == code, (entry, what)


def test_the_accepted_shapes_reach_the_workspace_check(lib):
    """The table's base call is valid but for its workspace: with 0 bytes it ends at RRL_E_WS, so every RRL_E_ARG row above
    is refused for the one thing it changes.  NULL value, both counts NULL and both orders given are accepted too; the
    workspace is the uniform entries' (rrl_chamfer_workspace_bytes)."""
    need = lib.rrl_chamfer_workspace_bytes(BASE["B"], BASE["N"], BASE["M"])
    assert need > 0
    for over in (dict(), dict(value=None), dict(count_x=None, count_y=None), dict(order_x=FAKE, order_y=FAKE)):
        assert _call(lib, "fwd", dict(over, ws_bytes=need - 1)) == E_WS, over
    assert _call(lib, "bwd", dict(B=0)) == 0  # no sample: nothing to do, as rrl_chamfer_bwd


def test_entries_in_the_header_and_the_binding(lib):
    from rrl_hip import _lib
    assert len(_lib._SIGS["rrl_chamfer_tree_fwd_counted"]) == len(FWD_ARGS) + 1
    assert len(_lib._SIGS["rrl_chamfer_bwd_counted"]) == len(BWD_ARGS) + 1


def test_python_layer_refuses_before_anything_touches_a_gpu():
    import loss
    from rrl_hip import ops
    x, y = torch.zeros(2, 8, 3), torch.zeros(2, 12, 3)
    for fn in (ops.chamfer, loss.chamfer_dist):
        with pytest.raises(ValueError, match="counts_x and counts_y come together"):
            fn(x, y, counts_x=[8, 8])
        with pytest.raises(ValueError, match="counts_x and counts_y come together"):
            fn(x, y, counts_y=[8, 8], per_sample=True)
        with pytest.raises(ValueError, match="one per sample"):
            fn(x, y, counts_x=[8, 8, 8], counts_y=[12, 12])
        with pytest.raises(ValueError, match="integers"):
            fn(x, y, counts_x=torch.tensor([8.0, 8.0]), counts_y=[12, 12])
        with pytest.raises(ValueError, match=r"\[0, 12\]"):
            fn(x, y, counts_x=[8, 8], counts_y=[12, 13])
        with pytest.raises(ValueError, match=r"\[0, 8\]"):
            fn(x, y, counts_x=torch.tensor([-1, 8]), counts_y=[12, 12])
    cap = ops.sort_capacity()
    big = torch.zeros(1, 1, 3).expand(1, cap + 1, 3)  # (a view: no memory behind the capacity + 1 rows)
    for kw in (dict(counts_x=[4], counts_y=[1]), dict(per_sample=True)):
        with pytest.raises(ValueError, match=r"ops\.chamfer\(x\[b:b\+1"):
            ops.chamfer(big, torch.zeros(1, 4, 3), **kw)
        with pytest.raises(ValueError, match="no ragged brute-force kernel"):
            loss.chamfer_dist(torch.zeros(1, 4, 3), big, **kw)
    with pytest.raises(ValueError, match="order_x and order_y come together"):
        ops.chamfer(x, y, torch.zeros(2, 64, dtype=torch.int32), counts_x=[8, 8], counts_y=[12, 12])
    # check_counts itself: a float tensor, a wrong length, a count above the capacity
    with pytest.raises(ValueError, match="integers"):
        ops.check_counts(torch.tensor([1.5, 2.0]), 2, 8, None, "counts_x")
    with pytest.raises(ValueError, match="one per sample"):
        ops.check_counts([1], 2, 8, None, "counts_x")
    with pytest.raises(ValueError, match=r"\[0, 8\]"):
        ops.check_counts([1, 9], 2, 8, None, "counts_x")
    # the advice of the ragged loss states now names the one-call form
    assert "ops.chamfer(" in ops._RAGGED_CHAMFER and "counts_x=" in ops._RAGGED_CHAMFER and "counts_y=" in ops._RAGGED_CHAMFER


def test_pack_points():
    from rrl_hip import ragged
    rng = np.random.default_rng(7)
    clouds = [rng.standard_normal((n, 3)).astype(np.float32) for n in (5, 0, 130, 64)]
    pts, cnt = ragged.pack_points(clouds, fill=float("nan"))
    assert pts.shape == (4, 130, 3) and pts.dtype == torch.float32 and cnt.dtype == torch.int32 and cnt.tolist() == [5, 0, 130, 64]
    for b, c in enumerate(clouds):
        np.testing.assert_array_equal(pts[b, :len(c)].numpy(), c)
        assert bool(torch.isnan(pts[b, len(c):]).all())
    pts2, cnt2 = ragged.pack_points([torch.from_numpy(c) for c in clouds], capacity=200, multiple=64)
    assert pts2.shape == (4, 256, 3) and float(pts2[0, 5:].abs().max()) == 0.0 and cnt2.tolist() == cnt.tolist()
    with pytest.raises(ValueError, match="pack_points: capacity"):
        ragged.pack_points(clouds, capacity=100)


def _assert_unambiguous(oracle, x, y, cx, cy, what):
    """Per sample on the truncated pair: the nearest neighbours are the same in float32 (the kernels' arithmetic) and in
    float64, and they are the oracle's -- first occurrence included; its minima are the float32 evaluation's bits."""
    for b in range(len(cx)):
        if cx[b] == 0 or cy[b] == 0:
            continue
        xs, ys = x[b:b + 1, :cx[b]], y[b:b + 1, :cy[b]]
        assert np.isfinite(xs).all() and np.isfinite(ys).all()
        ix32, iy32, _ = PR.chamfer_nearest(xs, ys, np.float32)
        ix64, iy64, _ = PR.chamfer_nearest(xs, ys, np.float64)
        np.testing.assert_array_equal(ix32, ix64, err_msg=f"{what} sample {b}")
        np.testing.assert_array_equal(iy32, iy64, err_msg=f"{what} sample {b}")
        mx, ax, my, ay = oracle.chamfer_parts(xs[0], ys[0])
        np.testing.assert_array_equal(ax, ix64[0])
        np.testing.assert_array_equal(ay, iy64[0])
        d = xs[0][:, None, :] - ys[0][None, :, :]
        d = d * d
        d2 = (d[..., 0] + d[..., 1]) + d[..., 2]
        assert d2.dtype == np.float32
        np.testing.assert_array_equal(mx.view(np.uint32), d2.min(1).view(np.uint32))
        np.testing.assert_array_equal(my.view(np.uint32), d2.min(0).view(np.uint32))


@pytest.mark.parametrize("name", sorted(CC.FLOAT_CASES))
def test_float_cases_have_unambiguous_minima(oracle, name):
    x, y, cx, cy = CC.float_case(name, "decoy")
    _assert_unambiguous(oracle, x, y, cx, cy, name)
    seed, B, N, M, _, _ = CC.FLOAT_CASES[name]
    assert x.shape == (B, N, 3) and y.shape == (B, M, 3) and max(cx) <= N and max(cy) <= M
    # the present rows do not depend on the filler; a decoy is a present point of the OTHER cloud, at distance zero
    for filler in CC.FILLERS:
        x2, y2, _, _ = CC.float_case(name, filler)
        for b in range(B):
            np.testing.assert_array_equal(x2[b, :cx[b]], x[b, :cx[b]])
            np.testing.assert_array_equal(y2[b, :cy[b]], y[b, :cy[b]])
            if filler == "nan":
                assert np.isnan(x2[b, cx[b]:]).all() and np.isnan(y2[b, cy[b]:]).all()
    for b in range(B):
        if cx[b] and cy[b]:
            for row in x[b, cx[b]:]:
                assert (y[b, :cy[b]] == row).all(1).any()
            for row in y[b, cy[b]:]:
                assert (x[b, :cx[b]] == row).all(1).any()
    parts, vals, value = CC.reference(oracle, x, y, cx, cy)
    assert all((p is None) == (cx[b] == 0 or cy[b] == 0) for b, p in enumerate(parts))
    assert np.isfinite(vals).all() and np.isfinite(value) and all((v > 0) == (p is not None) for v, p in zip(vals, parts))


def test_nan_case_is_what_it_says(oracle):
    """Apart from its one present NaN row the case is unambiguous; sample 0 has no NaN at all; torch's minima on the truncated
    pairs: sample 1's y -> x minima are all NaN (a NaN in the target cloud), of its x -> y minima only query 17."""
    x, y, cx, cy = CC.nan_case()
    assert np.isfinite(x[0]).all() and np.isfinite(y[0]).all() and cx[0] == x.shape[1] and cy[0] == y.shape[1]
    assert np.argwhere(np.isnan(x[1, :cx[1]])).tolist() == [[17, 1]] and np.isfinite(y[1, :cy[1]]).all()
    assert np.isnan(x[1, cx[1]]).any() and np.isnan(x[1, 150]).any() and np.isnan(y[1, cy[1]]).any() and np.isnan(y[1, 149]).any()
    _assert_unambiguous(oracle, x, y, [cx[0], 0], [cy[0], 0], "nan case, sample 0")
    keep = np.arange(cx[1]) != 17
    _assert_unambiguous(oracle, x[1:2, :cx[1]][:, keep], y[1:2], [cx[1] - 1], [cy[1]], "nan case, sample 1 without row 17")
    xt, yt = torch.from_numpy(x[1, :cx[1]]), torch.from_numpy(y[1, :cy[1]])
    d = ((xt[:, None, :] - yt[None, :, :]) ** 2).sum(-1)
    assert torch.isnan(d.min(1).values).nonzero().flatten().tolist() == [17] and bool(torch.isnan(d.min(0).values).all())


def test_backward_cases(oracle):
    """The integer case is exact: every scale 2 g / (cx + cy) is a power of two on both routes and the coordinates are small
    integers.  The float case's nearest-neighbour lists are the same in float32 and float64 (checked above), every present
    point has a contribution and some have more than two."""
    seed, B, N, M, cx, cy = CC.BACKWARD_INT
    tot = sum(a + b for a, b in zip(cx, cy))
    assert tot == 1024
    for b in range(B):
        for g in (CC.BACKWARD_INT_UPSTREAM[b], CC.BACKWARD_INT_SCALAR * (cx[b] + cy[b]) / tot):
            sc = PR.chamfer_scale(1, cx[b], cy[b], g)
            assert sc != 0 and np.log2(abs(sc)) == int(np.log2(abs(sc))) and float(np.float32(g)) == g
    x, y = PR.chamfer_int_case(seed, B, N, M)
    assert np.abs(x).max() <= 8 and np.abs(y).max() <= 8 and (x == np.round(x)).all()
    x, y, cx, cy = CC.float_case("backward_float")
    for b in range(len(cx)):
        ix, iy, _ = PR.chamfer_nearest(x[b:b + 1, :cx[b]], y[b:b + 1, :cy[b]], np.float64)
        r = PR.chamfer_backward_reference(x[b:b + 1, :cx[b]], y[b:b + 1, :cy[b]], ix, iy, CC.BACKWARD_FLOAT_UPSTREAM[b])
        assert np.all(r["ax"] > 0) and np.all(r["ay"] > 0) and max(r["kx"].max(), r["ky"].max()) > 2
