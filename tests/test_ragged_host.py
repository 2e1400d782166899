"""CPU-side checks of ragged batches (include/rrl.h rrl_opts.count1 / count2 / nlines): the ABI, the refusals -- before any
HIP call from C, as ValueError from the Python layer --, rrl_hip.ragged's packers, and that the inputs of
tests/test_gpu_ragged.py are not vacuous (the CPU oracle, sample by sample on the truncated arrays)."""
import ctypes

import numpy as np
import pytest
import torch

import ragged_cases as RC
from conftest import load_golden


@pytest.fixture(scope="module")
def lib():
    from rrl_hip import _lib, build
    build.build_lib()
    return _lib.load()


def test_counts_in_the_header_the_binding_and_the_library(lib):
    from rrl_hip import _lib
    names = [f for f, _ in _lib.Opts._fields_]
    assert names[-3:] == ["count1", "count2", "nlines"]  # appended: a caller compiled against the shorter struct keeps the defaults
    o = _lib.Opts(count1=512, count2=1024, nlines=2048)
    assert (o.count1, o.count2, o.nlines) == (512, 1024, 2048) and o.struct_bytes == ctypes.sizeof(_lib.Opts)


def _opts(**kw):
    from rrl_hip import _lib
    return _lib.Opts(**kw)


def test_refused_combinations_return_e_arg_before_any_launch(lib):
    """Every entry validates on the host: fake pointers are never dereferenced (no GPU here)."""
    from rrl_hip import _lib
    fake = ctypes.c_void_p(256)
    big = 1 << 40
    B, N, M, L = 2, 64, 64, 128
    cnt = dict(count1=512)
    ref = ctypes.byref
    fwd = lambda o, pool=0, tws=None: lib.rrl_loss_forward_ex(fake, fake, fake, fake, big, fake, B, N, M, L, 1, 1, 5, 5, pool, 3, 0, tws, ref(o), None)  # noqa: E731
    assert fwd(_opts(**cnt), pool=1) == -1                                   # pool
    assert fwd(_opts(**cnt), tws=ctypes.c_void_p(4096)) == -1                # target_ws
    rider = _lib.ChamferRider(256, big, 256, 256, 256, 0)
    assert fwd(_opts(chamfer=ctypes.addressof(rider), nlines=512)) == -1     # the Chamfer rider
    reg = lambda o, tws=None: lib.rrl_registration_forward_ex(fake, fake, fake, fake, fake, fake, big, fake, 4, N, M, L, 1, 1, 1, 5, 5, 3, 0, tws, ref(o), None)  # noqa: E731
    assert reg(_opts(problems=2, **cnt)) == -1                               # multi-pose
    assert reg(_opts(**cnt), tws=ctypes.c_void_p(4096)) == -1
    step = lambda o: lib.rrl_registration_step_ex(fake, fake, fake, fake, fake, fake, big, fake, fake, fake, fake, None, 4, N, M, L, 1, 1, 1, 5, 5, 3, 0, None, ref(o), None)  # noqa: E731
    assert step(_opts(problems=2, nlines=512)) == -1
    lstep = lambda o, tws=None: lib.rrl_loss_step_ex(fake, fake, fake, fake, fake, fake, big, fake, fake, fake, None, 4, N, M, L, 1, 1, 1, 5, 5, 3, 0, tws, ref(o), None)  # noqa: E731
    assert lstep(_opts(problems=2, count2=512)) == -1
    assert lstep(_opts(count2=512), tws=ctypes.c_void_p(4096)) == -1
    # clouds beyond the sort capacity are not served ragged (any scan mode)
    cap = lib.rrl_sort_capacity()
    assert lib.rrl_loss_forward_ex(fake, fake, fake, fake, 1 << 50, fake, 1, cap + 1, 64, 128, 1, 1, 5, 5, 0, 0, 0, None, ref(_opts(**cnt)), None) == -1
    # the staged build and scan entries report the plan's verdict too
    huge = 1 << 50
    assert lib.rrl_tri_prepare_ex(fake, fake, fake, huge, 1, cap + 1, 64, 128, ref(_opts(**cnt)), None) == -1
    assert lib.rrl_line_tri_scan_ex(fake, fake, huge, 1, cap + 1, 64, 128, 0, 0, ref(_opts(nlines=512)), None) == -1
    assert lib.rrl_line_tri_scan_ex(fake, fake, huge, 1, 64, cap + 1, 128, 3, 0, ref(_opts(count2=512)), None) == -1
    assert lib.rrl_tri_prepare_ex(fake, fake, fake, 0, 1, cap + 1, 64, 128, ref(_opts()), None) == -3  # (no counts: judged as before)
    # the staged entries: pool
    assert lib.rrl_line_pair_dist_ex(fake, fake, fake, fake, big, B, N, M, L, 1, 1, 5, 5, 1, ref(_opts(**cnt)), None) == -1
    assert lib.rrl_loss_reduce_ex(fake, big, fake, B, N, M, L, 1, 1, 5, 5, 1, ref(_opts(**cnt)), None) == -1
    # the backward of a ragged multi-pose call
    assert lib.rrl_registration_backward_ex(fake, fake, fake, fake, big, fake, fake, None, fake, fake, None, 4, N, M, L, 1, ref(_opts(problems=2, **cnt)), None) == -1
    # the wide entries (a wide range, or a narrow one through them)
    for e in (9, 5):
        assert lib.rrl_loss_forward_wide(fake, fake, fake, fake, big, fake, big, fake, B, N, M, L, 1, 1, e, e, 0, 3, 0, ref(_opts(**cnt)), None) == -1
    # the demo epoch
    a = _lib.DemoEpochArgs()
    a.struct_bytes, a.N, a.M, a.L, a.rounds = ctypes.sizeof(_lib.DemoEpochArgs), 64, 64, 2000, 10
    o = _opts(nlines=512)
    a.opts = ctypes.addressof(o)
    assert lib.rrl_demo_epoch(ref(a), None) == -1
    # a struct too short to reach the counts keeps the defaults: the same call is then judged on its other fields alone
    # (with a workspace of 0 bytes an accepted call ends at RRL_E_WS, still before any HIP call)
    small = lambda o, pool: lib.rrl_loss_forward_ex(fake, fake, fake, fake, 0, fake, B, N, M, L, 1, 1, 5, 5, pool, 3, 0, None, ref(o), None)  # noqa: E731
    short = _opts(**cnt)
    short.struct_bytes = _lib.Opts.count1.offset
    assert small(_opts(**cnt), 1) == -1 and small(short, 1) == -3 and small(_opts(**cnt), 0) == -3


def test_python_layer_refuses_before_anything_runs():
    from rrl_hip import dist, ops
    gate = ops._ragged_gate
    gate(False, pool=True, chamfer=True, target_from=object(), wide=True, problems=3)  # not ragged: nothing to refuse
    for kw, word in ((dict(pool=True), "pool=False"), (dict(chamfer=True), r"ops\.chamfer"), (dict(target_from=object()), "scan its target"),
                     (dict(wide=True), r"1\.\.4"), (dict(problems=2), "one call after the other")):
        with pytest.raises(ValueError, match=word):
            gate(True, **kw)
    # a state left by a ragged evaluation refuses what walks its workspace at the capacities
    class _State:
        dims, ragged, target_state = (2, 8, 8, 16, 2), True, None
    for fn in (ops.chamfer_from_state, ops._chamfer_from_loss, lambda s: ops.chamfer_group_means(s, 1)):
        with pytest.raises(ValueError, match=r"ragged batch.*ops\.chamfer"):
            fn(_State())
    with pytest.raises(ValueError, match="ragged batch.*scan its target"):
        ops._target_ws(_State(), 2, 8, 8, 16)
    carried = _State()
    carried.ragged, carried.target_state = False, _State()  # ... also through a state whose target was carried over from one
    with pytest.raises(ValueError, match="ragged batch"):
        ops.chamfer_from_state(carried)
    z = torch.zeros(1, 4, 9)
    with pytest.raises(ValueError, match="line_sharded_loss"):
        dist.line_sharded_loss(z, z, torch.zeros(1, 8, 6), nlines=[8])
    # host counts are validated: range, shape, type
    with pytest.raises(ValueError, match=r"\[0, 4096\]"):
        ops.check_counts([1, 5000], 2, 4096, None, "counts1")
    with pytest.raises(ValueError, match=r"\[0, 4096\]"):
        ops.check_counts(torch.tensor([-1, 7]), 2, 4096, None, "counts2")
    with pytest.raises(ValueError, match="one per sample"):
        ops.check_counts([1, 2, 3], 2, 4096, None, "nlines")
    with pytest.raises(ValueError, match="integers"):
        ops.check_counts(torch.tensor([1.0, 2.0]), 2, 4096, None, "nlines")
    assert ops.check_counts(None, 2, 4096, None, "nlines") is None
    # the public entries gate before they touch a GPU
    pts, ln = torch.zeros(2, 8, 9), torch.zeros(2, 16, 6)
    with pytest.raises(ValueError, match="pool=False"):
        ops.intersection_loss(pts, pts, ln, pool=True, counts1=[8, 8])
    with pytest.raises(ValueError, match=r"1\.\.4"):
        ops.intersection_loss(pts, pts, ln, rng=(1, 1, 9, 9), nlines=[16, 3])
    with pytest.raises(ValueError, match=r"ops\.chamfer"):
        ops.registration_loss(pts, torch.eye(3).repeat(2, 1, 1), torch.zeros(2, 3), pts, ln, chamfer=True, counts2=[8, 1])
    with pytest.raises(ValueError, match="one call after the other"):
        ops.registration_loss(pts, torch.eye(3).repeat(4, 1, 1), torch.zeros(4, 3), pts, ln, counts2=[8, 1])


def test_pack_round_trips():
    from rrl_hip import ragged
    import pre_dataloader as P
    rng = np.random.default_rng(5)
    clouds = [rng.standard_normal((n, 9)).astype(np.float32) for n in (5, 0, 130, 64)]
    tri, cnt = ragged.pack_clouds(clouds, fill=float("nan"))
    assert tri.shape == (4, 130, 9) and tri.dtype == torch.float32 and cnt.dtype == torch.int32 and cnt.tolist() == [5, 0, 130, 64]
    for b, c in enumerate(clouds):
        np.testing.assert_array_equal(tri[b, :len(c)].numpy(), c)
        assert bool(torch.isnan(tri[b, len(c):]).all())
    tri2, _ = ragged.pack_clouds([torch.from_numpy(c) for c in clouds], capacity=200, multiple=64)
    assert tri2.shape == (4, 256, 9) and float(tri2[0, 5:].abs().max()) == 0.0
    with pytest.raises(ValueError, match="capacity"):
        ragged.pack_clouds(clouds, capacity=100)
    lines = [rng.standard_normal((n, 6)).astype(np.float32) for n in (7, 3, 0, 9)]
    ln, nl = ragged.pack_lines(lines, capacity=12)
    assert ln.shape == (4, 12, 6) and nl.tolist() == [7, 3, 0, 9]
    np.testing.assert_array_equal(ln[3, :9].numpy(), lines[3])
    # kd_order rows of dataset items -> rows the contract accepts: (B, 64 ceil(cap / 64)), head = a permutation of [0, count)
    rows = [P.kd_order(c[:, :3]) if len(c) else np.zeros(0, np.int32) for c in clouds]
    order = ragged.pack_orders(rows, cnt, capacity=tri.shape[1])
    assert order.shape == (4, 192) and order.dtype == torch.int32
    for b, c in enumerate(clouds):
        assert sorted(order[b, :len(c)].tolist()) == list(range(len(c))) and int(order[b, len(c):].abs().max() if len(c) < 192 else 0) == 0
    with pytest.raises(ValueError, match="permutation"):
        ragged.pack_orders([[0, 0, 1]], [3])
    with pytest.raises(ValueError, match="permutation"):
        ragged.pack_orders([[0, 1]], [3])


@pytest.mark.parametrize("name", sorted(RC.BATCHES))
def test_synthetic_ragged_batches_are_not_vacuous(oracle, name):
    """Per sample, on the truncated arrays: at least one populated bucket and no NaN for every sample that has triangles
    in both clouds and more than one line -- the 1-triangle and the 63 / 64 / 65-triangle ones included."""
    capN, capM, capL, ss = RC.batch(oracle, name)
    populated = 0
    for b, s in enumerate(ss):
        assert len(s["tri1"]) <= capN and len(s["tri2"]) <= capM and len(s["lines"]) <= capL
        if len(s["tri1"]) == 0 or len(s["tri2"]) == 0 or len(s["lines"]) == 0:
            continue
        ref = oracle.loss(s["tri1"], s["tri2"], s["lines"], want_grad=False)
        assert not ref["nan"], (name, b)
        if not RC.may_be_empty(s):
            assert ref["n_buckets"] > 0 and ref["n_selected"] > 0, (name, b, RC.BATCHES[name][3][b])
            populated += 1
    assert populated >= len(ss) // 2
    if name == "BASE":  # the figures quoted in DESIGN ("Ragged batches")
        sel = [oracle.loss(s["tri1"], s["tri2"], s["lines"], want_grad=False) for s in ss]
        assert all(232 <= r["n_selected"] <= 359 and 4 <= r["n_buckets"] <= 16 for r in sel)
    rows = RC.BATCHES[name][3]
    c = {n for n, _, _ in rows} | {m for _, m, _ in rows}
    assert {0, 1, 63, 64, 65}.issubset(c) or name == "BASE"


def test_step_and_graph_inputs_are_not_vacuous(oracle):
    """BASE's clouds with uneven line counts and the lines of another sample per step (tests 3 .. 6 of the GPU file), and the
    counts a captured step is replayed with."""
    sets = [RC.step_samples(oracle, it) for it in range(3)] + [RC.step_samples(oracle, 0, c1, nl) for c1, nl in RC.GRAPH_VARIANTS]
    sets.append(RC.step_samples(oracle, 0, counts2=RC.HALF_C2))
    for ss in sets:
        for b, s in enumerate(ss):
            ref = oracle.loss(s["tri1"], s["tri2"], s["lines"], want_grad=False)
            assert not ref["nan"]
            assert RC.may_be_empty(s) or (ref["n_buckets"] > 0 and ref["n_selected"] > 0), b


def test_the_references_pairs_as_one_batch_are_not_vacuous(oracle):
    """Test 1 of the GPU file: only loss_edge_allmiss is empty."""
    for name in RC.REF_NAMES:
        g = load_golden(f"loss_{name}.npz")
        assert g["tri1"].shape[0] <= 2048 and g["tri2"].shape[0] <= 2048 and g["lines"].shape[0] <= 3000
        ref = oracle.loss(g["tri1"], g["tri2"], g["lines"], want_grad=False)
        if name == "edge_allmiss":
            assert ref["loss"] is None and ref["n_buckets"] == 0
        else:
            assert not bool(g["r0_empty"]) and ref["n_buckets"] > 0 and not ref["nan"]
