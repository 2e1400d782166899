"""CPU-side checks of the batched registration loop (include/rrl.h rrl_se3_adam_step_batch / rrl_register_epoch,
rrl_hip/register.py): what the two entries refuse and with which code -- fake pointers, no GPU: every refusal happens on the
host before the first launch, in the documented order RRL_E_ARG, RRL_E_RANGE, RRL_E_WS --, the ValueErrors of PairRegistration that need no GPU, and the
learning-rate schedule of PairRegistration.run against the demo's adjust_learning_rate."""
import ctypes
import importlib

import pytest
import torch

FAKE = ctypes.c_void_p(256)
BIG = 1 << 50
E_ARG, E_WS = -1, -3
CAP1 = "sort capacity + 1"

# rrl_se3_adam_step_batch: one valid call; a row overrides one or two of these
STEP_ARGS = ("xi", "gR", "gT", "m", "v", "state", "lr", "gate", "gate_stride", "b1", "b2", "eps", "R", "T", "gxi", "loss", "value",
             "table", "cursor", "nrows", "row", "aabb_rows", "row_stride", "count1", "N", "box", "B")
STEP_BASE = dict({k: FAKE for k in STEP_ARGS}, gate_stride=4, b1=0.9, b2=0.999, eps=1e-8, nrows=16, row_stride=16, N=300, B=3)
STEP = [
    ("null pointer (xi)", dict(xi=None), E_ARG),
    ("null pointer (m)", dict(m=None), E_ARG),
    ("null pointer (v)", dict(v=None), E_ARG),
    ("null pointer (state)", dict(state=None), E_ARG),
    ("null pointer (lr)", dict(lr=None), E_ARG),
    ("null pointer (R)", dict(R=None), E_ARG),
    ("null pointer (T)", dict(T=None), E_ARG),
    ("negative batch", dict(B=-1), E_ARG),
    ("a box without rows", dict(aabb_rows=None), E_ARG),
    ("a box over no capacity", dict(N=0), E_ARG),
    ("a box whose samples' rows overlap", dict(row_stride=8), E_ARG),
    ("negative gate stride", dict(gate_stride=-4), E_ARG),
    ("negative batch + null pointer", dict(B=-1, T=None), E_ARG),
    ("an empty batch + a box without rows", dict(B=0, aabb_rows=None), E_ARG),
    ("an empty batch is valid: no launch", dict(B=0), 0),
    ("an empty batch without the optional pointers", dict(B=0, gR=None, gT=None, gate=None, gxi=None, loss=None, value=None,
                                                          table=None, cursor=None, row=None, aabb_rows=None, count1=None,
                                                          box=None), 0),
]

# rrl_register_epoch: the struct's integer fields of one valid call (every pointer FAKE, both workspaces huge); a row
# overrides fields; "opts" is a dict of rrl_opts fields, "monitor" = False clears the monitor's pointers
EPOCH_INTS = dict(B=3, N=300, M=300, L=2048, rounds=10, transpose_r=0, ws_bytes=BIG, cham_ws_bytes=BIG, table_rows=16)
NO_MONITOR = dict(value=None)
RAGGED = dict(count1=512, count2=512)
EPOCH = [
    ("null struct", dict(args=None), E_ARG),
    ("a struct too short", dict(struct_bytes=64), E_ARG),
    ("a struct one field short", dict(struct_bytes="sizeof - 8"), E_ARG),
    ("empty batch", dict(B=0), E_ARG),
    ("negative batch", dict(B=-1), E_ARG),
    ("negative size", dict(N=-1), E_ARG),
    ("empty target", dict(M=0), E_ARG),
    ("no lines", dict(L=0), E_ARG),
    ("no sampler rounds", dict(rounds=0), E_ARG),
    ("a sampler without its radius", dict(radius=None), E_ARG),
    ("a sampler without its target box", dict(box2=None), E_ARG),
    ("a sampler whose ballots are misaligned", dict(tile_counts=260), E_ARG),
    ("multi-pose", dict(B=4, opts=dict(problems=2)), E_ARG),
    ("line counts: the sampler owns the line set", dict(opts=dict(nlines=512)), E_ARG),
    ("the monitor on a ragged batch", dict(opts=RAGGED), E_ARG),
    ("the monitor on a ragged source alone", dict(opts=dict(count1=512)), E_ARG),
    ("the monitor without its scratch", dict(cham_ws=None), E_ARG),
    ("the monitor without its pooled mean", dict(cham_mean=None), E_ARG),
    ("the monitor beyond the sort capacity", dict(N=CAP1), E_ARG),
    ("null pointer (xi)", dict(xi=None), E_ARG),
    ("null pointer (lr)", dict(lr=None), E_ARG),
    ("null pointer (box1)", dict(box1=None), E_ARG),
    ("null pointer of the step (src_tri)", dict(src_tri=None), E_ARG),
    ("null pointer of the step (lines)", dict(lines=None), E_ARG),
    ("null pointer of the step (ws)", dict(ws=None), E_ARG),
    ("the step's refusal: ragged beyond the sort capacity", dict(N=CAP1, opts=RAGGED, **NO_MONITOR), E_ARG),
    ("the step's refusal: L = 2^24", dict(L=1 << 24, **NO_MONITOR), E_ARG),
    ("short workspace", dict(ws_bytes=4096), E_WS),
    ("short workspace, ragged, no monitor", dict(ws_bytes=0, opts=RAGGED, **NO_MONITOR), E_WS),
    ("short Chamfer workspace", dict(cham_ws_bytes=64), E_WS),
    # given lines (rng_state NULL): the sampler's fields are not looked at -- the call gets as far as the workspace check
    ("given lines need no rounds", dict(rng_state=None, rounds=0, radius=None, box2=None, ws_bytes=0), E_WS),
    # invalid in two ways: RRL_E_ARG before RRL_E_WS
    ("multi-pose + short workspace", dict(B=4, opts=dict(problems=2), ws_bytes=0), E_ARG),
    ("the monitor on a ragged batch + short workspace", dict(opts=RAGGED, ws_bytes=0), E_ARG),
    ("null pointer + short workspace", dict(m=None, ws_bytes=0), E_ARG),
    ("no sampler rounds + short Chamfer workspace", dict(rounds=0, cham_ws_bytes=0), E_ARG),
    ("the step's null pointer + short workspace", dict(grad_loss=None, ws_bytes=0), E_ARG),
    ("line counts + short workspace", dict(opts=dict(nlines=512), ws_bytes=0), E_ARG),
    ("short struct + everything else", dict(struct_bytes=8, B=-1, ws_bytes=0), E_ARG),
]


@pytest.fixture(scope="module")
def lib():
    from rrl_hip import _lib, build
    build.build_lib()
    return _lib.load()


def call_step(lib, over):
    v = dict(STEP_BASE, **over)
    return lib.rrl_se3_adam_step_batch(*[v[k] for k in STEP_ARGS], None)


def call_epoch(lib, over):
    from rrl_hip import _lib
    over = dict(over)
    if "args" in over:
        return lib.rrl_register_epoch(None, None)
    cap1 = lib.rrl_sort_capacity() + 1
    a = _lib.RegisterEpochArgs()
    for name, kind in _lib.RegisterEpochArgs._fields_:
        if kind is ctypes.c_void_p and name != "opts":
            setattr(a, name, 256)
    a.struct_bytes = ctypes.sizeof(_lib.RegisterEpochArgs)
    a.b1, a.b2, a.eps = 0.9, 0.999, 1e-8
    for k, v in EPOCH_INTS.items():
        setattr(a, k, v)
    opts = _lib.Opts(**over.pop("opts")) if "opts" in over else None
    if opts is not None:
        a.opts = ctypes.addressof(opts)
    for k, v in over.items():
        if v == "sizeof - 8":
            v = ctypes.sizeof(_lib.RegisterEpochArgs) - 8
        setattr(a, k, cap1 if v is CAP1 else v)
    return lib.rrl_register_epoch(ctypes.byref(a), None)


def test_the_tables_cover_the_documented_codes():
    assert len({r[0] for r in STEP}) == len(STEP) and len({r[0] for r in EPOCH}) == len(EPOCH)
    assert {r[2] for r in STEP} == {E_ARG, 0} and {r[2] for r in EPOCH} == {E_ARG, E_WS}
    assert sum(" + " in r[0] for r in EPOCH) >= 6  # calls invalid in two ways: the documented order


@pytest.mark.parametrize("row", STEP, ids=lambda r: r[0])
def test_the_batched_pose_step_refuses_before_any_launch(lib, row):
    _, over, code = row
    assert call_step(lib, over) == code


@pytest.mark.parametrize("row", EPOCH, ids=lambda r: r[0])
def test_the_batched_epoch_refuses_before_its_first_launch(lib, row):
    _, over, code = row
    assert call_epoch(lib, over) == code


def test_pair_registration_refuses_with_the_alternative(lib):
    """The monitor together with counts, and clouds beyond ops.sort_capacity(): ValueError before anything touches a GPU."""
    from rrl_hip import ops, register
    tri = torch.zeros(2, 64, 9)
    with pytest.raises(ValueError, match=r"ops\.chamfer\(.*counts_x=.*per_sample=True"):
        register.PairRegistration(tri, tri, 2048, counts1=[64, 30], counts2=[64, 64], monitor=True)
    with pytest.raises(ValueError, match=r"ops\.chamfer"):
        register.PairRegistration(tri, tri, 2048, counts2=[64, 64], monitor=True)
    big = torch.zeros(1, 1, 9).expand(1, ops.sort_capacity() + 1, 9)  # (no memory behind it)
    with pytest.raises(ValueError, match=r"sort_capacity.*RegistrationStep"):
        register.PairRegistration(big, tri[:1], 2048)
    with pytest.raises(ValueError, match=r"sort_capacity"):
        register.register_pairs(tri[:1], big, 2048, n_epoch=1)
    with pytest.raises(ValueError, match="same B"):
        register.PairRegistration(tri, tri[:1], 2048)


def test_the_schedule_of_run_is_the_demos(lib):
    """PairRegistration.run for epochs 0 .. 2001 installs exactly the rates the demo's adjust_learning_rate installs (halved
    at epochs 0, 1000 and 2000), and writes lr [B] only when the rate changes."""
    from rrl_hip import register
    demo = importlib.import_module("test_demo_optimized_Lie_Algebra")

    class Optimizer:
        param_groups = [{'lr': register.DEMO_LR}]

    want, lr = [], register.DEMO_LR
    for epoch in range(2002):
        lr = demo.adjust_learning_rate(Optimizer, epoch, lr)
        assert Optimizer.param_groups[0]['lr'] == lr
        want.append(lr)

    class Filled:
        writes = []

        def fill_(self, value):
            self.writes.append(value)

    reg = object.__new__(register.PairRegistration)  # (no GPU: the schedule is host code around one C call per epoch)
    reg.epochs, reg.lr_value, reg.lr, got = 0, register.DEMO_LR, Filled(), []

    def epoch(lr=None):
        reg.set_lr(lr)
        got.append(reg.lr_value)
        reg.epochs += 1
    reg.epoch = epoch
    reg.run(1500)
    reg.run(502)  # (a second run continues the schedule's clock)
    assert got == want
    assert Filled.writes == [want[0], want[1000], want[2000]] == [1e-2, 5e-3, 2.5e-3]
    assert [register.scheduled_lr(e, 1.0) for e in (0, 1, 999, 1000, 1001, 2000)] == [0.5, 1.0, 1.0, 0.5, 1.0, 0.5]
