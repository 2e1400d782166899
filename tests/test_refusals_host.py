"""CPU-side check of what every exported entry of the loss pipeline REFUSES, and with which code (include/rrl.h: "Refusals").

A fixed table of calls with fake pointers and no GPU: every entry validates on the host before its first launch, so none of
the pointers is dereferenced.  PARENT holds calls that are invalid in exactly one way; their expected codes are the ones the
library returned BEFORE its host layer was rewritten around one call record (recorded from a build of that commit, not from
the code under test).  DOCUMENTED holds calls whose code follows from the header's text alone: calls invalid in two ways at
once (RRL_E_ARG before RRL_E_RANGE before RRL_E_WS), L = 2^24 and an unknown scan mode (RRL_E_ARG before any launch)."""
import ctypes

import pytest

FAKE = ctypes.c_void_p(256)
OTHER = ctypes.c_void_p(4096)
BIG = 1 << 50
E_ARG, E_RANGE, E_WS = -1, -2, -3

# one valid call: every row overrides one (PARENT) or two (DOCUMENTED) of these
BASE = dict(tri1=FAKE, tri2=FAKE, line=FAKE, ws=FAKE, ws_bytes=BIG, wws=FAKE, wws_bytes=BIG, loss=FAKE, src=FAKE, R=FAKE, t=FAKE,
            grad_loss=FAKE, grad_tri1=FAKE, grad_tri2=None, grad_src=None, gR=FAKE, gt=FAKE, payload=None, host_info=FAKE,
            B=2, N=64, M=64, L=2048, tr=1, s_m=1, s_n=1, e_m=5, e_n=5, pool=0, mode=3, chunk=0, tws=None, opts=None)

RANGE = ("s_m", "s_n", "e_m", "e_n")
SHAPE = ("B", "N", "M", "L")
# entry -> the names of its arguments, in order (`stream` is always NULL)
ARGS = {
    "rrl_tri_prepare": ("tri1", "tri2", "ws", "ws_bytes") + SHAPE,
    "rrl_tri_prepare_ex": ("tri1", "tri2", "ws", "ws_bytes") + SHAPE + ("opts",),
    "rrl_line_tri_scan": ("line", "ws", "ws_bytes") + SHAPE + ("mode", "chunk"),
    "rrl_line_tri_scan_ex": ("line", "ws", "ws_bytes") + SHAPE + ("mode", "chunk", "opts"),
    "rrl_line_pair_dist": ("tri1", "tri2", "line", "ws", "ws_bytes") + SHAPE + RANGE + ("pool",),
    "rrl_line_pair_dist_ex": ("tri1", "tri2", "line", "ws", "ws_bytes") + SHAPE + RANGE + ("pool", "opts"),
    "rrl_loss_reduce": ("ws", "ws_bytes", "loss") + SHAPE + RANGE + ("pool",),
    "rrl_loss_reduce_ex": ("ws", "ws_bytes", "loss") + SHAPE + RANGE + ("pool", "opts"),
    "rrl_loss_forward": ("tri1", "tri2", "line", "ws", "ws_bytes", "loss") + SHAPE + RANGE + ("pool", "mode", "chunk"),
    "rrl_loss_forward_cached": ("tri1", "tri2", "line", "ws", "ws_bytes", "loss") + SHAPE + RANGE + ("pool", "mode", "chunk", "tws"),
    "rrl_loss_forward_ex": ("tri1", "tri2", "line", "ws", "ws_bytes", "loss") + SHAPE + RANGE + ("pool", "mode", "chunk", "tws", "opts"),
    "rrl_loss_forward_info": ("tri1", "tri2", "line", "ws", "ws_bytes", "loss") + SHAPE + RANGE + ("pool", "mode", "chunk", "tws", "host_info"),
    "rrl_loss_backward": ("tri1", "tri2", "ws", "ws_bytes", "grad_loss", "grad_tri1", "grad_tri2") + SHAPE + ("pool",),
    "rrl_registration_forward": ("src", "R", "t", "tri2", "line", "ws", "ws_bytes", "loss") + SHAPE + ("tr",) + RANGE + ("mode", "chunk"),
    "rrl_registration_forward_cached": ("src", "R", "t", "tri2", "line", "ws", "ws_bytes", "loss") + SHAPE + ("tr",) + RANGE + ("mode", "chunk", "tws"),
    "rrl_registration_forward_ex": ("src", "R", "t", "tri2", "line", "ws", "ws_bytes", "loss") + SHAPE + ("tr",) + RANGE + ("mode", "chunk", "tws", "opts"),
    "rrl_registration_backward": ("src", "R", "tri2", "ws", "ws_bytes", "loss", "grad_loss", "grad_src", "gR", "gt", "payload") + SHAPE + ("tr",),
    "rrl_registration_backward_ex": ("src", "R", "tri2", "ws", "ws_bytes", "loss", "grad_loss", "grad_src", "gR", "gt", "payload") + SHAPE + ("tr", "opts"),
    "rrl_registration_step": ("src", "R", "t", "tri2", "line", "ws", "ws_bytes", "loss", "grad_loss", "gR", "gt", "payload") + SHAPE + ("tr",) + RANGE + ("mode", "chunk", "tws"),
    "rrl_registration_step_ex": ("src", "R", "t", "tri2", "line", "ws", "ws_bytes", "loss", "grad_loss", "gR", "gt", "payload") + SHAPE + ("tr",) + RANGE + ("mode", "chunk", "tws", "opts"),
    "rrl_loss_step_ex": ("tri1", "R", "t", "tri2", "line", "ws", "ws_bytes", "loss", "grad_loss", "grad_tri1", "grad_tri2") + SHAPE + ("tr",) + RANGE + ("mode", "chunk", "tws", "opts"),
    "rrl_loss_forward_wide": ("tri1", "tri2", "line", "ws", "ws_bytes", "wws", "wws_bytes", "loss") + SHAPE + RANGE + ("pool", "mode", "chunk", "opts"),
    "rrl_loss_backward_wide": ("wws", "wws_bytes", "grad_loss", "grad_tri1", "grad_tri2") + SHAPE + ("pool",),
}
CAP1 = "sort capacity + 1"  # (resolved against the library)
RAGGED = dict(count1=512)   # rrl_opts fields of a ragged batch

# (entry, what is wrong, overrides, the code the parent commit returned)
PARENT = [
    ("rrl_tri_prepare", "null pointer", dict(tri2=None), E_ARG),
    ("rrl_tri_prepare", "negative size", dict(N=-1), E_ARG),
    ("rrl_tri_prepare", "short workspace", dict(ws_bytes=0), E_WS),
    ("rrl_tri_prepare_ex", "null pointer", dict(ws=None), E_ARG),
    ("rrl_tri_prepare_ex", "negative size", dict(L=-1), E_ARG),
    ("rrl_tri_prepare_ex", "short workspace", dict(ws_bytes=4096), E_WS),
    ("rrl_tri_prepare_ex", "plan: ragged beyond the sort capacity", dict(N=CAP1, opts=RAGGED), E_ARG),
    ("rrl_line_tri_scan", "null pointer", dict(line=None), E_ARG),
    ("rrl_line_tri_scan", "negative size", dict(B=-1), E_ARG),
    ("rrl_line_tri_scan", "negative chunk", dict(chunk=-1), E_ARG),
    ("rrl_line_tri_scan", "unknown mode", dict(mode=4), E_ARG),
    ("rrl_line_tri_scan", "short workspace", dict(ws_bytes=0), E_WS),
    ("rrl_line_tri_scan_ex", "null pointer", dict(ws=None), E_ARG),
    ("rrl_line_tri_scan_ex", "negative size", dict(M=-1), E_ARG),
    ("rrl_line_tri_scan_ex", "unknown mode", dict(mode=-1), E_ARG),
    ("rrl_line_tri_scan_ex", "short workspace", dict(ws_bytes=0), E_WS),
    ("rrl_line_tri_scan_ex", "plan: ragged beyond the sort capacity", dict(M=CAP1, opts=dict(nlines=512)), E_ARG),
    ("rrl_line_pair_dist", "null pointer", dict(tri1=None), E_ARG),
    ("rrl_line_pair_dist", "negative size", dict(N=-1), E_ARG),
    ("rrl_line_pair_dist", "L = 2^24", dict(L=1 << 24), E_ARG),
    ("rrl_line_pair_dist", "bad range", dict(e_m=6), E_RANGE),
    ("rrl_line_pair_dist", "short workspace", dict(ws_bytes=0), E_WS),
    ("rrl_line_pair_dist_ex", "null pointer", dict(line=None), E_ARG),
    ("rrl_line_pair_dist_ex", "negative size", dict(L=-5), E_ARG),
    ("rrl_line_pair_dist_ex", "bad range", dict(s_n=0), E_RANGE),
    ("rrl_line_pair_dist_ex", "short workspace", dict(ws_bytes=0), E_WS),
    ("rrl_line_pair_dist_ex", "plan: ragged with pool", dict(pool=1, opts=RAGGED), E_ARG),
    ("rrl_loss_reduce", "null pointer", dict(loss=None), E_ARG),
    ("rrl_loss_reduce", "negative size", dict(M=-1), E_ARG),
    ("rrl_loss_reduce", "bad range", dict(e_n=6), E_RANGE),
    ("rrl_loss_reduce", "short workspace", dict(ws_bytes=0), E_WS),
    ("rrl_loss_reduce_ex", "null pointer", dict(ws=None), E_ARG),
    ("rrl_loss_reduce_ex", "negative size", dict(B=-2), E_ARG),
    ("rrl_loss_reduce_ex", "bad range", dict(s_m=0), E_RANGE),
    ("rrl_loss_reduce_ex", "short workspace", dict(ws_bytes=0), E_WS),
    ("rrl_loss_reduce_ex", "plan: ragged with pool", dict(pool=1, opts=RAGGED), E_ARG),
    ("rrl_loss_forward", "null pointer", dict(tri2=None), E_ARG),
    ("rrl_loss_forward", "negative size", dict(N=-1), E_ARG),
    ("rrl_loss_forward", "bad range", dict(e_m=6), E_RANGE),
    ("rrl_loss_forward", "short workspace", dict(ws_bytes=0), E_WS),
    ("rrl_loss_forward_cached", "null pointer", dict(loss=None), E_ARG),
    ("rrl_loss_forward_cached", "negative size", dict(L=-1), E_ARG),
    ("rrl_loss_forward_cached", "bad range", dict(s_m=0), E_RANGE),
    ("rrl_loss_forward_cached", "short workspace", dict(ws_bytes=0, tws=OTHER), E_WS),
    ("rrl_loss_forward_cached", "the target's workspace is this one", dict(tws=FAKE), E_ARG),
    ("rrl_loss_forward_ex", "null pointer", dict(line=None), E_ARG),
    ("rrl_loss_forward_ex", "negative size", dict(B=-1), E_ARG),
    ("rrl_loss_forward_ex", "bad range", dict(e_n=9), E_RANGE),
    ("rrl_loss_forward_ex", "short workspace", dict(ws_bytes=0), E_WS),
    ("rrl_loss_forward_ex", "plan: ragged with pool", dict(pool=1, opts=RAGGED), E_ARG),
    ("rrl_loss_forward_ex", "plan: ragged with a carried-over target", dict(tws=OTHER, opts=RAGGED), E_ARG),
    ("rrl_loss_forward_info", "null pointer", dict(host_info=None), E_ARG),
    ("rrl_loss_forward_info", "null pointer (of the forward)", dict(tri1=None), E_ARG),
    ("rrl_loss_forward_info", "negative size", dict(M=-1), E_ARG),
    ("rrl_loss_forward_info", "bad range", dict(s_n=0), E_RANGE),
    ("rrl_loss_forward_info", "short workspace", dict(ws_bytes=0), E_WS),
    ("rrl_loss_backward", "null pointer", dict(grad_loss=None), E_ARG),
    ("rrl_loss_backward", "negative size", dict(N=-1), E_ARG),
    ("rrl_loss_backward", "short workspace", dict(ws_bytes=0), E_WS),
    ("rrl_registration_forward", "null pointer", dict(R=None), E_ARG),
    ("rrl_registration_forward", "negative size", dict(N=-1), E_ARG),
    ("rrl_registration_forward", "bad range", dict(e_m=6), E_RANGE),
    ("rrl_registration_forward", "short workspace", dict(ws_bytes=0), E_WS),
    ("rrl_registration_forward_cached", "null pointer", dict(t=None), E_ARG),
    ("rrl_registration_forward_cached", "negative size", dict(B=-1), E_ARG),
    ("rrl_registration_forward_cached", "bad range", dict(s_m=0), E_RANGE),
    ("rrl_registration_forward_cached", "short workspace", dict(ws_bytes=0, tws=OTHER), E_WS),
    ("rrl_registration_forward_cached", "the target's workspace is this one", dict(tws=FAKE), E_ARG),
    ("rrl_registration_forward_ex", "null pointer", dict(src=None), E_ARG),
    ("rrl_registration_forward_ex", "negative size", dict(L=-1), E_ARG),
    ("rrl_registration_forward_ex", "bad range", dict(e_n=6), E_RANGE),
    ("rrl_registration_forward_ex", "short workspace", dict(ws_bytes=0), E_WS),
    ("rrl_registration_forward_ex", "plan: poses not a multiple of the problems", dict(B=4, opts=dict(problems=3)), E_ARG),
    ("rrl_registration_forward_ex", "plan: ragged multi-pose", dict(B=4, opts=dict(problems=2, count1=512)), E_ARG),
    ("rrl_registration_backward", "null pointer", dict(gR=None), E_ARG),
    ("rrl_registration_backward", "a payload without the loss", dict(payload=FAKE, loss=None), E_ARG),
    ("rrl_registration_backward", "negative size", dict(B=-1), E_ARG),
    ("rrl_registration_backward", "short workspace", dict(ws_bytes=0), E_WS),
    ("rrl_registration_backward_ex", "null pointer", dict(grad_loss=None), E_ARG),
    ("rrl_registration_backward_ex", "negative size", dict(B=-1), E_ARG),
    ("rrl_registration_backward_ex", "short workspace", dict(ws_bytes=0), E_WS),
    ("rrl_registration_backward_ex", "multi-pose with dL/dsrc", dict(B=4, grad_src=FAKE, opts=dict(problems=2)), E_ARG),
    ("rrl_registration_backward_ex", "ragged multi-pose", dict(B=4, opts=dict(problems=2, count1=512)), E_ARG),
    ("rrl_registration_backward_ex", "ragged beyond the sort capacity", dict(N=CAP1, opts=RAGGED), E_ARG),
    ("rrl_registration_step", "null pointer", dict(gt=None), E_ARG),
    ("rrl_registration_step", "negative size", dict(M=-1), E_ARG),
    ("rrl_registration_step", "bad range", dict(e_m=6), E_RANGE),
    ("rrl_registration_step", "short workspace", dict(ws_bytes=0), E_WS),
    ("rrl_registration_step", "the target's workspace is this one", dict(tws=FAKE), E_ARG),
    ("rrl_registration_step_ex", "null pointer", dict(grad_loss=None), E_ARG),
    ("rrl_registration_step_ex", "negative size", dict(N=-1), E_ARG),
    ("rrl_registration_step_ex", "bad range", dict(s_n=0), E_RANGE),
    ("rrl_registration_step_ex", "short workspace", dict(ws_bytes=0), E_WS),
    ("rrl_registration_step_ex", "plan: multi-pose outside scan mode cull", dict(B=4, mode=2, opts=dict(problems=2)), E_ARG),
    ("rrl_registration_step_ex", "plan: ragged multi-pose", dict(B=4, opts=dict(problems=2, nlines=512)), E_ARG),
    ("rrl_loss_step_ex", "null pointer", dict(grad_tri1=None), E_ARG),
    ("rrl_loss_step_ex", "a rotation without a translation", dict(t=None), E_ARG),
    ("rrl_loss_step_ex", "negative size", dict(L=-1), E_ARG),
    ("rrl_loss_step_ex", "bad range", dict(e_m=6), E_RANGE),
    ("rrl_loss_step_ex", "short workspace", dict(ws_bytes=0), E_WS),
    ("rrl_loss_step_ex", "plan: multi-pose without a transform", dict(B=4, R=None, t=None, opts=dict(problems=2)), E_ARG),
    ("rrl_loss_step_ex", "plan: ragged with a carried-over target", dict(tws=OTHER, opts=dict(count2=512)), E_ARG),
    ("rrl_loss_forward_wide", "null pointer", dict(wws=None), E_ARG),
    ("rrl_loss_forward_wide", "negative size", dict(N=-1), E_ARG),
    ("rrl_loss_forward_wide", "L = 2^24", dict(B=1, L=1 << 24, ws_bytes=1 << 62, wws_bytes=1 << 62), E_ARG),
    ("rrl_loss_forward_wide", "B L = 2^31", dict(B=1 << 10, L=1 << 21, ws_bytes=1 << 62, wws_bytes=1 << 62), E_ARG),
    ("rrl_loss_forward_wide", "unknown mode", dict(mode=4), E_ARG),
    ("rrl_loss_forward_wide", "bad range", dict(e_m=10), E_RANGE),
    ("rrl_loss_forward_wide", "short workspace", dict(ws_bytes=0), E_WS),
    ("rrl_loss_forward_wide", "short wide workspace", dict(wws_bytes=0), E_WS),
    ("rrl_loss_forward_wide", "ragged", dict(opts=RAGGED), E_ARG),
    ("rrl_loss_backward_wide", "null pointer", dict(grad_tri1=None), E_ARG),
    ("rrl_loss_backward_wide", "negative size", dict(B=-1), E_ARG),
    ("rrl_loss_backward_wide", "L = 2^24", dict(B=1, L=1 << 24, wws_bytes=1 << 62), E_ARG),
    ("rrl_loss_backward_wide", "short wide workspace", dict(wws_bytes=0), E_WS),
    ("rrl_demo_epoch", "null pointer", dict(args=None), E_ARG),
    ("rrl_demo_epoch", "a struct too short", dict(struct_bytes=64), E_ARG),
    ("rrl_demo_epoch", "negative size", dict(N=-1), E_ARG),
    ("rrl_demo_epoch", "no sampler rounds", dict(rounds=0), E_ARG),
    ("rrl_demo_epoch", "ragged", dict(opts=dict(nlines=512)), E_ARG),
    # (pipeline = 3: the previous epoch's launches carried this epoch's sampler, so no launch precedes the step's checks)
    ("rrl_demo_epoch", "short workspace", dict(ws_bytes=0, pipeline=3), E_WS),
]

# (entry, what is wrong, overrides, the code include/rrl.h documents)
DOCUMENTED = [
    ("rrl_loss_forward_ex", "null pointer + bad range", dict(line=None, e_m=6), E_ARG),
    ("rrl_loss_forward_ex", "bad range + short workspace", dict(e_m=6, ws_bytes=0), E_RANGE),
    ("rrl_loss_forward_ex", "negative size + short workspace", dict(N=-1, ws_bytes=0), E_ARG),
    ("rrl_registration_forward_ex", "bad range + short workspace", dict(s_m=0, ws_bytes=0), E_RANGE),
    ("rrl_registration_forward_ex", "plan refusal + short workspace", dict(B=4, opts=dict(problems=3), ws_bytes=0), E_ARG),
    ("rrl_registration_step_ex", "plan refusal + bad range", dict(B=4, opts=dict(problems=3), e_n=6), E_ARG),
    ("rrl_loss_step_ex", "bad range + short workspace", dict(e_n=6, ws_bytes=0), E_RANGE),
    ("rrl_line_pair_dist_ex", "plan refusal + bad range", dict(pool=1, opts=RAGGED, e_m=6), E_ARG),
    ("rrl_loss_reduce", "bad range + short workspace", dict(s_m=0, ws_bytes=0), E_RANGE),
    ("rrl_loss_forward_wide", "ragged + bad range", dict(opts=RAGGED, e_m=10), E_ARG),
    ("rrl_loss_forward_wide", "bad range + short workspace", dict(e_m=10, ws_bytes=0), E_RANGE),
    ("rrl_loss_forward", "L = 2^24", dict(B=1, L=1 << 24, ws_bytes=1 << 62), E_ARG),
    ("rrl_loss_forward_ex", "L = 2^24", dict(B=1, L=1 << 24, ws_bytes=1 << 62), E_ARG),
    ("rrl_registration_forward_ex", "L = 2^24", dict(B=1, L=1 << 24, ws_bytes=1 << 62), E_ARG),
    ("rrl_registration_step_ex", "L = 2^24", dict(B=1, L=1 << 24, ws_bytes=1 << 62), E_ARG),
    ("rrl_loss_step_ex", "L = 2^24", dict(B=1, L=1 << 24, ws_bytes=1 << 62), E_ARG),
    ("rrl_loss_forward_ex", "unknown mode", dict(mode=4), E_ARG),
    ("rrl_registration_forward_ex", "unknown mode", dict(mode=-1), E_ARG),
    ("rrl_registration_step_ex", "unknown mode", dict(mode=7), E_ARG),
    ("rrl_loss_step_ex", "negative chunk", dict(chunk=-1), E_ARG),
]


@pytest.fixture(scope="module")
def lib():
    from rrl_hip import _lib, build
    build.build_lib()
    return _lib.load()


def call(lib, entry, over):
    """The BASE call of `entry` with `over` applied; rrl_opts fields are given as a dict."""
    from rrl_hip import _lib
    over = dict(over)
    cap1 = lib.rrl_sort_capacity() + 1
    over = {k: (cap1 if v is CAP1 else v) for k, v in over.items()}
    opts = _lib.Opts(**over["opts"]) if isinstance(over.get("opts"), dict) else None
    if entry == "rrl_demo_epoch":
        if "args" in over:
            return lib.rrl_demo_epoch(None, None)
        a = _lib.DemoEpochArgs()
        for name, _ in _lib.DemoEpochArgs._fields_:
            if name not in ("struct_bytes", "N", "M", "L", "rounds", "transpose_r", "ws_bytes", "cham_ws_bytes", "b1", "b2", "eps",
                            "table_rows", "opts", "pipeline"):
                setattr(a, name, 256)
        a.struct_bytes, a.N, a.M, a.L, a.rounds, a.ws_bytes, a.cham_ws_bytes = ctypes.sizeof(_lib.DemoEpochArgs), 64, 64, 2048, 10, BIG, BIG
        pipeline = ctypes.c_int32(over.pop("pipeline", 0))
        a.pipeline = ctypes.addressof(pipeline)
        if opts is not None:
            a.opts = ctypes.addressof(opts)
        over.pop("opts", None)
        for k, v in over.items():
            setattr(a, k, v)
        return lib.rrl_demo_epoch(ctypes.byref(a), None)
    v = dict(BASE, **over)
    v["opts"] = ctypes.byref(opts) if opts is not None else None
    if entry.startswith("rrl_registration_step") and min(v[k] for k in SHAPE) >= 0:
        # (dL/dR, dL/dt in the workspace's GACC field, the fused op's convention: the records launch clears them, no fill here)
        from rrl_hip import ops
        gacc = FAKE.value + ops._WS.layout(*[v[k] for k in SHAPE])[1][ops._WS.index["gacc"]]
        v["gR"] = v["gR"] and ctypes.c_void_p(gacc)
        v["gt"] = v["gt"] and ctypes.c_void_p(gacc + 4 * 9 * v["B"])
    return getattr(lib, entry)(*[v[name] for name in ARGS[entry]], None)


def _id(row):
    return f"{row[0]}: {row[1]}"


def test_the_table_covers_every_entry_and_code():
    entries = {r[0] for r in PARENT}
    assert entries == set(ARGS) | {"rrl_demo_epoch"}
    assert len({_id(r) for r in PARENT + DOCUMENTED}) == len(PARENT) + len(DOCUMENTED)
    has_range = {e for e, a in ARGS.items() if "s_m" in a}
    for e in sorted(entries):
        what = {r[1] for r in PARENT if r[0] == e}
        codes = {r[3] for r in PARENT if r[0] == e}
        assert any(w.startswith("null pointer") for w in what) and "negative size" in what, e
        assert E_WS in codes and any(w.startswith("short") for w in what), e
        assert (E_RANGE in codes) == (e in has_range), e
        if e.endswith("_ex") and e != "rrl_registration_backward_ex":
            assert any(w.startswith("plan:") for w in what), e
    assert all(r[3] < 0 for r in PARENT + DOCUMENTED)


@pytest.mark.parametrize("row", PARENT, ids=_id)
def test_a_call_invalid_in_one_way_is_refused_as_before(lib, row):
    entry, _, over, code = row
    assert call(lib, entry, over) == code


@pytest.mark.parametrize("row", DOCUMENTED, ids=_id)
def test_the_documented_order_of_refusals(lib, row):
    entry, _, over, code = row
    assert call(lib, entry, over) == code
