"""How the loss pipeline treats the memory it computes in (include/rrl.h RRL_WS_TABLE / RRL_WW_TABLE, csrc/rrl_ws.h).

Every route of the table below runs on GUARDED memory of ARBITRARY prior content: while a route runs, every device buffer
rrl_hip.ops allocates -- workspaces, the Chamfer / order / normal-equation scratches, losses, gradients, keys, orders,
payloads -- is the middle of a buffer with 4096 bytes of a fill pattern on either side, pre-filled with the same pattern
(tests/ws_guard.py Arena: the allocators of rrl_hip.ops are replaced for the duration of the route, so the call records the
steps bake at construction point into guarded memory too; no seam in ops.py, no route that cannot be injected into).

  route          entries                                                                         shape (B, N, M, L)
  fused          rrl_loss_forward_ex strict / lazy / auto / cull x pool 0 / 1; rrl_loss_backward  2, 70, 130, 129
                 default and deterministic (GFIX), both gradients
  staged         rrl_tri_prepare_ex, rrl_line_tri_scan_ex, rrl_line_pair_dist_ex,                 2, 70, 130, 129
                 rrl_loss_reduce_ex, pool 0 / 1
  two_tiles      fused forward, the plan's reduce and the forced exchange reduce                  3, 512, 512, 1025
  wide_sort      fused forward cold and prepared (HISTG)                                          2, 4097, 300, 600
  prepared       order1 / order2; target_kept second call; target_from                            2, 512, 512, 1025
  chained        ops.LossStep x 3 (plain, chained, chained), lean and fat (RRL_CULL_FAT)           2, 1200, 1000, 3100 / 2500
  registration   rrl_registration_forward_ex / _backward_ex (TRI1, G1, RPART, GACC) default and   2, 200, 180, 600
                 deterministic; rrl_registration_step_ex x 2 with the payload
  ragged         counts1 / counts2 / nlines: one sample empty, one full, one partial: fused        3, 130, 130, 257
                 forward + deterministic backward, ops.LossStep x 2
  wide_range     rrl_loss_forward_wide + rrl_loss_backward_wide at (1, 1, 9, 9)                    1, 1024, 2048, 3000
  chamfer        the rider (make_opts(chamfer=)), rrl_chamfer_from_loss, rrl_chamfer_group_means   2, 512, 512, 1025
  multi_pose     rrl_registration_step_ex with rrl_opts.problems (2 poses x 2 problems)            4, 200, 180, 600
  readers        rrl_pose_normal_eq (its `part` scratch), rrl_shard_payload                        2, 200, 180, 600
  order          rrl_cloud_order, _points, _counted                                               n = 65, 4097

Checks, per route (test_route) -- one printed line each (pytest -s) with the fills run and the gap bytes looked at:
  (a) containment: both bands of EVERY allocation still hold the fill; every byte of the workspaces that belongs to no
      field (ws_guard.gaps: the padding behind each field, the tail) still holds it -- inside the three spans the host code
      clears with one fill across field boundaries (csrc/rrl_ws.h: the first six fields, MHIST .. MSUM, GACC up to KJC;
      wide: STATUS + NSEL) the padding may also read zero.
  (b) any prior content: fills 0x00, 0xFF (NaN floats, -1 integers) and 0xA5; "dirty": a complete evaluation of the same
      route on OTHER clouds and lines of the same shape first, then the route on the buffers that evaluation left
      (Arena.recycle).  Every output and every documented result field is bit-identical to the run on zeroed memory; the
      outputs that are "zeroed then accumulated" are pre-filled with the same garbage (0xFF: NaN).  Gradients of the default
      mode (float atomics): the fused route's and the wide route's against the float64 twin's bound
      (test_gpu_loss_stages.check_point_grad), the steps' by test_gpu_chain._assert_same; deterministic ones bit for bit.
      test_dirty_pairs: chained step -> fused forward, wide -> narrow, ragged -> uniform, registration step -> staged,
      strict -> cull, each on the shape of its first member.
  (c) what a call leaves behind, after a synchronise: the words that their last user REWINDS read zero -- MCTL CURSOR, TICK1,
      TICK2, ERR, MEDRDY, BAD, CHAM_GROUP (both), CHAM_TOP of every row, every CHAIN row, MSUM, STATUS[3], the wide
      workspace's STATUS[2], [3].  The words that are CLEARED BY THE NEXT CALL's first launch may hold anything: MHIST, the
      sixteen bucket words, MEDBITS, LSUM (include/rrl.h says which is which).  Also for the empty ragged sample and for an
      evaluation with no selected line (test_no_selected_line).
  (d) the same call again on its own leftovers gives the same bits ("again").
No fill is applied between linked calls (target_kept, target_from, RRL_F_CHAINED, forward -> backward).
Each route asserts that every sample selects at least 64 lines (the empty ragged sample excepted).
"""
import numpy as np
import pytest
import torch

import ws_guard as W
from test_gpu_chain import _assert_same, _poses, _snapshot
from test_gpu_loss_stages import Worst, check_point_grad, twin_of
from test_gpu_prepared import _hits_sorted, _same_evaluation, _with_fat

pytestmark = pytest.mark.gpu
FILLS = (0x00, 0xFF, 0xA5)
DIRT_FILL = 0xA5
GL = (1.0, -0.5, 2.0, 0.25)


@pytest.fixture(scope="module")
def ops():
    from rrl_hip import _lib, ops
    _lib.load()
    assert torch.cuda.is_available()
    return ops


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_inputs = {}


def inputs(oracle, name, variant=0):
    """The device tensors of table shape `name` (ws_guard.shape_batch), made once, outside any arena."""
    key = (name, variant)
    if key not in _inputs:
        if name == "wide_range":
            from loss_cases import golden_sample
            a, b = golden_sample("loss_ref_human0.npz"), golden_sample("loss_ref_human1.npz")
            if variant:  # other clouds and lines of the same shape
                a = dict(tri1=b["tri1"], tri2=b["tri2"], lines=np.concatenate([b["lines"], b["lines"]])[:len(a["lines"])])
            bt = dict(tri1=a["tri1"][None], tri2=a["tri2"][None], lines=a["lines"][None], samples=[a], rng=(1, 1, 9, 9))
        else:
            bt = W.shape_batch(oracle, name, variant)
        d = dict(t1=cu(bt["tri1"]), t2=cu(bt["tri2"]), ln=cu(bt["lines"]), rng=bt["rng"], samples=bt["samples"])
        for k in ("counts1", "counts2", "nlines"):
            d[k] = cu(bt[k]) if k in bt else None
        _inputs[key] = d
    return _inputs[key]


def miss_lines(B, L):
    """Lines that pass far from every cloud (tests/loss_cases.py empty_sample_batch): nothing is selected."""
    return cu(np.tile(np.array([[1.0, 0, 0, 0, 50, 50]], np.float32), (B, L, 1)))


def bits(t):
    """A clone of `t` whose equality is equality of bit patterns (NaN payloads included)."""
    t = t.detach().contiguous()
    if t.dtype == torch.float32:
        t = t.view(torch.int32)
    elif t.dtype == torch.float64:
        t = t.view(torch.int64)
    return t.clone()


class Run:
    """What one evaluation of a route leaves to be checked."""

    def __init__(self):
        self.bits = {}    # name -> tensor: bit-identical whatever the memory held before
        self.twin = []    # (name, gradient (B, n, 9), cloud "1" | "2", input set): default-mode gradients held to the twin
        self.snaps = []   # (name, test_gpu_chain._snapshot): the steps, compared by _assert_same
        self.close = {}   # name -> default-mode gradient compared by _assert_same's gradient rule
        self.ws = []      # (kind, workspace tensor, (B, N, M, L, G)): gap checks
        self.ctl = []     # (name, LossState): control words
        self.wide = []    # WideStates: their STATUS[2], [3]
        self.nsel = []    # (name, selected lines per sample (tensor), samples that may be empty)

    def put(self, name, t):
        assert name not in self.bits, name
        self.bits[name] = bits(t)

    def state(self, tag, st, counts=True, status=True, nl=None, empty=()):
        """The documented results of LossState `st`: loss, MED, BCNT, BSUM, INFO, STATUS[0..2], NSEL, the selected lines as
        a set, PMAX, COUNT1 / COUNT2 and the hit sets (counts: not after a chained step, which clears them), KJ, and HS / W /
        Q / D where KJ says a line is selected and a hit slot is live.  nl: the lines each sample has (a ragged call)."""
        B, N, M, L, G = st.dims
        dev = st.ws.device
        line = torch.arange(L, device=dev)[None, :]
        live = line < (nl.clamp(0, L).long()[:, None] if nl is not None else L)
        kj = torch.where(live, st.kj, torch.zeros_like(st.kj))
        sel = kj != 0
        k, j = (kj & 15).long(), (kj >> 4).long()
        a4, a16 = torch.arange(4, device=dev), torch.arange(16, device=dev)
        m1, m2 = sel[..., None] & (a4 < k[..., None]), sel[..., None] & (a4 < j[..., None])
        for name in ("loss", "med", "bcnt", "bsum", "info", "nsel", "pmax"):
            self.put(f"{tag}.{name}", getattr(st, name))
        if status:
            self.put(f"{tag}.status", st.status[:3])
        nsel = st.nsel.clamp(0, L).long()
        self.put(f"{tag}.sel", torch.where(line < nsel[:, None], st.sel, torch.full_like(st.sel, L)).sort(-1).values)
        self.put(f"{tag}.kj", kj)
        if counts:
            for w in (1, 2):
                cnt, hit = _hits_sorted(st, w)
                self.put(f"{tag}.count{w}", torch.where(live, cnt, torch.zeros_like(cnt)))
                self.put(f"{tag}.hit{w}", torch.where(live[..., None], hit, torch.zeros_like(hit)))
        for w, m in ((1, m1), (2, m2)):
            hs, wt, q = getattr(st, f"hs{w}"), bits(getattr(st, f"w{w}")), bits(getattr(st, f"Q{w}"))
            self.put(f"{tag}.hs{w}", torch.where(m, hs, torch.full_like(hs, -1)))
            self.put(f"{tag}.w{w}", torch.where(m[..., None], wt, torch.full_like(wt, -1)))
            self.put(f"{tag}.q{w}", torch.where(m[..., None], q, torch.full_like(q, -1)))
        d = bits(st.D)
        self.put(f"{tag}.d", torch.where(sel[..., None] & (a16 < (k * j)[..., None]), d, torch.full_like(d, -1)))
        self.ws.append((0, st.ws, tuple(st.dims)))
        self.ctl.append((tag, st))
        if G == B:
            self.nsel.append((tag, st.info[:, 1].clone(), tuple(empty)))
        return st


# ---------------------------------------------------------------------------------------------------- the routes
def route_fused(ops, oracle, v, shape="levels", modes=("strict", "lazy", "auto", "cull"), backward=True):
    d, run = inputs(oracle, shape, v), Run()
    for mode in modes:
        for pool in (False, True):
            run.state(f"{mode}/pool{int(pool)}", ops.loss_forward_raw(d["t1"], d["t2"], d["ln"], d["rng"], pool=pool, mode=mode))
    if not backward:
        return run
    B = d["t1"].shape[0]
    gl = cu(np.asarray(GL[:B], np.float32))
    for det in (False, True):
        ops.set_deterministic(det)
        try:
            p1, p2 = d["t1"].clone().requires_grad_(True), d["t2"].clone().requires_grad_(True)
            loss, info, status = ops.intersection_loss(p1, p2, d["ln"], d["rng"])
            (loss * gl).sum().backward()
        finally:
            ops.set_deterministic(False)
        run.state("backward det" if det else "backward", ops.last_state())
        if det:
            run.put("det.grad1", p1.grad)
            run.put("det.grad2", p2.grad)
        else:
            run.twin += [("points1.grad", p1.grad.clone(), "1", (shape, v)), ("points2.grad", p2.grad.clone(), "2", (shape, v))]
    return run


def route_staged(ops, oracle, v, shape="levels"):
    d, run = inputs(oracle, shape, v), Run()
    for pool in (False, True):
        run.state(f"staged/pool{int(pool)}", ops.loss_forward_raw(d["t1"], d["t2"], d["ln"], d["rng"], pool=pool, staged=True))
    return run


def route_two_tiles(ops, oracle, v, shape="two_tiles"):
    d, run = inputs(oracle, shape, v), Run()
    run.state("plan", ops.loss_forward_raw(d["t1"], d["t2"], d["ln"], d["rng"]))
    xchg = run.state("xchg", ops.loss_forward_raw(d["t1"], d["t2"], d["ln"], d["rng"], opts=ops.make_opts(reduce_mode="xchg")))
    run.put("xchg.pooled", ops.loss_forward_raw(d["t1"], d["t2"], d["ln"], d["rng"], pool=True,
                                                opts=ops.make_opts(reduce_mode="xchg")).loss)
    tiles = (xchg.dims[3] + 1023) // 1024
    run.put("xchg.blkcnt", xchg.blkcnt[:xchg.dims[0] * tiles])
    return run


def route_wide_sort(ops, oracle, v, shape="wide_sort"):
    d, run = inputs(oracle, shape, v), Run()
    cold = run.state("cold", ops.loss_forward_raw(d["t1"], d["t2"], d["ln"], d["rng"]))
    o1, o2 = ops.cloud_order(d["t1"]), ops.cloud_order(d["t2"])
    prep = run.state("prepared", ops.loss_forward_raw(d["t1"], d["t2"], d["ln"], d["rng"], opts=ops.make_opts(order1=o1, order2=o2)))
    for name, idx, n in (("cold", cold.idx1, d["t1"].shape[1]), ("prepared", prep.idx1, d["t1"].shape[1])):
        run.put(f"{name}.idx1 is a permutation", idx[:, :n].sort(-1).values)  # (the order inside a grid cell is arbitrary)
    assert torch.equal(prep.idx1, o1)
    return run


def route_prepared(ops, oracle, v, shape="prepared"):
    d, run = inputs(oracle, shape, v), Run()
    o1, o2 = ops.cloud_order(d["t1"]), ops.cloud_order(d["t2"])
    st = ops.loss_forward_raw(d["t1"], d["t2"], d["ln"], d["rng"], opts=ops.make_opts(order1=o1, order2=o2))
    run.state("first", st)
    # linked calls: the kept target's records stay where the first call built them; nothing is filled in between
    moved = d["t1"] + 0.01
    ops.loss_forward_raw(moved, d["t2"], d["ln"], d["rng"], opts=ops.make_opts(order1=o1, order2=o2, target_kept=True), state=st)
    run.state("kept", st)
    run.state("target_from", ops.loss_forward_raw(d["t1"], d["t2"], d["ln"], d["rng"], target_from=st,
                                                  opts=ops.make_opts(order1=o1, order2=o2)), counts=False)
    return run


def _step_calls(ops, run, tag, step, d, n, pose=True):
    B = step.dims[0]
    for it in range(n):
        R, t = _poses(B, it) if pose else (None, None)
        out = step(R, t, d["ln"])
        run.snaps.append((f"{tag}[{it}]", _snapshot(step, out)))


def route_chained(ops, oracle, v):
    run = Run()
    for fat, shape in (("0", "chain_lean"), ("1", "chain_fat")):
        d = inputs(oracle, shape, v)
        step = ops.LossStep(d["t1"], d["t2"], d["ln"].shape[1], want_payload=True)
        fused = []

        def calls():
            for it in range(3):
                R, t = _poses(step.dims[0], it)
                run.snaps.append((f"{shape}[{it}]", _snapshot(step, step(R, t, d["ln"]))))
                fused.append(step.fused)
        _with_fat(fat, calls)
        assert fused == [False, True, True], (shape, fused)  # the second and third call ran the chained launch
        run.put(f"{shape}.payload", step.payload[:2])
        run.state(shape, step.st, counts=False, status=False)
    return run


def route_registration(ops, oracle, v, shape="registration"):
    d, run = inputs(oracle, shape, v), Run()
    B = d["t1"].shape[0]
    R, t = _poses(B, 1)
    gl = cu(np.asarray(GL[:B], np.float32))
    for det in (False, True):
        # deterministic: the direct backward (fixed-order partial sums into GACC, which the forward zeroed); default: the route
        # through G1 (d/dsrc wanted: float atomics), whose outputs are written into buffers of their own
        ops.set_deterministic(det)
        try:
            src, Rg, tg = d["t1"].clone().requires_grad_(not det), R.clone().requires_grad_(True), t.clone().requires_grad_(True)
            loss, info, status = ops.registration_loss(src, Rg, tg, d["t2"], d["ln"], d["rng"])
            (loss * gl).sum().backward()
        finally:
            ops.set_deterministic(False)
        st = run.state("autograd det" if det else "autograd", ops.last_state())
        run.put(("det" if det else "default") + ".tri1", st.tri1t)
        for name, g in (("gR", Rg.grad), ("gt", tg.grad), ("gsrc", src.grad)):
            if g is None:
                continue
            if det:
                run.put(f"det.{name}", g)
            else:
                run.close[name] = g.clone()
    step = ops.RegistrationStep(d["t1"], d["t2"], d["ln"].shape[1], want_payload=True, deterministic=True)
    for it in range(2):
        R, t = _poses(B, it)
        loss, gR, gt, pay, info = step(R, t, d["ln"], grad_loss=gl)
        for name, x in (("loss", loss), ("gR", gR), ("gt", gt), ("payload", pay), ("info", info)):
            run.put(f"step[{it}].{name}", x)
    run.state("step", step.st)
    return run


def route_ragged(ops, oracle, v, shape="ragged"):
    d, run = inputs(oracle, shape, v), Run()
    B, L = d["t1"].shape[0], d["ln"].shape[1]
    counts = dict(counts1=d["counts1"], counts2=d["counts2"], nlines=d["nlines"])
    empty = [b for b, s in enumerate(d["samples"]) if s is None]
    st = run.state("forward", ops.loss_forward_raw(d["t1"], d["t2"], d["ln"], d["rng"], opts=ops.make_opts(**counts)),
                   nl=d["nlines"], empty=empty)
    gl = cu(np.asarray(GL[:B], np.float32))
    ops.set_deterministic(True)
    try:
        p1, p2 = d["t1"].clone().requires_grad_(True), d["t2"].clone().requires_grad_(True)
        loss, info, status = ops.intersection_loss(p1, p2, d["ln"], d["rng"], **counts)
        (loss * gl).sum().backward()
    finally:
        ops.set_deterministic(False)
    run.state("backward det", ops.last_state(), nl=d["nlines"], empty=empty)
    run.put("det.grad1", p1.grad)
    run.put("det.grad2", p2.grad)
    for b in range(B):  # rows beyond a count: exactly zero
        assert not bool(p1.grad[b, int(d["counts1"][b]):].any()) and not bool(p2.grad[b, int(d["counts2"][b]):].any())
    step = ops.LossStep(d["t1"], d["t2"], L, **counts)
    _step_calls(ops, run, "step", step, d, 2, pose=False)
    run.state("step", step.st, counts=False, status=False, nl=d["nlines"], empty=empty)
    assert float(st.loss[empty[0]]) == 0.0 and int(st.info[empty[0], 0]) == 0
    return run


def route_wide_range(ops, oracle, v, shape="wide_range"):
    d, run = inputs(oracle, shape, v), Run()
    p1, p2 = d["t1"].clone().requires_grad_(True), d["t2"].clone().requires_grad_(True)
    loss, info, _ = ops.intersection_loss(p1, p2, d["ln"], d["rng"])
    (loss * GL[1]).sum().backward()
    st = ops.last_state()
    assert isinstance(st, ops.WideState) and int(st.status[0]) == 0 and int(st.status[1]) > 0  # the hit recovery had entries
    B, N, M, L, G = st.dims
    for name in ("loss", "med", "bcnt", "bsum", "info", "nsel", "status"):
        run.put(f"wide.{name}", getattr(st, name))
    nsel = st.nsel.clamp(0, L).long()
    slot = torch.arange(L, device=st.wws.device)[None, :] < nsel[:, None]
    order = torch.where(slot, st.sel, torch.full_like(st.sel, L)).sort(-1)  # slots are handed out in any order: by line
    run.put("wide.sel", order.values)
    kj = torch.gather(torch.where(slot, st.kj, torch.zeros_like(st.kj)), 1, order.indices)
    run.put("wide.kj", kj)
    a8 = torch.arange(8, device=kj.device)
    for w, cnt in ((1, (kj & 15).long()), (2, (kj >> 4).long())):
        hs = torch.gather(getattr(st, f"hs{w}"), 1, order.indices[..., None].expand(-1, -1, 8))
        run.put(f"wide.hs{w}", torch.where(a8 < cnt[..., None], hs, torch.full_like(hs, -1)))
    for w in (1, 2):
        run.put(f"scan.count{w}", getattr(st.scan, f"count{w}"))
    run.put("scan.status", st.scan.status[:3])
    run.ws += [(0, st.scan.ws, tuple(st.dims)), (1, st.wws, tuple(st.dims))]
    run.ctl.append(("wide scan", st.scan))
    run.wide.append(st)
    run.nsel.append(("wide", st.info[:, 1].clone(), ()))
    run.twin += [("points1.grad", p1.grad.clone(), "1", (shape, v)), ("points2.grad", p2.grad.clone(), "2", (shape, v))]
    return run


def route_chamfer(ops, oracle, v, shape="prepared"):
    d, run = inputs(oracle, shape, v), Run()
    loss, info, _ = ops.intersection_loss(d["t1"], d["t2"], d["ln"], d["rng"], chamfer=True)
    st = run.state("rider", ops.last_state())
    assert st.cham_ride is not None and st.cham_ride.done, "the Chamfer walk did not ride in the scan launch"
    val, bx, by = ops.chamfer_from_state(st, keys=True)
    for name, x in (("value", val), ("best_x", bx), ("best_y", by), ("means", ops.chamfer_group_means(st, 2))):
        run.put(f"rider.{name}", x)
    plain = run.state("plain", ops.loss_forward_raw(d["t1"], d["t2"], d["ln"], d["rng"]))
    ws, bx2, by2, val2 = ops._chamfer_from_loss(plain)
    for name, x in (("value", val2), ("best_x", bx2), ("best_y", by2), ("means", ops.chamfer_group_means(plain, 1))):
        run.put(f"from_loss.{name}", x)
    run.ctl.append(("after rrl_chamfer_from_loss", plain))
    return run


def route_multi_pose(ops, oracle, v, shape="registration"):
    d, run = inputs(oracle, shape, v), Run()
    Bt = d["t1"].shape[0]
    poses = [_poses(Bt, it) for it in range(2)]
    R, t = torch.cat([p[0] for p in poses]).contiguous(), torch.cat([p[1] for p in poses]).contiguous()
    o1, o2 = ops.cloud_order(d["t1"]), ops.cloud_order(d["t2"])
    for det in (False, True):
        ops.set_deterministic(det)
        try:
            loss, gR, gt, info, st = ops.registration_step_raw(d["t1"], R, t, d["t2"], d["ln"], d["rng"], order1=o1, order2=o2)
        finally:
            ops.set_deterministic(False)
        run.state("det" if det else "default", st)
        if det:
            run.put("det.gR", gR)
            run.put("det.gt", gt)
        else:
            run.close["gR"], run.close["gt"] = gR.clone(), gt.clone()
    return run


def route_readers(ops, oracle, v, shape="registration"):
    d, run = inputs(oracle, shape, v), Run()
    B = d["t1"].shape[0]
    R, t = _poses(B, 0)
    loss, info, status = ops.registration_loss(d["t1"], R, t, d["t2"], d["ln"], d["rng"])
    st = run.state("forward", ops.last_state())
    run.put("normal_eq", ops.pose_normal_eq(st, d["rng"]))
    run.put("normal_eq again", ops.pose_normal_eq(st, d["rng"]))
    run.put("payload", ops.shard_payload(loss.detach(), state=st))
    run.ctl.append(("after the readers", st))
    return run


def route_order(ops, oracle, v):
    """The order inside a grid cell is arbitrary (csrc/rrl_cull.hip: an LDS cursor), so an order is compared as what it
    promises: every row's first n (counted: counts[b]) entries a permutation, zeros behind n; that ANY such order gives the
    same evaluation is the prepared and wide_sort routes' business, whose orders are made on the same prior content."""
    run = Run()
    for shape, n in (("levels", 65), ("wide_sort", 4097)):  # the sort from the points / the records launch + wide sort
        tri = inputs(oracle, shape, v)["t1"][:, :n].contiguous()
        B = tri.shape[0]
        assert tri.shape[1] == n
        cnt = torch.tensor([n, n // 2][:B], dtype=torch.int32, device=tri.device)
        for name, order, rows in ((f"{n}.tri", ops.cloud_order(tri), [n] * B),
                                  (f"{n}.points", ops.cloud_order(tri[..., :3].contiguous()), [n] * B),
                                  (f"{n}.counted", ops.cloud_order(tri, counts=cnt), cnt.tolist())):
            assert order.dtype == torch.int32 and tuple(order.shape) == (B, (n + 63) // 64 * 64)
            for b, k in enumerate(rows):
                run.put(f"{name}[{b}] sorted", order[b, :k].sort().values)
                assert torch.equal(run.bits[f"{name}[{b}] sorted"], torch.arange(k, dtype=torch.int32, device=tri.device)), (name, b)
            if "counted" not in name:
                run.put(f"{name} tail", order[:, n:])
                assert not bool(order[:, n:].any()), name
    assert any(k.startswith("65.") for k in run.bits) and any(k.startswith("4097.") for k in run.bits)
    return run


ROUTES = dict(fused=route_fused, staged=route_staged, two_tiles=route_two_tiles, wide_sort=route_wide_sort,
              prepared=route_prepared, chained=route_chained, registration=route_registration, ragged=route_ragged,
              wide_range=route_wide_range, chamfer=route_chamfer, multi_pose=route_multi_pose, readers=route_readers,
              order=route_order)


# ---------------------------------------------------------------------------------------------------- the checks
def rewound_words():
    from rrl_hip import _lib
    c = _lib.CONSTANTS
    return [c["RRL_MCTL_CURSOR"], c["RRL_MCTL_TICK1"], c["RRL_MCTL_TICK2"], c["RRL_MCTL_ERR"], c["RRL_MCTL_MEDRDY"],
            c["RRL_MCTL_BAD"], c["RRL_MCTL_CHAM_GROUP"], c["RRL_MCTL_CHAM_GROUP"] + 1, c["RRL_MCTL_CHAM_TOP"]]


def check_left_behind(run, what):
    """(c): the rewound words read zero once the stream is idle."""
    words = rewound_words()
    for tag, st in run.ctl:
        mctl = st.mctl[:, words]
        assert not bool(mctl.any()), (what, tag, "MCTL words not rewound", mctl.tolist())
        assert not bool(st.chain.any()), (what, tag, "CHAIN words not rewound", st.chain.tolist())
        assert not bool(st.msum.any()), (what, tag, "MSUM not rewound")
        assert int(st.status[3]) == 0, (what, tag, "STATUS[3] (the rigid backward's ticket) not rewound")
    for st in run.wide:
        assert not bool(st.status[2:].any()), (what, "the wide workspace's STATUS[2], [3]")


def check_contained(arena, run, what):
    """(a): the bands of every allocation, the gaps of every workspace; returns (allocations, gap bytes)."""
    n = arena.assert_bands(what)
    gap_bytes = 0
    for kind, ws, dims in run.ws:
        arena.record_of(ws)  # the workspace itself is a guarded allocation
        gap_bytes += W.check_gaps(ws, kind, dims, arena.fill)
    return n, gap_bytes


def check_selects(run, what):
    for tag, nsel, empty in run.nsel:
        for b, k in enumerate(nsel.tolist()):
            assert k == 0 if b in empty else k >= 64, (what, tag, b, k)


def grad_close(a, b, what):
    """test_gpu_chain._assert_same's rule for gradients that differ by the order of float atomics."""
    z = torch.zeros(1)
    same = dict(loss=z, info=z, kj=z, hs1=z, hs2=z, med=z, bsum=z, bcnt=z)
    _assert_same(dict(same, grad=a), dict(same, grad=b), what)


def check_twin(oracle, run, what, worst):
    for name, g, cloud, (shape, v) in run.twin:
        d = inputs(oracle, shape, v)
        g = g.cpu().numpy()
        for b, s in enumerate(d["samples"]):
            gl = GL[1] if shape == "wide_range" else GL[b]
            s1, s2, r64, r32 = twin_of(oracle, s["tri1"], s["tri2"], s["lines"], d["rng"])
            tri, other = (s["tri1"], s["tri2"]) if cloud == "1" else (s["tri2"], s["tri1"])
            check_point_grad(f"{what} {name}[{b}]", tri, g[b], (r64, r32), cloud, gl, worst, False, other)


def check_same(clean, run, what):
    """(b), (d): `run` against the run on zeroed memory."""
    assert sorted(clean.bits) == sorted(run.bits)
    for name, want in clean.bits.items():
        assert torch.equal(want, run.bits[name]), (what, name)
    assert [n for n, _ in clean.snaps] == [n for n, _ in run.snaps]
    for (name, a), (_, b) in zip(clean.snaps, run.snaps):
        _assert_same(a, b, (what, name))
    assert sorted(clean.close) == sorted(run.close)
    for name in clean.close:
        grad_close(clean.close[name], run.close[name], (what, name))


def evaluate(ops, fill, *calls, recycle=True):
    """The calls one after the other in one arena of `fill`, the buffers of each handed to the next as they are; the last
    call's Run and the arena, with the stream idle."""
    arena = W.Arena(fill)
    run = None
    try:
        with arena.patch(ops):
            for i, call in enumerate(calls):
                run = call()
                if i + 1 < len(calls):
                    torch.cuda.synchronize()
                    assert arena.recycle() > 0
        torch.cuda.synchronize()
    except Exception as e:  # a device fault ends the session: nothing more is started on a device that has faulted
        if any(w in str(e).lower() for w in ("hip error", "illegal memory", "memory access fault", "hiperror")):
            pytest.exit(f"GPU fault in the workspace tests: {e}", returncode=3)
        raise
    if len(calls) > 1:
        assert arena.reused > 0, "the second evaluation did not get the first one's buffers"
    return arena, run


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_route(ops, oracle, route):
    fn = ROUTES[route]
    worst = Worst(f"workspace / {route}")
    clean, gaps_seen, allocs, ran = None, 0, 0, []
    plans = [(f"0x{f:02X}", f, [lambda: fn(ops, oracle, 0)]) for f in FILLS]
    plans.append(("dirty", DIRT_FILL, [lambda: fn(ops, oracle, 1), lambda: fn(ops, oracle, 0)]))
    plans.append(("again", DIRT_FILL, [lambda: fn(ops, oracle, 0), lambda: fn(ops, oracle, 0)]))
    for label, fill, calls in plans:
        what = f"{route} / {label}"
        arena, run = evaluate(ops, fill, *calls)
        n, g = check_contained(arena, run, what)
        check_left_behind(run, what)
        check_selects(run, what)
        check_twin(oracle, run, what, worst)
        if clean is None:
            clean = run
        else:
            check_same(clean, run, what)
        allocs, gaps_seen = allocs + n, gaps_seen + g
        ran.append(label)
    print(f"\n[workspace] {route}: fills {' '.join(ran)}; {allocs} guarded allocations, {gaps_seen} gap bytes checked, "
          f"{len(clean.bits)} outputs / fields bit-identical, {len(clean.snaps)} step snapshots, {len(clean.twin) + len(clean.close)} "
          f"default-mode gradients")
    if worst.v:
        worst.show()


# (dirt, the route under test, the shape both run at): the dirt is a complete evaluation of ANOTHER route on the same buffers
def _pairs(ops, oracle):
    def chained_dirt():
        d = inputs(oracle, "chain_lean", 1)
        step = ops.LossStep(d["t1"], d["t2"], d["ln"].shape[1])
        run = Run()
        _step_calls(ops, run, "dirt", step, d, 3)
        assert step.fused
        run.state("dirt", step.st, counts=False, status=False)
        return run

    def registration_dirt():
        d = inputs(oracle, "registration", 1)
        step = ops.RegistrationStep(d["t1"], d["t2"], d["ln"].shape[1], want_payload=True)
        for it in range(2):
            step(*_poses(step.dims[0], it), d["ln"])
        run = Run()
        run.state("dirt", step.st)
        return run

    return {
        "chained step -> fused forward": (chained_dirt, lambda: route_fused(ops, oracle, 0, "chain_lean", ("cull",), False)),
        "wide -> narrow": (lambda: route_wide_range(ops, oracle, 1),
                           lambda: _narrow_on_wide_shape(ops, oracle)),
        "ragged -> uniform": (lambda: route_ragged(ops, oracle, 1), lambda: _uniform_on_ragged_shape(ops, oracle)),
        "registration step -> staged": (registration_dirt, lambda: route_staged(ops, oracle, 0, "registration")),
        "strict -> cull": (lambda: route_fused(ops, oracle, 1, "levels", ("strict",), False),
                           lambda: route_fused(ops, oracle, 0, "levels", ("cull",), False)),
    }


def _narrow_on_wide_shape(ops, oracle):
    d, run = inputs(oracle, "wide_range", 0), Run()
    run.state("narrow", ops.loss_forward_raw(d["t1"], d["t2"], d["ln"], W.NARROW))
    return run


def _uniform_on_ragged_shape(ops, oracle):
    """The full sample of the ragged batch in every row: a uniform batch at the ragged batch's capacities."""
    d, run = inputs(oracle, "ragged", 0), Run()
    full = [b for b in range(d["t1"].shape[0]) if int(d["nlines"][b]) == d["ln"].shape[1] and int(d["counts1"][b]) == d["t1"].shape[1]
            and int(d["counts2"][b]) == d["t2"].shape[1]][0]
    rep = lambda x: x[full:full + 1].expand_as(x).contiguous()  # noqa: E731
    run.state("uniform", ops.loss_forward_raw(rep(d["t1"]), rep(d["t2"]), rep(d["ln"]), d["rng"]))
    return run


PAIRS = ["chained step -> fused forward", "wide -> narrow", "ragged -> uniform", "registration step -> staged", "strict -> cull"]


@pytest.mark.parametrize("pair", PAIRS)
def test_dirty_pairs(ops, oracle, pair):
    """(b) dirty, other route: the second route on the buffers a complete evaluation of the first one left equals the second
    route on zeroed memory, stays contained and leaves its words rewound."""
    dirt, call = _pairs(ops, oracle)[pair]
    _, clean = evaluate(ops, 0x00, call)
    arena, run = evaluate(ops, DIRT_FILL, dirt, call)
    n, g = check_contained(arena, run, pair)
    check_left_behind(run, pair)
    check_selects(run, pair)
    check_same(clean, run, pair)
    print(f"\n[workspace] {pair}: fills 0x00 dirty; {n} guarded allocations ({arena.reused} reused dirty), {g} gap bytes checked, "
          f"{len(clean.bits)} outputs / fields bit-identical")


@pytest.mark.parametrize("fill", FILLS)
def test_no_selected_line(ops, oracle, fill):
    """(c) for evaluations that select nothing: the fused forward (single-tile reduce), the two-tile shape (tail kernel and
    exchange reduce) and a chained step leave loss 0, INFO 0 and every rewound word at zero on any prior content -- and the
    next, ordinary call on those buffers gives the bits of a call on zeroed memory."""
    def nothing():
        run = Run()
        for shape, kw in (("levels", {}), ("two_tiles", {}), ("two_tiles", dict(opts=ops.make_opts(reduce_mode="xchg")))):
            d = inputs(oracle, shape, 0)
            st = ops.loss_forward_raw(d["t1"], d["t2"], miss_lines(*d["ln"].shape[:2]), d["rng"], **kw)
            run.ctl.append((f"{shape} {sorted(kw)}", st))
            run.ws.append((0, st.ws, tuple(st.dims)))
            run.put(f"{shape}{sorted(kw)}.loss", st.loss)
            run.put(f"{shape}{sorted(kw)}.info", st.info)
        d = inputs(oracle, "chain_lean", 0)
        step = ops.LossStep(d["t1"], d["t2"], d["ln"].shape[1])
        for it in range(2):
            loss, grad, info = step(*_poses(step.dims[0], it), miss_lines(*d["ln"].shape[:2]))
        run.ctl.append(("chained", step.st))
        run.ws.append((0, step.st.ws, tuple(step.st.dims)))
        run.put("chained.loss", loss)
        run.put("chained.info", info)
        run.put("chained.grad", grad)
        return run

    def after():
        run = route_fused(ops, oracle, 0, "levels", ("cull",), False)
        more = route_two_tiles(ops, oracle, 0)
        run.bits.update({"two_tiles " + k: x for k, x in more.bits.items()})
        run.ws += more.ws
        run.ctl += more.ctl
        return run

    arena, run = evaluate(ops, fill, nothing)
    check_contained(arena, run, "nothing selected")
    check_left_behind(run, "nothing selected")
    for name, x in run.bits.items():
        assert not bool(x.any()), (name, "loss, INFO and gradient of an evaluation that selects nothing are zero")
    _, clean = evaluate(ops, 0x00, after)
    arena, run = evaluate(ops, fill, nothing, after)
    n, g = check_contained(arena, run, "after nothing selected")
    check_left_behind(run, "after nothing selected")
    check_same(clean, run, "after nothing selected")
    print(f"\n[workspace] nothing selected, fill 0x{fill:02X}: {n} guarded allocations, {g} gap bytes checked")


def test_same_evaluation_helper_agrees(ops, oracle):
    """The comparison this file makes field by field contains test_gpu_prepared._same_evaluation's: on 0xFF memory the cull
    forward equals the strict one by that helper too (both in guarded memory)."""
    d = inputs(oracle, "levels", 0)
    arena = W.Arena(0xFF)
    with arena.patch(ops):
        strict = ops.loss_forward_raw(d["t1"], d["t2"], d["ln"], d["rng"], mode="strict")
        cull = ops.loss_forward_raw(d["t1"], d["t2"], d["ln"], d["rng"], mode="cull")
    torch.cuda.synchronize()
    _same_evaluation(strict, cull)
    arena.assert_bands("strict / cull")
