"""The batched registration loop on the GPU (include/rrl.h rrl_se3_adam_step_batch / rrl_register_epoch,
rrl_hip/register.py), all by EQUALITY of bits against entries that existed before it: the batched pose
step against B calls of ops.se3_adam_step on slices, the one-call epoch against the composed epoch (rrl_sample_lines_rng +
RegistrationStep + one ops.se3_adam_step per sample), samples against the same samples in another batch, the first epoch of
a ragged batch against the B = 1 call on the truncated tensors, and register_pairs end to end.

Every comparison of poses runs with deterministic=True: the direct backward's float atomics differ from run to run by
themselves (tests/test_gpu_harness.py test_demo_epoch_chamfer_rides_in_the_scans_launch does the same)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_CAP = 300            # capacity of the small shapes: two partial rows of 256
COUNTS = [300, 257, 64, 0]  # rows: two, two, one, none -> (+inf, -inf)
L_SMALL = 2048


@pytest.fixture(scope="module")
def ops():
    from rrl_hip import _lib, ops
    _lib.load()
    assert torch.cuda.is_available()
    return ops


@pytest.fixture(scope="module")
def register():
    from rrl_hip import register
    return register


def same(a, b, what):
    """Bit for bit (NaN == NaN, -0 != +0)."""
    a, b = a.detach().contiguous().cpu(), b.detach().contiguous().cpu()
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    ia, ib = (a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else (a, b)
    bad = (ia != ib).nonzero()
    assert len(bad) == 0, f"{what}: {len(bad)} entries differ, first at {bad[0].tolist()}: {a[tuple(bad[0])]} != {b[tuple(bad[0])]}"


# ------------------------------------------------------------------------------------- 1: the batched pose step
def pose_inputs(B, seed, counts):
    """Everything one pose step reads and writes, per sample: gates mixing 0 and positive, rates and step counts (0, 5, 999)
    that differ per sample, cursors on both sides of the table's end, partial rows that are NaN beyond a sample's count."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    nblk, rows = (N_CAP + 255) // 256, 4
    t = dict(xi=0.3 * r(B, 6), gR=r(B, 3, 3), gT=r(B, 3), m=0.1 * r(B, 6), v=0.01 * r(B, 6).abs(),
             state=torch.tensor([[0.0, 5.0, 999.0][b % 3] for b in range(B)]),
             lr=torch.tensor([2e-2 / (1 + b % 5) for b in range(B)]),
             gate=torch.tensor([[(b * 7 + 1) % 3 * 11, 5, 6, 0] for b in range(B)], dtype=torch.int32),
             loss=r(B), value=r(B).abs(), table=torch.zeros(rows, B, 3), cursor=torch.tensor([b % (rows + 2) for b in range(B)]),
             row=torch.zeros(B, 3), R=torch.zeros(B, 3, 3), T=torch.zeros(B, 3), gxi=torch.zeros(B, 6), box=torch.zeros(B, 6))
    t["xi"][0, :3] = 0.0  # (the Taylor branch of the exponential)
    apart = r(B, nblk, 8)
    if counts is not None:
        for b in range(B):
            apart[b, (counts[b] + 255) // 256:] = float("nan")  # rows a ragged build does not write: never read
    t["apart"] = apart
    assert B < 3 or (0 in t["gate"][:, 0].tolist() and int(t["gate"][:, 0].max()) > 0)
    return {k: x.cuda().contiguous() for k, x in t.items()}


def run_singles(ops, t, counts, lean):
    """B calls of ops.se3_adam_step on sample b's slices (views: the calls write in place)."""
    B = t["xi"].shape[0]
    for b in range(B):
        nr = (N_CAP if counts is None else counts[b]) + 255 >> 8
        table_b = t["table"][:, b].contiguous()
        kw = {}
        if not lean:
            kw = dict(table=table_b, cursor=t["cursor"][b:b + 1], row=t["row"][b])
            if nr:
                kw.update(aabb_rows=t["apart"][b, :nr], box=t["box"][b])
            else:  # the single entry refuses a box without rows; rrl_aabb_counted's value for an empty cloud
                t["box"][b] = torch.tensor([float("inf")] * 3 + [float("-inf")] * 3)
        ops.se3_adam_step(t["xi"][b], None if lean else t["gR"][b], t["gT"][b], t["m"][b], t["v"][b], t["state"][b:b + 1],
                          t["lr"][b:b + 1], t["gate"][b], t["R"][b], t["T"][b], gxi=t["gxi"][b], loss=t["loss"][b:b + 1],
                          value=t["value"][b:b + 1], **kw)
        if not lean:
            t["table"][:, b] = table_b


def run_batch(ops, t, counts, lean):
    kw = {}
    if not lean:
        kw = dict(table=t["table"], cursor=t["cursor"], row=t["row"], aabb_rows=t["apart"], capacity=N_CAP, box=t["box"],
                  counts=None if counts is None else torch.tensor(counts, dtype=torch.int32, device="cuda"))
    ops.se3_adam_step_batch(t["xi"], None if lean else t["gR"], t["gT"], t["m"], t["v"], t["state"], t["lr"], t["gate"], t["R"],
                            t["T"], gate_stride=4, gxi=t["gxi"], loss=t["loss"], value=t["value"], **kw)


@pytest.mark.parametrize("B,ragged,lean", [(1, True, False), (3, True, False), (3, False, False), (70, True, False), (3, True, True)],
                         ids=["B1", "B3", "B3-no-counts", "B70", "B3-without-gR-table-box"])
def test_batched_pose_step_equals_single_steps_on_slices(ops, B, ragged, lean):
    """xi, m, v, state, R, T, gxi, row, the table, the cursors and the box after ONE launch for B poses == after B launches
    of the single-pose kernel on the slices, bit for bit, over two consecutive steps (the second reads what the first
    wrote).  NaN sits in every partial row beyond a sample's count; lean: once without gR, the table and the box."""
    counts = [COUNTS[b % 4] for b in range(B)] if ragged else None
    one, many = pose_inputs(B, 40 + B, counts), pose_inputs(B, 40 + B, counts)
    for step in range(2):
        run_batch(ops, one, counts, lean)
        run_singles(ops, many, counts, lean)
        for k in ("xi", "m", "v", "state", "R", "T", "gxi", "row", "table", "cursor", "box"):
            same(one[k], many[k], f"B = {B}, step {step}: {k}")
    assert torch.isfinite(one["xi"]).all() and torch.isfinite(one["R"]).all()
    if not lean:
        moved = (one["gate"][:, 0] > 0).cpu()
        assert torch.equal(one["state"].cpu(), pose_inputs(B, 40 + B, counts)["state"].cpu() + 2 * moved.float())
        assert torch.equal(one["cursor"].cpu(), torch.tensor([b % 6 + 2 for b in range(B)]))
        box = one["box"].cpu()
        for b in range(B):
            if counts is not None and counts[b] == 0:
                assert box[b].tolist() == [float("inf")] * 3 + [float("-inf")] * 3
            else:
                assert torch.isfinite(box[b]).all(), (b, box[b])  # no NaN row was read


# ------------------------------------------------------------------------------------- the clouds of tests 2 - 4
C1, C2 = [300, 257, 64], [280, 300, 130]


def clouds(seeds=(61, 62, 63), n=N_CAP, m=N_CAP, c1=None, c2=None):
    """synth.make_pair clouds stacked to (B, n, 9), (B, m, 9); with counts: pair b has c1[b] / c2[b] triangles, the rows
    beyond are NaN."""
    from rrl_hip import synth
    B = len(seeds)
    src, tar = np.full((B, n, 9), np.nan, np.float32), np.full((B, m, 9), np.nan, np.float32)
    for b, s in enumerate(seeds):
        nb, mb = (n if c1 is None else c1[b]), (m if c2 is None else c2[b])
        pr = synth.make_pair(s, nb, mb)
        src[b, :nb], tar[b, :mb] = pr["src_tri"], pr["tar_tri"]
    return torch.from_numpy(src).cuda(), torch.from_numpy(tar).cuda()


def xi_start(B, seed=7):
    return (0.05 * torch.randn(B, 6, generator=torch.Generator().manual_seed(seed))).cuda()


class Composed:
    """The epoch from the entries that existed before rrl_register_epoch: rrl_sample_lines_rng, ops.RegistrationStep, the
    per-sample monitor (ops.chamfer_group_means) and one ops.se3_adam_step per sample -- on its own buffers, started from
    the batched object's geometry and a generator state with the same seed."""

    def __init__(self, ops, reg, src, tar, c1, c2, seed, monitor):
        B, N, M, L = reg.step.dims
        self.ops, self.B, self.L, self.N, self.monitor, self.rounds = ops, B, L, N, monitor, reg.rounds
        self.rows = [((N if c1 is None else c1[b]) + 255) // 256 for b in range(B)]
        self.step = ops.RegistrationStep(src, tar, L, transpose_r=False, deterministic=True, counts1=c1, counts2=c2)
        self.radius, self.centers, self.box2 = reg.radius, reg.centers, reg.box2  # (read only)
        self.box1, self.xi, self.R, self.T = reg.box1.clone(), reg.xi.clone(), reg.R.clone(), reg.T.clone()
        self.m, self.v, self.state, self.lr = reg.m.clone(), reg.v.clone(), reg.adam_state.clone(), reg.lr.clone()
        self.rng = torch.tensor([seed, 0, 0, 0], dtype=torch.int64, device="cuda")
        self.lines, self.filled, self.tiles = torch.zeros_like(reg.lines), torch.zeros_like(reg.filled), torch.empty_like(reg.tiles)
        self.table, self.cursor, self.row = torch.zeros_like(reg.table), torch.zeros_like(reg.cursor), torch.zeros_like(reg.row)
        self.gxi = torch.zeros_like(reg.gxi)
        self.value = torch.zeros(B, device="cuda") if monitor else None

    def epoch(self):
        ops, P = self.ops, self.ops._p
        ops._run(self.lines.device, "rrl_sample_lines_rng", P(self.rng), P(self.radius), P(self.centers), P(self.box1), P(self.box2),
                 P(self.lines), P(self.filled), P(self.tiles), self.B, self.L, self.rounds)
        loss, gR, gt, _, info = self.step(self.R, self.T, self.lines)
        if self.monitor:
            self.value.copy_(ops.chamfer_group_means(self.step.st, groups=self.B))
        for b in range(self.B):
            table_b = self.table[:, b].contiguous()
            kw = dict(aabb_rows=self.step.st.apart[0, b, :self.rows[b]], box=self.box1[b]) if self.rows[b] else {}
            ops.se3_adam_step(self.xi[b], gR[b], gt[b], self.m[b], self.v[b], self.state[b:b + 1], self.lr[b:b + 1], info[b],
                              self.R[b], self.T[b], gxi=self.gxi[b], loss=loss[b:b + 1],
                              value=None if self.value is None else self.value[b:b + 1], table=table_b,
                              cursor=self.cursor[b:b + 1], row=self.row[b], **kw)
            self.table[:, b] = table_b
        return loss, gR, gt, info


@pytest.mark.parametrize("shape", ["uniform", "ragged", "uniform-monitor"])
def test_one_call_epoch_equals_the_composed_epoch(ops, register, shape):
    """6 epochs, B = 3, N = M = 300, L = 2048, from generators with the same seed: lines, filled, loss, gR, gt, xi, R, T, box1
    and the table after EVERY epoch, bit for bit -- uniform, ragged (counts 300 / 257 / 64 against 280 / 300 / 130) and
    uniform with the monitor, whose value[b] must equal ops.chamfer(moved first points, target first points,
    per_sample=True)[b] to the tolerance tests/test_gpu_ragged_chamfer.py holds that route to (one float32 ulp of the
    float64 mean: both are fixed-order double sums over the same minima, divided and rounded once)."""
    c1, c2 = (C1, C2) if shape == "ragged" else (None, None)
    monitor = shape == "uniform-monitor"
    src, tar = clouds(c1=c1, c2=c2)
    reg = register.PairRegistration(src, tar, L_SMALL, counts1=c1, counts2=c2, xi0=xi_start(3), seed=1234, monitor=monitor,
                                    deterministic=True, table_rows=8)
    ref = Composed(ops, reg, src, tar, c1, c2, 1234, monitor)
    for e in range(6):
        reg.epoch()
        loss, gR, gt, info = ref.epoch()
        for k, a, b in (("lines", reg.lines, ref.lines), ("filled", reg.filled, ref.filled), ("loss", reg.loss, loss),
                        ("gR", reg.step.gR, gR), ("gt", reg.step.gt, gt), ("info", reg.step.st.info, info), ("xi", reg.xi, ref.xi),
                        ("R", reg.R, ref.R), ("T", reg.T, ref.T), ("m", reg.m, ref.m), ("v", reg.v, ref.v),
                        ("state", reg.adam_state, ref.state), ("gxi", reg.gxi, ref.gxi), ("box1", reg.box1, ref.box1),
                        ("row", reg.row, ref.row), ("cursor", reg.cursor, ref.cursor), ("table", reg.table, ref.table)):
            same(a, b, f"{shape}, epoch {e}: {k}")
        if monitor:
            same(reg.value, ref.value, f"epoch {e}: value")
            want = ops.chamfer(reg.moved_points().contiguous(), tar[:, :, :3].contiguous(), per_sample=True)
            got, want = reg.value.cpu().numpy(), want.detach().cpu().numpy()
            ulps = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
            print(f"epoch {e}: monitor {got}, ops.chamfer per sample {want}, |diff| in ulps {ulps}")
            assert np.all(ulps <= 1.0), (e, got, want)
    assert int(reg.filled.min()) > 0 and bool((reg.step.st.info[:, 0] > 0).all())  # lines were drawn, every pair stepped
    assert float((reg.xi - xi_start(3)).abs().max()) > 1e-3
    hist = reg.history()
    assert [len(h) for h in hist] == [6, 6, 6] and all(h[5][1] is not None for h in hist)
    assert all((h[0][2] is not None) == monitor for h in hist)


# ------------------------------------------------------------------------------------- 3: samples do not see each other
def given_lines(ops, reg_like_src, tar, c2, L, seed):
    """One fixed line set per pair through the targets' boxes (the sampler's own, drawn once)."""
    box2 = ops.aabb(tar[:, :, :3].contiguous(), c2)
    radius = (box2[:, 3:] - box2[:, :3]).norm(dim=1)
    B = tar.shape[0]
    rng = torch.tensor([seed, 0, 0, 0], dtype=torch.int64, device="cuda")
    lines, filled = torch.zeros(B, L, 6, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
    tiles = torch.empty(B * 10 * ((L + 1023) // 1024) * 32, dtype=torch.int32, device="cuda")
    P = ops._p
    ops._run(lines.device, "rrl_sample_lines_rng", P(rng), P(radius.contiguous()), P(torch.zeros(B, 3, device="cuda")), P(box2), P(box2),
             P(lines), P(filled), P(tiles), B, L, 10)
    return lines


def test_samples_do_not_see_each_other(ops, register):
    """Given lines (rng_state NULL), 4 epochs, ragged: sample 1's clouds, counts and starting pose are replaced; every output
    of samples 0 and 2 is bit-identical."""
    outs = []
    src, tar = clouds(c1=C1, c2=C2)
    lines = given_lines(ops, src, tar, C2, L_SMALL, 99)
    for variant in range(2):
        c1, c2, s, t, xi0 = list(C1), list(C2), src.clone(), tar.clone(), xi_start(3)
        if variant:
            c1[1], c2[1] = 190, 222
            s2, t2 = clouds(seeds=(70, 71, 72), c1=c1, c2=c2)
            s[1], t[1] = s2[1], t2[1]
            xi0[1] = -3.0 * xi0[1]
        reg = register.PairRegistration(s, t, L_SMALL, counts1=c1, counts2=c2, xi0=xi0, lines=lines, deterministic=True,
                                        table_rows=4)
        assert reg.rng is None
        per_epoch = []
        for _ in range(4):
            reg.epoch()
            per_epoch.append({k: x.clone() for k, x in dict(
                loss=reg.loss, gR=reg.step.gR, gt=reg.step.gt, info=reg.step.st.info, xi=reg.xi, R=reg.R, T=reg.T, m=reg.m,
                v=reg.v, state=reg.adam_state, gxi=reg.gxi, box1=reg.box1, row=reg.row, cursor=reg.cursor,
                table=reg.table.transpose(0, 1), moved=reg.moved_points()[:, :64]).items()})
        same(reg.lines, lines, "the given lines are not overwritten")
        outs.append(per_epoch)
    changed = False
    for e in range(4):
        for k in outs[0][e]:
            for b in (0, 2):
                same(outs[0][e][k][b], outs[1][e][k][b], f"epoch {e}, sample {b}: {k}")
        changed |= not torch.equal(outs[0][e]["xi"][1], outs[1][e]["xi"][1])
    assert changed  # (sample 1 really was another problem)


# ------------------------------------------------------------------------------------- 4: the ragged contract, carried through
def test_first_epoch_per_sample_equals_the_single_pair_call(ops, register):
    """DESIGN section 12's contract through the new entry: sample b's loss and INFO row of the ragged batch's first epoch ==
    those of the B = 1 call on the truncated tensors with the same lines, bit for bit."""
    src, tar = clouds(c1=C1, c2=C2)
    lines = given_lines(ops, src, tar, C2, L_SMALL, 5)
    xi0 = xi_start(3)
    reg = register.PairRegistration(src, tar, L_SMALL, counts1=C1, counts2=C2, xi0=xi0, lines=lines, deterministic=True)
    reg.epoch()
    for b in range(3):
        one = register.PairRegistration(src[b:b + 1, :C1[b]].contiguous(), tar[b:b + 1, :C2[b]].contiguous(), L_SMALL,
                                        xi0=xi0[b:b + 1], lines=lines[b:b + 1], deterministic=True)
        one.epoch()
        same(one.loss, reg.loss[b:b + 1], f"sample {b}: loss")
        same(one.step.st.info, reg.step.st.info[b:b + 1], f"sample {b}: INFO")
        assert int(one.step.st.info[0, 0]) > 0 and float(one.loss[0]) > 0


# ------------------------------------------------------------------------------------- 5: end to end
E2E_PAIRS = ((41, 400, 333), (42, 300, 400), (43, 256, 380))  # (synth.make_pair seed, source and target triangles)
E2E_SEED = 5


def e2e_clouds():
    from rrl_hip import synth
    cap = 400
    src, tar = np.full((3, cap, 9), np.nan, np.float32), np.full((3, cap, 9), np.nan, np.float32)
    for b, (s, n, m) in enumerate(E2E_PAIRS):
        pr = synth.make_pair(s, n, m)
        src[b, :n], tar[b, :m] = pr["src_tri"], pr["tar_tri"]
    return torch.from_numpy(src).cuda(), torch.from_numpy(tar).cuda(), [p[1] for p in E2E_PAIRS], [p[2] for p in E2E_PAIRS]


def test_register_pairs_end_to_end(ops, register):
    """Three ragged synthetic pairs (400 / 333, 300 / 400, 256 / 380 triangles in a capacity of 400, NaN beyond), 4000 lines,
    60 epochs of register_pairs: every pair's Chamfer distance (ops.chamfer on the moved first points with the counts) ends
    below 0.8 times its start -- test_demo_end_to_end_reduces_chamfer's own threshold.
    Measured ratios end / start on one MI355X (E2E_PAIRS, sampler seed 5; the backward's float atomics move the last digits
    from run to run): register_pairs 0.6014 / 0.4632 / 0.6516; the existing B = 1 demo (graphed, device RNG, torch seed 5,
    60 epochs) on each pair alone 0.6097 / 0.4708 / 0.6282.  With sampler seed 11: 0.6104 / 0.4608 / 0.6346 against the
    demo's 0.6339 / 0.4564 / 0.6440.  (synth seeds 31 / 32 / 33 were also measured and not chosen: 0.73 / 0.62 / 0.74 and the
    demo's 0.75 / 0.67 / 0.75 leave less room under 0.8.)"""
    src, tar, c1, c2 = e2e_clouds()
    sp, tp = src[:, :, :3].contiguous(), tar[:, :, :3].contiguous()
    start = ops.chamfer(sp, tp, counts_x=c1, counts_y=c2, per_sample=True).cpu()
    reg = register.PairRegistration(src, tar, 4000, counts1=c1, counts2=c2, seed=E2E_SEED)
    reg.run(60)
    end = ops.chamfer(reg.moved_points().contiguous(), tp, counts_x=c1, counts_y=c2, per_sample=True).cpu()
    print("Chamfer start", start.tolist(), "end", end.tolist(), "ratio", (end / start).tolist())
    hist = reg.history()
    assert all(sum(h[1] is not None for h in hh) >= 50 for hh in hist)
    assert bool((end < 0.8 * start).all()), (start, end)
    R, T, hist2 = register.register_pairs(src, tar, 4000, n_epoch=2, counts1=c1, counts2=c2, seed=E2E_SEED)
    assert R.shape == (3, 3, 3) and T.shape == (3, 3) and [len(h) for h in hist2] == [2, 2, 2]
