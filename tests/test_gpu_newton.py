"""The second-order pose path on the GPU (include/rrl.h rrl_pose_normal_eq, rrl_se3_newton_step_batch,
rrl_register_newton_epoch; rrl_hip/newton.py).

1. The normal equations against the float64 twin (tests/newton_refs.py) on the workspace read back through the Python views,
   per sum |got - twin| <= NEQ_C 2^-23 sum|terms|; bit-identical over 20 calls; g against the chain-rule image of the
   deterministic direct backward's (dR, dt).
2. The pose step against the twin: backward error of the solve, clamps, orthonormality after 500 compositions, closed gates /
   singular / NaN systems, the box, the stopping rule.
3. The one-call epoch == sampler + forward + rrl_pose_normal_eq + step, bit for bit; samples do not see each other; the ragged
   contract.
4. End to end against the first-order loop."""
import numpy as np
import pytest
import torch

import kabsch_refs as KR
import newton_refs as NR
from test_gpu_register_batch import C1, C2, N_CAP, clouds, given_lines, same, xi_start

pytestmark = pytest.mark.gpu

U23 = 2.0 ** -23
# The allowance of a sum, in units of 2^-23 sum|terms|: twice the worst ratio measured over the cases of this file, 1.105
# (DESIGN.md section 15 has the table: 0.51 .. 1.11 per case).  The inputs are float32 and only the accumulation is double: a
# term carries the roundings of gD (seven float32 operations and two expf) and of its own two or three products.
NEQ_C = 2.21
# The solve's backward error in units of 2^-23 |A| |x|: x leaves the kernel as float32, |dx| <= 2^-24 |x| per component, so
# |A (x + dx) + g| <= 2^-24 |A| |x| = 0.5 units (the double Cholesky's own error, ~6 2^-53, disappears in it); twice that.
SOLVE_C = 1.0


@pytest.fixture(scope="module")
def ops():
    from rrl_hip import _lib, ops
    _lib.load()
    assert torch.cuda.is_available()
    return ops


@pytest.fixture(scope="module")
def newton():
    from rrl_hip import newton
    return newton


def poses(B, seed=3, angle=0.08):
    """(R (B, 3, 3), T (B, 3)) float32 on the GPU: y = x R + T, rotations of `angle` radians about seeded axes."""
    rs = np.random.default_rng(seed)
    R, T = np.zeros((B, 3, 3), np.float32), np.zeros((B, 3), np.float32)
    for b in range(B):
        w = rs.standard_normal(3)
        R[b], T[b] = NR.rodrigues(angle * w / np.linalg.norm(w)).T, 0.03 * rs.standard_normal(3)
    return torch.from_numpy(R).cuda(), torch.from_numpy(T).cuda()


def counted_clouds(seeds, n, m, c1=None, c2=None):
    """clouds() of full size with the rows beyond a count overwritten by NaN (a count may be 0)."""
    src, tar = clouds(seeds=seeds, n=n, m=m)
    for t, c in ((src, c1), (tar, c2)):
        if c is not None:
            for b, cb in enumerate(c):
                t[b, cb:] = float("nan")
    return src, tar


def fields_of(st, b):
    """Sample b's fields of a LossState as numpy arrays (the twin's input)."""
    g = lambda name: getattr(st, name)[b].cpu().numpy()  # noqa: E731
    return dict(kj=g("kj"), w1=g("w1"), Q1=g("Q1"), Q2=g("Q2"), D=g("D"), med=float(st.med[b]), bcnt=g("bcnt"), info=g("info"),
                hs1=g("hs1"))


# ------------------------------------------------------------------------------------- 1: the normal equations
FAR = torch.tensor([1.0, 0.0, 0.0, 0.0, 5.0, 5.0])  # a line that passes every cloud of this file at distance 7

# name -> B, N, M, L, mode, prepared, counts1, counts2, nlines, the sample whose lines all miss (or None)
NEQ_CASES = {
    "B1-64x257-L1000-cull-prepared": (1, 64, 257, 1000, "cull", True, None, None, None, None),
    "B3-300x300-L1025-cull-prepared-ragged": (3, 300, 300, 1025, "cull", True, [300, 0, 64], [280, 300, 130], None, None),
    "B3-300x257-L1025-cull-cold-nlines": (3, 300, 257, 1025, "cull", False, None, None, [1025, 0, 513], None),
    "B3-257x64-L33793-strict-cold": (3, 257, 64, 33 * 1024 + 1, "strict", False, None, None, None, 1),
    "B1-300x300-L33793-cull-prepared": (1, 300, 300, 33 * 1024 + 1, "cull", True, None, None, None, None),
    "B3-64x300-L1000-strict-cold-empty": (3, 64, 300, 1000, "strict", False, None, None, None, 2),
}


@pytest.fixture(scope="module")
def neq_runs(ops):
    """Every case evaluated ONCE: a deterministic RegistrationStep (forward + direct backward), rrl_pose_normal_eq on its
    workspace, the twin's sums per sample."""
    out = {}
    for name, (B, N, M, L, mode, prepared, c1, c2, nl, miss) in NEQ_CASES.items():
        seeds = tuple(range(80, 80 + B))
        src, tar = counted_clouds(seeds, N, M, c1, c2)
        full_src, full_tar = clouds(seeds=seeds, n=N, m=M)
        lines = given_lines(ops, full_src, full_tar, None, L, 17)
        if miss is not None:
            lines[miss] = FAR.cuda()
        R, T = poses(B)
        step = ops.RegistrationStep(src, tar, L, transpose_r=False, mode=mode, prepared=prepared, deterministic=True, counts1=c1,
                                    counts2=c2, nlines=nl)
        assert step.prepared == prepared
        loss, gR, gt, _, info = step(R, T, lines)
        neq = ops.pose_normal_eq(step.st)
        torch.cuda.synchronize()
        twins = [NR.normal_sums(fields_of(step.st, b)) for b in range(B)]
        out[name] = dict(step=step, src=src, R=R, T=T, neq=neq.clone(), gR=gR.clone(), gt=gt.clone(), info=info.clone(), twins=twins)
    return out


@pytest.mark.parametrize("name", list(NEQ_CASES))
def test_normal_equations_against_the_twin(ops, neq_runs, name):
    """Per sum |got - twin| <= NEQ_C 2^-23 sum|terms|; a sample without a populated bucket (a zero count, no lines, lines that
    all miss) gives sixteen zeros; every other sample has pairs."""
    B, N, M, L, mode, prepared, c1, c2, nl, miss = NEQ_CASES[name]
    run = neq_runs[name]
    got, info = run["neq"].cpu().numpy().astype(np.float64), run["info"].cpu().numpy()
    worst = 0.0
    for b in range(B):
        sums, abs_sums, n = run["twins"][b]
        empty = (c1 is not None and c1[b] == 0) or (c2 is not None and c2[b] == 0) or (nl is not None and nl[b] == 0) or miss == b
        assert (info[b, 0] == 0) == empty, (b, info[b])
        if empty:
            assert n == 0 and not np.any(run["neq"][b].cpu().numpy().view(np.int32)), (b, got[b])  # sixteen +0.0
            continue
        assert n > 0 and np.all(abs_sums > 0)
        ratio = np.abs(got[b] - sums) / (U23 * abs_sums)
        print(f"{name} sample {b}: {n} pairs, |got - twin| / (2^-23 sum|terms|) per sum: {np.array2string(ratio, precision=3)}")
        worst = max(worst, float(ratio.max()))
        assert np.all(ratio <= NEQ_C), (b, ratio)
    print(f"{name}: worst ratio {worst:.3f} (allowed {NEQ_C})")


def test_normal_equations_are_bit_identical_over_20_calls(ops, neq_runs):
    """Two cases (two tiles ragged; beyond 32 tiles): 20 more calls on the same workspace, into fresh buffers, all equal to
    the first call's bits."""
    for name in ("B3-300x300-L1025-cull-prepared-ragged", "B3-257x64-L33793-strict-cold"):
        run = neq_runs[name]
        for i in range(20):
            again = ops.pose_normal_eq(run["step"].st)
            same(again, run["neq"], f"{name}: call {i + 2}")


@pytest.mark.parametrize("name", list(NEQ_CASES))
def test_the_gradient_is_the_chain_rule_image_of_the_direct_backward(ops, neq_runs, name):
    """g_v against dL/dT and g_w against vee(A - A^T) + T x dL/dT, A = R^T dL/dR, of the deterministic RegistrationStep on the
    same inputs: |g - image| <= NEQ_C 2^-23 sum|terms of g| + (k + 3) 2^-24 sum|terms of the image| -- the first as above,
    the second the direct backward's documented form (k contributions summed in float32)."""
    B = NEQ_CASES[name][0]
    run = neq_runs[name]
    st, src = run["step"].st, run["src"].cpu().numpy().astype(np.float64)
    for b in range(B):
        sums, abs_sums, n = run["twins"][b]
        if n == 0:
            assert not np.any(run["gR"][b].cpu().numpy()) and not np.any(run["gt"][b].cpu().numpy())
            continue
        f = fields_of(st, b)
        p = NR.selected_pairs(f)
        tri = src[b][f["hs1"][p["line"], p["h"]]].reshape(-1, 3, 3)          # (pairs, point, xyz) of the source as given
        wk = f["w1"].astype(np.float64)[p["line"], p["h"]] / 3.0             # (pairs, point)
        gq = np.abs(2.0 * p["a"][:, None] * p["e"])                            # (pairs, xyz)
        aR = np.einsum("pkc,pk,pj->cj", np.abs(tri), wk, gq)
        at = (wk.sum(1)[:, None] * gq).sum(0)
        R, T = run["R"][b].cpu().numpy(), run["T"][b].cpu().numpy()
        gw, gv = NR.chain_rule_gradient(run["gR"][b].cpu().numpy(), run["gt"][b].cpu().numpy(), R, T)
        aw, av = NR.chain_rule_abs(aR, at, R, T)
        k = 3 * n
        got = run["neq"][b].cpu().numpy().astype(np.float64)
        allowed = NEQ_C * U23 * abs_sums[10:16] + (k + 3) * 2.0 ** -24 * np.concatenate([aw, av])
        err = np.abs(got[10:16] - np.concatenate([gw, gv]))
        print(f"{name} sample {b}: |g - image| / allowed {np.array2string(err / allowed, precision=4)}; "
              f"in units of 2^-23 sum|terms|: {np.array2string(err / (U23 * abs_sums[10:16]), precision=2)}")
        assert np.all(err <= allowed), (b, err / allowed)


# ------------------------------------------------------------------------------------- 2: the pose step
COUNTS = [300, 257, 64, 0]


def random_neq(rs, n=40, scale=1.0):
    """Sixteen sums of n random pairs (a PSD system with a step of moderate length)."""
    a = rs.uniform(0.1, 1.0, n)
    Q, e, s = rs.standard_normal((n, 3)), scale * 0.05 * rs.standard_normal((n, 3)), rs.uniform(0.2, 0.4, n)
    a2 = 2 * a
    cr = np.cross(Q, e)
    v = [a2 * Q[:, 0] * Q[:, 0], a2 * Q[:, 0] * Q[:, 1], a2 * Q[:, 0] * Q[:, 2], a2 * Q[:, 1] * Q[:, 1], a2 * Q[:, 1] * Q[:, 2],
         a2 * Q[:, 2] * Q[:, 2], a2 * s * Q[:, 0], a2 * s * Q[:, 1], a2 * s * Q[:, 2], a2 * s * s, a2 * cr[:, 0], a2 * cr[:, 1],
         a2 * cr[:, 2], a2 * s * e[:, 0], a2 * s * e[:, 1], a2 * s * e[:, 2]]
    return np.array([x.sum() for x in v], np.float32)


def step_inputs(B, seed):
    """Per sample: a system (every 5th all-zero, every 7th with a NaN sum, every 3rd scaled so that a clamp is hit), a gate
    (every 4th closed), controls that differ per sample, cursors on both sides of the table's end, partial rows that are NaN
    beyond the sample's count."""
    rs = np.random.default_rng(seed)
    neq = np.stack([random_neq(rs, scale=(30.0 if b % 3 == 1 else 1.0)) for b in range(B)])
    for b in range(B):
        if b % 5 == 2:
            neq[b] = 0.0
        if b % 7 == 4:
            neq[b, rs.integers(16)] = np.nan
    R, T = poses(B, seed)
    nblk, rows = (N_CAP + 255) // 256, 4
    apart = torch.randn(B, nblk, 8, generator=torch.Generator().manual_seed(seed))
    counts = [COUNTS[b % 4] for b in range(B)]
    for b in range(B):
        apart[b, (counts[b] + 255) // 256:] = float("nan")
    t = dict(neq=torch.from_numpy(neq), gate=torch.tensor([[0 if b % 4 == 3 else 5 + b, 1, 1, 0] for b in range(B)], dtype=torch.int32),
             damping=torch.tensor([[0.0, 1e-3, 1e-2, 1e-1][b % 4] for b in range(B)]), step=torch.tensor([[1.0, 0.5][b % 2] for b in range(B)]),
             max_rot=torch.tensor([0.2 / (1 + b % 3) for b in range(B)]), max_trans=torch.tensor([0.1 / (1 + b % 2) for b in range(B)]),
             tol_rot=torch.full((B,), 1e-3), tol_trans=torch.full((B,), 1e-3), R=R, T=T,
             loss=torch.randn(B, generator=torch.Generator().manual_seed(seed + 1)), value=torch.rand(B, generator=torch.Generator().manual_seed(seed + 2)),
             table=torch.zeros(rows, B, 3), cursor=torch.tensor([b % (rows + 2) for b in range(B)]), row=torch.zeros(B, 3),
             apart=apart, box=torch.zeros(B, 6), delta=torch.full((B, 6), 7.0), last_step=torch.full((B, 2), 7.0),
             state=torch.tensor([[b % 3, 0, -1, 9] for b in range(B)], dtype=torch.int32),
             counts=torch.tensor(counts, dtype=torch.int32))
    return {k: x.cuda().contiguous() for k, x in t.items()}, counts


def run_step(ops, t, patience=3, eps=1e-12):
    ops.se3_newton_step_batch(t["neq"], t["gate"], t["R"], t["T"], t["state"], damping=t["damping"], step=t["step"],
                              max_rot=t["max_rot"], max_trans=t["max_trans"], tol_rot=t["tol_rot"], tol_trans=t["tol_trans"],
                              patience=patience, eps=eps, gate_stride=4, loss=t["loss"], value=t["value"], table=t["table"],
                              cursor=t["cursor"], row=t["row"], aabb_rows=t["apart"], capacity=N_CAP, counts=t["counts"], box=t["box"],
                              delta=t["delta"], last_step=t["last_step"])


@pytest.mark.parametrize("B", [1, 3, 70])
def test_pose_step_against_the_twin(ops, B):
    """One launch for B poses against the twin, sample by sample: the state words; the solve's backward error
    |(H + damping diag H + eps I) x + g| <= SOLVE_C 2^-23 |A|_2 |x|; a clamped norm IS the clamp, bit for bit; the composed pose
    within 4 float32 ulps of the twin's on the device's own x; closed gates, all-zero and NaN systems leave R, T, delta and
    last_step untouched and say so in state[3]; the log row, the cursor and the box (NaN rows beyond a count never read)."""
    t, counts = step_inputs(B, 50 + B)
    before = {k: x.clone() for k, x in t.items()}
    run_step(ops, t)
    h = {k: x.cpu().numpy() for k, x in t.items()}
    h0 = {k: x.cpu().numpy() for k, x in before.items()}
    kinds, worst = set(), 0.0
    for b in range(B):
        args = dict(damping=float(h0["damping"][b]), step_scale=float(h0["step"][b]), max_rot=float(h0["max_rot"][b]),
                    max_trans=float(h0["max_trans"][b]), tol_rot=1e-3, tol_trans=1e-3, patience=3, eps=1e-12)
        Rn, Tn, st, x, ls = NR.step(h0["neq"][b].astype(np.float64), int(h0["gate"][b, 0]), h0["R"][b], h0["T"][b], h0["state"][b], **args)
        assert h["state"][b].tolist() == st.tolist(), (b, h["state"][b], st)
        kinds.add(int(st[3]))
        if st[3] != NR.STEPPED:
            for k in ("R", "T", "delta", "last_step"):
                assert np.array_equal(h[k][b].view(np.int32), h0[k][b].view(np.int32)), (b, k)
        else:
            H, g = NR.assemble(h0["neq"][b].astype(np.float64))
            A = NR.damped(H, args["damping"], 1e-12)
            xd = h["delta"][b].astype(np.float64)
            res = np.linalg.norm(A @ xd + g) / (U23 * np.linalg.norm(A, 2) * np.linalg.norm(xd))
            worst = max(worst, res)
            assert res <= SOLVE_C, (b, res)
            assert np.abs(xd - x).max() <= 4 * 2.0 ** -24 * np.abs(x).max() * np.linalg.cond(A)
            w, v, nw, nv = NR.clamp(xd, args["step_scale"], args["max_rot"], args["max_trans"])
            for got, norm, cap in ((h["last_step"][b, 0], nw, h0["max_rot"][b]), (h["last_step"][b, 1], nv, h0["max_trans"][b])):
                if norm == float(cap):
                    assert got == cap, (b, got, cap)  # the clamp itself, bit for bit
                    kinds.add("clamped")
                else:
                    assert abs(float(got) - norm) <= 2.0 ** -23 * norm
            R2, T2 = NR.compose(h0["R"][b], h0["T"][b], w, v)
            assert np.abs(h["R"][b] - R2).max() <= 4 * 2.0 ** -24 and np.abs(h["T"][b] - T2).max() <= 4 * 2.0 ** -24 * (1 + np.abs(T2).max())
            assert np.abs(h["R"][b].astype(np.float64) @ h["R"][b].astype(np.float64).T - np.eye(3)).max() <= 4 * 2.0 ** -24
        # the log row and the cursor (the Adam step's contract), the box
        want = [h0["loss"][b], h0["value"][b], 1.0 if h0["gate"][b, 0] > 0 else 0.0]
        assert h["row"][b].tolist() == want and h["cursor"][b] == h0["cursor"][b] + 1
        at = int(h0["cursor"][b])
        assert (h["table"][at, b].tolist() == want) if at < h["table"].shape[0] else not np.any(h["table"][:, b])
        nr = (counts[b] + 255) // 256
        if nr == 0:
            assert h["box"][b].tolist() == [float("inf")] * 3 + [float("-inf")] * 3
        else:
            rows = h0["apart"][b, :nr]
            assert h["box"][b].tolist() == rows[:, :3].min(0).tolist() + rows[:, 3:6].max(0).tolist()
    print(f"B = {B}: worst backward error {worst:.3f} x 2^-23 |A| |x| (allowed {SOLVE_C}); kinds {sorted(map(str, kinds))}")
    if B >= 3:
        assert {NR.STEPPED, NR.FAILED} <= kinds and "clamped" in kinds
    if B == 70:
        assert NR.GATED in kinds


def test_500_composed_steps_stay_orthonormal(ops):
    """500 steps of B = 3 fixed systems (rotations of up to 0.2 rad each, no stopping rule): R R^T - I within 1e-6, det R = +1."""
    t, _ = step_inputs(3, 91)
    t["neq"] = torch.from_numpy(np.stack([random_neq(np.random.default_rng(7 + b), scale=20.0) for b in range(3)])).cuda()
    t["gate"][:, 0] = 1
    for _ in range(500):
        run_step(ops, t, patience=0)
    R = t["R"].double().cpu()
    assert t["state"][:, 0].tolist() == [500 + b for b in range(3)] and t["state"][:, 3].tolist() == [0, 0, 0]
    assert float(t["last_step"][:, 0].min()) > 0.01  # (the poses really turned)
    err = (R @ R.transpose(1, 2) - torch.eye(3, dtype=torch.float64)).abs().max()
    print(f"500 compositions: max |R R^T - I| = {float(err):.3e}")
    assert float(err) <= 1e-6 and bool((torch.linalg.det(R) > 0.999).all())


def test_the_stopping_rule_on_the_device(ops):
    """B = 3, patience 3: sample 0's steps are tiny from the start -> done_epoch = 3, set once; sample 1 is calm twice, then
    takes a large step (the count starts again), then is calm three times -> 6; sample 2 never is.  A done pair's pose keeps
    its bits whatever system arrives, and its state says RRL_NEWTON_DONE."""
    t, _ = step_inputs(3, 77)
    rs = np.random.default_rng(1)
    small, big = random_neq(rs, scale=1e-4), random_neq(rs, scale=20.0)
    t["gate"][:, 0] = 1
    t["state"][:, 0] = 0
    t["damping"].fill_(1e-2); t["step"].fill_(1.0); t["max_rot"].fill_(0.2); t["max_trans"].fill_(0.1)
    plan = {0: [small] * 8, 1: [small, small, big, small, small, small, big, big], 2: [big] * 8}
    frozen = {}
    for e in range(8):
        t["neq"] = torch.from_numpy(np.stack([plan[b][e] for b in range(3)])).cuda()
        run_step(ops, t, patience=3)
        st = t["state"].cpu().numpy()
        for b, at in ((0, 3), (1, 6)):
            if e + 1 == at:
                assert st[b, 2] == at and st[b, 3] == NR.STEPPED
                frozen[b] = (t["R"][b].clone(), t["T"][b].clone())
            elif e + 1 > at:
                assert st[b, 2] == at and st[b, 3] == NR.DONE
                same(t["R"][b], frozen[b][0], f"sample {b}, epoch {e}: R frozen")
                same(t["T"][b], frozen[b][1], f"sample {b}, epoch {e}: T frozen")
            else:
                assert st[b, 2] == -1
        assert st[2, 2] == -1 and st[2, 3] == NR.STEPPED and st[:, 0].tolist() == [e + 1] * 3
    assert float(t["last_step"][0].max()) < 1e-3 and float(t["last_step"][2, 0]) > 1e-3


def test_both_steps_apply_one_stopping_rule(ops):
    """rrl_se3_newton_step_batch (diagonal systems: NR.diagonal_neq) and rrl_icp_step_batch (crafted fits: KR.stepped_fit) fed
    the same (rotation, translation) step lengths for 8 launches, B = 5, patience 3, tolerances 1e-3 and every length a
    factor 4 from them.  Pose 0: not calm, calm twice, a reset (the rotation alone is calm), calm three times -> done at 7;
    pose 1: calm from the start -> done at 3; pose 2: never calm; pose 3: done on entry; pose 4: fails in launches 3 and 7 on
    each side's own terms (gate 0 / RRL_FIT_FEW), which resets its count, and is done at 6.  Columns 0 .. 2 of the two states
    are equal after every launch, and the done pose keeps its bytes on both sides."""
    B, patience = 5, 3
    calm, far, mixed, fail = (2.5e-4, 2.5e-4), (4e-3, 4e-3), (2.5e-4, 4e-3), None
    plan = [[far, calm, calm, mixed, calm, calm, calm, far], [calm] * 8, [far] * 8, [far] * 8,
            [calm, calm, fail, calm, calm, calm, fail, calm]]
    state0 = torch.tensor([[0, 0, -1, 0]] * 3 + [[9, 3, 7, 0], [0, 0, -1, 0]], dtype=torch.int32).cuda()
    R0, T0 = poses(B)
    tols, one, zero = torch.full((B,), 1e-3).cuda(), torch.ones(B).cuda(), torch.zeros(B).cuda()
    fit = torch.zeros(B, 32, dtype=torch.float64).cuda()  # (abar = 0: the centroid moves by Tk - T)
    Rn, Tn, sn, Ri, Ti, si = R0.clone(), T0.clone(), state0.clone(), R0.clone(), T0.clone(), state0.clone()
    P = ops._p
    for e in range(8):
        row = [plan[b][e] for b in range(B)]
        ok = torch.tensor([r is not fail for r in row])
        lengths = [r or far for r in row]
        neq = torch.from_numpy(np.stack([NR.diagonal_neq(*x) for x in lengths])).cuda()
        ops.se3_newton_step_batch(neq, ok.to(torch.int32).cuda(), Rn, Tn, sn, damping=zero, step=one, max_rot=one, max_trans=one,
                                  tol_rot=tols, tol_trans=tols, patience=patience)
        fits = [KR.stepped_fit(Ri[b].cpu().numpy(), Ti[b].cpu().numpy(), *lengths[b]) for b in range(B)]
        Rk, Tk = (torch.from_numpy(np.stack([f[k] for f in fits])).cuda() for k in (0, 1))
        info = torch.zeros(B, 4, dtype=torch.int32)
        info[:, 1] = torch.where(ok, KR.FIT_OK, KR.FIT_FEW)
        info = info.cuda()
        ops._run(Ri.device, "rrl_icp_step_batch", P(Rk), P(Tk), P(info), P(fit), P(Ri), P(Ti), P(tols), P(tols), patience, None, None,
                 None, 0, None, None, P(si), B)
        torch.cuda.synchronize()
        assert torch.equal(sn[:, :3], si[:, :3]), (e, sn.tolist(), si.tolist())
        assert sn[:, 0].tolist() == [e + 1, e + 1, e + 1, e + 10, e + 1]
        for R, T in ((Rn, Tn), (Ri, Ti)):
            same(R[3], R0[3], f"launch {e}: the done pose's R")
            same(T[3], T0[3], f"launch {e}: the done pose's T")
    assert sn[:, 2].tolist() == [7, 3, -1, 7, 6] and sn[:, 1].tolist() == [3, 3, 0, 3, 3]
    assert sn[:, 3].tolist() == [NR.DONE] * 2 + [NR.STEPPED] + [NR.DONE] * 2 and si[:, 3].tolist() == [KR.ICP_DONE] * 2 + [KR.FIT_OK] + [KR.ICP_DONE] * 2


# ------------------------------------------------------------------------------------- 3: the one-call epoch
class Composed:
    """The epoch from its parts: rrl_sample_lines_rng, the registration FORWARD alone on a RegistrationStep's buffers and
    options (first call: build both clouds; later: kept target), the per-sample monitor, ops.pose_normal_eq,
    ops.se3_newton_step_batch -- on its own buffers, started from the one-call object's geometry, poses and controls."""

    def __init__(self, ops, reg, src, tar, c1, c2, seed):
        B, N, M, L = reg.step.dims
        self.ops, self.B, self.L, self.N, self.reg = ops, B, L, N, reg
        self.step = ops.RegistrationStep(src, tar, L, transpose_r=False, counts1=c1, counts2=c2)
        self.box1, self.R, self.T = reg.box1.clone(), reg.R.clone(), reg.T.clone()
        self.rng = torch.tensor([seed, 0, 0, 0], dtype=torch.int64, device="cuda")
        self.lines, self.filled, self.tiles = torch.zeros_like(reg.lines), torch.zeros_like(reg.filled), torch.empty_like(reg.tiles)
        self.table, self.cursor, self.row = torch.zeros_like(reg.table), torch.zeros_like(reg.cursor), torch.zeros_like(reg.row)
        self.state, self.delta, self.last_step = reg.state.clone(), reg.delta.clone(), reg.last_step.clone()
        self.neq = torch.zeros_like(reg.neq)
        self.value = torch.zeros(B, device="cuda") if reg.monitor else None

    def epoch(self):
        ops, P, reg, st = self.ops, self.ops._p, self.reg, self.step
        ops._run(self.lines.device, "rrl_sample_lines_rng", P(self.rng), P(reg.radius), P(reg.centers), P(self.box1), P(reg.box2),
                 P(self.lines), P(self.filled), P(self.tiles), self.B, self.L, reg.rounds)
        op, key = st._pick(False)
        ops._run(st.dev, "rrl_registration_forward_ex", P(st.src), P(self.R), P(self.T), P(st.tar), P(self.lines), *st._fixed_f, op)
        st._done(key)
        if self.value is not None:
            self.value.copy_(ops.chamfer_group_means(st.st, groups=self.B))
        ops.pose_normal_eq(st.st, neq=self.neq)
        ops.se3_newton_step_batch(self.neq, st.st.info, self.R, self.T, self.state, damping=reg.damping, step=reg.step_scale,
                                  max_rot=reg.max_rot, max_trans=reg.max_trans, tol_rot=reg.tol_rot, tol_trans=reg.tol_trans,
                                  patience=reg.patience, eps=reg.eps, gate_stride=4, loss=st.st.loss, value=self.value,
                                  table=self.table, cursor=self.cursor, row=self.row, aabb_rows=st.st.apart[0], capacity=self.N,
                                  counts=st.counts1, box=self.box1, delta=self.delta, last_step=self.last_step)


@pytest.mark.parametrize("shape", ["uniform", "ragged", "uniform-monitor"])
def test_one_call_epoch_equals_the_composed_sequence(ops, newton, shape):
    """6 epochs, N = M = 300, L = 2048, generators with the same seed: lines, filled, loss, INFO, the sixteen sums, R, T, delta,
    last_step, the state, box1, the log and the monitor's value after EVERY epoch, bit for bit -- uniform (B = 3), ragged
    (B = 4, counts 300 / 257 / 64 / 0 against 280 / 300 / 130 / 300: box1 must be ops.aabb of the moved points with the counts,
    rows beyond them NaN) and uniform with the monitor."""
    ragged, monitor = shape == "ragged", shape == "uniform-monitor"
    c1, c2 = ([300, 257, 64, 0], C2 + [300]) if ragged else (None, None)
    B = 4 if ragged else 3
    src, tar = counted_clouds((61, 62, 63, 64)[:B], N_CAP, N_CAP, c1, c2)
    R0, T0 = poses(B, 11, 0.1)
    reg = newton.NewtonRegistration(src, tar, 2048, counts1=c1, counts2=c2, R0=R0, T0=T0, seed=1234, monitor=monitor, table_rows=8,
                                    patience=2, tol_rot=0.05, tol_trans=0.05)
    ref = Composed(ops, reg, src, tar, c1, c2, 1234)
    for e in range(6):
        reg.epoch()
        ref.epoch()
        for k, a, b in (("lines", reg.lines, ref.lines), ("filled", reg.filled, ref.filled), ("loss", reg.loss, ref.step.st.loss),
                        ("info", reg.step.st.info, ref.step.st.info), ("neq", reg.neq, ref.neq), ("R", reg.R, ref.R), ("T", reg.T, ref.T),
                        ("delta", reg.delta, ref.delta), ("last_step", reg.last_step, ref.last_step), ("state", reg.state, ref.state),
                        ("box1", reg.box1, ref.box1), ("row", reg.row, ref.row), ("cursor", reg.cursor, ref.cursor),
                        ("table", reg.table, ref.table)):
            same(a, b, f"{shape}, epoch {e}: {k}")
        if monitor:
            same(reg.value, ref.value, f"epoch {e}: value")
        same(reg.box1, ops.aabb(reg.moved_points().contiguous(), reg.step.counts1), f"{shape}, epoch {e}: box1 == ops.aabb of the moved points")
    st = reg.state.cpu().numpy()
    assert st[:, 0].tolist() == [6] * B
    if ragged:
        assert st[3, 3] == NR.GATED and reg.box1[3].tolist() == [float("inf")] * 3 + [float("-inf")] * 3
        same(reg.R[3], R0[3], "a pair without a source keeps its pose")
    assert int(reg.filled[:3].min()) > 0 and bool((reg.step.st.info[:3, 0] > 0).all())  # (no box, no lines: the pair without a source)
    assert float((reg.R[:3] - R0[:3]).abs().max()) > 1e-3
    hist = reg.history()
    assert [len(h) for h in hist] == [6] * B and all(h[5][1] is not None for h in hist[:3])
    assert all((h[0][2] is not None) == monitor for h in hist[:3])
    xi = reg.xi()
    back = ops.se3_exp(xi.cuda())
    assert float((back[0] - reg.R).abs().max()) < 1e-5 and float((back[1] - reg.T).abs().max()) < 1e-5


def test_samples_do_not_see_each_other(ops, newton):
    """Given lines, 4 epochs, ragged: sample 1's clouds, counts and starting pose are replaced; every output of samples 0 and 2
    is bit-identical."""
    outs = []
    src, tar = clouds(c1=C1, c2=C2)
    lines = given_lines(ops, src, tar, C2, 2048, 99)
    for variant in range(2):
        c1, c2, s, t, xi0 = list(C1), list(C2), src.clone(), tar.clone(), xi_start(3)
        if variant:
            c1[1], c2[1] = 190, 222
            s2, t2 = clouds(seeds=(70, 71, 72), c1=c1, c2=c2)
            s[1], t[1] = s2[1], t2[1]
            xi0[1] = -3.0 * xi0[1]
        reg = newton.NewtonRegistration(s, t, 2048, counts1=c1, counts2=c2, xi0=xi0, lines=lines, table_rows=4)
        assert reg.rng is None
        per_epoch = []
        for _ in range(4):
            reg.epoch()
            per_epoch.append({k: x.clone() for k, x in dict(
                loss=reg.loss, info=reg.step.st.info, neq=reg.neq, R=reg.R, T=reg.T, delta=reg.delta, last_step=reg.last_step,
                state=reg.state, box1=reg.box1, row=reg.row, cursor=reg.cursor, table=reg.table.transpose(0, 1),
                moved=reg.moved_points()[:, :64]).items()})
        same(reg.lines, lines, "the given lines are not overwritten")
        outs.append(per_epoch)
    changed = False
    for e in range(4):
        for k in outs[0][e]:
            for b in (0, 2):
                same(outs[0][e][k][b], outs[1][e][k][b], f"epoch {e}, sample {b}: {k}")
        changed |= not torch.equal(outs[0][e]["R"][1], outs[1][e]["R"][1])
    assert changed


def test_first_epoch_per_sample_equals_the_single_pair_call(ops, newton):
    """Sample b's loss, INFO row, sixteen sums and stepped pose of the ragged batch's first epoch == those of the B = 1 call
    on the truncated tensors with the same lines, bit for bit."""
    src, tar = clouds(c1=C1, c2=C2)
    lines = given_lines(ops, src, tar, C2, 2048, 5)
    xi0 = xi_start(3)
    reg = newton.NewtonRegistration(src, tar, 2048, counts1=C1, counts2=C2, xi0=xi0, lines=lines)
    reg.epoch()
    for b in range(3):
        one = newton.NewtonRegistration(src[b:b + 1, :C1[b]].contiguous(), tar[b:b + 1, :C2[b]].contiguous(), 2048, xi0=xi0[b:b + 1],
                                        lines=lines[b:b + 1])
        one.epoch()
        for k, x, y in (("loss", one.loss, reg.loss), ("INFO", one.step.st.info, reg.step.st.info), ("neq", one.neq, reg.neq),
                        ("R", one.R, reg.R), ("T", one.T, reg.T), ("state", one.state, reg.state)):
            same(x, y[b:b + 1], f"sample {b}: {k}")
        assert int(one.step.st.info[0, 0]) > 0 and int(one.state[0, 3]) == NR.STEPPED


# ------------------------------------------------------------------------------------- 4: end to end
def test_newton_beats_the_first_order_loop_and_stops_by_itself(ops, newton):
    """The source of synth.make_pair(N = M = 512, noise 0, 5 degrees) against an EXACT rigid copy of it -- make_pair's own
    rotation (5 degrees about its axis) and translation applied to the source's points, centred like make_pair's target, the
    pseudo-triangles by synth.knn_triangles --, L = 4000, fixed seeds.  After 40 epochs the Newton pose's rotation-angle error
    against the known rotation is below PairRegistration's after the same 40 epochs; with check_every = 5, .run(200) returns
    early with every done_epoch >= 0.

    Measured on one MI355X (synth seeds 21 / 22 / 23, sampler seeds 9 and 10): NewtonRegistration 0.000 .. 0.013 degrees from
    epoch 5 on, PairRegistration 0.10 .. 0.68 degrees at epoch 40 (0.16 and 0.50 in two runs of this very test: float
    atomics; 0.2 .. 5.7 later: it jitters by its rate); the stopping
    rule ends every one of these runs after 5 epochs at <= 0.009 degrees.

    make_pair's OWN target is not a rigid copy: it is an independent sample of the surface (noise = 0 only leaves out the
    jitter), and the loss's minimum on such a pair is not at the generating rotation.  Measured on make_pair(21, 512, 512,
    noise=0, rot_deg=5), 300 epochs: started AT the generating rotation the Newton loop walks away to 2.5 .. 4.8 degrees within
    20 epochs and stays there, like the same loop started at the identity (3.2 .. 4.7) and like PairRegistration (1.8 .. 4.8,
    3.48 at epoch 40 against the Newton loop's 3.85); all three end at the same Chamfer distance (0.00428 .. 0.00435).  The
    angle to the generating rotation says nothing about either optimiser there, hence the rigid copy."""
    from rrl_hip import register, synth
    seed, n = 21, 512
    pr = synth.make_pair(seed, n, n, noise=0.0, rot_deg=5.0)
    rng = np.random.default_rng(seed)          # make_pair's own stream: two surfaces, then the axis
    synth._surface(rng, n); synth._surface(rng, n)
    Rot = synth._rotation(rng.standard_normal(3), 5.0)     # tar = src Rot^T + t: the row-convention pose is R = Rot^T
    copy = pr["src"].astype(np.float64) @ Rot.T + np.array([0.05, -0.03, 0.02])
    copy = (copy - copy.mean(0)).astype(np.float32)
    src = torch.from_numpy(pr["src_tri"]).cuda().reshape(1, n, 9)
    tar = torch.from_numpy(synth.knn_triangles(copy)).cuda().reshape(1, n, 9)

    def angle_error(R):
        d = R[0].double().cpu().numpy() @ Rot          # R Rot = R (Rot^T)^T
        return float(np.degrees(np.arccos(np.clip((np.trace(d) - 1.0) / 2.0, -1.0, 1.0))))
    first = register.PairRegistration(src, tar, 4000, seed=9)
    first.run(40)
    second = newton.NewtonRegistration(src, tar, 4000, seed=9, patience=0)
    second.run(40)
    e1, e2 = angle_error(first.R), angle_error(second.R)
    print(f"rotation-angle error after 40 epochs (start 5 degrees): PairRegistration {e1:.4f}, NewtonRegistration {e2:.4f} degrees")
    assert int(second.state[0, 0]) == 40 and int(second.state[0, 3]) == NR.STEPPED
    assert e2 < e1, (e1, e2)
    third = newton.NewtonRegistration(src, tar, 4000, seed=9)
    third.run(200, check_every=5)
    print(f"stopping rule: done_epoch {third.done_epoch.tolist()} after {third.epochs} epochs issued, error {angle_error(third.R):.4f} degrees, "
          f"last step {third.last_step.tolist()}")
    assert third.epochs < 200 and third.epochs % 5 == 0 and bool((third.done_epoch >= 0).all())
    R, T, hist = newton.register_pairs_newton(src, tar, 4000, n_epoch=2, seed=9)
    assert R.shape == (1, 3, 3) and T.shape == (1, 3) and [len(h) for h in hist] == [2]
