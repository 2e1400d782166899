"""The float64 twin of the Sinkhorn soft assignment (tests/sinkhorn_refs.py) against the reference's own run
(tests/golden/sinkhorn_rpm.npz, recorded from rpm/models/rpmnet.py sinkhorn and the lines 214-222 by make_golden_sinkhorn.py)
and against float64 autograd of the restated padded formulation; the new entries in the header and the binding; and every
refusal that needs no GPU -- the Python layer's and the C entries' (fake pointers: nothing is launched)."""
import ctypes

import numpy as np
import pytest
import torch

import sinkhorn_refs as SR
from conftest import load_golden

FAKE = 0x1000  # a non-NULL, 8-byte aligned pointer that is never dereferenced
E_ARG, E_WS = -1, -3

# the shapes of the GPU tests (tests/test_gpu_sinkhorn.py): one and two entries, both sides of the 64-lane wavefront and of the
# 64-column tile, more than one 128-row slice of a column pass (257, 1025), more than one 256-column round of a row pass (1025)
SHAPES = [(1, 1), (2, 3), (63, 65), (64, 64), (65, 63), (257, 130), (1025, 70), (70, 1025)]
ITERS = [0, 1, 5]
SIGMAS = [3.0, 30.0]
A_MAX_NOITER = 80.0  # n_iters = 0 is P = exp(A): float32 outputs hold it up to exp(88), so these entries are clamped


def make_inputs(seed, B, J, K, sigma, n_iters):
    """log_alpha ~ N(0, sigma^2) (B, J, K), xyz_ref uniform in the unit cube, upstream gW, gs, gc ~ N(0, 1); all float32."""
    rs = np.random.default_rng(seed)
    A = (sigma * rs.standard_normal((B, J, K))).astype(np.float32)
    if n_iters == 0:
        A = np.clip(A, -A_MAX_NOITER, A_MAX_NOITER)
    x = rs.uniform(-1.0, 1.0, (B, K, 3)).astype(np.float32)
    g = [rs.standard_normal(s).astype(np.float32) for s in ((B, J, 3), (B, J), (B, K))]
    return A, x, g


@pytest.fixture(scope="module")
def golden():
    return load_golden("sinkhorn_rpm.npz")


def test_twin_reproduces_the_reference_run(golden):
    """Both are float64 on the same inputs: forward within 1e-12 (absolute for log_perm, relative to max(1, largest entry)
    for the sums), gradients within 1e-11 of the sample's largest entry."""
    names = [str(c) for c in golden["cases"]]
    assert len(names) == 5
    for name in names:
        A, x = golden[f"{name}_log_alpha"], golden[f"{name}_xyz_ref"]
        slack, n = (int(v) for v in golden[f"{name}_spec"])
        f = SR.forward(A, x, n, bool(slack))
        for key in ("log_perm", "W", "s", "c"):
            want = golden[f"{name}_{key}"]
            assert np.abs(f[key] - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (name, key)
        g = SR.backward(A, x, golden[f"{name}_CW"], golden[f"{name}_Cs"], golden[f"{name}_Cc"], n, bool(slack), fwd=f)
        for b in range(A.shape[0]):
            for mine, key in ((g["dA"], "gA"), (g["gx"], "gx")):
                want = golden[f"{name}_{key}"][b]
                assert np.abs(mine[b] - want).max() <= 1e-11 * np.abs(want).max(), (name, key, b)
            assert (np.abs(g["dA"][b]) <= g["dA_abs"][b] * (1 + 1e-12)).all() and (np.abs(g["gx"][b]) <= g["gx_abs"][b] * (1 + 1e-12)).all()
        tr, W, s, c = SR.rpm_head(A, golden[f"{name}_xyz_src"], x, n, bool(slack))
        if A.shape[1] >= 3:  # (one point has no rotation: the recorded gap says so)
            assert (golden[f"{name}_gap"] >= 1e-3).all(), name
            want = golden[f"{name}_transform"]
            assert np.abs(tr.numpy() - want).max() <= 1e-10 * max(1.0, np.abs(want).max()), name


@pytest.mark.parametrize("J,K", SHAPES)
def test_twin_against_float64_autograd_of_the_padded_formulation(J, K):
    for i, (slack, n) in enumerate((s, n) for s in (True, False) for n in ITERS):
        sigma = SIGMAS[i % 2]
        A, x, g = make_inputs(7 * J + K + i, 2, J, K, sigma, n)
        f = SR.forward(A, x, n, slack)
        bw = SR.backward(A, x, *g, n, slack, fwd=f)
        lp, W, s, c, dA, gx = SR.padded_torch_grads(A, x, *g, n, slack)
        for mine, want, key in ((f["log_perm"], lp, "log_perm"), (f["W"], W, "W"), (f["s"], s, "s"), (f["c"], c, "c")):
            assert np.abs(mine - want).max() <= 1e-11 * max(1.0, np.abs(want).max()), (slack, n, key)
        for b in range(2):
            # (a cancelling sum -- without slack the outputs barely depend on A --: judged by the sample's largest sum |terms|)
            assert np.abs(bw["dA"][b] - dA[b]).max() <= 1e-11 * bw["dA_abs"][b].max(), (slack, n, b)
            assert np.abs(bw["gx"][b] - gx[b]).max() <= 1e-11 * bw["gx_abs"][b].max(), (slack, n, b)


def test_minus_infinity_entries_are_legal_with_slack():
    A, x, g = make_inputs(3, 1, 6, 5, 3.0, 5)
    A[0, 2, :] = -np.inf  # a whole row: only its slack entry is left
    A[0, 0, 1] = A[0, 4, 4] = -np.inf
    f = SR.forward(A, x, 5, True)
    assert f["P"][0, 2].max() == 0.0 and f["P"][0, 0, 1] == 0.0 and np.isfinite(f["s"]).all() and np.isfinite(f["W"]).all()


# ---- the C entries ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from rrl_hip import _lib, build
    build.build_lib()
    return _lib.load()


def sinkhorn_args(lib, **over):
    from rrl_hip import _lib
    k = _lib.SinkhornArgs()
    base = dict(struct_bytes=ctypes.sizeof(k), B=2, J=300, K=200, n_iters=5, slack=1, log_alpha=FAKE, xyz_ref=FAKE, count_src=None,
                count_ref=None, eps=1e-5, ws=FAKE, ws_bytes=int(lib.rrl_sinkhorn_workspace_bytes(2, 300, 200, 5)), W=FAKE, s=FAKE,
                c=FAKE, log_perm=None, info=FAKE)
    base.update(over)
    for name, v in base.items():
        setattr(k, name, v)
    return k


SINKHORN_REFUSALS = [dict(log_alpha=None), dict(xyz_ref=None), dict(ws=None), dict(W=None), dict(s=None), dict(c=None), dict(info=None),
                     dict(B=0), dict(B=-1), dict(B=32768), dict(J=0), dict(K=0), dict(J=16385), dict(K=16385), dict(n_iters=-1),
                     dict(n_iters=65), dict(struct_bytes=8), dict(ws=FAKE + 4)]


def test_c_refusals_return_their_codes_without_a_launch(lib):
    bwd = lambda k, gA=FAKE: lib.rrl_sinkhorn_bwd(ctypes.byref(k), None, None, None, gA, None, None)  # noqa: E731
    assert lib.rrl_sinkhorn_fwd(None, None) == E_ARG and lib.rrl_sinkhorn_bwd(None, None, None, None, FAKE, None, None) == E_ARG
    for over in SINKHORN_REFUSALS:
        assert lib.rrl_sinkhorn_fwd(ctypes.byref(sinkhorn_args(lib, **over)), None) == E_ARG, over
        assert bwd(sinkhorn_args(lib, **over)) == E_ARG, over
    assert bwd(sinkhorn_args(lib), None) == E_ARG  # (no g_log_alpha)
    short = int(lib.rrl_sinkhorn_workspace_bytes(2, 300, 200, 5)) - 1
    assert lib.rrl_sinkhorn_fwd(ctypes.byref(sinkhorn_args(lib, ws_bytes=short)), None) == E_WS
    assert bwd(sinkhorn_args(lib, ws_bytes=short)) == E_WS
    assert lib.rrl_sinkhorn_fwd(ctypes.byref(sinkhorn_args(lib, n_iters=6)), None) == E_WS  # (one more iteration: a longer history)
    # the size: potentials and adjoints (n + 1) (J + K) doubles each, s, N, the row scalars (8 J), 4 per column and 128-row slice
    assert lib.rrl_sinkhorn_workspace_bytes(2, 300, 200, 5) == 8 * 2 * (2 * 6 * 500 + 8 * 300 + 4 * 3 * 200)
    assert lib.rrl_sinkhorn_workspace_bytes(1, 1, 1, 0) == 8 * (2 * 2 + 8 + 4)
    for shape in ((0, 5, 5, 5), (32768, 5, 5, 5), (1, 0, 5, 5), (1, 5, 16385, 5), (1, 5, 5, 65), (1, 5, 5, -1)):
        assert lib.rrl_sinkhorn_workspace_bytes(*shape) == 0, shape


def test_entries_in_the_header_and_the_binding(lib):
    from rrl_hip import callsites, sinkhorn
    assert callable(sinkhorn.soft_assign) and callable(callsites.rpm_soft_correspondences) and callable(callsites.rpm_match_head)
    assert (sinkhorn.MAX_B, sinkhorn.MAX_DIM, sinkhorn.MAX_ITERS) == (32767, 16384, 64)


def test_python_refusals_need_no_gpu():
    from rrl_hip import sinkhorn
    ok = ((2, 8, 6), (2, 6, 3))
    sinkhorn.check_request(*ok)
    sinkhorn.check_request(*ok, 0, 0.0, (2,), (2,))
    for args, match in ((((2, 8, 6), (3, 6, 3)), "same B"), (((8, 6), (6, 3)), "same B"), (((2, 8, 6), (2, 7, 3)), "one point per column"),
                        (((2, 8, 6), (2, 6, 4)), "one point per column"), (((40000, 8, 6), (40000, 6, 3)), "32767"),
                        (((0, 8, 6), (0, 6, 3)), "32767"), (((1, 0, 6), (1, 6, 3)), "16384"), (((1, 16385, 6), (1, 6, 3)), "16384"),
                        ((*ok, -1), "n_iters"), ((*ok, 65), "n_iters"), ((*ok, 2.5), "n_iters"), ((*ok, 5, -1.0), "eps"),
                        ((*ok, 5, 1e-5, (3,)), "counts_src"), ((*ok, 5, 1e-5, None, (2, 1)), "counts_ref"),
                        ((*ok, 5, 1e-5, None, None, 1e-3), "early termination")):
        with pytest.raises(ValueError, match=match):
            sinkhorn.check_request(*args)
    with pytest.raises(TypeError):
        sinkhorn.soft_assign(np.zeros((1, 4, 3)), torch.zeros(1, 3, 3))
    with pytest.raises(ValueError, match="early termination"):
        sinkhorn.soft_assign(torch.zeros(1, 4, 3), torch.zeros(1, 3, 3), early_stop_eps=1e-4)
    with pytest.raises(ValueError, match=r"\[0, 4\]"):
        sinkhorn.soft_assign(torch.zeros(1, 4, 3), torch.zeros(1, 3, 3), counts_src=[5])
    with pytest.raises(ValueError, match="one point per column"):
        sinkhorn.soft_assign(torch.zeros(1, 4, 3), torch.zeros(1, 4, 3))


@pytest.mark.skipif(torch.cuda.is_available(), reason="the refusal of a machine without a GPU")
def test_without_a_gpu_the_call_raises():
    from rrl_hip import callsites, sinkhorn
    from rrl_hip._lib import RRLError
    with pytest.raises(RRLError):
        sinkhorn.soft_assign(torch.zeros(1, 4, 3), torch.zeros(1, 3, 3))
    with pytest.raises(RRLError):
        callsites.rpm_match_head(torch.zeros(1, 4, 3), torch.zeros(1, 4, 3), torch.zeros(1, 3, 3))


def test_without_the_library_the_call_raises(monkeypatch, tmp_path):
    from rrl_hip import _lib, ops, sinkhorn
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB", str(tmp_path / "absent.so"))
    monkeypatch.setattr(ops, "_home", lambda *a: torch.device("cpu"))
    monkeypatch.setattr(ops, "_prep", lambda t, *a: t.detach())
    with pytest.raises(_lib.RRLError, match="missing"):
        sinkhorn.soft_assign(torch.zeros(1, 4, 3), torch.zeros(1, 3, 3))
