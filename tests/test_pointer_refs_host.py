"""The host twin of the softmax pointer (tests/pointer_refs.py): its numpy fmaf against exact rational arithmetic, its chain
against the worst-case bound, its float64 head against the reference's own run (tests/golden/pointer_dcp.npz, recorded from
dcp/model.py SVDHead.forward by make_golden_pointer_dcp.py) and against float64 autograd of the reference formulation; the
new entries in the header and the binding; and every refusal that needs no GPU -- the Python layer's and the C entries' (fake
pointers: nothing is launched)."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import pointer_refs as PR
from conftest import load_golden

FAKE = 0x1000  # a non-NULL, 8-byte aligned pointer that is never dereferenced
E_ARG, E_WS = -1, -3
F32 = np.float32


def round_fraction_to_f32(q):
    """The float32 nearest to the rational q, ties to the even significand, decided in exact arithmetic."""
    f = F32(float(q))  # within one float32 step of the answer
    cands = [np.nextafter(f, F32(-np.inf)), f, np.nextafter(f, F32(np.inf))]
    best = min(cands, key=lambda c: (abs(Fraction(float(c)) - q), int(c.view(np.uint32)) & 1))
    return best


def tie_case():
    """(2, 5, 3, 4): small dyadic values whose products and sums meet float32 ties all the time, and in entry (0, 0) of sample
    0 the construction double rounding gets wrong: after channel 0 the chain is 2^40 + 2^17 (an odd significand), channel 1
    adds 2^16 (1 - 2^-46): the float64 sum is exactly the tie 2^40 + 2^17 + 2^16, the true value lies below it."""
    rs = np.random.default_rng(5)
    se = (rs.integers(-4096, 4097, (2, 5, 3)) * 2.0 ** -6 + rs.integers(0, 2, (2, 5, 3)) * 2.0 ** 17).astype(F32)
    te = (rs.integers(-4096, 4097, (2, 5, 4)) * 2.0 ** -7 + rs.integers(0, 2, (2, 5, 4)) * (1.0 + 2.0 ** -23)).astype(F32)
    se[0, 0, 0], te[0, 0, 0] = 2.0 ** 20, 2.0 ** 20 + 2.0 ** -3
    se[0, 1, 0], te[0, 1, 0] = 2.0 ** 8 * (1 + 2.0 ** -23), 2.0 ** 8 * (1 - 2.0 ** -23)
    se[0, 2:, 0] = 0.0
    return se, te


def test_numpy_fmaf_is_exact_against_rational_arithmetic():
    se, te = tie_case()
    assert se.shape == (2, 5, 3) and te.shape == (2, 5, 4)
    naive_differs = 0
    for b in range(2):
        got = PR.chains(se[b], te[b])
        for j in range(3):
            for k in range(4):
                acc, naive = F32(0.0), F32(0.0)
                for c in range(5):
                    acc = round_fraction_to_f32(Fraction(float(se[b, c, j])) * Fraction(float(te[b, c, k])) + Fraction(float(acc)))
                    naive = F32(np.float64(se[b, c, j]) * np.float64(te[b, c, k]) + np.float64(naive))
                assert got[j, k].tobytes() == acc.tobytes(), (b, j, k, got[j, k], acc)
                naive_differs += int(naive != acc)
    # the constructed tie: the exact chain keeps 2^40 + 2^17, rounding the float64 sum again would give 2^40 + 2^18
    assert PR.chains(se[0], te[0])[0, 0] == F32(2.0 ** 40 + 2.0 ** 17)
    assert F32(np.float64(se[0, 1, 0]) * np.float64(te[0, 1, 0]) + np.float64(F32(2.0 ** 40 + 2.0 ** 17))) == F32(2.0 ** 40 + 2.0 ** 18)
    assert naive_differs >= 1
    # single operations: both directions, both signs
    one, h = F32(2.0 ** 8 * (1 + 2.0 ** -23)), F32(2.0 ** 8 * (1 - 2.0 ** -23))
    for sign in (1.0, -1.0):
        c = F32(sign * (2.0 ** 40 + 2.0 ** 17))
        assert PR.fmaf32(F32(sign) * one, h, c) == c
        assert PR.fmaf32(F32(sign * 2.0 ** 8), F32(2.0 ** 8), c) == F32(sign * (2.0 ** 40 + 2.0 ** 18))  # (the true tie: to even)
        # (1 + 2^-11) (1 - 2^-11 + 2^-22) = 1 + 2^-33: 2^36 + 8 on top of 2^60 -- the float64 sum is the tie 2^60 + 2^36, the
        # true value lies above it, and the even neighbour is the wrong one
        a, b2 = F32(sign * 2.0 ** 18 * (1 + 2.0 ** -11)), F32(2.0 ** 18 * (1 - 2.0 ** -11 + 2.0 ** -22))
        assert np.float64(a) * np.float64(b2) == sign * (2.0 ** 36 + 8.0)
        assert PR.fmaf32(a, b2, F32(sign * 2.0 ** 60)) == F32(sign * (2.0 ** 60 + 2.0 ** 37))
        assert F32(np.float64(a) * np.float64(b2) + np.float64(F32(sign * 2.0 ** 60))) == F32(sign * 2.0 ** 60)


@pytest.mark.parametrize("C", [64, 512])
def test_chain_within_the_worst_case_bound(C):
    """|chain - exact| <= 1.001 C 2^-24 sum |a b|: C roundings, each at most half an ulp of a partial sum that sum |a b| bounds."""
    se, te, _, _ = PR.make_case(C, 17, 19, 1, 1.0, "random", seed=3)
    got = PR.chains(se[0], te[0]).astype(np.float64)
    a, b = se[0].astype(np.float64), te[0].astype(np.float64)
    bound = 1.001 * C * PR.U24 * (np.abs(a).T @ np.abs(b))
    err = np.abs(got - a.T @ b)
    assert (err <= bound).all(), (err / bound).max()
    assert err.max() > 0.0


@pytest.fixture(scope="module")
def golden():
    return load_golden("pointer_dcp.npz")


CASES = {"b2_c64_65x70": (2, 64, 65, 70), "b1_c512_33x40": (1, 512, 33, 40), "b2_c33_64x64_s4": (2, 33, 64, 64)}


def recorded_corr_bound(se, te, x, tw):
    """2 E_j max_k |x_k - corr_j| + 2^-23 |corr_j| of one sample: E_j the row's largest worst-case score bound, scaled."""
    C = se.shape[0]
    E = (1.001 * C * PR.U24 * (np.abs(se.astype(np.float64)).T @ np.abs(te.astype(np.float64))) * float(PR.scale(C))).max(1)
    dev = np.abs(x.astype(np.float64)[:, None, :] - tw["corr"][:, :, None]).max(2)
    return 2 * E[None, :] * dev + PR.U23 * np.abs(tw["corr"])


def test_twin_head_against_the_reference_recording(golden):
    names = [str(c) for c in golden["cases"]]
    assert names == list(CASES)
    for name in names:
        se, te, x, want = (golden[f"{name}_{k}"] for k in ("src_emb", "tgt_emb", "tgt", "src_corr"))
        assert se.shape == CASES[name][:3] and te.shape == (CASES[name][0], CASES[name][1], CASES[name][3])
        assert (golden[f"{name}_gap"] >= 1e-2).all()
        for b in range(se.shape[0]):
            tw = PR.head(PR.scores(se[b], te[b]), x[b])
            err = np.abs(tw["corr"] - want[b])
            bound = recorded_corr_bound(se[b], te[b], x[b], tw)
            assert (err <= bound).all(), (name, b, (err / bound).max())


@pytest.mark.parametrize("shape", [(5, 7, 9), (64, 33, 40), (33, 20, 12)])
def test_twin_formulas_against_float64_autograd_of_the_reference_formulation(shape):
    C, N, M = shape
    se, te, x, g = PR.make_case(C, N, M, 1, 2.0, "random", seed=11)
    t = [torch.tensor(v[0].astype(np.float64), requires_grad=True) for v in (se, te, x)]
    sc = torch.softmax(torch.matmul(t[0].transpose(1, 0).contiguous(), t[1]) / math.sqrt(C), dim=1)
    corr = torch.matmul(t[2], sc.transpose(1, 0).contiguous())
    (corr * torch.tensor(g[0].astype(np.float64))).sum().backward()
    zd = se[0].astype(np.float64).T @ te[0].astype(np.float64) / np.sqrt(np.float64(C))
    tw = PR.head(zd, x[0], g=g[0], src_emb=se[0], tgt_emb=te[0], sc=1.0 / np.sqrt(np.float64(C)))
    assert np.abs(tw["corr"] - corr.detach().numpy()).max() <= 1e-12
    assert np.abs(PR.exact(se[0], te[0], x[0]) - corr.detach().numpy()).max() <= 1e-12
    for mine, want in ((tw["d_src_emb"], t[0].grad), (tw["d_tgt_emb"], t[1].grad), (tw["d_tgt"], t[2].grad)):
        assert np.abs(mine - want.numpy()).max() <= 1e-12 * max(1.0, np.abs(want.numpy()).max())
    for name in ("d_src_emb", "d_tgt_emb", "d_tgt"):
        assert (np.abs(tw[name]) <= tw["abs_" + name] * (1 + 1e-12)).all()


def test_case_generator_kinds():
    for kind in PR.KINDS:
        se, te, x, g = PR.make_case(8, 6, 40, 2, 1.0, kind, seed=1)
        assert se.shape == (2, 8, 6) and te.shape == (2, 8, 40) and x.shape == (2, 3, 40) and g.shape == (2, 3, 6)
        assert all(v.dtype == np.float32 for v in (se, te, x, g))
        z = PR.scores(se[0], te[0]).astype(np.float64)
        if kind == "ascending":
            assert (np.diff(z, axis=1) > 0).all()
        elif kind == "one_hot":
            top = np.sort(z, axis=1)
            assert (top[:, -1] - top[:, -2] > 100).all()
        elif kind == "equal":
            assert (z == z[0, 0]).all()


# ---- the C entries ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from rrl_hip import _lib, build
    build.build_lib()
    return _lib.load()


def fwd_args(lib, **over):
    B, C, N, M = (over.pop(k, v) for k, v in (("B", 2), ("C", 64), ("N", 300), ("M", 200)))
    base = dict(src_emb=FAKE, tgt_emb=FAKE, tgt=FAKE, count_src=None, count_tgt=None, ws=FAKE,
                ws_bytes=int(lib.rrl_pointer_workspace_bytes(2, 64, 300, 200)), corr=FAKE, scores=None, info=None)
    base.update(over)
    return (*base.values(), B, C, N, M, None)


def bwd_args(lib, **over):
    B, C, N, M = (over.pop(k, v) for k, v in (("B", 2), ("C", 64), ("N", 300), ("M", 200)))
    base = dict(src_emb=FAKE, tgt_emb=FAKE, tgt=FAKE, count_src=None, count_tgt=None, ws=FAKE,
                ws_bytes=int(lib.rrl_pointer_workspace_bytes(2, 64, 300, 200)), g_corr=FAKE, d_src_emb=None, d_tgt_emb=None, d_tgt=None)
    base.update(over)
    return (*base.values(), B, C, N, M, None)


SHARED_REFUSALS = [dict(src_emb=None), dict(tgt_emb=None), dict(tgt=None), dict(ws=None), dict(B=-1), dict(B=32768), dict(C=0),
                   dict(C=1025), dict(N=0), dict(M=0), dict(N=16385), dict(M=16385)]


def test_c_refusals_return_their_codes_without_a_launch(lib):
    for over in SHARED_REFUSALS:
        assert lib.rrl_pointer_fwd(*fwd_args(lib, **dict(over))) == E_ARG, over
        assert lib.rrl_pointer_bwd(*bwd_args(lib, **dict(over))) == E_ARG, over
    assert lib.rrl_pointer_fwd(*fwd_args(lib, corr=None)) == E_ARG
    assert lib.rrl_pointer_bwd(*bwd_args(lib, g_corr=None)) == E_ARG
    short = int(lib.rrl_pointer_workspace_bytes(2, 64, 300, 200)) - 1
    for over in (dict(ws_bytes=short), dict(ws=FAKE + 4)):
        assert lib.rrl_pointer_fwd(*fwd_args(lib, **over)) == E_WS, over
        assert lib.rrl_pointer_bwd(*bwd_args(lib, **over)) == E_WS, over
    assert lib.rrl_pointer_fwd(*fwd_args(lib, B=0)) == 0 and lib.rrl_pointer_bwd(*bwd_args(lib, B=0)) == 0  # (no launch)


def test_workspace_holds_vectors_only(lib):
    """Per-row and per-slice vectors: below one eighth of one (B, N, M) float32 matrix at (8, 512, 2048, 2048), linear in B and
    N, stepping with the slices of M, independent of C; 0 for a shape that is refused."""
    from rrl_hip import _abi
    slice_ = _abi.CONSTANTS["RRL_POINTER_SLICE"]
    size = lib.rrl_pointer_workspace_bytes
    assert 0 < size(8, 512, 2048, 2048) < 8 * 2048 * 2048 * 4 // 8
    assert size(8, 512, 2048, 2048) == size(8, 1, 2048, 2048) == 8 * size(1, 512, 2048, 2048) == 2 * size(8, 512, 1024, 2048)
    assert size(1, 8, 100, slice_) == size(1, 8, 100, 1) < size(1, 8, 100, slice_ + 1) == size(1, 8, 100, 2 * slice_)
    assert size(3, 8, 100, 3 * slice_) % 8 == 0
    for shape in ((-1, 5, 5, 5), (32768, 5, 5, 5), (1, 0, 5, 5), (1, 1025, 5, 5), (1, 5, 0, 5), (1, 5, 16385, 5), (1, 5, 5, 0), (1, 5, 5, 16385)):
        assert size(*shape) == 0, shape


def test_entries_in_the_header_and_the_binding(lib):
    from rrl_hip import _abi, _lib, callsites, pointer
    for name in ("rrl_pointer_workspace_bytes", "rrl_pointer_fwd", "rrl_pointer_bwd"):
        assert name in _abi.PROTOS and name in _lib.EXPORTS and hasattr(lib, name)
    assert not any("pointer" in s for s in _abi.STRUCTS)
    assert len(_abi.PROTOS["rrl_pointer_fwd"][1]) == 15 and len(_abi.PROTOS["rrl_pointer_bwd"][1]) == 16
    assert callable(pointer.soft_pointer) and callable(callsites.dcp_soft_pointer) and callable(callsites.dcp_svd_head)
    assert (pointer.MAX_B, pointer.MAX_DIM, pointer.MAX_C) == (32767, 16384, 1024) and pointer.SLICE % 64 == 0


def test_python_refusals_need_no_gpu():
    from rrl_hip import pointer
    ok = ((2, 16, 8), (2, 16, 6), (2, 3, 6))
    pointer.check_request(*ok)
    pointer.check_request(*ok, (2,), (2,))
    for args, match in ((((2, 16, 8), (3, 16, 6), (2, 3, 6)), "B and C"), (((2, 16, 8), (2, 15, 6), (2, 3, 6)), "B and C"),
                        (((16, 8), (16, 6), (3, 6)), "channel-first"), (((2, 16, 8), (2, 16, 6), (2, 3, 7)), "one point per column"),
                        (((2, 16, 8), (2, 16, 6), (2, 6, 3)), "one point per column"),
                        (((40000, 16, 8), (40000, 16, 6), (40000, 3, 6)), "32767"), (((0, 16, 8), (0, 16, 6), (0, 3, 6)), "32767"),
                        (((1, 0, 8), (1, 0, 6), (1, 3, 6)), "1024"), (((1, 1025, 8), (1, 1025, 6), (1, 3, 6)), "1024"),
                        (((1, 4, 0), (1, 4, 6), (1, 3, 6)), "16384"), (((1, 4, 8), (1, 4, 16385), (1, 3, 16385)), "16384"),
                        ((*ok, (3,)), "counts_src"), ((*ok, None, (2, 1)), "counts_tgt")):
        with pytest.raises(ValueError, match=match):
            pointer.check_request(*args)
    with pytest.raises(TypeError):
        pointer.soft_pointer(np.zeros((1, 4, 3)), torch.zeros(1, 4, 3), torch.zeros(1, 3, 3))
    with pytest.raises(ValueError, match=r"\[0, 5\]"):
        pointer.soft_pointer(torch.zeros(1, 4, 5), torch.zeros(1, 4, 3), torch.zeros(1, 3, 3), counts_src=[6])
    with pytest.raises(ValueError, match="one point per column"):
        pointer.soft_pointer(torch.zeros(1, 4, 5), torch.zeros(1, 4, 3), torch.zeros(1, 3, 4))


@pytest.mark.skipif(torch.cuda.is_available(), reason="the refusal of a machine without a GPU")
def test_without_a_gpu_the_call_raises():
    from rrl_hip import callsites, pointer
    from rrl_hip._lib import RRLError
    with pytest.raises(RRLError):
        pointer.soft_pointer(torch.zeros(1, 4, 5), torch.zeros(1, 4, 3), torch.zeros(1, 3, 3))
    with pytest.raises(RRLError):
        callsites.dcp_svd_head(torch.zeros(1, 4, 5), torch.zeros(1, 4, 3), torch.zeros(1, 3, 5), torch.zeros(1, 3, 3))


def test_without_the_library_the_call_raises(monkeypatch, tmp_path):
    from rrl_hip import _lib, ops, pointer
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB", str(tmp_path / "absent.so"))
    monkeypatch.setattr(ops, "_home", lambda *a: torch.device("cpu"))
    monkeypatch.setattr(ops, "_prep", lambda t, *a: t.detach())
    with pytest.raises(_lib.RRLError, match="missing"):
        pointer.soft_pointer(torch.zeros(1, 4, 5), torch.zeros(1, 4, 3), torch.zeros(1, 3, 3))
