"""The host twin of the attention node (tests/attention_refs.py): its chains against exact rational arithmetic on a case built
to meet rounding ties, its float64 evaluation against the reference's own run (tests/golden/attention_dcp*.npz, recorded from
dcp/model.py by make_golden_attention.py, in float32 and float64), its gradient formulas against the recorded float64 autograd;
the new entries in the header and the binding; every refusal that needs no GPU -- the Python layer's and the C entries' (fake
pointers: nothing is launched); and the modules' state_dict keys against the recorded ones."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import attention_refs as AR
from conftest import load_golden
from test_pointer_refs_host import round_fraction_to_f32, tie_case

FAKE = 0x1000  # a non-NULL, 16-byte aligned pointer that is never dereferenced
E_ARG, E_WS = -1, -3
F32, F64 = np.float32, np.float64

# name -> (B, H, DK, N, M)
CASES = {"b2_h4_dk16_33x40": (2, 4, 16, 33, 40), "b1_h4_dk128_65x70": (1, 4, 128, 65, 70), "b2_h3_dk11_64x64": (2, 3, 11, 64, 64)}
# The Transformer's tolerance against its recording, in units of the recording's own float32-to-float64 distance.  The module
# is torch's float32 layers around six attention nodes; the recording's float32 run is the same layers around eager float32
# attention, and DESIGN section 27 measures the node's error against float64 at 0.7 .. 1.7 x eager float32's.  A float32 run that
# differs from the recorded one only in rounding therefore lies within about 1.7 distances of the float64 run and 2.7 of the
# float32 run; measured on the CPU with the twin (forward_rule) in the place of the node: 1.00 and 0.84.  4 leaves room
# for the GPU's own sum orders in the Linear layers and is far below what a wrong head, key or layer gives (> 1e4).
TRANSFORMER_FACTOR = 4.0


def recorded(g, name):
    """(float32 run, float64 run, distance) of one recorded result."""
    x = g[name]
    return x, x.astype(F64) + g[name + "_lo"].astype(F64), float(g[name + "_dist"])


@pytest.fixture(scope="module")
def golden():
    files = [load_golden(n) for n in ("attention_dcp.npz", "attention_dcp_dk128_fwd.npz", "attention_dcp_dk128_bwd.npz")]
    return {k: f[k] for f in files for k in f.files}


def test_chains_are_exact_against_rational_arithmetic_on_token_major_heads():
    """Two heads of five channels from pointer_refs' tie case, laid out token-major: the score chain runs over a head's OWN
    channels ascending, and the column chain of o over k ascending, each one rounding per step."""
    se, te = tie_case()                                   # (2, 5, 3), (2, 5, 4): sample -> head
    q = np.ascontiguousarray(se.transpose(2, 0, 1).reshape(3, 10))
    k = np.ascontiguousarray(te.transpose(2, 0, 1).reshape(4, 10))
    z = AR.scores(q, k, 2)
    sc = AR.scale(5)
    assert sc == F32(1.0 / np.sqrt(5.0))
    for h in range(2):
        for j in range(3):
            for c in range(4):
                acc = F32(0.0)
                for ch in range(5):
                    acc = round_fraction_to_f32(Fraction(float(q[j, 5 * h + ch])) * Fraction(float(k[c, 5 * h + ch])) + Fraction(float(acc)))
                assert z[h, j, c].tobytes() == F32(acc * sc).tobytes(), (h, j, c)
    assert z[0, 0, 0] == F32(F32(2.0 ** 40 + 2.0 ** 17) * sc)   # (the constructed tie of pointer_refs, not 2^40 + 2^18)
    # the column chain: weights and values on a dyadic grid that meets ties, checked through forward_rule
    rs = np.random.default_rng(3)
    zz = (rs.integers(-8, 1, (2, 3, 6))).astype(F32)
    zz[:, :, 2] = 0.0
    v = (rs.integers(-4096, 4097, (6, 10)) * 2.0 ** -6 + rs.integers(0, 2, (6, 10)) * 2.0 ** 17).astype(F32)
    got = AR.forward_rule(zz, v, 2)
    for h in range(2):
        for j in range(3):
            p = np.exp((zz[h, j] - zz[h, j].max()).astype(F32)).astype(F32)
            half = (np.arange(6) >> 2) & 1
            L = float(np.sum([float(x) for x in p[half == 0]])) + float(np.sum([float(x) for x in p[half == 1]]))
            assert got["L"][h, j] == L and got["rowmax"][h, j] == 0.0
            for c in range(5):
                acc = F32(0.0)
                for kk in range(6):
                    acc = round_fraction_to_f32(Fraction(float(p[kk])) * Fraction(float(v[kk, 5 * h + c])) + Fraction(float(acc)))
                assert got["out"][j, 5 * h + c].tobytes() == F32(F64(acc) / L).tobytes(), (h, j, c)


def score_move(E, v, H, out):
    """|out(z + dz) - out(z)| for |dz| <= E: 2 max_k E_jk max_k |v_kc - out_jc| (the mean of dz drops out of a softmax, each
    weight moves by at most twice the largest relative move), for E << 1."""
    vh, oh = AR.heads(v, H).astype(F64), AR.heads(out, H)
    dev = np.abs(vh[:, None, :, :] - oh[:, :, None, :]).max(2)
    return AR.merge(2 * E.max(2)[:, :, None] * dev) * 1.001


def test_twin_against_the_reference_recording(golden):
    assert [str(c) for c in golden["cases"]] == list(CASES)
    for name, (B, H, DK, N, M) in CASES.items():
        q, k, v = (golden[f"{name}_{x}"] for x in "qkv")
        o32, o64, dist = recorded(golden, f"{name}_out")
        assert q.shape == (B, N, H * DK) and k.shape == v.shape == (B, M, H * DK) and o32.shape == (B, N, H * DK)
        worst = 0.0
        for b in range(B):
            z = AR.scores(q[b], k[b], H)
            assert (np.abs(z.astype(F64) - AR.exact_scores(q[b], k[b], H)) <= AR.score_bound(q[b], k[b], H)).all()
            ev = AR.evaluate(z, v[b], H)
            move = score_move(AR.score_bound(q[b], k[b], H), v[b], H, ev["out"])
            err = np.abs(ev["out"] - o64[b])
            assert (err <= move + 1e-14).all(), (name, b, (err / move).max())
            rule = AR.forward_rule(z, v[b], H)["out"].astype(F64)
            assert (np.abs(rule - ev["out"]) <= ev["out_bound"]).all(), (name, b, "the rule against its own float64 evaluation")
            assert (np.abs(rule - o32[b]) <= ev["out_bound"] + move + dist).all(), (name, b, "against the float32 recording")
            worst = max(worst, float((np.abs(rule - ev["out"]) / ev["out_bound"]).max()))
        print(name, "rule / bound", round(worst, 3), "recording's float32-to-float64 distance", dist)


def test_gradient_formulas_against_the_recorded_float64_autograd(golden):
    """evaluate on exact float64 scores with the exact scale is the reference's own function: its three gradients equal the
    recorded float64 autograd of sum(out g) to float64 rounding (the recording keeps 2^-24 of its 1e-7 residual: 1e-13)."""
    for name, (B, H, DK, N, M) in CASES.items():
        q, k, v, g = (golden[f"{name}_{x}"] for x in "qkvg")
        for b in range(B):
            ev = AR.evaluate(AR.exact_scores(q[b], k[b], H), v[b], H, g=g[b], q=q[b], k=k[b], sc=1.0 / np.sqrt(F64(DK)))
            for key in ("out", "d_q", "d_k", "d_v"):
                want = recorded(golden, f"{name}_{key}")[1][b]
                assert np.abs(ev[key] - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (name, b, key)
            tw = AR.evaluate(AR.scores(q[b], k[b], H), v[b], H, g=g[b], q=q[b], k=k[b])
            for key in ("d_q", "d_k", "d_v"):
                assert (tw[key + "_bound"] > 0).all() and np.isfinite(tw[key + "_bound"]).all()
                assert np.abs(tw[key] - ev[key]).max() <= 1e-4 * max(1.0, np.abs(ev[key]).max()), (name, b, key)


def test_counts_in_the_twin():
    q, k, v, g = AR.make_case(1, 2, 3, 5, 7, 1.0, "random", 1)
    z = AR.scores(q[0], k[0], 2)
    ev = AR.evaluate(z, v[0], 2, nq=3, nt=4, g=g[0], q=q[0], k=k[0])
    small = AR.evaluate(z[:, :3, :4], v[0][:4], 2, g=g[0][:3], q=q[0][:3], k=k[0][:4])
    assert not ev["out"][3:].any() and not ev["d_q"][3:].any() and not ev["d_k"][4:].any() and not ev["d_v"][4:].any()
    for key in ("out", "d_q"):
        assert np.array_equal(ev[key][:3], small[key])
    for key in ("d_k", "d_v"):
        assert np.array_equal(ev[key][:4], small[key])
    empty = AR.evaluate(z, v[0], 2, nq=3, nt=0, g=g[0], q=q[0], k=k[0])
    assert not any(empty[key].any() for key in ("out", "d_q", "d_k", "d_v"))
    one = AR.forward_rule(z, v[0], 2, nq=5, nt=1)
    assert np.array_equal(one["out"], np.repeat(v[0][:1], 5, axis=0))


def test_case_generator_kinds():
    for kind in AR.KINDS:
        q, k, v, g = AR.make_case(2, 3, 8, 6, 40, 1.0, kind, seed=1)
        assert q.shape == g.shape == (2, 6, 24) and k.shape == v.shape == (2, 40, 24)
        assert all(x.dtype == F32 for x in (q, k, v, g))
        z = AR.scores(q[0], k[0], 3).astype(F64)
        if kind == "one_hot":
            top = np.sort(z, axis=2)
            assert (top[..., -1] - top[..., -2] > 100).all()
        elif kind == "equal":
            assert (z == z[:, :1, :1]).all()


# ---- the C entries ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from rrl_hip import _lib, build
    build.build_lib()
    return _lib.load()


DIMS = (("B", 2), ("H", 4), ("DK", 16), ("N", 300), ("M", 200))


def fwd_args(lib, **over):
    dims = [over.pop(k, v) for k, v in DIMS]
    base = dict(q=FAKE, k=FAKE, v=FAKE, count_q=None, count_kv=None, ws=FAKE, ws_bytes=int(lib.rrl_attention_workspace_bytes(2, 4, 300, 200)),
                out=FAKE, info=None)
    base.update(over)
    return (*base.values(), *dims, None)


def bwd_args(lib, **over):
    dims = [over.pop(k, v) for k, v in DIMS]
    base = dict(q=FAKE, k=FAKE, v=FAKE, count_q=None, count_kv=None, ws=FAKE, ws_bytes=int(lib.rrl_attention_workspace_bytes(2, 4, 300, 200)),
                out=FAKE, g_out=FAKE, d_q=None, d_k=None, d_v=None)
    base.update(over)
    return (*base.values(), *dims, None)


SHARED_REFUSALS = [dict(q=None), dict(k=None), dict(v=None), dict(ws=None), dict(out=None), dict(B=-1), dict(B=32768), dict(H=0), dict(H=17),
                   dict(DK=0), dict(DK=129), dict(N=0), dict(M=0), dict(N=16385), dict(M=16385)]


def test_c_refusals_return_their_codes_without_a_launch(lib):
    for over in SHARED_REFUSALS:
        assert lib.rrl_attention_fwd(*fwd_args(lib, **dict(over))) == E_ARG, over
        assert lib.rrl_attention_bwd(*bwd_args(lib, **dict(over))) == E_ARG, over
    assert lib.rrl_attention_bwd(*bwd_args(lib, g_out=None)) == E_ARG
    short = int(lib.rrl_attention_workspace_bytes(2, 4, 300, 200)) - 1
    for over in (dict(ws_bytes=short), dict(ws=FAKE + 4)):
        assert lib.rrl_attention_fwd(*fwd_args(lib, **over)) == E_WS, over
        assert lib.rrl_attention_bwd(*bwd_args(lib, **over)) == E_WS, over
    assert lib.rrl_attention_fwd(*fwd_args(lib, ws_bytes=short, N=0)) == E_ARG     # (the argument refusals come first)
    assert lib.rrl_attention_fwd(*fwd_args(lib, B=0)) == 0 and lib.rrl_attention_bwd(*bwd_args(lib, B=0)) == 0  # (no launch)
    scores = dict(q=FAKE, k=FAKE, count_q=None, count_kv=None, scores=FAKE)
    for over in (dict(q=None), dict(k=None), dict(scores=None)):
        assert lib.rrl_attention_scores(*{**scores, **over}.values(), 2, 4, 16, 300, 200, None) == E_ARG, over
    assert lib.rrl_attention_scores(*scores.values(), 2, 4, 129, 300, 200, None) == E_ARG
    assert lib.rrl_attention_scores(*scores.values(), 0, 4, 16, 300, 200, None) == 0


def test_workspace_is_two_doubles_per_row(lib):
    """Two doubles per (sample, head, row): independent of M (and of DK, which the size function does not even take); 0 for a
    shape that is refused."""
    size = lib.rrl_attention_workspace_bytes
    assert size(8, 4, 1024, 1024) == 8 * 4 * 1024 * 2 * 8 == size(8, 4, 1024, 1) == size(8, 4, 1024, 16384)
    assert size(3, 5, 7, 11) == 3 * 5 * 7 * 16 and size(0, 1, 1, 1) == 0
    assert size(8, 4, 2048, 2048) * 256 <= 8 * 4 * 2048 * 2048 * 4   # 1 / 256 of ONE (B, H, N, M) float32 matrix
    for shape in ((-1, 4, 5, 5), (32768, 4, 5, 5), (1, 0, 5, 5), (1, 17, 5, 5), (1, 4, 0, 5), (1, 4, 16385, 5), (1, 4, 5, 0), (1, 4, 5, 16385)):
        assert size(*shape) == 0, shape


def test_entries_in_the_header_and_the_binding(lib):
    from rrl_hip import _abi, _lib, attention, callsites
    for name in ("rrl_attention_workspace_bytes", "rrl_attention_fwd", "rrl_attention_bwd", "rrl_attention_scores"):
        assert name in _abi.PROTOS and name in _lib.EXPORTS and hasattr(lib, name)
    assert not any("attention" in s for s in _abi.STRUCTS)
    assert len(_abi.PROTOS["rrl_attention_fwd"][1]) == 15 and len(_abi.PROTOS["rrl_attention_bwd"][1]) == 18
    assert len(_abi.PROTOS["rrl_attention_workspace_bytes"][1]) == 4
    assert _abi.CONSTANTS["RRL_ATTENTION_MAX_DK"] == 128
    assert callable(attention.attend) and callable(callsites.dcp_attention) and callable(callsites.dcp_transformer)
    assert (attention.MAX_B, attention.MAX_DIM, attention.MAX_H, attention.MAX_DK) == (32767, 16384, 16, 128)


def test_python_refusals_need_no_gpu():
    from rrl_hip import attention
    ok = ((2, 8, 64), (2, 6, 64), (2, 6, 64), 4)
    attention.check_request(*ok)
    attention.check_request(*ok, (2,), (2,))
    for args, match in ((((2, 8, 64), (3, 6, 64), (3, 6, 64), 4), "B and D"), (((2, 8, 64), (2, 6, 32), (2, 6, 32), 4), "B and D"),
                        (((2, 8, 64), (2, 6, 64), (2, 7, 64), 4), "B and D"), (((8, 64), (6, 64), (6, 64), 4), "token-major"),
                        (((2, 8, 64), (2, 6, 64), (2, 6, 64), 0), "n_heads"), (((2, 8, 64), (2, 6, 64), (2, 6, 64), 17), "n_heads"),
                        (((2, 8, 64), (2, 6, 64), (2, 6, 64), 4.0), "n_heads"), (((2, 8, 64), (2, 6, 64), (2, 6, 64), 3), "multiple"),
                        (((2, 8, 258), (2, 6, 258), (2, 6, 258), 2), "128"), (((40000, 8, 64), (40000, 6, 64), (40000, 6, 64), 4), "32767"),
                        (((0, 8, 64), (0, 6, 64), (0, 6, 64), 4), "32767"), (((1, 0, 64), (1, 6, 64), (1, 6, 64), 4), "16384"),
                        (((1, 8, 64), (1, 16385, 64), (1, 16385, 64), 4), "16384"), ((*ok, (3,)), "counts_q"), ((*ok, None, (2, 1)), "counts_kv")):
        with pytest.raises(ValueError, match=match):
            attention.check_request(*args)
    with pytest.raises(TypeError):
        attention.attend(np.zeros((1, 4, 8)), torch.zeros(1, 4, 8), torch.zeros(1, 4, 8), 2)
    with pytest.raises(ValueError, match=r"\[0, 5\]"):
        attention.attend(torch.zeros(1, 5, 8), torch.zeros(1, 3, 8), torch.zeros(1, 3, 8), 2, counts_q=[6])
    with pytest.raises(ValueError, match="multiple"):
        attention.MultiHeadedAttention(3, 64)


@pytest.mark.skipif(torch.cuda.is_available(), reason="the refusal of a machine without a GPU")
def test_without_a_gpu_the_call_raises():
    from rrl_hip import attention, callsites
    from rrl_hip._lib import RRLError
    with pytest.raises(RRLError):
        attention.attend(torch.zeros(1, 5, 8), torch.zeros(1, 3, 8), torch.zeros(1, 3, 8), 2)
    with pytest.raises(RRLError):
        callsites.dcp_transformer(attention.Transformer(8, 2, 16, 1), torch.zeros(1, 8, 5), torch.zeros(1, 8, 3))


def test_without_the_library_the_call_raises(monkeypatch, tmp_path):
    from rrl_hip import _lib, attention, ops
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB", str(tmp_path / "absent.so"))
    monkeypatch.setattr(ops, "_home", lambda *a: torch.device("cpu"))
    monkeypatch.setattr(ops, "_prep", lambda t, *a: t.detach())
    with pytest.raises(_lib.RRLError, match="missing"):
        attention.attend(torch.zeros(1, 5, 8), torch.zeros(1, 3, 8), torch.zeros(1, 3, 8), 2)


# ---- the modules -------------------------------------------------------------------------------------------------------------
def twin_attend(q, k, v, n_heads, counts_q=None, counts_kv=None, with_info=False):
    """forward_rule in the place of the node, on the CPU (forward only)."""
    out = [AR.forward_rule(AR.scores(a, b, n_heads), c, n_heads)["out"] for a, b, c in zip(q.detach().numpy(), k.detach().numpy(), v.detach().numpy())]
    return torch.from_numpy(np.stack(out))


def test_modules_carry_the_reference_keys_and_reproduce_the_recording_with_the_twin(golden, monkeypatch):
    from rrl_hip import attention
    tg = load_golden("attention_dcp_transformer.npz")
    emb, heads, ff, blocks = (int(x) for x in tg["config"])
    module = attention.Transformer(emb, heads, ff, blocks)
    keys = [str(k) for k in tg["keys"]]
    assert sorted(module.state_dict()) == sorted(keys) and "model.encoder.layers.0.self_attn.linears.0.weight" in keys
    assert "model.decoder.layers.0.src_attn.linears.3.bias" in keys and "model.decoder.norm.a_2" in keys
    module.load_state_dict({k: torch.from_numpy(tg["sd_" + k]) for k in keys}, strict=True)
    mha = attention.MultiHeadedAttention(4, 64)
    mkeys = [str(k) for k in golden["mha_keys"]]
    assert sorted(mha.state_dict()) == sorted(mkeys)
    mha.load_state_dict({k: torch.from_numpy(golden["mha_sd_" + k]) for k in mkeys}, strict=True)
    monkeypatch.setattr(attention, "attend", twin_attend)
    with torch.no_grad():
        got = mha(*(torch.from_numpy(golden[f"mha_{x}"]) for x in ("query", "key", "value"))).numpy()
        src_e, tgt_e = (x.numpy() for x in module(torch.from_numpy(tg["src"]), torch.from_numpy(tg["tgt"])))
    o32, o64, dist = recorded(golden, "mha_out")
    assert got.shape == o32.shape and np.abs(got - o64).max() <= TRANSFORMER_FACTOR * dist, (np.abs(got - o64).max(), dist)
    for mine, name in ((src_e, "src_embedding"), (tgt_e, "tgt_embedding")):
        r32, r64, dist = recorded(tg, name)
        assert mine.shape == r32.shape
        e64, e32 = np.abs(mine - r64).max(), np.abs(mine - r32).max()
        print(name, "twin in place of the node: to float64", e64 / dist, "to float32", e32 / dist, "distances; distance", dist)
        assert e64 <= TRANSFORMER_FACTOR * dist and e32 <= TRANSFORMER_FACTOR * dist, (e64, e32, dist)


# ---- the node's lifetime ---------------------------------------------------------------------------------------------------------
def stubbed_node(monkeypatch):
    """attention.attend on CPU tensors with the C entries replaced by a recorder: the autograd plumbing alone."""
    import types

    from rrl_hip import _lib, attention, ops
    calls = []
    monkeypatch.setattr(_lib, "load", lambda: types.SimpleNamespace(rrl_attention_workspace_bytes=lambda B, H, N, M: 16 * B * H * N))
    monkeypatch.setattr(ops, "_home", lambda *a: torch.device("cpu"))
    monkeypatch.setattr(ops, "_prep", lambda t, *a: t.detach())
    monkeypatch.setattr(ops, "_run", lambda dev, name, *args: calls.append((name, args)))
    return attention, calls


def test_the_output_dies_with_its_last_reference(monkeypatch):
    """No reference cycle through the node: with the cyclic collector off, a weak reference to out is dead as soon as out is
    deleted, with and without a backward -- the output, the workspace and the kept projections do not outlive the step."""
    import gc
    import weakref
    attention, calls = stubbed_node(monkeypatch)
    q, k, v = (torch.zeros(2, n, 8, requires_grad=True) for n in (5, 3, 3))
    gc.collect()
    gc.disable()
    try:
        for backward in (False, True):
            out = attention.attend(q, k, v, 2)
            ref, node = weakref.ref(out), weakref.ref(out.grad_fn)
            if backward:
                out.sum().backward()
            del out
            assert ref() is None and node() is None, backward
    finally:
        gc.enable()
    assert [name for name, _ in calls] == ["rrl_attention_fwd", "rrl_attention_fwd", "rrl_attention_bwd"]


def test_info_reaches_the_entry_only_when_asked_for(monkeypatch):
    """The forward's ninth argument is info: NULL without with_info (the entry then launches no second kernel)."""
    attention, calls = stubbed_node(monkeypatch)
    q, k, v = (torch.zeros(2, n, 8) for n in (5, 3, 3))
    out = attention.attend(q, k, v, 2)
    out2, info = attention.attend(q, k, v, 2, with_info=True)
    assert out.shape == out2.shape == (2, 5, 8) and info.shape == (2,) and info.dtype == torch.int32
    assert calls[0][1][8] is None and calls[1][1][8] is not None and calls[0][1][7] is not None
