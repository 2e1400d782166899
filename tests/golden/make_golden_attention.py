#!/usr/bin/env python3
"""Generate tests/golden/attention_dcp*.npz -- DCP's attention, MultiHeadedAttention and Transformer on a few small cases --
by RUNNING THE REFERENCE's dcp/model.py (attention :27-34, MultiHeadedAttention :212-246, Transformer :373-401) on the CPU, in
float32 and on float64 copies of the same inputs and weights, with the helpers of make_golden.py (same stubs, same reference
checkout; the reference module imports h5py for its data loaders and, through utils, plyfile: empty stand-ins).

Run in the build container only (needs the reference checkout, see make_golden.py):

    python tests/golden/make_golden_attention.py

Only data is stored.  A float64 result X64 is stored beside its float32 run X as `X_lo` = float32(X64 - float64(X)): the pair
gives X64 back to 2^-24 of their DIFFERENCE (1e-14 here) at half the bytes, which keeps every file below the size limit of a
committed file; `X_dist` is max |X64 - X|.  Four files for the same reason:
  attention_dcp.npz              the cases b2_h4_dk16_33x40 and b2_h3_dk11_64x64 (inputs, out, gradients of sum(out g)) and one
                                 MultiHeadedAttention(4, 64) with its state dict
  attention_dcp_dk128_fwd.npz    the case b1_h4_dk128_65x70: inputs and out
  attention_dcp_dk128_bwd.npz    ... its gradients
  attention_dcp_transformer.npz  Transformer(emb_dims 64, 4 heads, ff_dims 128, 1 block), N = 33, M = 40: state dict (LayerNorm's
                                 a_2 / b_2 moved off their 1 / 0 defaults so that every key matters), inputs, both outputs
"""
import importlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402  (registers the stubs, names the reference checkout)

import torch  # noqa: E402

import attention_refs as AR  # noqa: E402

# name -> (B, H, DK, N, M, sigma)
CASES = {
    "b2_h4_dk16_33x40": (2, 4, 16, 33, 40, 1.0),
    "b1_h4_dk128_65x70": (1, 4, 128, 65, 70, 1.0),
    "b2_h3_dk11_64x64": (2, 3, 11, 64, 64, 2.0),
}
BIG = "b1_h4_dk128_65x70"
TRANSFORMER = dict(emb_dims=64, n_heads=4, ff_dims=128, n_blocks=1, B=2, N=33, M=40)


def reference_module():
    sys.modules.setdefault("h5py", types.ModuleType("h5py"))
    sys.modules.setdefault("plyfile", types.ModuleType("plyfile")).PlyData = object
    sys.path.insert(0, os.path.join(MG.REF, "exps_deep_learning", "dcp"))
    return importlib.import_module("model")


def both(kw, name, x32, x64):
    """X, X_lo and X_dist of one result."""
    x32, x64 = x32.detach().numpy(), x64.detach().numpy()
    assert x32.dtype == np.float32 and x64.dtype == np.float64
    kw[name] = x32
    kw[name + "_lo"] = (x64 - x32.astype(np.float64)).astype(np.float32)
    kw[name + "_dist"] = np.float64(np.abs(x64 - x32.astype(np.float64)).max())


def run_attention(ref, q, k, v, g, H, dtype):
    """The reference's attention() between the views of MultiHeadedAttention.forward, on token-major projections."""
    tq, tk, tv = (torch.from_numpy(x).to(dtype).requires_grad_(True) for x in (q, k, v))
    B, DK = q.shape[0], q.shape[2] // H
    qh, kh, vh = (x.view(B, -1, H, DK).transpose(1, 2).contiguous() for x in (tq, tk, tv))
    x, _ = ref.attention(qh, kh, vh)
    out = x.transpose(1, 2).contiguous().view(B, -1, H * DK)
    (out * torch.from_numpy(g).to(dtype)).sum().backward()
    return out, tq.grad, tk.grad, tv.grad


def main():
    ref = reference_module()
    small, big_fwd, big_bwd = dict(cases=np.array(list(CASES))), {}, {}
    for i, (name, (B, H, DK, N, M, sigma)) in enumerate(CASES.items()):
        q, k, v, g = AR.make_case(B, H, DK, N, M, sigma, "random", seed=2000 + i)
        r32 = run_attention(ref, q, k, v, g, H, torch.float32)
        r64 = run_attention(ref, q, k, v, g, H, torch.float64)
        fwd, bwd = (big_fwd, big_bwd) if name == BIG else (small, small)
        fwd.update({f"{name}_q": q, f"{name}_k": k, f"{name}_v": v, f"{name}_g": g})
        both(fwd, f"{name}_out", r32[0], r64[0])
        for key, a, b in zip(("d_q", "d_k", "d_v"), r32[1:], r64[1:]):
            both(bwd, f"{name}_{key}", a, b)
        print(name, "out dist", float(fwd[f"{name}_out_dist"]), "grad dists", [float(bwd[f"{name}_{key}_dist"]) for key in ("d_q", "d_k", "d_v")])

    torch.manual_seed(7)
    mha = ref.MultiHeadedAttention(4, 64)
    rs = np.random.default_rng(7)
    xq, xk, xv = (rs.standard_normal(s).astype(np.float32) for s in ((2, 33, 64), (2, 40, 64), (2, 40, 64)))
    with torch.no_grad():
        o32 = mha(*(torch.from_numpy(x) for x in (xq, xk, xv)))
        o64 = mha.double()(*(torch.from_numpy(x).double() for x in (xq, xk, xv)))
    mha.float()
    small.update(mha_query=xq, mha_key=xk, mha_value=xv, mha_keys=np.array(list(mha.state_dict())))
    small.update({f"mha_sd_{key}": val.numpy() for key, val in mha.state_dict().items()})
    both(small, "mha_out", o32, o64)
    print("mha dist", float(small["mha_out_dist"]))

    T = TRANSFORMER
    torch.manual_seed(11)
    tr = ref.Transformer(types.SimpleNamespace(emb_dims=T["emb_dims"], n_blocks=T["n_blocks"], dropout=0.0, ff_dims=T["ff_dims"],
                                               n_heads=T["n_heads"]))
    with torch.no_grad():
        for key, p in tr.named_parameters():
            if key.endswith("a_2") or key.endswith("b_2"):
                p.add_(0.1 * torch.randn_like(p))
    rs = np.random.default_rng(11)
    src = rs.standard_normal((T["B"], T["emb_dims"], T["N"])).astype(np.float32)
    tgt = rs.standard_normal((T["B"], T["emb_dims"], T["M"])).astype(np.float32)
    with torch.no_grad():
        s32, t32 = tr(torch.from_numpy(src), torch.from_numpy(tgt))
        sd = {key: val.clone() for key, val in tr.state_dict().items()}
        s64, t64 = tr.double()(torch.from_numpy(src).double(), torch.from_numpy(tgt).double())
    kw = dict(src=src, tgt=tgt, keys=np.array(list(sd)), config=np.array([T["emb_dims"], T["n_heads"], T["ff_dims"], T["n_blocks"]]))
    kw.update({f"sd_{key}": val.numpy() for key, val in sd.items()})
    both(kw, "src_embedding", s32, s64)
    both(kw, "tgt_embedding", t32, t64)
    print("transformer dists", float(kw["src_embedding_dist"]), float(kw["tgt_embedding_dist"]))

    MG.save("attention_dcp.npz", **small)
    MG.save("attention_dcp_dk128_fwd.npz", **big_fwd)
    MG.save("attention_dcp_dk128_bwd.npz", **big_bwd)
    MG.save("attention_dcp_transformer.npz", **kw)


if __name__ == "__main__":
    main()
