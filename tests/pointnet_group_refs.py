"""Host twin of the grouped PointNet (include/rrl.h rrl_pointnet_group_fwd / _bwd), numpy only, built on
pointnet_refs: position p = n S + s takes the place of a point, so the chain, the statistics, the coefficients and the activation
are pointnet_refs' own over the P = N S positions.  What is new here: the pool per point with the lowest-slot rule, and the last
layer's backward with its sparse term per point -- in the closed form of the header and by the dense rule on an explicit y_L.
Stage functions take the previous stage as arguments, so a test can feed the DEVICE's own previous stage.
"""
import numpy as np

import pointnet_refs as PR

F32, F64 = np.float32, np.float64
EPS = PR.EPS


def pool_points(y, a, d, S):
    """The last layer of one sample from its y (K, N S): ext (K, N) float32, arg (K, N) int32 the LOWEST slot of the maximum
    (a >= 0) or of the minimum (a < 0) over each point's S slots, out (K, N) float32."""
    K, P = y.shape
    y3 = y.reshape(K, P // S, S)
    up = (a >= 0.0)[:, None]
    arg = np.where(up, y3.argmax(2), y3.argmin(2)).astype(np.int32)   # numpy returns the first occurrence
    ext = np.take_along_axis(y3, arg[..., None].astype(np.int64), 2)[..., 0]
    t = ext.astype(F64) * a[:, None]
    t = t + d[:, None]
    return ext, arg, np.where(t < 0.0, 0.0, t).astype(F32)


def forward(x, params, groups, eps=EPS):
    """One sample: x (N, S, c0) float32 -> pointnet_refs.forward's dict over the positions (y, st, a, d, h) with ext, arg (K, N)
    and out (K, N) of the per-point pool."""
    N, S, c0 = x.shape
    fw = PR.forward(np.asarray(x, F32).reshape(N * S, c0), params, groups, eps)
    fw.pop("f")
    fw["ext"], fw["arg"], fw["out"] = pool_points(fw["y"][-1], fw["a"][-1], fw["d"][-1], S)
    return fw


def exact(x, params, groups, eps=EPS):
    """out (K, N) of one sample in plain float64 (torch's formulation: conv, group norm, relu, max over the slots)."""
    N, S, c0 = x.shape
    h = np.asarray(x, F64).reshape(N * S, c0).T
    for (W, b, gamma, beta), G in zip(PR.split(params), groups):
        y = W.astype(F64) @ h + b.astype(F64)[:, None]
        yg = y.reshape(G, -1)
        mu, var = yg.mean(1, keepdims=True), yg.var(1, keepdims=True)
        xh = ((yg - mu) / np.sqrt(var + eps)).reshape(y.shape)
        h = np.maximum(0.0, xh * gamma.astype(F64)[:, None] + beta.astype(F64)[:, None])
    return h.reshape(h.shape[0], N, S).max(2)


def positions(arg, S):
    """(K, N) positions n S + arg[c][n]."""
    return np.arange(arg.shape[1])[None, :] * S + arg.astype(np.int64)


def last_closed(h, W, b, gamma, mu, r, G, ext, arg, s, S, absmode=False):
    """The last layer of one sample in closed form (no P x K work): h = h_{L-1} (H, P), ext, arg, s (K, N) with s_{c,n} =
    g_out[c][n] [out[c][n] > 0] -> dh (H, P), dW (K, H), db, dgamma, dbeta (K,)."""
    K, H = W.shape
    P = h.shape[1]
    cpg, m = K // G, (K // G) * P
    Wd, bd, hd, gd = W.astype(F64), b.astype(F64), h.astype(F64), gamma.astype(F64)
    rg, mug = np.repeat(r, cpg), np.repeat(mu, cpg)
    x = (ext.astype(F64) - mug[:, None]) * rg[:, None]
    if absmode:
        Wd, bd, gd, x, mug = np.abs(Wd), np.abs(bd), np.abs(gd), np.abs(x), np.abs(mug)
    S1, S2 = hd.sum(1), hd @ hd.T
    dbeta, dgamma = s.sum(1), (s * x).sum(1)
    Pg = np.repeat((gd * dbeta).reshape(G, cpg).sum(1), cpg)
    Q = np.repeat((gd * dgamma).reshape(G, cpg).sum(1), cpg)
    if absmode:
        A, Bg = rg * Pg / m + rg * rg * Q * mug / m, rg * rg * Q / m
    else:
        A, Bg = -rg * Pg / m + rg * rg * Q * mug / m, -rg * rg * Q / m
    t = (rg * gd)[:, None] * s
    pos = positions(arg, S)
    sparse = np.einsum("cn,kcn->ck", t, hd[:, pos])
    dW = sparse + A[:, None] * S1[None, :] + Bg[:, None] * (Wd @ S2 + bd[:, None] * S1[None, :])
    db = t.sum(1) + P * A + Bg * (Wd @ S1 + P * bd)
    M = (Wd * Bg[:, None]).T @ Wd
    uv = (Wd * (A + Bg * bd)[:, None]).sum(0)
    dh = M @ hd + uv[:, None]
    np.add.at(dh.T, pos.ravel(), (t[:, :, None] * Wd[:, None, :]).reshape(-1, H))   # several channels may share a position
    return dh, dW, db, dgamma, dbeta


def last_dense(h, W, b, gamma, mu, r, G, arg, s, S):
    """The same by the dense rule on y_L = W h + b in float64 (P x K work): the check of the closed form."""
    y = W.astype(F64) @ h.astype(F64) + b.astype(F64)[:, None]
    dout = np.zeros_like(y)
    np.put_along_axis(dout, positions(arg, S), s, 1)
    dy, dgamma, dbeta = PR.gn_backward(y, dout, gamma, mu, r, G)
    return W.astype(F64).T @ dy, dy @ h.astype(F64).T, dy.sum(1), dgamma, dbeta


def backward(x, params, groups, y, mu, r, a, d, ext, arg, g_out, absmode=False):
    """One sample's gradients of sum(out g_out) from the forward's kept quantities -- y [per hidden layer (c, P) float32], mu, r
    [per layer (G,)], a, d [per layer (c,)], ext, arg (K, N) -- in float64: dict d_x (N, S, c0), dW, db, dgamma, dbeta [per layer].
    absmode: the same sums with every term replaced by its magnitude."""
    N, S, c0 = x.shape
    layers = PR.split(params)
    L = len(layers)
    hs = [np.ascontiguousarray(np.asarray(x, F32).reshape(N * S, c0).T)] + [PR.act(y[l], a[l], d[l]) for l in range(L - 1)]
    t = ext.astype(F64) * a[-1][:, None]
    t = t + d[-1][:, None]
    f = np.where(t < 0.0, 0.0, t).astype(F32)
    s = np.where(f > 0, g_out.astype(F64), 0.0)
    if absmode:
        s = np.abs(s)
    W, b, gamma, _ = layers[-1]
    dh, dW, db, dg, dbt = last_closed(hs[-1], W, b, gamma, mu[-1], r[-1], groups[-1], ext, arg, s, S, absmode)
    out = dict(dW=[dW], db=[db], dgamma=[dg], dbeta=[dbt])
    for l in range(L - 2, -1, -1):
        W, b, gamma, _ = layers[l]
        dout = dh * (hs[l + 1] > 0)
        dy, dg, dbt = PR.gn_backward(y[l], dout, gamma, mu[l], r[l], groups[l], absmode)
        hp, Wd = hs[l].astype(F64), W.astype(F64)
        if absmode:
            hp, Wd = np.abs(hp), np.abs(Wd)
        out["dW"].insert(0, dy @ hp.T); out["db"].insert(0, dy.sum(1)); out["dgamma"].insert(0, dg); out["dbeta"].insert(0, dbt)
        dh = Wd.T @ dy
    out["d_x"] = np.ascontiguousarray(dh.T).reshape(N, S, c0)
    return out


def backward_of_forward(x, params, groups, g_out, absmode=False):
    """backward() on the twin's own forward of one sample."""
    fw = forward(x, params, groups)
    st = fw["st"]
    return backward(x, params, groups, fw["y"][:-1], [q["mu"] for q in st], [q["r"] for q in st], fw["a"], fw["d"], fw["ext"],
                    fw["arg"], g_out, absmode)


RPM_KEYS = tuple(f"prepool.{i}.{kind}" for i in (0, 1, 3, 4, 6, 7) for kind in ("weight", "bias"))


def rpm_params(weights):
    """The flat params list from a {state_dict key: array} of the reference's prepool."""
    return [np.asarray(weights[k], F32) for k in RPM_KEYS]


def fixture_weights(fx, name):
    pre = f"{name}_w_"
    return {k[len(pre):]: fx[k] for k in fx.files if k.startswith(pre)}


def rpm_raw_case(bq, case="sphere_b2_130", tag="r030_k16"):
    """The recorded raw features (B, N, S, 10) of tests/golden/ball_query_rpm.npz: xyz expanded over the slots, dxyz, ppf --
    what FeatExtractionEarlyFusion.forward concatenates (rpm/models/feature_nets.py:184-193)."""
    xyz, dxyz, ppf = bq[f"{case}_xyz"], bq[f"{case}_{tag}_dxyz"], bq[f"{case}_{tag}_ppf"]
    return np.concatenate([np.broadcast_to(xyz[:, :, None, :], dxyz.shape), dxyz, ppf], -1).astype(F32)
