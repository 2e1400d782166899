"""Host twin of the PointNet encoder (include/rrl.h rrl_pointnet_fwd), numpy only.

The pre-activations restate the header's rule bit for bit: one float32 fmaf chain per (channel, point) that starts at the bias
and runs over the input channels ascending (pointer_refs.fmaf32).  Everything behind them is float64 from those float32 y:
the group sums, mu, r, the channels' a and d, the activation float32(max(0, double(y) a + d)) -- numpy multiplies and adds in
two operations, as the device does --, the extremum rule of the last layer.  Stage functions take the previous stage as an
argument, so a test can feed the DEVICE's own previous stage and compare one stage at a time.
"""
import numpy as np

from pointer_refs import fmaf32

F32, F64 = np.float32, np.float64
EPS = 1.0e-5


def chain(W, b, h):
    """y (c, N) float32 of one sample: W (c, cin), b (c,), h (cin, N) float32."""
    W = np.asarray(W, F32).reshape(W.shape[0], -1)
    acc = np.repeat(np.asarray(b, F32)[:, None], h.shape[1], axis=1)
    for k in range(W.shape[1]):
        acc = fmaf32(W[:, k][:, None], h[k][None, :], acc)
    return acc


def stats(y, G, eps=EPS):
    """Per group of y (c, N): dict of s = sum y, ss = sum y^2, their sums of magnitudes, mu, r (float64, (G,)) and m."""
    c, N = y.shape
    yd = y.astype(F64).reshape(G, -1)
    m = yd.shape[1]
    s, ss = yd.sum(1), (yd * yd).sum(1)
    mu = s / m
    var = np.maximum(0.0, ss / m - mu * mu)
    return dict(s=s, ss=ss, abs_s=np.abs(yd).sum(1), mu=mu, r=1.0 / np.sqrt(var + eps), m=m)


def coef(gamma, beta, mu, r):
    """a, d (c,) float64 from the group's mu, r (G,)."""
    cpg = gamma.shape[0] // mu.shape[0]
    a = gamma.astype(F64) * np.repeat(r, cpg)
    return a, beta.astype(F64) - np.repeat(mu, cpg) * a


def act(y, a, d):
    """h (c, N) float32 = float32(max(0, double(y) a + d)): a multiplication, an addition, one rounding; 0 where the sum is < 0, else the sum."""
    t = y.astype(F64) * a[:, None]
    t = t + d[:, None]
    return np.where(t < 0.0, 0.0, t).astype(F32)


def pool(y, a, d):
    """The last layer of one sample from its y (K, N): ext (K,) float32, arg (K,) the lowest index of the maximum (a >= 0) or
    of the minimum (a < 0), f (K,) float32."""
    up = a >= 0.0
    arg = np.where(up, y.argmax(1), y.argmin(1)).astype(np.int32)   # numpy's argmax / argmin return the first occurrence
    ext = y[np.arange(y.shape[0]), arg]
    t = ext.astype(F64) * a
    t = t + d
    return ext, arg, np.where(t < 0.0, 0.0, t).astype(F32)


def split(params):
    """[(W (c, cin), b, gamma, beta), ...] from the flat list."""
    return [(np.asarray(params[i], F32).reshape(params[i].shape[0], -1),) + tuple(np.asarray(p, F32) for p in params[i + 1:i + 4])
            for i in range(0, len(params), 4)]


def forward(points, params, groups, eps=EPS):
    """One sample: points (N, c0) float32 -> dict of y [per layer (c, N)], st [per layer stats], a, d [per layer], h [per hidden
    layer], ext, arg, f."""
    h = np.ascontiguousarray(np.asarray(points, F32).T)
    out = dict(y=[], st=[], a=[], d=[], h=[])
    layers = split(params)
    for l, ((W, b, gamma, beta), G) in enumerate(zip(layers, groups)):
        y = chain(W, b, h)
        st = stats(y, G, eps)
        a, d = coef(gamma, beta, st["mu"], st["r"])
        out["y"].append(y); out["st"].append(st); out["a"].append(a); out["d"].append(d)
        if l + 1 < len(layers):
            h = act(y, a, d)
            out["h"].append(h)
    out["ext"], out["arg"], out["f"] = pool(out["y"][-1], out["a"][-1], out["d"][-1])
    return out


def exact(points, params, groups, eps=EPS):
    """features (K,) of one sample in plain float64 (torch's formulation: conv, group norm, relu, max over the points)."""
    h = np.asarray(points, F64).T
    for (W, b, gamma, beta), G in zip(split(params), groups):
        y = W.astype(F64) @ h + b.astype(F64)[:, None]
        yg = y.reshape(G, -1)
        mu, var = yg.mean(1, keepdims=True), yg.var(1, keepdims=True)
        xh = ((yg - mu) / np.sqrt(var + eps)).reshape(y.shape)
        h = np.maximum(0.0, xh * gamma.astype(F64)[:, None] + beta.astype(F64)[:, None])
    return h.max(1)


FMR_KEYS = tuple(f"{blk}.{i}.{kind}" for blk, idx in (("h1", (0, 1, 3, 4)), ("h2", (0, 1, 3, 4, 6, 7))) for i in idx
                 for kind in ("weight", "bias"))


def fmr_params(weights):
    """The flat params list from a {state_dict key: array} of the reference's PointNet."""
    return [np.asarray(weights[k], F32) for k in FMR_KEYS]


def fixture_case(fx, name):
    """(points (B, N, 3), {key: array}) of a case of tests/golden/pointnet.npz."""
    pre = f"{name}_w_"
    return fx[f"{name}_p"], {k[len(pre):]: fx[k] for k in fx.files if k.startswith(pre)}


def make_stack(c0, widths, groups, seed=0, special=True):
    """A random stack's flat params (float32): W ~ N(0, 1 / cin), b small, gamma about 1, beta small.  special: channel 1 of the
    last layer gets gamma < 0 and channel 2 gamma = 0 (the minimum branch and the a = 0 branch of the extremum rule)."""
    rs = np.random.default_rng([seed, c0, len(widths)] + list(widths))
    out, last = [], c0
    for c in widths:
        out += [(rs.standard_normal((c, last)) / np.sqrt(last)).astype(F32), (0.1 * rs.standard_normal(c)).astype(F32),
                (1.0 + 0.2 * rs.standard_normal(c)).astype(F32), (0.2 * rs.standard_normal(c)).astype(F32)]
        last = c
    if special and widths[-1] >= 3:
        out[-2][1] = F32(-0.7)
        out[-2][2] = F32(0.0)
        out[-1][2] = F32(0.3)
    return out


# ---- the backward (include/rrl.h rrl_pointnet_bwd), float64 -------------------------------------------------------------------
def gn_backward(y, dout, gamma, mu, r, G, absmode=False):
    """GroupNorm's rule on one layer of one sample: y, dout (c, N), mu, r (G,) -> dy (c, N), dgamma, dbeta (c,).
    absmode: every term replaced by its magnitude (dout is then a magnitude already): the sums of |terms| behind the bounds."""
    c, N = y.shape
    cpg, m = c // G, (c // G) * N
    mu_c, r_c = np.repeat(mu, cpg)[:, None], np.repeat(r, cpg)[:, None]
    xhat = (y.astype(F64) - mu_c) * r_c
    g = gamma.astype(F64)[:, None]
    if absmode:
        xhat, g = np.abs(xhat), np.abs(g)
    dgamma, dbeta = (dout * xhat).sum(1), dout.sum(1)
    P = np.repeat((g[:, 0] * dbeta).reshape(G, cpg).sum(1), cpg)[:, None]
    Q = np.repeat((g[:, 0] * dgamma).reshape(G, cpg).sum(1), cpg)[:, None]
    dy = r_c * (g * dout + P / m + xhat * Q / m) if absmode else r_c * (g * dout - P / m - xhat * Q / m)
    return dy, dgamma, dbeta


def last_closed(h, W, b, gamma, mu, r, G, ext, arg, s, absmode=False):
    """The last layer of one sample in closed form (no N x K work): from h = h_{L-1} (H, N), the extrema ext (K,) at arg (K,) and
    s_c = g_f[c] [f[c] > 0] -> dh (H, N), dW (K, H), db, dgamma, dbeta (K,)."""
    K, H = W.shape
    N = h.shape[1]
    cpg, m = K // G, (K // G) * N
    Wd, bd, hd, gd = W.astype(F64), b.astype(F64), h.astype(F64), gamma.astype(F64)
    rg, mug = np.repeat(r, cpg), np.repeat(mu, cpg)
    x = (ext.astype(F64) - mug) * rg
    if absmode:
        Wd, bd, gd, x, mug = np.abs(Wd), np.abs(bd), np.abs(gd), np.abs(x), np.abs(mug)
    S1, S2 = hd.sum(1), hd @ hd.T
    P = np.repeat((gd * s).reshape(G, cpg).sum(1), cpg)
    Q = np.repeat((gd * s * x).reshape(G, cpg).sum(1), cpg)
    if absmode:
        A, Bg = rg * P / m + rg * rg * Q * mug / m, rg * rg * Q / m
    else:
        A, Bg = -rg * P / m + rg * rg * Q * mug / m, -rg * rg * Q / m
    t = rg * gd * s
    dW = t[:, None] * hd[:, arg].T + A[:, None] * S1[None, :] + Bg[:, None] * (Wd @ S2 + bd[:, None] * S1[None, :])
    db = t + N * A + Bg * (Wd @ S1 + N * bd)
    M = (Wd * Bg[:, None]).T @ Wd
    uv = (Wd * (A + Bg * bd)[:, None]).sum(0)
    dh = M @ hd + uv[:, None]
    np.add.at(dh.T, arg, t[:, None] * Wd)        # dh[:, arg_c] += t_c W[c]: several channels may share a point
    return dh, dW, db, s * x, s.copy()


def last_dense(h, W, b, gamma, mu, r, G, arg, s):
    """The same by the dense rule on y_L = W h + b in float64 (N x K work): the check of the closed form."""
    y = W.astype(F64) @ h.astype(F64) + b.astype(F64)[:, None]
    dout = np.zeros_like(y)
    dout[np.arange(y.shape[0]), arg] = s
    dy, dgamma, dbeta = gn_backward(y, dout, gamma, mu, r, G)
    return W.astype(F64).T @ dy, dy @ h.astype(F64).T, dy.sum(1), dgamma, dbeta


def backward(points, params, groups, y, mu, r, a, d, ext, arg, g_f, absmode=False):
    """One sample's gradients of sum(f g_f) from the forward's kept quantities -- y [per hidden layer (c, N) float32], mu, r [per
    layer (G,)], a, d [per layer (c,)], ext, arg (K,) -- in float64: dict d_points (N, c0), dW, db, dgamma, dbeta [per layer].
    absmode: the same sums with every term replaced by its magnitude."""
    layers = split(params)
    L = len(layers)
    hs = [np.ascontiguousarray(np.asarray(points, F32).T)] + [act(y[l], a[l], d[l]) for l in range(L - 1)]
    _, _, f = pool(ext[:, None], a[-1], d[-1])
    s = np.where(f > 0, g_f.astype(F64), 0.0)
    if absmode:
        s = np.abs(s)
    W, b, gamma, _ = layers[-1]
    dh, dW, db, dg, dbt = last_closed(hs[-1], W, b, gamma, mu[-1], r[-1], groups[-1], ext, arg, s, absmode)
    out = dict(dW=[dW], db=[db], dgamma=[dg], dbeta=[dbt])
    for l in range(L - 2, -1, -1):
        W, b, gamma, _ = layers[l]
        dout = dh * (hs[l + 1] > 0)
        dy, dg, dbt = gn_backward(y[l], dout, gamma, mu[l], r[l], groups[l], absmode)
        hp, Wd = hs[l].astype(F64), W.astype(F64)
        if absmode:
            hp, Wd = np.abs(hp), np.abs(Wd)
        out["dW"].insert(0, dy @ hp.T); out["db"].insert(0, dy.sum(1)); out["dgamma"].insert(0, dg); out["dbeta"].insert(0, dbt)
        dh = Wd.T @ dy
    out["d_points"] = np.ascontiguousarray(dh.T)
    return out


def backward_of_forward(points, params, groups, g_f, absmode=False):
    """backward() on the twin's own forward of one sample."""
    fw = forward(points, params, groups)
    st = fw["st"]
    return backward(points, params, groups, fw["y"][:-1], [s["mu"] for s in st], [s["r"] for s in st], fw["a"], fw["d"], fw["ext"],
                    fw["arg"], g_f, absmode)
