"""Float64 twins of the Sinkhorn soft assignment (include/rrl.h rrl_sinkhorn_fwd / rrl_sinkhorn_bwd).

forward / backward: the dual-potential form and the hand-derived reverse sweep, in numpy float64 -- the statement the
kernels are held to.  padded_torch: the padded-matrix formulation of rpm/models/rpmnet.py:48-118 and the lines 214-222
behind it, restated in torch at any dtype -- the twin is checked against it (and against the recorded reference run), and
its float32 evaluation on the CPU is the yardstick of the GPU tests."""
import numpy as np
import torch


def _lse(x, axis, sigma):
    """log(sum exp(x) + sigma) along `axis`; an empty or all -inf slice gives log(sigma)."""
    m = np.max(x, axis=axis, keepdims=True, initial=-np.inf)
    m = np.where(np.isfinite(m), m, 0.0)
    if sigma:
        m = np.maximum(m, 0.0)
    with np.errstate(divide="ignore"):
        return np.squeeze(m + np.log(np.exp(x - m).sum(axis=axis, keepdims=True) + sigma * np.exp(-m)), axis)


def forward(A, x, n_iters=5, slack=True, eps=1e-5):
    """A (B, J, K), x (B, K, 3) -> dict: U, V (lists of the potentials u^0 .. u^n, v^0 .. v^n), log_perm, P, s, c, N, W."""
    A, x = np.asarray(A, np.float64), np.asarray(x, np.float64)
    B, J, K = A.shape
    sigma = 1.0 if slack else 0.0
    U, V = [np.zeros((B, J))], [np.zeros((B, K))]
    for _ in range(n_iters):
        U.append(_lse(A - V[-1][:, None, :], 2, sigma))
        V.append(_lse(A - U[-1][:, :, None], 1, sigma))
    log_perm = A - U[-1][:, :, None] - V[-1][:, None, :]
    P = np.exp(log_perm)
    s, c, N = P.sum(2), P.sum(1), P @ x
    return dict(U=U, V=V, log_perm=log_perm, P=P, s=s, c=c, N=N, W=N / (s + eps)[..., None])


def backward(A, x, gW, gs, gc, n_iters=5, slack=True, eps=1e-5, fwd=None):
    """The reverse sweep by hand -> dict: dA (B, J, K), gx (B, K, 3), and the magnitudes a cancelling sum is judged by:
    dA_abs / gx_abs, the same sums with every term and every adjoint vector replaced by its absolute value (an upper bound
    of sum |terms| that also carries the cancellation inside the adjoint vectors), and dA_coef, the sum of the absolute
    coefficients in front of an entry's 2 n + 1 exponentials."""
    f = fwd or forward(A, x, n_iters, slack, eps)
    A, x = np.asarray(A, np.float64), np.asarray(x, np.float64)
    gW, gs, gc = (np.asarray(g, np.float64) for g in (gW, gs, gc))
    P, U, V = f["P"], f["U"], f["V"]
    den = f["s"] + eps
    gN = gW / den[..., None]
    gsp = gs - (gW * f["W"]).sum(-1) / den
    G = gsp[:, :, None] + gc[:, None, :] + gN @ x.transpose(0, 2, 1)
    Gabs = (np.abs(gs) + (np.abs(gW) * np.abs(f["W"])).sum(-1) / den)[:, :, None] + np.abs(gc)[:, None, :] + \
        np.abs(gN) @ np.abs(x).transpose(0, 2, 1)
    gx = P.transpose(0, 2, 1) @ gN
    gx_abs = P.transpose(0, 2, 1) @ np.abs(gN)
    dA, dA_abs, coef = P * G, P * Gabs, Gabs.copy()
    ub, vb = -(P * G).sum(2), -(P * G).sum(1)
    uba, vba = (P * Gabs).sum(2), (P * Gabs).sum(1)
    for t in range(n_iters - 1, -1, -1):
        Q = np.exp(A - U[t + 1][:, :, None] - V[t + 1][:, None, :])
        dA += vb[:, None, :] * Q
        dA_abs += vba[:, None, :] * Q
        coef += vba[:, None, :]
        ub = ub - (vb[:, None, :] * Q).sum(2)
        uba = uba + (vba[:, None, :] * Q).sum(2)
        S = np.exp(A - U[t + 1][:, :, None] - V[t][:, None, :])
        dA += ub[:, :, None] * S
        dA_abs += uba[:, :, None] * S
        coef += uba[:, :, None]
        vb, vba = -(ub[:, :, None] * S).sum(1), (uba[:, :, None] * S).sum(1)
        ub, uba = np.zeros_like(ub), np.zeros_like(uba)
    return dict(dA=dA, gx=gx, dA_abs=dA_abs, gx_abs=gx_abs, dA_coef=coef)


def padded_torch(log_alpha, xyz_ref, n_iters=5, slack=True, eps=1e-5):
    """The reference's formulation in torch, at the dtype of its inputs: the matrix padded with a zero row and column, each
    iteration a logsumexp over the rows that are normalised (all but the pad row) and one over the columns (all but the
    pad column); then perm = exp(.), weighted_ref = perm @ xyz_ref / (perm.sum(2) + eps).  Returns (log_perm, W, s, c)."""
    la = log_alpha
    if slack:
        la = torch.nn.functional.pad(la, (0, 1, 0, 1))
    for _ in range(n_iters):
        if slack:
            body = la[:, :-1, :] - torch.logsumexp(la[:, :-1, :], dim=2, keepdim=True)
            la = torch.cat((body, la[:, -1:, :]), dim=1)
            body = la[:, :, :-1] - torch.logsumexp(la[:, :, :-1], dim=1, keepdim=True)
            la = torch.cat((body, la[:, :, -1:]), dim=2)
        else:
            la = la - torch.logsumexp(la, dim=2, keepdim=True)
            la = la - torch.logsumexp(la, dim=1, keepdim=True)
    log_perm = la[:, :-1, :-1] if slack else la
    perm = torch.exp(log_perm)
    s = perm.sum(2)
    return log_perm, perm @ xyz_ref / (s[..., None] + eps), s, perm.sum(1)


def padded_torch_grads(A, x, gW, gs, gc, n_iters=5, slack=True, eps=1e-5, dtype=torch.float64):
    """Autograd of padded_torch at `dtype` on the CPU -> (log_perm, W, s, c, dA, gx) as float64 numpy arrays."""
    ta, tx = (torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for v in (A, x))
    lp, W, s, c = padded_torch(ta, tx, n_iters, slack, eps)
    up = [torch.tensor(np.asarray(g), dtype=dtype) for g in (gW, gs, gc)]
    ((W * up[0]).sum() + (s * up[1]).sum() + (c * up[2]).sum()).backward()
    return tuple(t.detach().double().numpy() for t in (lp, W, s, c, ta.grad, tx.grad))


def rpm_head(A, x_src, x_ref, n_iters=5, slack=True):
    """rpmnet.py:211-222 in float64 torch: (transform (B, 3, 4), W, s, c) -- padded_torch, then the weighted Kabsch solve of
    tests/kabsch_refs.py."""
    import kabsch_refs as KR
    ta, ts, tr = (torch.tensor(np.asarray(v), dtype=torch.float64) for v in (A, x_src, x_ref))
    _, W, s, c = padded_torch(ta, tr, n_iters, slack, 1e-5)
    return KR.rpm_transform(ts, W, s), W, s, c
