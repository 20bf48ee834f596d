"""Shared by test_gp_chain_cpu.py and test_gpu_gp_chain.py: the reference compositions (``Linear`` / ``leaky_relu`` / keep mask;
pooling / ``Linear`` / keep / ``sigmoid``) whose double backward autograd derives itself, the case builders, and the harness that
takes every first- and second-order output of either the composition or the op."""
import numpy as np
import torch

ALPHA = 0.2


# ------------------------------------------------------------------------------------------------ LinearNet
def make_net(widths, M, seed, two=0, resid=False, p=0.0, scale=1.0):
    """Weights, biases, input rows, cotangents and (``p``: host-drawn) keep masks of a net, fp64.  ``two``: the input's last ``two``
    columns are handed over as a second part.  ``scale`` multiplies the input and the biases, and with them every pre-activation."""
    rs = np.random.RandomState(seed)
    t = lambda *s: torch.from_numpy(rs.normal(size=s))
    c = dict(W=[t(o, i) / np.sqrt(i) for i, o in zip(widths[:-1], widths[1:])], b=[t(o) * 0.3 * scale for o in widths[1:]],
             x=t(M, widths[0]) * scale, go=t(M, widths[-1]), u=t(M, widths[0]), two=two,
             resid=t(M, widths[-1]) if resid else None, keeps=None, widths=list(widths), M=M)
    if p:
        c["keeps"] = [torch.from_numpy((rs.uniform(size=(M, o)) >= p) / (1 - p)) for o in widths[1:]]
    return c


def pre_activations(c, final_linear):
    """Z_l of every layer, in the case's dtype, under its keep masks."""
    x, out = c["x"], []
    L = len(c["W"])
    for l in range(L):
        z = torch.nn.functional.linear(x, c["W"][l], c["b"][l])
        out.append(z)
        x = z if (final_linear and l == L - 1) else torch.nn.functional.leaky_relu(z, ALPHA)
        if c["keeps"] is not None:
            x = x * c["keeps"][l]
    return out


def ref_net(x, resid, W, b, final_linear, keeps):
    """The reference composition: Linear / leaky_relu / keep mask per layer (mpgan/model.py:70-85), ``+ resid``."""
    L = len(W)
    for l in range(L):
        x = torch.nn.functional.linear(x, W[l], b[l])
        if not (final_linear and l == L - 1):
            x = torch.nn.functional.leaky_relu(x, ALPHA)
        if keeps is not None:
            x = x * keeps[l]
    return x if resid is None else x + resid


def net_derivatives(c, final_linear, op=None, conv=lambda t: t, use_u=True):
    """(y, first-order [x_bar, (resid_bar,) W_bar.., b_bar..], second-order [dPhi/dgo, dPhi/dW.., dPhi/db.., dPhi/dx]) with
    Phi = <u, x_bar>.  ``op(A, A2, W, b, resid)``: the op under test (the input in two parts when the case says so); None: the
    reference.  ``conv``: dtype / device of the leaves.  ``use_u`` "A2": u on the second part alone (the first's cotangent absent)."""
    x, go = conv(c["x"]).clone().requires_grad_(True), conv(c["go"]).clone().requires_grad_(True)
    W, b = [conv(w).clone().requires_grad_(True) for w in c["W"]], [conv(v).clone().requires_grad_(True) for v in c["b"]]
    r = None if c["resid"] is None else conv(c["resid"]).clone().requires_grad_(True)
    k = x.shape[1] - c["two"]
    if op is not None:
        A, A2 = (x[:, :k], x[:, k:]) if c["two"] else (x, None)
        y = op(A, A2, W, b, r)
    else:
        y = ref_net(x, r, W, b, final_linear, None if c["keeps"] is None else [conv(q) for q in c["keeps"]])
    wrt = [x] + ([r] if r is not None else []) + W + b
    first = torch.autograd.grad(y, wrt, go, create_graph=True)
    u = conv(c["u"])
    phi = (first[0][:, k:] * u[:, k:]).sum() if use_u == "A2" else (first[0] * u).sum()
    second = torch.autograd.grad(phi, [go] + W + b + [x], allow_unused=True, retain_graph=True)
    again = torch.autograd.grad(phi, [go] + W, allow_unused=True)
    return y.detach(), [f.detach() for f in first], list(second), list(again)


# ------------------------------------------------------------------------------------------------ the head
def make_head(B, N, F, seed, mask=True, zero_jet=False):
    """y, w, b, g, U, mu and a real-valued mask with exact zeros; jet 1 (when there is one) has a single real particle, and with
    ``zero_jet`` the last jet's mask is all zero (sum pooling only: the mean's divisor would be 1e-12)."""
    rs = np.random.RandomState(seed)
    t = lambda *s: torch.from_numpy(rs.normal(size=s))
    c = dict(y=t(B, N, F), w=t(1, F) / np.sqrt(F), b=t(1) * 0.3, g=t(B), U=t(B, N, F), mu=t(B, N, 1), mask=None,
             keep=torch.from_numpy((rs.uniform(size=B) >= 0.5) * 2.0))
    if mask:
        m = rs.uniform(0.1, 1.0, size=(B, N, 1))
        m[rs.uniform(size=(B, N, 1)) < 0.3] = 0.0
        m[:, 0] = 0.7
        if B > 1:
            m[1] = 0.0
            m[1, N // 2] = 1.0
        if zero_jet:
            m[B - 1] = 0.0
        c["mask"] = torch.from_numpy(m)
    return c


def ref_head(y, mask, w, b, mean, sigmoid, keep):
    """Pooling / Linear / keep / sigmoid as MPDiscriminator._post_mp, fnd_layer and the final activation compose them."""
    if mask is not None:
        x = (y * mask).sum(1)
        if mean:
            x = x / (mask.sum(1) + 1e-12)
    else:
        x = y.mean(1) if mean else y.sum(1)
    z = torch.nn.functional.linear(x, w, b).reshape(-1)
    if keep is not None:
        z = z * keep
    return torch.sigmoid(z) if sigmoid else z


def head_derivatives(c, mean, sigmoid, keep, op=None, use=("U", "mu"), conv=lambda t: t):
    """(out, first-order [y_bar, w_bar, b_bar, (m_bar)], second-order [dPhi/dg, /dy, /dw, /db, (/dm)], the second order once more)
    with Phi = <U, y_bar> + <mu, m_bar> over ``use``.  ``op(y, mask, w, b)``: the op under test; None: the reference."""
    y, w, b, g = (conv(c[n]).clone().requires_grad_(True) for n in ("y", "w", "b", "g"))
    m = None if c["mask"] is None else conv(c["mask"]).clone().requires_grad_(True)
    out = op(y, m, w, b) if op is not None else ref_head(y, m, w, b, mean, sigmoid, None if keep is None else conv(keep))
    wrt = [y, w, b] + ([m] if m is not None else [])
    first = torch.autograd.grad(out, wrt, g, create_graph=True)
    phi = 0
    if "U" in use:
        phi = phi + (first[0] * conv(c["U"])).sum()
    if "zeroU" in use:
        phi = phi + (first[0] * torch.zeros_like(first[0])).sum()
    if "mu" in use and m is not None:
        phi = phi + (first[3] * conv(c["mu"])).sum()
    targets = [g, y, w, b] + ([m] if m is not None else [])
    second = torch.autograd.grad(phi, targets, allow_unused=True, retain_graph=True)
    again = torch.autograd.grad(phi, targets, allow_unused=True)
    return out.detach(), [f.detach() for f in first], list(second), list(again)
