"""The TreeGCN layer (rkansal47/MPGAN ``ext_models/ext_models.py:254-282``, ``upsample``) restated in plain torch, in whatever dtype
its inputs have: the literal form, the collapsed form that ``ops.tree_gcn`` (mpg_tree_gcn_fwd / _bwd) computes, and the hand-written
backward of the collapsed form.  Not a test: tests/test_treegan_cpu.py and tests/test_gpu_treegan.py share it.

A layer's weights are a dict ``W_root`` (list of [out, width_i]), ``W_branch`` [P, in, g in], ``W0`` [in s, in], ``W1`` [out, in s],
``bias`` [1, g, out] or None (the last layer: no bias, no activation).  ``levels``: tree[0 .. d], [B, P_i, width_i]."""
import torch
import torch.nn.functional as F

ALPHA = 0.2


def layer_weights(sd, d, act=True, prefix="gcn.TreeGCN_"):
    """The weights of layer ``d`` out of a TreeGANG state dict."""
    k = f"{prefix}{d}."
    return {"W_root": [sd[f"{k}W_root.{i}.weight"] for i in range(d + 1)], "W_branch": sd[k + "W_branch"],
            "W0": sd[k + "W_loop.0.weight"], "W1": sd[k + "W_loop.1.weight"], "bias": sd[k + "bias"] if act else None}


def random_layer(features, degrees, d, support, act, gen, dtype=torch.float64, scale=1.0):
    """Random weights of layer ``d`` (unit-variance products: entries ~ N(0, 1 / fan_in)) and random levels for B jets are the
    caller's; this gives the weights."""
    P = 1
    for g in degrees[:d]:
        P *= g
    g, inn, out = degrees[d], features[d], features[d + 1]
    rn = lambda *s, fan: torch.randn(*s, generator=gen, dtype=dtype) * scale / fan ** 0.5
    return {"W_root": [rn(out, features[i], fan=features[i] * (d + 1)) for i in range(d + 1)],
            "W_branch": rn(P, inn, g * inn, fan=inn), "W0": rn(inn * support, inn, fan=inn),
            "W1": rn(out, inn * support, fan=inn * support), "bias": rn(1, g, out, fan=4.0) if act else None}


def random_levels(features, degrees, d, B, gen, dtype=torch.float64):
    """Levels 0 .. d of DISTINCT random values (a wrong ancestor index shows)."""
    out, P = [], 1
    for i in range(d + 1):
        out.append(torch.randn(B, P, features[i], generator=gen, dtype=dtype))
        P *= degrees[i]
    return out


def literal(levels, w):
    """The reference's lines, repeat / view included, through the [rows, in s] activation."""
    B, node = levels[0].size(0), levels[-1].size(1)
    out, inn = w["W1"].shape[0], levels[-1].size(2)
    g = w["W_branch"].shape[2] // inn
    root = 0
    for x, W in zip(levels, w["W_root"]):
        root = root + F.linear(x, W).repeat(1, 1, node // x.size(1)).view(B, -1, out)
    branch = F.leaky_relu(levels[-1].unsqueeze(2) @ w["W_branch"], ALPHA).view(B, node * g, inn)
    branch = F.linear(F.linear(branch, w["W0"]), w["W1"])
    branch = root.repeat(1, 1, g).view(B, -1, out) + branch
    if w["bias"] is not None:
        branch = F.leaky_relu(branch + w["bias"].repeat(1, node, 1), ALPHA)
    return branch


def ancestors(P, Pi):
    """anc_i(p) = p // (P / P_i) for p < P."""
    return torch.arange(P) // (P // Pi)


def collapsed(levels, w, probe=None):
    """The restatement: integer-division ancestors, Wc = W1 W0.  Returns (tree[d + 1], u [B, P g, in])."""
    B, P, inn = levels[-1].shape
    g = w["W_branch"].shape[2] // inn
    Wc = w["W1"] @ w["W0"]
    root = sum(x[:, ancestors(P, x.size(1))] @ W.t() for x, W in zip(levels, w["W_root"]))          # [B, P, out]
    zu = torch.einsum("bpk,pkn->bpn", levels[-1], w["W_branch"])
    u = F.leaky_relu(zu, ALPHA).reshape(B, P * g, inn)
    h = u @ Wc.t() + root.repeat_interleave(g, dim=1)
    if probe is not None:
        probe.setdefault("z", []).append(zu)
    if w["bias"] is None:
        return h, u
    z = h + w["bias"].repeat(1, P, 1)
    if probe is not None:
        probe["z"].append(z)
    return F.leaky_relu(z, ALPHA), u


def slope(t):
    return torch.where(t > 0, torch.ones_like(t), torch.full_like(t, ALPHA))


def backward(levels, w, y, u, dy):
    """The hand-written backward of ``collapsed``: (dlevels, dict of weight gradients).  The signs are read from the stored
    outputs y and u."""
    B, P, inn = levels[-1].shape
    g, out = w["W_branch"].shape[2] // inn, w["W1"].shape[0]
    Wc = w["W1"] @ w["W0"]
    act = w["bias"] is not None
    dz = dy * slope(y) if act else dy
    grads = {"bias": dz.reshape(B, P, g, out).sum((0, 1)).unsqueeze(0) if act else None}
    M = dz.reshape(-1, out).t() @ u.reshape(-1, inn)
    grads["W0"], grads["W1"] = w["W1"].t() @ M, M @ w["W0"].t()
    du = (dz @ Wc).reshape(B, P, g * inn) * slope(u.reshape(B, P, g * inn))
    grads["W_branch"] = torch.einsum("bpk,bpn->pkn", levels[-1], du)
    dlev = [torch.zeros_like(x) for x in levels]
    dlev[-1] += torch.einsum("bpn,pkn->bpk", du, w["W_branch"])
    S = dz.reshape(B, P, g, out).sum(2)
    grads["W_root"] = []
    for i, (x, W) in enumerate(zip(levels, w["W_root"])):
        Pi = x.size(1)
        Si = S.reshape(B, Pi, P // Pi, out).sum(2)
        grads["W_root"].append(Si.reshape(-1, out).t() @ x.reshape(-1, x.size(2)))
        dlev[i] += Si @ W
    return dlev, grads


def generator(sd, noise, nlayers, fn=collapsed):
    """A whole TreeGANG on a state dict: [B, prod(degrees), features[-1]]."""
    levels = [noise]
    for d in range(nlayers):
        y = fn(levels, layer_weights(sd, d, act=d < nlayers - 1))
        levels.append(y[0] if isinstance(y, tuple) else y)
    return levels[-1]
