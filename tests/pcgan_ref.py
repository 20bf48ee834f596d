"""PCGAN's set encoder (rkansal47/MPGAN ``ext_models/pcgan_model.py:4-144``) restated in plain torch, in whatever dtype its inputs
have: the equivariant stack with the max behind it as ``ops.set_encode_launch`` (mpg_set_encode_fwd) computes it, and the whole
encoder from a state dict.  Not a test: tests/test_pcgan_cpu.py checks it against the reference's own results
(tests/golden/pcgan.npz) and tests/test_gpu_set_encode.py uses it in fp64 as the yardstick of the kernel.

``pool``: 1 = max1 (PermEqui1_max), 2 = max (PermEqui2_max), 3 = mean (PermEqui2_mean); ``act``: 2 = tanh, 3 = softplus."""
import torch
import torch.nn.functional as F

POOLS = {"max1": 1, "max": 2, "mean": 3}
ACTS = {"tanh": 2, "softplus": 3}


def activation(z, act):
    return torch.tanh(z) if act == 2 else F.softplus(z)


def stack(x, gammas, biases, lambdas, pool, act, probe=None):
    """pooled [B, D_{L-1}] = max_n h_L of ``x`` [B, N, K_0].  ``probe``: a dict that receives the pre-activations ``z`` per layer."""
    h = x
    for l, G in enumerate(gammas):
        m = h.mean(1, keepdim=True) if pool == 3 else h.max(1, keepdim=True)[0]
        if pool == 1:
            z = (h - m) @ G.t()
        else:
            z = h @ G.t() - m @ lambdas[l].t()
        if biases[l] is not None:
            z = z + biases[l]
        if probe is not None:
            probe.setdefault("z", []).append(z)
        h = activation(z, act)
    return h.max(1)[0]


def stack_weights(sd, pool, prefix="phi."):
    """(gammas, biases, lambdas) of the three equivariant layers out of an encoder's state dict."""
    idx = (0, 2, 4)
    return ([sd[f"{prefix}{i}.Gamma.weight"] for i in idx], [sd[f"{prefix}{i}.Gamma.bias"] for i in idx],
            [sd[f"{prefix}{i}.Lambda.weight"] for i in idx] if pool != 1 else [None] * 3)


def encoder(sd, x, pool, act):
    """``G_inv_Tanh`` (act 2) / ``G_inv`` (act 3) from its state dict: the stack, the max, ``ro``."""
    s = stack(x, *stack_weights(sd, pool), pool, act)
    return activation(s @ sd["ro.0.weight"].t() + sd["ro.0.bias"], act) @ sd["ro.2.weight"].t() + sd["ro.2.bias"]


def random_stack(widths, pool, gen, dtype=torch.float64, scale=1.0):
    """Random weights of a stack over ``widths`` = [K_0, D_0, .., D_{L-1}]: entries ~ N(0, scale^2 / K_l), biases ~ N(0, 1 / 4)."""
    rn = lambda *s, std: torch.randn(*s, generator=gen, dtype=dtype) * std
    gammas = [rn(d, k, std=scale / k ** 0.5) for k, d in zip(widths[:-1], widths[1:])]
    biases = [rn(d, std=0.5) for d in widths[1:]]
    lambdas = [rn(d, k, std=scale / k ** 0.5) if pool != 1 else None for k, d in zip(widths[:-1], widths[1:])]
    return gammas, biases, lambdas


def negative_jets(B, N, K, gen, dtype=torch.float64):
    """Inputs with every x <= -1: a zero-filled pad row would win a max and would dilute a mean."""
    return -1.0 - torch.randn(B, N, K, generator=gen, dtype=dtype).abs()
