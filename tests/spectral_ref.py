"""The fp64 torch statement of ``mpg_spectral_norm`` / ``mpg_spectral_norm_bwd`` (include/mpgan_amd.h) and the cases the host
and the GPU tests of the spectral-norm kernels share (tests/test_spectral_cpu.py, tests/test_gpu_spectral.py)."""
import numpy as np
import torch

TIGHT = 1e-4
# 1 x 1; C and R below a wave; the discriminator's first edge layer (96 x 6); R and C beyond a 64-column tile and beyond the 16
# waves, each on its own; the node network's layers (256 x 224, 256 x 256)
SHAPES = [(1, 1), (8, 5), (6, 8), (96, 6), (300, 7), (16, 300), (256, 224), (256, 256)]
ITERATIONS = [0, 1, 3]


def power_iteration(W, u, v, P):
    """(u', v', sigma) after P passes, in the dtype of the arguments; nothing is written."""
    for _ in range(P):
        t = torch.mv(W.t(), u)
        v = t / (t.norm() + 1e-12)
        s = torch.mv(W, v)
        u = s / (s.norm() + 1e-12)
    return u, v, u.dot(torch.mv(W, v))


def forward_ref(W, u, v, P):
    """fp64: dict(W_eff, u, v, inv_sigma) of float32 inputs, u and v as constants of W_eff's differentiation."""
    W, u, v = W.double(), u.double(), v.double()
    with torch.no_grad():
        un, vn, _ = power_iteration(W, u, v, P)
    sigma = un.dot(torch.mv(W, vn))
    inv = 1.0 / (sigma + 1e-12)
    return {"W_eff": W * inv, "u": un, "v": vn, "inv_sigma": inv.reshape(1)}


def backward_ref(G, W_eff, u, v, inv_sigma, dW0=None):
    """fp64: dW0 + (G - <G, W_eff> u v^T) * inv_sigma."""
    G, W_eff, u, v = G.double(), W_eff.double(), u.double(), v.double()
    d = (G - (G * W_eff).sum() * torch.outer(u, v)) * inv_sigma.double()
    return d if dW0 is None else dW0.double() + d


def make_layer(R, C, P, seed):
    """float32 (W, u, v) of one layer: W ~ N(0, 1 / C) as nn.Linear scales it, u and v unit vectors as SpectralNorm draws them.
    For P = 0 the vectors are taken two fp64 passes on: sigma = u . W v of two RANDOM unit vectors is a sum that cancels to
    ~1 / sqrt(R C) of its terms, which no fp32 evaluation resolves to a fixed relative bar; P = 0 is the mode of vectors that have
    been iterated before."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * R + C)
    W = torch.randn(R, C, generator=g) / float(C) ** 0.5
    u = torch.nn.functional.normalize(torch.randn(R, generator=g), dim=0, eps=1e-12)
    v = torch.nn.functional.normalize(torch.randn(C, generator=g), dim=0, eps=1e-12)
    if P == 0:
        u64, v64, _ = power_iteration(W.double(), u.double(), v.double(), 2)
        u, v = u64.float(), v64.float()
    return W.contiguous(), u.contiguous(), v.contiguous()


def rel_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    den = np.abs(b).max()
    return float(np.abs(a - b).max() / (den if den > 0 else 1.0))


def scaled_err(a, b, scale):
    """max|a - b| over ``scale`` (``terms_scale``): for a result that is a DIFFERENCE of terms of that magnitude -- dW with
    G = W_eff, where G and <G, W_eff> u v^T cancel along the leading singular pair, exactly so for a rank-one W, whose dW vanishes
    for every G: such a result is known to the rounding of its terms, not of itself."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / scale)


def terms_scale(G, W_eff, u, v, inv_sigma, dW0=None):
    """The magnitude of the largest TERM of dW = dW0 + G inv_sigma - <G, W_eff> u v^T inv_sigma (fp64): ``scaled_err``'s scale."""
    G, W_eff, u, v, inv = G.double(), W_eff.double(), u.double(), v.double(), inv_sigma.double().abs()
    s = max(float(G.abs().max() * inv), float((G * W_eff).sum().abs() * u.abs().max() * v.abs().max() * inv))
    return s if dW0 is None else max(s, float(dW0.abs().max()))


def check_forward(got, W, u0, v0, P, what=""):
    """``got`` = (W_eff, u_out, v_out, inv_sigma, u after, v after) against the fp64 statement on the float32 inputs."""
    ref = forward_ref(W, u0, v0, P)
    W_eff, u_out, v_out, inv, u_now, v_now = (t.detach().cpu() for t in got)
    errs = {"W_eff": rel_err(W_eff, ref["W_eff"]), "u_out": rel_err(u_out, ref["u"]), "v_out": rel_err(v_out, ref["v"]),
            "inv_sigma": rel_err(inv, ref["inv_sigma"]), "u": rel_err(u_now, ref["u"] if P else u0.double()),
            "v": rel_err(v_now, ref["v"] if P else v0.double())}
    assert max(errs.values()) < TIGHT, (what, errs)
    if P == 0:   # neither vector is written
        assert torch.equal(u_now, u0) and torch.equal(v_now, v0), what
    else:        # the fresh copies are what was stored in place
        assert torch.equal(u_now, u_out) and torch.equal(v_now, v_out), what
    return ref
