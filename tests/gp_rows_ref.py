"""Inputs and fp64 statements for the tests of the twice-differentiable edge aggregation (``ops.EdgeRowsFn``): seeded cases built on
the CPU, the edge network restated in plain torch -- with LeakyReLU's own signs, or with gates handed in (the project's
sign-conditioned comparison: the kernel's kink decisions, read from what it parked) --, and the derivatives autograd forms from it."""
import numpy as np
import torch

H1, H2, H3 = 96, 160, 192
ALPHA = 0.2

# name -> (seed, N, F, mask kind, dropout p, sum?, k (None: fully connected), mask takes a gradient?).  B = 3 everywhere.
# The seeds are picked so that torch fp32 on the CPU decides every live, kept pre-activation's sign as fp64 does
# (``fp32_flips`` == 0, asserted by the test): a sign that fp32 itself cannot hold is no fair demand on the kernel.
CASES = {
    "n5_sum": (0, 5, 3, "frac", 0.0, True, None, True),
    "n33_mean_drop": (0, 33, 3, "frac", 0.5, False, None, True),
    "n40_sparse_jets_drop": (0, 40, 3, "live4+dead", 0.5, True, None, True),
    "n40_sparse_jets_skipped": (0, 40, 3, "live4+dead", 0.0, False, None, False),
    "n9_knn4_drop": (0, 9, 3, "frac", 0.5, True, 4, True),
    "n30_two_receivers_per_workgroup": (0, 30, 32, "frac", 0.0, True, None, True),   # (the training shape: tiles straddle receivers)
}
B = 3


def make_case(name, seed=None):
    """The case ``name`` (``seed``: another seed than the table's, for picking one)."""
    seed0, N, F, kind, p, sum_agg, k, mask_grad = CASES[name]
    seed = seed0 if seed is None else seed
    g = torch.Generator().manual_seed(1000 + seed)
    r = lambda *shape, sc=1.0: (torch.randn(*shape, generator=g, dtype=torch.float64) * sc).float().double()   # (fp32-representable)
    P = [r(H1, 2 * F, sc=0.5), r(H1, sc=0.1), r(H2, H1, sc=0.1), r(H2, sc=0.1), r(H3, H2, sc=0.1), r(H3, sc=0.1)]
    x = r(B, N, F, sc=0.5)
    m = (torch.rand(B, N, generator=g, dtype=torch.float64) * 0.9 + 0.05).float().double()   # fractional, in (0, 1)
    if kind == "live4+dead":
        m[0, 4:] = 0.0      # four live senders: whole tiles of this jet are masked
        m[1, :] = 0.0       # every sender masked
    abar, u, mu = r(B, N, H3), r(B, N, F, sc=0.1), r(B, N, sc=0.1)      # (mu: both signs)
    adj = torch.ones(B, N, N, dtype=torch.bool)
    if k is not None:   # receiver i lists its k nearest senders (itself included), ties to the lower index
        d = (x.unsqueeze(1) - x.unsqueeze(2)).norm(dim=3)
        idx = torch.sort(d, dim=2, stable=True).indices[:, :, :k]
        adj = torch.zeros(B, N, N, dtype=torch.bool).scatter_(2, idx, True)
    return dict(name=name, N=N, F=F, p=p, sum_agg=sum_agg, k=k, mask_grad=mask_grad, P=P, x=x, m=m, abar=abar, u=u, mu=mu, adj=adj,
                s=1.0 if sum_agg else 1.0 / (k if k is not None else N))


def adjacency_words(adj):
    """[B, N, N] bool -> the int32 neighbour words [B * N, ceil(N / 32)] of ``ops.knn_sets`` (bit j of row (b, i): i lists j)."""
    Bn, N, _ = adj.shape
    NW = (N + 31) // 32
    a = np.zeros((Bn * N, NW * 32), dtype=np.uint64)
    a[:, :N] = adj.reshape(Bn * N, N).numpy()
    w = (a.reshape(Bn * N, NW, 32) << np.arange(32, dtype=np.uint64)).sum(2).astype(np.uint32)
    return torch.from_numpy(w.view(np.int32).copy())


def pre_activations(x, P, keeps, dtype):
    """(Z1, Z2, Z3) [B, N, N, .] of the edge network with LeakyReLU's own signs, in ``dtype``."""
    W1, b1, W2, b2, W3, b3 = (t.to(dtype) for t in P)
    x = x.to(dtype)
    Bn, N, F = x.shape
    lre = torch.nn.functional.leaky_relu
    A = torch.cat((x.unsqueeze(2).expand(Bn, N, N, F), x.unsqueeze(1).expand(Bn, N, N, F)), 3)
    Z1 = A @ W1.t() + b1
    Z2 = (keeps[0].to(dtype) * lre(Z1, ALPHA)) @ W2.t() + b2
    Z3 = (keeps[1].to(dtype) * lre(Z2, ALPHA)) @ W3.t() + b3
    return Z1, Z2, Z3


def gated_agg(x, m, P, G, s, adj):
    """agg with the gates (keep-and-scale times LeakyReLU') handed in as constants: what the rule differentiates."""
    W1, b1, W2, b2, W3, b3 = P
    Bn, N, F = x.shape
    A = torch.cat((x.unsqueeze(2).expand(Bn, N, N, F), x.unsqueeze(1).expand(Bn, N, N, F)), 3)
    E = G[0] * (A @ W1.t() + b1)
    E = G[1] * (E @ W2.t() + b2)
    E = G[2] * (E @ W3.t() + b3)
    w = adj.to(x.dtype).unsqueeze(3)
    return s * (E * (w if m is None else w * m.reshape(Bn, 1, N, 1))).sum(2)


def derivatives(f, c, mask_grad=True):
    """value, first-order outputs (x_bar, [m_bar,] six parameter gradients) and the gradients of Phi = <u, x_bar> [+ <mu, m_bar>]
    with respect to (a_bar, x, [m,] parameters) of agg = f(x, m, P); without ``mask_grad`` the mask is a constant."""
    ab, xx = (c[k].clone().requires_grad_(True) for k in ("abar", "x"))
    mm = c["m"].clone().requires_grad_(mask_grad)
    PP = [t.clone().requires_grad_(True) for t in c["P"]]
    wrt = [xx] + ([mm] if mask_grad else []) + PP
    agg = f(xx, mm, PP)
    first = torch.autograd.grad(agg, wrt, ab, create_graph=True)
    phi = (first[0] * c["u"].to(agg.dtype).to(agg.device)).sum()
    if mask_grad:
        phi = phi + (first[1] * c["mu"].to(agg.dtype).to(agg.device)).sum()
    second = torch.autograd.grad(phi, [ab] + wrt, allow_unused=True)
    second = [torch.zeros_like(t) if g is None else g for g, t in zip(second, [ab] + wrt)]
    names = ["x"] + (["m"] if mask_grad else []) + ["W1", "b1", "W2", "b2", "W3", "b3"]
    return agg.detach(), dict(zip(names, (t.detach() for t in first))), dict(zip(["abar"] + names, second))


def live_kept(c, keeps):
    """Per layer, the elements whose sign matters: edges that exist, senders with a non-zero mask, elements kept by dropout."""
    live = (c["adj"] & (c["m"] != 0).unsqueeze(1)).unsqueeze(3)
    return [live & (k > 0) for k in keeps]


def fp32_flips(c, keeps):
    """How many live, kept pre-activation signs torch fp32 on the CPU decides differently from fp64."""
    z64, z32 = pre_activations(c["x"], c["P"], keeps, torch.float64), pre_activations(c["x"], c["P"], keeps, torch.float32)
    return sum(int((((a > 0) != (b > 0)) & w).sum()) for a, b, w in zip(z64, z32, live_kept(c, keeps)))
