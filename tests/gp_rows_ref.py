"""Inputs and fp64 statements for the tests of the twice-differentiable edge aggregation (``ops.EdgeRowsFn``): seeded cases built on
the CPU, the edge network restated in plain torch -- with LeakyReLU's own signs, or with gates handed in (the project's
sign-conditioned comparison: the kernel's kink decisions, read from what it parked) --, and the derivatives autograd forms from it."""
from collections import namedtuple

import numpy as np
import torch

H1, H2, H3 = 96, 160, 192
ALPHA = 0.2

# name -> (seed, N, F, mask kind, dropout p, sum?, k (None: fully connected), mask takes a gradient?).  B = 3 in all of these.
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

# The launch shapes the six cases above never take (each is a case of the same GPU test, tests/test_gpu_gp_rows.py; too large for
# the CPU suite, which iterates ``CASES`` alone).  ``there_for``: by launch plan the case runs under -- "planned" is ``ops.knn_plan`` as
# it is, "full_blocks" the plan of a launch with workgroups to spare (``ops.NUM_CUS`` patched to 1: as many receivers per workgroup
# as fit, the plan a training batch gets) -- what the case is there for under it; tests/test_gp_rows_cpu.py asserts
# every such property from ``ops.knn_plan`` / ``ops.knn_block_tiles``, so a change of the plan names the case that lost its path:
#   tiles_gt4          more than four tiles per workgroup: the waves' tile loop makes a second trip
#   tiles_eq4_short    exactly four tiles in the first workgroup, the last of them short
#   training_rw        the RW that ``knn_plan`` gives B = 256 jets of this N and k on the whole chip
#   straddle           some tile holds rows of more than one receiver
#   short_tile         some workgroup's last tile has fewer than 32 rows
#   short_workgroup    the jet's last workgroup has fewer receivers than the others
#   receiver_blocks    more than one workgroup per jet
#   one_tile           every workgroup is a single tile, and it holds every receiver of the jet
#   words_N            N neighbour words per receiver (words_2, words_5, words_6)
#   sparse_words       k < N over more than one word: the rank of a sender counts bits of several words
#   k_not_dividing_32  32 % k != 0
#   k1                 every receiver lists one sender
#   stage_gt_100k      more than 100 KiB of stage LDS per workgroup (every case stays within ``ops.KNN_LDS_BYTES``)
#   dmask_three_waves  N > 128: ``knn_dmask_kernel`` has hits to compact in all three of its waves
#   dmask_hits_three_waves  some sender is listed by receivers below 64, in 64..127 and from 128 on
#   dmask_all_threads  N = 192: every thread of ``knn_dmask_kernel`` looks at a receiver
#   skipped_tile       the mask takes no gradient and some 32-row tile beyond a workgroup's fourth has no unmasked sender
#   byte_drop          dropout in byte mode (a keep word per group of 8 features: every p but 0.5)
#   bit_drop           dropout in bit mode (p = 0.5)
#   no_mask            no mask is passed
#   slice_x            x is a feature-slice view ``x4[..., :F]`` of a [B, N, F + 1] tensor (row stride F + 1)
# The seeds: as for ``CASES``, ``fp32_flips`` == 0, which the test asserts.  Seed 0 gives that in every case, the three of some 10^7
# pre-activations included (n192_fc: 0 flips of 16.5 million on the CPU); without dropout the count is the CPU's alone and was
# taken there before any GPU run, with dropout the keep words are the device's and the count was taken with them.
PlanCase = namedtuple("PlanCase", "seed B N F kind p sum_agg k mask_grad slice_x there_for")
_TRAIN = ("tiles_eq4_short", "training_rw", "straddle", "short_tile", "short_workgroup", "receiver_blocks", "words_1")
PLAN_CASES = {
    "n30_training_plan": PlanCase(0, 3, 30, 32, "frac", 0.0, True, None, True, False, {"full_blocks": _TRAIN}),
    "n30_training_plan_byte": PlanCase(0, 3, 30, 3, "frac", 0.3, False, None, True, True,
                                       {"full_blocks": _TRAIN + ("byte_drop", "slice_x")}),
    "n150_fc": PlanCase(0, 1, 150, 3, "tail", 0.5, True, None, True, False,
                        {"planned": ("tiles_gt4", "short_tile", "words_5", "dmask_three_waves", "stage_gt_100k", "bit_drop")}),
    "n150_fc_skipped": PlanCase(0, 1, 150, 3, "tail", 0.0, False, None, False, False,
                                {"planned": ("tiles_gt4", "skipped_tile", "words_5", "stage_gt_100k")}),
    "n192_fc": PlanCase(0, 1, 192, 3, "frac", 0.0, False, None, True, False,
                        {"planned": ("tiles_gt4", "words_6", "dmask_all_threads", "dmask_three_waves", "stage_gt_100k")}),
    "n40_knn7": PlanCase(0, 2, 40, 32, "frac", 0.3, True, 7, True, False,
                         {"planned": ("words_2", "sparse_words", "k_not_dividing_32", "short_tile", "straddle", "byte_drop"),
                          "full_blocks": ("words_2", "sparse_words", "k_not_dividing_32", "tiles_eq4_short", "short_workgroup", "straddle",
                                          "byte_drop")}),
    "n150_knn20": PlanCase(0, 2, 150, 32, "frac", 0.0, False, 20, True, False,
                           {"planned": ("words_5", "sparse_words", "k_not_dividing_32", "dmask_three_waves", "receiver_blocks", "dmask_hits_three_waves"),
                            "full_blocks": ("words_5", "sparse_words", "k_not_dividing_32", "dmask_three_waves", "receiver_blocks",
                                            "tiles_eq4_short", "straddle", "dmask_hits_three_waves")}),
    "n30_knn1": PlanCase(0, 3, 30, 3, "frac", 0.5, True, 1, True, False, {"planned": ("k1", "one_tile", "bit_drop")}),
    "n9_nomask": PlanCase(0, 3, 9, 3, "none", 0.0, True, None, False, False, {"planned": ("no_mask", "straddle")}),
}
PLAN_RUNS = [(name, plan) for name, pc in PLAN_CASES.items() for plan in pc.there_for]


def case_fields(name):
    """(seed, B, N, F, mask kind, p, sum?, k, mask takes a gradient?, slice_x) of a case of either table."""
    if not isinstance(name, str):     # (a ``PlanCase`` of the caller's own)
        return tuple(name[:10])
    if name in CASES:
        seed, N, F, kind, p, sum_agg, k, mask_grad = CASES[name]
        return seed, B, N, F, kind, p, sum_agg, k, mask_grad, False
    return tuple(PLAN_CASES[name][:10])


def make_case(name, seed=None, B=None):
    """The case ``name`` of ``CASES`` or ``PLAN_CASES`` (``seed``: another seed than the table's, for picking one; ``B``: another
    number of jets).  ``m`` is None where no mask is passed."""
    seed0, B0, N, F, kind, p, sum_agg, k, mask_grad, slice_x = case_fields(name)
    seed, B = seed0 if seed is None else seed, B0 if B is None else B
    g = torch.Generator().manual_seed(1000 + seed)
    r = lambda *shape, sc=1.0: (torch.randn(*shape, generator=g, dtype=torch.float64) * sc).float().double()   # (fp32-representable)
    P = [r(H1, 2 * F, sc=0.5), r(H1, sc=0.1), r(H2, H1, sc=0.1), r(H2, sc=0.1), r(H3, H2, sc=0.1), r(H3, sc=0.1)]
    x = r(B, N, F, sc=0.5)
    m = (torch.rand(B, N, generator=g, dtype=torch.float64) * 0.9 + 0.05).float().double()   # fractional, in (0, 1)
    if kind == "live4+dead":
        m[0, 4:] = 0.0      # four live senders: whole tiles of this jet are masked
        m[1, :] = 0.0       # every sender masked
    elif kind == "tail":
        m[:, N - N // 3:] = 0.0     # jet-like: the last third of every jet is padding
    elif kind == "none":
        m = None
    else:
        assert kind == "frac", kind
    abar, u, mu = r(B, N, H3), r(B, N, F, sc=0.1), r(B, N, sc=0.1)      # (mu: both signs)
    adj = torch.ones(B, N, N, dtype=torch.bool)
    if k is not None:   # receiver i lists its k nearest senders (itself included), ties to the lower index
        d = (x.unsqueeze(1) - x.unsqueeze(2)).norm(dim=3)
        idx = torch.sort(d, dim=2, stable=True).indices[:, :, :k]
        adj = torch.zeros(B, N, N, dtype=torch.bool).scatter_(2, idx, True)
    return dict(name=name, B=B, N=N, F=F, p=p, sum_agg=sum_agg, k=k, mask_grad=mask_grad, slice_x=slice_x, P=P, x=x, m=m, abar=abar, u=u,
                mu=mu, adj=adj, s=1.0 if sum_agg else 1.0 / (k if k is not None else N))


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
    with respect to (a_bar, x, [m,] parameters) of agg = f(x, m, P); without ``mask_grad`` the mask is a constant (None: no mask)."""
    ab, xx = (c[k].clone().requires_grad_(True) for k in ("abar", "x"))
    mm = None if c["m"] is None else c["m"].clone().requires_grad_(mask_grad)
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
    live = (c["adj"] if c["m"] is None else c["adj"] & (c["m"] != 0).unsqueeze(1)).unsqueeze(3)
    return [live & (k > 0) for k in keeps]


def fp32_flips(c, keeps):
    """How many live, kept pre-activation signs torch fp32 on the CPU decides differently from fp64."""
    z64, z32 = pre_activations(c["x"], c["P"], keeps, torch.float64), pre_activations(c["x"], c["P"], keeps, torch.float32)
    return sum(int((((a > 0) != (b > 0)) & w).sum()) for a, b, w in zip(z64, z32, live_kept(c, keeps)))
