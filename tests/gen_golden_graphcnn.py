"""Fixtures of the GraphCNN-GAN generator, from the reference's own ``GraphCNNGANG`` (``ext_models/ext_models.py:75-157``).

PyG and torch_cluster are not needed: the reference module is imported through ``gen_golden_baselines.reference_module()`` and its
``NNConv``, ``knn_graph`` and ``torch_geometric.nn.BatchNorm`` are replaced by the per-edge restatements below (PyG 1.x semantics
as the reference uses them), so the reference's own constructor and forward drive them.

  tests/golden/graphcnn.npz                        graphcnng_layers [6, 5], N = 10, k = 4, B = 4, training mode, fp64: state dict,
                                                   noise, output, noise gradient and every parameter gradient for a stored cotangent
  tests/golden/published_graphcnn_g_weights.npz    the published generator's state dict (trained_models/graphcnn_g)
  tests/golden/published_graphcnn_g.npz            the reference's fp64 output for 4 jets on stored noise (sigma 0.2), eval mode

Seeds: of ``range(300)`` the one with the largest rank margin (``nnconv_ref.rank_margin``: how far the k-th and (k+1)-th neighbour
distances of any node of any layer are apart, and the nearest neighbour from the node itself, relative to the node's largest
distance); for the small net the smaller of that and the LeakyReLU margin (smallest |z| / max|z| over the pre-activations) decides.
The margins are stored.  No fixture is written with a rank margin below 1e-4 -- two orders above fp32 rounding of a distance, so
fp32 and fp64 pick the same neighbours.

    python tests/gen_golden_graphcnn.py        (needs the reference checkout: MPGAN_REFERENCE)
"""
import os
import sys
import types

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from gen_golden import OUT, REF, save_parts  # noqa: E402
from gen_golden_baselines import reference_module  # noqa: E402
import nnconv_ref as R  # noqa: E402

MIN_RANK_MARGIN = 1e-4
SMALL = dict(latent_dim=7, num_hits=10, graphcnng_layers=[6, 5], node_feat_size=3, num_knn=4, leaky_relu_alpha=0.2,
             graphcnng_tanh=True, device="cpu")
PUBLISHED = dict(latent_dim=128, num_hits=30, graphcnng_layers=[32, 24], node_feat_size=3, num_knn=20, leaky_relu_alpha=0.2,
                 graphcnng_tanh=False, device="cpu")
B = 4


def knn_graph(x, k, batch=None, loop=False):
    """``torch_cluster.knn_graph`` for jets of equal size: edge_index [2, E], row 0 the source j, row 1 the target i."""
    counts = torch.bincount(batch)
    N = int(counts[0])
    assert bool((counts == N).all())
    adj = R.knn_adjacency(x.detach().reshape(-1, N, x.shape[1]), k, loop)
    b, i, j = adj.nonzero(as_tuple=True)
    return torch.stack([b * N + j, b * N + i])


class NNConv(nn.Module):
    """PyG 1.x's NNConv, edge by edge."""

    def __init__(self, in_channels, out_channels, nn, aggr="add", root_weight=True, bias=True):
        super().__init__()
        assert aggr == "mean" and root_weight and bias
        self.in_channels, self.out_channels, self.nn = in_channels, out_channels, nn
        self.root = torch.nn.Parameter(torch.empty(in_channels, out_channels))
        self.bias = torch.nn.Parameter(torch.empty(out_channels))
        bound = 1.0 / np.sqrt(in_channels)
        self.root.data.uniform_(-bound, bound)
        self.bias.data.uniform_(-bound, bound)

    def forward(self, x, edge_index, edge_attr):
        src, dst = edge_index
        weight = self.nn(edge_attr).view(-1, self.in_channels, self.out_channels)
        msg = torch.matmul(x[src].unsqueeze(1), weight).squeeze(1)
        agg = torch.zeros(x.shape[0], self.out_channels, dtype=x.dtype).index_add_(0, dst, msg)
        cnt = torch.zeros(x.shape[0], dtype=x.dtype).index_add_(0, dst, torch.ones_like(dst, dtype=x.dtype))
        return agg / cnt.clamp(min=1.0).unsqueeze(1) + x @ self.root + self.bias


class BatchNorm(nn.Module):
    def __init__(self, in_channels):
        super().__init__()
        self.module = nn.BatchNorm1d(in_channels)

    def forward(self, x):
        return self.module(x)


def patched_reference():
    ref = reference_module()
    ref.NNConv, ref.knn_graph = NNConv, knn_graph
    ref.torch_geometric.nn.BatchNorm = BatchNorm
    return ref


def margins(net, cfg, noise, training):
    sd = {k: v.detach() for k, v in net.state_dict().items()}
    probe = {}
    R.generator(sd, noise, cfg["num_hits"], cfg["num_knn"], cfg["leaky_relu_alpha"], cfg["graphcnng_tanh"], training, probe=probe)
    mz = min(float(z.abs().min() / z.abs().max()) for z in probe["z"])
    return R.rank_margin(probe["x"], cfg["num_knn"], cfg["num_knn"] == cfg["num_hits"]), mz


def build_small(ref, seed):
    torch.manual_seed(seed)
    net = ref.GraphCNNGANG(types.SimpleNamespace(**SMALL)).double().train()
    g = torch.Generator().manual_seed(seed)
    noise = torch.randn(B, SMALL["latent_dim"], generator=g, dtype=torch.float64)
    cot = torch.randn(B, SMALL["num_hits"], SMALL["node_feat_size"], generator=g, dtype=torch.float64)
    return net, noise, cot


def main():
    if not os.path.isdir(REF):
        print(f"reference not found at {REF}; nothing generated")
        return 0
    ref = patched_reference()
    os.makedirs(OUT, exist_ok=True)

    best = None
    for seed in range(300):
        net, noise, _ = build_small(ref, seed)
        mr, mz = margins(net, SMALL, noise, True)
        if best is None or min(mr, mz) > best[0]:
            best = (min(mr, mz), seed, mr, mz)
    _, seed, mr, mz = best
    print("small net: seed", seed, "rank margin", mr, "min |z| / max|z|", mz)
    if mr < MIN_RANK_MARGIN:
        raise SystemExit(f"graphcnn.npz: rank margin {mr} below {MIN_RANK_MARGIN}; not written")
    net, noise, cot = build_small(ref, seed)
    arrays = {"seed": np.array(seed), "margin_rank": np.array(mr), "margin_z": np.array(mz), "noise": noise.numpy(), "cot": cot.numpy()}
    for k, v in net.state_dict().items():
        arrays[f"sd.{k}"] = v.detach().numpy().copy()
    xi = noise.clone().requires_grad_(True)
    out = net(xi)
    (out * cot).sum().backward()
    arrays.update(out=out.detach().numpy(), dnoise=xi.grad.numpy())
    for k, p in net.named_parameters():
        arrays[f"grad.{k}"] = p.grad.numpy()
    for k, v in net.state_dict().items():            # the running statistics after this one training forward
        if "running" in k or "num_batches" in k:
            arrays[f"after.{k}"] = v.detach().numpy().copy()
    np.savez_compressed(os.path.join(OUT, "graphcnn.npz"), **arrays)

    sd = torch.load(os.path.join(REF, "trained_models", "graphcnn_g", "G_best_epoch.pt"), map_location="cpu")
    G = ref.GraphCNNGANG(types.SimpleNamespace(**PUBLISHED))
    print("graphcnn_g", G.load_state_dict(sd), len(sd), "entries", sum(v.numel() for v in sd.values()), "numbers")
    save_parts("published_graphcnn_g_weights", {k: v.numpy() for k, v in sd.items()})
    G = G.double().eval()
    best = None
    for seed in range(300):
        noise = torch.randn(B, PUBLISHED["latent_dim"], generator=torch.Generator().manual_seed(seed)) * 0.2
        mr, _ = margins(G, PUBLISHED, noise.double(), False)
        if best is None or mr > best[0]:
            best = (mr, seed)
    mr, seed = best
    print("published: seed", seed, "rank margin", mr)
    if mr < MIN_RANK_MARGIN:
        raise SystemExit(f"published_graphcnn_g.npz: rank margin {mr} below {MIN_RANK_MARGIN}; not written")
    noise = torch.randn(B, PUBLISHED["latent_dim"], generator=torch.Generator().manual_seed(seed)) * 0.2
    with torch.no_grad():
        out = G(noise.double())
    np.savez_compressed(os.path.join(OUT, "published_graphcnn_g.npz"), seed=np.array(seed), margin_rank=np.array(mr),
                        noise=noise.numpy(), out=out.numpy())
    return 0


if __name__ == "__main__":
    sys.exit(main())
