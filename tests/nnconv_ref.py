"""fp64 restatement of the GraphCNN-GAN generator's pieces (rkansal47/MPGAN ``ext_models/ext_models.py:75-157``) as the reference
uses PyG 1.x's ``NNConv`` and ``torch_cluster.knn_graph``: the test-side reference of tests/test_graphcnn_cpu.py and
tests/test_gpu_graphcnn.py, and the stand-ins tests/gen_golden_graphcnn.py drives the reference's own class with.

  knn_adjacency     the graph per jet as a 0 / 1 matrix [B, N, N] (receiver i, sender j): the k nearest in Euclidean distance over
                    all features, self excluded unless ``loop``, stable sort (index order on ties), fewer than k candidates: all
  pack_bits         that matrix as the bit words ``mpg_knn_sets`` writes ([B N, ceil(N / 32)] int32)
  literal           NNConv, aggr mean, root weight, bias, edge attribute x_j - x_i: a weight matrix per edge
  factorised        y_i = vec(P_i) W3 + m_i Bn + x_i root + bias -- returns (y, P, m)
  backward          the closed-form gradients of the factorised layer
  generator         a whole ``GraphCNNGANG`` forward from a state dict
  rank_margin       how decided an input's neighbour sets are

Parameter layouts (PyG 1.x, as in the published files): nn.weight [Cin Cout, Cin], nn.bias [Cin Cout], root [Cin, Cout], bias [Cout]."""
import numpy as np
import torch
import torch.nn.functional as F


def knn_adjacency(x, k, loop):
    B, N, _ = x.shape
    d = (x.unsqueeze(1) - x.unsqueeze(2)).pow(2).sum(-1)      # [B, i, j]
    order = torch.sort(d, dim=2, stable=True).indices
    first = 0 if loop else 1
    adj = torch.zeros(B, N, N, dtype=x.dtype)
    return adj.scatter_(2, order[:, :, first:first + k], 1.0)


def pack_bits(adj):
    """[B, N, N] 0 / 1 -> int32 words [B N, ceil(N / 32)], bit j & 31 of word j >> 5 of row (b, i)."""
    B, N, _ = adj.shape
    W = (N + 31) // 32
    a = np.zeros((B * N, W * 32), dtype=np.uint64)
    a[:, :N] = adj.reshape(B * N, N).numpy() != 0
    words = (a.reshape(B * N, W, 32) << np.arange(32, dtype=np.uint64)).sum(2).astype(np.uint32)
    return torch.from_numpy(words.view(np.int32).copy())


def unpack_bits(words, B, N):
    w = words.numpy().view(np.uint32).astype(np.uint64)
    bits = (w[:, :, None] >> np.arange(32, dtype=np.uint64)) & 1
    return torch.from_numpy(bits.reshape(B, N, -1)[:, :, :N].astype(np.float64))


def literal(x, adj, nn_weight, nn_bias, root, bias):
    """x [B, N, Cin], adj [B, N, N] -> y [B, N, Cout]: every listed edge with its own [Cin, Cout] weight, mean over the listed."""
    B, N, Cin = x.shape
    Cout = root.shape[1]
    ea = x.unsqueeze(1) - x.unsqueeze(2)                                     # [B, i, j, Cin] = x_j - x_i
    We = F.linear(ea, nn_weight, nn_bias).view(B, N, N, Cin, Cout)
    msg = torch.einsum("bjc,bijco->bijo", x, We)
    cnt = adj.sum(2).clamp(min=1.0)
    agg = (msg * adj.unsqueeze(3)).sum(2) / cnt.unsqueeze(2)
    return agg + x @ root + bias


def moments(x, adj):
    """(P [B, N, Cin, Cin], m [B, N, Cin], 1 / n [B, N]) in the difference form."""
    cnt = adj.sum(2)
    inv = torch.where(cnt > 0, 1.0 / cnt.clamp(min=1.0), torch.zeros_like(cnt))
    ea = x.unsqueeze(1) - x.unsqueeze(2)                                     # [B, i, j, d]
    P = torch.einsum("bij,bjc,bijd->bicd", adj, x, ea) * inv[:, :, None, None]
    m = torch.einsum("bij,bjc->bic", adj, x) * inv[:, :, None]
    return P, m, inv


def factorised(x, adj, nn_weight, nn_bias, root, bias):
    Cin, Cout = root.shape
    P, m, _ = moments(x, adj)
    W3 = nn_weight.view(Cin, Cout, Cin)                                      # [c, o, d]
    y = torch.einsum("bicd,cod->bio", P, W3) + m @ nn_bias.view(Cin, Cout) + x @ root + bias
    return y, P, m


def backward(x, adj, nn_weight, nn_bias, root, bias, dy):
    """The closed form: dict of dx, nn_weight, nn_bias, root, bias for the cotangent dy [B, N, Cout]."""
    Cin, Cout = root.shape
    P, m, inv = moments(x, adj)
    W3 = nn_weight.view(Cin, Cout, Cin)
    G = torch.einsum("bio,cod->bicd", dy, W3)
    dm = dy @ nn_bias.view(Cin, Cout).t()
    ea = x.unsqueeze(1) - x.unsqueeze(2)
    dx = dy @ root.t() - torch.einsum("bicd,bic->bid", G, m)
    a = adj * inv.unsqueeze(2)                                               # [b, i, j] = 1 / n_i on listed edges
    s = torch.einsum("bicd,bijd->bijc", G, ea) + torch.einsum("bjd,bidc->bijc", x, G) + dm.unsqueeze(2)
    dx = dx + torch.einsum("bij,bijc->bjc", a, s)
    return {"x": dx, "nn_weight": torch.einsum("bicd,bio->cod", P, dy).reshape(Cin * Cout, Cin),
            "nn_bias": torch.einsum("bic,bio->co", m, dy).reshape(-1), "root": torch.einsum("bic,bio->co", x, dy),
            "bias": dy.sum((0, 1))}


def batch_norm(x, sd, prefix, training, eps=1e-5):
    if training:
        mean, var = x.mean(0), x.var(0, unbiased=False)
    else:
        mean, var = sd[prefix + "running_mean"], sd[prefix + "running_var"]
    return (x - mean) / torch.sqrt(var + eps) * sd[prefix + "weight"] + sd[prefix + "bias"]


def generator(sd, noise, N, k, alpha, tanh=False, training=False, probe=None):
    """``GraphCNNGANG.forward`` from a state dict (dtype of ``sd``): [B, N, node_feat_size].  ``probe``: a dict that receives the
    layers' inputs ("x") and the pre-activations of the LeakyReLUs ("z")."""
    B = noise.shape[0]
    z = F.linear(noise, sd["dense.weight"], sd["dense.bias"])
    zs = [z]
    x = F.leaky_relu(z, alpha)
    loop = k == N
    n_layers = sum(1 for key in sd if key.endswith(".root"))
    xs = []
    for i in range(n_layers):
        root = sd[f"layers.{i}.root"]
        x3 = x.reshape(B, N, root.shape[0])
        xs.append(x3)
        adj = knn_adjacency(x3.detach(), k, loop)
        y = literal(x3, adj, sd[f"layers.{i}.nn.weight"], sd[f"layers.{i}.nn.bias"], root, sd[f"layers.{i}.bias"])
        x = batch_norm(y.reshape(B * N, -1), sd, f"bn_layers.{i}.module.", training)
        if i < n_layers - 1:
            zs.append(x)
            x = F.leaky_relu(x, alpha)
    if probe is not None:
        probe["x"], probe["z"] = xs, zs
    if tanh:
        x = torch.tanh(x)
    return x.reshape(B, N, -1)


def rank_margin(xs, k, loop):
    """The smallest, over the layer inputs ``xs`` ([B, N, C] each) and all nodes, of (d_(k+1) - d_(k)) / d_max and
    (d_(1) - d_(0)) / d_max in a node's ascending distance list (d_(0) = 0 is the node itself; with ``loop`` the sets are ranks
    0 .. k-1 and the cut lies between d_(k-1) and d_(k)).  A cut beyond the list's end does not count."""
    worst = np.inf
    for x in xs:
        N = x.shape[1]
        d = torch.sort((x.unsqueeze(1) - x.unsqueeze(2)).pow(2).sum(-1).sqrt(), dim=2).values     # [B, N, N]
        dmax = d[:, :, -1:].clamp(min=1e-300)
        cut = k if loop else k + 1           # the first rank outside the set
        gaps = [(d[:, :, 1] - d[:, :, 0]) / dmax[:, :, 0]] if N > 1 else []
        if cut < N:
            gaps.append((d[:, :, cut] - d[:, :, cut - 1]) / dmax[:, :, 0])
        for g in gaps:
            worst = min(worst, float(g.min()))
    return worst
