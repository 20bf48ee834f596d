"""rGANG, rGAND and PointNetMixD (rkansal47/MPGAN ``ext_models/ext_models.py:14-72``, ``:160-207``).

Both discriminators have one shape: a small per-particle network over the B * N rows, a max (and mean) over each jet's particles,
a small network over the B pooled rows.  Routes of a call:

  CUDA tensors      every Linear on ``ops.FusedLinearFn`` (mpg_gemm); the LAST point layer together with the pooling on
                    ``ops.point_pool`` (mpg_point_pool_fwd / _bwd: the widest activation of the net, [B N, 512] / [B N, 1024],
                    is never written) where ``ops.point_pool_route`` says yes, else ``FusedLinearFn`` followed by torch.max /
                    torch.mean (``ops.OPTIONS["point_pool"]`` off -- MPG_POINT_POOL=0 -- or a shape beyond the kernel's limits);
  ... inside ``ops.double_backward_route`` (the gradient penalty; the published baselines were trained with loss "w", gp 10)
                    every Linear as ``ops.MatMulFn`` + bias, LeakyReLU and the pooling ATen's own: twice differentiable;
  CPU tensors       of any float dtype: plain ``torch.nn.functional`` formulas (the modules can be checked without a GPU).

``TreeGCN`` / ``TreeGANG`` (ext_models.py:211-333), the TreeGAN generator.  Routes of a layer:

  CUDA tensors      ``ops.tree_gcn`` (mpg_tree_gcn_fwd / _bwd: ancestor sum, branch product, W_loop collapsed to one [out, in]
                    matrix, bias and activation in one launch; the [B nodes, in support] activation, the widest of the net, is
                    never formed) where ``ops.tree_gcn_route`` says yes, else the un-fused route: the reference's literal layer
                    with every Linear on ``FusedLinearFn``, torch.matmul for W_branch and ATen's LeakyReLU
                    (``ops.OPTIONS["tree_gcn"]`` off -- MPG_TREE_GCN=0 --, a shape beyond the kernel's limits, ``upsample`` off);
  ... inside ``ops.double_backward_route`` the literal layer with every Linear an ``ops.MatMulFn``: twice differentiable;
  CPU tensors       of any float dtype: the literal layer in plain torch.

``NNConv`` / ``GraphBatchNorm`` / ``GraphCNNGANG`` (ext_models.py:75-157), the GraphCNN-GAN generator, without PyG or
torch_cluster.  The k-nearest-neighbour graph is ``ops.knn_sets`` (bit words; Euclidean distance over all features of the layer's
input, self excluded unless ``loop``, ties in index order).  Routes of a convolution:

  CUDA tensors      ``ops.nnconv``: ``ops.NNConvFn`` (mpg_nnconv_fwd / _bwd, the factorised form: no weight matrix per edge) where
                    ``ops.nnconv_route`` says yes, else the literal layer (``ops.nnconv_literal``: gather, per-edge weights on
                    ``FusedLinearFn``, torch.bmm, mean; ``ops.OPTIONS["nnconv"]`` off -- MPG_NNCONV=0 -- or beyond the limits);
                    batch norm on ``ops.BatchNormFn`` / ``ops.batchnorm_eval``;
  ... inside ``ops.double_backward_route`` the literal layer with every Linear an ``ops.MatMulFn`` and ATen's batch norm;
  CPU tensors       of any float dtype: the literal layer and the graph in plain torch.

``args`` is any object with the reference's attribute names (``latent_dim``, ``rgang_fc``, ``rgand_sfc``, ``rgand_fc``,
``pointnetd_pointfc``, ``pointnetd_fc``, ``num_hits``, ``node_feat_size``, ``leaky_relu_alpha``, ``mask``).
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F
from torch import Tensor, nn

from .. import ops


def _w2(layer: nn.Module) -> Tensor:
    """The [out, in] weight of a Linear or of a Conv1d of kernel size 1 ([out, in, 1]: a view, no copy)."""
    w = layer.weight
    return w if w.dim() == 2 else w.squeeze(-1)


def _linear(x: Tensor, layer: nn.Module, act: bool, alpha: float) -> Tensor:
    """One Linear (-> LeakyReLU) on the rows of ``x`` by the route of the module docstring."""
    W, b = _w2(layer), layer.bias
    if not x.is_cuda:
        y = F.linear(x, W, b)
        return F.leaky_relu(y, alpha) if act else y
    if ops.double_backward_on(x.device):
        y = ops.MatMulFn.apply(x, W, "nt")
        if b is not None:
            y = y + b
        return F.leaky_relu(y, alpha) if act else y
    return ops.FusedLinearFn.apply(x, W, b, act, alpha, 0.0, False, None)


def _pool(y: Tensor, B: int, N: int, mode: int) -> Tensor:
    y = y.reshape(B, N, y.shape[-1])
    parts = ([torch.max(y, dim=1)[0]] if mode & 1 else []) + ([torch.mean(y, dim=1)] if mode & 2 else [])
    return parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)


def _layer_and_pool(x: Tensor, layer: nn.Module, B: int, N: int, alpha: float, mode: int) -> Tensor:
    """LeakyReLU(Linear(x)) on the [B N, K] rows and the pooling over each jet's N rows: ``ops.point_pool`` where its route covers
    the call, else the layer and the pooling one after the other."""
    W = _w2(layer)
    if x.is_cuda and ops.point_pool_route(N, W.shape[1], W.shape[0], ops.double_backward_on(x.device)):
        return ops.point_pool(x, W, layer.bias, B, N, act=True, alpha=alpha, mode=mode)
    return _pool(_linear(x, layer, True, alpha), B, N, mode)


def _stack(widths, alpha, conv=False, last_act=True) -> nn.Sequential:
    """Linear (Conv1d of kernel 1) -> LeakyReLU pairs as the reference's nn.Sequential numbers them: layer i at index 2 i."""
    mods = []
    for i, (a, b) in enumerate(zip(widths[:-1], widths[1:])):
        mods.append(nn.Conv1d(a, b, 1) if conv else nn.Linear(a, b))
        if last_act or i < len(widths) - 2:
            mods.append(nn.LeakyReLU(negative_slope=alpha))
    return nn.Sequential(*mods)


def _linears(seq: nn.Sequential) -> list:
    return [m for m in seq if isinstance(m, (nn.Linear, nn.Conv1d))]


class rGANG(nn.Module):
    """FC generator (ext_models.py:14-36): Linear -> LeakyReLU over ``[latent_dim] + rgang_fc``, Linear to
    ``num_hits * node_feat_size``, Tanh; returns ``[B, num_hits, node_feat_size]``.  Keys ``model.{0,2,4,..}.weight|bias``.

    Deliberate difference, results-neutral: ``args.rgang_fc`` is NOT modified.  The reference ``insert(0, latent_dim)``s into the
    caller's list (ext_models.py:19) and relies on the caller's ``deepcopy``; this class builds its own width list."""

    def __init__(self, args):
        super().__init__()
        self.args = args
        self.alpha = float(args.leaky_relu_alpha)
        widths = [args.latent_dim] + list(args.rgang_fc)
        body = _stack(widths, self.alpha)
        self.model = nn.Sequential(*body, nn.Linear(widths[-1], args.num_hits * args.node_feat_size), nn.Tanh())

    def forward(self, x: Tensor, labels: Tensor = None, epoch=None) -> Tensor:
        lins = _linears(self.model)
        for k, lin in enumerate(lins):
            x = _linear(x, lin, k < len(lins) - 1, self.alpha)
        return torch.tanh(x).reshape(-1, self.args.num_hits, self.args.node_feat_size)


class rGAND(nn.Module):
    """rGAN discriminator (ext_models.py:39-72): Conv1d(kernel 1) -> LeakyReLU over ``[node_feat_size] + rgand_sfc`` on every
    particle, max over a jet's ``num_hits`` particles, Linear -> LeakyReLU over ``rgand_fc``, Linear to 1, Sigmoid (always on, as in
    the reference); returns ``[B, 1]``.  Keys ``sfc.{2i}.weight`` ([out, in, 1]) ``|bias``, ``fc.{2i}.weight|bias``.

    Deliberate difference, results-neutral: ``args.rgand_sfc`` / ``args.rgand_fc`` are NOT modified (the reference inserts the input
    widths into them, ext_models.py:44, :53)."""

    def __init__(self, args):
        super().__init__()
        self.args = args
        self.alpha = float(args.leaky_relu_alpha)
        sfc = [args.node_feat_size] + list(args.rgand_sfc)
        fc = [sfc[-1]] + list(args.rgand_fc)
        self.sfc = _stack(sfc, self.alpha, conv=True)
        self.fc = nn.Sequential(*_stack(fc, self.alpha), nn.Linear(fc[-1], 1), nn.Sigmoid())

    def forward(self, x: Tensor, labels: Tensor = None, epoch=None) -> Tensor:
        N, Fs = self.args.num_hits, self.args.node_feat_size
        x = x.reshape(-1, Fs)
        B = x.shape[0] // N
        point = _linears(self.sfc)
        for lin in point[:-1]:
            x = _linear(x, lin, True, self.alpha)
        x = _layer_and_pool(x, point[-1], B, N, self.alpha, 1)
        fc = _linears(self.fc)
        for k, lin in enumerate(fc):
            x = _linear(x, lin, k < len(fc) - 1, self.alpha)
        return torch.sigmoid(x)


class PointNetMixD(nn.Module):
    """PointNet-Mix discriminator (ext_models.py:160-207): Linear -> LeakyReLU over ``[node_feat_size] + pointnetd_pointfc`` on
    every particle, cat(max, mean) over a jet's particles, Linear -> LeakyReLU over ``pointnetd_fc``, Linear to 1, Sigmoid (always
    on); returns ``[B, 1]``.  With ``args.mask`` the input is ``[B, num_hits, node_feat_size + 1]`` (last column: mask - 0.5) and
    masked particles enter as (0, 0, -0.5).  Keys ``pointfc.{2i}.weight|bias``, ``fc.{2i}.weight|bias``.

    Two deliberate differences, both results-neutral:
      * ``args.pointnetd_pointfc`` / ``args.pointnetd_fc`` are NOT modified (the reference inserts and appends widths,
        ext_models.py:165-168);
      * ``forward`` does NOT modify the caller's tensor.  The reference adds 0.5 to ``x[:, :, 2]`` in place and takes it off the
        masked copy only (ext_models.py:199-202), which leaves the caller's third column shifted by +0.5.  Under graph replay on
        ``TrainStep``'s static batch that would drift by 0.5 per step."""

    def __init__(self, args):
        super().__init__()
        self.args = args
        self.alpha = float(args.leaky_relu_alpha)
        point = [args.node_feat_size] + list(args.pointnetd_pointfc)
        fc = [2 * point[-1]] + list(args.pointnetd_fc) + [1]
        self.pointfc = _stack(point, self.alpha)
        self.fc = nn.Sequential(*_stack(fc, self.alpha, last_act=False), nn.Sigmoid())
        # (0, 0, 0.5): the shift of the third feature around the masking; not a state-dict entry
        self.register_buffer("_shift", torch.tensor([0.0, 0.0, 0.5]), persistent=False)

    def forward(self, x: Tensor, labels: Tensor = None, epoch=None) -> Tensor:
        N, Fs = self.args.num_hits, self.args.node_feat_size
        B = x.size(0)
        if self.args.mask:
            # ((x + 0.5 e_2) * mask)[..., :3] - 0.5 e_2 of :199-202, out of place
            keep = (x[:, :, 3:4] >= 0).to(x.dtype)
            shift = self._shift.to(x.dtype)
            x = (x[:, :, :3] + shift) * keep - shift
        x = x.reshape(B * N, Fs)
        point = _linears(self.pointfc)
        for lin in point[:-1]:
            x = _linear(x, lin, True, self.alpha)
        x = _layer_and_pool(x, point[-1], B, N, self.alpha, 3)
        fc = _linears(self.fc)
        for k, lin in enumerate(fc):
            x = _linear(x, lin, k < len(fc) - 1, self.alpha)
        return torch.sigmoid(x)


def _plain_linear(x: Tensor, W: Tensor) -> Tensor:
    """x W^T, no bias, by the route of the module docstring."""
    if not x.is_cuda:
        return F.linear(x, W)
    if ops.double_backward_on(x.device):
        return ops.MatMulFn.apply(x.reshape(-1, x.shape[-1]), W, "nt").reshape(*x.shape[:-1], W.shape[0])
    return ops.FusedLinearFn.apply(x, W, None, False, 0.2, 0.0, False, None)


class TreeGCN(nn.Module):
    """One tree graph-convolution layer (ext_models.py:211-282): level ``depth`` ([B, node, features[depth]]) to level
    ``depth + 1`` ([B, node * degrees[depth], features[depth + 1]]).  Keys ``W_root.{i}.weight`` (i <= depth), ``W_branch``
    ([node, in, degree * in]; with ``upsample``), ``W_loop.{0,1}.weight``, ``bias`` ([1, degree, out]; read only with
    ``activation``).  Initialisation as the reference: W_branch xavier-uniform with relu gain, bias uniform in +-1 / sqrt(out), the
    Linears torch's default.

    Deliberate difference, results-neutral: ``forward`` returns a NEW list (the caller's levels and the new one) and does not
    append to the caller's (the reference does, ext_models.py:280)."""

    def __init__(self, depth, features, degrees, support=10, node=1, upsample=False, activation=True):
        super().__init__()
        self.depth, self.node, self.degree = depth, node, degrees[depth]
        self.in_feature, self.out_feature = features[depth], features[depth + 1]
        self.upsample, self.activation = upsample, activation
        self.features, self.degrees = [int(f) for f in features], [int(g) for g in degrees]
        self.W_root = nn.ModuleList([nn.Linear(features[i], self.out_feature, bias=False) for i in range(depth + 1)])
        if upsample:
            self.W_branch = nn.Parameter(torch.empty(node, self.in_feature, self.degree * self.in_feature))
        self.W_loop = nn.Sequential(nn.Linear(self.in_feature, self.in_feature * support, bias=False),
                                    nn.Linear(self.in_feature * support, self.out_feature, bias=False))
        self.bias = nn.Parameter(torch.empty(1, self.degree, self.out_feature))
        self.leaky_relu = nn.LeakyReLU(negative_slope=0.2)
        self.init_param()

    def init_param(self):
        if self.upsample:
            nn.init.xavier_uniform_(self.W_branch.data, gain=nn.init.calculate_gain("relu"))
        stdv = 1.0 / math.sqrt(self.out_feature)
        self.bias.data.uniform_(-stdv, stdv)

    def _literal(self, tree) -> Tensor:
        """The reference's layer as written (ext_models.py:254-279)."""
        batch, out = tree[0].size(0), self.out_feature
        root = 0
        for i in range(self.depth + 1):
            repeat_num = self.node // tree[i].size(1)
            root = root + _plain_linear(tree[i], self.W_root[i].weight).repeat(1, 1, repeat_num).view(batch, -1, out)
        if self.upsample:
            branch = F.leaky_relu(tree[-1].unsqueeze(2) @ self.W_branch, 0.2).view(batch, self.node * self.degree, self.in_feature)
            branch = _plain_linear(_plain_linear(branch, self.W_loop[0].weight), self.W_loop[1].weight)
            branch = root.repeat(1, 1, self.degree).view(batch, -1, out) + branch
        else:
            branch = root + _plain_linear(_plain_linear(tree[-1], self.W_loop[0].weight), self.W_loop[1].weight)
        if self.activation:
            branch = F.leaky_relu(branch + self.bias.repeat(1, self.node, 1), 0.2)
        return branch

    def next_level(self, tree) -> Tensor:
        """Level ``depth + 1`` from the levels 0 .. depth, by the route of the module docstring."""
        x = tree[-1]
        if (x.is_cuda and self.upsample and len(tree) == self.depth + 1
                and ops.tree_gcn_route(self.features, self.degrees, self.depth, ops.double_backward_on(x.device))):
            return ops.tree_gcn(tree, [m.weight for m in self.W_root], self.W_branch, self.W_loop[0].weight, self.W_loop[1].weight,
                                self.bias if self.activation else None, act=self.activation, alpha=0.2)
        return self._literal(tree)

    def forward(self, tree):
        tree = list(tree)
        return tree + [self.next_level(tree)]


class TreeGANG(nn.Module):
    """TreeGAN generator (ext_models.py:286-333): ``len(degrees)`` TreeGCN layers with ``upsample``, the last without bias and
    activation; ``forward(tree)`` takes the one-element list ``[noise [B, 1, features[0]]]`` and returns
    ``[B, prod(degrees), features[-1]]``, kept in ``pointcloud`` as well.  Keys ``gcn.TreeGCN_{d}.*``.

    Deliberate difference, results-neutral: ``forward`` does NOT append to the caller's list.  The reference grows the list it is
    given (ext_models.py:280), so a noise list passed twice would run on a tree of 1 + 2 * len(degrees) levels."""

    def __init__(self, features, degrees, support):
        super().__init__()
        self.layer_num = len(features) - 1
        assert self.layer_num == len(degrees), "Number of features should be one more than number of degrees."
        self.pointcloud = None
        vertex_num = 1
        self.gcn = nn.Sequential()
        for inx in range(self.layer_num):
            self.gcn.add_module("TreeGCN_" + str(inx), TreeGCN(inx, features, degrees, support=support, node=vertex_num, upsample=True,
                                                               activation=inx != self.layer_num - 1))
            vertex_num = int(vertex_num * degrees[inx])

    def forward(self, tree, labels=None):
        levels = list(tree)
        for layer in self.gcn:
            levels.append(layer.next_level(levels))
        self.pointcloud = levels[-1]
        return self.pointcloud

    def getPointcloud(self):
        return self.pointcloud[-1]


def knn_adjacency(x: Tensor, k: int, loop: bool) -> Tensor:
    """``torch_cluster.knn_graph`` per jet as a 0 / 1 adjacency [B, N, N] (receiver, sender) in plain torch: the senders of node i
    are the ``k`` nearest nodes of its jet in Euclidean distance over all features, self excluded unless ``loop``, equal distances
    in index order (a stable sort); with fewer than ``k`` candidates, all of them."""
    B, N, _ = x.shape
    d = (x.unsqueeze(1) - x.unsqueeze(2)).pow(2).sum(-1)              # [B, i, j]
    order = torch.sort(d, dim=2, stable=True).indices
    first = 0 if loop else 1
    adj = torch.zeros(B, N, N, dtype=x.dtype, device=x.device)
    return adj.scatter_(2, order[:, :, first:first + k], 1.0)


class NNConv(nn.Module):
    """PyG 1.x's ``NNConv`` in the one configuration the reference uses (ext_models.py:94-121): ``aggr="mean"``, ``root_weight``,
    ``bias``, the edge attribute x_j - x_i of a k-nearest-neighbour graph.  Keys ``root`` [in, out], ``bias`` [out] and ``nn.*``
    (the edge network, a Linear in -> in * out that keeps its own initialisation); ``root`` and ``bias`` are uniform in
    +-1 / sqrt(in) as PyG's ``reset_parameters`` leaves them.  ``forward(x [B, N, in], graph, k)`` takes the graph as the bit words
    of ``ops.knn_sets`` (CUDA) or as the adjacency of ``knn_adjacency`` (CPU) and returns the rows [B N, out]."""

    def __init__(self, in_channels, out_channels, nn, aggr="mean", root_weight=True, bias=True, **kwargs):
        super().__init__()
        if aggr != "mean":
            raise NotImplementedError(f"NNConv: aggr={aggr!r} is not built (the reference uses aggr='mean' only)")
        if not root_weight:
            raise NotImplementedError("NNConv: root_weight=False is not built (the reference uses root_weight=True only)")
        if not bias:
            raise NotImplementedError("NNConv: bias=False is not built (the reference uses bias=True only)")
        if kwargs:
            raise NotImplementedError(f"NNConv: {sorted(kwargs)} are not built")
        self.in_channels, self.out_channels, self.aggr = in_channels, out_channels, aggr
        self.nn = nn
        self.root = torch.nn.Parameter(torch.empty(in_channels, out_channels))
        self.bias = torch.nn.Parameter(torch.empty(out_channels))
        self.reset_parameters()

    def reset_parameters(self):
        bound = 1.0 / math.sqrt(self.in_channels)
        self.root.data.uniform_(-bound, bound)
        self.bias.data.uniform_(-bound, bound)

    def forward(self, x: Tensor, graph: Tensor, k: int) -> Tensor:
        B, N, _ = x.shape
        if x.is_cuda:
            return ops.nnconv(x, graph, self.nn.weight, self.nn.bias, self.root, self.bias, k=k)
        return ops.nnconv_literal(x, graph, self.nn.weight, self.nn.bias, self.root, self.bias, B, N, k)


class GraphBatchNorm(nn.Module):
    """``torch_geometric.nn.BatchNorm`` over the rows [B N, F]: a wrapper whose ``module`` is an ``nn.BatchNorm1d`` (keys
    ``module.weight|bias|running_mean|running_var|num_batches_tracked``).  CUDA: ``ops.BatchNormFn`` in training mode, with the
    running statistics kept as ``nn.BatchNorm1d`` keeps them, ``ops.batchnorm_eval`` in eval mode without a gradient; ATen's
    batch norm inside ``ops.double_backward_route``, in eval mode with a gradient, and on the CPU."""

    def __init__(self, in_channels, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True):
        super().__init__()
        self.module = nn.BatchNorm1d(in_channels, eps, momentum, affine, track_running_stats)

    def forward(self, x: Tensor) -> Tensor:
        bn = self.module
        batch_stats = self.training or not bn.track_running_stats
        if not x.is_cuda or ops.double_backward_on(x.device) or not bn.affine or (
                not batch_stats and torch.is_grad_enabled() and x.requires_grad):
            return bn(x)
        if not batch_stats:
            return ops.batchnorm_eval(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)
        y, mean, var = ops.BatchNormFn.apply(x, bn.weight, bn.bias, bn.eps)
        if bn.track_running_stats:   # running statistics as nn.BatchNorm1d keeps them (unbiased variance, momentum 0.1)
            with torch.no_grad():
                M = x.shape[0]
                bn.num_batches_tracked += 1
                mom = bn.momentum if bn.momentum is not None else 1.0 / float(bn.num_batches_tracked)
                bn.running_mean.mul_(1 - mom).add_(mean, alpha=mom)
                bn.running_var.mul_(1 - mom).add_(var, alpha=mom * M / max(M - 1, 1))
        return y


class GraphCNNGANG(nn.Module):
    """GraphCNN-GAN generator (ext_models.py:75-157): Linear ``latent_dim -> num_hits * graphcnng_layers[0]`` and LeakyReLU, then
    per layer a k-nearest-neighbour graph (``num_knn``) of the CURRENT features, ``NNConv``, batch norm and (but for the last, which
    ends in ``node_feat_size`` columns) LeakyReLU; Tanh with ``graphcnng_tanh``.  Returns ``[B, num_hits, node_feat_size]``.  Keys
    ``dense.*``, ``layers.{i}.{root,bias,nn.weight,nn.bias}``, ``edge_weights.{i}.{weight,bias}``, ``bn_layers.{i}.module.*``;
    ``edge_weights[i]`` IS ``layers[i].nn`` (one module under two names, as in the reference: ``parameters()`` yields it once).
    ``loop = (num_knn == num_hits)`` as in the reference."""

    def __init__(self, args):
        super().__init__()
        self.args = args
        self.alpha = float(args.leaky_relu_alpha)
        widths = list(args.graphcnng_layers) + [args.node_feat_size]
        self.dense = nn.Linear(args.latent_dim, args.num_hits * widths[0])
        self.layers, self.edge_weights, self.bn_layers = nn.ModuleList(), nn.ModuleList(), nn.ModuleList()
        for a, b in zip(widths[:-1], widths[1:]):
            self.edge_weights.append(nn.Linear(a, a * b))
            self.layers.append(NNConv(a, b, self.edge_weights[-1], aggr="mean", root_weight=True, bias=True))
            self.bn_layers.append(GraphBatchNorm(b))

    def forward(self, x: Tensor, labels: Tensor = None, epoch=None) -> Tensor:
        N, k = self.args.num_hits, self.args.num_knn
        loop = k == N
        x = _linear(x, self.dense, True, self.alpha)
        B = x.size(0)
        for i, (conv, bn) in enumerate(zip(self.layers, self.bn_layers)):
            x3 = x.reshape(B, N, conv.in_channels)
            with torch.no_grad():
                graph = ops.knn_sets(x3.detach(), None, k, self_loops=loop) if x.is_cuda else knn_adjacency(x3.detach(), k, loop)
            x = bn(conv(x3, graph, min(k, N if loop else N - 1)))
            if i < len(self.layers) - 1:
                x = F.leaky_relu(x, self.alpha)
        if self.args.graphcnng_tanh:
            x = torch.tanh(x)
        return x.reshape(B, N, self.args.node_feat_size)
