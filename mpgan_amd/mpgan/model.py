"""MPGAN networks on the fused MI355X hot path -- drop-in for the reference's ``mpgan`` package.

Same class names, constructor keywords, ``forward`` signatures and state-dict key names as
rkansal47/MPGAN ``mpgan/model.py`` (LinearNet :11-88, MPLayer :91-384, MPNet :387-569,
MPGenerator :572-757, MPDiscriminator :760-894), so ``setup_training.setup_mpgan`` /
``train.py`` / ``gen.py`` and published checkpoints work unchanged.  The arithmetic runs in
libmpgan_amd.so (HIP, gfx950); there is no CPU fallback.

Fused (``ops.FusedMPLayerFn``: the reference's default and every published ``mp_*`` configuration): edge network
[96, 160, 192], two hidden node layers, fully connected or ``fully_connected=False`` with ``num_knn`` / ``self_loops``,
and up to ``ops.EDGE_SCALARS`` scalars per edge -- the distance column of ``pos_diffs``, ``clabels``, ``mask_fne_np`` --
plus coordinate differences (``delta_coords``, folded into the layer-1 projection); ``mask_c`` masking, ``dea`` pooling;
spectral norm (``ops.spectral_weights``: the wrapped layers' W_bar / sigma from one grouped launch, packed per call).
Every other constructor option of the reference (more edge scalars, conditioning columns on the k-NN graph, other layer
widths, batch norm) runs un-fused, layer by layer on the HIP GEMM (``MPLayer._forward_edges``); the few options
the reference itself cannot run (``int_diffs``, ``mask_learn*``, ``mask_feat_bin``) raise ``NotImplementedError`` at
construction.  ``MPLayer.fused`` says which route a layer takes.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor, nn

from .. import ops


def _unsupported(**flags):
    bad = [k for k, v in flags.items() if v]
    if bad:
        raise NotImplementedError(
            "mpgan_amd: option(s) %s are outside the fused MI355X path (see DESIGN.md, scope)" % ", ".join(bad))


class SpectralNorm(nn.Module):
    """Spectral normalisation of a Linear layer as the reference wraps it (mpgan/spectral_normalization.py:11-61): the
    wrapped module keeps ``weight_bar`` (trained), ``weight_u`` / ``weight_v`` (power-iteration vectors, no gradient) and
    ``bias`` -- same state-dict keys (``module.weight_bar`` ...).  ``weight()`` runs one power iteration and
    returns  W_bar / (u' W_bar v + 1e-12)  with the gradient flowing through W_bar only, which the caller feeds to the
    fused Linear launch.  On the GPU that is one ``mpg_spectral_norm`` launch (``ops.spectral_weights``); ``LinearNet`` and
    ``MPLayer`` put all their wrapped layers into one such launch (``job()``).  CPU tensors and the twice-differentiable route
    (``ops.double_backward_route``) keep the torch formula."""

    def __init__(self, module: nn.Linear, power_iterations: int = 1):
        super().__init__()
        self.module, self.power_iterations = module, power_iterations
        w = module.weight
        u = nn.Parameter(torch.nn.functional.normalize(torch.randn(w.shape[0]), dim=0, eps=1e-12), requires_grad=False)
        v = nn.Parameter(torch.nn.functional.normalize(torch.randn(w.shape[1]), dim=0, eps=1e-12), requires_grad=False)
        del module._parameters["weight"]
        module.register_parameter("weight_u", u)
        module.register_parameter("weight_v", v)
        module.register_parameter("weight_bar", nn.Parameter(w.data))

    @property
    def bias(self):
        return self.module.bias

    def job(self):
        """(weight_bar, weight_u, weight_v): this layer's entry of a grouped ``ops.spectral_weights`` call."""
        mod = self.module
        return mod.weight_bar, mod.weight_u, mod.weight_v

    def weight(self) -> Tensor:
        mod = self.module
        u, v, w = mod.weight_u, mod.weight_v, mod.weight_bar
        if w.is_cuda and not ops.double_backward_on(w.device):
            # one launch (mpg_spectral_norm) with the contract of the lines below: the iteration out of place, u / v stored in place
            # at their own addresses, the backward on the launch's own copies of the vectors (ops.SpectralWeightsFn)
            return ops.spectral_weights([self.job()], self.power_iterations)[0]
        # The power iteration runs OUT OF PLACE and sigma is built from the fresh vectors, so autograd never saves u / v
        # themselves (train_D runs D(real) and D(fake) before one backward: writing u in place must not touch what an
        # earlier forward saved).  The new vectors are then stored IN PLACE, at the parameters' fixed addresses: a captured
        # hipGraph replays this very copy, so the iteration keeps accumulating across replayed steps as it does across the
        # reference's eager ones (spectral_normalization.py:29-39) -- rebinding ``.data`` would run once, at capture time.
        with torch.no_grad():
            un, vn = u, v
            for _ in range(self.power_iterations):
                t = torch.mv(w.t(), un)
                vn = t / (t.norm() + 1e-12)
                t = torch.mv(w, vn)
                un = t / (t.norm() + 1e-12)
            if self.power_iterations > 0:
                u.copy_(un)
                v.copy_(vn)
            else:
                un, vn = u.clone(), v.clone()
        sigma = un.dot(w.mv(vn))
        return w / (sigma + 1e-12)


def _spectral_group(layers) -> list:
    """The weight of every layer of ``layers`` as its launch takes it -- ``weight`` of a plain Linear, W_bar / sigma of a
    ``SpectralNorm`` -- with ALL the wrapped layers' power iterations in one grouped launch (``ops.spectral_weights``; layers with
    different iteration counts, which no constructor here builds, get a launch per count)."""
    out = [None if isinstance(l, SpectralNorm) else l.weight for l in layers]
    for P in sorted({l.power_iterations for l in layers if isinstance(l, SpectralNorm)}):
        idx = [k for k, l in enumerate(layers) if isinstance(l, SpectralNorm) and l.power_iterations == P]
        for k, W in zip(idx, ops.spectral_weights([layers[k].job() for k in idx], P)):
            out[k] = W
    return out


class LinearNet(nn.Module):
    """Stack of ``Linear -> LeakyReLU -> [BatchNorm1d] -> Dropout`` (last layer ``Linear -> Dropout`` when
    ``final_linear``); parameters live in ``self.net`` so keys read ``net.{i}.weight|bias`` (``bn.{i}.*`` with batch
    norm, ``net.{i}.module.weight_bar|weight_u|weight_v|bias`` with spectral norm: mpgan/model.py:55-68)."""

    def __init__(self, layers: list, input_size: int = 0, output_size: int = 0, final_linear: bool = False,
                 leaky_relu_alpha: float = 0.2, dropout_p: float = 0, batch_norm: bool = False,
                 spectral_norm: bool = False):
        super().__init__()
        widths = ([input_size] if input_size else []) + list(layers) + ([output_size] if output_size else [])
        self.final_linear = final_linear
        self.leaky_relu_alpha = leaky_relu_alpha
        self.dropout_p = float(dropout_p)
        self.batch_norm, self.spectral_norm = bool(batch_norm), bool(spectral_norm)
        self.net = nn.ModuleList(nn.Linear(i, o) for i, o in zip(widths[:-1], widths[1:]))
        if self.batch_norm:   # (one per layer, the last one unused when final_linear: as the reference registers them)
            self.bn = nn.ModuleList(nn.BatchNorm1d(o) for o in widths[1:])
        if self.spectral_norm:
            for i in range(len(self.net)):
                if i != len(self.net) - 1 or not final_linear:
                    self.net[i] = SpectralNorm(self.net[i])

    @property
    def plain(self) -> bool:
        """Neither normalisation: the form the fused kernels (and the grouped weight-gradient launches) take."""
        return not (self.batch_norm or self.spectral_norm)

    def _bn(self, i: int, x: Tensor) -> Tensor:
        bn = self.bn[i]
        if not (self.training or not bn.track_running_stats):
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

    def gp_chain_ok(self, double_backward: bool, options: dict = None) -> bool:
        """``ops.gp_chain_route`` with this net's facts: would a call inside ``ops.double_backward_route`` run as ``ops.LinearNetFn``?
        Host only."""
        if not self.plain:
            return False
        widths = [self.net[0].in_features] + [l.out_features for l in self.net]
        return ops.gp_chain_route(widths, self.final_linear, self.batch_norm, self.spectral_norm, double_backward, options=options)

    def _forward_dd(self, x: Tensor, resid: Tensor = None, x2: Tensor = None) -> Tensor:
        """The twice-differentiable form (``ops.double_backward_route``): Linear as ``ops.MatMulFn`` + bias, LeakyReLU and
        dropout as ATen's own (their derivative formulas are differentiable; dropout draws from torch's generator, as
        the reference's does).  Batch norm has a first-order kernel only.  With ``ops.OPTIONS["gp_chain"]`` a net that
        ``ops.gp_chain_route`` covers runs as ``ops.LinearNetFn`` instead: one chained launch per pass, its dropout keyed by the
        device seed and ``ops.next_tag``, the input rows as the two parts (x | x2) when ``x2`` is given."""
        if self.batch_norm:
            raise NotImplementedError("LinearNet: batch norm has no double-backward route (the gradient penalty needs one)")
        if self.gp_chain_ok(True):
            shp = x.shape
            y = ops.linear_net_dd(x.reshape(-1, shp[-1]), None if x2 is None else x2.reshape(-1, x2.shape[-1]),
                                  [l.weight for l in self.net], [l.bias for l in self.net], final_linear=self.final_linear,
                                  alpha=self.leaky_relu_alpha, p_drop=self.dropout_p, training=self.training,
                                  resid=None if resid is None else resid.reshape(-1, resid.shape[-1]))
            return y.reshape(*shp[:-1], y.shape[-1])
        if x2 is not None:
            x = torch.cat((x, x2), dim=-1)
        last = len(self.net) - 1
        shp = x.shape
        x = x.reshape(-1, shp[-1])
        for k, lin in enumerate(self.net):
            W = lin.weight() if isinstance(lin, SpectralNorm) else lin.weight
            x = ops.MatMulFn.apply(x, W, "nt")
            if lin.bias is not None:
                x = x + lin.bias
            if not (self.final_linear and k == last):
                x = torch.nn.functional.leaky_relu(x, self.leaky_relu_alpha)
            x = torch.nn.functional.dropout(x, self.dropout_p, self.training)
        x = x.reshape(*shp[:-1], x.shape[-1])
        return x if resid is None else x + resid

    def forward(self, x: Tensor, resid: Tensor = None, x2: Tensor = None) -> Tensor:
        """``resid`` (not in the reference signature): added to the output, inside the last layer's launch when that
        layer has no activation -- MAB's ``x + ff(x)``.  ``x2`` (neither): more input columns, held apart -- the net runs on
        (x | x2); only the twice-differentiable op takes the two parts as they are, every other route concatenates."""
        if x.is_cuda and ops.double_backward_on(x.device):
            return self._forward_dd(x, resid, x2)
        if x2 is not None:
            x = torch.cat((x, x2), dim=-1)
        last = len(self.net) - 1
        eff = _spectral_group(self.net) if (self.spectral_norm and x.is_cuda and ops.OPTIONS["sn_fused"]) else None
        for k, lin in enumerate(self.net):
            act = not (self.final_linear and k == last)
            fuse = resid if (k == last and not act) else None
            W = eff[k] if eff is not None else (lin.weight() if isinstance(lin, SpectralNorm) else lin.weight)
            if self.batch_norm and act:   # the norm sits between the activation and the dropout (:78-83)
                x = ops.FusedLinearFn.apply(x, W, lin.bias, True, self.leaky_relu_alpha, 0.0, self.training, None)
                x = self._bn(k, x.reshape(-1, x.shape[-1])).reshape(x.shape)
                x = ops.FusedDropoutFn.apply(x, self.dropout_p, self.training)
            else:
                x = ops.FusedLinearFn.apply(x, W, lin.bias, act, self.leaky_relu_alpha, self.dropout_p, self.training, fuse)
            if k == last and resid is not None and fuse is None:
                x = x + resid
        return x

    def __repr__(self):
        return f"{self.__class__.__name__}(net = {self.net})"


class MPLayer(nn.Module):
    """One message-passing iteration.  The reference's default configuration -- edge network [96, 160, 192] on
    [x_i ; x_j], two hidden node layers, fully connected or k-NN graph -- runs on ``ops.FusedMPLayerFn`` (fused edge
    kernels + chained node network).  Every other option of the reference's constructor (edge features ``pos_diffs`` /
    ``delta_r`` / ``delta_coords``, conditioning columns ``clabels`` / ``mask_fne_np``, other layer widths, batch norm) takes
    the un-fused route of ``_forward_edges`` -- spectral norm too when ``ops.OPTIONS["sn_fused"]`` is off; with it on (the
    default) the wrapped layers' normalised weights come from one grouped ``mpg_spectral_norm`` launch and feed the fused kernels --: the edge matrix is materialised as the reference builds it and the two
    networks run layer by layer on the HIP GEMM -- same results, none of the fused kernels' speed."""

    def __init__(self, input_node_size: int, fe_layers: list, fn_layers: list, output_node_size: int,
                 pos_diffs: bool = False, all_ef: bool = True, coords: str = "polarrel", delta_coords: bool = False,
                 delta_r: bool = True, int_diffs: bool = False, clabels: int = 0, mask_fne_np: bool = False,
                 fully_connected: bool = True, num_knn: int = 20, self_loops: bool = True, sum: bool = True,
                 **linear_args):
        super().__init__()
        # int_diffs reserves an input column of the edge network that the reference's forward never fills (:180, :284-317)
        _unsupported(int_diffs=int_diffs)
        self.input_node_size, self.output_node_size = input_node_size, output_node_size
        self.fe_layers, self.fn_layers = list(fe_layers), list(fn_layers)
        self.sum = sum
        self.pos_diffs, self.all_ef, self.coords = bool(pos_diffs), bool(all_ef), coords
        self.delta_coords, self.delta_r = bool(delta_coords), bool(delta_r)
        self.clabels, self.mask_fne_np = int(clabels), bool(mask_fne_np)
        # fully_connected=False: every receiver aggregates over its num_knn nearest senders only (reference _getA_knn);
        # the fused kernels walk all N senders with the neighbour sets as a per-edge 0/1 factor -- or, with
        # ops.OPTIONS["knn_sparse"], the sparse kernels work on the N * num_knn rows of the sets themselves (ops.knn_sparse_route)
        self.fully_connected, self.num_knn, self.self_loops = fully_connected, int(num_knn), bool(self_loops)
        num_ef = 0   # edge features appended to [x_i ; x_j] (:169-178)
        if self.pos_diffs:
            if self.delta_coords:
                num_ef += 3 if coords == "cartesian" else 2
            if self.delta_r or self.all_ef:
                num_ef += 1
        self.num_ef = num_ef
        extra = self.clabels + int(self.mask_fne_np)
        # What the fused kernels take besides [x_i ; x_j]: up to ops.EDGE_SCALARS scalars per edge, each times its own column
        # of fe.net.0.weight -- the distance column (delta_r / all_ef) and the conditioning columns, which the reference
        # tiles over ROWS and so are per-edge gathers (_edge_scalars) -- and coordinate differences, which are linear in
        # x_i, x_j and fold into the a | c projection (_folded_w1).  On the k-NN graph the one edge feature is the distance the
        # neighbours were ranked by (to the mask-scaled senders, mpgan/model.py:333-345, :372): the same scalar.  Not fused:
        # differences over ALL features with their own columns (all_ef + delta_coords: the reference sizes fe for 2-3 of
        # them and fails itself), more scalars than EDGE_SCALARS, other layer widths.
        nc = 3 if coords == "cartesian" else 2
        # the columns MPLayer.forward appends (:303-308): [diffs, dists] | [dists] | [diffs], diffs over nc coordinates or all features
        has_diffs = self.pos_diffs and self.delta_coords and (self.delta_r or not self.all_ef)
        self._dist_col = self.pos_diffs and (self.delta_r or self.all_ef)
        self._diff_cols = nc if (has_diffs and not self.all_ef) else 0
        self.n_es = int(self._dist_col) + extra
        consistent = num_ef == self._diff_cols + int(self._dist_col) and not (has_diffs and self.all_ef)
        # Spectral norm stays on the fused kernels: the five wrapped layers' W_bar / sigma are computed tensors, packed per call like a
        # folded W1 (forward).  Batch norm sits between a layer's activation and its dropout: not a form the fused kernels have.
        self.spectral_norm = bool(linear_args.get("spectral_norm"))
        # Every layer input of the node network's forward and input-gradient chains has to fit mpg_chain's fragment buffer
        # (ops.CHAIN_MAX_K): the first layer's [agg | x | conditioning] columns, both hidden widths, and the output width
        # (the first K of the backward chain).  A wider node network runs un-fused.
        chain_fits = max([self.fe_layers[-1] + input_node_size + extra, output_node_size] + self.fn_layers) <= ops.CHAIN_MAX_K
        self.fused = (list(self.fe_layers) == [ops.H1, ops.H2, ops.H3] and len(self.fn_layers) == 2 and chain_fits
                      and consistent and self.n_es <= ops.EDGE_SCALARS
                      and (self.fully_connected or (not self._diff_cols and extra == 0))
                      and not linear_args.get("batch_norm"))
        self.fe = LinearNet(self.fe_layers, input_size=2 * input_node_size + num_ef + extra, final_linear=False, **linear_args)
        self.fn = LinearNet(self.fn_layers, input_size=self.fe_layers[-1] + input_node_size + extra,
                            output_size=output_node_size, final_linear=True, **linear_args)

    def _forward_edges(self, x: Tensor, use_mask: bool, mask: Tensor, labels: Tensor, num_jet_particles: Tensor) -> Tensor:
        """The un-fused route: edge matrix built row by row as ``MPLayer.forward`` / ``_getA_*`` do (mpgan/model.py:
        206-381), edge and node networks through ``LinearNet`` (one fused Linear launch per layer)."""
        B, N, F = x.shape
        nc = 3 if self.coords == "cartesian" else 2
        if self.fully_connected:
            k = N
            xi, xj = x.unsqueeze(2).expand(B, N, N, F), x.unsqueeze(1).expand(B, N, N, F)   # edge (b, i, j) = [x_i ; x_j]
            cols = [xi, xj]
            if self.pos_diffs:
                diffs = (xj - xi) if self.all_ef else (xj[..., :nc] - xi[..., :nc])
                dists = torch.norm(diffs + 1e-12, dim=3, keepdim=True)
                if self.delta_r and self.delta_coords:
                    cols += [diffs, dists]
                elif self.delta_r or self.all_ef:
                    cols += [dists]
                elif self.delta_coords:
                    cols += [diffs]
            edge_mask = mask.unsqueeze(1) if use_mask else None   # the sender's mask
        else:
            k = self.num_knn
            if k + int(not self.self_loops) > N:
                raise ValueError(f"num_knn = {k} neighbours (self_loops = {self.self_loops}) out of {N} nodes")
            xs = (((1 - 1e4) * mask + 1e4) * x) if use_mask else x   # zero-masked senders are pushed out of reach
            dd = xs.unsqueeze(1) - x.unsqueeze(2)
            if self.pos_diffs and not self.all_ef:
                dd = dd[..., :nc]
            order = torch.sort(torch.norm(dd + 1e-12, dim=3), dim=2)
            first = int(not self.self_loops)
            idx = order.indices[:, :, first:first + k]

            def neighbours(t):
                return torch.gather(t.unsqueeze(1).expand(B, N, N, t.shape[-1]), 2,
                                    idx.unsqueeze(3).expand(B, N, k, t.shape[-1]))
            cols = [x.unsqueeze(2).expand(B, N, k, F), neighbours(x)]
            if self.pos_diffs:
                cols.append(order.values[:, :, first:first + k].unsqueeze(3))
            edge_mask = neighbours(mask) if use_mask else None
        A = torch.cat(cols, dim=3).reshape(B * N * k, -1)
        # conditioning columns: ``t.repeat(rows / B, 1)`` tiles the [B, C] block, so ROW r gets the entry of jet r mod B
        # (:249, :253, :272, :276) -- reproduced as the reference computes it
        if self.clabels:
            A = torch.cat((A, labels[:, :self.clabels].repeat(N * k, 1)), dim=1)
        if self.mask_fne_np:
            A = torch.cat((A, num_jet_particles.repeat(N * k, 1)), dim=1)
        E = self.fe(A.contiguous()).reshape(B, N, k, self.fe_layers[-1])
        if edge_mask is not None:
            E = E * edge_mask
        agg = E.sum(dim=2) if self.sum else E.mean(dim=2)
        if not (self.clabels or self.mask_fne_np) and x.is_cuda and ops.double_backward_on(x.device) and self.fn.gp_chain_ok(True):
            return self._fn_parts(agg, x)
        h = torch.cat((agg, x), dim=2).reshape(B * N, -1)
        if self.clabels:
            h = torch.cat((h, labels[:, :self.clabels].repeat(N, 1)), dim=1)
        if self.mask_fne_np:
            h = torch.cat((h, num_jet_particles.repeat(N, 1)), dim=1)
        return self.fn(h.contiguous()).reshape(B, N, self.output_node_size)

    def forward(self, x: Tensor, use_mask: bool = False, mask: Tensor = None, labels: Tensor = None,
                num_jet_particles: Tensor = None, *, handoff: "ops.LayerHandoff" = None) -> Tensor:
        """``handoff`` (not in the reference signature): this call's link to the layers around it, from ``MPNet._run_layers``."""
        assert not (use_mask and mask is None), "need ``mask`` tensor if using ``use_mask`` option"
        assert not (self.clabels and labels is None), "need ``labels`` tensor if using ``clabels`` option"
        assert not (self.mask_fne_np and num_jet_particles is None), "need ``num_jet_particles`` tensor if using ``mask_fne_np`` option"
        if x.is_cuda and ops.double_backward_on(x.device) and self.gp_rows_ok(x.shape[0], x.shape[1], True):
            return self._forward_rows(x, use_mask, mask)
        if (not self.fused or (x.is_cuda and ops.double_backward_on(x.device))
                or (self.spectral_norm and not ops.OPTIONS["sn_fused"])):
            return self._forward_edges(x, use_mask, mask, labels, num_jet_particles)
        fe, fn = self.fe.net, self.fn.net
        nbr = None
        if not self.fully_connected:
            if self.num_knn + int(not self.self_loops) > x.shape[1]:
                raise ValueError(f"num_knn = {self.num_knn} neighbours (self_loops = {self.self_loops}) out of {x.shape[1]} nodes")
            with torch.no_grad():   # (with pos_diffs and not all_ef the reference ranks by the coordinates alone, :340-345)
                xr = x[..., :(3 if self.coords == "cartesian" else 2)] if (self.pos_diffs and not self.all_ef) else x
                nbr = ops.knn_sets(xr, mask if use_mask else None, self.num_knn, self.self_loops)
        es, xfn = self._edge_scalars(x, labels, num_jet_particles, mask if (use_mask and not self.fully_connected) else None)
        # the six weights as the launches take them: with spectral norm, fe.net.0..2 and fn.net.0..1 are W_bar / sigma out of ONE
        # grouped launch (a wrapped layer's ``.weight`` is a method, not a tensor); fn.net.2, the final linear layer, is not wrapped
        W1, W2, W3, V1, V2, V3 = _spectral_group([*fe, *fn])
        packed = None
        if self._diff_cols:
            W1 = self._folded_w1(W1)   # (not a parameter: its images are packed for this call)
        elif not self.spectral_norm:   # (nor are W_bar / sigma: they change with every forward)
            packed = self._packed()
        # consecutive fused layers of a network hand each other the layer-1 node terms a | c (ops.LayerHandoff): the launch
        # that produces a layer's output rows also projects them for the layer above
        # (a layer on the sparse k-NN route -- ops.knn_sparse_route -- takes and offers no hand-off; spectral-norm layers stay dense)
        if ops.knn_sparse_route(nbr is not None, self.n_es, x.shape[1], self.num_knn, spectral_norm=self.spectral_norm):
            handoff = None
        if handoff is not None:
            nxt = handoff.above
            if packed is None:   # (images packed for this call: nothing from below fits them; the layer above may still take its chain)
                handoff.below = None
            elif (nxt is not None and nxt.fused and not nxt._diff_cols and not nxt.spectral_norm and nxt.training == self.training
                  and nxt.n_es == 0):
                handoff.next = (nxt._packed(), nxt.fe.net[0].bias)
        return ops.FusedMPLayerFn.apply(
            x, mask if use_mask else None,
            W1, fe[0].bias, W2, fe[1].bias, W3, fe[2].bias,
            V1, fn[0].bias, V2, fn[1].bias, V3, fn[2].bias, es, xfn,
            ops.MPLayerSettings(self.sum, self.fe.leaky_relu_alpha, self.fe.dropout_p, self.training, packed, nbr, self.num_knn,
                                self.n_es, handoff, not torch.is_grad_enabled(), not self.spectral_norm))

    def gp_rows_ok(self, B: int, N: int, double_backward: bool, options: dict = None) -> bool:
        """``ops.gp_rows_route`` with this layer's facts: would a call on B jets of N particles inside ``ops.double_backward_route``
        take the twice-differentiable row kernels (``_forward_rows``)?  Host only."""
        return ops.gp_rows_route(B, N, N if self.fully_connected else self.num_knn, fused=self.fused, n_es=self.n_es,
                                 diff_cols=self._diff_cols, spectral_norm=self.spectral_norm,
                                 batch_norm=self.fe.batch_norm or self.fn.batch_norm, double_backward=double_backward, options=options)

    def _forward_rows(self, x: Tensor, use_mask: bool, mask: Tensor) -> Tensor:
        """The twice-differentiable route on the row kernels (``ops.EdgeRowsFn``): the edge aggregation as one op over explicit edge
        rows -- a fully connected layer is k = N with every sender listed, a k-NN layer takes its ``ops.knn_sets`` words, constants as
        on the other routes --, the node network in its ``_forward_dd`` form.  The edge dropout's tags come from ``ops.next_tag``
        and its seed is the device seed, like every fused call's.  The penalty differentiates with respect to the input alone
        (train.py:304-311), so that first derivative (``create_graph=True``) leaves the parameter gradients out; the penalty's
        backward has them, of both orders."""
        B, N, _ = x.shape
        fe, nbr = self.fe.net, None
        if not self.fully_connected:
            if self.num_knn + int(not self.self_loops) > N:
                raise ValueError(f"num_knn = {self.num_knn} neighbours (self_loops = {self.self_loops}) out of {N} nodes")
            with torch.no_grad():
                nbr = ops.knn_sets(x, mask if use_mask else None, self.num_knn, self.self_loops)
        agg = ops.EdgeRowsFn.apply(x, mask if use_mask else None, fe[0].weight, fe[0].bias, fe[1].weight, fe[1].bias, fe[2].weight,
                                   fe[2].bias, ops.EdgeRowsSettings(self.sum, self.fe.leaky_relu_alpha, self.fe.dropout_p, self.training,
                                                                    self._packed(), nbr, self.num_knn, None, False))
        if self.fn.gp_chain_ok(True):
            return self._fn_parts(agg, x)
        h = torch.cat((agg, x), dim=2).reshape(B * N, -1)
        return self.fn(h.contiguous()).reshape(B, N, self.output_node_size)

    def _fn_parts(self, agg: Tensor, x: Tensor) -> Tensor:
        """The node network on (agg | x) held apart (``ops.LinearNetFn``'s two-part input): no ``torch.cat`` and none of its derivatives."""
        B, N, _ = x.shape
        return self.fn(agg.reshape(B * N, -1), x2=x.reshape(B * N, -1)).reshape(B, N, self.output_node_size)

    def _folded_w1(self, W1: Tensor) -> Tensor:
        """fe.net.0.weight with the coordinate-difference columns folded into the node columns: the reference appends
        x_j[:nc] - x_i[:nc] to [x_i ; x_j] (mpgan/model.py:297-313), and W_d (x_j - x_i) is -W_d x_i + W_d x_j.  Built with
        torch operations, so the columns' gradients come out of autograd."""
        F, nc = self.input_node_size, self._diff_cols
        Wd = torch.nn.functional.pad(W1[:, 2 * F:2 * F + nc], (0, F - nc))
        return torch.cat((W1[:, :F] - Wd, W1[:, F:2 * F] + Wd, W1[:, 2 * F + nc:]), dim=1)

    def _edge_scalars(self, x: Tensor, labels: Tensor, num_jet_particles: Tensor, knn_mask: Tensor = None):
        """``(es [B, N senders, EDGE_SCALARS, N receivers] or None, xfn [B, N, F + E] or None)``: the scalars the fused edge
        kernels multiply with their own columns of fe.net.0.weight -- the distance ||x_j - x_i + 1e-12|| (mpgan/model.py:
        299-302; 4 bytes per edge instead of the edge matrix) and the conditioning columns AS THE REFERENCE TILES THEM:
        ``t.repeat(rows / B, 1)`` gives ROW r the entry of jet r mod B (:249, :253), a per-edge gather for the edge network
        and a per-node one for the node network (:272, :276).  (On the k-NN graph the reference's edge rows are (b, i, rank);
        the conditioning columns are then tiled over THOSE rows, which the fused kernels -- walking all senders -- do not
        have: clabels / mask_fne_np with fully_connected=False stay on the un-fused route.)"""
        if self.n_es == 0:
            return None, None
        B, N, F = x.shape
        cols = []
        if self._dist_col:
            xs = x if knn_mask is None else ((1 - 1e4) * knn_mask + 1e4) * x   # k-NN: zero-masked senders pushed away (:333-335)
            d = xs.unsqueeze(1) - x.unsqueeze(2)                # [B, i, j, F] = x_j - x_i
            if not self.all_ef:
                d = d[..., :(3 if self.coords == "cartesian" else 2)]
            cols.append(torch.norm(d + 1e-12, dim=3).transpose(1, 2))   # [B, j, i]
        xfn = None
        if self.clabels or self.mask_fne_np:
            erow = (torch.arange(B * N * N, device=x.device) % B).reshape(B, N, N).transpose(1, 2)   # [B, j, i]: jet of edge row (b, i, j)
            nrow = torch.arange(B * N, device=x.device) % B
            extra = []
            for t in ([labels[:, q] for q in range(self.clabels)] + ([num_jet_particles[:, 0]] if self.mask_fne_np else [])):
                cols.append(t.to(x.dtype)[erow])
                extra.append(t.to(x.dtype)[nrow].reshape(B, N, 1))
            xfn = torch.cat([x] + extra, dim=2)
        cols += [torch.zeros_like(cols[0])] * (ops.EDGE_SCALARS - len(cols))
        return torch.stack(cols, dim=2), xfn

    def _packed(self) -> "ops.PackedMPLayer":
        """Persistent weight images of this layer for the current mode (dropout scale) -- rebuilt when a
        parameter changes (``PackedMPLayer.ensure``) or on ``refresh_packed()``.  Not for a spectral-norm layer: its weights are
        new tensors on every forward, packed by that call."""
        assert not self.spectral_norm, "MPLayer._packed: a spectral-norm layer has no persistent weight images"
        dscale = ops.drop_params(self.fe.dropout_p)[1] if self.training else 1.0
        params = tuple(l.weight for l in (*self.fe.net, *self.fn.net))
        # keyed by the DEVICE of the weights as well: ``nn.DataParallel`` (the reference's multi-GPU mode,
        # setup_training.py:1418-1421) replicates a module by shallow-copying its __dict__, so all replicas see this one
        # dict, each from its own device's thread -- every replica gets (and replaces) only its own device's entry
        key = (dscale, ops.FWD_F16, params[0].device.index if params[0].is_cuda else -1)
        cache = self.__dict__.setdefault("_pack_cache", {})
        pk = cache.get(key)
        if pk is None or any(a is not b for a, b in zip(pk.params, params)):
            plist = tuple(q for l in (*self.fe.net, *self.fn.net) for q in (l.weight, l.bias))
            pk = cache[key] = ops.PackedMPLayer(params, self.input_node_size, self.output_node_size, key[0], key[1], plist=plist)
        return pk

    def packed_sets(self):
        """The weight-image sets built so far (``train.TrainStep`` rebuilds those of a whole network together)."""
        return list(self.__dict__.get("_pack_cache", {}).values())

    def refresh_packed(self):
        """Re-pack after an update torch cannot see (a kernel writing the parameters' storage directly)."""
        for pk in self.packed_sets():
            pk.refresh()

    def __repr__(self):
        return f"{self.__class__.__name__}(fe = {self.fe}, \n fn = {self.fn})"


class MPNet(nn.Module):
    """``mp_iters`` MPLayers with generator-/discriminator-specific hooks around them."""

    def __init__(self, num_particles: int, input_node_size: int, mp_iters: int = 2,
                 fe_layers: list = [96, 160, 192], fn_layers: list = [256, 256], fe1_layers: list = None,
                 fn1_layers: list = None, hidden_node_size: int = 32, output_node_size: int = 0,
                 final_activation: str = "", linear_args: dict = {}, mp_args: dict = {},
                 mp_args_first_layer: dict = {}, mask_args: dict = {}):
        super().__init__()
        self.num_particles = num_particles
        self.input_node_size = input_node_size
        self.hidden_node_size = hidden_node_size
        self.output_node_size = output_node_size if output_node_size > 0 else hidden_node_size
        self.mp_iters = mp_iters
        self.final_activation = final_activation
        self.linear_args = linear_args
        self.mask_args = mask_args
        first = {**mp_args, **mp_args_first_layer}
        self._init_mask(**mask_args)
        sizes = [input_node_size] + [hidden_node_size] * (mp_iters - 1) + [self.output_node_size]
        self.mp_layers = nn.ModuleList()
        for k in range(mp_iters):
            fe_k = (fe1_layers or fe_layers) if k == 0 else fe_layers
            fn_k = (fn1_layers or fn_layers) if k == 0 else fn_layers
            self.mp_layers.append(MPLayer(sizes[k], fe_k, fn_k, sizes[k + 1], **(first if k == 0 else mp_args),
                                          **linear_args))

    def _run_layers(self, x, use_mask, mask, labels, njp):
        """The loop over ``mp_layers`` (mpgan/model.py:511-512).  It owns the coupling of consecutive layers: each call gets its
        own ``ops.LayerHandoff``, which names the handoff of the layer below and the layer above (objects of this pass alone:
        ``nn.DataParallel`` replicas, each on its own thread, never share one)."""
        handoff = None
        for layer, above in zip(self.mp_layers, [*self.mp_layers[1:], None]):
            handoff = ops.LayerHandoff(handoff, above)
            x = layer(x, use_mask, mask, labels, njp, handoff=handoff)
        return x

    def forward(self, x: Tensor, labels: Tensor = None) -> Tensor:
        x = self._pre_mp(x, labels)
        x, use_mask, mask, njp = self._get_mask(x, labels, **self.mask_args)
        x = self._run_layers(x, use_mask, mask, labels, njp)
        x = self._post_mp(x, labels, use_mask, mask, njp)
        return self._finish(x, mask)

    def _finish(self, x, mask):
        """Final activation (reference ``_final_activation``, :533-538) and ``_final_mask``."""
        if self.final_activation == "tanh":
            x = torch.tanh(x)
        elif self.final_activation == "sigmoid":
            x = torch.sigmoid(x)
        return self._final_mask(x, mask, **self.mask_args)

    # hooks
    def _init_mask(self, **mask_args):
        pass

    def _pre_mp(self, x, labels):
        return x

    def _get_mask(self, x, labels, **mask_args):
        return x, False, None, None

    def _post_mp(self, x, labels, use_mask, mask, num_jet_particles):
        return x

    def _final_mask(self, x, mask, **mask_args):
        return x

    def __repr__(self):
        return f"MPLayers = {self.mp_layers})"


def _rank_mask(first_feature: Tensor, labels: Tensor, num_particles: int) -> Tensor:
    """mask_c: the n = int(label * N) lowest-noise particles are real (reference :689-699: rank by
    ``argsort().argsort()``).  The rank of particle i is the number of particles that sort before it -- counted
    directly (one comparison + one sum over an [B, N, N] boolean) instead of two device sorts; equal values are
    ordered by index."""
    n_minus_1 = (labels[:, -1] * num_particles).int() - 1
    xi, xj = first_feature.unsqueeze(2), first_feature.unsqueeze(1)
    idx = torch.arange(first_feature.shape[1], device=first_feature.device)
    before = (xj < xi) | ((xj == xi) & (idx.unsqueeze(0) < idx.unsqueeze(1)).unsqueeze(0))
    rank = before.sum(2)
    return (rank <= n_minus_1.unsqueeze(1)).unsqueeze(2).float()


class MPGenerator(MPNet):
    def __init__(self, lfc: bool = False, lfc_latent_size: int = 128, **mpnet_args):
        super().__init__(**mpnet_args)
        self.lfc = lfc
        if lfc:
            self.lfc_layer = nn.Linear(lfc_latent_size, self.num_particles * self.input_node_size)

    def _init_mask(self, mask_learn: bool = False, mask_learn_sep: bool = False, fmg: list = [64], **mask_args):
        _unsupported(mask_learn=mask_learn, mask_learn_sep=mask_learn_sep)

    def _pre_mp(self, x, labels):
        if self.lfc:
            x = ops.FusedLinearFn.apply(x, self.lfc_layer.weight, self.lfc_layer.bias, False, 0.2, 0.0, False)
            x = x.reshape(x.shape[0], self.num_particles, self.input_node_size)
        return x

    def _get_mask(self, x, labels=None, mask_learn=False, mask_learn_bin=True, mask_learn_sep=False, mask_c=True,
                  mask_fne_np=False, **mask_args):
        if not mask_c:
            return x, False, None, None
        if x.is_cuda:  # one launch (ops.rank_mask) instead of the comparison / sum / compare chain below
            return x, True, ops.rank_mask(x[:, :, 0], labels, self.num_particles).unsqueeze(2), None
        return x, True, _rank_mask(x[:, :, 0], labels, self.num_particles), None

    def _finish(self, x, mask):
        if x.is_cuda and self.final_activation in ops.ACT_CODES and not self.mask_args.get("mask_feat_bin", False):
            # tanh + the (mask - 0.5) column in one launch each way
            return ops.GenTailFn.apply(x, mask, ops.ACT_CODES[self.final_activation])
        return super()._finish(x, mask)

    def generate_into(self, x: Tensor, labels: Tensor, out: Tensor) -> Tensor:
        """``forward`` for callers that own the output rows (``out`` [B, N, F+1], e.g. the second half of a
        discriminator batch) and need no gradient: ``train.TrainStep``'s D step and bulk generation."""
        assert not torch.is_grad_enabled() and x.is_cuda
        x = self._pre_mp(x, labels)
        x, use_mask, mask, njp = self._get_mask(x, labels, **self.mask_args)
        x = self._run_layers(x, use_mask, mask, labels, njp)
        return ops.gen_tail_into(x, mask, ops.ACT_CODES[self.final_activation], out)

    def noise_mask_ok(self) -> bool:
        """The mask is a function of the input noise alone (mask_c on the noise's own first feature: no latent layer in
        front): a caller may draw both in one launch (``ops.normal_noise_masked``) and hand the mask in as ``premask``."""
        return bool(self.mask_args.get("mask_c", True)) and not self.mask_args.get("mask_feat_bin", False) and not self.lfc

    def generate_parts(self, x: Tensor, labels: Tensor, feat_out: Tensor = None, mask_out: Tensor = None, ign_out: Tensor = None,
                       premask=None):
        """``forward`` without gluing the mask column on: (particle features [B, N, F] after the final activation, mask
        [B, N, 1], None).  A discriminator's ``features_parts`` takes them as they are -- no mask column to write, to split off
        again and to pad a gradient for (``train.TrainStep``; the modules' ``forward`` keeps the reference's [B, N, F+1]
        tensors).  ``feat_out`` / ``mask_out`` (without gradients): the caller's rows to write into."""
        assert x.is_cuda and self.mask_args.get("mask_c", True) and not self.mask_args.get("mask_feat_bin", False)
        x = self._pre_mp(x, labels)
        if premask is not None:       # (mask [B, N], 1 - mask) drawn with the noise
            mask2d = premask[0]
        else:
            mask2d = ops.rank_mask(x[:, :, 0], labels, self.num_particles, out=None if mask_out is None else mask_out.view(x.shape[0], -1))
        mask = mask2d.unsqueeze(2)
        x = self._run_layers(x, True, mask, labels, None)
        act = ops.ACT_CODES[self.final_activation]
        if feat_out is not None:
            assert not torch.is_grad_enabled()
            return ops.gen_tail_into(x, None, act, feat_out), mask, None
        return ops.GenTailFn.apply(x, None, act), mask, None

    def _final_mask(self, x, mask, mask_feat_bin: bool = False, **mask_args):
        _unsupported(mask_feat_bin=mask_feat_bin)
        return torch.cat((x, mask - 0.5), dim=2) if mask is not None else x

    def __repr__(self):
        lfc_str = f"LFC = {self.lfc_layer},\n" if self.lfc else ""
        return f"{self.__class__.__name__}({lfc_str}MPLayers = {self.mp_layers})"


class MPDiscriminator(MPNet):
    def __init__(self, dea: bool = True, dea_sum: bool = True, fnd: list = [], mask_fnd_np: bool = False,
                 **mpnet_args):
        super().__init__(output_node_size=1 if not dea else 0, **mpnet_args)
        self.dea, self.dea_sum, self.mask_fnd_np = dea, dea_sum, bool(mask_fnd_np)
        if dea:   # (mask_fnd_np: the fraction of real particles is one more input of the final network, :803)
            self.fnd_layer = LinearNet(fnd, input_size=self.hidden_node_size + int(self.mask_fnd_np), output_size=1,
                                       final_linear=True, **self.linear_args)

    def _get_mask(self, x, labels, mask_manual=False, mask_learn=False, mask_learn_sep=False, mask_c=True,
                  mask_fne_np=False, mask_fnd_np=False, **mask_args):
        use_mask = bool(mask_manual or mask_learn or mask_c or mask_learn_sep)
        mask = x[:, :, -1:] + 0.5 if (use_mask or mask_fnd_np) else None   # (:881-883)
        if use_mask:
            x = x[:, :, :-1]
        njp = torch.mean(mask, dim=1) if mask_fne_np else None           # fraction of real particles, [B, 1] (:888)
        if njp is not None and all(l.fused for l in self.mp_layers):
            # the fused layers take the mask as data (its factor on the senders has no gradient there; nothing upstream of a
            # mask column is ever trained: the generator's comes out of a ranking) -- consistently so: the particle count
            # derived from it carries none either, instead of the partial gradient its columns alone would give
            njp = njp.detach()
        return x, use_mask, mask, njp

    def fused_head(self):
        """(weight [1, F], bias, mean-pooling?, sigmoid?, dropout p) when pooling + ``fnd_layer`` + final activation are
        the single-launch head of ``ops.DiscHeadFn`` (``dea`` with an empty ``fnd`` list: the reference default), else None."""
        if (not self.dea or self.mask_fnd_np or len(self.fnd_layer.net) != 1 or not self.fnd_layer.plain
                or self.final_activation not in ("", "sigmoid")):
            return None
        lin = self.fnd_layer.net[0]
        return lin.weight, lin.bias, not self.dea_sum, self.final_activation == "sigmoid", self.fnd_layer.dropout_p

    def features(self, x: Tensor, labels: Tensor = None):
        """The message-passing part of ``forward``: (last layer's node features [B, N, F], mask [B, N, 1] or None)."""
        x = self._pre_mp(x, labels)
        x, use_mask, mask, njp = self._get_mask(x, labels, **self.mask_args)
        x = self._run_layers(x, use_mask, mask, labels, njp)
        return x, (mask if use_mask else None)

    def parts_ok(self) -> bool:
        """Whether ``features_parts`` is ``features`` (the mask is used as a mask only: the reference's default)."""
        a = self.mask_args
        return (bool(a.get("mask_c", True)) and not a.get("mask_fne_np", False) and not a.get("mask_fnd_np", False)
                and not self.mask_fnd_np and not any(l.clabels or l.mask_fne_np for l in self.mp_layers))

    def features_parts(self, x3: Tensor, mask: Tensor, labels: Tensor = None, ignore: Tensor = None):
        """``features`` for callers that hold the particle features [B, N, F] and the mask [B, N, 1] apart (``parts_ok``)."""
        x = self._pre_mp(x3, labels)
        x = self._run_layers(x, True, mask, labels, None)
        return x, mask

    def forward(self, x: Tensor, labels: Tensor = None) -> Tensor:
        dd = x.is_cuda and ops.double_backward_on(x.device)
        head = self.fused_head() if (x.is_cuda and (not dd or ops.gp_head_route(x.shape[1], True))) else None
        if head is None:
            return super().forward(x, labels)
        y, mask = self.features(x, labels)
        w, b, mean, sigmoid, p = head
        if dd:   # (the mask is real-valued here and takes a gradient: ops.DiscHeadDDFn)
            return ops.DiscHeadDDFn.apply(y, mask, w, b, ops.DiscHeadDDSettings(mean, sigmoid, p, self.training, None, False)).unsqueeze(1)
        return ops.DiscHeadFn.apply(y, mask, w, b, mean, sigmoid, p, self.training).unsqueeze(1)

    def _post_mp(self, x, labels, use_mask, mask, num_jet_particles):
        mean = not (self.dea and self.dea_sum)
        if use_mask:
            x = (x * mask).sum(1)
            if mean:
                x = x / (mask.sum(1) + 1e-12)
        else:
            x = x.mean(1) if mean else x.sum(1)
        if not self.dea:
            return x
        if self.mask_fnd_np:
            x = torch.cat((num_jet_particles, x), dim=1)   # (:826-827: the reference needs mask_fne_np on as well)
        return self.fnd_layer(x.contiguous())

    def __repr__(self):
        dea_str = f",\nFND = {self.fnd_layer}" if self.dea else ""
        return f"{self.__class__.__name__}(MPLayers = {self.mp_layers}{dea_str})"
