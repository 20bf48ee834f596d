"""PCGAN's networks (rkansal47/MPGAN ``ext_models/pcgan_model.py``): the permutation-equivariant layers ``PermEqui1_max``,
``PermEqui2_max``, ``PermEqui2_mean`` (:4-42), the set encoders ``G_inv_Tanh`` / ``G_inv`` (:45-144), the decoder ``G`` (:219-248) and
the latent GAN's ``latent_G`` / ``latent_D`` (:322-357) -- the eight classes the reference's pipeline builds
(setup_training.py:1371-1400, :1429-1456).  Same class names, constructor arguments, ``forward`` signatures and state-dict keys; the
constructors do not ``print(self)``.  ``D``, ``skipD``, ``skipG`` and ``ALPHA`` are used by nothing in the reference and are not here.

PCGAN is a latent GAN: every real batch goes through the frozen, pre-trained encoder (train.py:837-839), ``latent_G`` / ``latent_D``
work on its [B, z1] rows, and the decoder turns a latent row plus per-particle noise into particles for evaluation.  The encoder is
the only part on B N rows.  Routes of an encoder call:

  CUDA tensors      ``phi`` and the max over particles on ``ops.set_encode_launch`` (mpg_set_encode_fwd: one launch, the [B N, d_dim]
                    activations stay in LDS) where ``ops.set_encode_route`` says yes -- the option on, sizes inside the kernel's
                    limits, nothing in the call needing a gradient (the launch is forward only); else layer by layer with every
                    Linear on ``ops.FusedLinearFn`` (mpg_gemm) and ATen's max, mean, tanh and softplus, which is differentiable;
  ... inside ``ops.double_backward_route`` every Linear as ``ops.MatMulFn`` + bias: twice differentiable;
  CPU tensors       of any float dtype: plain torch.

``ro``, ``latent_G``, ``latent_D`` and the decoder run on the same per-Linear routes (LeakyReLU in the GEMM's epilogue, Softplus and
Tanh ATen's)."""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import Tensor, nn

from .. import ops
from .ext_models import _linear


def _lin(x: Tensor, layer: nn.Linear, act: bool = False) -> Tensor:
    """``layer`` (-> LeakyReLU 0.2) on the last dimension of ``x`` by the route of the module docstring."""
    y = _linear(x.reshape(-1, x.shape[-1]), layer, act, 0.2)
    return y.reshape(*x.shape[:-1], y.shape[-1])


class PermEqui1_max(nn.Module):
    """Gamma(x - max_n x) on ``x`` [B, N, in_dim] (pcgan_model.py:4-12)."""
    set_encode_pool = 1

    def __init__(self, in_dim, out_dim):
        super().__init__()
        self.Gamma = nn.Linear(in_dim, out_dim)

    def forward(self, x):
        xm, _ = x.max(1, keepdim=True)
        return _lin(x - xm, self.Gamma)


class PermEqui2_max(nn.Module):
    """Gamma(x) - Lambda(max_n x) on ``x`` [B, N, in_dim] (pcgan_model.py:15-27)."""
    set_encode_pool = 2

    def __init__(self, in_dim, out_dim):
        super().__init__()
        self.Gamma = nn.Linear(in_dim, out_dim)
        self.Lambda = nn.Linear(in_dim, out_dim, bias=False)

    def forward(self, x):
        xm, _ = x.max(1, keepdim=True)
        return _lin(x, self.Gamma) - _lin(xm, self.Lambda)


class PermEqui2_mean(nn.Module):
    """Gamma(x) - Lambda(mean_n x) on ``x`` [B, N, in_dim] (pcgan_model.py:30-42)."""
    set_encode_pool = 3

    def __init__(self, in_dim, out_dim):
        super().__init__()
        self.Gamma = nn.Linear(in_dim, out_dim)
        self.Lambda = nn.Linear(in_dim, out_dim, bias=False)

    def forward(self, x):
        xm = x.mean(1, keepdim=True)
        return _lin(x, self.Gamma) - _lin(xm, self.Lambda)


_EQUI = {"max": PermEqui2_max, "max1": PermEqui1_max, "mean": PermEqui2_mean}


class _SetEncoder(nn.Module):
    """What ``G_inv_Tanh`` and ``G_inv`` share: ``phi`` = three equivariant layers, each behind the activation; a max over the
    particles; ``ro`` = Linear, activation, Linear.  Keys ``phi.{0,2,4}.Gamma.weight|bias`` (``.Lambda.weight`` with pools "max" and
    "mean"), ``ro.{0,2}.weight|bias``."""
    act_name = "tanh"

    def __init__(self, x_dim, d_dim, z1_dim, pool="mean"):
        super().__init__()
        if pool not in _EQUI:
            raise ValueError(f"{type(self).__name__}: pool must be one of {sorted(_EQUI)}, got {pool!r}")
        self.d_dim, self.x_dim, self.z1_dim, self.pool = d_dim, x_dim, z1_dim, pool
        act = nn.Tanh if self.act_name == "tanh" else nn.Softplus
        equi = _EQUI[pool]
        self.phi = nn.Sequential(equi(x_dim, d_dim), act(), equi(d_dim, d_dim), act(), equi(d_dim, d_dim), act())
        self.ro = nn.Sequential(nn.Linear(d_dim, d_dim), act(), nn.Linear(d_dim, z1_dim))
        self.faster_parameters = [p for p in self.parameters()]

    def pooled(self, x: Tensor) -> Tensor:
        """max_n phi(x) [B, d_dim] by the route of the module docstring."""
        layers = [m for m in self.phi if isinstance(m, tuple(_EQUI.values()))]
        if x.is_cuda and x.dim() == 3 and x.dtype == torch.float32:
            params = [p for m in layers for p in m.parameters()]
            needs_grad = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params))
            widths = [layers[0].Gamma.in_features] + [m.Gamma.out_features for m in layers]
            if ops.set_encode_route(x.shape[1], widths, layers[0].set_encode_pool, self.act_name, needs_grad,
                                    ops.double_backward_on(x.device)):
                return ops.set_encode_launch(x, [m.Gamma.weight for m in layers], [m.Gamma.bias for m in layers],
                                             [getattr(m, "Lambda", m.Gamma).weight for m in layers],
                                             pool=layers[0].set_encode_pool, act=self.act_name)
        return self.phi(x).max(1)[0]

    def forward(self, x):
        act = torch.tanh if self.act_name == "tanh" else F.softplus
        return _lin(act(_lin(self.pooled(x), self.ro[0])), self.ro[2])


class G_inv_Tanh(_SetEncoder):
    """The set encoder the latent GAN is trained on (pcgan_model.py:45-93): ``x`` [B, N, x_dim] to [B, z1_dim]."""
    act_name = "tanh"


class G_inv(_SetEncoder):
    """The set encoder with Softplus in place of Tanh (pcgan_model.py:96-144)."""
    act_name = "softplus"


class G(nn.Module):
    """The decoder (pcgan_model.py:219-248): ``main(fc(z1) + fu(z2))`` with ``z1`` [B, 1, z1_dim] and ``z2`` [B, N, z2_dim] gives
    [B, N, x_dim]; ``main`` = Softplus -> Linear five times over the width max(250, 2 z1_dim).  Keys ``fc.weight|bias``,
    ``fu.weight``, ``main.{1,3,5,7,9}.weight|bias``."""

    def __init__(self, x_dim, z1_dim, z2_dim):
        super().__init__()
        self.z1_dim, self.z2_dim, self.x_dim = z1_dim, z2_dim, x_dim
        hid_d = max(250, 2 * z1_dim)
        self.fc = nn.Linear(z1_dim, hid_d)
        self.fu = nn.Linear(z2_dim, hid_d, bias=False)
        mods = []
        for out in (hid_d, hid_d, hid_d, hid_d, x_dim):
            mods += [nn.Softplus(), nn.Linear(hid_d, out)]
        self.main = nn.Sequential(*mods)
        self.faster_parameters = [p for p in self.parameters()]

    def forward(self, z1, z2):
        x = _lin(z1, self.fc) + _lin(z2, self.fu)
        for m in self.main:
            x = _lin(x, m) if isinstance(m, nn.Linear) else F.softplus(x)
        return x


def _leaky_mlp(widths) -> nn.Sequential:
    """Linear -> LeakyReLU(0.2) over ``widths``, the last Linear bare: layer i at index 2 i."""
    mods = []
    for i, (a, b) in enumerate(zip(widths[:-1], widths[1:])):
        mods += ([nn.LeakyReLU(negative_slope=0.2)] if i else []) + [nn.Linear(a, b)]
    return nn.Sequential(*mods)


def _run_leaky_mlp(model: nn.Sequential, x: Tensor) -> Tensor:
    lins = [m for m in model if isinstance(m, nn.Linear)]
    for k, lin in enumerate(lins):
        x = _lin(x, lin, act=k < len(lins) - 1)
    return x


class latent_G(nn.Module):
    """The latent generator (pcgan_model.py:322-338): noise [B, latent_dim] to a latent row [B, z1_dim].  Keys
    ``model.{0,2,..}.weight|bias``."""

    def __init__(self, latent_dim, z1_dim, layers=[256, 512]):
        super().__init__()
        self.model = _leaky_mlp([latent_dim] + list(layers) + [z1_dim])

    def forward(self, x, labels=None):
        return _run_leaky_mlp(self.model, x)


class latent_D(nn.Module):
    """The latent critic (pcgan_model.py:341-357): a latent row [B, z1_dim] to [B, 1], no final activation (Wasserstein loss)."""

    def __init__(self, z1_dim, layers=[512, 256]):
        super().__init__()
        self.model = _leaky_mlp([z1_dim] + list(layers) + [1])

    def forward(self, x, labels=None, epoch=None):
        return _run_leaky_mlp(self.model, x)


def load_pcgan_encoder(state_dict_or_path, x_dim, d_dim, z1_dim, pool) -> G_inv_Tanh:
    """The frozen, pre-trained encoder as the reference uses it (setup_training.py:1429-1437, train.py:837-839): a ``G_inv_Tanh``
    with the given state dict (or the file that holds one) loaded ``strict=True``, in ``eval()`` with nothing requiring grad -- so a
    plain ``G_inv(data)`` on the GPU takes the one-launch route."""
    sd = state_dict_or_path
    if not isinstance(sd, dict):
        sd = torch.load(sd, map_location="cpu")
    net = G_inv_Tanh(x_dim, d_dim, z1_dim, pool=pool)
    net.load_state_dict(sd, strict=True)
    net.faster_parameters = [p for p in net.parameters()]
    return net.eval().requires_grad_(False)
