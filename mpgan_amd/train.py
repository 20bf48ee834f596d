"""One G+D training iteration on the fused path, host side.

Mirrors the reference's ``train_D`` / ``train_G`` (train.py:398-523): losses ``ls`` (default, train.py:368-370,
:471-472), ``og``, ``w``, ``hinge`` (``calc_D_loss`` :331-395, ``calc_G_loss`` :465-476), optimizers RMSprop
(default), Adam, Adadelta as ``setup_training.optimizers`` builds them (setup_training.py:1511-1523),
generator noise ~ N(0, sd=0.2) sampled on the device every step
(train.py:100-141), D in train mode (dropout on) in both sub-steps, G in eval mode in the D step.
``--num-critic`` / ``--num-gen`` (setup_training.py:239-250) decide which of the two runs on a batch (train.py:841, :864;
``TrainStep(num_critic=..., num_gen=...)``): a ``step()`` is one batch of the reference's epoch loop and runs train_D and
train_G, train_D alone or train_G alone, each kind captured into graphs of its own.
The gradient penalty (train.py:286-324, ``--gp``) needs a second derivative through D.  The fused ops are first-order
only (``once_differentiable``), so the penalty's own pass D(interpolated) takes the double-backward route
(``ops.double_backward_route``: every product an ``ops.MatMulFn`` on the HIP GEMM, the rest ATen) while D(real) and
D(generated) stay on the fused kernels; both discriminators (``MPDiscriminator``, ``GAPT_D``) have that route.
Jet augmentation (``--aug-*``, train.py:438-442, :508-511; ``TrainStep(augment=...)``) is one affine map per jet drawn on the
device inside the iteration (``ops.augment``), from the seed that keys the noise and the dropout masks.
Label smoothing / label noise (``--label-smoothing`` / ``--label-noise``, train.py:341-363; ``TrainStep(label_smoothing=...,
label_noise=...)``) are per-jet targets drawn on the device by one launch in front of D's head (``ops.label_targets``).
The augmentation probability can follow the discriminator (``Augment(adaptive_prob=True)``, the reference's unimplemented
``--adaptive-prob``): ADA's rule on D's outputs for the real jets, one launch behind D's head (``ops.ada_update``); under a
process group the ranks settle one probability from the sign count of all their jets, which rides in D's gradient all-reduce
(``ops.ada_count`` behind the head, ``ops.ada_settle`` behind the all-reduce).
The training data can live on the device as well (``TrainStep(loader=data.DeviceJetLoader(...))``): the batch is then gathered by
one launch at the top of the iteration, inside the capture, in the order of a keyed shuffle.
An averaged generator (``TrainStep(ema=Ema(...))``; Yazici et al. 2019, StyleGAN's ``G_ema``) is kept by G's optimizer launch
itself -- two more memory streams in its loop -- and handed out as a module by ``ema_generator()``.
Learning-rate schedules and gradient clipping (``TrainStep(lr_schedule=LrSchedule(...), grad_clip=GradClip(...))``) are settled on the
device by one launch in front of each optimizer launch (``mpg_step_control``), which then reads its rate and its gradient scale from
device memory: neither is a constant of the captured graphs.

Two pieces of work the reference does and throws away are not done (results-neutral, SURVEY.md
section 3.1): the D step does not back-propagate into G (its gradients are zeroed before use,
train.py:495), and the G step does not form D's weight gradients (zeroed at train.py:420).

MI355X specifics: parameters and gradients of each network live in ONE flat buffer (a single
fused RMSprop launch, a single RCCL all-reduce per network per step), and the whole iteration is
captured into hipGraphs (three segments, split at the two gradient all-reduces) and replayed.
"""
from __future__ import annotations

import copy
import ctypes as C
import os
from typing import Optional

import torch
from torch import nn

from . import _lib, ops, dist as mdist
from .mpgan import MPGenerator, MPDiscriminator
from .step_options import (ADA_DEFAULTS, AUG_SITES, AdaController, Augment, Augmenter, DeviceWords, Ema, EmaState, GradClip,  # noqa: F401
                           LabelDraw, LrSchedule, Schedule, SeedState, StepControl, ada_rule, effective_targets)

LR = {  # setup_training.py:848-872 (lr_disc, lr_gen) per jet type for model = mpgan
    "g": (3e-5, 1e-5), "t": (6e-5, 2e-5), "q": (1.5e-5, 0.5e-5),
}


def default_mpgan(num_particles: int = 30, disc_dropout: float = 0.5, gen_dropout: float = 0.0, device="cuda",
                  loss: str = "ls", spectral_norm_gen: bool = False, spectral_norm_disc: bool = False,
                  batch_norm_gen: bool = False, batch_norm_disc: bool = False):
    """MPGenerator / MPDiscriminator exactly as ``setup_training.setup_mpgan`` builds them from the
    reference's default arguments (setup_training.py:1195-1293, defaults :415-548); ``loss`` picks D's final
    activation as :1250 does (none for ``w`` / ``hinge``, sigmoid otherwise); the four normalisation switches are
    ``--spectral-norm-gen/-disc`` and ``--batch-norm-gen/-disc`` (:254-262 -> linear_args, :1207-1223)."""
    def lin(p, bn=False, sn=False):
        return {"leaky_relu_alpha": 0.2, "dropout_p": p, "batch_norm": bn, "spectral_norm": sn}
    mp_args = {"pos_diffs": False, "all_ef": False, "coords": "polarrel", "delta_coords": False, "delta_r": False,
               "int_diffs": False, "clabels": 0, "mask_fne_np": False, "fully_connected": True, "num_knn": 10,
               "self_loops": True, "sum": True}
    common = {"num_particles": num_particles, "hidden_node_size": 32, "fe_layers": [96, 160, 192],
              "fn_layers": [256, 256], "fn1_layers": None}
    mask_args = {"mask_feat": False, "mask_feat_bin": False, "mask_weights": False, "mask_manual": False,
                 "mask_exp": False, "mask_real_only": False, "mask_learn": False, "mask_learn_bin": True,
                 "mask_learn_sep": False, "fmg": [64], "mask_disc_sep": False, "mask_fnd_np": False,
                 "mask_c": True, "mask_fne_np": False}
    G = MPGenerator(mp_iters=2, fe1_layers=None, final_activation="tanh", output_node_size=3, input_node_size=32,
                    lfc=False, lfc_latent_size=128, **common, mp_args=dict(mp_args),
                    mp_args_first_layer={"clabels": 0}, linear_args=lin(gen_dropout, batch_norm_gen, spectral_norm_gen),
                    mask_args=dict(mask_args))
    D = MPDiscriminator(mp_iters=2, fe1_layers=None, final_activation="" if loss in ("w", "hinge") else "sigmoid",
                        input_node_size=3, dea=True,
                        dea_sum=True, fnd=[], mask_fnd_np=False, **common, mp_args=dict(mp_args),
                        mp_args_first_layer={"clabels": 0, "all_ef": False},
                        linear_args=lin(disc_dropout, batch_norm_disc, spectral_norm_disc), mask_args=dict(mask_args))
    return G.to(device), D.to(device)


def default_gapt(num_particles: int = 30, disc_dropout: float = 0.5, gen_dropout: float = 0.0, device="cuda",
                 use_isab: bool = False):
    """GAPT_G / GAPT_D as ``setup_training.setup_gapt`` builds them from the reference's defaults
    (setup_training.py:1296-1347; 4 / 2 SAB layers, 4 heads, embed 64: :552-581)."""
    from .gapt import GAPT_G, GAPT_D

    def lin(p):
        return {"leaky_relu_alpha": 0.2, "dropout_p": p, "batch_norm": False, "spectral_norm": False}
    common = {"num_particles": num_particles, "num_heads": 4, "embed_dim": 64, "sab_fc_layers": [],
              "use_mask": True, "use_isab": use_isab, "num_isab_nodes": 10}
    G = GAPT_G(sab_layers=4, output_feat_size=3, final_fc_layers=[], dropout_p=gen_dropout, layer_norm=False,
               **common, linear_args=lin(gen_dropout))
    D = GAPT_D(sab_layers=2, input_feat_size=3, final_fc_layers=[], dropout_p=disc_dropout, layer_norm=False,
               **common, linear_args=lin(disc_dropout))
    return G.to(device), D.to(device)


LR_GAPT = (1.5e-4, 0.5e-4)  # setup_training.py:856-857, :869-870


OPTIMIZERS = ("rmsprop", "adam", "adadelta")


class FlatParams:
    """All parameters of a module re-pointed into one flat fp32 buffer, with a flat gradient buffer
    whose views are pre-installed as ``p.grad`` (autograd accumulates into them in place) and the flat
    optimiser state.  state_dict() keys/shapes of the module are untouched.

    ``optimizer``: "rmsprop" (torch.optim.RMSprop defaults), "adam" (weight_decay 5e-4, betas as given) or
    "adadelta" -- the three choices of ``setup_training.optimizers`` (setup_training.py:1511-1523), each ONE fused
    launch over the flat buffer.  ``state_dict()`` / ``load_state_dict()`` speak the matching ``torch.optim``
    class's own format, so the reference's ``*_optim_<epoch>.pt`` files (train.py:534-535, reloaded at
    setup_training.py:1525-1535) are read and written as they are.

    ``ema`` (a ``step_options.Ema``; ``batch_size``: the jets one step consumes, which ``Ema(kimg=...)`` needs): the launch also
    folds the new parameters into their exponential moving average ``self.ema`` (``mpg_*_ema``); ``self.ema_state`` holds its
    step word and the launch's ticket.  ``tail``: that many floats more at the end of the gradient buffer (``self.tail``), which
    travel in its all-reduce and belong to no parameter.  ``control`` (a ``step_options.StepControl`` on the parameters' device):
    ``step`` issues ``mpg_step_control`` and then the ``mpg_*_ctl`` optimizer launch, which takes the learning rate and the gradient
    scale from the control's device words instead of its arguments."""

    def __init__(self, module: nn.Module, optimizer: str = "rmsprop", betas=(0.9, 0.999), weight_decay: float = 5e-4,
                 ema: Optional[Ema] = None, batch_size: Optional[int] = None, tail: int = 0,
                 control: Optional[StepControl] = None):
        if optimizer not in OPTIMIZERS:
            raise ValueError(f"optimizer must be one of {OPTIMIZERS}, got {optimizer!r}")
        # Only what is TRAINED goes into the flat buffers: frozen parameters (spectral norm's power-iteration vectors,
        # requires_grad = False) are never stepped by the reference's optimizers either -- filtered out by requires_grad
        # or left with grad None (setup_training.py:1500-1523) -- and Adam's weight decay would otherwise move them.
        all_ps = list(module.parameters())
        self._trained_idx = [i for i, p in enumerate(all_ps) if p.requires_grad]   # positions in module.parameters()
        self._n_all = len(all_ps)
        ps = [all_ps[i] for i in self._trained_idx]
        if not ps:
            raise ValueError("FlatParams: the module has no trainable parameter")
        self.params = ps
        self.module = module
        self.optimizer, self.betas, self.weight_decay = optimizer, tuple(betas), float(weight_decay)
        n = sum(p.numel() for p in ps)
        dev = ps[0].device
        self.flat = torch.empty(n, device=dev, dtype=torch.float32)
        # ``tail`` floats behind the n gradients ride in the same buffer -- and so in the network's one gradient all-reduce
        # (``grad_all``: what TrainStep reduces) -- without being gradients: the p.grad views and every optimizer launch cover the
        # first n only (the adaptive augmentation's sign count: step_options.AdaController)
        self.grad_all = torch.zeros(n + int(tail), device=dev, dtype=torch.float32)
        self.grad = self.grad_all[:n] if tail else self.grad_all
        self.tail = self.grad_all[n:] if tail else None
        self.sq = torch.zeros(n, device=dev, dtype=torch.float32)       # square_avg / exp_avg_sq
        self.aux = torch.zeros(n, device=dev, dtype=torch.float32) if optimizer != "rmsprop" else None  # exp_avg / acc_delta
        # optimiser steps taken.  Adam needs the count in its arithmetic, so it lives in device memory (a replayed
        # hipGraph must see it advance); the others only report it in state_dict(): host counter.
        self.step_count = torch.zeros((), device=dev, dtype=torch.float32)
        self._host_steps = 0
        self._spans = []
        off = 0
        for p in ps:
            k = p.numel()
            self.flat[off:off + k].copy_(p.data.reshape(-1))
            p.data = self.flat[off:off + k].view_as(p)
            p.grad = self.grad[off:off + k].view_as(p)
            self._spans.append((off, k, tuple(p.shape)))
            off += k
        self.n = n
        self.lr = None  # last learning rate used (for state_dict's param_groups)
        self.carried = []   # the carried entries (step_options.py) that travel with this optimizer's state dict; TrainStep fills it
        # the averaged parameters: a copy of ``flat`` to start from, the words (t, ticket) and the block the launch takes
        self.ema = self.ema_state = self._ema_block = self.ema_carried = None
        if ema is not None:
            beta = ema.beta_for(batch_size)
            self.ema = self.flat.clone()
            self.ema_state = torch.zeros(2, device=dev, dtype=torch.uint32)
            self._ema_block = _lib.MpgEma(C.c_void_p(self.ema.data_ptr()), C.c_void_p(self.ema_state.data_ptr()), beta, ema.start,
                                          int(ema.warmup))
            self.ema_carried = EmaState(self.flat, self.ema, self.ema_state, beta, ema.start, ema.warmup)
        if control is not None:
            if not isinstance(control, StepControl):
                raise TypeError(f"control must be a step_options.StepControl, got {type(control).__name__}")
            if control.state.device != dev:
                raise ValueError(f"control lives on {control.state.device}, the parameters on {dev}")
        self.control = control

    def zero_grad(self):
        self.grad.zero_()

    # -- the fused step -----------------------------------------------------------------------------
    def step(self, lr: float, gscale: float = 1.0, zero_grad: bool = False, advance_seed: torch.Tensor = None):
        """One optimiser step over the flat buffer; ``gscale`` multiplies the gradient first; ``zero_grad``: the gradient
        buffer is cleared by the same launch, behind its last use; ``advance_seed``: the device's dropout / noise seed
        (``ops.seed_tensor``) is moved on by ``ops.SEED_STEP`` in the same launch -- ``ops.bump_seed`` of the next iteration
        without a kernel of its own.  With a ``control`` the launch in front settles the learning rate and the gradient scale on
        the device (schedule and clipping; ``gscale`` goes into it) and ``lr`` is not looked at: ``control.set_base`` moves it."""
        if self.control is not None:
            return self._controlled_step(gscale, zero_grad, advance_seed)
        self.lr = lr
        vp = lambda t: C.c_void_p(t.data_ptr())
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        L = _lib.lib()
        z = int(zero_grad)
        cnt, add = (None, 0) if advance_seed is None else (vp(advance_seed), ops.SEED_STEP)
        # (the averaged entry point takes the same arguments with the MpgEma block in front of the stream)
        name = "mpg_" + self.optimizer + ("" if self._ema_block is None else "_ema")
        tail = (st,) if self._ema_block is None else (C.byref(self._ema_block), st)
        if self.optimizer == "rmsprop":
            args = (vp(self.flat), vp(self.grad), vp(self.sq), self.n, lr, 0.99, 1e-8, gscale, z, cnt, add)
        elif self.optimizer == "adam":
            args = (vp(self.flat), vp(self.grad), vp(self.aux), vp(self.sq), vp(self.step_count), self.n,
                    lr, self.betas[0], self.betas[1], 1e-8, self.weight_decay, gscale, z, cnt, add)
        else:
            args = (vp(self.flat), vp(self.grad), vp(self.sq), vp(self.aux), self.n, lr, 0.9, 1e-6, gscale, z, cnt, add)
        _lib.check(getattr(L, name)(*args, *tail), name)
        if not (self.flat.is_cuda and torch.cuda.is_current_stream_capturing()):  # a capture records the launch, it does not run it
            self._host_steps += 1

    def _controlled_step(self, gscale: float, zero_grad: bool, advance_seed):
        """``mpg_step_control`` over the gradient as it stands, then the ``mpg_*_ctl`` entry point: the plain one's arguments (lr
        and gscale unused) with the control's block and the nullable averaged-generator block in front of the stream."""
        ctl = self.control
        ctl.launch(self.grad, gscale)
        vp = lambda t: C.c_void_p(t.data_ptr())
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        z = int(zero_grad)
        cnt, add = (None, 0) if advance_seed is None else (vp(advance_seed), ops.SEED_STEP)
        name = "mpg_" + self.optimizer + "_ctl"
        tail = (C.byref(ctl.block), None if self._ema_block is None else C.byref(self._ema_block), st)
        if self.optimizer == "rmsprop":
            args = (vp(self.flat), vp(self.grad), vp(self.sq), self.n, 0.0, 0.99, 1e-8, gscale, z, cnt, add)
        elif self.optimizer == "adam":
            args = (vp(self.flat), vp(self.grad), vp(self.aux), vp(self.sq), vp(self.step_count), self.n,
                    0.0, self.betas[0], self.betas[1], 1e-8, self.weight_decay, gscale, z, cnt, add)
        else:
            args = (vp(self.flat), vp(self.grad), vp(self.sq), vp(self.aux), self.n, 0.0, 0.9, 1e-6, gscale, z, cnt, add)
        _lib.check(getattr(_lib.lib(), name)(*args, *tail), name)
        if not torch.cuda.is_current_stream_capturing():
            self._host_steps += 1

    def note_step(self):
        """Count one step that ran inside a replayed hipGraph (``TrainStep.step`` calls this)."""
        self._host_steps += 1

    @property
    def steps(self) -> float:
        return float(self.step_count) if self.optimizer == "adam" else float(self._host_steps)

    def rmsprop(self, lr: float, alpha: float = 0.99, eps: float = 1e-8, gscale: float = 1.0):
        assert self.optimizer == "rmsprop" and alpha == 0.99 and eps == 1e-8
        self.step(lr, gscale)

    # -- torch.optim-compatible state ---------------------------------------------------------------
    _STATE_KEYS = {"rmsprop": ("square_avg", None), "adam": ("exp_avg_sq", "exp_avg"), "adadelta": ("square_avg", "acc_delta")}
    # (the carried entries' keys, under the names they had here)
    SEED_KEY, SEED_RANK_KEY, BATCH_KEY, ADA_KEY = SeedState.KEY, SeedState.RANK_KEY, Schedule.KEY, AdaController.KEY

    def _torch_optimizer(self, lr):
        """A torch.optim instance over detached CPU stand-ins of the parameters: the source of truth for the
        ``param_groups`` defaults of this torch version."""
        stand_ins = [torch.zeros(shape) for _, _, shape in self._spans]
        if self.optimizer == "rmsprop":
            return torch.optim.RMSprop(stand_ins, lr=lr)
        if self.optimizer == "adam":
            return torch.optim.Adam(stand_ins, lr=lr, weight_decay=self.weight_decay, betas=self.betas)
        return torch.optim.Adadelta(stand_ins, lr=lr)

    def state_dict(self, lr: float = None, filtered: bool = True) -> dict:
        """What a ``torch.optim.<Optimizer>`` would hold after the same steps.  ``filtered`` (default): built over the
        trainable parameters only, as ``setup_training.optimizers`` does under ``--spectral-norm-gen``
        (``filter(lambda p: p.requires_grad, ...)``, setup_training.py:1500-1509) -- and identical to the unfiltered form for
        a module without frozen parameters.  ``filtered=False``: built over ALL of ``module.parameters()``, frozen ones
        included without state (what the reference's other branch gives a spectral-norm discriminator)."""
        lr = self.lr if lr is None else lr
        if self.control is not None:     # (the effective rate, where a torch.optim.lr_scheduler would leave it)
            lr = self.control.next_lr()
        sd = self._torch_optimizer(1e-2 if lr is None else lr).state_dict()
        k_sq, k_aux = self._STATE_KEYS[self.optimizer]
        steps = torch.tensor(self.steps, dtype=torch.float32)
        if not filtered:
            sd["param_groups"][0]["params"] = list(range(self._n_all))
        if float(steps) > 0:
            for i, (off, k, shape) in enumerate(self._spans):
                ent = {"step": steps.clone(), k_sq: self.sq[off:off + k].view(shape).clone()}
                if k_aux is not None:
                    ent[k_aux] = self.aux[off:off + k].view(shape).clone()
                sd["state"][i if filtered else self._trained_idx[i]] = ent
        for c in self.carried:
            c.save(sd["param_groups"][0])
        return sd

    def load_state_dict(self, sd: dict):
        """Take over the per-parameter state of a ``torch.optim`` state dict of the matching optimizer class.  Its indices
        are positions either in the list of trainable parameters or in all of ``module.parameters()`` (see
        ``state_dict``): told apart by the length of its parameter group; entries may be missing (parameters that were
        never stepped).  Returns the learning rate recorded in it."""
        k_sq, k_aux = self._STATE_KEYS[self.optimizer]
        state = sd["state"]
        groups = sd.get("param_groups") or [{}]
        n_listed = sum(len(g.get("params", ())) for g in groups)
        if n_listed == len(self._spans) or (n_listed == 0 and len(state) <= len(self._spans)):
            index = list(range(len(self._spans)))
        elif n_listed == self._n_all:
            index = self._trained_idx
        else:
            raise ValueError(f"optimizer state lists {n_listed} parameters; the module has {len(self._spans)} trainable "
                             f"of {self._n_all}")
        known = set(index)
        stray = [k for k in state if int(k) not in known]
        if stray:
            raise ValueError(f"optimizer state has entries for parameters {stray} that are not trained here")
        self.sq.zero_()
        if self.aux is not None:
            self.aux.zero_()
        steps = 0.0
        for (off, k, shape), i in zip(self._spans, index):
            ent = state.get(i, state.get(str(i)))
            if ent is None:
                continue
            if k_sq not in ent:
                raise ValueError(f"state of parameter {i} has no {k_sq!r}: not a torch.optim {self.optimizer} state dict")
            if tuple(ent[k_sq].shape) != shape:
                raise ValueError(f"state of parameter {i} has shape {tuple(ent[k_sq].shape)}, expected {shape}")
            self.sq[off:off + k].copy_(ent[k_sq].reshape(-1))
            if k_aux is not None:
                self.aux[off:off + k].copy_(ent[k_aux].reshape(-1))
            steps = max(steps, float(ent.get("step", 0.0)))
        self.step_count.fill_(steps)
        self._host_steps = int(steps)
        self.lr = groups[0].get("lr", self.lr)
        if self.control is not None:     # (a file without the control's key resumes the schedule at the optimizer's step count)
            self.control.loaded_steps = int(steps)
        for c in self.carried:
            c.load(groups[0])
        return self.lr

    def versions(self) -> int:
        """Sum of the autograd version counters of the parameters: changes when anything but the fused optimiser (which
        works on the flat buffer, behind autograd's back) writes them -- ``load_state_dict``, an in-place edit."""
        return sum(p._version for p in self.params)


def _set_requires_grad(flat: "FlatParams", flag: bool):
    for p in flat.params:    # (the trained ones: frozen parameters stay frozen)
        p.requires_grad_(flag)


def _forward_writes_no_state(module: nn.Module) -> bool:
    """No batch norm (running_mean / running_var / num_batches_tracked) and no spectral norm (weight_u / weight_v) anywhere
    in ``module``: its forward reads parameters and buffers only."""
    from .mpgan.model import LinearNet, SpectralNorm
    for m in module.modules():
        if isinstance(m, (SpectralNorm, nn.modules.batchnorm._BatchNorm)) or (isinstance(m, LinearNet) and not m.plain):
            return False
    return True


LOSSES = ("ls", "og", "w", "hinge")


def d_loss(loss: str, out: torch.Tensor, B: int, real: Optional[torch.Tensor] = None,
           extra: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``calc_D_loss`` (train.py:331-395) on D's outputs for the CONCATENATED
    batch ``out[:B]`` = real, ``out[B:]`` = generated: D_real_loss + D_fake_loss, each a mean over its B jets.
    Written on the whole vector with a 0/1 target (no slicing: a slice costs a zero-fill and a copy in autograd).
    Label smoothing / noise (train.py:353-363; ``og`` / ``ls`` only): ``real`` = the per-jet targets and ``extra`` the scalar of
    ``effective_targets``, added to the value."""
    out = out.reshape(-1)
    if real is None:
        real = (torch.arange(2 * B, device=out.device) < B).to(out.dtype)   # 1 for the real half
    if extra is not None:
        return d_loss(loss, out, B, real) + extra.reshape(())
    if loss == "ls":
        return ((out - real) ** 2).sum() / B
    if loss == "og":  # nn.BCELoss (clamps its logarithms at -100)
        return torch.nn.functional.binary_cross_entropy(out, real, reduction="sum") / B
    sign = 1.0 - 2.0 * real                                             # -1 real, +1 generated
    if loss == "w":
        return (sign * out).sum() / B
    if loss == "hinge":
        return torch.relu(1.0 + sign * out).sum() / B
    raise ValueError(f"loss must be one of {LOSSES}, got {loss!r}")


def g_loss(loss: str, out: torch.Tensor) -> torch.Tensor:
    """``calc_G_loss`` (train.py:465-476) on D's outputs for generated jets."""
    out = out.reshape(-1)
    if loss == "ls":
        return ((out - 1.0) ** 2).mean()
    if loss == "og":   # nn.BCELoss against ones: logarithm clamped at -100, its backward's denominator at 1e-12
        return torch.nn.functional.binary_cross_entropy(out, torch.ones_like(out))
    if loss in ("w", "hinge"):
        return -out.mean()
    raise ValueError(f"loss must be one of {LOSSES}, got {loss!r}")


class _GenAhead:
    """The generator-ahead branch of ``TrainStep``: train_G's generator forward on a side stream beside the D step."""
    # Where it joins: at the end of the D segment when that segment is a hipGraph of its own (a capture must end with every
    # forked stream joined), otherwise only where the G step picks its jets up -- so that the D all-reduce (graph_collectives:
    # inside the one graph; eagerly: between the segments) waits for D's backward and its weight-gradient stream alone, not for
    # the generator's forward beside them

    def __init__(self, dev):
        self.dev = dev
        self.stream = None     # (made by the first fork)
        self.jets = None       # what the forked call returned, until ``take``
        self.open = False      # forked and not joined yet
        self.joined = None     # "seg_D" | "seg_G": where the last iteration / capture joined the branch (tests read it)

    def fork(self, generate):  # generate() on the side stream, behind everything the main stream holds so far
        if self.stream is None:
            self.stream = torch.cuda.Stream(device=self.dev)
        main = torch.cuda.current_stream(self.dev)
        self.stream.wait_stream(main)
        self.open = True
        with torch.cuda.stream(self.stream):
            self.jets = generate()
        for t in (self.jets if isinstance(self.jets, tuple) else (self.jets,)):
            if t is not None:
                t.record_stream(main)   # (its consumer, the G step, runs on this stream)

    def join(self, place: str):  # an open branch is ordered before whatever follows on the main stream
        if self.open:
            torch.cuda.current_stream(self.dev).wait_stream(self.stream)
            self.open, self.joined = False, place

    def take(self):  # the forked call's jets (None without a fork), handed over once
        jets, self.jets = self.jets, None
        return jets


class TrainStep:
    """G+D iteration (train.py:829-878 body) with static buffers, optional hipGraph replay and an
    optional process group for data-parallel gradient averaging (RCCL over xGMI).  ``num_critic`` / ``num_gen``: the reference's
    ``--num-critic`` / ``--num-gen`` -- ``step()`` is one batch of the epoch loop and trains D, G or both as train.py:841 / :864
    say for ``batch_ndx`` (``start_epoch()`` where the reference's ``for batch_ndx, ...`` begins); ``last_ran`` names what ran.
    ``track_epoch_losses``: the epoch's loss sums on the device, read by ``epoch_losses()``.  ``label_smoothing`` / ``label_noise``:
    calc_D_loss's two options (train.py:341-363) for ``og`` / ``ls`` -- ``ls`` + smoothing in the reference's [B, B] broadcast
    form, ``og`` + smoothing refused as the reference's BCELoss refuses it, ``w`` / ``hinge`` untouched by either.
    ``ema`` (``step_options.Ema``): an exponential moving average of G's weights, folded by G's optimizer launch (so it moves on
    the batches that train G and on no other; identical on every rank, as the weights are); ``ema_generator()`` hands it out as
    a module, ``fG.ema`` / ``fG.ema_state`` are its buffers.
    ``lr_schedule`` (``step_options.LrSchedule``) / ``grad_clip`` (``step_options.GradClip``): a learning-rate schedule over each
    optimizer's own steps and clipping of each network's (rank-averaged) gradient by its global L2 norm, settled on the device by
    one launch in front of each optimizer launch (``mpg_step_control``), inside the capture; each takes one object for both
    networks or a ``(disc, gen)`` pair whose entries may be None.  ``set_lr`` moves the base rates without a recapture;
    ``step_control`` reads step counts, rates, factors and gradient norms back."""

    def __init__(self, G: nn.Module, D: nn.Module, batch_size: int, num_particles: int, latent: int = 32,
                 lr_disc: float = 3e-5, lr_gen: float = 1e-5, noise_std: float = 0.2, use_graphs: bool = True,
                 process_group=None, world_size: int = 1, batch_real_fake: bool = True, loss: str = "ls",
                 optimizer: str = "rmsprop", betas=(0.9, 0.999), gp_lambda: float = 0.0,
                 graph_collectives: Optional[bool] = None, augment=None, loader=None, num_critic: int = 1, num_gen: int = 1,
                 track_epoch_losses: bool = False, label_smoothing: bool = False, label_noise: float = 0.0,
                 ema: Optional[Ema] = None, lr_schedule=None, grad_clip=None, gp_rows: Optional[bool] = None,
                 gp_attn: Optional[bool] = None, gp_chain: Optional[bool] = None, _ada_split: bool = False):
        if loss not in LOSSES:
            raise ValueError(f"loss must be one of {LOSSES}, got {loss!r}")
        self.dev = dev = next(G.parameters()).device
        gpu = dev.type == "cuda"
        # Label smoothing / label noise (``LabelDraw``), ``og`` / ``ls`` only: ``label_drawn``, ``label_targets`` and ``label_extra``
        # are its three buffers
        self._labels = LabelDraw.from_args(loss, label_smoothing, label_noise, batch_size, dev)
        self.label_smoothing, self.label_noise, self.labels_on = bool(label_smoothing), float(label_noise), self._labels is not None
        if self.labels_on:
            self.label_targets, self.label_extra, self.label_drawn = self._labels.targets, self._labels.extra, self._labels.drawn
        for name, v in (("num_critic", num_critic), ("num_gen", num_gen)):
            if isinstance(v, bool) or not isinstance(v, int) or v < 1:
                raise ValueError(f"{name} must be an integer >= 1, got {v!r}")
        if num_critic > 1 and num_gen > 1:
            raise ValueError(f"num_critic = {num_critic} with num_gen = {num_gen}: the reference's --num-gen says \"num-critic must be "
                             "1 for this to apply\" (setup_training.py:249; train.py:841 ignores num_gen when num_critic > 1)")
        # The update schedule (``--num-critic`` / ``--num-gen``): ``step()`` is one batch of the reference's epoch loop
        # (train.py:829-878) and ``batch_ndx`` its ``enumerate`` index, kept on the host (``start_epoch`` restarts it);
        # ``last_ran`` names what the last ``step()`` ran.
        self.num_critic, self.num_gen = num_critic, num_gen
        self.last_ran = ()

        # Every MPG_* switch of this file is read HERE, once, as the step is built: a change of the environment afterwards
        # reaches neither a later iteration nor ``capture``.  What each one does is said where its attribute is set, below.
        def _switch(name: str, default: str = "1") -> str:
            return os.environ.get(name, default)
        on = {k: _switch(k) != "0" for k in ("MPG_PARTS", "MPG_GEN_AHEAD", "MPG_GEN_AHEAD_LATE", "MPG_WGRAD_SIDE", "MPG_BRIDGE", "MPG_NOISE_MASK")}
        if graph_collectives is None:
            graph_collectives = _switch("MPG_GRAPH_COLLECTIVES", "") == "1"
        # (tests, measurements: the three graphs of a multi-rank iteration without a process group)
        self.split_graphs = bool(_switch("MPG_SPLIT_GRAPHS", ""))
        self.gp_lambda = float(gp_lambda)
        # the penalty's MPLayers on the twice-differentiable row kernels where ``ops.gp_rows_route`` covers them (None: as
        # ``ops.OPTIONS["gp_rows"]`` / MPG_GP_ROWS says as the step is built)
        self.gp_rows = bool(ops.OPTIONS["gp_rows"]) if gp_rows is None else bool(gp_rows)
        # ... and the penalty's attention cores on the twice-differentiable attention kernels where ``ops.gp_attn_route`` covers them
        # (None: as ``ops.OPTIONS["gp_attn"]`` / MPG_GP_ATTN says as the step is built).  The core has no parameters: nothing it
        # hands to autograd meets a gradient of the second stream, so ``wgrad_side`` stays as it is
        self.gp_attn = bool(ops.OPTIONS["gp_attn"]) if gp_attn is None else bool(gp_attn)
        # ... and the penalty's LinearNets and D's head as one twice-differentiable op each where ``ops.gp_chain_route`` /
        # ``ops.gp_head_route`` cover them (None: as ``ops.OPTIONS["gp_chain"]`` / MPG_GP_CHAIN says as the step is built)
        self.gp_chain = bool(ops.OPTIONS["gp_chain"]) if gp_chain is None else bool(gp_chain)
        self.GP = torch.zeros((), device=dev)   # last penalty value (the reference's losses["gp"])
        self.fixed_alpha = None   # tests: the interpolation weights [B, 1, 1] instead of fresh uniform samples
        self.G, self.D = G, D
        self.loss = loss
        # train_D evaluates D on the real and on the generated batch (train.py:432-447).  D has no cross-sample
        # coupling (no batch norm), so one pass over the concatenated 2B jets gives the same outputs and the same
        # summed gradients as the reference's two passes -- with half the launches and twice the workgroups per
        # launch (jets have different multiplicities; more workgroups than CUs evens that out).
        # (with batch norm in D the two passes normalise over their own B jets each: kept as the reference's two passes)
        self.batch_real_fake = batch_real_fake and not any(isinstance(m, nn.modules.batchnorm._BatchNorm) for m in D.modules())
        self.B, self.N, self.latent = batch_size, num_particles, latent
        self.lr_disc, self.lr_gen, self.noise_std = lr_disc, lr_gen, noise_std
        self.pg, self.world = process_group, world_size
        # RCCL collectives can be captured into a hipGraph like kernels: the two gradient all-reduces then sit INSIDE
        # one graph and a multi-rank iteration is a single replay.  Opt-in (argument, or MPG_GRAPH_COLLECTIVES=1):
        # the default keeps the all-reduces as ordinary calls between three graph segments.
        self.graph_collectives = bool(graph_collectives) and process_group is not None
        self.state = ops.dev_state(dev)
        if ema is not None and not isinstance(ema, Ema):
            raise TypeError(f"ema must be a step_options.Ema, got {type(ema).__name__}")
        # (Ema(kimg=...): the half-life counts the jets of all ranks)
        # the step controls (``StepControl``): one per network that has a schedule or a clip; None: that optimizer's launch as it was
        def _pair(v, name, cls):
            pair = tuple(v) if isinstance(v, (tuple, list)) else (v, v)
            if len(pair) != 2 or not all(x is None or isinstance(x, cls) for x in pair):
                raise TypeError(f"{name} must be a step_options.{cls.__name__}, None or a (disc, gen) pair of those, got {v!r}")
            return pair
        scheds, clips = _pair(lr_schedule, "lr_schedule", LrSchedule), _pair(grad_clip, "grad_clip", GradClip)
        if not gpu and any(x is not None for x in scheds + clips):
            raise ValueError("lr_schedule / grad_clip: the step control is a launch in front of the fused optimizer launch; the "
                             "step's networks are not on a GPU")
        ctl_D, ctl_G = (None if s is None and c is None else StepControl(lr, s, c, dev)
                        for lr, s, c in zip((lr_disc, lr_gen), scheds, clips))
        self.fG = FlatParams(G, optimizer, betas, ema=ema, batch_size=batch_size * world_size, control=ctl_G)
        self._ema_twin = None        # (``ema_generator`` builds it on first use)
        # (adaptive augmentation over ranks: the sign count's slot at the tail of D's gradient buffer, see ``AdaController``)
        ada_split = (augment is not None and AdaController.splits(augment, process_group, world_size, _ada_split)
                     and ops.augment_flags(augment.aug_r90, augment.aug_f, augment.aug_t, augment.aug_s) != 0)
        self.fD = FlatParams(D, optimizer, betas, tail=1 if ada_split else 0, control=ctl_D)
        self._schedule = Schedule()      # (the schedule's batch index: saved with G's optimizer state, see ``batch_ndx``)
        self._seed = None
        if gpu:
            # The generator's noise and every dropout mask come from counter-based streams keyed by the DEVICE seed, which
            # torch.manual_seed does not reach.  Unless the caller has set it (ops.set_seed), derive it here from torch's
            # seed -- the reference's contract: torch.manual_seed(seed), setup_training.py:184 -- and this process's rank,
            # so that data-parallel ranks never share noise or masks; it is saved / restored with G's optimizer state.
            # A second TrainStep on the same device under the same (torch seed, rank) -- a bench's secondary workload, a step
            # re-created for another batch size -- leaves the stream where the first one has brought it; a new torch.manual_seed
            # in between starts it afresh.
            rank = 0
            if torch.distributed.is_available() and torch.distributed.is_initialized():
                rank = torch.distributed.get_rank(process_group)
            key = (torch.initial_seed(), rank)
            if self.state.seed_is_default and self.state.auto_seed_key != key:
                ops.set_seed(ops.derived_seed(*key), dev, _auto=True)
                self.state.auto_seed_key = key
            self._seed = SeedState(dev, rank)
            # arrival counters of the sender-chunked launches (ops._tickets): allocated and zeroed HERE, on the default stream, for
            # the step's largest launch (the D step's 2B jets) -- never inside a capture, never first on a side stream
            ops.reserve_tickets(dev, 2 * batch_size * ((num_particles + 31) // 32))
        self.data = torch.zeros(batch_size, num_particles, 4, device=dev)
        self.labels = torch.zeros(batch_size, 1, device=dev)
        self._real = torch.cat([torch.ones(batch_size, device=dev), torch.zeros(batch_size, device=dev)])
        # the discriminator's real + generated batch of the D step: real jets in the first half (set_batch), the
        # generator's output rows land in the second half; labels likewise
        self._dcat = torch.zeros(2 * batch_size, num_particles, 4, device=dev)
        self._labels2 = torch.zeros(2 * batch_size, 1, device=dev)
        # ... and, where both networks take it (``generate_parts`` / ``features_parts``), held APART: particle features, mask and
        # 1 - mask of the 2B jets.  The reference glues the mask on as a fourth column, D splits it off again and autograd pads
        # the gradient back to four columns: three elementwise launches per pass that carry no information
        self._x3 = torch.zeros(2 * batch_size, num_particles, 3, device=dev)
        self._mask2 = torch.zeros(2 * batch_size, num_particles, 1, device=dev)
        self._ign2 = torch.zeros(2 * batch_size, num_particles, device=dev)
        self.parts = (gpu and hasattr(G, "generate_parts") and hasattr(D, "features_parts") and D.parts_ok()
                      and getattr(G, "use_mask", True) and not getattr(G, "lfc", False)
                      and getattr(G, "mask_args", {}).get("mask_c", True) and on["MPG_PARTS"])
        self.D_loss = torch.zeros((), device=dev)
        self.G_loss = torch.zeros((), device=dev)
        self.use_graphs = use_graphs and gpu
        self._graphs = None          # the D+G iteration's graphs
        self._alone_graphs = {}      # "D" / "G": the graphs of a batch on which only one of the two trains, captured on first use
        self._pool = None            # (the memory pool all of them share)
        # Epoch losses (train.py:862, :865, :960-962): sums of D_loss, GP and G_loss in device memory, added to behind the launch
        # that writes each loss -- one small launch per loss, only when asked for; ``epoch_losses`` reads them
        self.epoch_sums = {k: torch.zeros((), device=dev) for k in ("D", "gp", "G")} if track_epoch_losses else None
        self._epoch_steps = 0
        # The G step's generator forward depends on nothing the D step writes (G's weights, fresh noise, the labels): it is
        # launched at the top of the D step on a second stream and runs BESIDE it -- the edge launches of a batch of 256 jets
        # are one workgroup per CU and as long as their fullest jet, so a fifth of the chip idles at the end of each; work
        # from an independent stream starts on those CUs (measured on one box: 104.3k -> 105.9k jets/s).  Message-passing
        # generators only: the attention blocks are one-wave-per-jet latency chains with no idle CUs to fill, and a second
        # stream beside them cost 4.7 % (650.6k -> 619.8k).  MPG_GEN_AHEAD=0 switches it off.
        # Only for a generator whose forward writes NO module state: with batch norm (running statistics) or spectral norm
        # (power-iteration vectors) the forked train-mode forward would update what the D step's eval-mode call reads on
        # the main stream at the same time -- a race, and the reference's order the other way round (train.py:432-447 before
        # :500-511).
        self.gen_ahead = gpu and isinstance(G, MPGenerator) and _forward_writes_no_state(G) and on["MPG_GEN_AHEAD"]
        self._ahead = _GenAhead(dev)      # (never forked without gen_ahead)
        # The launches that only produce weight gradients (mpg_edge_dw + reduction, the grouped node-network weight
        # gradients: about a quarter of the step) feed nothing before the optimizer: they run on a second side stream, forked
        # per layer behind mpg_edge_bwd and joined at the end of the backward (before the all-reduce / optimizer step), so
        # that they start on CUs the one-round data-gradient launches leave idle and their launch boundaries stop
        # serialising with the data path.  MPG_WGRAD_SIDE=0 switches it off.
        self.wgrad_side = gpu and on["MPG_WGRAD_SIDE"]
        # (not beside the penalty on the rows route: there D's edge-network parameters get gradients from two sides in one backward --
        #  added into .grad by the fused layers' launches on that second stream, and handed to autograd by the twice-differentiable
        #  op, whose accumulation runs on the main stream.  On one stream the two are ordered, in eager execution and in a replay alike)
        # (nor beside the chained LinearNets and the head: their parameter gradients are autograd values as well)
        if self.gp_lambda and (self.gp_rows or self.gp_chain):
            self.wgrad_side = False
        self._wside = None
        # The generator-ahead branch is forked at the top of the D segment (MPG_GEN_AHEAD_LATE=0: beside the D step's own
        # generator call), or -- default -- behind the D step's last data-gradient launch, beside the weight-gradient tail
        # (_backward): the lower layer's mpg_edge_dw, its reduction, the grouped weight gradients, the optimizer and the packing
        # are small or latency-bound launches that leave most CUs idle, and two full-chip forwards fill them
        self.gen_ahead_late = self.gen_ahead and self.wgrad_side and on["MPG_GEN_AHEAD_LATE"]
        self.bridge = gpu and on["MPG_BRIDGE"]      # (see ``_bridge``)
        # Jet augmentation (``Augmenter``): one launch on the generated half of the D step's batch, one each way between the
        # generator's jets and the discriminator in the G step -- and its adaptive probability (``AdaController``), which moves
        # the augmenter's probability word ``aug_p``.  With the four switches off there is nothing to adapt: no launch, no buffers.
        self.aug = self.aug_p = self._ada = None
        if augment is not None:
            self.aug_p = torch.full((1,), float(augment.aug_prob), device=dev)
            self.aug = Augmenter.from_args(augment, self.aug_p, batch_size)
        if self.aug is not None:
            self.aug_params = self.aug.params
            self._ada = AdaController.from_args(augment, self.aug_p, loss, batch_size, world_size, process_group, _ada_split,
                                                self.fD.tail)
        self.ada_state, self.ada_r = (None, None) if self._ada is None else (self._ada.state, self._ada.r)    # (the controller's words)
        # the generator's noise and its jets' masks drawn by one launch (MPG_NOISE_MASK=0: mpg_normal, then mpg_rank_mask)
        self.noise_mask = gpu and on["MPG_NOISE_MASK"]
        self.fixed_noise = None  # tests: (noise_D, noise_G) used instead of fresh samples
        self._seen_versions = (self.fD.versions(), self.fG.versions())
        # the flat gradient buffers start as zeros and every optimizer launch of an iteration leaves them cleared again
        # (FlatParams.step(zero_grad=True)): no memset of its own at the top of train_D / train_G.  A caller that accumulates
        # into the networks' .grad between iterations calls ``mark_grads_dirty()``.
        self._clean = {"D": True, "G": True}
        # what outlives an iteration, by the optimizer file that carries it (the keys' order in G's file: seed, rank, batch_ndx)
        self.fG.carried = [c for c in (self._seed, self._schedule) if c is not None]
        self.fD.carried = [c for c in (self._ada,) if c is not None]
        if self.epoch_sums is not None:
            self.fG.carried.append(DeviceWords(self.epoch_sums.values()))
        if self.fG.ema_carried is not None:      # (the average and its words: the warm-up of ``capture`` puts both back)
            self.fG.carried.append(self.fG.ema_carried)
        for f in (self.fD, self.fG):             # (the controls' words: t, base, out)
            if f.control is not None:
                f.carried.append(f.control)
        # a device-resident data set (data.DeviceJetLoader): its feed launch is the first thing of every iteration
        self.loader = None
        if loader is not None:
            self.attach_loader(loader)

    @property
    def gen_join(self):      # ("seg_D" | "seg_G", None before the first join: tests read it)
        return self._ahead.joined

    def attach_loader(self, loader):
        """Take the batches from ``loader`` (``data.DeviceJetLoader``) instead of ``set_batch``: one launch at the top of the D
        segment, inside the capture on every route.  Before the first captured ``step``."""
        if self._graphs is not None or self._alone_graphs:
            raise RuntimeError("attach_loader: the iteration has been captured already (the feed launch is part of the graph); "
                               "attach the loader before the first step")
        if loader.batch_size != self.B or loader.num_particles != self.N:
            raise ValueError(f"loader serves batches of {loader.batch_size} jets of {loader.num_particles} particles; the step "
                             f"was built for {self.B} x {self.N}")
        if loader.device != self.data.device:
            raise ValueError(f"loader lives on {loader.device}, the step on {self.data.device}")
        self.loader = loader
        self.fG.carried.append(DeviceWords([loader.cursor]))     # (the warm-up iterations of ``capture`` consume no jets)

    # -- the three segments between collectives ------------------------------------------------
    def _noise(self, which: int = 0):
        if self.fixed_noise is not None:
            return self.fixed_noise[which]
        if self.dev.type == "cuda":   # counter-based, keyed by the device seed (bumped once per iteration) and the draw's site
            return ops.normal_noise((self.B, self.N, self.latent), self.noise_std, site=which, device=self.dev)
        return torch.empty(self.B, self.N, self.latent, device=self.dev).normal_(0.0, self.noise_std)

    def _noise_masked(self, which: int, mask_out=None, ign_out=None):
        """(noise, premask): the generator's input and -- when its mask depends on nothing else (``noise_mask_ok``) -- the
        jets' masks from the same launch, written into the caller's rows when given; premask None otherwise."""
        if (self.fixed_noise is None and self.noise_mask and self.dev.type == "cuda"
                and getattr(self.G, "noise_mask_ok", lambda: False)() and (self.N * self.latent) % 2 == 0):
            z, m, ig = ops.normal_noise_masked((self.B, self.N, self.latent), self.noise_std, self.labels, site=which, device=self.dev,
                                               mask_out=None if mask_out is None else mask_out.view(self.B, -1),
                                               ignore_out=None if ign_out is None else ign_out.view(self.B, -1))
            return z, (m, ig)
        return self._noise(which), None

    def _fused_ends(self) -> bool:
        """Generator able to write its jets into a caller-owned batch and discriminator whose pooling / last Linear /
        final activation / loss are the single fused head (``ops.disc_head_loss``): the default MPGAN and GAPT
        configurations.  Then an iteration has no autograd node and no elementwise ATen kernel between the last
        message-passing / attention block and the loss, in either direction."""
        return (self.dev.type == "cuda" and hasattr(self.G, "generate_into") and hasattr(self.D, "features")
                and getattr(self.D, "fused_head", lambda: None)() is not None and self.batch_real_fake
                and not self.gp_lambda)

    def set_aug_prob(self, p: float):
        """The augmentation probability from the next iteration on (the reference's ``aug_prob`` / ``augment_p[-1]``); a
        captured graph reads it from device memory: no recapture.  Under ``adaptive_prob`` the controller goes on from the value."""
        if self.aug_p is None:
            raise RuntimeError("TrainStep was built without augmentation")
        self.aug_p.fill_(float(p))

    def set_lr(self, lr_disc: Optional[float] = None, lr_gen: Optional[float] = None):
        """The base learning rates from the next step on (None: as it is).  On a network built with ``lr_schedule=`` / ``grad_clip=``
        the value is written to device memory on the current stream and a captured graph follows it: no recapture.  On a network
        without, the rate is an argument of the optimizer launch and a constant of a captured graph: allowed until the first
        capture, an error after it."""
        for name, lr, flat in (("lr_disc", lr_disc, self.fD), ("lr_gen", lr_gen, self.fG)):
            if lr is None:
                continue
            if flat.control is not None:
                flat.control.set_base(lr)
            elif self._graphs is not None or self._alone_graphs:
                raise RuntimeError(f"set_lr({name}=...): the iteration has been captured with this learning rate as a constant of "
                                   "its graphs; build the step with lr_schedule= (LrSchedule([]) keeps the rate as it is) or "
                                   "grad_clip= to move it afterwards")
            setattr(self, name, float(lr))

    @property
    def step_control(self) -> dict:
        """{"D": {...}, "G": {...}}: per network ``t`` (controlled optimizer steps taken) and the last step's ``lr`` (effective),
        ``factor`` (the schedule's), ``norm`` (of the rank-averaged gradient, 0 when none is computed) and ``clip`` (the factor the
        clipping put on the gradient); None for a network without control.  Synchronises -- read it once per epoch, beside the
        loss log, not per iteration."""
        if self.fD.control is None and self.fG.control is None:
            raise RuntimeError("TrainStep was built without lr_schedule / grad_clip")
        return {k: None if f.control is None else f.control.read() for k, f in (("D", self.fD), ("G", self.fG))}

    @property
    def ada(self) -> dict:
        """{p, r, sign_sum, steps} of the adaptive probability: the probability now, the last finished interval's r (0 before the
        first), and the open interval's sign sum and count of D steps.  Read-only, and the one place that synchronises."""
        if self._ada is None:
            raise RuntimeError("TrainStep was built without adaptive_prob (or with every augmentation switch off)")
        return self._ada.read()

    @property
    def ada_keep_out(self) -> bool:      # (tests: the controller's hook)
        return self._ada.keep_out

    @ada_keep_out.setter
    def ada_keep_out(self, keep: bool):
        self._ada.keep_out = keep

    @property
    def ada_last_out(self):
        return self._ada.last_out

    def _augment(self, x: torch.Tensor, site: int, in_place: bool = False) -> torch.Tensor:
        return self.aug.apply(x, site, in_place)

    def _bridge(self) -> bool:
        """GAPT: gen's ``final_fc`` + tanh and disc's ``input_embedding`` as one launch each way (``ops.GenDiscBridgeFn``;
        MPG_BRIDGE=0: the three launches).  Not while augmenting: the map sits between the tanh and the embedding."""
        if self.aug is not None or not self.bridge or not hasattr(self.G, "bridge_head") or not hasattr(self.D, "bridge_tail"):
            return False
        h, t = self.G.bridge_head(), self.D.bridge_tail()
        # (final_fc's weight is a view into the flat parameter buffer: the launch reads its rows as float4 -- a generator composed
        # so that the view starts off a 16-byte boundary takes the three launches instead)
        return h is not None and t is not None and ops.bridge_fusable(h[0].shape[1], h[0].shape[0], t[0].shape[0]) \
            and t[0].shape[1] == h[0].shape[0] and h[0].data_ptr() % 16 == 0

    def _route(self, rows_ok: bool = True) -> str:
        """How the generator's jets reach the discriminator in the segment that asks (``rows_ok=False``: not by "rows")."""
        #   "rows"    the one-launch bridge (``generate_rows`` -> ``features_rows``)
        #   "parts"   features and mask held apart (``generate_parts`` -> ``features_parts``)
        #   "into"    the [B, N, 4] batch with the fused head (``generate_into`` / ``G(...)`` -> ``features``)
        #   "module"  the plain modules with a torch loss: gradient penalty, batch norm in D, CPU toy networks
        # Asked at the top of each segment and never kept: ``GAPT_G.bridge_head`` depends on ``G.training``, which differs
        # between train_D and train_G, and weights may be swapped between steps.
        if not self._fused_ends():
            return "module"
        if not self.parts:
            return "into"
        return "rows" if rows_ok and self._bridge() else "parts"

    def _generate_for_D(self, route: str):
        """train_D's generated half (train.py:432-442), without gradient: (the generated jets, augmented in place; the 2B jets of
        the static batch as ``_features`` takes them, the generated ones written behind the real ones -- None on "module")."""
        # ("rows": the generator's rows stand in for the features and there are no jets yet -- never augmented: ``_bridge``)
        own = slice(self.B, None)
        with torch.no_grad():
            if route in ("rows", "parts"):
                rows = {"mask_out": self._mask2[own], "ign_out": self._ign2[own]}
                z, pm = self._noise_masked(0, **rows)
                if route == "rows":
                    fake, jets = None, (self.G.generate_rows(z, self.labels, premask=pm, **rows)[0], self._mask2, self._ign2)
                else:
                    fake, jets = self._x3[own], (self._x3, self._mask2, self._ign2)
                    self.G.generate_parts(z, self.labels, feat_out=fake, premask=pm, **rows)
            elif route == "into":
                fake, jets = self._dcat[own], self._dcat
                self.G.generate_into(self._noise(0), self.labels, fake)
            else:
                fake, jets = self.G(self._noise(0), self.labels), None
            if self.aug is not None:       # (D(real) sees the batch as it is: train.py:425 runs before the augmentation)
                fake = self._augment(fake, AUG_SITES["D_fake"], in_place=True)
        return fake, jets

    def _generate(self, route: str):
        """train_G's ``gen_data = gen(...)`` (train.py:500-511): (rows or particle features, mask, 1 - mask) or [B, N, 4] jets."""
        if route in ("rows", "parts"):
            z, pm = self._noise_masked(1)
            return (self.G.generate_rows if route == "rows" else self.G.generate_parts)(z, self.labels, premask=pm)
        return self.G(self._noise(1), self.labels)

    def _features(self, route: str, jets, labels, gen_step: bool):
        """D up to its fused head on a fused route: (y, mask) for ``_head_loss_backward``."""
        if route == "into":
            return self.D.features(jets, labels)
        x, mask, ign = jets
        if route == "parts":
            return self.D.features_parts(x, mask, labels, ignore=ign)
        head, real = self.G.bridge_head(), None
        if not gen_step:
            # (the generator takes no gradient in train_D: its final_fc enters the launch as plain data; the generated
            # features are written behind the real ones)
            head, real = (head[0].detach(), None if head[1] is None else head[1].detach(), head[2]), self._x3
        return self.D.features_rows(x, head, real, mask, labels, ignore=ign)

    def _head_loss_backward(self, y, mask, gen_step: bool, then=None):
        """The fused head with its loss (train_D: with the head's own weight gradients), then the backward from (y, dy)."""
        w, b, mean, sigmoid, p = self.D.fused_head()
        # (train_D under label smoothing / noise: the targets ``LabelDraw.draw`` left; calc_G_loss has neither)
        lab = {"targets": self.label_targets, "loss_extra": self.label_extra} if self.labels_on and not gen_step else {}
        out, dy = ops.disc_head_loss(y, mask, w, b, mean=mean, sigmoid=sigmoid, p_drop=p, training=self.D.training, loss=self.loss,
                                     n_real=self.B, gen_step=gen_step, count=self.B, loss_out=self.G_loss if gen_step else self.D_loss,
                                     want_dy=True, wgrad=None if gen_step else (w.grad, None if b is None else b.grad), **lab)
        if self._ada is not None and not gen_step:     # (directly behind the head, on its stream: train_G's augmentation reads the new p)
            self._ada.update(out, self.B)
        self._sum_epoch("G" if gen_step else "D")
        self._backward(y, dy, then)

    def _sum_epoch(self, key: str):   # epoch_loss[key] += ... (train.py:862, :865) in device memory, behind the launch that wrote the loss
        if self.epoch_sums is not None:
            self.epoch_sums[key].add_({"D": self.D_loss, "gp": self.GP, "G": self.G_loss}[key])

    def _seg_D(self, join: bool = True, fork: bool = True):  # train_D up to and including backward (train.py:419-460)
        # (join=False: the generator-ahead branch stays open for a _seg_G that follows in the same graph / eager run;
        # fork=False: a batch on which the generator does not train -- no _seg_G follows, so the branch is never opened)
        self._open_batch()
        if fork and self.gen_ahead and not self.gen_ahead_late:
            self._fork_generator()
        self.G.eval()
        if not self._clean["D"]:     # (cleared by the optimizer launch of the iteration before: see _seg_G)
            self.fD.zero_grad()
        self._clean["D"] = False
        _set_requires_grad(self.fD, True)
        try:
            self._seg_D_body(self._fork_generator if fork and self.gen_ahead_late else None)
        finally:
            if join:     # everything of this segment is ordered before whatever follows it
                self._ahead.join("seg_D")

    def _open_batch(self):   # the top of every batch, whichever network trains on it
        if self.loader is not None:     # (first: the generator-ahead branch reads self.labels)
            self.loader.feed(self)
        # parameter gradients are added straight into the flat buffers (no AccumulateGrad kernel per parameter)
        self.state.grad_into_param = True
        self.state.order_cache = None   # (ops.jet_order: the masks of this iteration live where last iteration's did)
        # (the dropout / noise seed of this iteration was set by the last launch of the iteration before: _close_batch)
        self.D.train()

    def _close_batch(self, net: str):   # the batch's last optimizer step ("D" | "G"), which also moves the seed on
        # (what ops.bump_seed at the head of the next train_D would do in a launch of its own)
        flat, lr = (self.fD, self.lr_disc) if net == "D" else (self.fG, self.lr_gen)
        flat.step(lr, gscale=1.0 / self.world, zero_grad=True, advance_seed=ops.seed_tensor(self.dev))
        self._clean[net] = True
        self._refresh_packed(flat.module)
        self.state.grad_into_param = False

    def _fork_generator(self):
        """train_G's ``gen_data = gen(...)`` (train.py:500-511) on the side stream, in training mode."""
        # (never by the "rows" route: the branch exists for ``MPGenerator`` only -- ``gen_ahead`` -- which has no bridge)
        # G's weight images are shared by this forward and the D step's own generator call: built (on first use, or behind an
        # outside write) on THIS stream, before the fork -- built inside the forward they would be written on the side stream
        # while the other call reads them
        self.G.train()
        for m in self.G.modules():
            if hasattr(m, "_packed") and getattr(m, "fused", False):
                m._packed().ensure()
        self._ahead.fork(lambda: self._generate(self._route(rows_ok=False)))

    def _seg_D_body(self, late_fork=None):
        route = self._route()
        fake, jets = self._generate_for_D(route)
        if route != "module":
            if self.labels_on:
                self._labels.draw()
            # real jets sit in the first half of the static batch; the generator has written the second half itself
            return self._head_loss_backward(*self._features(route, jets, self._labels2, False), False, late_fork)
        if self.batch_real_fake:
            out = self.D(torch.cat([self.data, fake], 0), torch.cat([self.labels, self.labels], 0))
        else:
            out = torch.cat([self.D(self.data.clone(), self.labels).reshape(-1), self.D(fake, self.labels).reshape(-1)])
        if self.labels_on:     # (drawn where calc_D_loss draws them: behind both passes of D, in front of the penalty)
            self._labels.draw()
            loss = d_loss(self.loss, out, self.B, self.label_targets, self.label_extra)
        else:
            loss = d_loss(self.loss, out, self.B, self._real)
        self.D_loss.copy_(loss.detach())   # (D_real_loss + D_fake_loss: the reference's losses["D"] leaves the penalty out)
        self._sum_epoch("D")
        if self.gp_lambda:
            real = self.data
            if self.aug is not None:       # (calc_D_loss is handed the augmented real batch: train.py:441, :452)
                with torch.no_grad():
                    real = self._augment(self.data, AUG_SITES["D_real"])
            gp = self.gradient_penalty(real, fake)
            self.GP.copy_(gp.detach())
            self._sum_epoch("gp")
            loss = loss + gp
        if self._ada is not None:
            # behind the penalty's augmentation of the real batch: every augmentation launch of this D step has read the old p
            self._ada.update(out.detach().reshape(-1), self.B)
        self._backward(loss, then=late_fork)

    def gradient_penalty(self, real: torch.Tensor, fake: torch.Tensor) -> torch.Tensor:
        """``gradient_penalty`` of train.py:286-324:  gp_lambda * mean_b (|| dD(x_b)/dx_b ||_2 - 1)^2  at
        x = a real + (1 - a) generated, a ~ U[0, 1) per jet; D is called without labels, the norm runs over all
        particles and features of a jet (mask column included) with 1e-12 under the root.  D(x) runs on the
        double-backward route, so that the penalty can be back-propagated into D's parameters (a discriminator that is
        plain torch is twice differentiable as it is; the fused kernels decline a second derivative loudly)."""
        B = real.shape[0]
        alpha = self.fixed_alpha if self.fixed_alpha is not None else torch.rand(B, 1, 1, device=real.device)
        x = (alpha * real + (1 - alpha) * fake.detach()).requires_grad_(True)
        prev, ops.OPTIONS["gp_rows"] = ops.OPTIONS["gp_rows"], self.gp_rows
        prev_attn, ops.OPTIONS["gp_attn"] = ops.OPTIONS["gp_attn"], self.gp_attn
        prev_chain, ops.OPTIONS["gp_chain"] = ops.OPTIONS["gp_chain"], self.gp_chain
        try:
            with ops.double_backward_route(self.dev):
                prob = self.D(x)
                grads = torch.autograd.grad(prob, x, torch.ones_like(prob), create_graph=True, retain_graph=True)[0]
        finally:
            ops.OPTIONS["gp_rows"], ops.OPTIONS["gp_attn"], ops.OPTIONS["gp_chain"] = prev, prev_attn, prev_chain
        norm = torch.sqrt((grads.reshape(B, -1) ** 2).sum(1) + 1e-12)
        return self.gp_lambda * ((norm - 1) ** 2).mean()

    def _backward(self, root, grad=None, then=None):
        """root.backward(grad) with the stand-alone Linear layers' weight gradients collected and issued as grouped
        launches that add straight into the flat gradient buffers."""
        # (then: called behind the last of them and before the weight-gradient stream joins, never behind a failed backward --
        # train_D's late fork of the generator-ahead branch)
        self.state.deferred_wgrad = ops.WgradBatch()
        if self.wgrad_side:
            if self._wside is None:
                self._wside = torch.cuda.Stream(device=self.dev)
            self.state.wgrad_stream = self._wside
        try:
            torch.autograd.backward([root], None if grad is None else [grad])
            self.state.deferred_wgrad.flush()
            if then is not None:
                then()
        finally:
            self.state.deferred_wgrad = None
            if self.wgrad_side:
                # join: the weight gradients are complete before whatever follows the backward (all-reduce, optimizer step)
                self.state.wgrad_stream = None
                torch.cuda.current_stream(self.dev).wait_stream(self._wside)
                self.state.wgrad_keep.clear()

    @staticmethod
    def _refresh_packed(module: nn.Module):
        # the fused optimiser wrote the parameters behind autograd's back: rebuild the layers' cached weight images,
        # all layers of the network in as few launches as the pack-job limit allows
        packs = []
        for m in module.modules():
            if hasattr(m, "packed_sets"):
                packs += m.packed_sets()
            elif hasattr(m, "refresh_packed"):
                m.refresh_packed()
        if packs:
            ops.refresh_many(packs)

    def _settle_ada(self):   # first behind D's gradient all-reduce: the ranks' sign counts have been added (``AdaController.settle``)
        if self._ada is not None and self._ada.split:
            self._ada.settle()

    def _seg_D_end(self):  # D_optimizer.step() (train.py:461) of a batch on which the generator does not train
        self._settle_ada()
        # the seed moves on HERE, as it does in G's optimizer launch otherwise (_seg_end): the next critic step would redraw this
        # one's generator noise, dropout masks and augmentation maps without it
        self._close_batch("D")

    def _seg_G(self, alone: bool = False):  # D_optimizer.step() (train.py:461) + train_G up to backward (:494-520)
        if alone:
            # a batch on which the discriminator does not train (num_gen > 1): what the top of _seg_D sets up, and train_G --
            # the data loader yields the batch all the same, and train_G takes its labels (train.py:832-835, :872)
            self._open_batch()
        else:
            self._settle_ada()     # (in front of train_G's augmentation, which reads the new p)
            # optimizer.zero_grad() of the next train_D (train.py:419) rides in this launch: the buffer is cleared behind its last use
            self.fD.step(self.lr_disc, gscale=1.0 / self.world, zero_grad=True)
            self._clean["D"] = True
            self._refresh_packed(self.D)
        self.G.train()
        if not self._clean["G"]:
            self.fG.zero_grad()
        self._clean["G"] = False
        _set_requires_grad(self.fD, False)
        self._ahead.join("seg_G")    # (a branch the D segment left open: its jets are used from here on)
        ahead = self._ahead.take()
        route = self._route(rows_ok=ahead is None)     # (the branch's jets came by ``_route(rows_ok=False)`` as well)
        fake = self._generate(route) if ahead is None else ahead
        if self.aug is not None:     # (here, on the main stream, also for jets the generator-ahead branch made)
            if isinstance(fake, tuple):
                fake = (self._augment(fake[0], AUG_SITES["G_fake"]),) + tuple(fake[1:])
            else:
                fake = self._augment(fake, AUG_SITES["G_fake"])
        if route != "module":
            self._head_loss_backward(*self._features(route, fake, self.labels, True), True)
        else:
            loss = g_loss(self.loss, self.D(fake, self.labels))
            self._backward(loss)
            self.G_loss.copy_(loss.detach())
            self._sum_epoch("G")
        _set_requires_grad(self.fD, True)

    def _seg_end(self):  # G_optimizer.step() (train.py:521)
        self._close_batch("G")

    def mark_grads_dirty(self):
        """Tell the step that something outside it wrote the networks' .grad buffers (they are views of the flat gradient
        buffers): both are cleared HERE, eagerly, on the current stream.  The iteration itself has no memset -- every optimizer
        launch leaves its buffer cleared behind its last use, so ``.grad`` reads as zeros after ``step()`` (log gradient norms
        between ``_seg_D`` / ``_seg_G`` and the following segment) -- and a captured hipGraph contains none either: a host
        flag read at capture time could not reach a replay."""
        self.fD.zero_grad()
        self.fG.zero_grad()
        self._clean = {"D": True, "G": True}

    def _allreduce(self, flat: FlatParams):
        # sum; 1/world is folded into the optimiser step.  (grad_all: the buffer with its tail -- D's carries the sign count)
        mdist.allreduce_sum_(flat.grad_all, self.pg, self.world)

    # -- which of train_D / train_G a batch runs, and the segments of each kind of batch --------------
    KINDS = {"DG": ("D", "G"), "D": ("D",), "G": ("G",)}

    def _kind(self, batch_ndx: int) -> str:
        """"DG", "D" or "G": what the reference's loop runs on batch ``batch_ndx`` of an epoch."""
        b = batch_ndx
        run_D = self.num_critic > 1 or (b == 0 or (b - 1) % self.num_gen == 0)      # train.py:841
        run_G = self.num_critic == 1 or (b - 1) % self.num_critic == 0             # train.py:864
        return "DG" if run_D and run_G else ("D" if run_D else "G")                # (never neither: one of the two counts is 1)

    def _segments(self, kind: str, joined: bool = False):
        """The segments of one batch of ``kind``, in order: (segment, the network whose gradient all-reduce follows it or None)."""
        # (joined: the D segment ends with the generator-ahead branch joined -- a hipGraph of its own; otherwise the branch stays
        # open for the _seg_G that follows in the same graph / eager run)
        if kind == "DG":
            seg_D = self._seg_D if joined else (lambda: self._seg_D(join=False))
            return [(seg_D, self.fD), (self._seg_G, self.fG), (self._seg_end, None)]
        if kind == "D":
            return [(lambda: self._seg_D(fork=False), self.fD), (self._seg_D_end, None)]
        return [(lambda: self._seg_G(alone=True), self.fG), (self._seg_end, None)]

    def _eager(self, kind: str = "DG"):
        for seg, flat in self._segments(kind):
            seg()
            if flat is not None:
                self._allreduce(flat)

    def _training_state(self):
        """Everything an iteration changes: the losses; parameters, optimiser moments and step counters; what a FORWARD
        changes -- the modules' buffers (batch norm's running statistics and batch counter) and frozen parameters (spectral
        norm's power-iteration vectors, written in place by ``SpectralNorm.weight``); and the device words of every carried
        entry (the dropout seed, the epoch's sums, the loader's cursor, the adaptive probability)."""
        ts = [self.D_loss, self.G_loss, self.GP]
        for f in (self.fD, self.fG):
            ts += [f.flat, f.sq, f.step_count] + ([f.aux] if f.aux is not None else [])
            ts += list(f.module.buffers()) + [p for p in f.module.parameters() if not p.requires_grad]
            ts += [t for c in f.carried for t in c.tensors()]
        return ts

    def capture(self, warmup: int = 3, kind: str = "DG"):
        """Warm up eagerly on a side stream, then capture the three segments into hipGraphs.  The warm-up iterations are
        real ones (kernels get loaded, their LDS limits set, the allocator's pools filled -- none of which may happen
        during a capture): the training state is saved before and put back after them, so capturing -- which ``step``
        does on its first call -- leaves parameters, optimiser state, step counters and the dropout seed where they
        were.  (A run resumed from a checkpoint continues from exactly the state it loaded.)
        ``kind``: the batch captured -- "DG" (train_D and train_G), or "D" / "G" where the num_critic / num_gen schedule runs
        one of them alone; ``step`` captures each on its first use, in the middle of a run as well, all from one memory pool."""
        if kind not in self.KINDS:
            raise ValueError(f"kind must be one of {tuple(self.KINDS)}, got {kind!r}")
        s = torch.cuda.Stream(device=self.dev)
        s.wait_stream(torch.cuda.current_stream(self.dev))
        with torch.cuda.stream(s):
            if warmup:
                saved = [t.clone() for t in self._training_state()]
                host = (self.fD._host_steps, self.fG._host_steps)
                # torch's generator on this device (the noise, the gradient penalty's interpolation weights and the dropout
                # of the double-backward route draw from it): the warm-up's draws are taken back as well
                rng = torch.cuda.get_rng_state(self.dev) if self.dev.type == "cuda" else None
            for _ in range(warmup):
                self._eager(kind)
            if warmup:
                for t, v in zip(self._training_state(), saved):
                    t.copy_(v)
                self.fD._host_steps, self.fG._host_steps = host
                if rng is not None:
                    torch.cuda.synchronize(self.dev)
                    torch.cuda.set_rng_state(rng, self.dev)
                self._refresh_packed(self.D)
                self._refresh_packed(self.G)
        torch.cuda.current_stream(self.dev).wait_stream(s)
        torch.cuda.synchronize(self.dev)
        graphs = []
        # one graph per segment between collectives; without a process group the whole iteration is one graph
        if self.graph_collectives:
            if torch.distributed.get_backend(self.pg) != "nccl":
                raise RuntimeError("graph_collectives needs an nccl (RCCL) process group: only its collectives are stream operations")
            reduce = lambda flat: (lambda: self._allreduce(flat))
            groups = [[f for seg, flat in self._segments(kind) for f in ((seg,) if flat is None else (seg, reduce(flat)))]]
        elif self._split():
            groups = [(seg,) for seg, _ in self._segments(kind, joined=True)]
        else:   # (D and G segments in ONE graph: the branch may stay open across them)
            groups = [[seg for seg, _ in self._segments(kind)]]
        for segs in groups:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, pool=self._pool):
                for seg in segs:
                    seg()
            self._pool = g.pool()
            graphs.append(g)
        if kind == "DG":
            self._graphs = graphs
        else:
            self._alone_graphs[kind] = graphs
        if self.loader is not None:
            self.loader._captured = True

    def _split(self) -> bool:   # the gradient all-reduces are ordinary calls between the graphs of a batch
        return (self.world > 1 or self.pg is not None or self.split_graphs) and not self.graph_collectives

    def set_batch(self, data: torch.Tensor, labels: torch.Tensor):
        if self.loader is not None:
            raise RuntimeError("set_batch: this step takes its batches from the attached DeviceJetLoader, whose feed launch "
                               "overwrites these buffers at the top of every iteration; build the step without a loader to "
                               "set batches by hand")
        self.data.copy_(data, non_blocking=True)
        self.labels.copy_(labels, non_blocking=True)
        self._dcat[:self.B].copy_(self.data)
        self._x3[:self.B].copy_(self.data[..., :3])
        self._mask2[:self.B].copy_(self.data[..., 3:] + 0.5)
        self._ign2[:self.B].copy_(0.5 - self.data[..., 3])
        self._labels2[:self.B].copy_(self.labels)
        self._labels2[self.B:].copy_(self.labels)

    def sync_external_writes(self):
        """Parameters written from outside since the last step -- ``load_state_dict`` of a checkpoint (resume,
        setup_training.py:1406-1416), an in-place edit -- went into the flat buffer (the parameters are views of it), but
        the layers' packed weight images are only rebuilt behind an optimiser step, inside the captured segments: rebuild
        them now, eagerly.  Called by ``step``; cheap when nothing changed (one pass over the version counters)."""
        seen = (self.fD.versions(), self.fG.versions())
        if seen != self._seen_versions:
            if self.dev.type == "cuda":
                self._refresh_packed(self.D)
                self._refresh_packed(self.G)
            self._seen_versions = seen

    def ema_generator(self) -> nn.Module:
        """The averaged generator as a module of G's class with G's state-dict keys, in eval mode: its trained parameters are
        views into ``fG.ema``, everything else (buffers; frozen parameters: spectral norm's u / v, batch norm's running
        statistics) is copied from G by every call, and its packed weight images are rebuilt by every call -- the optimizer
        launch writes the average behind autograd's back.  Take it for ``gen.JetSampler``, ``gen.generate_jets``,
        ``evaluation.evaluate_generator`` and ``checkpoint.save_models(..., G_ema=)``.  The twin is built once and every call
        returns the same object; it does not synchronise.  Once further steps have run, call it AGAIN before sampling: the
        parameters follow by themselves, the weight images only through this call."""
        if self.fG.ema is None:
            raise RuntimeError("TrainStep was built without ema")
        fG = self.fG
        if self._ema_twin is None:
            twin = copy.deepcopy(self.G)
            ps = list(twin.parameters())
            for (off, k, shape), i in zip(fG._spans, fG._trained_idx):
                ps[i].data = fG.ema[off:off + k].view(shape)
                ps[i].grad = None
            self._ema_twin = twin
        twin = self._ema_twin
        with torch.no_grad():
            for dst, src in zip(twin.buffers(), self.G.buffers()):
                dst.copy_(src)
            for dst, src in zip(twin.parameters(), self.G.parameters()):
                if not src.requires_grad:
                    dst.copy_(src)
        twin.eval()
        if self.dev.type == "cuda":
            self._refresh_packed(twin)
        return twin

    def check_range(self):
        """Raise ``FloatingPointError`` if the run has left the numeric range of the fused path (fp16 operands
        with power-of-two scales): a weight image overflowed or a weight / loss is no longer finite.  Synchronises -- call it
        once per epoch, next to the reference's loss logging (train.py:526-540), not per iteration."""
        import math
        st = ops.range_status(self.dev)
        losses = (float(self.D_loss), float(self.G_loss))
        if st or not all(math.isfinite(v) for v in losses):
            raise FloatingPointError(
                f"mpgan_amd: outside the fused path's numeric range (guard word {st}: 1 = |weight x operand scale| > 65504 in an "
                f"fp16 image, 2 = non-finite weight; losses D {losses[0]}, G {losses[1]})")

    @property
    def batch_ndx(self) -> int:
        """The reference's ``batch_ndx`` (train.py:829) of the batch the next ``step()`` is: steps since ``start_epoch``."""
        return self._schedule.batch_ndx

    @batch_ndx.setter
    def batch_ndx(self, b: int):
        self._schedule.batch_ndx = int(b)

    def start_epoch(self):
        """Where the reference's ``for batch_ndx, data in enumerate(...)`` begins (train.py:829): the schedule restarts -- batch
        0 trains D whatever ``num_gen`` is, and G only with ``num_critic`` = 1 -- and so do the epoch's loss sums (train.py:940-941).
        With ``num_critic = num_gen = 1`` every batch runs both and nothing depends on the index."""
        self.batch_ndx = 0
        self._epoch_steps = 0
        if self.epoch_sums is not None:
            for t in self.epoch_sums.values():
                t.zero_()

    def epoch_losses(self, reset: bool = True) -> dict:
        """{"D", "gp", "G"}: the sums of the losses of the ``step()`` calls since ``start_epoch`` (or the last reset), divided as
        the reference's epoch log divides them (train.py:960-962): the D side by steps / num_gen, G by steps / num_critic --
        not by how often each ran (batch 0 and the schedule's phase make those differ).  Reads the sums: the one
        synchronisation of ``track_epoch_losses``."""
        if self.epoch_sums is None:
            raise RuntimeError("TrainStep was built without track_epoch_losses")
        n = self._epoch_steps
        if n == 0:
            raise RuntimeError("epoch_losses: no step() since the sums were last reset")
        sums = dict(zip(self.epoch_sums, torch.stack(list(self.epoch_sums.values())).tolist()))
        out = {"D": sums["D"] / (n / self.num_gen), "gp": sums["gp"] / (n / self.num_gen), "G": sums["G"] / (n / self.num_critic)}
        if reset:
            self._epoch_steps = 0
            for t in self.epoch_sums.values():
                t.zero_()
        return out

    def step(self):
        """One batch of the reference's epoch loop (train.py:829-878): train_D and / or train_G as ``num_critic`` / ``num_gen``
        say for ``batch_ndx``, which it moves on."""
        self.sync_external_writes()
        kind = self._kind(self.batch_ndx)
        if not self.use_graphs:
            self._eager(kind)
        else:
            graphs = self._graphs if kind == "DG" else self._alone_graphs.get(kind)
            if graphs is None:
                self.capture(kind=kind)
                graphs = self._graphs if kind == "DG" else self._alone_graphs[kind]
            if len(graphs) == 1:
                graphs[0].replay()
            else:   # (the gradient all-reduces between the segments' graphs)
                for g, (_, flat) in zip(graphs, self._segments(kind)):
                    g.replay()
                    if flat is not None:
                        self._allreduce(flat)
            for net in self.KINDS[kind]:     # (only the networks this replay stepped)
                (self.fD if net == "D" else self.fG).note_step()
        self.last_ran = self.KINDS[kind]
        self.batch_ndx += 1
        self._epoch_steps += 1

    # -- optimiser state in the reference's checkpoint format (train.py:534-535, setup_training.py:1525-1535) -----
    def optimizer_state_dicts(self):
        """(D_optimizer.state_dict(), G_optimizer.state_dict()) as the reference's ``save_models`` stores them."""
        return self.fD.state_dict(self.lr_disc), self.fG.state_dict(self.lr_gen)

    def load_optimizer_state_dicts(self, sd_D: dict, sd_G: dict):
        self.fD.load_state_dict(sd_D)
        self.fG.load_state_dict(sd_G)
