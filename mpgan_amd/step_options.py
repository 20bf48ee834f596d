"""The options of the captured training iteration (``train.TrainStep``) as objects, and the step state that outlives an iteration.

Each option owns its configuration, its device words and its one launch with the CPU statement beside it (the host-logic tests run
toy modules on the CPU): ``Augmenter`` (``--aug-*``), ``AdaController`` (``Augment.adaptive_prob``), ``LabelDraw``
(``--label-smoothing`` / ``--label-noise``), ``StepControl`` (``LrSchedule`` / ``GradClip``: the learning rate and the gradient scale
of an optimizer launch).  ``train`` re-exports the public names.
"""
from __future__ import annotations

from dataclasses import dataclass
from types import SimpleNamespace
from typing import Optional

import torch

from . import ops
from .mpgan import augment as maugment


@dataclass
class Augment:
    """The reference's augmentation switches (``--aug-r90 / --aug-f / --aug-t / --aug-s``, ``--translate-ratio``, ``--scale-sd``,
    ``--aug-prob``; setup_training.py:385-402, its defaults) for ``TrainStep(augment=...)``; the reference's own argument
    namespace has the same field names and is taken as it is.
    ``adaptive_prob`` (``--adaptive-prob``, setup_training.py:399; the reference reads ``augment_p[-1]`` under it and never fills
    it): the probability is moved on the device by ADA's rule (Karras et al. 2020) from D's outputs on the real jets -- every
    ``ada_interval`` D steps by ``B * ada_interval / (1000 * ada_kimg)``, up while the mean sign of (D(real) - midpoint) exceeds
    ``ada_target``, down while it falls short (``ops.ada_update``).  ``aug_prob`` is then the STARTING value: the paper starts at
    0, and that is the usual choice -- the field's default of 1 is the reference's for a fixed probability and is not overridden.
    The three ``ada_*`` fields are ADA's published defaults; a reference namespace lacks them and gets these."""
    aug_r90: bool = False
    aug_f: bool = False
    aug_t: bool = False
    aug_s: bool = False
    translate_ratio: float = 0.125
    scale_sd: float = 0.125
    aug_prob: float = 1.0      # (rand_mix: p == 1 takes nothing)
    adaptive_prob: bool = False
    ada_target: float = 0.6
    ada_interval: int = 4
    ada_kimg: float = 500.0


AUG_SITES = {"D_fake": 0, "G_fake": 1, "D_real": 2}   # ops.augment's sites within an iteration
ADA_DEFAULTS = {f: Augment.__dataclass_fields__[f].default for f in ("ada_target", "ada_interval", "ada_kimg")}


def _f32(v: float) -> float:
    """``v`` rounded to fp32 (to nearest even), as a Python float"""
    return float(torch.tensor(float(v), dtype=torch.float32))


def ada_count_rule(out, n_real: int, mid: float) -> int:
    """``mpg_ada_count`` in Python on a host tensor ``out``: the count of sign(out[:n_real] - mid); a tie or a NaN counts on
    neither side."""
    o, mid = out.detach().reshape(-1)[:n_real].float(), torch.tensor(mid, dtype=torch.float32)
    return int((o > mid).sum()) - int((o < mid).sum())


def ada_settle_rule(s: float, n_real_total: int, target: float, step: float, interval: int, sign_sum: int, steps: int, p: float,
                    r: float):
    """``mpg_ada_settle`` in Python: (sign_sum, steps, p, r) after the D step whose sign count, summed over the ranks, is ``s``.
    ``s`` that is not an integer within [-n_real_total, n_real_total] -- a broken collective -- moves nothing and gives r = NaN.
    The one division and the one sum are torch's fp32 operations on fp32 operands."""
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)
    s = float(s)
    if not (abs(s) <= n_real_total and s == int(s)):      # (a NaN fails the first comparison)
        return sign_sum, steps, p, float("nan")
    target = float(f32(target))
    sign_sum += int(s)
    steps += 1
    if steps != interval:
        return sign_sum, steps, p, r
    r = float(f32(sign_sum) / f32(n_real_total * interval))
    if r > target:
        p = float(f32(p) + f32(step))
    elif r < target:
        p = float(f32(p) - f32(step))
    return 0, 0, min(1.0, max(0.0, p)), r


def ada_rule(out, n_real: int, mid: float, target: float, step: float, interval: int, sign_sum: int, steps: int, p: float, r: float):
    """``mpg_ada_update`` (include/mpgan_amd.h) in Python on a host tensor ``out``: (sign_sum, steps, p, r) after one D step -- its
    two halves, ``ada_count_rule`` and ``ada_settle_rule``, one behind the other.  The CPU path of ``TrainStep`` (host-logic
    tests with toy modules)."""
    return ada_settle_rule(ada_count_rule(out, n_real, mid), n_real, target, step, interval, sign_sum, steps, p, r)


def effective_targets(y_real: torch.Tensor, y_fake: torch.Tensor, smoothing: bool):
    """(t [2B], extra): calc_D_loss's labels ``Y_real`` / ``Y_fake`` (train.py:353-363, after the noise) as ``d_loss`` and the fused
    head take them -- loss = sum_b term(out_b, t_b) / B + extra.  Without smoothing the labels are [B, 1] like D's outputs: t = Y,
    extra = 0.  With smoothing they are [B] and ``MSELoss(out [B, 1], Y [B])`` broadcasts to [B, B] (train.py:369-370):
    mean_ij (out_i - Y_j)^2 = mean_i (out_i - mean(Y))^2 + popvar(Y) per half, so t is each half's mean and extra the two
    population variances.  Any device and dtype."""
    y_real, y_fake = y_real.reshape(-1), y_fake.reshape(-1)
    if not smoothing:
        return torch.cat([y_real, y_fake]), torch.zeros((), device=y_real.device, dtype=y_real.dtype)
    t = torch.cat([y_real.mean().expand(y_real.numel()), y_fake.mean().expand(y_fake.numel())])
    return t, y_real.var(unbiased=False) + y_fake.var(unbiased=False)


# -- step state that outlives an iteration, and the options that own some ------------------------------------------------------
# A carried entry has ``tensors()`` -- the device words an iteration moves: ``TrainStep.capture`` snapshots them before its warm-up
# and puts them back after -- and ``save(group)`` / ``load(group)`` -- its keys in an optimizer file's parameter group (torch.optim's
# own load_state_dict carries unknown group keys along untouched); a missing key loads the entry's default.
# ``FlatParams.carried`` lists the entries that travel with that optimizer's file.  No entry refers back to the TrainStep: a cycle
# would leave the step's hipGraphs to the garbage collector, which may run in the middle of another step's capture.

class DeviceWords:
    """Carried device words that no optimizer file holds: the epoch's loss sums, the loader's cursor (the loader has a
    ``state_dict`` of its own)."""

    def __init__(self, tensors):
        self._tensors = list(tensors)

    def tensors(self):
        return self._tensors

    def save(self, group: dict):
        pass

    def load(self, group: dict):
        pass


class SeedState(DeviceWords):
    """The dropout / noise seed of ``device`` and this process's rank in the data-parallel group, in G's file."""
    KEY, RANK_KEY = "mpgan_amd_seed", "mpgan_amd_seed_rank"

    def __init__(self, device, rank: int):
        super().__init__([ops.seed_tensor(device)])
        self.device, self.rank = device, rank

    def save(self, group):
        group[self.KEY] = ops.get_seed(self.device)
        group[self.RANK_KEY] = int(self.rank)

    def load(self, group):
        if self.KEY in group:    # (a file without the field leaves the seed alone)
            # a resumed run goes on with the noise / dropout stream where the saved one stopped, not from its start -- on the rank
            # that wrote the file.  The reference's checkpoint is ONE file per epoch (train.py:534-535): every other rank of a
            # resumed data-parallel run moves the saved value by its distance in rank (ops.rerank_seed), so that no two ranks
            # share noise or masks behind a resume either.
            ops.set_seed(ops.rerank_seed(int(group[self.KEY]), int(group.get(self.RANK_KEY, 0)), self.rank), self.device)


class Schedule(DeviceWords):
    """``batch_ndx`` of the num_critic / num_gen schedule -- a host integer -- in G's file."""
    KEY = "mpgan_amd_batch_ndx"

    def __init__(self):
        super().__init__([])
        self.batch_ndx = 0

    def save(self, group):
        group[self.KEY] = int(self.batch_ndx)

    def load(self, group):    # (a file without the field -- the reference's, an older one -- resumes at the top of an epoch)
        self.batch_ndx = int(group.get(self.KEY, 0))


class Ema:
    """The averaged generator of ``TrainStep(ema=...)``: an exponential moving average of G's weights, folded inside G's optimizer
    launch (``mpg_*_ema``; include/mpgan_amd.h states the rule).  Exactly one of ``beta`` -- the decay per G
    step, in [0, 1) -- and ``kimg`` -- StyleGAN's parametrisation: the average's half-life in thousands of jets,
    ``beta = 0.5 ** (jets per G step / (1000 * kimg))``, computed once on the host in fp64 and rounded to fp32 (``beta_for``).
    ``start``: G steps before averaging begins -- until then the average follows the weights.  ``warmup``: the decay ramps up as
    ``min(beta, (1 + k) / (10 + k))`` over the k averaged steps so far, so that the early average forgets the starting weights."""

    def __init__(self, beta: Optional[float] = None, kimg: Optional[float] = None, start: int = 0, warmup: bool = False):
        if (beta is None) == (kimg is None):
            raise ValueError(f"Ema: give exactly one of beta and kimg, got beta = {beta!r}, kimg = {kimg!r}")
        if beta is not None and (isinstance(beta, bool) or not 0.0 <= float(beta) < 1.0):      # (a NaN fails both comparisons)
            raise ValueError(f"Ema: beta must lie in [0, 1), got {beta!r}")
        if kimg is not None and (isinstance(kimg, bool) or not float(kimg) > 0.0):
            raise ValueError(f"Ema: kimg must be > 0, got {kimg!r}")
        if isinstance(start, bool) or not isinstance(start, int) or not 0 <= start <= 0x7FFFFFFF:
            raise ValueError(f"Ema: start must be an integer >= 0 (and below 2^31), got {start!r}")
        self.beta = None if beta is None else float(beta)
        self.kimg = None if kimg is None else float(kimg)
        self.start, self.warmup = start, bool(warmup)

    def beta_for(self, batch_size: Optional[int]) -> float:
        """The decay per G step as the kernel takes it: an fp32 value held by a Python float.  ``batch_size``: the jets one G
        step consumes (all ranks together); only ``kimg`` needs it."""
        if self.beta is not None:
            return _f32(self.beta)
        if batch_size is None or batch_size < 1:
            raise ValueError(f"Ema(kimg = {self.kimg}): the decay depends on the batch size, got {batch_size!r}")
        beta = _f32(0.5 ** (batch_size / (1000.0 * self.kimg)))
        if not 0.0 <= beta < 1.0:      # (a half-life so long that the decay rounds to 1 in fp32: the average would never move)
            raise ValueError(f"Ema(kimg = {self.kimg}) at {batch_size} jets per step gives a decay of {beta} in fp32, outside [0, 1)")
        return beta

    def __repr__(self):
        which = f"beta={self.beta}" if self.beta is not None else f"kimg={self.kimg}"
        return f"Ema({which}, start={self.start}, warmup={self.warmup})"


class EmaState(DeviceWords):
    """The averaged generator's state, in G's file: the average itself and its two words (t, ticket) are what an iteration
    moves; the file carries ``{t, beta, start, warmup}`` -- the average's values travel as ``G_ema_<epoch>.pt``
    (``checkpoint.save_models`` / ``load_ema``).  Loading sets the average to the weights as they stand (the loaded ones, after
    ``checkpoint.load_models``) until ``load_ema`` brings the saved average; a file without the key also restarts t at 0.
    ``beta``, ``start`` and ``warmup`` are the step's own, as built; the saved ones are a record."""
    KEY = "mpgan_amd_ema"

    def __init__(self, flat: torch.Tensor, ema: torch.Tensor, state: torch.Tensor, beta: float, start: int, warmup: bool):
        super().__init__([ema, state])
        self.flat, self.ema, self.state = flat, ema, state
        self.beta, self.start, self.warmup = beta, start, warmup

    @property
    def t(self) -> int:
        """Averaged G steps counted so far (reads the word: synchronises)."""
        return int(self.state[0].item())

    def restart(self, t: int = 0):
        """The average set to the weights as they stand, the step word to ``t``, the ticket to 0."""
        if not 0 <= int(t) <= 0xFFFFFFFF:
            raise ValueError(f"saved averaged-generator state counts {t} steps: not a 32-bit count")
        self.ema.copy_(self.flat)
        self.state.copy_(torch.tensor([int(t), 0], dtype=torch.int64).to(torch.uint32))

    def save(self, group):
        group[self.KEY] = {"t": self.t, "beta": self.beta, "start": self.start, "warmup": self.warmup}

    def load(self, group):
        ent = group.get(self.KEY)
        self.restart(0 if ent is None else int(ent["t"]))


class AdaController:
    """The adaptive augmentation probability (``Augment.adaptive_prob``), in D's file: one launch behind the D
    step's head (``update``) adds the signs of D(real) - mid to ``state`` = (sign sum, D steps counted) and, every ``interval`` D
    steps, moves ``p`` -- the augmenter's own probability word -- by ``step`` and leaves the interval's r in ``r``: all in device
    memory, inside the capture.
    Data-parallel ranks (``split``) settle ONE p: ``update`` is then the count launch alone, which stores this rank's sign count
    into ``slot`` -- the float at the tail of D's flat gradient buffer, so D's gradient all-reduce adds the ranks' counts -- and
    ``settle``, first in the segment behind that all-reduce, runs the rule on the sum with ``n_total`` real jets per D step."""
    KEY = "mpgan_amd_ada"

    def __init__(self, p: torch.Tensor, mid: float, target: float, interval: int, step: float, n_total: Optional[int] = None,
                 slot: Optional[torch.Tensor] = None):
        self.mid, self.target, self.interval, self.step = mid, target, interval, step
        self.p, self.p0 = p, float(p)
        self.state = torch.zeros(2, device=p.device, dtype=torch.int32)
        self.r = torch.zeros(1, device=p.device)
        self.split, self.slot, self.n_total = slot is not None, slot, n_total      # (the slot is transient: not carried, not saved)
        self.keep_out = False    # tests: keep the D step's last ``out`` tensor in ``last_out`` (no launch of its own)
        self.last_out = None

    @staticmethod
    def splits(augment, process_group, world_size: int, split: bool = False) -> bool:
        """Does the controller ``augment`` asks for take the two-launch route?  With a process group of more than one rank, or
        when forced (tests, the bench); one rank keeps the one launch."""
        return bool(getattr(augment, "adaptive_prob", False)) and (bool(split) or (process_group is not None and world_size > 1))

    @classmethod
    def from_args(cls, augment, p: torch.Tensor, loss: str, batch_size: int, world_size: int, process_group=None,
                  split: bool = False, slot: Optional[torch.Tensor] = None):
        """The controller ``augment`` (an ``Augment`` or the reference's namespace) asks for, or None.  ``slot``: the tail of D's
        flat gradient buffer on the split route (``splits``; a float of its own when none is given)."""
        if not getattr(augment, "adaptive_prob", False):
            return None
        if world_size > 1 and process_group is None:
            raise ValueError(f"adaptive_prob with world_size = {world_size} and no process group: every rank would settle the "
                             "probability from its own batches and the ranks would drift apart (there is nothing to all-reduce "
                             "the sign sum over); pass the ranks' process_group")
        target, interval, kimg = (getattr(augment, k, v) for k, v in ADA_DEFAULTS.items())
        if isinstance(interval, bool) or not isinstance(interval, int) or interval < 1:
            raise ValueError(f"ada_interval must be an integer >= 1, got {interval!r}")
        if not 0.0 <= float(target) <= 1.0:
            raise ValueError(f"ada_target must lie in [0, 1], got {target!r}")
        if not float(kimg) > 0.0:
            raise ValueError(f"ada_kimg must be > 0, got {kimg!r}")
        n_total = batch_size * world_size      # the real jets of one D step, all ranks together
        if n_total > ops.ADA_COUNT_MAX:
            raise ValueError(f"adaptive_prob with batch_size * world_size = {n_total} > 2^24: the ranks' sign counts would not add "
                             "exactly in fp32")
        if n_total * interval > 2**31 - 1:
            raise ValueError(f"adaptive_prob: batch_size * world_size * ada_interval = {n_total * interval} does not fit the int32 "
                             "sign sum")
        if cls.splits(augment, process_group, world_size, split):
            slot = torch.zeros(1, device=p.device) if slot is None else slot
        else:
            slot = None
        # mid: the midpoint of the loss's two targets (sigmoid outputs against 1 / 0; raw scores either side of 0);
        # step: p can cross [0, 1] in ada_kimg thousand real jets (of all ranks) -- rounded to fp32 once, here
        return cls(p, 0.5 if loss in ("og", "ls") else 0.0, _f32(target), interval, _f32(n_total * interval / (1000.0 * float(kimg))),
                   n_total, slot)

    def read(self) -> dict:
        """{p, r, sign_sum, steps}; synchronises.  p and r are fp32 values held exactly by the Python floats."""
        s = self.state.tolist()
        return {"p": float(self.p), "r": float(self.r), "sign_sum": int(s[0]), "steps": int(s[1])}

    def write(self, ent: Optional[dict]):
        """Put a saved ``read`` back (None: the starting probability, an empty interval, r = 0)."""
        if ent is None:
            ent = {"p": self.p0, "r": 0.0, "sign_sum": 0, "steps": 0}
        if not 0 <= int(ent["steps"]) < self.interval:
            raise ValueError(f"saved adaptive-augmentation state counts {ent['steps']} D steps into an interval of {self.interval}")
        self.p.fill_(float(ent["p"]))
        self.r.fill_(float(ent["r"]))
        self.state.copy_(torch.tensor([int(ent["sign_sum"]), int(ent["steps"])], dtype=torch.int32))

    def update(self, out: torch.Tensor, n_real: int):
        """The launch behind the D step's head; ``out``: D's outputs, the real half first.  Every augmentation launch that follows
        in stream order reads the new probability.  CPU (host-logic tests with toy modules): ``ada_rule``."""
        if self.keep_out:
            self.last_out = out
        if self.split:      # (the count alone: ``settle`` follows behind D's gradient all-reduce)
            if self.p.is_cuda:
                ops.ada_count(out, n_real, self.mid, self.slot)
            else:
                self.slot.fill_(float(ada_count_rule(out, n_real, self.mid)))
            return
        if self.p.is_cuda:
            ops.ada_update(out, n_real, self.mid, self.target, self.step, self.interval, self.state, self.p, self.r)
            return
        now = self.read()
        sign_sum, steps, p, r = ada_rule(out, n_real, self.mid, self.target, self.step, self.interval, now["sign_sum"], now["steps"],
                                         now["p"], now["r"])
        self.write({"p": p, "r": r, "sign_sum": sign_sum, "steps": steps})

    def settle(self):
        """The split route's second launch, first in the segment behind D's gradient all-reduce: the slot now holds the sign
        count of all ranks.  Every rank computes the same p from it.  CPU: ``ada_settle_rule``."""
        if self.p.is_cuda:
            ops.ada_settle(self.slot, self.n_total, self.target, self.step, self.interval, self.state, self.p, self.r)
            return
        now = self.read()
        sign_sum, steps, p, r = ada_settle_rule(float(self.slot), self.n_total, self.target, self.step, self.interval, now["sign_sum"],
                                                now["steps"], now["p"], now["r"])
        self.write({"p": p, "r": r, "sign_sum": sign_sum, "steps": steps})

    def tensors(self):    # (the warm-up's D steps move neither the probability nor the open interval)
        return [self.p, self.state, self.r]

    def save(self, group):
        group[self.KEY] = self.read()

    def load(self, group):    # (a file without the field resumes at the starting probability with an empty interval)
        self.write(group.get(self.KEY))


class Augmenter:
    """Jet augmentation (train.py:438-442, :508-511): one affine map of (eta, phi) per jet, drawn on the device from the seed that
    keys the noise and the dropout masks (``ops.augment``).  The probability ``p`` lives in device memory -- a captured graph
    follows ``TrainStep.set_aug_prob`` and the controller's updates; ``params[site]``: the last maps drawn at each of ``AUG_SITES``."""

    def __init__(self, flags: int, translate_ratio: float, scale_sd: float, p: torch.Tensor, batch_size: int):
        self.flags, self.translate_ratio, self.scale_sd, self.p = flags, float(translate_ratio), float(scale_sd), p
        self.params = [torch.zeros(batch_size, 6, device=p.device) for _ in AUG_SITES]

    @classmethod
    def from_args(cls, augment, p: torch.Tensor, batch_size: int):
        """None with all four switches off: the step without augmentation, launch for launch."""
        flags = ops.augment_flags(augment.aug_r90, augment.aug_f, augment.aug_t, augment.aug_s)
        return cls(flags, augment.translate_ratio, augment.scale_sd, p, batch_size) if flags else None

    def apply(self, x: torch.Tensor, site: int, in_place: bool = False) -> torch.Tensor:
        """``augment.augment(args, x, p)`` at ``site``; on the device with ``ops.AugmentFn``'s backward where ``x`` takes a
        gradient.  CPU (host-logic tests with toy modules): the torch statement with torch's generator."""
        if not self.p.is_cuda:
            args = SimpleNamespace(device=self.p.device, aug_r90=self.flags & ops.AUG_R90, aug_f=self.flags & ops.AUG_FLIP,
                                   aug_t=self.flags & ops.AUG_TRANSLATE, aug_s=self.flags & ops.AUG_SCALE,
                                   translate_ratio=self.translate_ratio, scale_sd=self.scale_sd)
            return maugment.augment(args, x, float(self.p))
        if torch.is_grad_enabled() and x.requires_grad:
            return ops.AugmentFn.apply(x, self.p, self.flags, self.translate_ratio, self.scale_sd, site, self.params[site])
        return ops.augment(x, self.p, self.flags, self.translate_ratio, self.scale_sd, site, out=x if in_place else None,
                           params=self.params[site])[0]


class LabelDraw:
    """Label smoothing / label noise of calc_D_loss (train.py:353-363, ``--label-smoothing`` / ``--label-noise``): the D step's
    per-jet targets, drawn by one small launch in front of the head (``ops.label_targets``) from the seed that keys the noise and
    the dropout masks.  ``drawn``: the labels Y of the last D step as drawn; ``targets`` / ``extra``: what the loss made of them
    (``effective_targets``)."""

    def __init__(self, smoothing: bool, noise: float, batch_size: int, dev):
        self.smoothing, self.noise, self.B = smoothing, noise, batch_size
        self.targets = torch.zeros(2 * batch_size, device=dev)
        self.extra = torch.zeros(1, device=dev)
        self.drawn = torch.zeros(2 * batch_size, device=dev)

    @classmethod
    def from_args(cls, loss: str, label_smoothing, label_noise, batch_size: int, dev):
        """None with neither option on, and for ``w`` / ``hinge``, which never look at them (as in the reference): no launch, no
        buffers, the step as it was."""
        if isinstance(label_noise, bool) or not 0.0 <= float(label_noise) <= 1.0:
            raise ValueError(f"label_noise is a probability in [0, 1], got {label_noise!r}")
        if label_smoothing and loss == "og":
            raise ValueError("label_smoothing with loss = 'og': the reference draws the smoothed labels with shape [B] "
                             "(train.py:354-355) and its nn.BCELoss refuses them against outputs [B, 1] (\"Using a target size ... "
                             "that is different to the input size\", train.py:366); smoothing runs with loss = 'ls' only")
        on = loss in ("og", "ls") and (bool(label_smoothing) or float(label_noise) > 0.0)
        return cls(bool(label_smoothing), float(label_noise), batch_size, dev) if on else None

    def draw(self):
        """calc_D_loss's ``Y_real`` / ``Y_fake`` of this D step into the three buffers.  CPU (host-logic tests with toy modules):
        the reference's own four calls in its order, from torch's generator."""
        B = self.B
        if self.targets.is_cuda:
            ops.label_targets(B, self.smoothing, self.noise, self.targets.device, out=(self.targets, self.extra, self.drawn))
            return
        if self.smoothing:
            y_real = torch.empty(B).uniform_(0.7, 1.2)
            y_fake = torch.empty(B).uniform_(0.0, 0.3)
        else:
            y_real, y_fake = torch.ones(B), torch.zeros(B)
        if self.noise:
            y_real[torch.rand(B) < self.noise] = 0
            y_fake[torch.rand(B) < self.noise] = 1
        t, extra = effective_targets(y_real, y_fake, self.smoothing)
        self.targets.copy_(t)
        self.extra.copy_(extra.reshape(1))
        self.drawn.copy_(torch.cat([y_real, y_fake]))


# -- the optimizer-step control: learning-rate schedule and gradient clipping on the device ------------------------------------
LR_KNOTS = 8                 # MPG_LR_KNOTS of include/mpgan_amd.h
LR_KNOT_STEP_MAX = 1 << 24   # (knot steps convert to fp32 exactly up to here)


class LrSchedule:
    """The learning-rate schedule of ``TrainStep(lr_schedule=...)``: up to 8 knots ``(step, factor)``, the factor multiplying the
    base learning rate; constant before the first and behind the last knot, linear in between (include/mpgan_amd.h states the
    rule).  ``step`` counts that optimizer's own steps -- D steps for D, G steps for G.  Steps: integers,
    strictly increasing, in [0, 2^24]; factors: finite and >= 0, held as fp32.  No knots: the factor is 1.  Cosine or exponential
    shapes are approximated by knots: the rule stays one division and three fp32 operations with a bit-exact host twin."""

    def __init__(self, knots=()):
        knots = list(knots)
        if len(knots) > LR_KNOTS:
            raise ValueError(f"LrSchedule: at most {LR_KNOTS} knots, got {len(knots)}")
        out, last = [], -1
        for kn in knots:
            try:
                step, f = kn
            except (TypeError, ValueError):
                raise ValueError(f"LrSchedule: a knot is a (step, factor) pair, got {kn!r}") from None
            if isinstance(step, bool) or not isinstance(step, int) or not 0 <= step <= LR_KNOT_STEP_MAX:
                raise ValueError(f"LrSchedule: a knot's step must be an integer in [0, 2^24], got {step!r}")
            if step <= last:
                raise ValueError(f"LrSchedule: knot steps must be strictly increasing, got {step!r} behind {last!r}")
            if isinstance(f, bool) or not (0.0 <= float(f) < float("inf")):      # (a NaN fails both comparisons)
                raise ValueError(f"LrSchedule: a knot's factor must be finite and >= 0, got {f!r}")
            if not _f32(f) < float("inf"):
                raise ValueError(f"LrSchedule: a knot's factor must be finite in fp32, got {f!r}")
            out.append((step, _f32(f)))
            last = step
        self.knots = tuple(out)

    @classmethod
    def warmup(cls, steps: int):
        """A linear ramp from 0 to 1 over the first ``steps`` steps, 1 from then on."""
        if isinstance(steps, bool) or not isinstance(steps, int) or steps < 1:
            raise ValueError(f"LrSchedule.warmup: steps must be an integer >= 1, got {steps!r}")
        return cls([(0, 0.0), (steps, 1.0)])

    @classmethod
    def warmup_decay(cls, warmup: int, hold_until: int, end: int, final: float = 0.0):
        """A linear ramp from 0 to 1 over ``warmup`` steps (0: none), 1 until step ``hold_until``, a linear decay to ``final`` at step
        ``end``, ``final`` from then on."""
        for name, v in (("warmup", warmup), ("hold_until", hold_until), ("end", end)):
            if isinstance(v, bool) or not isinstance(v, int) or v < 0:
                raise ValueError(f"LrSchedule.warmup_decay: {name} must be an integer >= 0, got {v!r}")
        if not warmup <= hold_until < end:
            raise ValueError(f"LrSchedule.warmup_decay: needs warmup <= hold_until < end, got {warmup!r}, {hold_until!r}, {end!r}")
        knots = [(0, 0.0), (warmup, 1.0)] if warmup else [(0, 1.0)]
        if hold_until > warmup:
            knots.append((hold_until, 1.0))
        return cls(knots + [(end, final)])

    def factor(self, t: int) -> float:
        """The factor at step ``t`` as the kernel computes it (fp32 operations, one rounding each), held by a Python float."""
        f32 = lambda v: torch.tensor(v, dtype=torch.float32)
        ks = self.knots
        if not ks:
            return 1.0
        if t <= ks[0][0]:
            return ks[0][1]
        if t >= ks[-1][0]:
            return ks[-1][1]
        k = max(i for i in range(len(ks) - 1) if ks[i][0] <= t)
        w = f32(float(t - ks[k][0])) / f32(float(ks[k + 1][0] - ks[k][0]))
        return float(f32(ks[k][1]) + w * (f32(ks[k + 1][1]) - f32(ks[k][1])))

    def __repr__(self):
        return f"LrSchedule({list(self.knots)})"


class GradClip:
    """Gradient clipping of ``TrainStep(grad_clip=...)``: ``torch.nn.utils.clip_grad_norm_`` with the L2 norm over all of a
    network's gradients (averaged over the data-parallel ranks), as a factor on the optimizer launch's ``gscale``.
    ``max_norm > 0`` clips; ``GradClip(None)`` clips nothing and turns the norm's read-out on (``TrainStep.step_control``)."""

    def __init__(self, max_norm: Optional[float] = None):
        if max_norm is not None and (isinstance(max_norm, bool) or not 0.0 < float(max_norm) < float("inf")):
            raise ValueError(f"GradClip: max_norm must be finite and > 0 (or None for the norm's read-out alone), got {max_norm!r}")
        self.max_norm = None if max_norm is None else _f32(max_norm)
        if self.max_norm is not None and not 0.0 < self.max_norm < float("inf"):
            raise ValueError(f"GradClip: max_norm must be finite and > 0 in fp32, got {max_norm!r}")

    def __repr__(self):
        return f"GradClip({self.max_norm})"


class StepControl(DeviceWords):
    """One optimizer's step control (``mpg_step_control``; include/mpgan_amd.h states the rule), in that optimizer's file: the
    words an iteration moves are ``state`` = (t, ticket), ``base`` -- the base learning rate, which ``set_base`` writes -- and
    ``out`` = (lr_eff, s, norm, factor), which the ``mpg_*_ctl`` optimizer launch reads.  The file carries
    ``{t, base, knots, max_norm}``; the knots and ``max_norm`` are the step's own, as built, and the saved ones a record.  A file
    without the key -- the reference's -- resumes the schedule where its optimizer stands: t = the loaded step count
    (``loaded_steps``, which ``FlatParams.load_state_dict`` sets first)."""
    KEY = "mpgan_amd_step_ctl"

    def __init__(self, base: float, schedule: Optional[LrSchedule] = None, clip: Optional[GradClip] = None, device="cpu"):
        from . import _lib
        if schedule is not None and not isinstance(schedule, LrSchedule):
            raise TypeError(f"lr_schedule must be a step_options.LrSchedule, got {type(schedule).__name__}")
        if clip is not None and not isinstance(clip, GradClip):
            raise TypeError(f"grad_clip must be a step_options.GradClip, got {type(clip).__name__}")
        if isinstance(base, bool) or not 0.0 <= float(base) < float("inf"):
            raise ValueError(f"the base learning rate must be finite and >= 0, got {base!r}")
        dev = torch.device(device)
        self.state = torch.zeros(2, device=dev, dtype=torch.uint32)
        self.base = torch.full((1,), float(base), device=dev)
        self.out = torch.zeros(4, device=dev)
        self.out[0], self.out[3] = float(base), 1.0       # (what a read before the first step shows)
        self.partials = torch.zeros(256, device=dev, dtype=torch.float64)     # scratch of the launch: not carried
        super().__init__([self.state, self.base, self.out])
        self.knots = () if schedule is None else schedule.knots
        self.max_norm = None if clip is None else clip.max_norm
        self.want_norm = clip is not None
        self.loaded_steps = 0
        b = _lib.MpgStepCtl()
        b.state, b.base, b.out, b.partials = (t.data_ptr() for t in (self.state, self.base, self.out, self.partials))
        b.nknots = len(self.knots)
        for k, (step, f) in enumerate(self.knots):
            b.knot_step[k], b.knot_f[k] = step, f
        b.max_norm = 0.0 if self.max_norm is None else self.max_norm
        b.want_norm = int(self.want_norm)
        self.block = b

    def launch(self, grad: torch.Tensor, gscale: float):
        """The launch in front of the optimizer launch, on the current stream; ``grad``: the network's n gradients.  Host tensors:
        ``mpg_step_control_host``, the same body."""
        import ctypes as C
        from . import _lib
        g = C.c_void_p(grad.data_ptr())
        if self.state.is_cuda:
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            _lib.check(_lib.lib().mpg_step_control(g, grad.numel(), gscale, C.byref(self.block), st), "mpg_step_control")
        else:
            _lib.check(_lib.lib().mpg_step_control_host(g, grad.numel(), gscale, C.byref(self.block)), "mpg_step_control_host")

    @property
    def t(self) -> int:
        """Controlled steps taken so far (reads the word: synchronises)."""
        return int(self.state[0].item())

    def set_t(self, t: int):
        if not 0 <= int(t) <= 0xFFFFFFFF:
            raise ValueError(f"saved step-control state counts {t} steps: not a 32-bit count")
        self.state.copy_(torch.tensor([int(t), 0], dtype=torch.int64).to(torch.uint32))

    def set_base(self, lr: float):
        """The base learning rate from the next step on, written on the current stream: a captured graph reads it from device
        memory."""
        if isinstance(lr, bool) or not 0.0 <= float(lr) < float("inf"):
            raise ValueError(f"the base learning rate must be finite and >= 0, got {lr!r}")
        self.base.fill_(float(lr))

    def gmul(self, norm: float) -> float:
        """The clipping factor the rule makes of an fp32 ``norm`` (fp32 operations, one rounding each)."""
        if self.max_norm is None:
            return 1.0
        f32 = lambda v: torch.tensor(v, dtype=torch.float32)
        q = f32(self.max_norm) / (f32(norm) + f32(1e-6))
        return 1.0 if float(q) > 1.0 else float(q)

    def next_lr(self) -> float:
        """The learning rate of the step about to be taken, base * factor(t) in fp32 -- where a ``torch.optim.lr_scheduler`` leaves
        ``param_groups[0]["lr"]`` between steps.  Synchronises."""
        f32 = lambda v: torch.tensor(v, dtype=torch.float32)
        return float(f32(float(self.base)) * f32(LrSchedule(self.knots).factor(self.t)))

    def read(self) -> dict:
        """{t, lr, factor, norm, clip}: the steps taken, and the last step's effective learning rate, schedule factor, gradient
        norm (0 when none is computed) and clipping factor.  Synchronises."""
        lr_eff, _, norm, factor = self.out.tolist()
        return {"t": self.t, "lr": lr_eff, "factor": factor, "norm": norm, "clip": self.gmul(norm)}

    def save(self, group):
        group[self.KEY] = {"t": self.t, "base": float(self.base), "knots": [list(k) for k in self.knots], "max_norm": self.max_norm}

    def load(self, group):
        ent = group.get(self.KEY)
        if ent is None:
            self.set_t(self.loaded_steps)
            return
        self.set_t(int(ent["t"]))
        self.set_base(float(ent["base"]))
