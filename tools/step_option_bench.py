"""What one option of the captured training iteration costs next to the step without it, on one GPU.  One JSON object per line on
stdout and in --out.

    python tools/step_option_bench.py --option {labels,ada,critic,sn,ema,ctl,gp} [--model gapt] [--reps 10] [--out profiles/<option>_bench.jsonl]

MPGAN at N = 30, B = 256, the captured iteration, one process.  Two steps over the same weights and batch -- a baseline and the
same with the option on -- and, where the option adds one launch to the D segment, that launch on its own outside any graph:

labels   baseline: the default step.  Option: ``label_smoothing=True, label_noise=0.1`` (+ ``mpg_label_targets``, and the head
         reads its targets from memory).  Rows: a default_step, b labels_step, c label_launch.
ada      three steps: the four augmentations at p = 0.5 (a fixed_p_step), the same with ``adaptive_prob=True`` on the one-launch
         route (b adaptive_step: + ``mpg_ada_update`` behind the head) and on the two-launch route that data-parallel ranks take,
         forced on this one rank (d split_step: + ``mpg_ada_count`` behind the head and ``mpg_ada_settle`` in front of D's
         optimizer launch, one float more in D's gradient buffer).  Lone launches: c ada_launch, e count_launch, f settle_launch.
critic   baseline: the default step.  Option: ``num_critic=5`` (--num-critic).  Rows: a default_step, b d_only_replay (a batch
         on which only D trains), c dg_replay (both train: the launches of a), d mean_per_batch (over two full cycles).
sn       three steps: a default_step (for scale), and spectral norm in G and D with ``ops.OPTIONS["sn_fused"]`` off (b
         sn_unfused_step) and on (c sn_fused_step).  Held to: the median of (c) is not above the median of (b).

ema      baseline: the default step.  Option: ``ema=Ema(kimg=10)`` -- G's optimizer launch also folds the averaged generator; no
         launch is added, so there is no lone launch to time.  Rows: a default_step, b ema_step.

ctl      baseline: the default step.  Option: ``lr_schedule=LrSchedule.warmup_decay(100, 5000, 6000, 0.1), grad_clip=GradClip(1.0)``
         on both networks (+ ``mpg_step_control`` in front of each optimizer launch, which reads its rate and its gradient scale
         from memory).  Rows: a default_step, b ctl_step, c ctl_launch_D, d ctl_launch_G (each network's launch alone, over a
         gradient of that network's size).

gp       two steps with ``loss="w", gp_lambda=10``: the penalty's D(x) on the materialised edge matrix (a gp_step_edges: the
         route ``ops.double_backward_route`` has always taken) and on the twice-differentiable row kernels (b gp_step_rows:
         ``gp_rows=True``), at N = 30, B = 256 and again at N = 150, B = 16.  Held to, per shape: the median of (b) is not above the
         median of (a), measured in the same run.
         ``--model gapt``: the attention discriminator instead, the penalty's attention cores as broadcast products (a gp_step_dd:
         ``MAB._forward_dd`` as it has always run) and on the twice-differentiable attention kernels (b gp_step_attn:
         ``gp_attn=True``), at N = 30, B = 512 and at N = 150, B = 64.  Held to, per shape: the median of (b) is not above the
         median of (a) by more than (a)'s own run-to-run spread (max - min of its repetitions).
         Both models: a third step (c gp_step_rows_chain / c gp_step_attn_chain) adds ``gp_chain=True`` to (b) -- the penalty's
         LinearNets and D's head as one twice-differentiable op each.  Held to, per shape: the median of (c) is not above the
         median of (b) by more than (b)'s own run-to-run spread.

Every ``step()`` and every lone launch sits between two HIP events of its own -- in all rows alike, so that what an event pair
costs cancels between them.  A repetition is --batches steps of each kind (critic: two full cycles of the schedule) taken
alternately, then as many lone launches; the rows are the means within a repetition, reported as median / min / max over --reps
repetitions behind a warm-up that captures every graph.  No speed claim is made.  The last line states what the option is held to.
labels, ada: (b) - (a) is at most the run-to-run spread of (a) (max - min of its repetitions) plus (c); ada also: (d) - (b) is at
most the spread of (b) plus (f) -- the baseline of the split route is the unchanged one-launch route of the same process.  critic: (c) within
the spread of (a), and (b) <= (a).  ema: (b) - (a) is at most the run-to-run spread of (a).  ctl: (b) - (a) is at most the spread of
(a) plus (c) plus (d).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpgan_amd import data as mdata, ops, train  # noqa: E402

N, B = 30, 256
SMOOTHING, NOISE, P0 = True, 0.1, 0.5


def build(**kw):
    G, D = train.default_mpgan(N)
    lrs = train.LR["g"]
    ts = train.TrainStep(G, D, B, N, lr_disc=lrs[0], lr_gen=lrs[1], use_graphs=True, **kw)
    x, labels = mdata.synthetic_jets(B, N, seed=1)
    ts.set_batch(x.cuda(), labels.cuda())
    return ts


def timed(fn):
    """microseconds between an event before and an event behind ``fn()``"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b)


def jsonl_sink(path):
    """emit(record): one JSON line on stdout and, with a path, appended to that file"""
    sink = open(path, "a") if path else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()
    return emit


def _augment(**kw):
    return train.Augment(aug_r90=True, aug_f=True, aug_t=True, aug_s=True, aug_prob=P0, **kw)


def _label_launch(opt):
    out = tuple(torch.empty(k, device="cuda") for k in (2 * B, 1, 2 * B))
    return lambda: ops.label_targets(B, SMOOTHING, NOISE, "cuda", out=out)


def _ada_launch(opt):
    a = opt._ada
    out = torch.rand(2 * B, device="cuda")
    words = (torch.zeros(2, dtype=torch.int32, device="cuda"), torch.full((1,), P0, device="cuda"), torch.zeros(1, device="cuda"))
    return lambda: ops.ada_update(out, B, a.mid, a.target, a.step, a.interval, *words)


def _launch_condition(opt_name, base_name, launch_name):
    """(b) - (a) at most the spread of (a) plus (c), under the field names of the option's earlier lines"""
    def condition(med, us, rows):
        diff = med[rows[1]] - med[rows[0]]
        spread = float(np.max(us[rows[0]]) - np.min(us[rows[0]]))
        return {"row": "condition", f"{opt_name}_minus_{base_name}_us": diff, f"spread_{base_name}_us": spread,
                f"{launch_name}_launch_us": med[rows[2]], "within_spread_plus_launch": bool(diff <= spread + med[rows[2]])}
    return condition


def _critic_condition(med, us, rows):
    a, d_only, dg = (med[r] for r in rows[:3])
    spread = float(np.max(us[rows[0]]) - np.min(us[rows[0]]))
    return {"row": "conditions", "dg_minus_default_us": dg - a, "spread_default_us": spread,
            "dg_within_spread_of_default": bool(abs(dg - a) <= spread), "d_only_minus_default_us": d_only - a,
            "d_only_le_default": bool(d_only <= a)}


def _ema_condition(med, us, rows):
    diff = med[rows[1]] - med[rows[0]]
    spread = float(np.max(us[rows[0]]) - np.min(us[rows[0]]))
    return {"row": "condition", "ema_minus_default_us": diff, "spread_default_us": spread, "within_spread": bool(diff <= spread)}


# option -> baseline step's arguments, option step's arguments, the lone launch (or None), row names, fields of every row, the
# condition line, fields that close the condition line
OPTIONS = {
    "labels": dict(base=lambda a: {}, opt=lambda a: dict(label_smoothing=SMOOTHING, label_noise=NOISE), launch=_label_launch,
                   rows=("a default_step", "b labels_step", "c label_launch"),
                   fields=lambda a, opt: {"label_smoothing": SMOOTHING, "label_noise": NOISE},
                   condition=_launch_condition("labels", "default", "label"), tail=lambda opt: {"label_extra": float(opt.label_extra)}),
    "critic": dict(base=lambda a: {}, opt=lambda a: dict(num_critic=a.num_critic), launch=None,
                   rows=("a default_step", "b d_only_replay", "c dg_replay", "d mean_per_batch"),
                   fields=lambda a, opt: {"num_critic": a.num_critic}, condition=_critic_condition, tail=lambda opt: {}),
    "ema": dict(base=lambda a: {}, opt=lambda a: dict(ema=train.Ema(kimg=10)), launch=None, rows=("a default_step", "b ema_step"),
                fields=lambda a, opt: {"ema_kimg": 10, "ema_beta": opt.fG.ema_carried.beta}, condition=_ema_condition,
                tail=lambda opt: {"ema_t": opt.fG.ema_carried.t}),
}


def ada_bench(args, emit):
    """--option ada: three captured steps in one process -- fixed p, adaptive on the one-launch route, adaptive on the split route
    (``_ada_split=True``: what a rank of several runs, without the all-reduce) -- alternated, every ``step()`` between two HIP
    events; then the three lone launches."""
    rows = ("a fixed_p_step", "b adaptive_step", "d split_step", "c ada_launch", "e count_launch", "f settle_launch")
    torch.manual_seed(0)
    steps = [build(augment=_augment()), build(augment=_augment(adaptive_prob=True)),
             build(augment=_augment(adaptive_prob=True), _ada_split=True)]
    one, split = steps[1], steps[2]
    assert not one._ada.split and split._ada.split and split.fD.grad_all.numel() == split.fD.n + 1
    a = one._ada
    out = torch.rand(2 * B, device="cuda")
    words = (torch.zeros(2, dtype=torch.int32, device="cuda"), torch.full((1,), P0, device="cuda"), torch.zeros(1, device="cuda"))
    slot = torch.zeros(1, device="cuda")
    launches = [_ada_launch(one), lambda: ops.ada_count(out, B, a.mid, slot),
                lambda: ops.ada_settle(slot, B, a.target, a.step, a.interval, *words)]
    for _ in range(3):   # warm-up: captures every graph
        for fn in (*(ts.step for ts in steps), *launches):
            fn()
    torch.cuda.synchronize()
    us = {r: [] for r in rows}
    for _ in range(args.reps):
        t = {r: [] for r in rows}
        for _ in range(args.batches):        # (alternated: the rows share whatever the box does meanwhile)
            for r, ts in zip(rows[:3], steps):
                t[r].append(timed(ts.step))
        for r, fn in zip(rows[3:], launches):
            t[r] = [timed(fn) for _ in range(args.batches)]
        for r in rows:
            us[r].append(float(np.mean(t[r])))
    med = {}
    for name, v in us.items():
        med[name] = float(np.median(v))
        emit({"model": "mpgan", "B": B, "N": N, "aug_prob": P0, "ada_interval": a.interval, "ada_step": a.step, "row": name,
              "reps": args.reps, "batches_per_rep": args.batches, "median_us": med[name], "min_us": float(np.min(v)),
              "max_us": float(np.max(v))})
    emit({"model": "mpgan", "B": B, **_launch_condition("adaptive", "fixed", "ada")(med, us, (rows[0], rows[1], rows[3])),
          "D_loss": float(one.D_loss), "G_loss": float(one.G_loss), "ada": one.ada})
    diff, spread = med[rows[2]] - med[rows[1]], float(np.max(us[rows[1]]) - np.min(us[rows[1]]))
    emit({"model": "mpgan", "B": B, "row": "condition_split", "split_minus_adaptive_us": diff, "spread_adaptive_us": spread,
          "settle_launch_us": med[rows[5]], "count_launch_us": med[rows[4]],
          "within_spread_plus_settle": bool(diff <= spread + med[rows[5]]), "D_loss": float(split.D_loss),
          "G_loss": float(split.G_loss), "ada": split.ada})


def ctl_bench(args, emit):
    """--option ctl: the default step and the step with a schedule and a clip on both networks, alternated, every ``step()`` between
    two HIP events; then each network's ``mpg_step_control`` launch alone, over a gradient of that network's size."""
    from mpgan_amd.step_options import GradClip, LrSchedule, StepControl
    rows = ("a default_step", "b ctl_step", "c ctl_launch_D", "d ctl_launch_G")
    sched, clip = LrSchedule.warmup_decay(100, 5000, 6000, 0.1), GradClip(1.0)
    torch.manual_seed(0)
    base, opt = build(), build(lr_schedule=sched, grad_clip=clip)
    launches = []
    for flat, lr in ((opt.fD, opt.lr_disc), (opt.fG, opt.lr_gen)):
        ctl, g = StepControl(lr, sched, clip, "cuda"), torch.randn(flat.n, device="cuda")
        launches.append(lambda ctl=ctl, g=g: ctl.launch(g, 1.0))
    for _ in range(3):   # warm-up: captures every graph
        for fn in (base.step, opt.step, *launches):
            fn()
    torch.cuda.synchronize()
    us = {r: [] for r in rows}
    for _ in range(args.reps):
        t = {r: [] for r in rows}
        for _ in range(args.batches):        # (alternated: the rows share whatever the box does meanwhile)
            t[rows[0]].append(timed(base.step))
            t[rows[1]].append(timed(opt.step))
        for r, fn in zip(rows[2:], launches):
            t[r] = [timed(fn) for _ in range(args.batches)]
        for r in rows:
            us[r].append(float(np.mean(t[r])))
    med = {}
    for name, v in us.items():
        med[name] = float(np.median(v))
        emit({"model": "mpgan", "B": B, "N": N, "lr_knots": [list(k) for k in sched.knots], "max_norm": clip.max_norm, "n_D": opt.fD.n,
              "n_G": opt.fG.n, "row": name, "reps": args.reps, "batches_per_rep": args.batches, "median_us": med[name],
              "min_us": float(np.min(v)), "max_us": float(np.max(v))})
    diff, spread = med[rows[1]] - med[rows[0]], float(np.max(us[rows[0]]) - np.min(us[rows[0]]))
    emit({"model": "mpgan", "B": B, "row": "condition", "ctl_minus_default_us": diff, "spread_default_us": spread,
          "ctl_launch_D_us": med[rows[2]], "ctl_launch_G_us": med[rows[3]],
          "within_spread_plus_launches": bool(diff <= spread + med[rows[2]] + med[rows[3]]), "D_loss": float(opt.D_loss),
          "G_loss": float(opt.G_loss), "step_control": opt.step_control})


def sn_bench(args, emit):
    """--option sn: three captured steps in one process -- the default step (for scale), and spectral norm in G and D built under
    ``ops.OPTIONS["sn_fused"]`` off (a launch per wrapped layer, MPLayer._forward_edges) and on (one grouped launch per network
    part, the fused edge kernels) -- alternated, every ``step()`` between two HIP events."""
    rows = ("a default_step", "b sn_unfused_step", "c sn_fused_step")
    torch.manual_seed(0)
    steps = []
    for sn, on in ((False, True), (True, False), (True, True)):
        ops.OPTIONS["sn_fused"] = on
        G, D = train.default_mpgan(N, spectral_norm_gen=sn, spectral_norm_disc=sn)
        lrs = train.LR["g"]
        ts = train.TrainStep(G, D, B, N, lr_disc=lrs[0], lr_gen=lrs[1], use_graphs=True)
        x, labels = mdata.synthetic_jets(B, N, seed=1)
        ts.set_batch(x.cuda(), labels.cuda())
        for _ in range(3):   # warm-up: captures the graph, under this leg's switch
            ts.step()
        torch.cuda.synchronize()
        steps.append(ts)
    ops.OPTIONS["sn_fused"] = True
    assert all(l.fused for ts in steps for l in (*ts.G.mp_layers, *ts.D.mp_layers))
    us = {r: [] for r in rows}
    for _ in range(args.reps):
        t = {r: [] for r in rows}
        for _ in range(args.batches):        # (alternated: the rows share whatever the box does meanwhile)
            for r, ts in zip(rows, steps):
                t[r].append(timed(ts.step))
        for r in rows:
            us[r].append(float(np.mean(t[r])))
    med = {}
    for name, v in us.items():
        med[name] = float(np.median(v))
        emit({"model": "mpgan", "B": B, "N": N, "spectral_norm": name != rows[0], "row": name, "reps": args.reps,
              "batches_per_rep": args.batches, "median_us": med[name], "min_us": float(np.min(v)), "max_us": float(np.max(v))})
    emit({"model": "mpgan", "B": B, "row": "condition", "fused_minus_unfused_us": med[rows[2]] - med[rows[1]],
          "fused_le_unfused": bool(med[rows[2]] <= med[rows[1]]),
          **{f"{k}_loss_{r[2:]}": float(getattr(ts, k + "_loss")) for r, ts in zip(rows[1:], steps[1:]) for k in ("D", "G")}})


def gp_bench(args, emit):
    """--option gp: the captured --gp iteration with the penalty on the existing route and on the rows route, alternated in one
    process, every ``step()`` between two HIP events; at the headline shape and at N = 150, B = 16."""
    if args.model == "gapt":
        return gp_attn_bench(args, emit)
    rows = ("a gp_step_edges", "b gp_step_rows", "c gp_step_rows_chain")
    for n, b in ((N, B), (150, 16)):
        torch.manual_seed(0)
        steps = []
        for gp_rows, gp_chain in ((False, False), (True, False), (True, True)):
            G, D = train.default_mpgan(n, loss="w")
            lrs = train.LR["g"]
            ts = train.TrainStep(G, D, b, n, lr_disc=lrs[0], lr_gen=lrs[1], use_graphs=True, loss="w", gp_lambda=10.0, gp_rows=gp_rows,
                                 gp_chain=gp_chain)
            x, labels = mdata.synthetic_jets(b, n, seed=1)
            ts.set_batch(x.cuda(), labels.cuda())
            for _ in range(3):   # warm-up: captures the graph
                ts.step()
            torch.cuda.synchronize()
            steps.append(ts)
        assert all(l.gp_rows_ok(b, n, True, dict(ops.OPTIONS, gp_rows=True)) for l in steps[1].D.mp_layers)
        us = {r: [] for r in rows}
        for _ in range(args.reps):
            t = {r: [] for r in rows}
            for _ in range(args.batches):        # (alternated: the rows share whatever the box does meanwhile)
                for r, ts in zip(rows, steps):
                    t[r].append(timed(ts.step))
            for r in rows:
                us[r].append(float(np.mean(t[r])))
        med = {}
        for name, v in us.items():
            med[name] = float(np.median(v))
            emit({"model": "mpgan", "B": b, "N": n, "loss": "w", "gp_lambda": 10.0, "gp_rows": name != rows[0], "gp_chain": name == rows[2],
                  "row": name, "reps": args.reps, "batches_per_rep": args.batches, "median_us": med[name], "min_us": float(np.min(v)),
                  "max_us": float(np.max(v)), "jets_per_s": b / (med[name] * 1e-6)})
        spread = float(np.max(us[rows[1]]) - np.min(us[rows[1]]))
        emit({"model": "mpgan", "B": b, "N": n, "row": "condition", "rows_minus_edges_us": med[rows[1]] - med[rows[0]],
              "rows_le_edges": bool(med[rows[1]] <= med[rows[0]]),
              "chain_minus_rows_us": med[rows[2]] - med[rows[1]], "spread_rows_us": spread,
              "chain_within_spread_of_rows": bool(med[rows[2]] - med[rows[1]] <= spread),
              **{f"{k}_{r[2:]}": float(getattr(ts, k)) for r, ts in zip(rows, steps) for k in ("D_loss", "GP")}})
        del steps
        torch.cuda.empty_cache()


def gp_attn_bench(args, emit):
    """--option gp --model gapt: the captured --gp iteration of GAPT with the penalty's attention cores on the existing route and on
    the attention kernels, alternated in one process, every ``step()`` between two HIP events; at N = 30, B = 512 and N = 150, B = 64."""
    rows = ("a gp_step_dd", "b gp_step_attn", "c gp_step_attn_chain")
    for n, b in ((30, 512), (150, 64)):
        torch.manual_seed(0)
        steps = []
        for gp_attn, gp_chain in ((False, False), (True, False), (True, True)):
            G, D = train.default_gapt(n)
            lrs = train.LR_GAPT
            ts = train.TrainStep(G, D, b, n, latent=64, lr_disc=lrs[0], lr_gen=lrs[1], use_graphs=True, loss="w", gp_lambda=10.0,
                                 gp_attn=gp_attn, gp_chain=gp_chain)
            x, labels = mdata.synthetic_jets(b, n, seed=1)
            ts.set_batch(x.cuda(), labels.cuda())
            for _ in range(3):   # warm-up: captures the graph
                ts.step()
            torch.cuda.synchronize()
            steps.append(ts)
        us = {r: [] for r in rows}
        for _ in range(args.reps):
            t = {r: [] for r in rows}
            for _ in range(args.batches):        # (alternated: the rows share whatever the box does meanwhile)
                for r, ts in zip(rows, steps):
                    t[r].append(timed(ts.step))
            for r in rows:
                us[r].append(float(np.mean(t[r])))
        med = {}
        for name, v in us.items():
            med[name] = float(np.median(v))
            emit({"model": "gapt", "B": b, "N": n, "loss": "w", "gp_lambda": 10.0, "gp_attn": name != rows[0], "gp_chain": name == rows[2],
                  "row": name, "reps": args.reps, "batches_per_rep": args.batches, "median_us": med[name], "min_us": float(np.min(v)),
                  "max_us": float(np.max(v)), "jets_per_s": b / (med[name] * 1e-6)})
        diff, spread = med[rows[1]] - med[rows[0]], float(np.max(us[rows[0]]) - np.min(us[rows[0]]))
        spread_b = float(np.max(us[rows[1]]) - np.min(us[rows[1]]))
        emit({"model": "gapt", "B": b, "N": n, "row": "condition", "attn_minus_dd_us": diff, "spread_dd_us": spread,
              "attn_within_spread_of_dd": bool(diff <= spread),
              "chain_minus_attn_us": med[rows[2]] - med[rows[1]], "spread_attn_us": spread_b,
              "chain_within_spread_of_attn": bool(med[rows[2]] - med[rows[1]] <= spread_b),
              **{f"{k}_{r[2:]}": float(getattr(ts, k)) for r, ts in zip(rows, steps) for k in ("D_loss", "GP")}})
        del steps
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--option", choices=sorted([*OPTIONS, "ada", "sn", "ctl", "gp"]), required=True)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batches", type=int, default=10, help="steps of each kind per repetition (critic: two cycles of the schedule)")
    ap.add_argument("--num-critic", type=int, default=5)
    ap.add_argument("--model", choices=["mpgan", "gapt"], default="mpgan", help="gapt: with --option gp only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.model != "mpgan" and args.option != "gp":
        raise SystemExit("--model gapt is measured by --option gp only")
    if not torch.cuda.is_available():
        raise SystemExit(f"{args.option}_bench: no GPU visible (timings are taken on the device or not at all)")
    emit = jsonl_sink(args.out)
    if args.option == "sn":
        return sn_bench(args, emit)
    if args.option == "ada":
        return ada_bench(args, emit)
    if args.option == "ctl":
        return ctl_bench(args, emit)
    if args.option == "gp":
        return gp_bench(args, emit)
    o = OPTIONS[args.option]
    critic = args.option == "critic"
    batches = 2 * args.num_critic if critic else args.batches
    torch.manual_seed(0)
    base, opt = build(**o["base"](args)), build(**o["opt"](args))
    launch = o["launch"](opt) if o["launch"] else None
    for _ in range(batches + 1 if critic else 3):   # warm-up: captures every graph (critic: leaves the schedule on batch 1, both train)
        base.step()
        opt.step()
        if launch:
            launch()
    torch.cuda.synchronize()
    assert not critic or opt.batch_ndx % args.num_critic == 1
    rows = o["rows"]
    us = {r: [] for r in rows}
    for _ in range(args.reps):
        ta, by_kind = [], {("D", "G"): [], ("D",): []}
        for _ in range(batches):        # (alternated: the rows share whatever the box does meanwhile)
            ta.append(timed(base.step))
            t = timed(opt.step)
            by_kind[opt.last_ran].append(t)
        us[rows[0]].append(float(np.mean(ta)))
        if critic:
            assert len(by_kind[("D", "G")]) == 2 and len(by_kind[("D",)]) == batches - 2
            for r, ts in zip(rows[1:], (by_kind[("D",)], by_kind[("D", "G")], by_kind[("D",)] + by_kind[("D", "G")])):
                us[r].append(float(np.mean(ts)))
        else:
            us[rows[1]].append(float(np.mean(by_kind[("D", "G")])))
            if launch:
                us[rows[2]].append(float(np.mean([timed(launch) for _ in range(batches)])))
    med = {}
    for name, v in us.items():
        med[name] = float(np.median(v))
        emit({"model": "mpgan", "B": B, "N": N, **o["fields"](args, opt), "row": name, "reps": args.reps, "batches_per_rep": batches,
              "median_us": med[name], "min_us": float(np.min(v)), "max_us": float(np.max(v))})
    emit({"model": "mpgan", "B": B, **({"num_critic": args.num_critic} if critic else {}), **o["condition"](med, us, rows),
          "D_loss": float(opt.D_loss), "G_loss": float(opt.G_loss), **o["tail"](opt)})


if __name__ == "__main__":
    main()
