"""What the batches of a num_critic schedule cost next to the default iteration, on one GPU.  One JSON object per line on stdout
and in --out.

    python tools/critic_bench.py [--reps 10] [--num-critic 5] [--out profiles/critic_bench.jsonl]

MPGAN at N = 30, B = 256, the captured iteration, one process.  Two steps over the same weights and batch: the default
``TrainStep`` and ``TrainStep(num_critic=5)``.  Rows:

(a) default_step        one ``step()`` of the default step (train_D and train_G)
(b) d_only_replay       one ``step()`` of the scheduled step on a batch where only D trains
(c) dg_replay           one ``step()`` of the scheduled step on a batch where both train -- the launches of (a)
(d) mean_per_batch      two full cycles of the schedule (2 x num_critic batches), per batch

Every ``step()`` sits between two HIP events of its own -- in all rows alike, so that what an event pair costs cancels between
them.  A repetition is two full cycles of the scheduled step and as many default steps, taken alternately; the rows are the means
within a repetition, reported as median / min / max over --reps repetitions behind a warm-up that captures every graph.  No
speed-up is claimed.  The last line states the two conditions the schedule is held to: (c) within the run-to-run spread of (a)
(max - min of (a)'s repetitions), and (b) <= (a).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpgan_amd import data as mdata, train  # noqa: E402

N, B = 30, 256


def build(**kw):
    G, D = train.default_mpgan(N)
    lrs = train.LR["g"]
    ts = train.TrainStep(G, D, B, N, lr_disc=lrs[0], lr_gen=lrs[1], use_graphs=True, **kw)
    x, labels = mdata.synthetic_jets(B, N, seed=1)
    ts.set_batch(x.cuda(), labels.cuda())
    return ts


def timed_step(ts):
    """(what the step ran, microseconds between an event before and an event behind it)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    ts.step()
    b.record()
    b.synchronize()
    return ts.last_ran, 1e3 * a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--num-critic", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("critic_bench: no GPU visible (timings are taken on the device or not at all)")
    sink = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()
    torch.manual_seed(0)
    plain, sched = build(), build(num_critic=args.num_critic)
    cycle = 2 * args.num_critic
    for _ in range(cycle + 1):          # warm-up: captures the three graphs, and leaves the schedule on batch 1 (both train)
        plain.step()
        sched.step()
    torch.cuda.synchronize()
    assert sched.batch_ndx % args.num_critic == 1
    us = {"a default_step": [], "b d_only_replay": [], "c dg_replay": [], "d mean_per_batch": []}
    for _ in range(args.reps):
        a, by_kind = [], {("D",): [], ("D", "G"): []}
        for _ in range(cycle):          # (alternated: the rows share whatever the box does meanwhile)
            a.append(timed_step(plain)[1])
            ran, t = timed_step(sched)
            by_kind[ran].append(t)
        assert len(by_kind[("D", "G")]) == 2 and len(by_kind[("D",)]) == cycle - 2
        us["a default_step"].append(float(np.mean(a)))
        us["b d_only_replay"].append(float(np.mean(by_kind[("D",)])))
        us["c dg_replay"].append(float(np.mean(by_kind[("D", "G")])))
        us["d mean_per_batch"].append(float(np.mean(by_kind[("D",)] + by_kind[("D", "G")])))
    med = {}
    for name, v in us.items():
        med[name] = float(np.median(v))
        emit({"model": "mpgan", "B": B, "N": N, "num_critic": args.num_critic, "row": name, "reps": args.reps, "batches_per_rep": cycle,
              "median_us": med[name], "min_us": float(np.min(v)), "max_us": float(np.max(v))})
    a, d_only, dg = med["a default_step"], med["b d_only_replay"], med["c dg_replay"]
    spread = float(np.max(us["a default_step"]) - np.min(us["a default_step"]))
    emit({"model": "mpgan", "B": B, "num_critic": args.num_critic, "row": "conditions", "dg_minus_default_us": dg - a, "spread_default_us": spread,
          "dg_within_spread_of_default": bool(abs(dg - a) <= spread), "d_only_minus_default_us": d_only - a,
          "d_only_le_default": bool(d_only <= a), "D_loss": float(sched.D_loss), "G_loss": float(sched.G_loss)})


if __name__ == "__main__":
    main()
