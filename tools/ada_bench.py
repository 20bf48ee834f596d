"""What the adaptive augmentation probability costs next to the augmenting iteration with a fixed probability, on one GPU.  One
JSON object per line on stdout and in --out.

    python tools/ada_bench.py [--reps 10] [--out profiles/ada_bench.jsonl]

MPGAN at N = 30, B = 256, the captured iteration, one process.  Two steps over the same weights and batch, both with the four
augmentations on at p = 0.5: ``TrainStep(augment=Augment(...))`` and the same with ``adaptive_prob=True``, whose D segment holds one
more launch (``mpg_ada_update``) behind the head.  Rows:

(a) fixed_p_step        one ``step()`` of the augmenting step with a fixed probability
(b) adaptive_step       one ``step()`` of the step whose probability the controller moves
(c) ada_launch          ``ops.ada_update`` for the same B on its own, outside any graph

Every ``step()`` and every launch of (c) sits between two HIP events of its own -- in all rows alike, so that what an event pair
costs cancels between them.  A repetition is --batches steps of each kind taken alternately, then as many launches of (c); the
rows are the means within a repetition, reported as median / min / max over --reps repetitions behind a warm-up that captures
both graphs.  No speed claim is made.  The last line states the one condition the option is held to: (b) - (a) is at most the
run-to-run spread of (a) (max - min of its repetitions) plus (c).
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
P0 = 0.5


def build(**kw):
    G, D = train.default_mpgan(N)
    lrs = train.LR["g"]
    aug = train.Augment(aug_r90=True, aug_f=True, aug_t=True, aug_s=True, aug_prob=P0, **kw)
    ts = train.TrainStep(G, D, B, N, lr_disc=lrs[0], lr_gen=lrs[1], use_graphs=True, augment=aug)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batches", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ada_bench: no GPU visible (timings are taken on the device or not at all)")
    sink = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()
    torch.manual_seed(0)
    fixed, adaptive = build(), build(adaptive_prob=True)
    assert adaptive._ada is not None and fixed._ada is None
    a = adaptive._ada
    out = torch.rand(2 * B, device="cuda")
    words = (torch.zeros(2, dtype=torch.int32, device="cuda"), torch.full((1,), P0, device="cuda"), torch.zeros(1, device="cuda"))
    launch = lambda: ops.ada_update(out, B, a.mid, a.target, a.step, a.interval, *words)
    for _ in range(3):                  # warm-up: captures both graphs, loads the controller's kernel
        fixed.step()
        adaptive.step()
        launch()
    torch.cuda.synchronize()
    us = {"a fixed_p_step": [], "b adaptive_step": [], "c ada_launch": []}
    for _ in range(args.reps):
        ta, tb = [], []
        for _ in range(args.batches):   # (alternated: the rows share whatever the box does meanwhile)
            ta.append(timed(fixed.step))
            tb.append(timed(adaptive.step))
        tc = [timed(launch) for _ in range(args.batches)]
        us["a fixed_p_step"].append(float(np.mean(ta)))
        us["b adaptive_step"].append(float(np.mean(tb)))
        us["c ada_launch"].append(float(np.mean(tc)))
    med = {}
    for name, v in us.items():
        med[name] = float(np.median(v))
        emit({"model": "mpgan", "B": B, "N": N, "aug_prob": P0, "ada_interval": a.interval, "ada_step": a.step, "row": name,
              "reps": args.reps, "batches_per_rep": args.batches, "median_us": med[name], "min_us": float(np.min(v)),
              "max_us": float(np.max(v))})
    diff = med["b adaptive_step"] - med["a fixed_p_step"]
    spread = float(np.max(us["a fixed_p_step"]) - np.min(us["a fixed_p_step"]))
    emit({"model": "mpgan", "B": B, "row": "condition", "adaptive_minus_fixed_us": diff, "spread_fixed_us": spread,
          "ada_launch_us": med["c ada_launch"], "within_spread_plus_launch": bool(diff <= spread + med["c ada_launch"]),
          "D_loss": float(adaptive.D_loss), "G_loss": float(adaptive.G_loss), "ada": adaptive.ada})


if __name__ == "__main__":
    main()
