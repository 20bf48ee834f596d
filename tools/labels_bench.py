"""What label smoothing / label noise cost next to the default iteration, on one GPU.  One JSON object per line on stdout and in
--out.

    python tools/labels_bench.py [--reps 10] [--out profiles/labels_bench.jsonl]

MPGAN at N = 30, B = 256, the captured iteration, one process.  Two steps over the same weights and batch: the default
``TrainStep`` and ``TrainStep(label_smoothing=True, label_noise=0.1)``, whose D segment holds one more launch
(``mpg_label_targets``) and whose head reads its targets from memory.  Rows:

(a) default_step        one ``step()`` of the default step
(b) labels_step         one ``step()`` of the step with both options on
(c) label_launch        ``ops.label_targets`` for the same B on its own, outside any graph

Every ``step()`` and every launch of (c) sits between two HIP events of its own -- in all rows alike, so that what an event pair
costs cancels between them.  A repetition is --batches steps of each kind taken alternately, then as many launches of (c); the
rows are the means within a repetition, reported as median / min / max over --reps repetitions behind a warm-up that captures
both graphs.  No speed claim is made.  The last line states the one condition the options are held to: (b) - (a) is at most the
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
SMOOTHING, NOISE = True, 0.1


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batches", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("labels_bench: no GPU visible (timings are taken on the device or not at all)")
    sink = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()
    torch.manual_seed(0)
    plain, labelled = build(), build(label_smoothing=SMOOTHING, label_noise=NOISE)
    assert labelled.labels_on and not plain.labels_on
    out = tuple(torch.empty(k, device="cuda") for k in (2 * B, 1, 2 * B))
    launch = lambda: ops.label_targets(B, SMOOTHING, NOISE, "cuda", out=out)
    for _ in range(3):                  # warm-up: captures both graphs, loads the label kernel
        plain.step()
        labelled.step()
        launch()
    torch.cuda.synchronize()
    us = {"a default_step": [], "b labels_step": [], "c label_launch": []}
    for _ in range(args.reps):
        a, b = [], []
        for _ in range(args.batches):   # (alternated: the rows share whatever the box does meanwhile)
            a.append(timed(plain.step))
            b.append(timed(labelled.step))
        c = [timed(launch) for _ in range(args.batches)]
        us["a default_step"].append(float(np.mean(a)))
        us["b labels_step"].append(float(np.mean(b)))
        us["c label_launch"].append(float(np.mean(c)))
    med = {}
    for name, v in us.items():
        med[name] = float(np.median(v))
        emit({"model": "mpgan", "B": B, "N": N, "label_smoothing": SMOOTHING, "label_noise": NOISE, "row": name, "reps": args.reps,
              "batches_per_rep": args.batches, "median_us": med[name], "min_us": float(np.min(v)), "max_us": float(np.max(v))})
    diff = med["b labels_step"] - med["a default_step"]
    spread = float(np.max(us["a default_step"]) - np.min(us["a default_step"]))
    emit({"model": "mpgan", "B": B, "row": "condition", "labels_minus_default_us": diff, "spread_default_us": spread,
          "label_launch_us": med["c label_launch"], "within_spread_plus_launch": bool(diff <= spread + med["c label_launch"]),
          "D_loss": float(labelled.D_loss), "G_loss": float(labelled.G_loss), "label_extra": float(labelled.label_extra)})


if __name__ == "__main__":
    main()
