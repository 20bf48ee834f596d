"""What feeding the training step costs, on one GPU.  One JSON object per line on stdout and in --out.

    python tools/loader_bench.py [--model mpgan|gapt|both] [--reps 10] [--iters 50] [--out profiles/loader_bench.jsonl]

MPGAN at N = 30, B = 256 and GAPT at N = 30, B = 512, the captured iteration, over n = 100 000 synthetic jets
(``data.synthetic_jets``).  Rows, per model:

(a) step_fixed_batch     ``step()`` alone on a batch set once -- the quantity behind bench.py's headline
(b) set_batch_device     ``set_batch`` of a batch that already lies on the device, then ``step()``
(c) dataloader_host      ``DataLoader(JetArrayDataset, shuffle=True)`` -> ``.cuda()`` -> ``set_batch`` -> ``step()``
(d) step_with_loader     ``step()`` with a ``DeviceJetLoader`` attached (the feed launch inside the graph)
    feed_launch          ``mpg_batch_feed`` on its own: --chain launches captured into one graph and replayed, divided by their number

Every row is the time between two HIP events around --iters iterations ((c): --host-iters), divided by their number; the rows are
taken alternately, --reps times in one process behind a warm-up, and reported as median / min / max.  (c) idles the device while
the host collates: the events see that gap, which is the point.  The last line per model states the two conditions the feed is
held to: (d) <= (b), and (d) <= (a) + feed_launch + spread(a), spread(a) = max - min of row (a)'s repetitions.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpgan_amd import data as mdata, train  # noqa: E402

N_JETS, N = 100_000, 30


def build(model, B, loader=None):
    if model == "mpgan":
        G, D = train.default_mpgan(N)
        latent, lrs = 32, train.LR["g"]
    else:
        G, D = train.default_gapt(N)
        latent, lrs = 64, train.LR_GAPT
    return train.TrainStep(G, D, B, N, latent=latent, lr_disc=lrs[0], lr_gen=lrs[1], use_graphs=True, loader=loader)


def raw_jets(x):
    """Normalised synthetic jets back in JetNet's raw range: what ``JetArrayDataset`` takes (and normalises again)."""
    mx = x.new_tensor(mdata.FEATURE_MAXES["g"])
    return (x - x.new_tensor(mdata.FEATURE_SHIFTS)) / x.new_tensor(mdata.FEATURE_NORMS) * mx


def between_events(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / iters


def run(model, B, args, emit):
    torch.manual_seed(0)
    x, labels = mdata.synthetic_jets(N_JETS, N, seed=1)
    ts = build(model, B)                                       # rows (a), (b), (c)
    loader = mdata.DeviceJetLoader((x, labels), B, "cuda")
    tl = build(model, B, loader)                               # row (d)
    xd, ld = x.cuda(), labels.cuda()
    resident = [(xd[k * B:(k + 1) * B].clone(), ld[k * B:(k + 1) * B].clone()) for k in range(8)]
    host = torch.utils.data.DataLoader(mdata.JetArrayDataset(raw_jets(x).numpy(), split="all"), batch_size=B, shuffle=True,
                                       drop_last=True)
    state = {"k": 0, "it": iter(host)}
    ts.set_batch(*resident[0])

    def b_row():
        state["k"] = (state["k"] + 1) % len(resident)
        ts.set_batch(*resident[state["k"]])
        ts.step()

    def c_row():
        try:
            d, l = next(state["it"])
        except StopIteration:
            state["it"] = iter(host)
            d, l = next(state["it"])
        ts.set_batch(d.cuda(), l.cuda())
        ts.step()

    # the feed launch on its own: --chain of them captured into one graph (launched from Python one by one, the host's own
    # overhead per call would be what the events see) -- a replay is --chain launches back to back on the device
    loader.feed(tl)
    torch.cuda.synchronize()
    chain = torch.cuda.CUDAGraph()
    with torch.cuda.graph(chain):
        for _ in range(args.chain):
            loader.feed(tl)
    # name -> (what one iteration runs, iterations between the events, launches per iteration)
    rows = {"a step_fixed_batch": (ts.step, args.iters, 1), "b set_batch_device": (b_row, args.iters, 1),
            "c dataloader_host": (c_row, args.host_iters, 1), "d step_with_loader": (tl.step, args.iters, 1),
            "feed_launch": (chain.replay, 5, args.chain)}
    for fn, _, _ in rows.values():                             # warm-up: captures both steps, fills the allocator's pools
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    us = {name: [] for name in rows}
    for _ in range(args.reps):                                 # (alternated: the rows share whatever the box does meanwhile)
        for name, (fn, iters, per) in rows.items():
            us[name].append(between_events(fn, iters) / per)
    med = {}
    for name, v in us.items():
        med[name] = float(np.median(v))
        emit({"model": model, "B": B, "N": N, "n": N_JETS, "row": name, "per": rows[name][1] * rows[name][2], "reps": args.reps,
              "median_us": med[name], "min_us": float(np.min(v)), "max_us": float(np.max(v))})
    a, b, d, feed = (med[k] for k in ("a step_fixed_batch", "b set_batch_device", "d step_with_loader", "feed_launch"))
    spread = float(np.max(us["a step_fixed_batch"]) - np.min(us["a step_fixed_batch"]))
    emit({"model": model, "B": B, "row": "conditions", "d_minus_b_us": d - b, "d_le_b": bool(d <= b),
          "d_minus_a_us": d - a, "feed_launch_us": feed, "spread_a_us": spread, "d_le_a_plus_feed_plus_spread": bool(d <= a + feed + spread),
          "set_batch_cost_us": b - a, "dataloader_cost_us": med["c dataloader_host"] - a,
          "D_loss": float(tl.D_loss), "position": loader.position})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="both")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--host-iters", type=int, default=10)
    ap.add_argument("--chain", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loader_bench: no GPU visible (timings are taken on the device or not at all)")
    sink = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()
    for model, B in (("mpgan", 256), ("gapt", 512)):
        if args.model in (model, "both"):
            run(model, B, args, emit)


if __name__ == "__main__":
    main()
