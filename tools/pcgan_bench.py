"""What the one-launch set encoder (``ops.OPTIONS["set_encode"]``: mpg_set_encode_fwd) costs next to the un-fused route (every Linear
on ``FusedLinearFn`` with ATen's max, subtract and tanh between them) in ``mpgan_amd.ext_models.G_inv_Tanh``, on one GPU.  One JSON
object per line on stdout and in --out.

    python tools/pcgan_bench.py [--reps 10] [--batches 10] [--batch 256] [--particles 30] [--out profiles/set_encode_bench.jsonl]

One process.  The frozen encoder at the published widths (x_dim 3, d_dim = z1_dim = 256, pool max1; ``load_pcgan_encoder`` on a
randomly initialised state dict: the time does not depend on the values) on --batch jets of --particles particles, the whole forward,
``ro`` included.  Rows: a unfused_fwd, b fused_fwd -- eager launches, as train.py:839 calls the encoder --, c unfused_fwd_graph,
d fused_fwd_graph -- replays of the same forward captured with torch.cuda.graph, which take the host's launch cost out.  The routes
are alternated and every timed region sits between two HIP events of its own.  A repetition is --batches regions of each kind; the
rows are the means within a repetition, reported as median / min / max over --reps repetitions behind a warm-up.

No speed-up is promised.  The last line states ONE condition per pair: the fused route's median is not above the un-fused route's
median by more than the un-fused route's own min-max spread.  The yardstick is the un-fused route: it is made of launches the
library had before the fused one.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from knn_bench import jsonl_sink, measure  # noqa: E402

WIDTHS = dict(x_dim=3, d_dim=256, z1_dim=256, pool="max1")


def runs(torch, ops, B, N):
    """[(row, closure)]: the same module and batch under both settings of the option, eager and as graph replays."""
    from mpgan_amd import ext_models
    torch.manual_seed(0)
    enc = ext_models.load_pcgan_encoder(ext_models.G_inv_Tanh(**WIDTHS).state_dict(), **WIDTHS).cuda()
    x = torch.cat((torch.randn(B, N, 2) * 0.1, torch.rand(B, N, 1) - 0.5), 2).cuda()

    def eager(fused):
        def go():
            ops.OPTIONS["set_encode"] = fused
            enc(x)
        return go

    def replay(fused):
        go = eager(fused)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                go()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            go()
        return graph.replay
    return [("a unfused_fwd", eager(False)), ("b fused_fwd", eager(True)), ("c unfused_fwd_graph", replay(False)),
            ("d fused_fwd_graph", replay(True))]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batches", type=int, default=10, help="timed regions of each kind per repetition")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--particles", type=int, default=30)
    ap.add_argument("--out", default=os.path.join("profiles", "set_encode_bench.jsonl"))
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("pcgan_bench: no GPU visible (timings are taken on the device or not at all)")
    from mpgan_amd import ops
    emit = jsonl_sink(args.out)
    was = ops.OPTIONS["set_encode"]
    try:
        pairs = runs(torch, ops, args.batch, args.particles)
        for _ in range(5):   # warm-up of every row
            for _, fn in pairs:
                fn()
        torch.cuda.synchronize()
        us = measure(torch, pairs, args.reps, args.batches)
        med = {}
        head = {"net": "G_inv_Tanh", "B": args.batch, "N": args.particles}
        for r, v in us.items():
            med[r] = float(np.median(v))
            emit({**head, "row": r, "captured": r.endswith("_graph"), "reps": args.reps, "batches_per_rep": args.batches,
                  "median_us": med[r], "min_us": float(np.min(v)), "max_us": float(np.max(v))})
        cond = {**head, "row": "condition"}
        for what, a, b in (("fwd", "a unfused_fwd", "b fused_fwd"), ("fwd_graph", "c unfused_fwd_graph", "d fused_fwd_graph")):
            spread = float(np.max(us[a]) - np.min(us[a]))
            cond.update({f"{what}_fused_minus_unfused_us": med[b] - med[a], f"{what}_spread_unfused_us": spread,
                         f"{what}_fused_not_above_unfused_by_more_than_spread": bool(med[b] - med[a] <= spread),
                         f"{what}_ratio_unfused_over_fused": med[a] / med[b]})
        emit(cond)
    finally:
        ops.OPTIONS["set_encode"] = was
    return 0


if __name__ == "__main__":
    sys.exit(main())
