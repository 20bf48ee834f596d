"""What the fused TreeGCN launches (``ops.OPTIONS["tree_gcn"]``: mpg_tree_gcn_fwd / _bwd) cost next to the un-fused route (the
reference's literal layer on ``FusedLinearFn``, torch.matmul and ATen's LeakyReLU, the [rows, in support] activation of W_loop
included) in ``mpgan_amd.ext_models.TreeGANG``, on one GPU.  One JSON object per line on stdout and in --out.

    python tools/treegan_bench.py [--reps 10] [--batches 10] [--batch 256] [--out profiles/treegan_bench.jsonl]

One process.  ``TreeGANG`` at the default configuration (features [96, 64, 64, 64, 64, 3], degrees [2, 2, 2, 2, 2], support 10) and
--batch jets, eager launches.  Rows: a unfused_fwd, b fused_fwd (forward under no_grad), c unfused_fwd_bwd, d fused_fwd_bwd
(forward + backward with all parameter gradients; the noise asks for none, as in training).  The routes are alternated and every
timed region sits between two HIP events of its own.  A repetition is --batches regions of each kind; the rows are the means within
a repetition, reported as median / min / max over --reps repetitions behind a warm-up.

No speed-up is promised.  The last line states ONE condition per direction: the fused route's median is not above the un-fused
route's median by more than the un-fused route's own min-max spread.  The yardstick is the un-fused route: it is made of launches
the library had before the fused ones.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from knn_bench import jsonl_sink, measure  # noqa: E402

DEFAULT = dict(features=[96, 64, 64, 64, 64, 3], degrees=[2, 2, 2, 2, 2], support=10)


def runs(torch, ops, B):
    """{row: closure}: the same module and noise under both settings of the option."""
    from mpgan_amd import ext_models
    torch.manual_seed(0)
    net = ext_models.TreeGANG(**DEFAULT).cuda()
    noise = torch.randn(B, 1, DEFAULT["features"][0], device="cuda") * 0.2
    up = torch.randn(B, 32, 3, device="cuda")

    def fwd(fused):
        def go():
            ops.OPTIONS["tree_gcn"] = fused
            with torch.no_grad():
                net([noise])
        return go

    def fwd_bwd(fused):
        def go():
            ops.OPTIONS["tree_gcn"] = fused
            (net([noise]) * up).sum().backward()
        return go
    return [("a unfused_fwd", fwd(False)), ("b fused_fwd", fwd(True)), ("c unfused_fwd_bwd", fwd_bwd(False)),
            ("d fused_fwd_bwd", fwd_bwd(True))]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batches", type=int, default=10, help="timed regions of each kind per repetition")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=os.path.join("profiles", "treegan_bench.jsonl"))
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("treegan_bench: no GPU visible (timings are taken on the device or not at all)")
    from mpgan_amd import ops
    emit = jsonl_sink(args.out)
    was = ops.OPTIONS["tree_gcn"]
    try:
        pairs = runs(torch, ops, args.batch)
        for _ in range(5):   # warm-up of every row
            for _, fn in pairs:
                fn()
        torch.cuda.synchronize()
        us = measure(torch, pairs, args.reps, args.batches)
        med = {}
        for r, v in us.items():
            med[r] = float(np.median(v))
            emit({"net": "TreeGANG", "B": args.batch, "row": r, "captured": False, "reps": args.reps, "batches_per_rep": args.batches,
                  "median_us": med[r], "min_us": float(np.min(v)), "max_us": float(np.max(v))})
        cond = {"net": "TreeGANG", "B": args.batch, "row": "condition"}
        for what, a, b in (("fwd", "a unfused_fwd", "b fused_fwd"), ("fwd_bwd", "c unfused_fwd_bwd", "d fused_fwd_bwd")):
            spread = float(np.max(us[a]) - np.min(us[a]))
            cond.update({f"{what}_fused_minus_unfused_us": med[b] - med[a], f"{what}_spread_unfused_us": spread,
                         f"{what}_fused_not_above_unfused_by_more_than_spread": bool(med[b] - med[a] <= spread),
                         f"{what}_ratio_unfused_over_fused": med[a] / med[b]})
        emit(cond)
    finally:
        ops.OPTIONS["tree_gcn"] = was
    return 0


if __name__ == "__main__":
    sys.exit(main())
