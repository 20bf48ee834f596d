"""What the fused layer-and-pool launch (``ops.OPTIONS["point_pool"]``: mpg_point_pool_fwd / _bwd) costs next to the un-fused route
(``FusedLinearFn`` for the last point layer, then torch.max / torch.mean on its [B N, C] output) in the baseline discriminators of
``mpgan_amd.ext_models``, on one GPU.  One JSON object per line on stdout and in --out.

    python tools/baseline_bench.py [--reps 10] [--batches 10] [--batch 256] [--out profiles/point_pool_bench.jsonl]

One process.  ``PointNetMixD`` (pointfc [64, 128, 1024], fc [512], mask) and ``rGAND`` (sfc [64, 128, 256, 256, 512], fc [128, 64]) at
N = 30 particles and --batch jets, eager launches (a discriminator call is a dozen launches issued from Python).  Rows per network:
a unfused_fwd, b fused_fwd (forward under no_grad), c unfused_fwd_bwd, d fused_fwd_bwd (forward + backward with the input gradient
and all parameter gradients).  The routes are alternated and every timed region sits between two HIP events of its own.  A
repetition is --batches regions of each kind; the rows are the means within a repetition, reported as median / min / max over
--reps repetitions behind a warm-up.

No speed-up is promised.  The last line of a network states ONE condition per direction: the fused route's median is not above the
un-fused route's median by more than the un-fused route's own min-max spread.
"""
import argparse
import json
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from knn_bench import jsonl_sink, measure  # noqa: E402

N = 30
ARGS = dict(rgand_sfc=[64, 128, 256, 256, 512], rgand_fc=[128, 64], pointnetd_pointfc=[64, 128, 1024], pointnetd_fc=[512],
            num_hits=N, node_feat_size=3, leaky_relu_alpha=0.2, mask=True)


def runs(torch, ops, name, B):
    """{row: closure} for one network: the same module and input under both settings of the option."""
    from mpgan_amd import data as mdata, ext_models
    torch.manual_seed(0)
    net = (ext_models.PointNetMixD if name == "PointNetMixD" else ext_models.rGAND)(types.SimpleNamespace(**ARGS)).cuda()
    jets, _ = mdata.synthetic_jets(B, N, seed=1)
    x = jets.cuda() if name == "PointNetMixD" else jets[..., :3].contiguous().cuda()
    x.requires_grad_(True)
    up = torch.randn(B, 1, device="cuda")

    def fwd(fused):
        def go():
            ops.OPTIONS["point_pool"] = fused
            with torch.no_grad():
                net(x)
        return go

    def fwd_bwd(fused):
        def go():
            ops.OPTIONS["point_pool"] = fused
            (net(x) * up).sum().backward()
        return go
    return [("a unfused_fwd", fwd(False)), ("b fused_fwd", fwd(True)), ("c unfused_fwd_bwd", fwd_bwd(False)),
            ("d fused_fwd_bwd", fwd_bwd(True))]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batches", type=int, default=10, help="timed regions of each kind per repetition")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=os.path.join("profiles", "point_pool_bench.jsonl"))
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("baseline_bench: no GPU visible (timings are taken on the device or not at all)")
    from mpgan_amd import ops
    emit = jsonl_sink(args.out)
    was = ops.OPTIONS["point_pool"]
    try:
        for name in ("PointNetMixD", "rGAND"):
            pairs = runs(torch, ops, name, args.batch)
            for _ in range(5):   # warm-up of every row
                for _, fn in pairs:
                    fn()
            torch.cuda.synchronize()
            us = measure(torch, pairs, args.reps, args.batches)
            med = {}
            for r, v in us.items():
                med[r] = float(np.median(v))
                emit({"net": name, "N": N, "B": args.batch, "row": r, "captured": False, "reps": args.reps, "batches_per_rep": args.batches,
                      "median_us": med[r], "min_us": float(np.min(v)), "max_us": float(np.max(v))})
            cond = {"net": name, "N": N, "B": args.batch, "row": "condition"}
            for what, a, b in (("fwd", "a unfused_fwd", "b fused_fwd"), ("fwd_bwd", "c unfused_fwd_bwd", "d fused_fwd_bwd")):
                spread = float(np.max(us[a]) - np.min(us[a]))
                cond.update({f"{what}_fused_minus_unfused_us": med[b] - med[a], f"{what}_spread_unfused_us": spread,
                             f"{what}_fused_not_above_unfused_by_more_than_spread": bool(med[b] - med[a] <= spread),
                             f"{what}_ratio_unfused_over_fused": med[a] / med[b]})
            emit(cond)
    finally:
        ops.OPTIONS["point_pool"] = was
    return 0


if __name__ == "__main__":
    sys.exit(main())
