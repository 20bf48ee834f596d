"""What the fused NNConv launches (``ops.OPTIONS["nnconv"]``: mpg_nnconv_fwd / _bwd) cost next to the un-fused route (PyG's literal
layer on ``FusedLinearFn``, torch.bmm and ATen: a [B N k, Cin Cout] weight tensor per edge) in ``mpgan_amd.ext_models.GraphCNNGANG``,
on one GPU.  One JSON object per line on stdout and in --out.

    python tools/graphcnn_bench.py [--reps 10] [--batches 10] [--batch 256] [--out profiles/graphcnn_bench.jsonl]

One process.  ``GraphCNNGANG`` at the published configuration (latent_dim 128, graphcnng_layers [32, 24], 30 particles, k = 20) and
--batch jets, training mode, eager launches.  Rows: a unfused_fwd, b fused_fwd (forward under no_grad), c unfused_fwd_bwd,
d fused_fwd_bwd (forward + backward with all parameter gradients; the noise asks for none, as in training).  The routes are
alternated and every timed region sits between two HIP events of its own.  A repetition is --batches regions of each kind; the rows
are the means within a repetition, reported as median / min / max over --reps repetitions behind a warm-up.  Two more rows give
``torch.cuda.max_memory_allocated`` of ONE forward + backward per route, over what was allocated before it.

No speed-up is promised.  The last line states ONE condition per direction: the fused route's median is not above the un-fused
route's median by more than the un-fused route's own min-max spread.  The yardstick is the un-fused route: there was no GraphCNN-GAN
generator before, and that route is made of launches the library had.
"""
import argparse
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from knn_bench import jsonl_sink, measure  # noqa: E402

PUBLISHED = dict(latent_dim=128, num_hits=30, graphcnng_layers=[32, 24], node_feat_size=3, num_knn=20, leaky_relu_alpha=0.2,
                 graphcnng_tanh=False, device="cuda")


def runs(torch, ops, B):
    """{row: closure}: the same module and noise under both settings of the option."""
    from mpgan_amd import ext_models
    torch.manual_seed(0)
    net = ext_models.GraphCNNGANG(types.SimpleNamespace(**PUBLISHED)).cuda().train()
    noise = torch.randn(B, PUBLISHED["latent_dim"], device="cuda") * 0.2
    up = torch.randn(B, PUBLISHED["num_hits"], PUBLISHED["node_feat_size"], device="cuda")

    def fwd(fused):
        def go():
            ops.OPTIONS["nnconv"] = fused
            with torch.no_grad():
                net(noise)
        return go

    def fwd_bwd(fused):
        def go():
            ops.OPTIONS["nnconv"] = fused
            net.zero_grad(set_to_none=True)
            (net(noise) * up).sum().backward()
        return go
    return [("a unfused_fwd", fwd(False)), ("b fused_fwd", fwd(True)), ("c unfused_fwd_bwd", fwd_bwd(False)),
            ("d fused_fwd_bwd", fwd_bwd(True))]


def peak_bytes(torch, fn):
    """The peak allocation of one call of ``fn`` over what is allocated before it."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batches", type=int, default=10, help="timed regions of each kind per repetition")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=os.path.join("profiles", "graphcnn_bench.jsonl"))
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("graphcnn_bench: no GPU visible (timings are taken on the device or not at all)")
    from mpgan_amd import ops
    emit = jsonl_sink(args.out)
    was = ops.OPTIONS["nnconv"]
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
            emit({"net": "GraphCNNGANG", "B": args.batch, "row": r, "captured": False, "reps": args.reps, "batches_per_rep": args.batches,
                  "median_us": med[r], "min_us": float(np.min(v)), "max_us": float(np.max(v))})
        for r, fn in pairs[2:]:
            emit({"net": "GraphCNNGANG", "B": args.batch, "row": r + " peak_bytes", "max_memory_allocated": peak_bytes(torch, fn)})
        cond = {"net": "GraphCNNGANG", "B": args.batch, "row": "condition"}
        for what, a, b in (("fwd", "a unfused_fwd", "b fused_fwd"), ("fwd_bwd", "c unfused_fwd_bwd", "d fused_fwd_bwd")):
            spread = float(np.max(us[a]) - np.min(us[a]))
            cond.update({f"{what}_fused_minus_unfused_us": med[b] - med[a], f"{what}_spread_unfused_us": spread,
                         f"{what}_fused_not_above_unfused_by_more_than_spread": bool(med[b] - med[a] <= spread),
                         f"{what}_ratio_unfused_over_fused": med[a] / med[b]})
        emit(cond)
    finally:
        ops.OPTIONS["nnconv"] = was
    return 0


if __name__ == "__main__":
    sys.exit(main())
