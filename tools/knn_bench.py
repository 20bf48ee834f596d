"""What the sparse k-NN route of the fused MPLayer (``ops.OPTIONS["knn_sparse"]``: the B * N * k rows of the neighbour sets) costs next
to the dense route (all N * N pairs with the neighbour bit as a factor), on one GPU.  One JSON object per line on stdout and in --out.

    python tools/knn_bench.py [--reps 10] [--batches 10] [--sizes 150,20,16 30,10,256] [--no-steps] [--out profiles/knn_bench.jsonl]

One process.  Per size (N, k, B):

layer   one MPLayer (32 -> 32 features, fully_connected=False, num_knn=k, the mask of ``data.synthetic_jets``), forward + backward
        with all parameter gradients.  Each route's launches are captured once into a HIP graph and the replays are timed: run
        eagerly a layer is a dozen launches issued from Python and both routes cost what the host takes to issue them (1.2 ms at
        either size) -- ``--eager-layers`` times that instead.  Rows: a dense_layer, b sparse_layer.
step    the whole captured ``TrainStep`` of an MPGAN whose MPLayers are all on the k-NN graph, D's dropout on.  Rows: c dense_step,
        d sparse_step.  Each step is captured under its own setting of the option and replays the launches it was captured with.

The two routes are alternated and every timed region sits between two HIP events of its own.  A repetition is --batches regions of
each kind; the rows are the means within a repetition, reported as median / min / max over --reps repetitions behind a warm-up.
Every size's first line gives the algorithmic FLOPs of the edge network's two dense layers (fe.net.1, fe.net.2; forward, data
gradients and weight gradients: three products per layer) on both routes, computed from the shapes alone: B N N rows against B N k.

No ratio is promised.  The last line of a size states ONE condition, for N = 150, k = 20: the sparse layer's median is below the
dense layer's median by more than the dense route's own min-max spread.  The dense route is the code this option leaves untouched.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H1, H2, H3 = 96, 160, 192


def edge_flops(B, N, k):
    """Algorithmic FLOPs of fe.net.1 + fe.net.2 over one forward + backward (three products per layer, 2 FLOPs per multiply-add):
    (dense route: B N N edge rows, sparse route: B N k)."""
    per_row = 3 * 2 * (H1 * H2 + H2 * H3)
    return B * N * N * per_row, B * N * k * per_row


def parse_sizes(text):
    sizes = []
    for item in text:
        N, k, B = (int(v) for v in item.split(","))
        if not 0 < k < N:
            raise SystemExit(f"knn_bench: k = {k} of N = {N} (the sparse route takes 0 < k < N)")
        sizes.append((N, k, B))
    return sizes


def timed(torch, fn):
    """microseconds between an event before and an event behind ``fn()``"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b)


def jsonl_sink(path):
    sink = open(path, "a") if path else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()
    return emit


def layer_runs(torch, ops, N, k, B, eager=False):
    """(dense, sparse): closures that run one forward + backward of the same layer on the same input under their route -- replays of
    a graph captured per route, or (``eager``) the launches themselves."""
    from mpgan_amd import data as mdata
    from mpgan_amd.mpgan import MPLayer
    torch.manual_seed(0)
    jets, _ = mdata.synthetic_jets(B, N, seed=1)
    mask = (jets[..., 3:4] + 0.5).cuda().contiguous()
    x = (torch.randn(B, N, 32, device="cuda") * 0.5).requires_grad_(True)
    up = torch.randn(B, N, 32, device="cuda")
    layer = MPLayer(32, [96, 160, 192], [256, 256], 32, fully_connected=False, num_knn=k).cuda()

    def run(sparse):
        def go():
            ops.OPTIONS["knn_sparse"] = sparse
            y = layer(x, True, mask)
            (y * up).sum().backward()
        if eager:
            return go
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):   # (warm-up: weight images, tickets and the allocator's pools exist before the capture)
            for _ in range(3):
                go()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            go()
        return graph.replay
    return run(False), run(True)


def step_runs(torch, ops, N, k, B):
    """(dense, sparse): the ``step`` of two captured TrainSteps over the same weights and batch."""
    from mpgan_amd import data as mdata, train
    steps = []
    for sparse in (False, True):
        ops.OPTIONS["knn_sparse"] = sparse
        torch.manual_seed(0)
        G, D = train.default_mpgan(N)
        for l in (*G.mp_layers, *D.mp_layers):
            l.fully_connected, l.num_knn = False, k
        lrs = train.LR["g"]
        ts = train.TrainStep(G, D, B, N, lr_disc=lrs[0], lr_gen=lrs[1], use_graphs=True)
        x, labels = mdata.synthetic_jets(B, N, seed=1)
        ts.set_batch(x.cuda(), labels.cuda())
        for _ in range(3):   # warm-up: captures the graph, under this leg's setting
            ts.step()
        torch.cuda.synchronize()
        steps.append(ts)
    return steps[0].step, steps[1].step, steps


def measure(torch, pairs, reps, batches):
    """{row: [mean microseconds of a repetition]} for the (row, closure) ``pairs``, alternated within a repetition."""
    us = {r: [] for r, _ in pairs}
    for _ in range(reps):
        t = {r: [] for r, _ in pairs}
        for _ in range(batches):
            for r, fn in pairs:
                t[r].append(timed(torch, fn))
        for r in t:
            us[r].append(float(np.mean(t[r])))
    return us


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batches", type=int, default=10, help="timed regions of each kind per repetition")
    ap.add_argument("--sizes", nargs="+", default=["150,20,16", "30,10,256"], help="N,k,B per size")
    ap.add_argument("--no-steps", action="store_true", help="layers only")
    ap.add_argument("--eager-layers", action="store_true", help="time the layers' launches as Python issues them, not graph replays")
    ap.add_argument("--flops-only", action="store_true", help="print the FLOP counts and stop (needs no device)")
    ap.add_argument("--out", default=os.path.join("profiles", "knn_bench.jsonl"))
    args = ap.parse_args(argv)
    sizes = parse_sizes(args.sizes)
    flops = {s: edge_flops(s[2], s[0], s[1]) for s in sizes}
    if args.flops_only:
        for (N, k, B), (fd, fs) in flops.items():
            print(json.dumps({"N": N, "k": k, "B": B, "row": "edge_flops", "dense": fd, "sparse": fs, "ratio": fd / fs}))
        return 0
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("knn_bench: no GPU visible (timings are taken on the device or not at all)")
    from mpgan_amd import ops
    emit = jsonl_sink(args.out)
    was = ops.OPTIONS["knn_sparse"]
    try:
        for N, k, B in sizes:
            fd, fs = flops[(N, k, B)]
            plan = ops.knn_plan(B, N, k, True)
            emit({"N": N, "k": k, "B": B, "row": "edge_flops", "dense": fd, "sparse": fs, "ratio": fd / fs, "receivers_per_workgroup": plan.RW,
                  "workgroups": plan.workgroups, "parked_bytes_per_jet": plan.parked_bytes // B, "grad_bytes_per_jet": plan.grad_bytes // B})
            dense, sparse = layer_runs(torch, ops, N, k, B, eager=args.eager_layers)
            pairs = [("a dense_layer", dense), ("b sparse_layer", sparse)]
            if not args.no_steps:
                dstep, sstep, keep = step_runs(torch, ops, N, k, B)
                pairs += [("c dense_step", dstep), ("d sparse_step", sstep)]
            for _ in range(3):   # warm-up of every row
                for _, fn in pairs:
                    fn()
            torch.cuda.synchronize()
            us = measure(torch, pairs, args.reps, args.batches)
            med = {}
            for r, v in us.items():
                med[r] = float(np.median(v))
                emit({"N": N, "k": k, "B": B, "row": r, "captured": not (args.eager_layers and r.endswith("layer")), "reps": args.reps, "batches_per_rep": args.batches, "median_us": med[r],
                      "min_us": float(np.min(v)), "max_us": float(np.max(v))})
            a, b = "a dense_layer", "b sparse_layer"
            spread = float(np.max(us[a]) - np.min(us[a]))
            cond = {"N": N, "k": k, "B": B, "row": "condition", "dense_minus_sparse_layer_us": med[a] - med[b], "spread_dense_layer_us": spread,
                    "sparse_below_dense_by_more_than_spread": bool(med[a] - med[b] > spread), "layer_ratio_dense_over_sparse": med[a] / med[b],
                    "held_to": bool((N, k) == (150, 20))}
            if not args.no_steps:
                cond["step_ratio_dense_over_sparse"] = med["c dense_step"] / med["d sparse_step"]
                cond.update({f"{n}_loss_{r}": float(getattr(ts, n + "_loss")) for r, ts in zip(("dense", "sparse"), keep) for n in ("D", "G")})
            emit(cond)
    finally:
        ops.OPTIONS["knn_sparse"] = was
    return 0


if __name__ == "__main__":
    sys.exit(main())
