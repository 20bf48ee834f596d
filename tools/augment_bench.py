"""Timings of the device-side jet augmentation (csrc/augment.hip) on one GPU.  One JSON object per line on stdout and in --out.

    python tools/augment_bench.py [--section kernels|step|gapt|trace-plain|trace-aug] [--reps 20] [--out profiles/augment_bench.jsonl]

kernels      mpg_augment (in place) and mpg_augment_bwd at B = 256 and 4096, N = 30 and 150, all four stages at p = 0.5; beside
             them, in the same process on the same tensors, the nearest thing to an empty launch this library has (mpg_augment
             of one jet without particles and without stages) and one eager ``mpgan.augment.augment`` call with all four stages.
             A launch of a few microseconds is below what a pair of HIP events resolves: --chain launches go between two events
             and the time is divided by their number (launches in a stream, back to back), median of --reps after a warm-up.
step         the captured MPGAN iteration at B = 256, N = 30: ``augment=None`` against aug_prob = 0.5, both built in this process,
             --iters replays between two events, the two steps alternated --reps times; medians and their difference.
gapt         the same at GAPT's B = 512, N = 30: the plain step with the one-launch bridge, the plain step without it
             (MPG_BRIDGE=0) and the augmented step (which leaves the bridge).
trace-plain / trace-aug   --iters replays of the plain / the augmented captured MPGAN iteration and nothing else: the program to put
             behind ``rocprofv3 --kernel-trace --stats --`` for the launch counts (tools/augment_bench.py counts nothing itself).
"""
import argparse
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpgan_amd import ops, train  # noqa: E402
from mpgan_amd.mpgan import augment as maugment  # noqa: E402

ALL, RATIO, SD = 15, 0.125, 0.125


def timed(fn, chain, reps, warm=3):
    """Median / min / max over ``reps`` of (time of ``chain`` calls of fn between two HIP events) / chain, in microseconds."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(chain):
            fn()
        b.record()
        b.synchronize()
        us.append(1e3 * a.elapsed_time(b) / chain)
    return {"median_us": float(np.median(us)), "min_us": float(np.min(us)), "max_us": float(np.max(us))}


def kernels(args, emit):
    p = torch.full((1,), 0.5, device="cuda")
    ref_args = SimpleNamespace(device="cuda", aug_r90=True, aug_f=True, aug_t=True, aug_s=True, translate_ratio=RATIO, scale_sd=SD)
    one = torch.zeros(1, 6, device="cuda")
    emit({"what": "near-empty launch (mpg_augment, 1 jet, N = 0, no stage)", "chain": args.chain,
          **timed(lambda: ops.augment_params(1, p, 0, RATIO, SD, 0, out=one), args.chain, args.reps)})
    for B in (256, 4096):
        for N in (30, 150):
            x = torch.randn(B, N, 3, device="cuda")
            dy, dx = torch.randn(B, N, 3, device="cuda"), torch.empty(B, N, 3, device="cuda")
            prm = torch.empty(B, 6, device="cuda")
            L, st = ops._lib.lib(), ops._stream
            emit({"what": "mpg_augment", "B": B, "N": N, "chain": args.chain,
                  **timed(lambda: ops.augment(x, p, ALL, RATIO, SD, 0, out=x, params=prm), args.chain, args.reps)})
            emit({"what": "mpg_augment_bwd", "B": B, "N": N, "chain": args.chain,
                  **timed(lambda: ops.check(L.mpg_augment_bwd(ops._p(dy), ops._p(dx), N * 3, 3, 3, B, N, ops._p(prm), st()), "mpg_augment_bwd"),
                          args.chain, args.reps)})
            emit({"what": "eager mpgan.augment.augment (torch, host draws)", "B": B, "N": N, "chain": 1,
                  **timed(lambda: maugment.augment(ref_args, x, 0.5), 1, args.reps)})


def build(model, B, N, augment, bridge=True):
    old = os.environ.get("MPG_BRIDGE")
    os.environ["MPG_BRIDGE"] = "1" if bridge else "0"
    try:
        if model == "mpgan":
            G, D = train.default_mpgan(N)
            latent, lrs = 32, train.LR["g"]
        else:
            G, D = train.default_gapt(N)
            latent, lrs = 64, train.LR_GAPT
        ts = train.TrainStep(G, D, B, N, latent=latent, lr_disc=lrs[0], lr_gen=lrs[1], use_graphs=True, augment=augment)
    finally:
        os.environ.pop("MPG_BRIDGE", None) if old is None else os.environ.__setitem__("MPG_BRIDGE", old)
    from mpgan_amd import data
    x, labels = data.synthetic_jets(B, N, seed=1)
    ts.set_batch(x.cuda(), labels.cuda())
    ts.capture()
    return ts


def aug_cfg():
    return train.Augment(aug_r90=True, aug_f=True, aug_t=True, aug_s=True, translate_ratio=RATIO, scale_sd=SD, aug_prob=0.5)


def compare(model, B, N, variants, args, emit):
    torch.manual_seed(0)
    steps = {name: build(model, B, N, aug, bridge) for name, (aug, bridge) in variants.items()}
    us = {name: [] for name in steps}
    for ts in steps.values():
        for _ in range(args.iters):
            ts.step()
    torch.cuda.synchronize()
    for _ in range(args.reps):          # (alternated: the variants share whatever the box does meanwhile)
        for name, ts in steps.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.iters):
                ts.step()
            b.record()
            b.synchronize()
            us[name].append(1e3 * a.elapsed_time(b) / args.iters)
    med = {name: float(np.median(v)) for name, v in us.items()}
    for name, v in us.items():
        emit({"what": f"{model} captured iteration, {name}", "B": B, "N": N, "iters": args.iters, "reps": args.reps,
              "median_us": med[name], "min_us": float(np.min(v)), "max_us": float(np.max(v)),
              "bridge_route": bool(steps[name]._bridge()), "D_loss": float(steps[name].D_loss)})
    first = next(iter(med))
    emit({"what": f"{model}: difference to '{first}'", **{name: med[name] - med[first] for name in med if name != first}})


def trace(augment, args):
    ts = build("mpgan", 256, 30, augment)
    torch.cuda.synchronize()
    for _ in range(args.iters):
        ts.step()
    torch.cuda.synchronize()
    print(json.dumps({"what": "trace", "augment": augment is not None, "captured_warmup_iterations": 3, "replays": args.iters}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--section", default="kernels")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--chain", type=int, default=200)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_bench: no GPU visible (timings are taken on the device or not at all)")
    sink = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps({"section": args.section, **rec})
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()
    if args.section == "kernels":
        kernels(args, emit)
    elif args.section == "step":
        compare("mpgan", 256, 30, {"augment=None": (None, True), "aug_prob=0.5": (aug_cfg(), True)}, args, emit)
    elif args.section == "gapt":
        compare("gapt", 512, 30, {"augment=None, bridge": (None, True), "augment=None, MPG_BRIDGE=0": (None, False),
                                  "aug_prob=0.5": (aug_cfg(), True)}, args, emit)
    elif args.section in ("trace-plain", "trace-aug"):
        trace(aug_cfg() if args.section == "trace-aug" else None, args)
    else:
        raise SystemExit(f"unknown section {args.section}")


if __name__ == "__main__":
    main()
