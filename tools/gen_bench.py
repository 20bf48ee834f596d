"""Bulk generation on one GPU: eager ``gen.generate_jets`` against ``gen.JetSampler.sample``.  One JSON object per case on stdout
and appended to --out.

    python tools/gen_bench.py [--reps 10] [--out profiles/gen_bench.jsonl] [--cases mpgan30c256,...]

One process.  Cases (generator at its real widths, default initialisation -- the work does not depend on the weights):

    mpgan30c256    MPGAN, N = 30,  chunk 256,   65 536 jets
    mpgan30c4096   MPGAN, N = 30,  chunk 4096,  65 536 jets
    mpgan150c64    MPGAN, N = 150, chunk 64,    16 384 jets
    gapt30c4096    GAPT,  N = 30,  chunk 4096,  65 536 jets

Both paths produce the same thing, ``[jets, N, 3]`` un-normalised on the device.  The eager path is handed one label per jet,
already on the device (it has no label draw of its own); the sampler draws its labels from the same table inside its chunk.  A
repetition is one whole call of each path, taken alternately, each between two HIP events of its own (so what an event pair costs
cancels between them) and ended by the second event's synchronise; the figures are jets / second from the median, the fastest and
the slowest of --reps repetitions behind a warm-up of two calls each (which loads every kernel and captures the sampler's graph).

Launches per chunk are counted, not timed, in a pass of their own: calls into the HIP library (``mpg_*`` entry points) and ATen
operators that launch (views and allocations left out), for one more chunk of the eager path and for the sampler's chunk run
eagerly -- what its graph holds; with the graph the host submits one replay and one launch (``mpg_jets_finish``) per chunk.

No speed-up is promised.  Each line states the one condition the sampler is held to: its median time is not above the eager
path's median by more than the eager path's own spread (max - min of its repetitions).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
from torch.utils._python_dispatch import TorchDispatchMode

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpgan_amd import _lib, data as mdata, gen, train  # noqa: E402

CASES = {
    "mpgan30c256": ("mpgan", 30, 256, 65536),
    "mpgan30c4096": ("mpgan", 30, 4096, 65536),
    "mpgan150c64": ("mpgan", 150, 64, 16384),
    "gapt30c4096": ("gapt", 30, 4096, 65536),
}
NO_LAUNCH = ("view", "reshape", "slice", "select", "squeeze", "unsqueeze", "expand", "detach", "alias", "transpose", "permute",
             "as_strided", "empty", "t.default", "_unsafe_view", "lift_fresh", "split", "unbind", "chunk", "narrow")


class _Counts(TorchDispatchMode):
    """ATen operators that launch, by name, while the mode is on; and -- through ``hip`` -- calls into the HIP library."""

    def __init__(self):
        super().__init__()
        self.aten, self.hip = 0, 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        name = str(func).replace("aten.", "")
        if not name.startswith(NO_LAUNCH):
            self.aten += 1
        return func(*args, **(kwargs or {}))


class _LibProxy:
    def __init__(self, lib, counts):
        self._lib, self._counts = lib, counts

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("mpg_"):
            return fn

        def call(*a):
            self._counts.hip += 1
            return fn(*a)
        return call


def counted(fn):
    """(calls into the HIP library, launching ATen operators) of ``fn()``."""
    real = _lib.lib()
    with _Counts() as c:
        _lib._lib = _LibProxy(real, c)
        try:
            fn()
        finally:
            _lib._lib = real
    torch.cuda.synchronize()
    return c.hip, c.aten


def timed(fn):
    """seconds between an event before and an event behind ``fn()``"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return 1e-3 * a.elapsed_time(b)


def run_case(name, reps):
    model, N, chunk, jets = CASES[name]
    torch.manual_seed(0)
    G, _ = (train.default_mpgan if model == "mpgan" else train.default_gapt)(N)
    _, table = mdata.synthetic_jets(8192, N, seed=1)             # the data set's num_particles / N
    table = table.reshape(-1).cuda()
    labels = table[torch.randint(0, table.numel(), (jets,), device="cuda")].reshape(-1, 1)
    sampler = gen.JetSampler(G, table, N, chunk=chunk, model=model, seed=1)
    out = torch.empty(jets, N, 3, device="cuda")
    eager = lambda n=jets: gen.generate_jets(G, n, num_particles=N, labels=labels[:n], model=model, batch_size=chunk)
    fused = lambda: sampler.sample(jets, out=out)
    for _ in range(2):
        eager()
        fused()
    torch.cuda.synchronize()
    t = {"eager": [], "sampler": []}
    for _ in range(reps):
        t["eager"].append(timed(eager))
        t["sampler"].append(timed(fused))
    # launches, in a pass of their own
    one, two = counted(lambda: eager(chunk)), counted(lambda: eager(2 * chunk))
    was = G.training
    G.eval()
    with torch.no_grad():
        front = counted(sampler._front)
    G.train(was)
    rate = lambda ts: {"median": jets / float(np.median(ts)), "min": jets / max(ts), "max": jets / min(ts)}
    e, s = np.asarray(t["eager"]), np.asarray(t["sampler"])
    spread = float(e.max() - e.min())
    ok = bool(np.median(s) <= np.median(e) + spread)
    return {
        "case": name, "model": model, "N": N, "chunk": chunk, "jets": jets, "reps": reps,
        "eager_jets_per_s": rate(e), "sampler_jets_per_s": rate(s),
        "eager_s": {"median": float(np.median(e)), "min": float(e.min()), "max": float(e.max())},
        "sampler_s": {"median": float(np.median(s)), "min": float(s.min()), "max": float(s.max())},
        "launches_per_chunk": {
            "eager": {"hip_library_calls": two[0] - one[0], "aten_launching_ops": two[1] - one[1]},
            "eager_once_per_call": {"hip_library_calls": 2 * one[0] - two[0], "aten_launching_ops": 2 * one[1] - two[1]},
            "sampler_graph_holds": {"hip_library_calls": front[0], "aten_launching_ops": front[1]},
            "sampler_host_submissions": {"graph_replays": 1, "hip_library_calls": 1},
        },
        "condition": "sampler median time <= eager median time + (eager max - eager min)",
        "condition_holds": ok,
        "device": torch.cuda.get_device_name(0), "source_digest": _lib.source_digest(),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default=",".join(CASES))
    args = ap.parse_args()
    names = [c for c in args.cases.split(",") if c]
    for c in names:
        if c not in CASES:
            raise SystemExit(f"gen_bench: unknown case {c!r} (one of {', '.join(CASES)})")
    if not torch.cuda.is_available():
        raise SystemExit("gen_bench: no GPU visible (timings are taken on the device or not at all)")
    sink = open(args.out, "a") if args.out else None
    for c in names:
        rec = run_case(c, args.reps)
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()
        print(f"# {c}: sampler {rec['sampler_jets_per_s']['median']:.4g} jets/s, eager {rec['eager_jets_per_s']['median']:.4g} jets/s; "
              f"condition {'holds' if rec['condition_holds'] else 'FAILS'}", flush=True)


if __name__ == "__main__":
    main()
