"""Timings of the evaluation metrics (mpgan_amd/evaluation.py) on one GPU: mpg_jet_obs for 50k jets at N = 30 and 150 with
and without the EFPs (HIP events), the whole ``evaluate`` with the default keys on 50k + 50k jets (host clock around a
device synchronise), and the fp64 CPU path for comparison.  One JSON object per line on stdout and in --out.

    python tools/eval_bench.py [--jets 50000] [--reps 20] [--out profiles/eval_bench.jsonl]

The floor beside each kernel time is the FLOP count of the full N^3 product M = Theta diag(z) Theta (2 N^3 per jet,
3.4e11 FLOP for 50k jets at N = 150) over the 157.3 TFLOP/s fp32 peak; the kernel forms only the tiles of one triangle of M and
only as many rows as a jet has particles, so its own FLOP count is lower than that model's."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpgan_amd import data, evaluation as ev  # noqa: E402

PEAK_F32 = 157.3e12


def jets_of(n, N, seed, law="gluon"):
    x, _ = data.synthetic_jets(n, N, seed=seed, dist=law)
    return data.unnormalise_jets(x, "g")


def time_kernel(jets, with_efps, reps):
    for _ in range(3):
        ev._obs_cuda(jets, with_efps, True)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ev._obs_cuda(jets, with_efps, True)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jets", type=int, default=50000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu-jets", type=int, default=2000, help="jets the fp64 CPU path is timed on (scaled to --jets)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("eval_bench: no GPU visible; these timings are only meaningful on one")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").close()
    dev = torch.device("cuda:0")
    emit({"device": torch.cuda.get_device_name(0), "jets": a.jets, "reps": a.reps}, a.out)
    for N in (30, 150):
        cpu_jets = jets_of(a.jets, N, seed=N)
        jets = cpu_jets.to(dev)
        n_real = float((cpu_jets[..., 2] != 0).sum(1).double().mean())
        floor_ms = 2.0 * N ** 3 * a.jets / PEAK_F32 * 1e3
        for with_efps in (False, True):
            med, lo, hi = time_kernel(jets, with_efps, a.reps)
            rec = {"what": "mpg_jet_obs", "N": N, "efps": with_efps, "ms_median": med, "ms_min": lo, "ms_max": hi,
                   "mean_particles": n_real}
            if with_efps:
                rec.update({"floor_ms_2N3_at_peak": floor_ms, "floor_over_time": floor_ms / med})
            emit(rec, a.out)
        # the fp64 CPU statement of the same observables, timed on a slice and scaled to --jets
        k = min(a.cpu_jets, a.jets)
        t0 = time.perf_counter()
        ev._obs_cpu(cpu_jets[:k], True, True)
        dt = time.perf_counter() - t0
        emit({"what": "cpu_fp64_observables", "N": N, "jets_timed": k, "threads": torch.get_num_threads(), "s": dt,
              "s_scaled_to_jets": dt * a.jets / k}, a.out)
    # the whole evaluate, default keys, 50k real + 50k generated-like jets at N = 30 (num_w1_eval_samples 10000: 5 batches)
    real, gen = jets_of(a.jets, 30, seed=1).to(dev), jets_of(a.jets, 30, seed=2, law="quark").to(dev)
    for keys in (("w1p", "w1m"), ("w1p", "w1m", "w1efp")):
        times = []
        for r in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev.evaluate({k: [] for k in keys}, real, gen, "g", num_w1_eval_samples=10000, rng=np.random.RandomState(r))
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        emit({"what": "evaluate", "keys": list(keys), "N": 30, "real": a.jets, "gen": a.jets,
              "s_first": times[0], "s_median_rest": float(np.median(times[1:]))}, a.out)


if __name__ == "__main__":
    main()
