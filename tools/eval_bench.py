"""Timings of the evaluation metrics (mpgan_amd/evaluation.py) on one GPU: mpg_jet_obs for 50k jets at N = 30 and 150 with
and without the EFPs (HIP events), the whole ``evaluate`` with the default keys on 50k + 50k jets (host clock around a
device synchronise), and the fp64 CPU path for comparison.  One JSON object per line on stdout and in --out.

    python tools/eval_bench.py [--jets 50000] [--reps 20] [--out profiles/eval_bench.jsonl] [--section all|w1|emd30|emd150|fpd]

The ``emd30`` / ``emd150`` sections time the exact pairwise jet EMDs behind coverage and MMD (mpg_jet_emd): at N = 30 the
default ``cov_mmd`` problem, 10 batches of 100 x 100 pairs (ten launches between two HIP events, median of --reps after a
warm-up), the same ten matrices through the fp64 host build of the solver on 16 threads (host clock, median of 3) -- the
yardstick, there being no earlier GPU code -- their ratio, the whole ``cov_mmd`` on the device, and the augmentations per
pair against the solver's cap; at N = 150 one batch of 100 x 100.  ``--section all`` runs each of the two in a child
process of its own under a time limit (--emd-timeout seconds), so a kernel that does not come back ends that step alone.

The ``fpd`` section (a run of its own; it APPENDS to --out) times mpg_jet_efps_d4, the 21 connected EFPs of degree <= 4 behind FPD
and KPD, on the same 50k jets at N = 30 and 150 (HIP events, median of --reps after warm-ups), beside it in the same process
mpg_jet_obs with its five EFPs -- the same tile pass over M, so the yardstick --, the fp64 host path of the 36 columns once on a
slice, and whole ``fpd`` and ``kpd`` calls with their defaults on 50k + 50k rows of device features.

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


def emd_section(N, batches, reps, out, k=100):
    from mpgan_amd import _lib
    rs = np.random.RandomState(N)
    real, gen = jets_of(2000, N, seed=N + 1), jets_of(2000, N, seed=N + 2, law="quark")
    draws = [(rs.choice(len(real), k), rs.choice(len(gen), k)) for _ in range(batches)]
    pairs_h = [(gen[ig].contiguous(), real[ir].contiguous()) for ir, ig in draws]
    pairs_d = [(g.cuda(), r.cuda()) for g, r in pairs_h]
    for _ in range(2):
        for g, r in pairs_d:
            ev._emds(g, r, 1.0)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        outs = [ev._emds(g, r, 1.0) for g, r in pairs_d]
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    host_s, iters = [], []
    for rep in range(3):
        t0 = time.perf_counter()
        outs_h = [ev._emds(g, r, 1.0) for g, r in pairs_h]
        host_s.append(time.perf_counter() - t0)
    err = max(float((o.cpu().double() - h).abs().max()) for o, h in zip(outs, outs_h))
    for g, r in pairs_h:
        D = torch.empty(k, k, dtype=torch.float64)
        st, it = torch.empty(k, k, dtype=torch.int32), torch.empty(k, k, dtype=torch.int32)
        _lib.check(_lib.lib().mpg_jet_emd_host_iters(g.data_ptr(), 3 * N, r.data_ptr(), 3 * N, 3, k, k, N, 1.0, D.data_ptr(),
                                                     st.data_ptr(), it.data_ptr(), 16), "mpg_jet_emd_host_iters")
        iters.append(it)
    iters = torch.cat(iters).double()
    med = float(np.median(ms))
    emit({"what": "mpg_jet_emd", "N": N, "pairs": [batches, k, k], "ms_median": med, "ms_min": float(np.min(ms)),
          "ms_max": float(np.max(ms)), "us_per_pair": med * 1e3 / (batches * k * k),
          "host_fp64_16_threads_s_median": float(np.median(host_s)), "host_over_device": float(np.median(host_s)) * 1e3 / med,
          "max_abs_device_minus_host": err, "augmentations_mean": float(iters.mean()), "augmentations_max": int(iters.max()),
          "augmentation_cap": 32 * (N + 1)}, out)
    rd, gd = real.cuda(), gen.cuda()
    times = []
    for r in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cov, mmd = ev.cov_mmd(rd, gd, num_eval_samples=k, num_batches=batches, rng=np.random.RandomState(r))
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    emit({"what": "cov_mmd", "N": N, "num_eval_samples": k, "num_batches": batches, "s_first": times[0],
          "s_median_rest": float(np.median(times[1:])), "coverage": cov, "mmd": mmd}, out)


def time_events(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def fpd_section(a):
    dev = torch.device("cuda:0")
    feats = {}
    for N in (30, 150):
        cpu_jets = jets_of(a.jets, N, seed=N)
        jets = cpu_jets.to(dev)
        old = time_events(lambda: ev._obs_cuda(jets, True, True), a.reps)
        new = time_events(lambda: ev._efp_primes_cuda(jets, True), a.reps)
        emit({"what": "mpg_jet_efps_d4", "N": N, "jets": a.jets, "ms_median": new[0], "ms_min": new[1], "ms_max": new[2],
              "mpg_jet_obs_efps_ms_median": old[0], "mpg_jet_obs_efps_ms_min": old[1], "over_mpg_jet_obs": new[0] / old[0]}, a.out)
        k = min(a.cpu_jets, a.jets)
        t0 = time.perf_counter()
        ev.efps(cpu_jets[:k], efpset_args=[("d<=", 4)])
        dt = time.perf_counter() - t0
        emit({"what": "cpu_fp64_efps_d4", "N": N, "jets_timed": k, "threads": torch.get_num_threads(), "s": dt,
              "s_scaled_to_jets": dt * a.jets / k}, a.out)
        if N == 30:
            feats["real"] = ev.efps(jets, efpset_args=[("d<=", 4)])
            feats["gen"] = ev.efps(jets_of(a.jets, N, seed=2, law="quark").to(dev), efpset_args=[("d<=", 4)])
    for name, fn in (("fpd", ev.fpd), ("kpd", ev.kpd)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        val, err = fn(feats["real"], feats["gen"])
        torch.cuda.synchronize()
        emit({"what": name, "rows": [a.jets, a.jets], "columns": 36, "defaults": True, "s": time.perf_counter() - t0,
              "value": val, "error": err}, a.out)


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
    ap.add_argument("--section", default="all", choices=("all", "w1", "emd30", "emd150", "fpd"))
    ap.add_argument("--emd-timeout", type=int, default=300, help="seconds each EMD section may take as a child of --section all")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("eval_bench: no GPU visible; these timings are only meaningful on one")
    if a.section in ("emd30", "emd150"):
        emd_section(30, 10, a.reps, a.out) if a.section == "emd30" else emd_section(150, 1, max(3, a.reps // 4), a.out)
        return
    if a.section == "fpd":
        fpd_section(a)
        return
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").close()
    dev = torch.device("cuda:0")
    emit({"device": torch.cuda.get_device_name(0), "jets": a.jets, "reps": a.reps}, a.out)
    if a.section == "all":   # each EMD step in a fresh process with a time limit of its own; a step that fails ends the run
        import subprocess
        for sec in ("emd30", "emd150"):
            subprocess.run([sys.executable, os.path.abspath(__file__), "--section", sec, "--reps", str(a.reps), "--out", a.out],
                           check=True, timeout=a.emd_timeout)
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
