"""CPU: the adaptive augmentation probability (``Augment.adaptive_prob``) -- the rule of ``mpg_ada_update`` restated in numpy from
include/mpgan_amd.h (``restate`` below; the reference names the option and never implements it, so this restatement is the
specification) against ``mpg_ada_update_host``, the kernel's own body compiled for the host, bit for bit; the C ABI's refusals;
``train.Augment``'s new fields; and the host logic of ``TrainStep`` on toy networks: trajectory, resume, refusals."""
import ctypes as C
import copy
import re
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from test_dist_cpu import ToyG, _torch_rmsprop, _inputs, N, LAT
from test_labels_cpu import LabelFreeD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mpgan_amd.h")

N_REAL = (1, 2, 63, 64, 65, 255, 256, 257, 515)      # one jet, the wave's edges, the workgroup's edges, more jets than threads
F32 = np.float32


def restate(out, n_real, mid, target, step, interval, state, p, r):
    """One launch of ``mpg_ada_update`` as include/mpgan_amd.h states it: (state, p, r) afterwards.  ``out``: float32 array;
    ``state``: (sign sum, D steps counted) as Python integers; ``mid``, ``target``, ``step``, ``p``, ``r``: np.float32."""
    o = out[:n_real]
    s = int(np.count_nonzero(o > mid)) - int(np.count_nonzero(o < mid))       # (a NaN fails both comparisons)
    sign_sum, steps = state[0] + s, state[1] + 1
    if steps != interval:
        return (sign_sum, steps), p, r
    r = F32(sign_sum) / F32(n_real * interval)                                # two conversions, one fp32 division
    assert r.dtype == np.float32
    if r > target:
        p = p + step                                                          # one fp32 sum
    elif r < target:
        p = p - step
    assert p.dtype == np.float32
    p = F32(0) if p < 0 else (F32(1) if p > 1 else p)
    return (0, 0), p, r


def host_update(out, n_real, mid, target, step, interval, state, p, r):
    """The same through ``mpg_ada_update_host``; returns (code, state, p, r)."""
    from mpgan_amd import _lib
    o = np.ascontiguousarray(out, dtype=np.float32)
    st, pp, rr = np.array(state, dtype=np.int32), np.array([p], dtype=np.float32), np.array([r], dtype=np.float32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    code = _lib.lib().mpg_ada_update_host(ptr(o), n_real, float(mid), float(target), float(step), interval, ptr(st), ptr(pp), ptr(rr))
    return code, (int(st[0]), int(st[1])), pp[0], rr[0]


def _bits(v):
    return np.asarray(v, dtype=np.float32).view(np.uint32).item()


def _same(got, want):
    (gs, gp, gr), (ws, wp, wr) = got, want
    return gs == ws and _bits(gp) == _bits(wp) and _bits(gr) == _bits(wr)


def outputs(n, seed, mid=0.5, nan=True):
    """D's outputs for n jets: uniform around ``mid``, with values exactly equal to ``mid`` planted (and one NaN)."""
    g = np.random.default_rng(seed)
    o = (g.random(n, dtype=np.float32) - F32(0.45) + F32(mid)).astype(np.float32)
    o[g.integers(0, n, size=max(1, n // 7))] = mid
    if nan and n > 2:
        o[int(g.integers(0, n))] = np.nan
    return o


def test_symbols_are_exported_with_the_documented_signature():
    from mpgan_amd import _lib
    lib = _lib.lib()
    txt = open(HEADER).read()
    names = ["out", "n_real", "mid", "target", "step", "interval", "state", "aug_p", "r_out"]
    for sym, tail in (("mpg_ada_update", ["stream"]), ("mpg_ada_update_host", [])):
        assert hasattr(lib, sym)
        decl = re.search(r"^int\s+" + sym + r"\s*\(([^;]*)\);", txt, flags=re.M | re.S).group(1)
        assert [a.split()[-1].lstrip("*") for a in decl.split(",")] == names + tail
        res, args = _lib.SIGNATURES[sym]
        assert res is C.c_int and len(args) == len(names) + len(tail)
        assert args[1] is C.c_int and args[2:5] == [C.c_float] * 3 and args[5] is C.c_int


@pytest.mark.parametrize("interval", [1, 4])
@pytest.mark.parametrize("n_real", N_REAL)
def test_host_twin_against_the_restatement(n_real, interval):
    """``interval`` launches on one state from p = 0.5 (so that the last one closes the interval), outputs with planted ``mid``
    values and a NaN: state, p and r after every launch, bit for bit."""
    mid, target, step = F32(0.5), F32(0.6), F32(0.01)
    state, p, r = (0, 0), F32(0.5), F32(0)
    for k in range(interval):
        o = outputs(n_real, 100 * n_real + k)
        want = restate(o, n_real, mid, target, step, interval, state, p, r)
        code, *got = host_update(o, n_real, mid, target, step, interval, state, p, r)
        assert code == 0 and _same(got, want), (k, got, want)
        state, p, r = want
    assert state == (0, 0) and _bits(p) != _bits(F32(0.5)) and abs(float(r)) <= 1.0


def test_mid_and_nan_count_on_neither_side():
    o = np.array([0.5, 0.5, np.nan, 0.75, 0.5, 0.25, 0.75], dtype=np.float32)      # two above, one below
    code, state, p, r = host_update(o, 7, 0.5, 0.6, 0.01, 2, (0, 0), 0.3, 0.0)
    assert code == 0 and state == (1, 1) and _bits(p) == _bits(F32(0.3)) and r == 0
    assert _same((state, p, r), restate(o, 7, F32(0.5), F32(0.6), F32(0.01), 2, (0, 0), F32(0.3), F32(0)))
    o[:] = 0.5
    code, state, p, r = host_update(o, 7, 0.5, 0.6, 0.01, 1, (0, 0), 0.3, 0.0)     # r = 0 < target: down
    assert code == 0 and state == (0, 0) and r == 0 and _bits(p) == _bits(F32(0.3) - F32(0.01))


@pytest.mark.parametrize("n_real", [1, 65, 515])
def test_all_above_and_all_below(n_real):
    for fill, want_r in ((0.9, 1.0), (0.1, -1.0)):
        o = np.full(n_real, fill, dtype=np.float32)
        state, p, r = (0, 0), F32(0.5), F32(0)
        for _ in range(4):
            code, state, p, r = host_update(o, n_real, 0.5, 0.6, 0.125, 4, state, p, r)
            assert code == 0
        assert state == (0, 0) and float(r) == want_r and float(p) == 0.5 + 0.125 * want_r


def test_r_equal_to_the_target_leaves_p():
    """3 of 4 above, 1 below: r = 2 / 4 = 0.5 = target exactly; p must not move (and does with any other target)."""
    o = np.array([0.9, 0.8, 0.7, 0.2], dtype=np.float32)
    p0 = F32(0.37)
    code, state, p, r = host_update(o, 4, 0.5, 0.5, 0.01, 1, (0, 0), p0, 0.0)
    assert code == 0 and state == (0, 0) and float(r) == 0.5 and _bits(p) == _bits(p0)
    assert _same((state, p, r), restate(o, 4, F32(0.5), F32(0.5), F32(0.01), 1, (0, 0), p0, F32(0)))
    assert float(host_update(o, 4, 0.5, 0.25, 0.01, 1, (0, 0), p0, 0.0)[2]) > float(p0)
    assert float(host_update(o, 4, 0.5, 0.75, 0.01, 1, (0, 0), p0, 0.0)[2]) < float(p0)


def test_both_clamps():
    up, down = np.full(5, 0.9, dtype=np.float32), np.full(5, 0.1, dtype=np.float32)
    for o, p0, end in ((up, 0.999, 1.0), (down, 0.001, 0.0)):
        want = restate(o, 5, F32(0.5), F32(0.6), F32(0.01), 1, (0, 0), F32(p0), F32(0))
        code, *got = host_update(o, 5, 0.5, 0.6, 0.01, 1, (0, 0), p0, 0.0)
        assert code == 0 and _same(got, want) and float(got[1]) == end
        code, *again = host_update(o, 5, 0.5, 0.6, 0.01, 1, got[0], got[1], got[2])     # and stays there
        assert code == 0 and float(again[1]) == end


def test_twelve_launches_at_interval_four():
    """Three intervals on one state, compared launch by launch; the outputs drift from mostly below to mostly above ``mid``."""
    n, mid, target, step = 65, F32(0.0), F32(0.6), F32(0.03)
    state, p, r = (0, 0), F32(0.05), F32(0)
    seen = []
    for k in range(12):
        o = (outputs(n, 7 + k, mid=0.0) + F32(0.12 * (k // 4) - 0.1)).astype(np.float32)
        want = restate(o, n, mid, target, step, 4, state, p, r)
        code, *got = host_update(o, n, mid, target, step, 4, state, p, r)
        assert code == 0 and _same(got, want), (k, got, want)
        state, p, r = want
        assert state[1] == (k + 1) % 4
        seen.append(float(p))
    assert len(set(seen)) >= 3 and seen[0] == seen[2] != seen[3]      # (p moves at launches 3, 7, 11 only)


def test_refusals_of_the_c_abi():
    o = np.zeros(4, dtype=np.float32)
    ok = dict(out=o, n_real=4, mid=0.5, target=0.6, step=0.01, interval=2, state=(0, 0), p=0.5, r=0.0)
    assert host_update(**ok)[0] == 0
    for bad in (dict(n_real=0), dict(n_real=2**30 + 1), dict(interval=0), dict(n_real=2**30, interval=2), dict(target=-0.1),
                dict(target=1.5), dict(target=float("nan")), dict(step=-1.0), dict(step=float("nan"))):
        assert host_update(**dict(ok, **bad))[0] == -1, bad      # (refused before anything is read)
    from mpgan_amd import _lib
    L = _lib.lib()
    st, one = np.zeros(2, dtype=np.int32), np.zeros(1, dtype=np.float32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.mpg_ada_update_host(None, 4, 0.5, 0.6, 0.01, 2, ptr(st), ptr(one), ptr(one)) == -1
    assert L.mpg_ada_update_host(ptr(o), 4, 0.5, 0.6, 0.01, 2, None, ptr(one), ptr(one)) == -1
    assert L.mpg_ada_update_host(ptr(o), 4, 0.5, 0.6, 0.01, 2, ptr(st), None, ptr(one)) == -1
    assert L.mpg_ada_update_host(ptr(o), 4, 0.5, 0.6, 0.01, 2, ptr(st), ptr(one), None) == -1
    assert L.mpg_ada_update(None, 4, 0.5, 0.6, 0.01, 2, None, None, None, None) == -1      # (refused before any launch)


def test_ops_refuses_host_tensors_and_bad_arguments():
    from mpgan_amd import ops
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.ada_update(torch.zeros(4), 4, 0.5, 0.6, 0.01, 2, torch.zeros(2, dtype=torch.int32), torch.zeros(1), torch.zeros(1))


# ---- train.Augment --------------------------------------------------------------------------------------------------------------
def test_augment_defaults_are_adas_published_ones():
    from mpgan_amd import train
    a = train.Augment()
    assert (a.adaptive_prob, a.ada_target, a.ada_interval, a.ada_kimg) == (False, 0.6, 4, 500.0)
    assert a.aug_prob == 1.0                                   # (the fixed-probability default is left alone)
    assert train.ADA_DEFAULTS == {"ada_target": 0.6, "ada_interval": 4, "ada_kimg": 500.0}
    a = train.Augment(aug_t=True, adaptive_prob=True, aug_prob=0.0, ada_target=0.5, ada_interval=2, ada_kimg=0.128)
    assert a.adaptive_prob and a.ada_interval == 2


# ---- TrainStep on the CPU ------------------------------------------------------------------------------------------------------
B_TOY = 4
ADA = dict(aug_t=True, aug_f=True, adaptive_prob=True, aug_prob=0.25, ada_target=0.5, ada_interval=2, ada_kimg=0.064)


def _toy_step(augment, seed=3, **kw):
    from mpgan_amd import train
    torch.manual_seed(seed)
    G, D = ToyG(), LabelFreeD()
    data, labels, nD, nG = _inputs(B_TOY)
    ts = train.TrainStep(G, D, B_TOY, N, latent=LAT, lr_disc=1e-2, lr_gen=2e-2, use_graphs=False, augment=augment, **kw)
    ts.set_batch(data, labels)
    ts.fixed_noise = (nD, nG)
    return ts


def test_reference_namespace_without_the_ada_fields_gets_the_defaults():
    from mpgan_amd import train
    ns = SimpleNamespace(aug_r90=False, aug_f=True, aug_t=True, aug_s=False, translate_ratio=0.125, scale_sd=0.125, aug_prob=0.0,
                         adaptive_prob=True)
    ts = _toy_step(ns)
    a = ts._ada
    assert (a.target, a.interval, a.mid) == (float(F32(0.6)), 4, 0.5)
    assert _bits(a.step) == _bits(F32(B_TOY * 4 / (1000 * 500.0))) and float(F32(a.step)) == a.step
    assert ts.ada == {"p": 0.0, "r": 0.0, "sign_sum": 0, "steps": 0}
    ns.ada_target, ns.ada_interval, ns.ada_kimg = 0.75, 3, 1.0
    a = _toy_step(ns)._ada
    assert (a.target, a.interval) == (0.75, 3) and _bits(a.step) == _bits(F32(B_TOY * 3 / 1000.0))
    assert _toy_step(ns, loss="w")._ada.mid == 0.0 and _toy_step(ns, loss="hinge")._ada.mid == 0.0 and _toy_step(ns, loss="og")._ada.mid == 0.5


def test_refusals_and_the_switches_off():
    from mpgan_amd import train
    with pytest.raises(ValueError, match="drift apart"):
        _toy_step(train.Augment(**ADA), world_size=2)
    for bad in (dict(ada_interval=0), dict(ada_interval=2.0), dict(ada_target=1.5), dict(ada_kimg=0.0)):
        with pytest.raises(ValueError, match=next(iter(bad))):
            _toy_step(train.Augment(**dict(ADA, **bad)))
    # all four switches off: adaptive_prob does nothing, as Augment without switches does nothing today
    off = _toy_step(train.Augment(adaptive_prob=True, aug_prob=0.25), world_size=1)
    assert off.aug is None and off._ada is None and off.ada_state is None and off.fD.carried == []
    with pytest.raises(RuntimeError, match="adaptive_prob"):
        off.ada
    fixed = _toy_step(train.Augment(aug_t=True, aug_prob=0.25))
    assert fixed.aug is not None and fixed._ada is None and train.FlatParams.ADA_KEY not in fixed.optimizer_state_dicts()[0]["param_groups"][0]


def _trajectory(ts, steps, ps=None):
    outs = []
    for _ in range(steps):
        ts.step()
        outs.append(ts.ada_last_out.detach().reshape(-1).numpy().copy())
        if ps is not None:
            ps.append(ts.ada)
    return outs


def test_cpu_step_follows_the_restatement_over_nine_steps(monkeypatch):
    from mpgan_amd import train
    monkeypatch.setattr(train.FlatParams, "step", _torch_rmsprop)
    ts = _toy_step(train.Augment(**ADA))
    assert ts._route() == "module" and _bits(ts._ada.step) == _bits(F32(0.125))
    ts.ada_keep_out = True
    torch.manual_seed(11)
    seen = []
    outs = _trajectory(ts, 9, seen)
    state, p, r = (0, 0), F32(0.25), F32(0)
    for k, (o, got) in enumerate(zip(outs, seen)):
        assert o.shape == (2 * B_TOY,) and o.dtype == np.float32
        state, p, r = restate(o, B_TOY, F32(0.5), F32(0.5), F32(0.125), 2, state, p, r)
        assert got == {"p": float(p), "r": float(r), "sign_sum": state[0], "steps": state[1]}, (k, got, state, p, r)
    assert seen[-1]["steps"] == 1 and len({s["p"] for s in seen}) >= 3          # (nine D steps: four intervals and a half)
    ts.set_aug_prob(0.5)                                                        # overwritten: the controller goes on from there
    ts.step()
    state, p, r = restate(ts.ada_last_out.reshape(-1).numpy(), B_TOY, F32(0.5), F32(0.5), F32(0.125), 2, state, F32(0.5), r)
    assert ts.ada == {"p": float(p), "r": float(r), "sign_sum": 0, "steps": 0} and float(p) in (0.375, 0.5, 0.625)


def test_gradient_penalty_route_updates_behind_the_real_batchs_augmentation(monkeypatch):
    """gp_lambda > 0: the D step augments the real batch for the penalty (site D_real) behind D's two passes.  From p = 0 with
    every real jet above ``mid`` (target 0) the interval closes on the first D step and p becomes 0.125; the D step's own
    launches -- D_real among them -- must have read the old p = 0, which takes no augmentation, and train_G's the new one."""
    from mpgan_amd import train
    monkeypatch.setattr(train.FlatParams, "step", _torch_rmsprop)
    ts = _toy_step(train.Augment(**dict(ADA, aug_prob=0.0, ada_target=0.0, ada_interval=1, ada_kimg=0.032)), gp_lambda=1.0)
    seen = []
    real_aug = ts._augment
    monkeypatch.setattr(ts, "_augment", lambda x, site, in_place=False: (seen.append((site, float(ts.aug_p))), real_aug(x, site, in_place))[1])
    ts.fixed_alpha = torch.rand(B_TOY, 1, 1, generator=torch.Generator().manual_seed(2))
    ts.step()
    sites = train.AUG_SITES
    assert [s for s, _ in seen] == [sites["D_fake"], sites["D_real"], sites["G_fake"]]
    p_new = ts.ada["p"]
    assert [p for _, p in seen] == [0.0, 0.0, p_new] and p_new in (0.0, 0.125)
    assert ts.ada["steps"] == 0 and abs(ts.ada["r"]) <= 1.0


def _save(ts):
    sd_D, sd_G = ts.optimizer_state_dicts()
    return copy.deepcopy((ts.D.state_dict(), ts.G.state_dict(), sd_D, sd_G, torch.get_rng_state()))


def _resume(saved, drop_entry=False):
    from mpgan_amd import train
    d, g, sd_D, sd_G, rng = copy.deepcopy(saved)
    if drop_entry:
        del sd_D["param_groups"][0][train.FlatParams.ADA_KEY]
    ts = _toy_step(train.Augment(**ADA), seed=99)          # other weights: everything comes from what was saved
    ts.D.load_state_dict(d)
    ts.G.load_state_dict(g)
    ts.load_optimizer_state_dicts(sd_D, sd_G)
    torch.set_rng_state(rng)
    return ts


def test_resume_in_mid_interval_equals_the_uninterrupted_run(monkeypatch):
    from mpgan_amd import train
    monkeypatch.setattr(train.FlatParams, "step", _torch_rmsprop)
    ts = _toy_step(train.Augment(**ADA))
    torch.manual_seed(11)
    for _ in range(3):
        ts.step()
    saved = _save(ts)
    entry = saved[2]["param_groups"][0][train.FlatParams.ADA_KEY]
    assert entry == ts.ada and entry["steps"] == 1            # in the middle of the second interval
    for _ in range(4):
        ts.step()
    again = _resume(saved)
    assert again.ada == entry
    for _ in range(4):
        again.step()
    assert again.ada == ts.ada
    assert torch.equal(again.fD.flat, ts.fD.flat) and torch.equal(again.fG.flat, ts.fG.flat)
    # a file without the entry: the starting probability and an empty interval, whatever the step held
    bare = _resume(saved, drop_entry=True)
    assert bare.ada == {"p": 0.25, "r": 0.0, "sign_sum": 0, "steps": 0}
    with pytest.raises(ValueError, match="interval"):
        bad = copy.deepcopy(saved)
        bad[2]["param_groups"][0][train.FlatParams.ADA_KEY]["steps"] = 2
        _resume(bad)
