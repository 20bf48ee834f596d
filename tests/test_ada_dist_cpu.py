"""CPU: the adaptive augmentation probability across data-parallel ranks -- ``mpg_ada_count`` + ``mpg_ada_settle`` (their bodies
compiled for the host) against ``mpg_ada_update_host`` bit for bit, with the outputs split over W ranks and the ranks' slots added
in fp32; the settle's answer to a broken collective; and ``TrainStep`` on toy networks over gloo: two ranks settle ONE
probability, the one ``ada_rule`` gives on the outputs of both."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from spawn_util import spawn_joined
from test_ada_cpu import ADA, _bits, host_update
from test_dist_cpu import ToyG, _torch_rmsprop, _inputs, N, LAT
from test_labels_cpu import LabelFreeD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
CATALOGUE = [(n, W, interval) for n in (1, 5, 65) for W in (1, 2, 3) for interval in (1, 4)]
STEPS = 12


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def host_count(out, n_real, mid):
    """``mpg_ada_count_host`` on a float32 array: (code, the slot as np.float32; 7.25 where the call stored nothing)."""
    from mpgan_amd import _lib
    o, slot = np.ascontiguousarray(out, dtype=np.float32), np.array([7.25], dtype=np.float32)
    code = _lib.lib().mpg_ada_count_host(_ptr(o), n_real, float(mid), _ptr(slot))
    return code, slot[0]


def host_settle(slot, n_total, target, step, interval, state, p, r):
    """``mpg_ada_settle_host``: (code, state, p, r) afterwards."""
    from mpgan_amd import _lib
    sl = np.array([slot], dtype=np.float32)
    st, pp, rr = np.array(state, dtype=np.int32), np.array([p], dtype=np.float32), np.array([r], dtype=np.float32)
    code = _lib.lib().mpg_ada_settle_host(_ptr(sl), n_total, float(target), float(step), interval, _ptr(st), _ptr(pp), _ptr(rr))
    return code, (int(st[0]), int(st[1])), pp[0], rr[0]


def step_outputs(n_total, t, mid, seed):
    """D's outputs of all ranks at step ``t`` of ``STEPS``: they drift from mostly below ``mid`` to mostly above it, with exact
    ties at ``mid``, a NaN and both infinities planted where there is room."""
    g = np.random.default_rng(seed * 1000 + t)
    drift = F32(-0.35 + 0.7 * t / (STEPS - 1))
    o = (g.random(n_total, dtype=np.float32) - F32(0.5) + drift + F32(mid)).astype(np.float32)
    o[g.integers(0, n_total, size=max(1, n_total // 6))] = mid
    if n_total >= 3:
        o[int(g.integers(0, n_total))] = np.nan
    if n_total >= 5:
        i, j = g.choice(n_total, size=2, replace=False)
        o[i], o[j] = np.inf, -np.inf
    return o


@pytest.mark.parametrize("n,W,interval", CATALOGUE)
def test_count_then_settle_is_update_bit_for_bit(n, W, interval):
    """After each of 12 steps: the W ranks' counts, added with torch.sum in fp32, settled with n W jets == one update of all."""
    mid, target, step = F32(0.5), F32(0.1), F32(0.07)
    one = split = ((0, 0), F32(0.3), F32(0))
    moved = False
    for t in range(STEPS):
        o = step_outputs(n * W, t, mid, seed=n * 10 + W)
        code, *one = host_update(o, n * W, mid, target, step, interval, *one)
        assert code == 0
        slots = []
        for r in range(W):
            code, slot = host_count(o[r * n:(r + 1) * n], n, mid)
            assert code == 0 and float(slot) == int(slot) and abs(int(slot)) <= n
            slots.append(slot)
        total = torch.sum(torch.tensor(np.array(slots, dtype=np.float32)))
        assert total.dtype == torch.float32
        code, *split = host_settle(float(total), n * W, target, step, interval, *split)
        assert code == 0
        assert split[0] == one[0] and _bits(split[1]) == _bits(one[1]) and _bits(split[2]) == _bits(one[2]), (t, split, one)
        moved |= _bits(one[1]) != _bits(F32(0.3))
    assert moved      # (the catalogue moves p: the comparison is not one of untouched words)


def test_the_count_is_a_store_and_counts_ties_and_nans_on_neither_side():
    o = np.array([0.5, np.nan, 0.75, 0.25, 0.25, np.inf, -np.inf, 0.5], dtype=np.float32)
    code, slot = host_count(o, 8, 0.5)
    assert code == 0 and float(slot) == -1.0       # (2 above, 3 below; the 7.25 the slot held is gone)
    assert host_count(o, 3, 0.5)[1] == 1.0


@pytest.mark.parametrize("slot", [0.5, float("nan"), 11.0, -11.0, float("inf")])
def test_a_broken_slot_moves_nothing_and_gives_r_nan(slot):
    """10 real jets in all: a fraction, a NaN and n_total + 1 are not sign counts of 10 jets -- the collective is broken."""
    for interval, state in ((1, (0, 0)), (4, (3, 3)), (4, (-2, 1))):
        code, st, p, r = host_settle(slot, 10, 0.5, 0.125, interval, state, F32(0.25), F32(0.75))
        assert code == 0 and st == state and _bits(p) == _bits(F32(0.25)) and np.isnan(r)
    # (and the edge itself is a count: all ten on one side)
    code, st, p, r = host_settle(-10.0, 10, 0.5, 0.125, 1, (0, 0), F32(0.25), F32(0.75))
    assert code == 0 and st == (0, 0) and p == F32(0.125) and r == F32(-1)


def test_refusals_of_the_two_entries():
    from mpgan_amd import _lib
    L = _lib.lib()
    o, one, st = np.zeros(4, dtype=np.float32), np.zeros(1, dtype=np.float32), np.zeros(2, dtype=np.int32)
    assert L.mpg_ada_count_host(_ptr(o), (1 << 24) + 1, 0.5, _ptr(one)) == -1
    assert L.mpg_ada_count_host(_ptr(o), 0, 0.5, _ptr(one)) == -1
    assert L.mpg_ada_count_host(None, 4, 0.5, _ptr(one)) == -1 and L.mpg_ada_count_host(_ptr(o), 4, 0.5, None) == -1
    assert L.mpg_ada_count(None, 4, 0.5, None, None) == -1                       # (refused before any launch)
    ok = lambda **kw: L.mpg_ada_settle_host(_ptr(one), kw.get("n", 8), kw.get("target", 0.5), kw.get("step", 0.1), kw.get("interval", 2),
                                            _ptr(st), _ptr(one), _ptr(one))
    assert ok() == 0
    assert ok(n=0) == -1 and ok(interval=0) == -1 and ok(target=1.5) == -1 and ok(step=-0.1) == -1
    assert ok(n=1 << 30, interval=2) == -1                                       # (the int32 check applies to the total)
    assert L.mpg_ada_settle(None, 8, 0.5, 0.1, 2, None, None, None, None) == -1


def test_python_halves_are_the_rule():
    """``ada_rule`` is ``ada_count_rule`` then ``ada_settle_rule``, and agrees with the host twins."""
    from mpgan_amd import step_options as so
    state = (0, 0, 0.3, 0.0)
    host = ((0, 0), F32(0.3), F32(0))
    for t in range(STEPS):
        o = step_outputs(13, t, 0.5, seed=5)
        s = so.ada_count_rule(torch.from_numpy(o), 13, 0.5)
        assert float(host_count(o, 13, 0.5)[1]) == s
        halves = so.ada_settle_rule(float(s), 13, 0.1, float(F32(0.07)), 4, *state)
        state = so.ada_rule(torch.from_numpy(o), 13, 0.5, 0.1, float(F32(0.07)), 4, *state)
        assert halves[:3] == state[:3] and _bits(halves[3]) == _bits(state[3])
        _, *host = host_update(o, 13, 0.5, F32(0.1), F32(0.07), 4, *host)
        assert (state[0], state[1]) == host[0] and _bits(state[2]) == _bits(host[1]) and _bits(state[3]) == _bits(host[2])
    assert np.isnan(so.ada_settle_rule(0.5, 13, 0.1, 0.07, 4, 2, 1, 0.3, 0.0)[3])


# ---- TrainStep over gloo ---------------------------------------------------------------------------------------------------------
B_RANK, STEPS_DIST = 4, 5


def _ada_step(rank, world, pg, **kw):
    from mpgan_amd import train
    torch.manual_seed(3)       # (every rank the same weights)
    G, D = ToyG(), LabelFreeD()
    data, labels, nD, nG = _inputs(B_RANK * world)
    sl = slice(rank * B_RANK, (rank + 1) * B_RANK)
    ts = train.TrainStep(G, D, B_RANK, N, latent=LAT, lr_disc=1e-2, lr_gen=2e-2, use_graphs=False, augment=train.Augment(**ADA),
                         process_group=pg, world_size=world, **kw)
    ts.set_batch(data[sl], labels[sl])
    ts.fixed_noise = (nD[sl], nG[sl])
    ts.ada_keep_out = True
    return ts


def _ada_worker(rank, world, port, out):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    from mpgan_amd import dist as mdist, train
    r, w, pg = mdist.init_from_env("gloo")
    train.FlatParams.step = _torch_rmsprop      # (in this child alone: libmpgan_amd has no CPU optimizer)
    ts = _ada_step(rank, world, pg)
    torch.manual_seed(50 + rank)      # (the augmentation draws differ between the ranks)
    assert ts._ada.split and ts.fD.grad_all.numel() == ts.fD.n + 1 and ts.fD.grad.numel() == ts.fD.n
    trace = []
    for _ in range(STEPS_DIST):
        ts.step()
        trace.append((ts.ada, ts.ada_last_out.detach().reshape(-1)[:B_RANK].clone()))
    out[rank] = (trace, ts._ada.step, ts._ada.n_total, ts.fD.flat.clone())
    dist.destroy_process_group()


def test_two_ranks_settle_one_probability_over_gloo():
    """5 steps at interval 2: both ranks hold the same {p, r, sign_sum, steps} after every step, and it is ``ada_rule`` replayed
    over the outputs of both ranks' real jets.  (On one rank's own outputs the ranks would drift apart.)"""
    world = 2
    out = mp.get_context("spawn").Manager().dict()
    spawn_joined(_ada_worker, (world, 29571, out), world)
    (tr0, step, n_total, fD0), (tr1, step1, _, fD1) = out[0], out[1]
    from mpgan_amd import step_options as so
    assert n_total == world * B_RANK and step == step1
    assert _bits(step) == _bits(F32(world * B_RANK * ADA["ada_interval"] / (1000.0 * ADA["ada_kimg"])))
    assert torch.equal(fD0, fD1)
    state, moved = (0, 0, ADA["aug_prob"], 0.0), False
    for (ada0, o0), (ada1, o1) in zip(tr0, tr1):
        assert ada0 == ada1
        state = so.ada_rule(torch.cat([o0, o1]), n_total, 0.5, float(F32(ADA["ada_target"])), step, ADA["ada_interval"], *state)
        assert ada0 == {"p": state[2], "r": state[3], "sign_sum": state[0], "steps": state[1]}
        moved |= ada0["p"] != ADA["aug_prob"]
    assert moved and tr0[-1][0]["steps"] == STEPS_DIST % ADA["ada_interval"]


@pytest.mark.parametrize("schedule", [{}, {"num_critic": 3}, {"num_gen": 2}], ids=["DG", "num_critic3", "num_gen2"])
def test_one_rank_split_route_equals_the_one_launch_route(schedule, monkeypatch):
    """``_ada_split=True`` on one rank: the two halves around D's (absent) all-reduce leave what the one launch leaves -- on D+G
    batches, on D-only batches (the settle sits in front of D's closing optimizer step) and across G-only ones --, and the slot
    rides at the tail of D's gradient buffer without being a gradient; a checkpoint moves between the routes."""
    from mpgan_amd import train
    monkeypatch.setattr(train.FlatParams, "step", _torch_rmsprop)
    runs = []
    for split in (False, True):
        torch.manual_seed(9)
        ts = _ada_step(0, 1, None, _ada_split=split, **schedule)
        assert ts._ada.split is split and ts.fD.grad_all.numel() == ts.fD.n + int(split)
        assert (ts.fD.tail is None) == (not split) and ts.fD.grad.data_ptr() == ts.fD.grad_all.data_ptr()
        trace = []
        for _ in range(STEPS_DIST):
            ts.step()
            trace.append(ts.ada)
        runs.append((trace, ts.fD.flat.clone(), ts.fG.flat.clone(), ts))
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])
    assert float(runs[1][3].fD.tail) == int(float(runs[1][3].fD.tail))       # (the last count, still in the slot)
    # the slot is transient: the files are the same and load either way
    sd_one, sd_split = runs[0][3].optimizer_state_dicts(), runs[1][3].optimizer_state_dicts()
    assert sd_one[0]["param_groups"][0][train.FlatParams.ADA_KEY] == sd_split[0]["param_groups"][0][train.FlatParams.ADA_KEY]
    runs[0][3].load_optimizer_state_dicts(*sd_split)
    runs[1][3].load_optimizer_state_dicts(*sd_one)
    assert runs[0][3].ada == runs[1][3].ada == runs[0][0][-1]


def test_refusals_of_the_step():
    from mpgan_amd import train
    with pytest.raises(ValueError, match="drift apart"):
        _ada_step(0, 2, None)
    with pytest.raises(ValueError, match="2\\^24"):
        train.AdaController.from_args(train.Augment(**ADA), torch.zeros(1), "ls", (1 << 23) + 1, 2, process_group=object())
    with pytest.raises(ValueError, match="int32"):
        train.AdaController.from_args(train.Augment(**dict(ADA, ada_interval=256)), torch.zeros(1), "ls", 1 << 23, 2,
                                      process_group=object())
