"""GPU: the adaptive augmentation probability across data-parallel ranks -- ``ops.ada_count`` and ``ops.ada_settle`` against
their host twins and against ``ops.ada_update`` bit for bit, the settle's answer to a broken slot, ``TrainStep`` on the split
route on one rank (eager, captured, and against the one-launch route), and two ranks on the one GPU over gloo that settle ONE
probability: the one ``ada_rule`` gives on the outputs of both."""
import os
import sys

import numpy as np
import pytest
import torch

from spawn_util import spawn_joined
from test_ada_cpu import F32, _bits, _same
from test_ada_dist_cpu import CATALOGUE, STEPS, host_count, host_settle, step_outputs
from test_gpu_ada import _read, _words
from test_gpu_augment import _reset_tags
from test_gpu_schedule import _all_equal, _device_seed, _state, _step

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# n = 257 per rank: more than one stride of the 256 threads, all four waves' LDS words in use
DEVICE_CATALOGUE = CATALOGUE + [(257, 1, 4), (257, 2, 1)]


@pytest.mark.parametrize("n,W,interval", DEVICE_CATALOGUE)
def test_count_and_settle_against_the_host_twins_and_the_one_launch(n, W, interval):
    """12 steps on one state: every rank's count against ``mpg_ada_count_host``, the settle of their fp32 sum (torch.sum on the
    device) against ``mpg_ada_settle_host``, and both against ``ops.ada_update`` of all n W outputs -- state as integers, p and r
    as bit patterns, after every step."""
    from mpgan_amd import ops
    mid, target, step = F32(0.5), F32(0.1), F32(0.07)
    one, split = _words((0, 0), 0.3, 0.0), _words((0, 0), 0.3, 0.0)
    host = ((0, 0), F32(0.3), F32(0))
    slots = torch.full((W,), 7.25, device="cuda")
    moved = False
    for t in range(STEPS):
        o = step_outputs(n * W, t, mid, seed=n * 10 + W)
        out = torch.from_numpy(np.concatenate([o, np.full(3, 0.9, dtype=np.float32)])).cuda()   # (a read past the n W would show)
        ops.ada_update(out, n * W, mid, target, step, interval, *one)
        want_slots = []
        for r in range(W):
            ops.ada_count(out[r * n:], n, mid, slots[r:r + 1])
            want_slots.append(host_count(o[r * n:(r + 1) * n], n, mid)[1])
        total = torch.sum(slots).reshape(1)
        assert total.dtype == torch.float32
        ops.ada_settle(total, n * W, target, step, interval, *split)
        code, *host = host_settle(float(torch.sum(torch.tensor(np.array(want_slots, dtype=np.float32)))), n * W, target, step, interval,
                                  *host)
        got_one, got_split = _read(*one), _read(*split)
        assert slots.cpu().numpy().tolist() == [float(s) for s in want_slots], t
        assert code == 0 and _same(got_split, tuple(host)), (t, got_split, host)
        assert _same(got_split, got_one), (t, got_split, got_one)
        moved |= _bits(got_split[1]) != _bits(F32(0.3))
    assert moved      # (the catalogue moves p: the comparison is not one of untouched words)


@pytest.mark.parametrize("slot", [0.5, float("nan"), 11.0, -11.0, float("inf")])
def test_a_broken_slot_on_the_device(slot):
    from mpgan_amd import ops
    for interval, state in ((1, (0, 0)), (4, (3, 3))):
        st, p, r = _words(state, 0.25, 0.75)
        ops.ada_settle(torch.tensor([slot], device="cuda"), 10, 0.5, 0.125, interval, st, p, r)
        got = _read(st, p, r)
        assert got[0] == state and _bits(got[1]) == _bits(F32(0.25)) and np.isnan(got[2]), (interval, got)
        want = host_settle(slot, 10, 0.5, 0.125, interval, state, F32(0.25), F32(0.75))
        assert want[1] == got[0] and _bits(want[2]) == _bits(got[1]) and np.isnan(want[3])


def test_argument_checks():
    from mpgan_amd import ops
    out, slot = torch.zeros(8, device="cuda"), torch.full((1,), 7.25, device="cuda")
    st, p, r = _words((0, 0), 0.5, 0.0)
    for bad in (dict(n_real=9), dict(n_real=0), dict(slot=torch.zeros(2, device="cuda")), dict(slot=torch.zeros(1)),
                dict(slot=slot.double()), dict(out=torch.zeros(8, 2, device="cuda")[:, 0])):
        with pytest.raises(ValueError):
            ops.ada_count(**dict(dict(out=out, n_real=8, mid=0.5, slot=slot), **bad))
    ok = dict(slot=slot, n_real_total=8, target=0.6, step=0.01, interval=2, state=st, aug_p=p, r_out=r)
    for bad in (dict(n_real_total=0), dict(interval=0), dict(n_real_total=2**30, interval=2), dict(target=1.5), dict(step=-0.01),
                dict(step=float("nan")), dict(state=st.float()), dict(aug_p=torch.zeros(2, device="cuda")), dict(r_out=torch.zeros(1)),
                dict(slot=torch.zeros(2, device="cuda"))):
        with pytest.raises(ValueError):
            ops.ada_settle(**dict(ok, **bad))
    torch.cuda.synchronize()
    assert st.tolist() == [0, 0] and float(p) == 0.5 and float(slot) == 7.25          # (nothing was launched)


# ---- the step ------------------------------------------------------------------------------------------------------------------
B = 8
# B * ada_interval / (1000 * ada_kimg) = 16 / 128 = 0.125 exactly
ADA = dict(aug_t=True, aug_f=True, adaptive_prob=True, aug_prob=0.25, ada_target=0.5, ada_interval=2, ada_kimg=0.128)


def _run_split(split, use_graphs, steps=4, n_graphs=1, **kw):
    from mpgan_amd import train
    with _device_seed() as seed:
        seed()
        ts = _step("mpgan", B, disc_dropout=0.0, augment=train.Augment(**ADA), fixed=True, use_graphs=use_graphs, _ada_split=split,
                   **kw)
        assert ts._route() != "module" and ts._ada.split is split and ts.fD.grad_all.numel() == ts.fD.n + int(split)
        if use_graphs:
            _reset_tags()
            ts.capture(warmup=0)
            assert len(ts._graphs) == n_graphs
        seen = []
        for _ in range(steps):
            if not use_graphs:
                _reset_tags()
            ts.step()
            seen.append((_state(ts), ts.ada))
    return seen


def test_one_rank_split_route_eager_captured_and_the_one_launch_route():
    """MPGAN at N = 30, B = 8, interval 2, fixed noise, 4 steps: the split route eagerly and captured, bit for bit; and both equal
    to the one-launch route in parameters, optimizer state, seed, p, r and the open interval after every step."""
    one = _run_split(False, False)
    eager, captured = _run_split(True, False), _run_split(True, True)
    for k, (a, b, c) in enumerate(zip(one, eager, captured)):
        assert _all_equal(b[0], c[0]) and b[1] == c[1], (k, b[1], c[1])
        assert _all_equal(a[0], b[0]) and a[1] == b[1], (k, a[1], b[1])
    assert one[-1][1]["steps"] == 0 and len({s[1]["p"] for s in one}) >= 2       # (two intervals closed; p moved)


def test_world1_nccl_group_split_route_with_the_all_reduce_in_place():
    """A world-size-1 RCCL group: D's buffer of n + 1 floats goes through a real ``dist.all_reduce`` between the count and the
    settle -- eagerly, between the three graphs of a batch, and captured inside the one graph (``graph_collectives``) -- and every
    route lands on the bits of the one-launch route without a group."""
    import torch.distributed as dist
    one = _run_split(False, False)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29577")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        pg = dist.group.WORLD
        runs = [_run_split(True, False, process_group=pg), _run_split(True, True, n_graphs=3, process_group=pg),
                _run_split(True, True, n_graphs=1, process_group=pg, graph_collectives=True)]
    finally:
        dist.destroy_process_group()
    for run in runs:
        for k, (a, b) in enumerate(zip(one, run)):
            assert _all_equal(a[0], b[0]) and a[1] == b[1], (k, a[1], b[1])


def _rank_main(rank, world, port, out):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    from mpgan_amd import dist as mdist, train
    from oracle import train_ref as T
    from oracle.train_ref import synthetic_batch
    torch.cuda.set_device(0)
    r, w, pg = mdist.init_from_env("gloo")
    Br, N, steps = 4, 30, 4
    G, D = train.default_mpgan(N, disc_dropout=0.0)
    if rank == 0:
        G.load_state_dict(T.init_state_dict(T.mpgan_param_shapes(True), 41, torch.float32))
        D.load_state_dict(T.init_state_dict(T.mpgan_param_shapes(False), 42, torch.float32))
    mdist.broadcast_module(G, 0, pg)
    mdist.broadcast_module(D, 0, pg)
    data, labels = synthetic_batch(Br * world, N, seed=3)
    sl = slice(rank * Br, (rank + 1) * Br)
    ts = train.TrainStep(G, D, Br, N, lr_disc=train.LR["g"][0], lr_gen=train.LR["g"][1], use_graphs=True, process_group=pg,
                         world_size=world, augment=train.Augment(**ADA))
    ts.set_batch(data[sl].cuda(), labels[sl].cuda())
    ts.ada_keep_out = True       # (before the capture: the graph's own ``out`` tensor is the one kept)
    ts.capture(warmup=0)
    assert len(ts._graphs) == 3 and ts._ada.split and ts._ada.n_total == Br * world
    trace = []
    for _ in range(steps):
        ts.step()
        torch.cuda.synchronize()
        trace.append((ts.ada, ts.ada_last_out.detach().reshape(-1)[:Br].cpu()))
    out[rank] = (trace, ts._ada.step, ts.fD.flat.cpu())
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_on_one_gpu_settle_one_probability():
    """B = 4 per rank, interval 2, captured (three graphs, D's all-reduce between the count and the settle), 4 steps: the ranks'
    ``ts.ada`` are equal after every step and are ``ada_rule`` replayed over the real jets' outputs of both; D's weights too."""
    import torch.multiprocessing as mp
    from mpgan_amd import step_options as so
    world = 2
    out = mp.get_context("spawn").Manager().dict()
    spawn_joined(_rank_main, (world, 29573, out), world)
    (tr0, step, fD0), (tr1, step1, fD1) = out[0], out[1]
    assert step == step1 == 0.125 and torch.equal(fD0, fD1)
    state = (0, 0, ADA["aug_prob"], 0.0)
    for k, ((ada0, o0), (ada1, o1)) in enumerate(zip(tr0, tr1)):
        assert ada0 == ada1, (k, ada0, ada1)
        state = so.ada_rule(torch.cat([o0, o1]), 8, 0.5, ADA["ada_target"], step, ADA["ada_interval"], *state)
        assert ada0 == {"p": state[2], "r": state[3], "sign_sum": state[0], "steps": state[1]}, (k, ada0, state)
    assert tr0[-1][0]["steps"] == 0
