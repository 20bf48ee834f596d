"""CPU: ``gen.JetSampler`` over data-parallel ranks as far as it lives on the host -- how a call's chunks are dealt to the ranks
(``gen.rank_chunks``), the row arithmetic that lands a rank's chunks one behind the other in its own array (``mpg_jets_finish``'s
rule from include/mpgan_amd.h, restated), the interleave of ``sample_all``, and the refusals of ``mpg_jets_finish_stride``, which
return before any HIP call."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

CHUNK = 3


@pytest.mark.parametrize("W", [1, 2, 3])
@pytest.mark.parametrize("num", [0, 1, 5, 6, 7])
def test_rank_chunks_partition_the_call_in_stream_order(num, W):
    from mpgan_amd import gen
    per_rank = [gen.rank_chunks(num, CHUNK, r, W) for r in range(W)]
    chunks = -(-num // CHUNK)
    rounds = -(-chunks // W)
    assert all(len(rs) == rounds for rs in per_rank)                  # every rank replays equally often
    for rs in per_rank:                                               # a rank's own ranges: in stream order, each within a chunk
        assert all(0 <= a <= b <= num and b - a <= CHUNK for a, b in rs)
        assert all(rs[k][1] <= rs[k + 1][0] for k in range(len(rs) - 1))
        sizes = [b - a for a, b in rs]                                # full ones, at most one short one, then empty ones
        assert sizes == sorted(sizes, reverse=True) and sum(0 < s < CHUNK for s in sizes) <= 1
    # chunk c of the call sits at place c // W of rank c % W, and the non-empty ranges tile [0, num)
    dealt = [per_rank[c % W][c // W] for c in range(rounds * W)]
    assert dealt == [(min(c * CHUNK, num), min((c + 1) * CHUNK, num)) for c in range(rounds * W)]
    rows = [g for a, b in dealt for g in range(a, b)]
    assert rows == list(range(num))


def test_rank_chunks_refuses_nonsense():
    from mpgan_amd import gen
    for bad in ((-1, 3, 0, 1), (4, 0, 0, 1), (4, 3, 2, 2), (4, 3, -1, 2), (4, 3, 0, 0)):
        with pytest.raises(ValueError):
            gen.rank_chunks(*bad)
    assert gen.rank_chunks(7, 3) == [(0, 3), (3, 6), (6, 7)]           # one rank: today's chunks


@pytest.mark.parametrize("W", [1, 2, 3])
@pytest.mark.parametrize("calls", [(10,), (6, 6), (1, 0, 7), (5, 12)])
def test_the_launches_rows_land_where_sample_all_reads_them(calls, W):
    """The host's part of a W-rank sampler replayed with integers: each launch covers stream rows cursor .. cursor + B - 1, writes
    row r = g - row0 of the rank's array when r < total (uint64 arithmetic) and moves the cursor by W B; ``sample_all`` reads
    chunk k of rank r as chunk k W + r of the call.  The gathered rows must be the next rows of the ONE stream, call after call."""
    from mpgan_amd import gen
    B, M = CHUNK, 2**64
    cursor = [r * B for r in range(W)]                 # the device words
    start = 0                                          # the stream row a call begins at
    for n in calls:
        K = len(gen.rank_chunks(n, B, 0, W))
        local = np.full((W, max(K * B, 1)), -1, dtype=np.int64)
        for r in range(W):
            ranges = gen.rank_chunks(n, B, r, W)
            total = sum(b - a for a, b in ranges)
            pos = cursor[r]                            # (JetSampler._pos)
            for k in range(len(ranges)):
                row0 = pos - k * B
                for b in range(B):
                    g = cursor[r] + b
                    row = (g - row0) % M
                    if row < total:
                        assert local[r, row] == -1     # no row written twice
                        local[r, row] = g
                cursor[r] += W * B
                pos += W * B
            assert (local[r, :total] >= 0).all() and (local[r, total:] == -1).all()
        gathered = local[:, :K * B].reshape(W, K, B).transpose(1, 0, 2).reshape(-1)[:n]
        assert gathered.tolist() == list(range(start, start + n))
        start += K * W * B                             # whole rounds are consumed
        assert cursor == [start + r * B for r in range(W)]


def test_finish_stride_refuses_without_a_device_and_the_wrapper_keeps_its_signature():
    from mpgan_amd import _lib, ops
    L = _lib.lib()
    buf = np.zeros(16, dtype=np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    f3 = (C.c_float * 3)(1.0, 1.0, 1.0)
    fin = lambda **kw: L.mpg_jets_finish_stride(kw.get("feat", p), 3, None, kw.get("B", 2), 2, f3, f3, f3, kw.get("out", p), None, 0,
                                                kw.get("total", 2), 1, kw.get("stride", 4), p, kw.get("seed", p), p, None)
    for bad in (dict(stride=0), dict(stride=-4), dict(B=0), dict(total=-1), dict(feat=None), dict(out=None), dict(seed=None)):
        assert fin(**bad) == -1, bad
    assert not buf.any()
    assert inspect.signature(ops.jets_finish).parameters["stride"].default is None


def test_sampler_arguments():
    from mpgan_amd import gen, train
    ps = inspect.signature(gen.JetSampler.__init__).parameters
    assert (ps["rank"].default, ps["world_size"].default, ps["process_group"].default) == (0, 1, None)
    G, _ = train.default_mpgan(30, device="cpu")
    for bad in (dict(rank=2, world_size=2), dict(rank=-1, world_size=2), dict(world_size=0)):
        with pytest.raises(ValueError, match="rank"):
            gen.JetSampler(G, torch.linspace(0, 1, 31), 30, **bad)
    with pytest.raises(RuntimeError, match="no CPU path"):
        gen.JetSampler(G, torch.linspace(0, 1, 31), 30, rank=1, world_size=2)
