"""GPU: ``gen.JetSampler`` over data-parallel ranks -- ``ops.jets_finish(stride=)`` on the stream's words, and two ranks on the
one GPU over gloo whose ``sample_all`` must be the one-rank sampler's stream bit for bit, masks included: one call, two calls
against one, resume across world sizes, and ``evaluate_generator`` on both ranks."""
import os
import sys

import numpy as np
import pytest
import torch

from spawn_util import spawn_joined

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK, N = 3, 33           # a jet of 33 particles crosses a 32-receiver block


def test_jets_finish_with_a_stride_of_two_chunks():
    """Three launches with stride = 2 B from a cursor of B (rank 1 of 2): after each the cursor, the seed word of the chunk the
    cursor now stands at, and the ticket back at zero; the rows land where ``row0`` puts them and nowhere else."""
    from mpgan_amd import data, ops
    B, n, key = 2, 2, 0xFEDCBA9876543210
    feat = torch.rand(B, n, 3, device="cuda") - 0.5
    cursor = torch.full((1,), B, dtype=torch.int64, device="cuda")
    seed = torch.full((1,), ops.u64_as_i64(ops.chunk_seed(key, 1)), dtype=torch.int64, device="cuda")
    ticket = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = torch.full((3 * B + 1, n, 3), -7.0, device="cuda")
    kw = dict(maxes=data.FEATURE_MAXES["g"], norms=data.FEATURE_NORMS, shifts=data.FEATURE_SHIFTS, key=key, cursor=cursor, seed=seed,
              ticket=ticket)
    want = data.unnormalise_jets(torch.cat((feat, torch.full((B, n, 1), 0.5, device="cuda")), 2), "g")
    for k in range(3):
        cur = B + k * 2 * B
        ops.jets_finish(feat, None, out, row0=cur - k * B, total=3 * B, stride=2 * B, **kw)
        torch.cuda.synchronize()
        assert int(cursor.item()) == cur + 2 * B
        assert int(seed.item()) & (2**64 - 1) == ops.chunk_seed(key, (cur + 2 * B) // B) == (key + (2 * k + 3) * ops.CHUNK_SEED_STEP) % 2**64
        assert int(ticket.item()) == 0
        assert torch.equal(out[k * B:(k + 1) * B], want) and bool((out[(k + 1) * B:] == -7.0).all())
    with pytest.raises(ValueError):
        ops.jets_finish(feat, None, out, stride=0, **kw)
    # stride = None is mpg_jets_finish: the cursor moves by B
    ops.jets_finish(feat, None, out, row0=int(cursor.item()), total=B, **kw)
    torch.cuda.synchronize()
    assert int(cursor.item()) == 7 * B + B and int(seed.item()) & (2**64 - 1) == ops.chunk_seed(key, 8)


def _rank_main(rank, world, port, out):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    from mpgan_amd import data, dist as mdist, evaluation as ev, gen, ops, train
    from test_gpu_sampler import _table
    torch.cuda.set_device(0)
    r, w, pg = mdist.init_from_env("gloo")
    torch.manual_seed(0)
    G, _ = train.default_mpgan(N)       # (the same seed on every rank: equal weights)
    G.eval()
    table = _table(N)
    ranked = lambda seed, **kw: gen.JetSampler(G, table, N, chunk=CHUNK, seed=seed, with_mask=True, rank=rank, world_size=world,
                                               process_group=pg, **kw)
    single = lambda seed: gen.JetSampler(G, table, N, chunk=CHUNK, seed=seed, with_mask=True)
    same = lambda a, b: torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])

    # one call of 10: four chunks, two rounds; the last chunk is short by two jets
    s, one = ranked(7), single(7)
    assert int(s.cursor.item()) == rank * CHUNK and int(s.seed.item()) & (2**64 - 1) == ops.chunk_seed(s.key, rank)
    mine = s.sample_all(10)
    want = one.sample(10)
    torch.cuda.synchronize()
    assert mine[0].shape == (10, N, 3) and mine[1].shape == (10, N) and bool(mine[0].any())
    assert same(mine, want)
    assert s.position == 12 + rank * CHUNK and int(s._ticket.item()) == 0
    assert int(s.seed.item()) & (2**64 - 1) == ops.chunk_seed(s.key, 4 + rank)
    sd = s.state_dict()
    assert sd == {"key": gen.sampler_key(7), "cursor": 12 + rank * CHUNK, "chunk": CHUNK, "n": N + 1, "rank": rank, "world_size": world}

    # this rank's own rows: the chunks c = rank (mod 2) of the call
    own = ranked(7).sample(10)
    torch.cuda.synchronize()
    rows = [g for a, b in gen.rank_chunks(10, CHUNK, rank, world) for g in range(a, b)]
    assert own[0].shape[0] == len(rows) == (6 if rank == 0 else 4) and same(own, (want[0][rows], want[1][rows]))

    # the state into new samplers of both worlds (built under another key): the next rows continue the one-rank stream
    nxt = one.sample(6)
    again, alone = ranked(99), single(99)
    again.load_state_dict(sd)
    alone.load_state_dict(sd)
    assert alone.state_dict() == {"key": gen.sampler_key(7), "cursor": 12, "chunk": CHUNK, "n": N + 1}
    assert same(again.sample_all(6), nxt) and same(alone.sample(6), nxt)
    back = ranked(99)
    back.load_state_dict(one.state_dict())           # (a one-rank state at row 18: three rounds of two)
    assert same(back.sample_all(4), one.sample(4))
    odd = single(7)
    odd.sample(3)
    with pytest.raises(ValueError, match="rounds"):
        ranked(7).load_state_dict(odd.state_dict())  # (row 3 is half a round)

    # two calls of 6 equal one call of 12 (a round is 6 rows)
    a, b = ranked(11), ranked(11)
    first, second = a.sample_all(6), a.sample_all(6)
    whole = b.sample_all(12)
    torch.cuda.synchronize()
    assert same((torch.cat((first[0], second[0])), torch.cat((first[1], second[1]))), whole) and same(whole, single(11).sample(12))
    # eager launches, and a call that leaves this world's second rank without a row
    e = ranked(11, use_graphs=False)
    assert same(e.sample_all(12), whole)
    tiny = ranked(13).sample_all(2)
    assert tiny[0].shape == (2, N, 3) and same(tiny, single(13).sample(2))

    # the periodic evaluation: the same entry on every rank
    x, labels = data.synthetic_jets(64, N, seed=4)
    real = data.unnormalise_jets(x, "g").cuda()
    es = gen.JetSampler(G, labels, N, chunk=16, seed=1, rank=rank, world_size=world, process_group=pg)
    got = ev.evaluate_generator(G, real, "g", num_samples=64, keys=("w1m",), num_w1_eval_samples=32, rng=np.random.RandomState(0),
                                sampler=es)
    lone = ev.evaluate_generator(G, real, "g", num_samples=64, keys=("w1m",), num_w1_eval_samples=32, rng=np.random.RandomState(0),
                                 sampler=gen.JetSampler(G, labels, N, chunk=16, seed=1))
    assert es.position == 64 + rank * 16
    out[rank] = (np.asarray(got["w1m"][0]), np.asarray(lone["w1m"][0]))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_on_one_gpu_reproduce_the_one_rank_stream():
    import torch.multiprocessing as mp
    world = 2
    out = mp.get_context("spawn").Manager().dict()
    spawn_joined(_rank_main, (world, 29575, out), world)
    (w0, lone0), (w1, lone1) = out[0], out[1]
    assert np.all(np.isfinite(w0)) and np.array_equal(w0, w1)
    assert np.array_equal(w0, lone0) and np.array_equal(lone0, lone1)      # (and the one-rank sampler's entry)
