"""The masks of the sender-list tests, defined once: tests/test_edge_partition_cpu.py asserts from a model of the kernels'
partition that every case still reaches the path it is there for, tests/test_gpu_edge_lists.py runs them.

The four sender-loop kernels of the fused MPLayer (csrc/edge_{fwd,bwd}{1,2}_impl.h) list a workgroup's unmasked senders in LDS
and walk that list.  A case is a name, B, N and -- per jet -- the sorted tuple of its unmasked particle indices, with the set
of things it is ``there_for``:

  empty_share   whole-list mode (N <= 160): some workgroup's share of the list is empty
  tickets       more than one sender chunk: the chunks' partial sums are added up by the workgroup that arrives last
  one_receiver  the last receiver block holds exactly one receiver
  index_mode    N > 160: every chunk lists its own index range
  masked_chunk  index mode: some chunk's index range holds no unmasked sender
  uneven_chunk  index mode: the last chunk's index range is shorter than the others'

Chunk bounds are never literals: they come from ``ops.edge_plan`` as it is when the cases are built."""
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "name B N sets there_for")


def plan(B, N):
    from mpgan_amd import ops
    return ops.edge_plan(B, N, mask=True, need_grad=True)


def chunk_bounds(N, SC):
    """Index ranges [lo, hi) of the SC sender chunks (JC = ceil(N / SC))."""
    JC = -(-N // SC)
    return [(min(N, sc * JC), min(N, sc * JC + JC)) for sc in range(SC)]


def _r(a, b=None):
    return tuple(range(a)) if b is None else tuple(range(a, b))


def _d16_sets():
    # N = 150, B = 16: unmasked counts 0, 1, 2, 4, 5, 150 -- the FIRST k indices in jets 0..5, the LAST k in jets 6..11 -- and four
    # jets with seeded random sets of at least one particle
    N, rs = 150, np.random.RandomState(150)
    counts = (0, 1, 2, 4, 5, 150)
    sets = [_r(k) for k in counts] + [_r(N - k, N) for k in counts]
    for _ in range(4):
        sets.append(tuple(sorted(int(j) for j in rs.permutation(N)[: rs.randint(1, N + 1)])))
    return tuple(sets)


def _e161_sets():
    # jet 0: unmasked only in the last chunk; jet 1: unmasked everywhere except one whole chunk in the middle
    B, N = 2, 161
    cb = chunk_bounds(N, plan(B, N).SC)
    lo, hi = cb[-1]
    mlo, mhi = cb[len(cb) // 2]
    return (_r(lo, hi), tuple(j for j in range(N) if not mlo <= j < mhi))


def _e192_sets():
    # jet 0: empty; jet 1: exactly one sender per chunk, at a place that moves with the chunk
    B, N = 2, 192
    cb = chunk_bounds(N, plan(B, N).SC)
    return ((), tuple(lo + (3 * sc) % (hi - lo) for sc, (lo, hi) in enumerate(cb) if hi > lo))


def cases():
    """Every case, by name."""
    W = ("empty_share", "tickets")
    I = ("index_mode", "masked_chunk", "uneven_chunk", "tickets")
    cs = [
        Case("A_empty_beside_full", 4, 30, ((), _r(30), (29,), _r(8)), W),
        Case("B_no_sender", 2, 30, ((), ()), W),
        Case("C33_last_receiver", 2, 33, ((32,), (0, 32)), W + ("one_receiver",)),
        Case("C64_last_tile", 2, 64, ((), _r(56, 64)), W),
        Case("C65_last_receiver", 2, 65, ((), (64,)), W + ("one_receiver",)),
        Case("D16_n150", 16, 150, _d16_sets(), W),
        Case("D2_n150", 2, 150, ((149,), _r(16)), W),
        Case("E161_index_mode", 2, 161, _e161_sets(), I),
        Case("E192_index_mode", 2, 192, _e192_sets(), I),
        Case("K_knn", 2, 30, ((), (3, 11, 20)), W),
    ]
    return {c.name: c for c in cs}


def one_particle_instead_of_none(case):
    """The same case with every empty jet given exactly one particle (the same shape, so the same plan): what the other jets
    compute must not notice."""
    sets = tuple(s if len(s) else (case.N // 2,) for s in case.sets)
    return case._replace(name=case.name + "_filled", sets=sets)


def mask_of(case):
    """[B, N, 1] float64 numpy array of 0 / 1."""
    m = np.zeros((case.B, case.N, 1))
    for b, s in enumerate(case.sets):
        m[b, list(s), 0] = 1
    return m
