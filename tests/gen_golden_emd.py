#!/usr/bin/env python3
"""Generate the golden energy mover's distances of tests/test_emd_cpu.py and tests/test_gpu_emd.py: tests/golden/emd_*.npz.

Each file holds ``a`` [na, N, 3] and ``b`` [nb, N, 3] (fp32 un-normalised jets, zero-pT padding in random slots) and
``D`` [na, nb] (fp64): the optimum of the transportation problem that include/mpgan_amd.h states for mpg_jet_emd, solved
here by ``scipy.optimize.linprog(method="highs")`` on the fp64 values of those fp32 jets -- a solver that shares nothing with
csrc/jet_emd.hip.  Needs scipy; the tests that run on the GPU read only the files.

Sets: N = 30, 48 x 48, multiplicity laws gluon and top; N = 150, 8 x 8; N in {1, 2, 31, 32, 33}, 6 x 6; and a hand-made set
(an empty jet, jets of equal pT sums, a jet against itself, a duplicated row).

The "slots" sets (emd_slots_n{N}, 5 x 5, and emd_hand70) fill the node slots and launch shapes that those never reach.
mpg_jet_emd keeps node v in register slot v / 64 of lane v % 64 and is built for 1, 2 and 6 slots (2N + 2 <= 64, <= 128, more);
a workgroup runs 4 waves up to N = 60, 3 to 69, 2 to 86, 1 from 87, and needs more than 64 KiB of LDS from N = 125.  The N
are the two sides of each of those lines and the largest N; every set has two jets per side with pT > 0 in every slot, so
that a pair of them has all 2N + 2 nodes, which the generator asserts.  These files also hold ``D_R04`` (the same pairs at
R = 0.4, rounded to fp32 as the C entry receives it) and ``nodes`` [na, nb] (int32): n_a + n_b + 2, the nodes of each pair.

The N = 30 gluon set also decides coverage on the device against coverage on the host, which must agree exactly: nearest
neighbours must not be near-ties.  For that set the generator asserts that, in every row and every column of D, the
second-smallest distance is at least 4 x the fp32 bar (2e-5 max S) above the smallest, and moves to the next seed if not
(seed 7: gap 4.0e-3, 5.5 bars).  The top set is compared distance by distance only; its gap is recorded, not required.

Run:  python tests/gen_golden_emd.py            every set
      python tests/gen_golden_emd.py slots      the emd_slots_* sets and emd_hand70 only
      python tests/gen_golden_emd.py slots --check   regenerate those and compare with the committed files, writing nothing
"""
import os
import sys

import numpy as np
import torch
from scipy.optimize import linprog
from scipy.sparse import coo_matrix

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "golden")
sys.path.insert(0, os.path.dirname(HERE))

from mpgan_amd import data  # noqa: E402

GPU_BAR = 2e-5
SLOT_NS = (31, 32, 60, 61, 63, 64, 69, 70, 86, 87, 124, 125, 160)
R04 = float(np.float32(0.4))   # the C entries take R as a float: the radius they are given is 0.4 rounded to fp32 (1.5e-8 off)


def scattered_jets(B, N, law, seed):
    """Un-normalised [B, N, 3] synthetic jets with their zero-pT padding moved to random slots of each jet."""
    x, _ = data.synthetic_jets(B, N, seed=seed, dist=law)
    jets = data.unnormalise_jets(x, "g")
    g = torch.Generator().manual_seed(seed)
    perm = torch.rand(B, N, generator=g).argsort(1)
    return torch.gather(jets, 1, perm[:, :, None].expand(B, N, 3)).contiguous().numpy().astype(np.float32)


def emd_lp(A, B, R=1.0):
    """The definition, literally: particles of positive pT, cost theta / R, one slack particle at cost 1 on the lighter jet."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    A, B = A[A[:, 2] > 0], B[B[:, 2] > 0]
    wa, wb = A[:, 2].copy(), B[:, 2].copy()
    C = np.sqrt((A[:, None, 0] - B[None, :, 0]) ** 2 + (A[:, None, 1] - B[None, :, 1]) ** 2) / R
    d = wa.sum() - wb.sum()
    if d < 0:
        wa, C = np.append(wa, -d), np.vstack([C, np.ones((1, C.shape[1]))])
    elif d > 0:
        wb, C = np.append(wb, d), np.hstack([C, np.ones((C.shape[0], 1))])
    n, m = len(wa), len(wb)
    if n == 0 or m == 0:
        return 0.0
    cell = np.arange(n * m)
    Aeq = coo_matrix((np.ones(2 * n * m), (np.concatenate([cell // m, n + cell % m]), np.concatenate([cell, cell]))),
                     shape=(n + m, n * m)).tocsr()
    # the two totals agree only up to rounding; the last constraint follows from the others, so it is left out
    r = linprog(C.ravel(), A_eq=Aeq[:-1], b_eq=np.concatenate([wa, wb])[:-1], bounds=(0, None), method="highs")
    assert r.status == 0, r.message
    return float(r.fun)


def scale(A, B, R=1.0):
    """S of the tests' bars: (sum pT_A + sum pT_B) max(1, theta_max / R) over the particles of positive pT."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    A, B = A[A[:, 2] > 0], B[B[:, 2] > 0]
    s = A[:, 2].sum() + B[:, 2].sum()
    if len(A) == 0 or len(B) == 0:
        return s
    th = np.sqrt((A[:, None, 0] - B[None, :, 0]) ** 2 + (A[:, None, 1] - B[None, :, 1]) ** 2).max() / R
    return s * max(1.0, th)


def matrix(a, b, R=1.0):
    return np.array([[emd_lp(x, y, R) for y in b] for x in a])


def nearest_gap(D):
    """Smallest (second-best - best) over the rows and the columns of D."""
    r, c = np.sort(D, axis=1), np.sort(D, axis=0)
    return min((r[:, 1] - r[:, 0]).min(), (c[1] - c[0]).min())


def save(name, a, b, D):
    np.savez_compressed(os.path.join(OUT, name), a=a, b=b, D=D)
    print(f"{name}: a {a.shape} b {b.shape} D mean {D.mean():.6f}", flush=True)


def hand_made():
    """N = 6: an empty jet; two jets of equal pT sums (no slack between them); a jet and its copy (a duplicated row, and the
    jet against itself); a jet of duplicated particles; one particle.  a = b = the same seven jets."""
    z = [0.0, 0.0, 0.0]
    jets = np.array([
        [z, z, z, z, z, z],
        [[0.1, 0.0, 0.5], z, [-0.2, 0.1, 0.25], [0.0, -0.3, 0.25], z, z],
        [[0.0, 0.2, 0.125], [0.3, 0.3, 0.375], z, z, [-0.1, -0.1, 0.25], [0.2, -0.2, 0.25]],
        [[0.05, 0.02, 0.3], [0.4, -0.1, 0.2], [-0.3, 0.2, 0.1], z, [0.0, 0.0, 0.7], z],
        [[0.05, 0.02, 0.3], [0.4, -0.1, 0.2], [-0.3, 0.2, 0.1], z, [0.0, 0.0, 0.7], z],
        [[0.1, 0.1, 0.2], [0.1, 0.1, 0.2], [0.1, 0.1, 0.2], [-0.1, 0.0, 0.3], [-0.1, 0.0, 0.3], z],
        [z, z, z, [1.5, -1.0, 2.0], z, z],
    ], dtype=np.float32)
    return jets, jets.copy()


def full_jet(rs, N):
    """pT > 0 in every slot: (eta, phi) uniform in +-0.4, pT a Dirichlet draw times a total in [0.5, 1]."""
    jet = np.empty((N, 3), np.float32)
    jet[:, :2] = rs.uniform(-0.4, 0.4, (N, 2))
    jet[:, 2] = rs.dirichlet(np.ones(N)) * rs.uniform(0.5, 1.0)
    assert np.all(jet[:, 2] > 0)
    return jet


def slot_side(rs, N):
    """Five jets: two full, one with about half its slots at pT = 0 (random positions), one particle, an empty jet."""
    half = full_jet(rs, N)
    dead = rs.rand(N) < 0.5
    dead[rs.randint(N)] = False
    half[dead, 2] = 0
    one = np.zeros((N, 3), np.float32)
    one[rs.randint(N)] = (rs.uniform(-0.4, 0.4), rs.uniform(-0.4, 0.4), rs.uniform(0.5, 1.0))
    return np.stack([full_jet(rs, N), full_jet(rs, N), half, one, np.zeros((N, 3), np.float32)])


def slot_set(N):
    rs = np.random.RandomState(7000 + N)
    a, b = slot_side(rs, N), slot_side(rs, N)
    for side in (a, b):
        assert [(x[:, 2] > 0).sum() for x in side[[0, 1, 3, 4]]] == [N, N, 1, 0]
        assert side[0, :, 2].sum() != side[1, :, 2].sum()
    return a, b


def hand_made_70():
    """N = 70, every slot live (142 nodes: register slots 0 to 2 of the six-slot build); a = b = the same five jets.
    Jets 0 and 1: pT multiples of 2^-10 of equal sum, exact in fp32 in any order, so neither slack takes part.
    Jets 2 and 3: a jet and its copy (a duplicated row, and the jet against itself).  Jet 4: 35 coincident pairs."""
    N = 70
    rs = np.random.RandomState(70)
    k0, k1 = rs.randint(1, 33, N), rs.randint(1, 33, N)
    i = 0
    while k1.sum() != k0.sum():                # move jet 1's sum to jet 0's one unit at a time, every pT staying positive
        step = 1 if k1.sum() < k0.sum() else -1
        if k1[i % N] + step >= 1:
            k1[i % N] += step
        i += 1
    jets = np.stack([full_jet(rs, N) for _ in range(5)])
    jets[0, :, 2], jets[1, :, 2] = k0 / 1024.0, k1 / 1024.0
    assert not np.array_equal(k0, k1)
    for order in (slice(None), slice(None, None, -1)):
        assert jets[0, order, 2].sum(dtype=np.float32) == jets[1, order, 2].sum(dtype=np.float32) == k0.sum() / 1024.0
    jets[3] = jets[2]
    jets[4, 35:] = jets[4, :35]
    assert np.all(jets[..., 2] > 0)
    return jets, jets.copy()


def node_counts(a, b):
    return ((a[:, None, :, 2] > 0).sum(2) + (b[None, :, :, 2] > 0).sum(2) + 2).astype(np.int32)


def save_slots(name, a, b, check):
    arrays = dict(a=a, b=b, D=matrix(a, b), D_R04=matrix(a, b, R04), nodes=node_counts(a, b))
    path = os.path.join(OUT, name + ".npz")
    if check:
        old = np.load(path, allow_pickle=False)
        assert sorted(old.files) == sorted(arrays)
        for k, v in arrays.items():
            if k.startswith("D"):             # the LP's optimum, not its vertex, is what reproduces: to its own tolerance
                assert np.allclose(old[k], v, rtol=0, atol=1e-12), (name, k, np.abs(old[k] - v).max())
            else:
                assert old[k].dtype == v.dtype and np.array_equal(old[k], v), (name, k)
        print(f"{name}: reproduced", flush=True)
        return
    np.savez_compressed(path, **arrays)
    print(f"{name}: a {a.shape} nodes max {arrays['nodes'].max()} D mean {arrays['D'].mean():.6f} "
          f"D_R04 mean {arrays['D_R04'].mean():.6f}", flush=True)


def slots(check=False):
    for N in SLOT_NS:
        a, b = slot_set(N)
        nodes = node_counts(a, b)
        assert np.all(nodes[:2, :2] == 2 * N + 2) and nodes.max() == 2 * N + 2 and nodes[4, 4] == 2 and nodes[3, 3] == 4
        save_slots(f"emd_slots_n{N}", a, b, check)
    a, b = hand_made_70()
    assert np.all(node_counts(a, b) == 142)
    save_slots("emd_hand70", a, b, check)


def main():
    os.makedirs(OUT, exist_ok=True)
    if sys.argv[1:2] == ["slots"]:
        return slots(check="--check" in sys.argv)
    for law, seed0, decides_coverage in (("gluon", 7, True), ("top", 8, False)):
        for seed in range(seed0, seed0 + 20):
            jets = scattered_jets(96, 30, law, seed)
            a, b = jets[:48], jets[48:]
            D = matrix(a, b)
            bar = GPU_BAR * max(scale(x, y) for x in a for y in b)
            gap = nearest_gap(D)
            print(f"N=30 {law} seed {seed}: nearest-neighbour gap {gap:.3e}, fp32 bar {bar:.3e} ({gap / bar:.1f} x)", flush=True)
            if gap >= 4 * bar or not decides_coverage:
                break
        else:
            raise SystemExit("no seed with a nearest-neighbour gap of 4 bars")
        np.savez_compressed(os.path.join(OUT, f"emd_n30_{law}"), a=a, b=b, D=D, seed=seed, gap=gap, bar=bar,
                            decides_coverage=decides_coverage)
        print(f"emd_n30_{law}: D mean {D.mean():.6f}", flush=True)
    jets = scattered_jets(16, 150, "gluon", 150)
    save("emd_n150", jets[:8], jets[8:], matrix(jets[:8], jets[8:]))
    for N in (1, 2, 31, 32, 33):
        jets = scattered_jets(12, N, "uniform" if N > 2 else "top", 100 + N)
        save(f"emd_n{N}", jets[:6], jets[6:], matrix(jets[:6], jets[6:]))
    a, b = hand_made()
    save("emd_hand", a, b, matrix(a, b))
    slots()


if __name__ == "__main__":
    main()
