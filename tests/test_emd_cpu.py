"""CPU: the exact jet EMD solver's host build (mpg_jet_emd_host, csrc/jet_emd.hip -- the code the GPU kernel runs, in fp64)
against a linear-programming statement of the definition, its invariances, and coverage / MMD on top of it
(mpgan_amd/evaluation.py).  Bars: |got - ref| <= 1e-9 S with S = (sum pT_A + sum pT_B) max(1, theta_max / R)."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from mpgan_amd import _lib, data, evaluation as ev

GOLDENS = ("emd_n30_gluon", "emd_n30_top", "emd_n150", "emd_n1", "emd_n2", "emd_n31", "emd_n32", "emd_n33", "emd_hand")
# every node slot and launch shape of the GPU build live (tests/gen_golden_emd.py): also R = 0.4 and the node counts
SLOT_NS = (31, 32, 60, 61, 63, 64, 69, 70, 86, 87, 124, 125, 160)
SLOTS = tuple("emd_slots_n%d" % N for N in SLOT_NS) + ("emd_hand70",)
TOL = 1e-9


def golden(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    return d["a"], d["b"], d["D"]


def golden_r04(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    return d["D_R04"], d["nodes"]


def scales(a, b, R=1.0):
    """S[i, j] = (sum pT + sum pT') max(1, theta_max / R) over the particles of positive pT of a[i] and b[j]."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    S = np.empty((len(a), len(b)))
    for i, x in enumerate(a):
        x = x[x[:, 2] > 0]
        for j, y in enumerate(b):
            y = y[y[:, 2] > 0]
            th = np.sqrt((x[:, None, 0] - y[None, :, 0]) ** 2 + (x[:, None, 1] - y[None, :, 1]) ** 2).max() / R if len(x) and len(y) else 0.0
            S[i, j] = (x[:, 2].sum() + y[:, 2].sum()) * max(1.0, th)
    return S


def host_emd(a, b, R=1.0, threads=16):
    """(D fp64, status, augmentations) straight from the C entry."""
    a, b = torch.as_tensor(a)[..., :3].float().contiguous(), torch.as_tensor(b)[..., :3].float().contiguous()
    na, nb, N = a.shape[0], b.shape[0], a.shape[1]
    D = torch.empty(na, nb, dtype=torch.float64)
    st, it = torch.full((na, nb), -7, dtype=torch.int32), torch.empty(na, nb, dtype=torch.int32)
    rc = _lib.lib().mpg_jet_emd_host_iters(a.data_ptr(), 3 * N, b.data_ptr(), 3 * N, 3, na, nb, N, R, D.data_ptr(), st.data_ptr(),
                                           it.data_ptr(), threads)
    assert rc == 0
    return D.numpy(), st.numpy(), it.numpy()


def check(got, ref, S, tol=TOL):
    err = np.abs(got - ref) / S.clip(min=1e-300)
    print("max |got - ref| / S = %.3e" % err.max())
    assert np.all(np.abs(got - ref) <= tol * S), float(err.max())


@pytest.mark.parametrize("N,law,R", [(30, "gluon", 1.0), (12, "uniform", 1.0), (30, "top", 0.4)])
def test_host_solver_matches_linprog_on_a_fresh_sample(N, law, R):
    from gen_golden_emd import emd_lp, scattered_jets
    jets = scattered_jets(10, N, law, seed=1000 + N)
    a, b = jets[:5], jets[5:]
    ref = np.array([[emd_lp(x, y, R) for y in b] for x in a])
    got = ev.emds(a, b, R=R)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (5, 5)
    check(got, ref, scales(a, b, R))
    assert np.array_equal(ev.emds(torch.from_numpy(a), torch.from_numpy(b), R=R).numpy(), got)


@pytest.mark.parametrize("name", GOLDENS + SLOTS)
def test_host_solver_matches_golden(name):
    a, b, D = golden(name)
    got, status, iters = host_emd(a, b)
    assert np.all(status == 0)
    N = a.shape[1]
    print("augmentations: mean %.1f max %d cap %d" % (iters.mean(), iters.max(), 32 * (N + 1)))
    assert iters.max() < 32 * (N + 1)
    check(got, D, scales(a, b))
    # one thread, sixteen threads: the same bits
    assert np.array_equal(host_emd(a, b, threads=1)[0], got)
    if name in SLOTS:
        D04, nodes = golden_r04(name)
        assert np.array_equal(nodes, (a[:, None, :, 2] > 0).sum(2) + (b[None, :, :, 2] > 0).sum(2) + 2)
        assert nodes.max() == 2 * N + 2                         # a pair that fills every node of the launch
        got, status, iters = host_emd(a, b, R=0.4)
        print("R = 0.4 augmentations: mean %.1f max %d" % (iters.mean(), iters.max()))
        assert np.all(status == 0) and iters.max() < 32 * (N + 1)
        check(got, D04, scales(a, b, 0.4))


@pytest.mark.parametrize("name", ["emd_slots_n63", "emd_slots_n160"])
def test_scaling_every_pt_by_a_power_of_two_scales_the_distances_exactly(name):
    """The weights meet only sums, differences, minima and one product with a cost each; the costs and the potentials never
    see them.  So pT x 2^k gives 2^k times the same bits (no pT here is within 2^10 of the fp32 subnormals)."""
    a, b, _ = golden(name)
    pt = np.concatenate([a[..., 2].ravel(), b[..., 2].ravel()])
    assert pt[pt > 0].min() > 2.0 ** -100 and pt.max() < 2.0 ** 100
    D, status, iters = host_emd(a, b)
    for k in (10, -10):
        f = np.array([1, 1, 2.0 ** k], np.float32)
        Dk, statusk, itersk = host_emd(a * f, b * f)
        assert np.array_equal(Dk, D * 2.0 ** k) and np.array_equal(statusk, status) and np.array_equal(itersk, iters)


def test_symmetry_self_distance_permutation_and_duplicates():
    a, b, _ = golden("emd_n30_gluon")
    a, b = a[:12], b[:12]
    S = scales(a, b)
    Dab, Dba = host_emd(a, b)[0], host_emd(b, a)[0]
    assert np.all(np.abs(Dab - Dba.T) <= TOL * S)
    Daa = host_emd(a, a)[0]
    assert np.all(np.diag(Daa) <= TOL * np.diag(scales(a, a)))
    rs = np.random.RandomState(0)
    ap = np.stack([x[rs.permutation(len(x))] for x in a])
    assert np.all(np.abs(host_emd(ap, b)[0] - Dab) <= TOL * S)
    # duplicated rows and columns, anywhere in the matrix: bit-identical distances
    ia, ib = np.array([3, 0, 3, 7, 7, 3, 11]), np.array([5, 5, 1, 0, 5])
    Ddup = host_emd(a[ia], b[ib])[0]
    assert np.array_equal(Ddup, Dab[ia][:, ib])


def test_hand_made_cases():
    a, b, D = golden("emd_hand")
    got = ev.emds(a, b)
    pt = a[..., 2].astype(np.float64).sum(1)
    assert got[0, 0] == 0.0                                     # two empty jets
    assert np.allclose(got[0], pt, rtol=1e-12, atol=0)          # an empty jet is all slack: the other jet's pT sum
    assert pt[1] == pt[2] and abs(got[1, 2] - D[1, 2]) <= TOL * 2  # equal pT sums: no slack particle
    assert np.array_equal(got[3], got[4]) and got[3, 3] <= TOL and got[3, 4] <= TOL   # a copy, and a jet against itself
    check(got, D, scales(a, b))


def test_arguments():
    a, b, _ = golden("emd_n2")
    lib = _lib.lib()
    for N in (0, ev.MAX_PARTICLES + 1):
        x = torch.zeros(2, max(N, 1), 3)
        out = torch.full((2, 2), -1.0, dtype=torch.float64)
        assert lib.mpg_jet_emd_host(x.data_ptr(), 3 * N, x.data_ptr(), 3 * N, 3, 2, 2, N, 1.0, out.data_ptr(), None, 4) == -1
        assert torch.all(out == -1.0)
    with pytest.raises(ValueError):
        ev.emds(np.zeros((2, ev.MAX_PARTICLES + 1, 3), np.float32), np.zeros((2, ev.MAX_PARTICLES + 1, 3), np.float32))
    with pytest.raises(ValueError):
        ev.emds(a, b[:, :1])
    assert ev.emds(a[:0], b).shape == (0, 6)
    # a fourth (mask) column is stepped over; float64 input is read as fp32
    a4 = np.concatenate([a, (a[..., 2:] > 0).astype(np.float32)], 2)
    assert np.array_equal(ev.emds(a4, b), ev.emds(a, b))
    assert np.array_equal(ev.emds(a4, np.concatenate([b, b[..., 2:]], 2)), ev.emds(a, b))
    assert np.array_equal(ev.emds(a.astype(np.float64), b), ev.emds(a, b))
    # a search that finds no path (non-finite coordinates) is reported, not returned as a distance
    bad = a.copy()
    bad[0, :, 0] = np.nan
    with pytest.raises(RuntimeError, match="status"):
        ev.emds(bad, b)


def numpy_cov_mmd(D, n_real, n_gen, k, batches, rng):
    """The definition on a precomputed D[gen, real]: a plain loop over the same draws."""
    covs, mmds = [], []
    for _ in range(batches):
        i_real = rng.choice(n_real, k)
        i_gen = rng.choice(n_gen, k)
        Db = D[i_gen][:, i_real]
        mmds.append(np.mean(np.min(Db, axis=0)))
        covs.append(len(np.unique(np.argmin(Db, axis=1))) / k)
    return float(np.mean(covs)), float(np.mean(mmds))


@pytest.mark.parametrize("name", ["emd_n30_gluon", "emd_n30_top"])
def test_cov_mmd_equals_a_numpy_loop_over_the_golden_distances(name):
    gen, real, D = golden(name)
    for k, batches, seed in ((48, 3, 1), (20, 5, 2)):
        ref_cov, ref_mmd = numpy_cov_mmd(D, len(real), len(gen), k, batches, np.random.RandomState(seed))
        cov, mmd = ev.cov_mmd(real, gen, num_eval_samples=k, num_batches=batches, rng=np.random.RandomState(seed))
        assert isinstance(cov, float) and isinstance(mmd, float)
        assert cov == ref_cov
        assert abs(mmd - ref_mmd) <= TOL * scales(gen, real).max()
    cov_t, mmd_t = ev.cov_mmd(torch.from_numpy(real), torch.from_numpy(gen), 20, 5, rng=np.random.RandomState(2))
    assert (cov_t, mmd_t) == (cov, mmd)


def test_evaluate_appends_coverage_and_mmd_after_the_w1_keys():
    x, _ = data.synthetic_jets(400, 30, seed=3, dist="gluon")
    y, _ = data.synthetic_jets(400, 30, seed=4, dist="quark")
    real, gen = data.unnormalise_jets(x, "g"), data.unnormalise_jets(y, "g")
    kw = dict(num_w1_eval_samples=100, num_cov_mmd_eval_samples=12)
    rng = np.random.RandomState(9)
    before = ev.evaluate({"w1p": [], "w1m": []}, real, gen, "g", rng=rng, **kw)
    assert sorted(before) == ["w1m", "w1p"]                     # a dict without the keys gains nothing
    cov, mmd = ev.cov_mmd(real, gen, num_eval_samples=12, rng=rng)   # the draws that follow those of the W1 keys
    after = ev.evaluate({"coverage": [], "mmd": [], "w1p": [], "w1m": []}, real, gen, "g", rng=np.random.RandomState(9), **kw)
    for k in ("w1p", "w1m"):
        assert np.array_equal(after[k][0], before[k][0])
    assert after["coverage"] == [cov] and after["mmd"] == [mmd]
    assert 0 < cov <= 1 and mmd > 0
    only = ev.evaluate({"mmd": []}, real, gen, "g", rng=np.random.RandomState(9), **kw)
    assert list(only) == ["mmd"] and len(only["mmd"]) == 1
