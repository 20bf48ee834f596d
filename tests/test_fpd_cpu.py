"""CPU: FPD and KPD (mpgan_amd/evaluation.py) -- the 36 EFPs of degree <= 4 against the definition of the set and against
brute-force sums over index tuples, the Frechet distance against scipy's matrix square root, ``fpd`` / ``kpd`` against plain
numpy / scipy loops with the same draws, their freedom from the column order, and the plumbing around them."""
import itertools
import os
import re

import numpy as np
import pytest
import torch
from scipy.linalg import sqrtm
from scipy.optimize import curve_fit

from mpgan_amd import checkpoint, evaluation as ev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D4 = [("d<=", 4)]


def random_jets(n, N, seed, pad_frac=0.3):
    """[n, N, 3] (eta, phi, pt) with zero-pT padding scattered through each jet (never all of it)."""
    rs = np.random.RandomState(seed)
    eta = rs.normal(0, 0.2, size=(n, N))
    phi = rs.normal(0, 0.2, size=(n, N))
    pt = rs.exponential(0.05, size=(n, N))
    pad = rs.rand(n, N) < pad_frac
    pad[:, rs.randint(N)] = False
    return np.stack([eta, phi, np.where(pad, 0.0, pt)], axis=2)


# ------------------------------------------------------------------------------------- 1. the set is the definition
def canonical(edges):
    """Smallest relabelling of a multigraph on vertices 0 .. nv-1 (all used): a sorted tuple of sorted pairs."""
    nv = 1 + max((max(e) for e in edges), default=0)
    return min(tuple(sorted(tuple(sorted((p[a], p[b]))) for a, b in edges)) for p in itertools.permutations(range(nv)))


def components(edges):
    """The connected components of a multigraph without isolated vertices, each relabelled to 0 .. k-1."""
    verts = sorted({v for e in edges for v in e})
    comp = {v: v for v in verts}
    for _ in verts:
        for a, b in edges:
            comp[a] = comp[b] = min(comp[a], comp[b])
    out = []
    for root in sorted(set(comp.values())):
        mine = [v for v in verts if comp[v] == root]
        out.append(tuple((mine.index(a), mine.index(b)) for a, b in edges if comp[a] == root))
    return out


def connected_multigraphs(d):
    """Canonical forms of the connected loopless multigraphs with d edges (on at most d + 1 vertices)."""
    if d == 0:
        return {()}
    found = set()
    for nv in range(2, d + 2):
        pairs = list(itertools.combinations(range(nv), 2))
        for edges in itertools.combinations_with_replacement(pairs, d):
            if {v for e in edges for v in e} == set(range(nv)) and len(components(edges)) == 1:
                found.add(canonical(edges))
    return found


def test_the_set_is_every_multigraph_with_at_most_four_edges():
    primes = {d: connected_multigraphs(d) for d in range(5)}
    assert [len(primes[d]) for d in range(5)] == [1, 1, 2, 5, 12]
    # every multiset of connected graphs with at least one edge each and at most 4 edges in all; the empty multiset is the
    # graph of one vertex
    pool = [(d, g) for d in range(1, 5) for g in sorted(primes[d])]
    by_degree = {d: set() for d in range(5)}
    for k in range(5):
        for combo in itertools.combinations_with_replacement(pool, k):
            deg = sum(d for d, _ in combo)
            if deg <= 4:
                by_degree[deg].add(tuple(sorted(g for _, g in combo)))
    assert [len(by_degree[d]) for d in range(5)] == [1, 1, 3, 8, 23]
    want = set().union(*by_degree.values())
    got = [tuple(sorted(canonical(c) for c in components(g))) for g in ev.EFP_D4_GRAPHS]
    assert len(got) == 36 == len(set(got)) == ev.NUM_EFPS_D4
    assert set(got) == want
    # the first 21 are the connected ones; each composite is the disjoint union of the prime columns it names
    assert all(len(g) <= 1 for g in got[:21]) and all(len(g) >= 2 for g in got[21:])
    for k, factors in enumerate(ev.EFP_D4_FACTORS):
        assert tuple(sorted(got[f][0] for f in factors if got[f])) == got[k]
        assert all(0 < f < 21 for f in factors) or factors == (0,)


# ------------------------------------------------------------------------------------- 2. values
def brute_efp(jet, edges, normed=True):
    """sum over all index tuples of prod z_vertex prod theta_edge, straight from the edge list."""
    eta, phi, pt = jet[:, 0], jet[:, 1], jet[:, 2]
    z = pt / pt.sum() if normed and pt.sum() != 0 else pt
    th = np.sqrt((eta[:, None] - eta[None, :]) ** 2 + (phi[:, None] - phi[None, :]) ** 2)
    nv = 1 + max((max(e) for e in edges), default=0)
    L = "abcdefgh"
    spec = ",".join(L[:nv]) + "".join("," + L[a] + L[b] for a, b in edges) + "->"
    return float(np.einsum(spec, *([z] * nv), *([th] * len(edges)), optimize=True))


def brute_all(jets, normed=True):
    return np.array([[brute_efp(j, g, normed) for g in ev.EFP_D4_GRAPHS] for j in jets])


@pytest.mark.parametrize("N", [1, 2, 5, 9])
def test_all_36_columns_match_brute_force(N):
    jets = random_jets(5, N, seed=100 + N)
    got = ev.efps(jets, efpset_args=D4)
    ref = brute_all(jets)
    assert got.shape == (5, 36) and got.dtype == np.float64
    assert np.all(np.abs(got - ref) <= 1e-12 * np.abs(ref) + 1e-300), np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300))
    # composites are the products of their factors
    for k, factors in enumerate(ev.EFP_D4_FACTORS):
        np.testing.assert_allclose(got[:, k], np.prod(got[:, list(factors)], axis=1), rtol=1e-14, atol=0)
    # the five connected 4-vertex graphs are today's efps, and the default set is unchanged
    np.testing.assert_allclose(got[:, 13:18], ev.efps(jets), rtol=1e-12, atol=1e-300)
    assert np.array_equal(ev.efps(jets), ev.efps(jets, efpset_args=[("n==", 4), ("d==", 4), ("p==", 1)]))
    assert ev.efps(jets).shape == (5, 5)


def test_one_prime_at_thirty_particles():
    jets = random_jets(2, 30, seed=8)
    got = ev.efps(jets, efpset_args=D4)
    for k in (12, 18, 20):
        ref = np.array([brute_efp(j, ev.EFP_D4_GRAPHS[k]) for j in jets])
        np.testing.assert_allclose(got[:, k], ref, rtol=1e-12)


def test_torch_in_torch_out_and_other_sets_raise():
    jets = random_jets(3, 7, seed=2)
    t = ev.efps(torch.from_numpy(jets), efpset_args=D4)
    assert isinstance(t, torch.Tensor) and t.dtype == torch.float64
    assert np.array_equal(t.numpy(), ev.efps(jets, efpset_args=(("d<=", 4),), efp_jobs=4))
    for other in ([("d<=", 5)], [("d<=", 4), ("p==", 1)], [("n==", 4)]):
        with pytest.raises(NotImplementedError):
            ev.efps(jets, efpset_args=other)


def test_unnormalised_columns_scale_with_the_number_of_vertices():
    jets = random_jets(4, 8, seed=5)
    s = jets[..., 2].sum(1)
    nv = np.array([1 + max((max(e) for e in g), default=0) for g in ev.EFP_D4_GRAPHS])
    raw = ev.efps(jets, normed=False, efpset_args=D4)
    np.testing.assert_allclose(raw, ev.efps(jets, efpset_args=D4) * s[:, None] ** nv[None, :], rtol=1e-12)
    np.testing.assert_allclose(raw, brute_all(jets, normed=False), rtol=1e-12)


def test_padding_permutation_and_an_empty_jet():
    jets = random_jets(4, 12, seed=3, pad_frac=0.0)
    base = ev.efps(jets, efpset_args=D4)
    rs = np.random.RandomState(0)
    padded = np.zeros((4, 20, 3))
    padded[:, np.sort(rs.choice(20, 12, replace=False))] = jets
    for other in (jets[:, rs.permutation(12)], padded):
        np.testing.assert_allclose(ev.efps(other, efpset_args=D4), base, rtol=1e-12)
    for normed in (True, False):
        assert np.all(ev.efps(np.zeros((2, 4, 3)), normed=normed, efpset_args=D4) == 0)
    one = ev.efps(np.array([[[0.3, 0.1, 0.7], [0.0, 0.0, 0.0]]]), efpset_args=D4)[0]
    assert one[0] == 1.0 and np.all(one[1:] == 0)


# ------------------------------------------------------------------------------------- 3. Frechet distance
def scipy_frechet(mu1, s1, mu2, s2):
    return float(np.sum((mu1 - mu2) ** 2) + np.trace(s1) + np.trace(s2) - 2 * np.trace(sqrtm(s1 @ s2)).real)


def random_cov(rs, F):
    A = rs.normal(size=(F, 3 * F))
    return A @ A.T / (3 * F)


@pytest.mark.parametrize("F", [1, 4, 36])
def test_frechet_distance_matches_scipy_sqrtm(F):
    rs = np.random.RandomState(F)
    mu1, mu2, s1, s2 = rs.normal(size=F), rs.normal(size=F), random_cov(rs, F), random_cov(rs, F)
    assert ev.frechet_distance(mu1, s1, mu2, s2) == pytest.approx(scipy_frechet(mu1, s1, mu2, s2), rel=1e-9)
    got = ev.frechet_distance(torch.from_numpy(mu1), torch.from_numpy(s1), torch.from_numpy(mu2), torch.from_numpy(s2))
    assert got == ev.frechet_distance(mu1, s1, mu2, s2)
    assert abs(ev.frechet_distance(mu1, s1, mu1, s1)) <= 1e-12 * np.trace(s1)


def test_frechet_distance_of_commuting_covariances():
    # S1 = Q diag(a) Q^T, S2 = Q diag(b) Q^T: Tr sqrt(S1 S2) = sum sqrt(a b), so the distance is |dmu|^2 + sum (sqrt a - sqrt b)^2
    rs = np.random.RandomState(1)
    Q, _ = np.linalg.qr(rs.normal(size=(6, 6)))
    a, b = rs.uniform(0.5, 2, 6), rs.uniform(0.5, 2, 6)
    mu1, mu2 = rs.normal(size=6), rs.normal(size=6)
    want = np.sum((mu1 - mu2) ** 2) + np.sum((np.sqrt(a) - np.sqrt(b)) ** 2)
    # (fp64 rounding of Q diag Q^T and of the eigen-solver: a few 1e-16 of the traces, which are ~20x the result)
    assert ev.frechet_distance(mu1, (Q * a) @ Q.T, mu2, (Q * b) @ Q.T) == pytest.approx(want, rel=1e-12)
    assert ev.frechet_distance(mu1, np.diag(a), mu2, np.diag(b)) == pytest.approx(want, rel=1e-13)


def test_frechet_distance_with_a_constant_column():
    rs = np.random.RandomState(2)
    X, Y = rs.normal(size=(500, 5)), rs.normal(0.2, 1.3, size=(500, 5))
    X1, Y1 = np.insert(X, 2, 1.0, axis=1), np.insert(Y, 2, 1.0, axis=1)
    stats = lambda Z: (Z.mean(0), np.cov(Z, rowvar=False))
    full = ev.frechet_distance(*stats(X1), *stats(Y1))
    assert np.isfinite(full)
    assert full == pytest.approx(ev.frechet_distance(*stats(X), *stats(Y)), rel=1e-12)
    # constant in one set only: still finite and equal to scipy's value
    X2 = np.insert(X, 2, rs.normal(size=500), axis=1)
    got = ev.frechet_distance(*stats(X2), *stats(Y1))
    assert np.isfinite(got) and got == pytest.approx(scipy_frechet(*stats(X2), *stats(Y1)), rel=1e-7)


# ------------------------------------------------------------------------------------- 4. fpd and kpd as stated
def ref_fpd(X, Y, min_samples, max_samples, num_batches, num_points, rs, normalise=True):
    if normalise:
        top = np.max(np.abs(X), axis=0)
        X, Y = X / top, Y / top
    sizes = (1 / np.linspace(1.0 / min_samples, 1.0 / max_samples, num_points)).astype("int32")
    vals = []
    for size in sizes:
        pts = []
        for _ in range(num_batches):
            a, b = X[rs.choice(len(X), size=size)], Y[rs.choice(len(Y), size=size)]
            pts.append(scipy_frechet(a.mean(0), np.cov(a, rowvar=False), b.mean(0), np.cov(b, rowvar=False)))
        vals.append(np.mean(pts))
    params, covs = curve_fit(lambda x, i, s: i + s * x, 1 / sizes, vals, bounds=([0, 0], [np.inf, np.inf]))
    free = np.polyfit(1 / sizes, vals, 1)     # (slope, intercept) without bounds
    return params[0], np.sqrt(np.diag(covs)[0]), free


def test_fpd_matches_a_numpy_scipy_loop_inside_the_bounds():
    rs = np.random.RandomState(0)
    X = rs.normal(size=(3000, 8)) * rs.uniform(0.5, 2, 8)
    Y = rs.normal(0.1, 1.1, size=(2500, 8)) * rs.uniform(0.5, 2, 8)
    args = dict(min_samples=300, max_samples=1500, num_batches=5, num_points=6)
    val, err, free = ref_fpd(X, Y, rs=np.random.RandomState(42), **args)
    assert free[0] > 0 and free[1] > 0
    got = ev.fpd(X, Y, **args)                      # private RandomState(42) by default
    assert got[0] == pytest.approx(val, rel=1e-6) and got[1] == pytest.approx(err, rel=1e-3)
    again = ev.fpd(torch.from_numpy(X), torch.from_numpy(Y), rng=np.random.RandomState(42), **args)
    assert again == got
    # the default draws leave numpy's global stream alone
    np.random.seed(7)
    before = np.random.get_state()[1].copy()
    ev.fpd(X, Y, **args)
    assert np.array_equal(before, np.random.get_state()[1])
    # real EFP features, 36 strongly correlated columns
    E1 = ev.efps(random_jets(1500, 8, seed=1), efpset_args=D4)
    E2 = ev.efps(random_jets(1500, 8, seed=2) * np.array([1.2, 1.0, 1.0]), efpset_args=D4)
    args = dict(min_samples=400, max_samples=1200, num_batches=3, num_points=4)
    val, err, _ = ref_fpd(E1, E2, rs=np.random.RandomState(42), **args)
    got = ev.fpd(E1, E2, **args)
    assert got[0] == pytest.approx(val, rel=1e-6) and got[1] == pytest.approx(err, rel=1e-3)


def test_fpd_with_the_slope_bound_active():
    # far-apart means, two columns, one batch per size: the finite-sample bias is far below the batch-to-batch noise, and with
    # these draws the unconstrained slope is negative
    rs = np.random.RandomState(3)
    X, Y = rs.normal(size=(2000, 2)), rs.normal(3.0, 1.0, size=(2000, 2))
    args = dict(min_samples=200, max_samples=1000, num_batches=1, num_points=5, normalise=False)
    val, err, free = ref_fpd(X, Y, rs=np.random.RandomState(SLOPE_SEED), **args)
    assert free[0] < 0, free
    got = ev.fpd(X, Y, seed=SLOPE_SEED, **args)
    assert got[0] == pytest.approx(val, rel=1e-6) and got[1] == pytest.approx(err, rel=1e-3)
    # and the intercept bound: y = slope * x through the origin with noise that pulls the free intercept below 0
    x = np.array([1.0, 2.0, 3.0, 4.0])
    y = np.array([0.8, 2.3, 2.9, 4.2])
    assert np.polyfit(x, y, 1)[1] < 0
    p, c = curve_fit(lambda x, i, s: i + s * x, x, y, bounds=([0, 0], [np.inf, np.inf]))
    a, b, e = ev._bounded_line_fit(x, y)
    assert abs(a) <= 1e-6 * b and b == pytest.approx(p[1], rel=1e-6) and e == pytest.approx(np.sqrt(c[0, 0]), rel=1e-3)


SLOPE_SEED = 4         # (of seeds 0 .. 11, seeds 1, 4, 5, 8, 9, 10 give a negative free slope on these inputs)


def ref_kpd(X, Y, num_batches, batch_size, degree, rs):
    top = np.max(np.abs(X), axis=0)
    X, Y = X / top, Y / top
    vals, size = [], 0.0
    for _ in range(num_batches):
        a, b = X[rs.choice(len(X), size=batch_size)], Y[rs.choice(len(Y), size=batch_size)]
        K = lambda p, q: (p @ q.T / p.shape[1] + 1.0) ** degree
        XX, YY, XY = K(a, a), K(b, b), K(a, b)
        m = batch_size
        t = ((XX.sum() - np.trace(XX)) / (m * (m - 1)), (YY.sum() - np.trace(YY)) / (m * (m - 1)), 2 * np.mean(XY))
        size = max(size, *t)
        vals.append(t[0] + t[1] - t[2])
    lo, hi = np.percentile(vals, [16.275, 83.725])
    return np.median(vals), (hi - lo) / 2, size


@pytest.mark.parametrize("degree", [4, 3])
def test_kpd_matches_a_direct_numpy_evaluation(degree, monkeypatch):
    E1 = ev.efps(random_jets(2000, 8, seed=1), efpset_args=D4)
    E2 = ev.efps(random_jets(2000, 8, seed=2) * np.array([1.2, 1.0, 1.0]), efpset_args=D4)
    monkeypatch.setattr(ev, "_KPD_ROWS", 300)       # several uneven row chunks
    med, err, size = ref_kpd(E1, E2, 6, 700, degree, np.random.RandomState(42))
    got = ev.kpd(E1, E2, num_batches=6, batch_size=700, degree=degree)
    assert abs(got[0] - med) <= 1e-9 * size and abs(got[1] - err) <= 1e-9 * size
    assert got[0] > 0 and got[1] > 0
    assert ev.kpd(torch.from_numpy(E1), torch.from_numpy(E2), num_batches=6, batch_size=700, degree=degree,
                  rng=np.random.RandomState(42)) == got


# ------------------------------------------------------------------------------------- 5. order freedom
def test_fpd_and_kpd_do_not_depend_on_the_column_order():
    E1 = ev.efps(random_jets(2000, 10, seed=11), efpset_args=D4)
    E2 = ev.efps(random_jets(2000, 10, seed=12) * np.array([1.1, 1.1, 1.0]), efpset_args=D4)
    perm = np.random.RandomState(5).permutation(36)
    fargs = dict(min_samples=500, max_samples=1500, num_batches=3, num_points=4)
    f0, f1 = ev.fpd(E1, E2, **fargs), ev.fpd(E1[:, perm], E2[:, perm], **fargs)
    print("fpd", f0, f1)
    assert f1[0] == pytest.approx(f0[0], rel=1e-9) and f1[1] == pytest.approx(f0[1], rel=1e-9)
    k0, k1 = ev.kpd(E1, E2, num_batches=4, batch_size=800), ev.kpd(E1[:, perm], E2[:, perm], num_batches=4, batch_size=800)
    print("kpd", k0, k1)
    assert k1[0] == pytest.approx(k0[0], rel=1e-9) and k1[1] == pytest.approx(k0[1], rel=1e-9)


# ------------------------------------------------------------------------------------- 6. plumbing
def test_evaluate_appends_fpd_and_kpd_only_with_efps(tmp_path):
    real, gen = random_jets(400, 12, seed=3), random_jets(400, 12, seed=4)
    keys, eval_keys = checkpoint.loss_keys(kpd=True)
    assert keys[-2:] == ["fpd", "kpd"] and "kpd" not in checkpoint.loss_keys()[0]
    plain = ev.evaluate({k: [] for k in keys}, real, gen, "g", num_w1_eval_samples=100, rng=np.random.RandomState(1))
    assert plain["fpd"] == [] and plain["kpd"] == []
    re_, ge_ = ev.efps(real, efpset_args=D4), ev.efps(gen, efpset_args=D4)
    fargs = dict(min_samples=100, max_samples=300, num_batches=2, num_points=4)
    kargs = dict(num_batches=3, batch_size=150)
    losses = {k: [] for k in keys}
    ev.evaluate(losses, real, gen, "g", num_w1_eval_samples=100, rng=np.random.RandomState(1), real_efps=re_, gen_efps=ge_,
                fpd_args=fargs, kpd_args=kargs)
    assert np.shape(losses["fpd"][0]) == (2,) and np.shape(losses["kpd"][0]) == (2,)
    assert np.array_equal(losses["fpd"][0], np.array(ev.fpd(re_, ge_, **fargs)))
    assert np.array_equal(losses["kpd"][0], np.array(ev.kpd(re_, ge_, **kargs)))
    for k in ("w1p", "w1m"):        # the earlier keys' draws are what they were
        assert np.array_equal(losses[k][0], plain[k][0])
    # one evaluation round-trips with its shape
    path = str(tmp_path / "losses")
    checkpoint.save_losses({k: losses[k] for k in ("fpd", "kpd")}, path)
    back = checkpoint.load_losses(path, ("fpd", "kpd"), eval_keys)
    for k in ("fpd", "kpd"):
        assert np.shape(back[k]) == (1, 2)
        np.testing.assert_allclose(np.array(back[k]), np.array(losses[k]), rtol=1e-15)


def test_best_epoch_update():
    best = [[0, 10.0]]
    losses = {"fpd": [np.array([0.5, 0.1])]}
    assert not checkpoint.best_epoch_update(best, 0, losses) and best == [[0, 10.0]]       # epoch 0 never counts
    assert checkpoint.best_epoch_update(best, 5, losses) and best[-1] == [5, pytest.approx(0.6)]
    losses["fpd"].append(np.array([0.55, 0.1]))
    assert not checkpoint.best_epoch_update(best, 10, losses) and len(best) == 2
    losses["fpd"].append(np.array([0.3, 0.05]))
    assert checkpoint.best_epoch_update(best, 15, losses) and best[-1] == [15, pytest.approx(0.35)]
    assert not checkpoint.best_epoch_update(best, 20, {"w1m": []}) and not checkpoint.best_epoch_update(best, 20, {"fpd": []})


def test_jet_efps_d4_is_declared_and_exported():
    txt = open(os.path.join(ROOT, "include", "mpgan_amd.h")).read()
    assert re.search(r"^int\s+mpg_jet_efps_d4\s*\(", txt, flags=re.M)
    assert int(re.search(r"^#define\s+MPG_JET_EFPS_D4_PRIMES\s+(\d+)\s*$", txt, flags=re.M).group(1)) == ev.NUM_EFP_D4_PRIMES
    from mpgan_amd import _lib
    assert "mpg_jet_efps_d4" in _lib.SIGNATURES
    assert hasattr(_lib.lib(), "mpg_jet_efps_d4")
