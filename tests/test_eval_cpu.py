"""CPU: the evaluation metrics (mpgan_amd/evaluation.py) -- the fp64 observables against brute-force definitions, the W1
distances against scipy, the reference's evaluate layout -- and the C ABI entry point of their kernel."""
import os
import re

import numpy as np
import pytest
import torch
from scipy.stats import wasserstein_distance

from mpgan_amd import checkpoint, evaluation as ev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_jets(n, N, seed, pad_frac=0.3):
    """[n, N, 3] (eta, phi, pt) with zero-pT padding scattered through each jet (never all of it)."""
    rs = np.random.RandomState(seed)
    eta = rs.normal(0, 0.2, size=(n, N))
    phi = rs.normal(0, 0.2, size=(n, N))
    pt = rs.exponential(0.05, size=(n, N))
    pad = rs.rand(n, N) < pad_frac
    pad[:, rs.randint(N)] = False
    return np.stack([eta, phi, np.where(pad, 0.0, pt)], axis=2)


def brute_efps(jets, normed=True):
    """The five multigraphs as 4-index sums of their edge lists (a, b, c, d), straight from the definitions."""
    out = []
    for jet in jets:
        eta, phi, pt = jet[:, 0], jet[:, 1], jet[:, 2]
        z = pt / pt.sum() if normed else pt
        th = np.sqrt((eta[:, None] - eta[None, :]) ** 2 + (phi[:, None] - phi[None, :]) ** 2)
        e = lambda spec, *ops: np.einsum("a,b,c,d," + spec, z, z, z, z, *ops)
        out.append([
            e("ab,ab,bc,cd->", th, th, th, th),   # a=b-c-d
            e("ab,bc,bc,cd->", th, th, th, th),   # a-b=c-d
            e("ca,ca,cb,cd->", th, th, th, th),   # 3-star, one edge doubled
            e("ab,bc,ac,cd->", th, th, th, th),   # triangle + pendant
            e("ab,bc,cd,da->", th, th, th, th),   # 4-cycle
        ])
    return np.array(out)


def four_vector_mass(jets):
    eta, phi, pt = jets[..., 0], jets[..., 1], jets[..., 2]
    E = (pt * np.cosh(eta)).sum(1)
    px, py, pz = (pt * np.cos(phi)).sum(1), (pt * np.sin(phi)).sum(1), (pt * np.sinh(eta)).sum(1)
    return np.sqrt(np.maximum(E ** 2 - px ** 2 - py ** 2 - pz ** 2, 0)), px, py, pz


@pytest.mark.parametrize("N", [1, 2, 5, 17, 30])
def test_efps_match_brute_force(N):
    jets = random_jets(6, N, seed=N)
    got = ev.efps(jets)
    ref = brute_efps(jets)
    assert got.shape == (6, 5) and got.dtype == np.float64
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    assert np.all(np.abs(got - ref) <= 1e-12 * np.abs(ref) + 1e-300)


def test_two_particle_closed_form_and_single_particle():
    r = 0.37
    jet = np.array([[[0.1, -0.2, 0.5], [0.1 + r * 0.6, -0.2 + r * 0.8, 0.5]]])
    got = ev.efps(jet)[0]
    np.testing.assert_allclose(got[[0, 1, 2, 4]], r ** 4 / 8, rtol=1e-13)
    assert abs(got[3]) < 1e-18
    assert np.all(ev.efps(np.array([[[0.3, 0.1, 0.7], [0.0, 0.0, 0.0]]])) == 0)


def test_permutation_and_zero_padding_change_nothing():
    jets = random_jets(4, 12, seed=3, pad_frac=0.0)
    base_e, base_k = ev.efps(jets), np.stack(list(ev.jet_features(jets).values()), 1)
    rs = np.random.RandomState(0)
    perm = jets[:, rs.permutation(12)]
    padded = np.zeros((4, 20, 3))
    slots = np.sort(rs.choice(20, 12, replace=False))
    padded[:, slots] = jets
    for other in (perm, padded):
        np.testing.assert_allclose(ev.efps(other), base_e, rtol=1e-12)
        np.testing.assert_allclose(np.stack(list(ev.jet_features(other).values()), 1), base_k, rtol=1e-12, atol=1e-15)


def test_unnormalised_efps_scale_with_the_fourth_power_of_the_pt_sum():
    jets = random_jets(5, 10, seed=7)
    s = jets[..., 2].sum(1)
    np.testing.assert_allclose(ev.efps(jets, normed=False), ev.efps(jets) * s[:, None] ** 4, rtol=1e-12)
    np.testing.assert_allclose(ev.efps(jets, normed=False), brute_efps(jets, normed=False), rtol=1e-12)


def test_jet_features_match_an_explicit_four_vector_sum():
    jets = random_jets(50, 30, seed=11)
    f = ev.jet_features(jets)
    m, px, py, pz = four_vector_mass(jets)
    np.testing.assert_allclose(f["mass"], m, rtol=1e-9)
    np.testing.assert_allclose(f["pt"], np.hypot(px, py), rtol=1e-13)
    np.testing.assert_allclose(f["eta"], np.arcsinh(pz / np.hypot(px, py)), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(f["phi"], np.arctan2(py, px), rtol=1e-12, atol=1e-14)
    # torch in, torch out (same values); the mask column of [n, N, 4] is ignored
    t = torch.from_numpy(np.concatenate([jets, np.ones_like(jets[..., :1])], 2))
    assert torch.allclose(ev.jet_features(t)["mass"], torch.from_numpy(f["mass"]), rtol=1e-14, atol=0)
    # an all-padding jet gives zeros, not NaN
    assert all(float(v[0]) == 0 for v in ev.jet_features(np.zeros((1, 4, 3))).values())


@pytest.mark.parametrize("nu,nv,ties", [(100, 100, False), (37, 250, False), (60, 45, True), (1, 9, True)])
def test_wasserstein_1d_matches_scipy(nu, nv, ties):
    rs = np.random.RandomState(nu * nv)
    u, v = rs.normal(size=nu), rs.normal(0.3, 1.5, size=nv)
    if ties:
        u, v = np.round(u, 1), np.round(v, 1)
    got = float(ev.wasserstein_1d(torch.from_numpy(u), torch.from_numpy(v)))
    assert got == pytest.approx(wasserstein_distance(u, v), rel=1e-12, abs=1e-15)
    assert float(ev.wasserstein_1d(u, u)) == 0.0


def _ref_batches(x1, x2, k, nb, rs, fn):
    out = []
    for _ in range(nb):
        i1, i2 = rs.choice(len(x1), k), rs.choice(len(x2), k)
        out.append(fn(x1[i1], x2[i2]))
    return np.array(out)


def test_w1m_w1p_w1efp_match_a_scipy_loop_with_the_same_draws():
    real, gen = random_jets(300, 20, seed=1), random_jets(250, 20, seed=2)
    gen[..., 2] *= 1.1
    k, nb = 80, 4
    # w1m
    m1, m2 = four_vector_mass(real)[0], four_vector_mass(gen)[0]
    ref = _ref_batches(m1, m2, k, nb, np.random.RandomState(5), wasserstein_distance)
    mean, std = ev.w1m(real, gen, num_eval_samples=k, num_batches=nb, rng=np.random.RandomState(5))
    assert mean == pytest.approx(ref.mean(), rel=1e-9) and std == pytest.approx(ref.std(), rel=1e-7)
    # w1p, zero-norm particles excluded, per feature
    def w1p_one(a, b):
        pa = a[np.linalg.norm(a, axis=2) != 0]
        pb = b[np.linalg.norm(b, axis=2) != 0]
        return [wasserstein_distance(pa[:, f], pb[:, f]) for f in range(3)]
    ref = _ref_batches(real, gen, k, nb, np.random.RandomState(6), w1p_one)
    means, stds = ev.w1p(real, gen, num_eval_samples=k, num_batches=nb, average_over_features=False,
                         rng=np.random.RandomState(6))
    np.testing.assert_allclose(means, ref.mean(0), rtol=1e-12)
    np.testing.assert_allclose(stds, ref.std(0), rtol=1e-9)
    mean, std = ev.w1p(real, gen, num_eval_samples=k, num_batches=nb, rng=np.random.RandomState(6))
    assert mean == pytest.approx(ref.mean(0).mean(), rel=1e-12) and std == pytest.approx(np.linalg.norm(ref.std(0)), rel=1e-9)
    # w1efp
    e1, e2 = brute_efps(real[:, :8]), brute_efps(gen[:, :8])
    ref = _ref_batches(e1, e2, k, nb, np.random.RandomState(7),
                       lambda a, b: [wasserstein_distance(a[:, i], b[:, i]) for i in range(5)])
    means, stds = ev.w1efp(real[:, :8], gen[:, :8], num_eval_samples=k, num_batches=nb, average_over_efps=False,
                           rng=np.random.RandomState(7))
    np.testing.assert_allclose(means, ref.mean(0), rtol=1e-9)
    np.testing.assert_allclose(stds, ref.std(0), rtol=1e-6)


def test_default_rng_is_numpys_global_stream():
    real, gen = random_jets(100, 10, seed=1), random_jets(100, 10, seed=2)
    np.random.seed(42)
    a = ev.w1m(real, gen, num_eval_samples=30, num_batches=3)
    b = ev.w1m(real, gen, num_eval_samples=30, num_batches=3, rng=np.random.RandomState(42))
    assert a == b


def test_evaluate_layout_and_losses_round_trip(tmp_path):
    real, gen = random_jets(400, 16, seed=3), random_jets(400, 16, seed=4)
    keys, eval_keys = checkpoint.loss_keys(efp=True)
    losses = {k: [] for k in keys}
    for epoch in range(2):
        ev.evaluate(losses, real, gen, "g", num_particles=16, num_w1_eval_samples=100, rng=np.random.RandomState(epoch))
    assert [np.shape(x) for x in losses["w1p"]] == [(6,), (6,)]
    assert [np.shape(x) for x in losses["w1m"]] == [(2,), (2,)]
    assert [np.shape(x) for x in losses["w1efp"]] == [(10,), (10,)]
    assert losses["fpd"] == [] and losses["D"] == []
    assert all(np.all(np.isfinite(x)) and np.all(np.asarray(x) >= 0) for k in ("w1p", "w1m", "w1efp") for x in losses[k])
    # 400 // 100 = 4 batches, drawn in the reference's order: w1p first, then w1m
    rs = np.random.RandomState(0)
    ev.w1p(real, gen, num_eval_samples=100, num_batches=4, rng=rs)
    ref = ev.w1m(real, gen, num_eval_samples=100, num_batches=4, rng=rs)
    np.testing.assert_allclose(losses["w1m"][0], ref, rtol=1e-12)
    path = str(tmp_path / "losses")
    metrics = ("w1p", "w1m", "w1efp")
    checkpoint.save_losses({k: losses[k] for k in metrics}, path)
    back = checkpoint.load_losses(path, metrics, eval_keys, start_epoch=1)
    for k in metrics:
        np.testing.assert_allclose(np.array(back[k]), np.array(losses[k]), rtol=1e-15)
    with pytest.raises(NotImplementedError):
        ev.evaluate({"fpnd": []}, real, gen, "g", num_w1_eval_samples=100)


def test_jet_obs_is_declared_and_exported():
    txt = open(os.path.join(ROOT, "include", "mpgan_amd.h")).read()
    assert re.search(r"^int\s+mpg_jet_obs\s*\(", txt, flags=re.M)
    defs = {k: int(v) for k, v in re.findall(r"^#define\s+(MPG_JET_OBS_\w+)\s+(\d+)\s*$", txt, flags=re.M)}
    assert defs["MPG_JET_OBS_MAX_N"] == ev.MAX_PARTICLES
    from mpgan_amd import _lib
    assert "mpg_jet_obs" in _lib.SIGNATURES
    assert hasattr(_lib.lib(), "mpg_jet_obs")
