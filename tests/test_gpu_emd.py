"""GPU: the exact jet EMD kernel (mpg_jet_emd, csrc/jet_emd.hip) against the golden linear-programming optima of
tests/gen_golden_emd.py, its determinism and argument checks, and coverage / MMD on the device against the host path.

Bar: |got - ref| <= 2e-5 S, S = (sum pT_A + sum pT_B) max(1, theta_max / R).  An exact basic solution in fp32 is at most
n + m + 1 <= 61 flows, each a chain of subtractions of the weights, times a cost: about 61 x 2^-24 S ~ 4e-6 S; 2e-5 is five
times that, and the bar mpg_jet_obs meets for the EFPs."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from mpgan_amd import _lib, evaluation as ev

pytestmark = pytest.mark.gpu

GOLDENS = ("emd_n30_gluon", "emd_n30_top", "emd_n150", "emd_n1", "emd_n2", "emd_n31", "emd_n32", "emd_n33", "emd_hand")
BAR = 2e-5


def golden(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    return d["a"], d["b"], d["D"]


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


def device_emd(a, b, R=1.0):
    """(D fp32, status) straight from the C entry, on cuda:0."""
    a, b = torch.as_tensor(a).float().contiguous().cuda(), torch.as_tensor(b).float().contiguous().cuda()
    na, nb, N, ld = a.shape[0], b.shape[0], a.shape[1], a.shape[2]
    D = torch.full((na, nb), -1.0, device="cuda")
    st = torch.full((na, nb), -7, dtype=torch.int32, device="cuda")
    rc = _lib.lib().mpg_jet_emd(a.data_ptr(), N * ld, b.data_ptr(), N * ld, ld, na, nb, N, R, D.data_ptr(), st.data_ptr(),
                                torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    return D.cpu().numpy(), st.cpu().numpy()


@pytest.mark.parametrize("name", GOLDENS)
def test_kernel_matches_golden(name):
    a, b, D = golden(name)
    got, status = device_emd(a, b)
    S = scales(a, b)
    err = np.abs(got.astype(np.float64) - D) / S.clip(min=1e-300)
    print("%s: max |got - ref| / S = %.3e (bar %.0e)" % (name, err.max(), BAR))
    assert np.all(status == 0)
    assert np.all(np.isfinite(got))
    assert np.all(np.abs(got.astype(np.float64) - D) <= BAR * S), float(err.max())
    # the public entry: same bits, a CUDA tensor back; a fourth (mask) column is stepped over
    out = ev.emds(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda())
    assert out.is_cuda and out.dtype == torch.float32 and np.array_equal(out.cpu().numpy(), got)
    a4, b4 = np.concatenate([a, a[..., 2:]], 2), np.concatenate([b, b[..., 2:]], 2)
    assert np.array_equal(device_emd(a4, b4)[0], got)


def test_radius():
    a, b, _ = golden("emd_n30_gluon")
    a, b = a[:8], b[:8]
    ref = ev.emds(a, b, R=0.4)                                  # the host build of the same solver, fp64
    got, status = device_emd(a, b, R=0.4)
    assert np.all(status == 0) and np.all(np.abs(got - ref) <= BAR * scales(a, b, 0.4))


@pytest.mark.parametrize("name", ["emd_n30_top", "emd_n150", "emd_n33"])
def test_two_launches_are_bit_identical(name):
    a, b, _ = golden(name)
    assert np.array_equal(device_emd(a, b)[0], device_emd(a, b)[0])


@pytest.mark.parametrize("na", [1, 7, 100])
@pytest.mark.parametrize("nb", [1, 7, 100])
def test_shapes_and_duplicated_rows(na, nb):
    """Draws with replacement from the golden jets: every entry is the golden's, and equal jets give equal bits wherever they
    sit in the launch."""
    a, b, D = golden("emd_n30_gluon")
    full, _ = device_emd(a, b)
    rs = np.random.RandomState(na * 1000 + nb)
    ia, ib = rs.choice(len(a), na), rs.choice(len(b), nb)
    got, status = device_emd(a[ia], b[ib])
    assert got.shape == (na, nb) and np.all(status == 0)
    assert np.array_equal(got, full[ia][:, ib])
    assert np.all(np.abs(got - D[ia][:, ib]) <= BAR * scales(a, b)[ia][:, ib])


def test_hand_made_duplicate_is_bit_identical():
    a, b, _ = golden("emd_hand")
    got, status = device_emd(a, b)
    assert np.all(status == 0)
    assert np.array_equal(got[3], got[4]) and np.array_equal(got[:, 3], got[:, 4])
    assert got[0, 0] == 0.0 and got[3, 3] <= BAR * 2.6 and got[3, 4] <= BAR * 2.6


def test_n_out_of_range_returns_minus_one_without_launching():
    lib = _lib.lib()
    x = torch.zeros(2, 200, 3, device="cuda")
    out = torch.full((2, 2), -1.0, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    for N in (0, ev.MAX_PARTICLES + 1):
        assert lib.mpg_jet_emd(x.data_ptr(), 600, x.data_ptr(), 600, 3, 2, 2, N, 1.0, out.data_ptr(), None, stream) == -1
    assert lib.mpg_jet_emd(x.data_ptr(), 600, x.data_ptr(), 600, 3, 0, 2, 30, 1.0, out.data_ptr(), None, stream) == -1
    torch.cuda.synchronize()
    assert torch.all(out == -1.0)
    with pytest.raises(ValueError):
        ev.emds(torch.zeros(2, ev.MAX_PARTICLES + 1, 3, device="cuda"), torch.zeros(2, ev.MAX_PARTICLES + 1, 3, device="cuda"))
    assert lib.mpg_jet_emd(x.data_ptr(), 600, x.data_ptr(), 600, 3, 2, 2, ev.MAX_PARTICLES, 1.0, out.data_ptr(), None, stream) == 0
    torch.cuda.synchronize()
    assert torch.all(out == 0.0)                                # empty jets at the largest N: all zeros


def test_non_finite_input_raises():
    a, b, _ = golden("emd_n2")
    bad = a.copy()
    bad[0, :, 0] = np.nan
    with pytest.raises(RuntimeError, match="status"):
        ev.emds(torch.from_numpy(bad).cuda(), torch.from_numpy(b).cuda())


def test_cov_mmd_on_the_device_equals_the_host_path():
    """N = 30, k = 48, 3 batches, the same seeded draws: MMD within the fp32 bar, coverage equal exactly.  The gluon set's
    nearest neighbours are 4.0e-3 apart at least (5.5 bars, asserted by tests/gen_golden_emd.py); draws with replacement
    repeat jets, and those exact ties fall the same way on both paths because equal jets give equal bits."""
    d = np.load(os.path.join(GOLDEN, "emd_n30_gluon.npz"), allow_pickle=False)
    gen, real = d["a"], d["b"]
    assert bool(d["decides_coverage"]) and float(d["gap"]) >= 4 * float(d["bar"])
    cov_h, mmd_h = ev.cov_mmd(real, gen, num_eval_samples=48, num_batches=3, rng=np.random.RandomState(5))
    cov_d, mmd_d = ev.cov_mmd(torch.from_numpy(real).cuda(), torch.from_numpy(gen).cuda(), num_eval_samples=48, num_batches=3,
                              rng=np.random.RandomState(5))
    print("coverage host %.6f device %.6f; mmd host %.9f device %.9f" % (cov_h, cov_d, mmd_h, mmd_d))
    assert cov_d == cov_h
    assert abs(mmd_d - mmd_h) <= BAR * scales(gen, real).max()
    # every row and every column of one batch: the same nearest neighbour on both paths
    rs = np.random.RandomState(6)
    i_real, i_gen = rs.choice(48, 48), rs.choice(48, 48)
    Dh = ev.emds(gen[i_gen], real[i_real])
    Dd = ev.emds(torch.from_numpy(gen[i_gen]).cuda(), torch.from_numpy(real[i_real]).cuda())
    assert np.array_equal(ev._first_argmin(Dd).cpu().numpy(), np.argmin(Dh, axis=1))
    assert np.array_equal(ev._first_argmin(Dd.t()).cpu().numpy(), np.argmin(Dh, axis=0))


def test_evaluate_with_coverage_and_mmd_on_the_device():
    d = np.load(os.path.join(GOLDEN, "emd_n30_gluon.npz"), allow_pickle=False)
    gen, real = torch.from_numpy(d["a"]).cuda(), torch.from_numpy(d["b"]).cuda()
    losses = ev.evaluate({"w1m": [], "coverage": [], "mmd": []}, real, gen, "g", num_w1_eval_samples=16,
                         num_cov_mmd_eval_samples=20, rng=np.random.RandomState(1))
    host = ev.evaluate({"w1m": [], "coverage": [], "mmd": []}, real.cpu(), gen.cpu(), "g", num_w1_eval_samples=16,
                       num_cov_mmd_eval_samples=20, rng=np.random.RandomState(1))
    assert losses["coverage"] == host["coverage"]
    assert abs(losses["mmd"][0] - host["mmd"][0]) <= BAR * 40
