"""GPU: the exact jet EMD kernel (mpg_jet_emd, csrc/jet_emd.hip) against the golden linear-programming optima of
tests/gen_golden_emd.py, its determinism and argument checks, and coverage / MMD on the device against the host path.

Bar: |got - ref| <= 2e-5 S, S = (sum pT_A + sum pT_B) max(1, theta_max / R).  An exact basic solution in fp32 is at most
n + m + 1 <= 61 flows, each a chain of subtractions of the weights, times a cost: about 61 x 2^-24 S ~ 4e-6 S; 2e-5 is five
times that, and the bar mpg_jet_obs meets for the EFPs.  The larger pairs of the second half of this file carry the same rule
with their own flow count: max(2e-5, 5 (n_a + n_b + 1) 2^-24) S, 9.6e-5 S for two full jets of 160."""
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


# ------------------------------------------------------------------------------------------- node slots and launch shapes
# The kernel keeps node v in register slot v / 64 of lane v % 64 and is built for 1, 2 and 6 slots: 2N + 2 <= 64, <= 128,
# more.  A workgroup runs 4 waves up to N = 60, 3 to 69, 2 to 86, 1 from 87, on (3 (2N + 2) + (N + 1)^2) floats of LDS per
# wave, rounded up to 4: above 64 KiB from N = 125.  The emd_slots_n{N} sets (tests/gen_golden_emd.py) are 5 x 5 pairs of two
# jets with every slot live, a half-empty jet, one particle and an empty jet, on both sides of each of those lines; their
# full pairs hold all 2N + 2 nodes.  The bar follows the rule of the module docstring to these sizes: a basic solution has at
# most n_a + n_b + 1 flows, each good to 2^-24 S, times five -- and never below the 2e-5 S of the small sets.
SLOT_NS = (31, 32, 60, 61, 63, 64, 69, 70, 86, 87, 124, 125, 160)


def slots_golden(name, R=1.0):
    d = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    return d["a"], d["b"], d["D" if R == 1.0 else "D_R04"], d["nodes"]


def bars(a, b, R=1.0):
    """bar[i, j] = max(2e-5, 5 (n_a + n_b + 1) 2^-24) S[i, j]"""
    flows = (np.asarray(a)[:, None, :, 2] > 0).sum(2) + (np.asarray(b)[None, :, :, 2] > 0).sum(2) + 1
    return np.maximum(BAR, 5 * flows * 2.0 ** -24) * scales(a, b, R)


def launch_shape(N):
    """(register slots per lane, waves per workgroup, LDS bytes of a workgroup) of the launch for N particles."""
    per_wave = 4 * ((3 * (2 * N + 2) + (N + 1) ** 2 + 3) // 4 * 4)
    waves = max(1, min(4, 65536 // per_wave))
    return (1 if 2 * N + 2 <= 64 else 2 if 2 * N + 2 <= 128 else 6), waves, waves * per_wave


def raw_emd(a, ld_jet_a, b, ld_jet_b, ld_part, na, nb, N, R=1.0, slack=0):
    """mpg_jet_emd on the flat CUDA buffers a and b; (D fp32 [na * nb + slack], status), the slack poisoned like the rest."""
    D = torch.full((na * nb + slack,), -1.0, device="cuda")
    st = torch.full((na * nb + slack,), -7, dtype=torch.int32, device="cuda")
    rc = _lib.lib().mpg_jet_emd(a.data_ptr(), ld_jet_a, b.data_ptr(), ld_jet_b, ld_part, na, nb, N, R, D.data_ptr(), st.data_ptr(),
                                torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    return D.cpu().numpy(), st.cpu().numpy()


def host_status(a, b, R=1.0):
    """Statuses of the host build of the same solver."""
    a, b = torch.as_tensor(a).float().contiguous(), torch.as_tensor(b).float().contiguous()
    na, nb, N = a.shape[0], b.shape[0], a.shape[1]
    D, st = torch.empty(na, nb, dtype=torch.float64), torch.full((na, nb), -7, dtype=torch.int32)
    assert _lib.lib().mpg_jet_emd_host(a.data_ptr(), 3 * N, b.data_ptr(), 3 * N, 3, na, nb, N, R, D.data_ptr(), st.data_ptr(), 16) == 0
    return st.numpy()


def check_against_lp(name, got, status, a, b, D, R=1.0):
    bar, diff = bars(a, b, R), np.abs(got.astype(np.float64) - D)
    S = scales(a, b, R).clip(min=1e-300)                          # (two empty jets: S = 0, and the distance is 0 exactly)
    k = np.unravel_index(np.argmax(diff / S), S.shape)
    flows = (a[:, None, :, 2] > 0).sum(2) + (b[None, :, :, 2] > 0).sum(2) + 1
    big = flows == flows.max()
    print("%s R = %g: max |got - ref| / S = %.3e (bar %.2e S there); over the largest pairs %.3e (bar %.2e S)"
          % (name, R, (diff / S.clip(min=1e-300)).max(), bar[k] / S[k], (diff / S)[big].max(), (bar / S)[big].max()))
    assert np.all(status == 0)
    assert np.all(np.isfinite(got))
    assert np.all(diff <= bar), float((diff / S.clip(min=1e-300)).max())


@pytest.mark.parametrize("R", [1.0, 0.4])
@pytest.mark.parametrize("N", SLOT_NS)
def test_every_node_slot_and_launch_shape_against_the_lp(N, R):
    name = "emd_slots_n%d" % N
    a, b, D, nodes = slots_golden(name, R)
    assert a.shape == b.shape == (5, N, 3)
    # what this launch covers: the full pairs fill every node, so the last lane and the last slot in use hold a live node
    assert np.all(nodes[:2, :2] == 2 * N + 2) and nodes.max() == 2 * N + 2
    slots, waves, lds = launch_shape(N)
    print("%s: %d nodes at most (slot %d, lane %d), %d-slot build, %d waves per workgroup, %d bytes of LDS"
          % (name, nodes.max(), (nodes.max() - 1) // 64, (nodes.max() - 1) % 64, slots, waves, lds))
    assert slots == (1 if N <= 31 else 2 if N <= 63 else 6) and (nodes.max() - 1) // 64 == (2 * N + 1) // 64 < slots
    assert waves == (4 if N <= 60 else 3 if N <= 69 else 2 if N <= 86 else 1) and (lds > 65536) == (N >= 125)
    got, status = device_emd(a, b, R=R)
    check_against_lp(name, got, status, a, b, D, R)


@pytest.mark.parametrize("N", [60, 61, 70, 87])
def test_pair_tail_leaves_the_memory_behind_the_outputs_alone(N):
    """25 pairs on 4, 3, 2 and 1 waves per workgroup: the last workgroup is partly empty for 4, 3 and 2."""
    a, b, D, _ = slots_golden("emd_slots_n%d" % N)
    waves = launch_shape(N)[1]
    assert waves == {60: 4, 61: 3, 70: 2, 87: 1}[N] and (25 % waves != 0 or waves == 1)
    ref, ref_status = device_emd(a, b)
    got, status = raw_emd(torch.from_numpy(a).cuda(), 3 * N, torch.from_numpy(b).cuda(), 3 * N, 3, 5, 5, N, slack=64)
    assert np.all(got[25:] == -1.0) and np.all(status[25:] == -7)
    assert np.array_equal(got[:25].reshape(5, 5), ref) and np.all(status[:25] == 0) and np.all(ref_status == 0)
    assert np.all(np.abs(ref.astype(np.float64) - D) <= bars(a, b))


@pytest.mark.parametrize("N", [63, 64, 160])
def test_placement_in_the_launch_does_not_change_the_bits(N):
    a, b, _, _ = slots_golden("emd_slots_n%d" % N)
    full, status = device_emd(a, b)
    assert np.all(status == 0)
    assert np.array_equal(device_emd(a[::-1].copy(), b[::-1].copy())[0], full[::-1, ::-1])
    for i in (0, 2):                                              # a full jet, the half-empty one
        assert np.array_equal(device_emd(a[i:i + 1], b)[0], full[i:i + 1])
        assert np.array_equal(device_emd(a, b[i:i + 1])[0], full[:, i:i + 1])


@pytest.mark.parametrize("N", [32, 125])
def test_strides_of_a_and_b_differ_and_the_gaps_are_nan(N):
    """ld_part = 4, ld_jet_a = 4N + 5, ld_jet_b = 4N; NaN in the fourth column and in every gap: the bits of the contiguous
    launch."""
    a, b, _, _ = slots_golden("emd_slots_n%d" % N)
    full, status = device_emd(a, b)
    assert np.all(status == 0)
    lda, ldb = 4 * N + 5, 4 * N
    bbuf = np.full((5, N, 4), np.nan, np.float32)
    bbuf[:, :, :3] = a
    abuf = np.full((5, lda), np.nan, np.float32)
    abuf[:, :4 * N] = bbuf.reshape(5, 4 * N)
    bbuf[:, :, :3] = b
    assert np.isnan(abuf).sum() == 5 * (N + 5) and np.isnan(bbuf).sum() == 5 * N
    got, status = raw_emd(torch.from_numpy(abuf).cuda(), lda, torch.from_numpy(bbuf).cuda(), ldb, 4, 5, 5, N)
    assert np.all(status == 0)
    assert np.array_equal(got.reshape(5, 5), full)


@pytest.mark.parametrize("N", [63, 160])
def test_scaling_every_pt_by_a_power_of_two_scales_the_distances_exactly(N):
    """The weights meet only sums, differences, minima and one product with a cost; costs and potentials never see them
    (tests/test_emd_cpu.py asserts the same of the host build)."""
    a, b, _, _ = slots_golden("emd_slots_n%d" % N)
    full, status = device_emd(a, b)
    assert np.all(status == 0)
    for k in (10, -10):
        f = np.array([1, 1, 2.0 ** k], np.float32)
        got, status = device_emd(a * f, b * f)
        assert np.all(status == 0)
        assert np.array_equal(got, full * np.float32(2.0 ** k))


def test_symmetry():
    a, b, D, _ = slots_golden("emd_slots_n64")
    Dab, sab = device_emd(a, b)
    Dba, sba = device_emd(b, a)
    assert np.all(sab == 0) and np.all(sba == 0)
    bar = bars(a, b) + bars(b, a).T
    diff = np.abs(Dab.astype(np.float64) - Dba.T)
    print("emd_slots_n64: max |D(a, b) - D(b, a)^T| / S = %.3e" % (diff / scales(a, b).clip(min=1e-300)).max())
    assert np.all(diff <= bar)


def test_hand_made_70():
    """Equal pT sums (both slacks dead), a jet against itself, a duplicated row, coincident particles, with slots 1 and 2 live."""
    a, b, D, nodes = slots_golden("emd_hand70")
    assert np.all(nodes == 142) and a[0, :, 2].sum(dtype=np.float32) == a[1, :, 2].sum(dtype=np.float32)
    got, status = device_emd(a, b)
    check_against_lp("emd_hand70", got, status, a, b, D)
    assert np.array_equal(got[2], got[3]) and np.array_equal(got[:, 2], got[:, 3])
    bar = bars(a, b)
    assert 0 <= got[2, 2] <= bar[2, 2] and 0 <= got[2, 3] <= bar[2, 3]
    got04, status04 = device_emd(a, b, R=0.4)
    check_against_lp("emd_hand70", got04, status04, a, b, slots_golden("emd_hand70", 0.4)[2], 0.4)


@pytest.mark.parametrize("name", ["emd_n30_gluon", "emd_slots_n70"])
def test_a_failed_pair_stays_alone(name):
    """One jet of a with NaN eta: its row reports what the host build reports, every other pair -- its neighbours in the
    workgroup (4 waves at N = 30, 2 at N = 70) among them -- keeps its bits."""
    a, b = golden(name)[:2]
    a, b = a[:5], b[:5]
    N = a.shape[1]
    assert launch_shape(N)[1] == (4 if N == 30 else 2)
    good, status = device_emd(a, b)
    assert np.all(status == 0)
    bad = a.copy()
    bad[2, :, 0] = np.nan
    got, status = device_emd(bad, b)
    ref_status = host_status(bad, b)
    assert np.array_equal(status, ref_status)
    assert np.any(status[2] != 0) and np.all(status[[0, 1, 3, 4]] == 0)
    assert np.array_equal(got[[0, 1, 3, 4]], good[[0, 1, 3, 4]])
    with pytest.raises(RuntimeError, match="status"):
        ev.emds(torch.from_numpy(bad).cuda(), torch.from_numpy(b).cuda())
