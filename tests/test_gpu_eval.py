"""GPU: the evaluation metrics' kernel (mpg_jet_obs, csrc/jet_obs.hip) against the fp64 CPU statement of the same
formulas (mpgan_amd/evaluation.py), its determinism and argument checks, and the metrics end to end on the device."""
import numpy as np
import pytest
import torch

from conftest import rel_err
from mpgan_amd import data, evaluation as ev

pytestmark = pytest.mark.gpu

LAWS = ("gluon", "uniform", "top", "quark")


def scattered_jets(B, N, law, seed):
    """Un-normalised [B, N, 3] synthetic jets with their zero-pT padding moved to random slots of each jet."""
    x, _ = data.synthetic_jets(B, N, seed=seed, dist=law)
    jets = data.unnormalise_jets(x, "g")
    g = torch.Generator().manual_seed(seed)
    perm = torch.rand(B, N, generator=g).argsort(1)
    return torch.gather(jets, 1, perm[:, :, None].expand(B, N, 3)).contiguous()


def check_efps(got, ref):
    got, ref = got.double().cpu(), ref.double()
    assert torch.isfinite(got).all()
    err = (got - ref).abs()
    assert torch.all(err <= 2e-5 * ref.abs()), float((err / ref.abs().clamp_min(1e-300)).max())


def check_kin(got, ref):
    for c in range(4):
        assert rel_err(got[:, c].cpu(), ref[:, c]) <= 1e-5, (c, rel_err(got[:, c].cpu(), ref[:, c]))


@pytest.mark.parametrize("B", [1, 7, 4096])
@pytest.mark.parametrize("N", [1, 2, 30, 31, 32, 33, 64, 150, 160])
def test_kernel_matches_fp64(N, B):
    law = LAWS[(N + B) % 4]
    jets = scattered_jets(B, N, law, seed=N * 10 + B)
    ref_kin, ref_efp = ev._obs_cpu(jets, True, True)
    for ld_part in (3, 4):
        x = jets if ld_part == 3 else torch.cat([jets, (jets[..., 2:] != 0).float()], 2)
        xd = x.cuda()
        kin, efp = ev._obs_cuda(xd, True, True)
        check_efps(efp, ref_efp)
        check_kin(kin, ref_kin)
        # kinematics alone: same values without the EFP pass
        kin_only, none = ev._obs_cuda(xd, False, True)
        assert none is None
        check_kin(kin_only, ref_kin)


def test_unnormalised_efps():
    jets = scattered_jets(7, 30, "gluon", seed=3)
    _, ref = ev._obs_cpu(jets, True, False)
    check_efps(ev.efps(jets.cuda(), normed=False), ref)


def test_two_launches_are_bit_identical():
    jets = scattered_jets(512, 150, "gluon", seed=5).cuda()
    a = ev._obs_cuda(jets, True, True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        b = ev._obs_cuda(jets, True, True)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    small = jets[:64, :30].contiguous()
    assert torch.equal(ev._obs_cuda(small, True, True)[1], ev._obs_cuda(small, True, True)[1])


def test_argument_errors():
    from mpgan_amd import _lib
    x = torch.zeros(2, 161, 3, device="cuda")
    kin = torch.empty(2, 4, device="cuda")
    efp = torch.empty(2, 5, device="cuda")
    lib = _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    assert lib.mpg_jet_obs(x.data_ptr(), x.stride(0), 3, 2, 161, 3, kin.data_ptr(), efp.data_ptr(), s) != 0
    assert lib.mpg_jet_obs(x.data_ptr(), x.stride(0), 3, 2, 0, 3, kin.data_ptr(), efp.data_ptr(), s) != 0
    assert lib.mpg_jet_obs(x.data_ptr(), x.stride(0), 3, 2, 150, 1, kin.data_ptr(), None, s) != 0   # EFPs without efp
    with pytest.raises(ValueError):
        ev.efps(x)


def test_evaluate_on_the_device_equals_the_cpu_path():
    real = scattered_jets(2000, 30, "gluon", seed=1)
    gen = scattered_jets(2000, 30, "quark", seed=2)
    keys = ("w1p", "w1m", "w1efp")
    cpu = ev.evaluate({k: [] for k in keys}, real, gen, "g", num_w1_eval_samples=500, rng=np.random.RandomState(9))
    gpu = ev.evaluate({k: [] for k in keys}, real.cuda(), gen.cuda(), "g", num_w1_eval_samples=500,
                      rng=np.random.RandomState(9))
    # particle features: the same fp32 inputs, W1 in fp64 on either device
    np.testing.assert_allclose(gpu["w1p"][0], cpu["w1p"][0], rtol=1e-6)
    # jet observables: fp32 kernel against fp64.  W1 moves by at most the largest change of any sample (1-Lipschitz), and
    # a population std over batches by at most as much
    for key, col in (("w1m", lambda k, e: k[:, 3:4]), ("w1efp", lambda k, e: e)):
        d = 0.0
        for j in (real, gen):
            k64, e64 = ev._obs_cpu(j, True, True)
            k32, e32 = ev._obs_cuda(j.cuda(), True, True)
            assert torch.isfinite(k32).all() and torch.isfinite(e32).all()
            d = max(d, float((col(k32, e32).double().cpu() - col(k64, e64)).abs().max()))
        n = len(gpu[key][0]) // 2
        for i in range(len(gpu[key][0])):
            assert abs(gpu[key][0][i] - cpu[key][0][i]) <= 2 * d + 1e-9 * abs(cpu[key][0][i]), (key, i, d)
            if i < n:
                assert gpu[key][0][i] == pytest.approx(cpu[key][0][i], rel=1e-3)
    # W1 of a sample against itself is exactly zero on the device
    m = ev.jet_features(real.cuda())["mass"]
    assert float(ev.wasserstein_1d(m, m)) == 0.0


def test_evaluate_generator_default_mpgan():
    from mpgan_amd import train
    torch.manual_seed(0)
    G, _ = train.default_mpgan(num_particles=30)
    real = scattered_jets(4096, 30, "gluon", seed=4).cuda()
    keys = ("w1p", "w1m", "w1efp")
    losses = ev.evaluate_generator(G, real, "g", num_samples=4096, keys=keys, num_w1_eval_samples=1024,
                                   rng=np.random.RandomState(0))
    assert [np.shape(losses[k][0]) for k in keys] == [(6,), (2,), (10,)]
    assert all(np.all(np.isfinite(losses[k][0])) for k in keys)
