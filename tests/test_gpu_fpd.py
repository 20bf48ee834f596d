"""GPU: mpg_jet_efps_d4 (csrc/jet_efp.hip) against the fp64 host statement of the same closed forms (which
tests/test_fpd_cpu.py pins to the definitions), its determinism and argument checks, and FPD / KPD on device features
against the host path."""
import numpy as np
import pytest
import torch

from mpgan_amd import data, evaluation as ev

pytestmark = pytest.mark.gpu

LAWS = ("gluon", "uniform", "top", "quark")
D4 = [("d<=", 4)]


def scattered_jets(B, N, law, seed):
    """Un-normalised [B, N, 3] synthetic jets with their zero-pT padding moved to random slots of each jet."""
    x, _ = data.synthetic_jets(B, N, seed=seed, dist=law)
    jets = data.unnormalise_jets(x, "g")
    g = torch.Generator().manual_seed(seed)
    perm = torch.rand(B, N, generator=g).argsort(1)
    return torch.gather(jets, 1, perm[:, :, None].expand(B, N, 3)).contiguous()


def check_primes(got, ref):
    """2e-5 relative per element (every summand is non-negative: the bar of the five EFPs of mpg_jet_obs carries over), which
    also demands exact zeros where the host path has zeros."""
    got, ref = got.double().cpu(), ref.double()
    assert got.shape == ref.shape == (ref.shape[0], 21)
    assert torch.isfinite(got).all()
    err = (got - ref).abs()
    assert torch.all(err <= 2e-5 * ref.abs()), float((err / ref.abs().clamp_min(1e-300)).max())


@pytest.mark.parametrize("B", [1, 7, 4096])
@pytest.mark.parametrize("N", [1, 2, 30, 31, 32, 33, 64, 150, 160])
def test_kernel_matches_fp64(N, B):
    law = LAWS[(N + B) % 4]
    jets = scattered_jets(B, N, law, seed=N * 10 + B)
    for normed in (True, False):
        ref = ev._efp_primes_cpu(jets, normed)
        if N == 1:
            assert torch.all(ref[:, 1:] == 0)
        if N <= 2:
            assert torch.all(ref[:, [6, 12, 16]] == 0)          # no triangle on two particles
        for ld_part in (3, 4):
            x = jets if ld_part == 3 else torch.cat([jets, (jets[..., 2:] != 0).float()], 2)
            check_primes(ev._efp_primes_cuda(x.cuda(), normed), ref)


def test_public_efps_on_the_device():
    jets = scattered_jets(64, 30, "gluon", seed=3)
    got = ev.efps(jets.cuda(), efpset_args=D4)
    ref = ev.efps(jets, efpset_args=D4)
    assert got.is_cuda and got.dtype == torch.float64 and got.shape == (64, 36)
    # composites multiply up to four fp32 primes: 4 x 2e-5
    assert torch.all((got.cpu() - ref).abs() <= 8e-5 * ref.abs())
    # the five shared columns are the kernel of the five-EFP set to fp32 rounding of either
    five = ev.efps(jets.cuda()).double()
    assert torch.all((got[:, 13:18] - five).abs() <= 4e-5 * five.abs())
    # the default set still runs mpg_jet_obs: the same bits as the direct call
    assert torch.equal(ev.efps(jets.cuda()), ev._obs_cuda(jets.cuda(), True, True)[1])


def test_two_launches_are_bit_identical():
    jets = scattered_jets(512, 150, "gluon", seed=5).cuda()
    a = ev._efp_primes_cuda(jets, True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        b = ev._efp_primes_cuda(jets, True)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    small = jets[:64, :30].contiguous()
    a = ev._efp_primes_cuda(small, True)
    with torch.cuda.stream(s):
        b = ev._efp_primes_cuda(small, True)
    torch.cuda.synchronize()
    assert torch.equal(a, b)


def test_argument_errors():
    from mpgan_amd import _lib
    x = torch.zeros(2, 161, 3, device="cuda")
    out = torch.empty(2, 21, device="cuda")
    lib = _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    assert lib.mpg_jet_efps_d4(x.data_ptr(), x.stride(0), 3, 2, 0, 2, out.data_ptr(), s) != 0
    assert lib.mpg_jet_efps_d4(x.data_ptr(), x.stride(0), 3, 2, 161, 2, out.data_ptr(), s) != 0
    assert lib.mpg_jet_efps_d4(x.data_ptr(), x.stride(0), 3, 2, 150, 2, None, s) != 0
    assert lib.mpg_jet_efps_d4(x.data_ptr(), x.stride(0), 3, 2, 150, 1, out.data_ptr(), s) != 0    # mpg_jet_obs's EFP bit
    assert lib.mpg_jet_efps_d4(x.data_ptr(), x.stride(0), 3, 2, 150, 6, out.data_ptr(), s) != 0
    assert lib.mpg_jet_efps_d4(x.data_ptr(), x.stride(0), 3, 2, 150, 2, out.data_ptr(), s) == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        ev.efps(x, efpset_args=D4)


# |gpu - cpu| / |cpu| of the two metrics on the fixed input below, measured on an MI355X (gfx950, ROCm 7): the fp32 kernel's
# features against the fp64 host path's, same draws.  The kernel is deterministic, so the asserted 4x only has to cover
# other builds of the host's eigen-solver and libm.
# Measured: fpd cpu 1.9080687912e-03 +- 7.39e-04, gpu 1.9080691338e-03: gap 1.80e-07;
#           kpd cpu -4.0863192893e-05 +- 2.98e-05, gpu -4.0863180371e-05: gap 3.06e-07 (the two laws are close: the unbiased MMD
#           estimate is below its own spread, and negative).
FPD_GAP_MEASURED = 1.80e-7
KPD_GAP_MEASURED = 3.06e-7


def test_fpd_and_kpd_on_device_features_against_the_host_path():
    real, gen = scattered_jets(4000, 30, "gluon", seed=1), scattered_jets(4000, 30, "quark", seed=2)
    fargs = dict(min_samples=1000, max_samples=4000, num_batches=5, num_points=5)
    kargs = dict(num_batches=6, batch_size=1000)
    re_c, ge_c = ev.efps(real, efpset_args=D4), ev.efps(gen, efpset_args=D4)
    re_g, ge_g = ev.efps(real.cuda(), efpset_args=D4), ev.efps(gen.cuda(), efpset_args=D4)
    assert re_g.is_cuda and ge_g.is_cuda
    f_c, f_g = ev.fpd(re_c, ge_c, rng=np.random.RandomState(3), **fargs), ev.fpd(re_g, ge_g, rng=np.random.RandomState(3), **fargs)
    k_c, k_g = ev.kpd(re_c, ge_c, rng=np.random.RandomState(4), **kargs), ev.kpd(re_g, ge_g, rng=np.random.RandomState(4), **kargs)
    fgap, kgap = abs(f_g[0] - f_c[0]) / abs(f_c[0]), abs(k_g[0] - k_c[0]) / abs(k_c[0])
    print("fpd cpu", f_c, "gpu", f_g, "gap", fgap)
    print("kpd cpu", k_c, "gpu", k_g, "gap", kgap)
    assert f_c[1] > 0 and k_c[1] > 0
    # (a) rounding of the fp32 features sits below the metric's own reported uncertainty
    assert abs(f_g[0] - f_c[0]) <= f_c[1]
    assert abs(k_g[0] - k_c[0]) <= k_c[1]
    # (b) 4x the measured gap
    assert fgap <= 4 * FPD_GAP_MEASURED
    assert kgap <= 4 * KPD_GAP_MEASURED


def test_evaluate_generator_with_fpd_and_kpd():
    from mpgan_amd import train
    torch.manual_seed(0)
    G, _ = train.default_mpgan(num_particles=30)
    real = scattered_jets(4096, 30, "gluon", seed=4).cuda()
    keys = ("w1m", "fpd", "kpd")
    kw = dict(num_samples=4096, keys=keys, num_w1_eval_samples=1024,
              fpd_args=dict(min_samples=500, max_samples=2000, num_batches=3, num_points=4),
              kpd_args=dict(num_batches=4, batch_size=500))
    torch.manual_seed(1)
    a = ev.evaluate_generator(G, real, "g", rng=np.random.RandomState(0), **kw)
    assert [np.shape(a[k][0]) for k in keys] == [(2,), (2,), (2,)]
    assert all(np.all(np.isfinite(a[k][0])) for k in keys)
    torch.manual_seed(1)
    b = ev.evaluate_generator(G, real, "g", rng=np.random.RandomState(0), real_efps=ev.efps(real, efpset_args=D4), **kw)
    for k in keys:
        assert np.array_equal(a[k][0], b[k][0]), k
