"""GPU: device-side jet augmentation (csrc/augment.hip, ops.augment / ops.AugmentFn) and its place in ``train.TrainStep``.

The kernel draws ONE affine map of (eta, phi) per jet from the device seed and applies it; the tests check the application
against the torch statement of the same map (``ops.augment_apply_reference``), the structure and the distributions of the
maps, the streams, the backward, and the training step's semantics (train.py:438-442, :508-511).

Statistical bounds are 5 sigma of the sampling error of B_STAT jets, computed here from B_STAT; the seed is fixed
(``ops.set_seed``), so every run sees the same draws."""
import itertools
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ALL = 15                      # MPG_AUG_R90 | _FLIP | _TRANSLATE | _SCALE
R90, FLIP, TRANSLATE, SCALE = 1, 2, 4, 8
RATIO, SD = 0.5, 0.25
B_STAT = 16384
EPS = 2.0 ** -23
P_ALL = float(torch.nextafter(torch.tensor(1.0), torch.tensor(0.0)))   # every jet takes the stage (p == 1 itself: none does)
IDENT = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)


def _p(v):
    return torch.full((1,), float(v), device="cuda")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _apply_bound(x, params):
    """2 * 2^-23 * (|a00 x0| + |a01 x1| + |t0|) and the same for phi, in fp64: the kernel's FMAs and the torch statement differ
    only in whether a product is rounded before the addition."""
    q = params.double()
    x0, x1 = x[..., 0].double().abs(), x[..., 1].double().abs()
    c = lambda k: q[:, k].abs().reshape(-1, 1)
    return torch.stack((c(0) * x0 + c(1) * x1 + c(4), c(2) * x0 + c(3) * x1 + c(5)), dim=2) * 2 * EPS


def _check_apply(x, y, params, what):
    from mpgan_amd import ops
    ref = ops.augment_apply_reference(x, params)
    err = (y[..., :2].double() - ref[..., :2].double()).abs()
    bound = _apply_bound(x, params)
    worst = float((err - bound).max())
    print(f"{what}: max err {float(err.max()):.3e}, max bound {float(bound.max()):.3e}, worst err - bound {worst:.3e}")
    assert bool((err <= bound).all()), what
    assert torch.equal(_bits(y[..., 2:]), _bits(x[..., 2:])), what     # columns >= 2: bit-identical


def _jets(B, N, F, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(B, N, F, device="cuda", generator=g)


# ---- 1. apply -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 30, 63, 64, 65, 160])
@pytest.mark.parametrize("B", [1, 7])
@pytest.mark.parametrize("ld", [3, 4])
def test_apply_matches_the_torch_statement(N, B, ld):
    from mpgan_amd import ops
    ops.set_seed(0x5EED0001 + 131 * N + 7 * B + ld)
    x = _jets(B, N, ld, seed=N + B)
    p = _p(0.5)
    # out of place, rows of ld floats with F = ld features
    y, prm = ops.augment(x, p, ALL, RATIO, SD, site=0)
    assert y.data_ptr() != x.data_ptr() and prm.shape == (B, 6)
    _check_apply(x, y, prm, "out of place")
    # in place: same maps (same seed, same site), same values
    z = x.clone()
    y2, prm2 = ops.augment(z, p, ALL, RATIO, SD, site=0, out=z)
    assert y2 is z and torch.equal(_bits(prm2), _bits(prm)) and torch.equal(_bits(z), _bits(y))
    # a non-contiguous jet stride: the second half of a 2B-jet buffer as the target, in place; the first half stays
    buf = torch.cat((_jets(B, N, ld, seed=99), x), 0)
    keep = buf.clone()
    ops.augment(buf[B:], p, ALL, RATIO, SD, site=0, out=buf[B:])
    assert torch.equal(_bits(buf[B:]), _bits(y)) and torch.equal(_bits(buf[:B]), _bits(keep[:B]))
    if ld == 4:
        # F = 3 features in rows of 4 floats (a mask column the call does not own): in place and into another such view
        wide, other = x.clone(), torch.full_like(x, 7.0)
        ops.augment(wide[..., :3], p, ALL, RATIO, SD, site=0, out=wide[..., :3])
        ops.augment(x[..., :3], p, ALL, RATIO, SD, site=0, out=other[..., :3])
        for t in (wide, other):
            assert torch.equal(_bits(t[..., :3]), _bits(y[..., :3]))
        assert torch.equal(_bits(wide[..., 3]), _bits(x[..., 3])) and bool((other[..., 3] == 7.0).all())
    # every flag off: the identity map, exactly, and the values bit for bit
    y0, prm0 = ops.augment(x, p, 0, RATIO, SD, site=0)
    assert torch.equal(prm0, torch.tensor(IDENT, device="cuda").expand(B, 6)) and torch.equal(_bits(y0), _bits(x))


# ---- 2. / 3. the maps ---------------------------------------------------------------------------------------------------
def _maps(flags, p, site=0, seed=0xA06A06):
    from mpgan_amd import ops
    ops.set_seed(seed)
    x = _jets(B_STAT, 2, 3, seed=1)
    _, prm = ops.augment(x, _p(p), flags, RATIO, SD, site=site)
    also = ops.augment_params(B_STAT, _p(p), flags, RATIO, SD, site)     # the maps alone: the same maps
    assert torch.equal(_bits(also), _bits(prm))
    return prm.cpu()


def test_structure_of_every_map():
    q = _maps(ALL, 0.5)
    a00, a01, a10, a11, t0, t1 = (q[:, k] for k in range(6))
    diag = (a01 == 0) & (a10 == 0) & (a00.abs() == a11.abs()) & (a00 != 0)
    anti = (a00 == 0) & (a11 == 0) & (a01.abs() == a10.abs()) & (a01 != 0)
    assert bool((diag | anti).all())
    assert bool(anti.any()) and bool((t0 != 0).any()) and bool((a00.abs() + a01.abs() != 1).any())   # (every stage is at work)
    q = _maps(ALL & ~SCALE, 0.5)
    assert bool(((q[:, :4].abs() == 1) | (q[:, :4] == 0)).all()) and bool((q[:, :4].abs().sum(1) == 2).all())
    q = _maps(ALL & ~TRANSLATE, 0.5)
    assert bool((q[:, 4:] == 0).all())


def _is_ident(q):
    return (q == torch.tensor(IDENT)).all(1)


def _within(value, mean, sigma, what):
    print(f"{what}: {value:.6g}, expected {mean:.6g} +- 5 x {sigma:.3g}")
    assert abs(value - mean) <= 5 * sigma, what


@pytest.mark.parametrize("p", [0.25, 0.5])
def test_take_frequency_of_each_stage(p):
    """Each flag alone.  A taken translation or scaling is visible in the map; a taken rotation with k = 0 or a flip with both
    signs +1 is not, so for those two the frequency is counted among the jets whose transformation -- known from the run in
    which every jet takes the stage -- is not the identity (n of them: the bound uses n)."""
    for flag, name in ((R90, "r90"), (FLIP, "flip"), (TRANSLATE, "translate"), (SCALE, "scale")):
        visible = ~_is_ident(_maps(flag, P_ALL))
        n = int(visible.sum())
        assert n > (0.7 if flag in (R90, FLIP) else 0.999) * B_STAT, (name, n)
        taken = ~_is_ident(_maps(flag, p))
        assert not bool((taken & ~visible).any())
        _within(float(taken[visible].float().mean()), p, math.sqrt(p * (1 - p) / n), f"take frequency of {name} at p = {p}")


def test_distribution_of_every_transformation():
    B = B_STAT
    # rotations: every jet takes one; the four multiples of 90 degrees a quarter each
    q = _maps(R90, P_ALL)
    rot = {0: (1, 0, 0, 1), 1: (0, -1, 1, 0), 2: (-1, 0, 0, -1), 3: (0, 1, -1, 0)}
    counts = {k: int((q[:, :4] == torch.tensor(v, dtype=torch.float32)).all(1).sum()) for k, v in rot.items()}
    assert sum(counts.values()) == B and bool((q[:, 4:] == 0).all())
    for k, c in counts.items():
        _within(c / B, 0.25, math.sqrt(0.25 * 0.75 / B), f"rotation by {k} x 90 degrees")
    # flips: both signs fair and independent
    q = _maps(FLIP, P_ALL)
    assert bool((q[:, (0, 3)].abs() == 1).all()) and bool((q[:, (1, 2, 4, 5)] == 0).all())
    sx, sy = q[:, 0].double(), q[:, 3].double()
    _within(float((sx > 0).double().mean()), 0.5, math.sqrt(0.25 / B), "flip: eta sign +1")
    _within(float((sy > 0).double().mean()), 0.5, math.sqrt(0.25 / B), "flip: phi sign +1")
    _within(float((sx * sy).mean()), 0.0, 1 / math.sqrt(B), "flip: correlation of the two signs")
    # translations: uniform in +- ratio / 2
    q = _maps(TRANSLATE, P_ALL)
    assert torch.equal(q[:, :4], torch.tensor(IDENT[:4]).expand(B, 4)) and bool((q[:, 4:].abs() <= RATIO / 2).all())
    for k, name in ((4, "eta"), (5, "phi")):
        t = q[:, k].double()
        _within(float(t.mean()), 0.0, RATIO / math.sqrt(12 * B), f"translation {name}: mean")
        # (variance of the sample variance of a uniform law of width w: (mu4 - sigma^4) / B = w^4 (1/80 - 1/144) / B = w^4 / (180 B))
        _within(float((t ** 2).mean()), RATIO ** 2 / 12, RATIO ** 2 / math.sqrt(180 * B), f"translation {name}: variance")
    _within(float((q[:, 4].double() * q[:, 5].double()).mean()), 0.0, RATIO ** 2 / 12 / math.sqrt(B), "translation: eta-phi covariance")
    # scalings: log f / scale_sd standard normal
    q = _maps(SCALE, P_ALL)
    assert bool((q[:, 0] == q[:, 3]).all()) and bool((q[:, 0] > 0).all()) and bool((q[:, (1, 2, 4, 5)] == 0).all())
    g = q[:, 0].double().log() / SD
    _within(float(g.mean()), 0.0, 1 / math.sqrt(B), "scaling: mean of log f / sd")
    _within(float((g ** 2).mean()), 1.0, math.sqrt(2.0 / B), "scaling: variance of log f / sd")


# ---- 4. p == 1 and p == 0 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1.0, 0.0])
def test_probability_one_and_zero_take_nothing(p):
    """rand_mix returns the untouched batch at p == 1 (the reference's quirk, kept), and u < 0 never holds."""
    from mpgan_amd import ops
    ops.set_seed(77)
    x = _jets(257, 30, 3, seed=2)
    y, prm = ops.augment(x, _p(p), ALL, RATIO, SD, site=1)
    assert bool(_is_ident(prm.cpu()).all()) and torch.equal(_bits(y), _bits(x))


# ---- 5. streams ---------------------------------------------------------------------------------------------------------
def test_streams():
    from mpgan_amd import ops
    x = _jets(64, 30, 3, seed=3)
    p = _p(0.5)

    def run(site):
        y, prm = ops.augment(x, p, ALL, RATIO, SD, site=site)
        return y, prm

    ops.set_seed(4242)
    y0, q0 = run(0)
    y0b, q0b = run(0)
    assert torch.equal(_bits(q0), _bits(q0b)) and torch.equal(_bits(y0), _bits(y0b))     # same (seed, tag): same bits
    q = [q0, run(1)[1], run(2)[1]]
    for i, j in itertools.combinations(range(3), 2):
        assert not torch.equal(q[i], q[j]), (i, j)                                         # the three sites: three streams
        assert float((q[i] != q[j]).any(1).float().mean()) > 0.5
    ops.bump_seed()
    assert not torch.equal(run(0)[1], q0)                                                  # the next iteration: new maps
    ops.set_seed(4242)
    assert torch.equal(_bits(run(0)[1]), _bits(q0))


# ---- 6. backward --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,F", [(7, 30, 3), (1, 65, 4), (7, 160, 4)])
def test_backward_matches_autograd_through_the_torch_statement(B, N, F):
    from mpgan_amd import ops
    ops.set_seed(0xBAC0 + N)
    x = _jets(B, N, F, seed=5).requires_grad_(True)
    w = _jets(B, N, F, seed=6)
    prm = torch.empty(B, 6, device="cuda")
    y = ops.AugmentFn.apply(x, _p(0.5), ALL, RATIO, SD, 1, prm)
    _check_apply(x.detach(), y.detach(), prm, "forward")
    (y * w).sum().backward()
    x2 = x.detach().clone().requires_grad_(True)
    (ops.augment_apply_reference(x2, prm) * w).sum().backward()
    q, g0, g1 = prm.double(), w[..., 0].double().abs(), w[..., 1].double().abs()
    c = lambda k: q[:, k].abs().reshape(-1, 1)
    bound = torch.stack((c(0) * g0 + c(2) * g1, c(1) * g0 + c(3) * g1), dim=2) * 2 * EPS     # dx = A^T dy
    err = (x.grad[..., :2].double() - x2.grad[..., :2].double()).abs()
    print(f"backward: max err {float(err.max()):.3e}, max bound {float(bound.max()):.3e}")
    assert bool((err <= bound).all())
    assert torch.equal(_bits(x.grad[..., 2:]), _bits(w[..., 2:]))


# ---- 7. TrainStep -------------------------------------------------------------------------------------------------------
B_TS, N_TS = 8, 30


class _env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def _reset_tags():
    """The dropout sites of the fused ops are numbered by a per-device counter in host order: two steps that are to draw the same
    masks start from the same count."""
    from mpgan_amd import ops
    ops.dev_state("cuda").tags = itertools.count(1)


def _aug(p, **kw):
    from mpgan_amd import train
    return train.Augment(aug_r90=True, aug_f=True, aug_t=True, aug_s=True, translate_ratio=RATIO, scale_sd=SD, aug_prob=p, **kw)


def _step(model, augment, use_graphs=False, fixed_noise=False):
    """A TrainStep over the default MPGAN / GAPT networks (dropout 0.5 in D) from fixed weights, data and device seed."""
    from mpgan_amd import ops, train
    from oracle import train_ref as T
    if model == "mpgan":
        G, D = train.default_mpgan(N_TS)
        shapes, latent, lrs = T.mpgan_param_shapes, 32, train.LR["g"]
    else:
        G, D = train.default_gapt(N_TS)
        shapes, latent, lrs = T.gapt_param_shapes, 64, train.LR_GAPT
    G.load_state_dict(T.init_state_dict(shapes(True), 41, torch.float32))
    D.load_state_dict(T.init_state_dict(shapes(False), 42, torch.float32))
    data, labels = T.synthetic_batch(B_TS, N_TS, seed=3)
    ts = train.TrainStep(G, D, B_TS, N_TS, latent=latent, lr_disc=lrs[0], lr_gen=lrs[1], use_graphs=use_graphs, augment=augment)
    ts.set_batch(data.cuda(), labels.cuda())
    if fixed_noise:
        gen = torch.Generator(device="cuda").manual_seed(5)
        ts.fixed_noise = (torch.randn(B_TS, N_TS, latent, device="cuda", generator=gen) * 0.2,
                          torch.randn(B_TS, N_TS, latent, device="cuda", generator=gen) * 0.2)
    ops.set_seed(0x7EA1)
    _reset_tags()
    return ts


def _result(ts):
    torch.cuda.synchronize()
    return ts.fD.flat.clone(), ts.fG.flat.clone(), float(ts.D_loss), float(ts.G_loss)


def _same(a, b):
    print("losses", a[2:4], b[2:4], "max |dD|", float((a[0] - b[0]).abs().max()), "max |dG|", float((a[1] - b[1]).abs().max()))
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2:4] == b[2:4]


@pytest.mark.parametrize("model", ["mpgan", "gapt"])
def test_step_with_probability_zero_is_the_step_without(model):
    """(a) the launches of the augmentation are there and apply the identity: losses and parameters bit for bit those of
    ``augment=None`` (GAPT: of the step without the one-launch bridge, which an augmenting step leaves)."""
    ts = _step(model, _aug(0.0))
    assert ts.aug is not None and not ts._bridge()
    for _ in range(2):
        ts.step()
    with_it = _result(ts)
    assert all(bool(_is_ident(q.cpu()).all()) for q in ts.aug_params[:2])
    with _env(MPG_BRIDGE="0"):
        plain = _step(model, None)
        for _ in range(2):
            plain.step()
    assert _same(with_it, _result(plain))


@pytest.mark.parametrize("model", ["mpgan", "gapt"])
def test_captured_step_equals_eager_and_follows_the_device_probability(model):
    """(b) three replays of the captured iteration against three eager iterations at aug_prob = 0.5: bit-identical, with new
    maps on every replay (the eager iterations reuse the dropout sites a graph keeps from its capture: the counter is put back
    before each).  (c) ``set_aug_prob(0.0)`` reaches the captured graph: the next replay draws identity maps only."""
    eager = _step(model, _aug(0.5))
    maps_e = []
    for _ in range(3):
        _reset_tags()
        eager.step()
        maps_e.append([q.clone() for q in eager.aug_params[:2]])
    res_e = _result(eager)
    cap = _step(model, _aug(0.5), use_graphs=True)
    cap.capture(warmup=0)
    graphs = cap._graphs
    maps_c = []
    for _ in range(3):
        cap.step()
        maps_c.append([q.clone() for q in cap.aug_params[:2]])
    assert _same(res_e, _result(cap))
    for it in range(3):
        for site in range(2):
            assert torch.equal(maps_e[it][site], maps_c[it][site]), (it, site)
            assert not bool(_is_ident(maps_c[it][site].cpu()).all())
            if it:
                assert not torch.equal(maps_c[it][site], maps_c[it - 1][site]), (it, site)
        assert not torch.equal(maps_c[it][0], maps_c[it][1])
    cap.set_aug_prob(0.0)
    cap.step()
    torch.cuda.synchronize()
    assert cap._graphs is graphs
    assert all(bool(_is_ident(q.cpu()).all()) for q in cap.aug_params[:2])


@pytest.mark.parametrize("model", ["mpgan", "gapt"])
def test_parts_route_and_generic_route_agree_under_augmentation(model):
    """(d) features and mask held apart (one in-place launch on ``_x3[B:]``) against the reference's [B, N, 4] tensors
    (MPG_PARTS=0: in place on ``_dcat[B:]``, rows of 4 floats): the bar of tests/test_gpu_train.py's
    ``test_features_and_mask_held_apart_change_no_result`` for these two routes -- bit-identical."""
    res = []
    for parts in ("1", "0"):
        with _env(MPG_PARTS=parts):
            ts = _step(model, _aug(0.5), fixed_noise=True)
            assert ts.parts == (parts == "1")
            for _ in range(2):
                ts.step()
            res.append(_result(ts) + ([q.clone() for q in ts.aug_params[:2]],))
    assert all(torch.equal(a, b) for a, b in zip(res[0][4], res[1][4]))
    assert _same(res[0], res[1])


@pytest.mark.parametrize("model", ["mpgan", "gapt"])
def test_discriminator_sees_real_jets_as_they_are_and_generated_jets_augmented(model):
    """(e) train_D: D(real) runs on the batch as it is (train.py:425 is in front of the augmentation), the generated half is
    the generator's jets under the maps of site 0."""
    from mpgan_amd import ops
    ts = _step(model, _aug(0.5), fixed_noise=True)
    data = ts.data.clone()
    ts.step()
    with torch.no_grad():     # what the second iteration's D step will generate (G moves only at the end of an iteration)
        ts.G.eval()
        generated = ts.G.generate_parts(ts.fixed_noise[0], ts.labels)[0].clone()
    ts.step()
    torch.cuda.synchronize()
    assert ts.parts and torch.equal(ts._x3[:B_TS], data[..., :3])
    q = ts.aug_params[0]
    assert not bool(_is_ident(q.cpu()).all())
    _check_apply(generated, ts._x3[B_TS:], q, "generated half of the D step's batch")


def test_gradient_penalty_receives_the_augmented_real_batch():
    """``calc_D_loss`` is handed the augmented ``data`` (train.py:441, :452): with gp_lambda > 0 the real batch goes through
    site 2 on its way into the penalty -- and nowhere else (``TrainStep.data`` stays as set)."""
    from mpgan_amd import ops, train
    from oracle import train_ref as T
    G, D = train.default_mpgan(N_TS, loss="w")
    data, labels = T.synthetic_batch(B_TS, N_TS, seed=3)
    ts = train.TrainStep(G, D, B_TS, N_TS, use_graphs=False, loss="w", gp_lambda=10.0, augment=_aug(0.5))
    ts.set_batch(data.cuda(), labels.cuda())
    ops.set_seed(0x7EA1)
    seen = []
    inner = ts.gradient_penalty
    ts.gradient_penalty = lambda real, fake: (seen.append((real.clone(), fake.clone())), inner(real, fake))[1]
    ts.step()
    torch.cuda.synchronize()
    real, fake = seen[0]
    q = ts.aug_params[2]
    assert not bool(_is_ident(q.cpu()).all()) and torch.equal(ts.data, data.cuda())
    _check_apply(ts.data, real, q, "real batch of the gradient penalty")
    assert math.isfinite(float(ts.GP)) and math.isfinite(float(ts.D_loss))
