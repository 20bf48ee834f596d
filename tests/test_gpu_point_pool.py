"""GPU: the layer-and-pool launches (mpg_point_pool_fwd / _bwd, ``ops.PointPoolFn``) against the fp64 restatement of
tests/baselines_ref.py, the baseline networks of ``mpgan_amd.ext_models`` against the reference's own results
(tests/golden/baselines.npz), and ``TrainStep`` with a PointNet-Mix discriminator behind the default MP generator.

Bars: TIGHT = 1e-4 on forward values, TOL = 1e-3 on gradients (BASELINE.json's), metric ``conftest.rel_err``.  The two decisions of
the op -- the argmax row and the sign of a pre-activation -- are compared with fp64's only where fp64 itself is decided by more
than the forward bar: a top-two gap above 2 TIGHT max|y|, |z| >= TIGHT max|z|.  The share of entries those conditions leave out is
computed from fp64 alone and must stay below 1 % (about 0.03 % for the Gaussian inputs used)."""
import copy
import types

import numpy as np
import pytest
import torch

import baselines_ref as R
from conftest import assert_grads, load_golden, rel_err

pytestmark = pytest.mark.gpu

TIGHT, TOL = 1e-4, 1e-3
POISON = 0x5A5A5A5A


def make(B, N, K, C, seed, scale=1.0, ldx=None):
    """x [B N, K] (rows of stride ``ldx``), W [C, K] ~ scale N(0, 1) / sqrt(K), bias ~ scale 0.5 N(0, 1): fp64 on the CPU."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B * N, K, generator=g, dtype=torch.float64) * scale
    W = torch.randn(C, K, generator=g, dtype=torch.float64) * scale / K ** 0.5
    b = torch.randn(C, generator=g, dtype=torch.float64) * 0.5 * scale
    return x, W, b


def to_dev(x, ldx=None):
    """fp32 on the GPU; ``ldx``: as the leading columns of a wider, poisoned array."""
    if ldx is None:
        return x.float().cuda()
    wide = torch.full((x.shape[0], ldx), float("nan"), device="cuda")
    wide[:, :x.shape[1]] = x.float().cuda()
    return wide[:, :x.shape[1]]


def launch(x, W, b, B, N, act, alpha, mode, ldx=None, grad=True):
    from mpgan_amd import ops
    C = W.shape[0]
    am = torch.full((B, C), -7, dtype=torch.int32, device="cuda") if grad else None
    ng = torch.full((B * N, (C + 31) // 32), POISON, dtype=torch.int32, device="cuda") if grad else None
    pooled = ops.point_pool_launch(to_dev(x, ldx), W.float().cuda(), b.float().cuda(), B, N, act=act, alpha=alpha, mode=mode,
                                   argmax=am, neg=ng)
    torch.cuda.synchronize()
    return pooled, am, ng


#        B,   N,   K,    C, mode, act, ldx
FWD = [(3,   1,  20,   40, 3, 1, None),
       (3,  30,  20,   40, 3, 1, None),
       (3,  32,  20,   40, 1, 1, None),
       (3,  33,  20,   40, 2, 1, None),
       (3, 150,  20,   40, 3, 0, None),
       (3, 160,  20,   40, 3, 1, 21),
       (1,  30,   3,   40, 3, 1, 4),
       (3,  30, 128,   40, 1, 1, 136),
       (1,  33, 256,   40, 3, 1, None),
       (3,  30,  20,    1, 3, 1, None),
       (1,  30, 128, 1024, 3, 1, None),
       (1, 160, 256, 1024, 3, 0, None),
       (300, 30, 20,   40, 3, 1, None)]


@pytest.mark.parametrize("B, N, K, C, mode, act, ldx", FWD)
def test_forward_vs_fp64(B, N, K, C, mode, act, ldx):
    alpha = 0.2
    x, W, b = make(B, N, K, C, seed=1000 * N + K + C + mode)
    ref, pr = R.layer_pool(x, W, b, B, N, act=bool(act), alpha=alpha, mode=mode)
    pooled, am, ng = launch(x, W, b, B, N, bool(act), alpha, mode, ldx)
    err = rel_err(pooled.cpu(), ref)
    z, y = pr["z"], pr["y"]
    # what fp64 decides by less than the forward bar is left out -- and that must be a small share
    gap_ok = R.top_two_gap(y) > 2 * TIGHT * float(y.abs().max())
    z_ok = z.abs() >= TIGHT * float(z.abs().max())
    out_gap, out_z = 1 - float(gap_ok.double().mean()), 1 - float(z_ok.double().mean())
    print(f"pooled err {err:.3g}; left out: gaps {out_gap:.3g}, signs {out_z:.3g}")
    assert err <= TIGHT
    assert out_gap <= 0.01 and out_z <= 0.01
    bits = R.unpack_bits(ng, C)
    assert torch.equal(bits[z_ok], pr["neg"][z_ok])
    words = ng.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    if C % 32:
        assert not (words[:, -1] >> (C % 32)).any()         # bits of columns >= C are clear
    if mode & 1:
        got = am.cpu().long()
        assert bool(((got >= 0) & (got < N)).all())
        at = torch.gather(y, 1, got.unsqueeze(1)).squeeze(1)
        assert float((y.max(1)[0] - at).max()) <= TIGHT * float(y.abs().max())
        assert torch.equal(got[gap_ok], pr["argmax"][gap_ok])
    else:
        assert bool((am == -7).all())                        # mean only: no argmax is written


@pytest.mark.parametrize("N", [30, 33])
def test_pad_rows_take_no_part(N):
    """x >= 0.5, W <= -0.5 and bias 4 on every other channel: a pad row of the last 32-row tile (z = bias = 4) would win the max
    and lift the mean."""
    B, K, C, alpha = 2, 20, 40, 0.2
    g = torch.Generator().manual_seed(N)
    x = 0.5 + torch.rand(B * N, K, generator=g, dtype=torch.float64)
    W = torch.randn(C, K, generator=g, dtype=torch.float64) / K ** 0.5
    b = torch.randn(C, generator=g, dtype=torch.float64) * 0.5
    W[::2] = -0.5 - torch.rand(C // 2, K, generator=g, dtype=torch.float64)
    b[::2] = 4.0
    ref, pr = R.layer_pool(x, W, b, B, N, act=True, alpha=alpha, mode=3)
    assert float(ref[:, :C][:, ::2].max()) < 0          # the real rows are all negative there
    pooled, am, _ = launch(x, W, b, B, N, True, alpha, 3)
    assert rel_err(pooled.cpu()[:, :C], ref[:, :C]) <= TIGHT and rel_err(pooled.cpu()[:, C:], ref[:, C:]) <= TIGHT
    got = am.cpu().long()
    assert bool((got < N).all())
    gap_ok = R.top_two_gap(pr["y"]) > 2 * TIGHT * float(pr["y"].abs().max())
    assert torch.equal(got[gap_ok], pr["argmax"][gap_ok])
    assert bool(gap_ok[:, ::2].any()) and bool(gap_ok[:, 1::2].any())     # (both kinds of channel take part in that)


def test_ties_go_to_the_lowest_row():
    B, N, K, C, alpha = 2, 30, 20, 40, 0.2
    x, W, b = make(B, N, K, C, seed=5)
    x3 = x.reshape(B, N, K)
    x3[:, 3] *= 3.0
    x3[:, 17] = x3[:, 3]
    _, pr = R.layer_pool(x, W, b, B, N, act=True, alpha=alpha, mode=1)
    others = torch.cat([pr["y"][:, :17], pr["y"][:, 18:]], 1)
    wins = (R.first_argmax(others) == 3) & (R.top_two_gap(others) > 2 * TIGHT * float(pr["y"].abs().max()))
    assert int(wins.sum()) >= 10
    _, am, _ = launch(x, W, b, B, N, True, alpha, 1)
    assert bool((am.cpu()[wins] == 3).all())


def test_zero_row_takes_the_negative_slope():
    """z = 0 exactly (a zero row, zero bias): !(z > 0), so the row's gradient is alpha g / N under mode 2 (torch's convention)."""
    from mpgan_amd import ops
    B, N, K, C, alpha = 2, 30, 20, 40, 0.25
    x, W, b = make(B, N, K, C, seed=6)
    x.reshape(B, N, K)[:, 5] = 0
    b.zero_()
    _, am, ng = launch(x, W, b, B, N, True, alpha, 2)
    assert bool(R.unpack_bits(ng, C).reshape(B, N, C)[:, 5].all())
    g = torch.randn(B, C, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    dz = ops.point_pool_bwd_launch(g.float().cuda(), None, ng, B, N, C, act=True, alpha=alpha, mode=2).cpu().reshape(B, N, C)
    assert rel_err(dz[:, 5], alpha * g.float().double() / N) <= 1e-6


@pytest.mark.parametrize("B, N, K, C, mode, act", [(3, 30, 20, 40, 3, 1), (2, 33, 128, 40, 1, 1), (2, 150, 20, 70, 2, 0),
                                                   (2, 30, 20, 70, 3, 1)])
def test_backward_launch_vs_formula(B, N, K, C, mode, act):
    """dz on the argmax rows and sign words THE FORWARD PRODUCED: at most three fp32 roundings away from the fp64 formula."""
    from mpgan_amd import ops
    alpha = 0.2
    x, W, b = make(B, N, K, C, seed=B + N + C)
    _, am, ng = launch(x, W, b, B, N, bool(act), alpha, mode)
    width = C * (2 if mode == 3 else 1)
    g = torch.randn(B, width, generator=torch.Generator().manual_seed(2)).cuda()
    dz = ops.point_pool_bwd_launch(g, am if mode & 1 else None, ng if act else None, B, N, C, act=bool(act), alpha=alpha, mode=mode)
    ref = R.pool_bwd(g.cpu().double(), am.cpu(), R.unpack_bits(ng, C), B, N, C, act=bool(act), alpha=alpha, mode=mode)
    assert dz.shape == (B * N, C) and rel_err(dz.cpu(), ref) <= 1e-6


def _decided_seed(B, N, K, C, mode):
    """The first seed of range(40) whose fp64 min|z| and smallest top-two gap are both >= 1e-3 at inputs and weights of scale 8."""
    for seed in range(40):
        x, W, b = make(B, N, K, C, seed=seed, scale=8.0)
        _, pr = R.layer_pool(x, W, b, B, N, act=True, alpha=0.2, mode=mode)
        if float(pr["z"].abs().min()) >= 1e-3 and (not mode & 1 or float(R.top_two_gap(pr["y"]).min()) >= 1e-3):
            return seed
    raise AssertionError("no decided seed in range(40)")


@pytest.mark.parametrize("B, N, K, C, mode", [(3, 30, 20, 64, 3), (2, 33, 128, 40, 1)])
def test_point_pool_fn_gradients_vs_fp64_autograd(B, N, K, C, mode):
    from mpgan_amd import ops
    alpha = 0.2
    x, W, b = make(B, N, K, C, seed=_decided_seed(B, N, K, C, mode), scale=8.0)
    cot = torch.randn(B, C * (2 if mode == 3 else 1), generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    leaves = [t.clone().requires_grad_(True) for t in (x, W, b)]
    ref, _ = R.layer_pool(*leaves, B, N, act=True, alpha=alpha, mode=mode)
    (ref * cot).sum().backward()
    dev = [t.float().cuda().requires_grad_(True) for t in (x, W, b)]
    out = ops.point_pool(dev[0], dev[1], dev[2], B, N, act=True, alpha=alpha, mode=mode)
    (out * cot.float().cuda()).sum().backward()
    torch.cuda.synchronize()
    assert rel_err(out.detach().cpu(), ref.detach()) <= TIGHT
    for name, a, r in zip(("dx", "dW", "db"), dev, leaves):
        err = rel_err(a.grad.cpu(), r.grad)
        print(name, f"{err:.3g}")
        assert err <= TOL, (name, err)


def test_launch_shape_independence():
    """Two runs give the same bits; the jets of a B = 3 call have the bits of jets 0-2 of a B = 300 call built from them."""
    N, K, C, alpha = 30, 20, 40, 0.2
    x300, W, b = make(300, N, K, C, seed=9)
    x3 = x300[:3 * N].clone()
    a = launch(x3, W, b, 3, N, True, alpha, 3)
    a2 = launch(x3, W, b, 3, N, True, alpha, 3)
    big = launch(x300, W, b, 300, N, True, alpha, 3)
    for t, t2, tb in zip(a, a2, big):
        assert torch.equal(t, t2)
        assert torch.equal(t, tb[:t.shape[0]])


def test_no_grad_call_writes_no_by_products(monkeypatch):
    """Under ``no_grad`` the op hands the launch no argmax / sign buffer, and a launch without them leaves poisoned ones alone; a
    mean-only launch does not touch an argmax buffer it is given."""
    from mpgan_amd import ops
    B, N, K, C = 3, 30, 20, 40
    x, W, b = make(B, N, K, C, seed=4)
    am = torch.full((B, C), POISON, dtype=torch.int32, device="cuda")
    ng = torch.full((B * N, 2), POISON, dtype=torch.int32, device="cuda")
    seen = []
    real = ops.point_pool_launch
    monkeypatch.setattr(ops, "point_pool_launch", lambda *a, **k: (seen.append((k["argmax"], k["neg"])), real(*a, **k))[1])
    dev = [t.float().cuda().requires_grad_(True) for t in (x, W, b)]
    with torch.no_grad():
        p0 = ops.point_pool(*dev, B, N, act=True, alpha=0.2, mode=3)
    p1 = ops.point_pool(*dev, B, N, act=True, alpha=0.2, mode=3)
    ops.point_pool_launch(dev[0].detach(), dev[1].detach(), dev[2].detach(), B, N, act=True, alpha=0.2, mode=2, argmax=am, neg=None)
    torch.cuda.synchronize()
    assert seen[0] == (None, None) and seen[1][0] is not None and seen[1][1] is not None
    assert torch.equal(p0, p1.detach())
    assert bool((am == POISON).all()) and bool((ng == POISON).all())


def test_the_activation_is_not_materialised():
    from mpgan_amd import ops
    B, N, K, C = 64, 30, 128, 1024
    x, W, b = (t.float().cuda() for t in make(B, N, K, C, seed=8))
    with torch.no_grad():
        ops.point_pool(x, W, b, B, N, act=True, alpha=0.2, mode=3)      # (the library is loaded, the seed word exists)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = ops.point_pool(x, W, b, B, N, act=True, alpha=0.2, mode=3)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
    assert out.shape == (B, 2 * C)
    print("peak above the inputs:", peak, "bytes; the activation would be", B * N * C * 4)
    assert peak < B * N * C * 4


# ------------------------------------------------------------------------------------------------ the modules
N_HITS, FS = 30, 3
SMALL = dict(latent_dim=16, rgang_fc=[24, 32], rgand_sfc=[32, 48, 96], rgand_fc=[40, 24], pointnetd_pointfc=[32, 48, 160],
             pointnetd_fc=[64], num_hits=N_HITS, node_feat_size=FS, leaky_relu_alpha=0.2, mask=True)
RESTATED = {"rgand": lambda sd, x: R.rgand(sd, x, N_HITS, FS), "pnet": lambda sd, x: R.pointnet_mix(sd, x, N_HITS, FS, mask=True)}


@pytest.fixture(scope="module")
def golden():
    return load_golden("baselines.npz")


def _case(g, name):
    t = lambda a: torch.from_numpy(np.asarray(a))
    sd = {k[len(name) + 4:]: t(v) for k, v in g.items() if k.startswith(name + ".sd.")}
    gr = {k[len(name) + 6:]: g[k] for k in g if k.startswith(name + ".grad.")}
    return sd, t(g[name + ".x"]), t(g["cot"]), g[name + ".out"], g[name + ".dx"], gr


def _module(name, sd):
    from mpgan_amd import ext_models
    net = {"rgand": ext_models.rGAND, "pnet": ext_models.PointNetMixD}[name](types.SimpleNamespace(**copy.deepcopy(SMALL)))
    net.load_state_dict({k: v.float() for k, v in sd.items()})
    return net.cuda()


@pytest.mark.parametrize("name", ["rgand", "pnet"])
def test_modules_vs_reference_golden(golden, name, monkeypatch):
    from mpgan_amd import ops
    sd, x, cot, out, dx, gr = _case(golden, name)
    net = _module(name, sd)
    calls = []
    real = ops.point_pool
    monkeypatch.setattr(ops, "point_pool", lambda *a, **k: (calls.append(k["mode"]), real(*a, **k))[1])
    xi = x.float().cuda().requires_grad_(True)
    x0 = xi.detach().clone()
    o = net(xi)
    (o * cot.float().cuda()).sum().backward()
    torch.cuda.synchronize()
    assert calls == [1 if name == "rgand" else 3]                  # the fused launch ran, once
    assert torch.equal(xi.detach(), x0)
    assert rel_err(o.detach().cpu(), out) <= TIGHT
    # the control: the restatement in fp32 (the reference's arithmetic)
    _, cdx, cgr = R.grads(RESTATED[name], {k: v.float() for k, v in sd.items()}, x.float(), cot.float())
    got = {"dx": xi.grad.cpu().numpy(), **{k: p.grad.cpu().numpy() for k, p in net.named_parameters()}}
    ref = {"dx": dx, **gr}
    control = {"dx": cdx.numpy(), **{k: v.numpy() for k, v in cgr.items()}}
    assert_grads(got, ref, TOL, control=control, what=f"ext_models {name}")
    # the un-fused route (MPG_POINT_POOL=0): the same outputs
    monkeypatch.setitem(ops.OPTIONS, "point_pool", False)
    with torch.no_grad():
        o2 = net(x.float().cuda())
    assert calls == [1 if name == "rgand" else 3]
    assert rel_err(o2.cpu(), o.detach().cpu()) <= TIGHT


def test_published_fc_generator_on_the_gpu():
    import json
    import os
    from conftest import GOLDEN
    from mpgan_amd import ext_models, gen
    with open(os.path.join(GOLDEN, "baselines_manifest.json")) as f:
        args = json.load(f)["args"]
    G = ext_models.rGANG(types.SimpleNamespace(**args))
    G.load_state_dict({k: torch.from_numpy(v) for k, v in load_golden("published_fc_g_weights.npz").items()})
    G = G.cuda().eval()
    g = load_golden("published_fc_g.npz")
    out = gen.gen(args, G, 8, N_HITS, model="rgan", noise=torch.from_numpy(g["noise"]).cuda())
    assert out.shape == (8, N_HITS, FS) and rel_err(out.detach().cpu(), g["out"]) <= TIGHT
    assert gen.gen_multi_batch(args, G, 4, 6, N_HITS, out_device="cuda", detach=True, model="rgan").shape == (6, N_HITS, FS)


# ------------------------------------------------------------------------------------------------ TrainStep
def _step_nets(B, N):
    from oracle import train_ref as T
    from mpgan_amd import ext_models, train
    G, _ = train.default_mpgan(N, disc_dropout=0.0)
    G.load_state_dict(T.init_state_dict(T.mpgan_param_shapes(True), 41, torch.float32))
    torch.manual_seed(7)
    D = ext_models.PointNetMixD(types.SimpleNamespace(**copy.deepcopy(SMALL))).cuda()
    return G, D


def test_train_step_replay_equals_eager_and_keeps_the_batch():
    """loss "ls", MPGenerator against PointNetMixD(mask): three eager and three replayed steps leave bit-identical parameters, and
    the static real batch is what ``set_batch`` put there (the reference's forward would shift its third column per step)."""
    from mpgan_amd import train
    from oracle.train_ref import synthetic_batch
    B, N = 8, 30
    data, labels = synthetic_batch(B, N, seed=3)
    res = []
    for use_graphs in (False, True):
        G, D = _step_nets(B, N)
        ts = train.TrainStep(G, D, B, N, use_graphs=use_graphs, loss="ls")
        ts.set_batch(data.cuda(), labels.cuda())
        before = ts.data.clone()
        gen = torch.Generator(device="cuda").manual_seed(5)
        ts.fixed_noise = (torch.randn(B, N, 32, device="cuda", generator=gen) * 0.2,
                          torch.randn(B, N, 32, device="cuda", generator=gen) * 0.2)
        if use_graphs:
            ts.capture(warmup=0)
        for _ in range(3):
            ts.step()
        torch.cuda.synchronize()
        assert torch.equal(ts.data, before)
        res.append((ts.fD.flat.clone(), ts.fG.flat.clone(), float(ts.D_loss), float(ts.G_loss)))
    assert bool(torch.isfinite(res[0][0]).all()) and bool(torch.isfinite(res[0][1]).all())
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert res[0][2:] == res[1][2:]


def test_train_step_gradient_penalty_vs_fp64():
    """loss "w", gp 10 (what the published baselines were trained with): the penalty of one D step against the fp64 restatement on
    the same real batch, generated batch and interpolation weights."""
    from mpgan_amd import train
    from oracle.train_ref import synthetic_batch
    B, N = 8, 30
    data, labels = synthetic_batch(B, N, seed=3)
    G, D = _step_nets(B, N)
    ts = train.TrainStep(G, D, B, N, use_graphs=False, loss="w", gp_lambda=10.0, lr_disc=0.0)
    ts.set_batch(data.cuda(), labels.cuda())
    gen = torch.Generator(device="cuda").manual_seed(5)
    nD = torch.randn(B, N, 32, device="cuda", generator=gen) * 0.2
    ts.fixed_noise = (nD, nD)
    ts.fixed_alpha = torch.rand(B, 1, 1, device="cuda", generator=gen)
    with torch.no_grad():
        fake = G(nD, ts.labels)
    ts._seg_D()
    torch.cuda.synchronize()
    sd = {k: v.detach().cpu().double() for k, v in D.state_dict().items()}
    ref = R.gradient_penalty(lambda x: R.pointnet_mix(sd, x, N, FS, mask=True), ts.data.cpu().double(), fake.cpu().double(),
                             ts.fixed_alpha.cpu().double(), 10.0)
    ref = ref.detach()
    print("GP", float(ts.GP), "fp64", float(ref))
    assert float(ref) > 0 and abs(float(ts.GP) - float(ref)) <= TOL * abs(float(ref))
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in D.parameters())
