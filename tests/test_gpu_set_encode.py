"""GPU: the set-encoder launch (mpg_set_encode_fwd, ``ops.set_encode_launch``) against the fp64 restatement of tests/pcgan_ref.py, and
``ext_models``' PCGAN nets against the reference's own results (tests/golden/pcgan*.npz, published_pcgan_g_inv_t.npz).

Bars: TIGHT = 1e-4 on forward values, TOL = 1e-3 on gradients (BASELINE.json's), metric ``conftest.rel_err``.  Every input of the
launch has x <= -1, so a zero-filled pad row would win a max and dilute a mean; each forward case first shows, in fp64 alone, that
one zero row appended to every jet moves the result by more than 100 TIGHT -- a case that does not is invalid, not passed."""
import copy

import numpy as np
import pytest
import torch

import pcgan_ref as R
from conftest import CONTROL_CEILING, assert_grads, load_golden, rel_err

pytestmark = pytest.mark.gpu

TIGHT, TOL = 1e-4, 1e-3
POISON = -77.0
PAD = 3          # NaN columns behind a row of x; poisoned columns on either side of pooled's rows


def dev(t):
    return None if t is None else t.float().cuda()


def launch(x, gammas, biases, lambdas, pool, act):
    """The launch on fp32 copies, x with ``ldx`` = K + PAD and NaN in the slack, pooled inside a poisoned array that must survive."""
    from mpgan_amd import ops
    B, N, K = x.shape
    D = gammas[-1].shape[0]
    xw = torch.full((B, N, K + PAD), float("nan"), device="cuda")
    xw[:, :, :K] = dev(x)
    wide = torch.full((B + 2, D + 2 * PAD), POISON, device="cuda")
    out = ops.set_encode_launch(xw[:, :, :K], [dev(t) for t in gammas], [dev(t) for t in biases], [dev(t) for t in lambdas],
                                pool=pool, act=act, pooled=wide[1:-1, PAD:PAD + D])
    torch.cuda.synchronize()
    mask = torch.ones_like(wide, dtype=torch.bool)
    mask[1:-1, PAD:PAD + D] = False
    assert bool((wide[mask] == POISON).all()) and out.data_ptr() == wide[1:-1, PAD:PAD + D].data_ptr()
    return out.clone()


def case(N, widths, B, pool, scale=1.0):
    """Weights and inputs of a case in fp64 with fp32 values (so the launch sees exactly what the yardstick sees)."""
    g = torch.Generator().manual_seed(1000 * N + 10 * B + pool + len(widths))
    gammas, biases, lambdas = R.random_stack(widths, pool, g, scale=scale)
    f32 = lambda ts: [None if t is None else t.float().double() for t in ts]
    return R.negative_jets(B, N, widths[0], g).float().double(), f32(gammas), f32(biases), f32(lambdas)


def pad_row_matters(x, gammas, biases, lambdas, pool, act, ref):
    """From fp64 alone: does one zero row appended to each jet move the result by more than 100 TIGHT?"""
    xz = torch.cat((x, torch.zeros(x.shape[0], 1, x.shape[2], dtype=x.dtype)), 1)
    return rel_err(R.stack(xz, gammas, biases, lambdas, pool, act), ref) > 100 * TIGHT


#         N,   widths,                   B
SHAPES = [(1,   [3, 1],                   1),     # one particle, one channel, one jet, one layer
          (2,   [4, 40, 1, 40],           3),     # a layer of one channel: K = 1 behind it
          (30,  [3, 256, 256, 256],       5),     # the published widths; four jets per workgroup, the second workgroup holds one
          (31,  [20, 40, 256, 40, 1],     3),     # four layers of unequal widths, K_0 of two k-steps
          (32,  [3, 40],                  5),     # a full row tile
          (33,  [4, 256, 40, 256],        3),     # two row tiles per jet, the second of one row; two jets per workgroup
          (64,  [3, 40, 40, 40],          3),     # two full tiles; the second workgroup holds one jet
          (65,  [20, 256],                1),     # three tiles: one jet per workgroup, the fourth wave idle
          (96,  [3, 40, 256, 40],         1),
          (127, [4, 40, 40, 40, 40],      1),     # four tiles, the last short of one row
          (128, [3, 256, 256, 256, 256],  1),     # every limit at once
          (30,  [3, 40, 40, 40],          300)]   # 75 workgroups


@pytest.mark.parametrize("act", [2, 3])
@pytest.mark.parametrize("pool", [1, 2, 3])
@pytest.mark.parametrize("N, widths, B", SHAPES)
def test_forward_vs_fp64(N, widths, B, pool, act):
    x, gammas, biases, lambdas = case(N, widths, B, pool)
    ref = R.stack(x, gammas, biases, lambdas, pool, act)
    assert float(x.max()) <= -1.0 and pad_row_matters(x, gammas, biases, lambdas, pool, act, ref), "invalid case"
    got = launch(x, gammas, biases, lambdas, pool, act)
    err = rel_err(got.cpu(), ref)
    print(f"N {N} widths {widths} B {B} pool {pool} act {act}: {err:.3g}")
    assert got.shape == ref.shape and err <= TIGHT


@pytest.mark.parametrize("pool", [1, 2, 3])
def test_softplus_takes_both_branches(pool):
    x, gammas, biases, lambdas = case(30, [3, 40, 40], 5, pool, scale=12.0)
    probe = {}
    ref = R.stack(x, gammas, biases, lambdas, pool, 3, probe=probe)
    z = torch.cat([t.reshape(-1) for t in probe["z"]])
    assert bool((z > 20).any()) and bool((z < -20).any()) and bool((z.abs() < 20).any())
    assert pad_row_matters(x, gammas, biases, lambdas, pool, 3, ref), "invalid case"
    err = rel_err(launch(x, gammas, biases, lambdas, pool, 3).cpu(), ref)
    print(f"softplus beyond 20, pool {pool}: {err:.3g}")
    assert err <= TIGHT


@pytest.mark.parametrize("N, widths, B, picks", [(30, [3, 40, 40, 40], 300, (0, 1, 2, 3, 150, 298, 299)), (64, [3, 40, 40, 40], 3, (0, 1, 2)),
                                                 (65, [20, 256], 3, (0, 2))])
@pytest.mark.parametrize("pool", [1, 3])
def test_a_jets_bits_do_not_depend_on_the_batch_or_the_run(N, widths, B, picks, pool):
    x, gammas, biases, lambdas = case(N, widths, B, pool)
    full = launch(x, gammas, biases, lambdas, pool, 2)
    assert torch.equal(full, launch(x, gammas, biases, lambdas, pool, 2))
    for b in picks:
        alone = launch(x[b:b + 1], gammas, biases, lambdas, pool, 2)
        assert torch.equal(alone[0], full[b]), b
    # ... nor on its position: the batch reversed
    assert torch.equal(launch(x.flip(0), gammas, biases, lambdas, pool, 2), full.flip(0))


def published():
    sd = {k: torch.from_numpy(v) for k, v in load_golden("published_pcgan_g_inv_t_weights.npz").items()}
    return sd, load_golden("published_pcgan_g_inv_t.npz")


def count_launches(monkeypatch):
    from mpgan_amd import ops
    calls, real = [], ops.set_encode_launch
    monkeypatch.setattr(ops, "set_encode_launch", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


def test_published_encoder_fused_and_unfused(monkeypatch):
    """The published top-quark encoder (|w| up to 6.6) on its 8 stored jets against the reference's fp64 output, on the one-launch
    route and on the un-fused route.  Measured on an MI355X: one launch 1.17e-06, un-fused 1.04e-06 -- both inside TIGHT, so the
    rule for an un-fused route that misses it (the one-launch bar becomes twice the un-fused error) does not come into play."""
    from mpgan_amd import ext_models, ops
    sd, g = published()
    enc = ext_models.load_pcgan_encoder(sd, 3, 256, 256, "max1").cuda()
    x = torch.from_numpy(g["x"]).cuda()
    calls = count_launches(monkeypatch)
    monkeypatch.setitem(ops.OPTIONS, "set_encode", True)
    fused = enc(x)                                   # a plain call, grad mode on, as train.py:839 makes it
    assert len(calls) == 1 and not fused.requires_grad
    monkeypatch.setitem(ops.OPTIONS, "set_encode", False)
    unfused = enc(x)
    assert len(calls) == 1
    e_f, e_u = rel_err(fused.cpu(), g["out"]), rel_err(unfused.cpu(), g["out"])
    print(f"published encoder: fused {e_f:.3g}, un-fused {e_u:.3g}")
    assert fused.shape == (8, 256) and e_u <= TIGHT
    assert e_f <= (TIGHT if e_u <= TIGHT else 2 * e_u)


ENCODERS = ["enc_max1", "enc_max", "enc_mean", "enc_max1_x4", "encsp_mean"]


@pytest.fixture(scope="module")
def golden():
    return {k: torch.from_numpy(np.asarray(v)) for k, v in load_golden("pcgan.npz").items()}


def small_net(name, golden):
    import json
    import os
    from conftest import GOLDEN
    from mpgan_amd import ext_models
    with open(os.path.join(GOLDEN, "pcgan_manifest.json")) as f:
        spec = json.load(f)["small"][name]
    net = getattr(ext_models, spec["class"])(*spec["args"])
    net.load_state_dict({k[len(name) + 4:]: v for k, v in golden.items() if k.startswith(name + ".sd.")}, strict=True)
    return net


@pytest.mark.parametrize("name", ENCODERS)
def test_module_routes(name, golden, monkeypatch):
    """Frozen, the encoder takes the one launch; with a parameter requiring grad it takes the un-fused route, whose input and
    parameter gradients meet the reference's."""
    from mpgan_amd import ops
    monkeypatch.setitem(ops.OPTIONS, "set_encode", True)
    calls = count_launches(monkeypatch)
    net = small_net(name, golden).cuda()
    x = golden[f"{name}.x"].cuda()
    ref_out = golden[f"{name}.out"]
    frozen = copy.deepcopy(net).requires_grad_(False)
    out = frozen(x)
    assert len(calls) == 1 and rel_err(out.cpu(), ref_out) <= TIGHT
    with torch.no_grad():
        assert torch.equal(net(x), out) and len(calls) == 2          # grad mode off: the parameters' flags do not matter
    with ops.double_backward_route("cuda"):
        assert rel_err(frozen(x).cpu(), ref_out) <= TIGHT and len(calls) == 2
    assert rel_err(frozen(x.requires_grad_(True)).detach().cpu(), ref_out) <= TIGHT and len(calls) == 2   # the input asks
    x = x.detach().requires_grad_(True)
    out = net(x)
    (out * golden[f"{name}.cot"].float().cuda()).sum().backward()
    assert len(calls) == 2 and rel_err(out.detach().cpu(), ref_out) <= TIGHT
    got = {"dx": x.grad.cpu().numpy(), **{k: p.grad.cpu().numpy() for k, p in net.named_parameters()}}
    ref = {"dx": golden[f"{name}.dx"].numpy(), **{k: golden[f"{name}.grad.{k}"].numpy() for k, _ in net.named_parameters()}}
    assert_grads(got, ref, TOL, what=f"ext_models {name} un-fused")


@pytest.mark.parametrize("name", ["dec", "latent_G", "latent_D"])
def test_row_nets_vs_reference_golden(name, golden):
    net = small_net(name, golden).cuda()
    xs = [golden[f"{name}.{t}"].cuda().requires_grad_(True) for t in ("x", "x2") if f"{name}.{t}" in golden]
    out = net(*xs)
    (out * golden[f"{name}.cot"].float().cuda()).sum().backward()
    assert rel_err(out.detach().cpu(), golden[f"{name}.out"]) <= TIGHT
    got = {k: p.grad.cpu().numpy() for k, p in net.named_parameters()}
    ref = {k: golden[f"{name}.grad.{k}"].numpy() for k in got}
    for t, x in zip(("dx", "dx2"), xs):
        got[t], ref[t] = x.grad.cpu().numpy(), golden[f"{name}.{t}"].numpy()
    control = None
    if name != "dec":      # LeakyReLU nets: the fp32 evaluation of the same module as ``assert_grads``' control
        cpu = small_net(name, golden)
        xc = golden[f"{name}.x"].clone().requires_grad_(True)
        (cpu(xc) * golden[f"{name}.cot"].float()).sum().backward()
        control = {"dx": xc.grad.numpy(), **{k: p.grad.numpy() for k, p in cpu.named_parameters()}}
    assert_grads(got, ref, TOL, control=control, what=f"ext_models {name}")


def test_captured_forward_follows_in_place_weight_updates(monkeypatch):
    """The frozen encoder captured with torch.cuda.graph replays to the eager result, and after an in-place change of a Gamma to
    the new eager result, bit for bit: the launch reads the parameters themselves."""
    from mpgan_amd import ext_models, ops
    monkeypatch.setitem(ops.OPTIONS, "set_encode", True)
    sd, g = published()
    enc = ext_models.load_pcgan_encoder(sd, 3, 256, 256, "max1").cuda()
    x = torch.from_numpy(g["x"]).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            enc.pooled(x)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    calls = count_launches(monkeypatch)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = enc.pooled(x)
    assert len(calls) == 1
    graph.replay()
    torch.cuda.synchronize()
    eager = enc.pooled(x)
    assert torch.equal(out, eager)
    with torch.no_grad():
        enc.phi[2].Gamma.weight.mul_(-0.75)
        enc.phi[4].Gamma.bias.add_(0.125)
    graph.replay()
    torch.cuda.synchronize()
    eager2 = enc.pooled(x)
    assert torch.equal(out, eager2) and not torch.equal(eager, eager2)


def latent_gan_iteration(enc, lD, lG, data, noise, alpha, route):
    """One iteration of the latent GAN as train.py runs it with loss "w" and gp 10: the frozen encoder on the real batch, the
    critic's step with the gradient penalty on ``alpha`` [B, 1] (train.py:288-323), the generator's step; Adam on both.  Returns the
    gradients the two steps saw."""
    optD = torch.optim.Adam(lD.parameters(), lr=1e-4, betas=(0.9, 0.999))
    optG = torch.optim.Adam(lG.parameters(), lr=1e-4, betas=(0.9, 0.999))
    real = enc(data)
    fake = lG(noise).detach()
    optD.zero_grad()
    loss = lD(fake).mean() - lD(real).mean()
    inter = (alpha.expand_as(real) * real + (1 - alpha.expand_as(real)) * fake).detach().requires_grad_(True)
    with route():
        prob = lD(inter)
        (grad,) = torch.autograd.grad(prob, inter, torch.ones_like(prob), create_graph=True, retain_graph=True)
        gp = 10.0 * ((torch.sqrt((grad.reshape(grad.shape[0], -1) ** 2).sum(1) + 1e-12) - 1) ** 2).mean()
        (loss + gp).backward()
    grads = {"D." + k: p.grad.detach().cpu().numpy().copy() for k, p in lD.named_parameters()}
    optD.step()
    optG.zero_grad()
    (-lD(lG(noise)).mean()).backward()
    grads.update({"G." + k: p.grad.detach().cpu().numpy().copy() for k, p in lG.named_parameters()})
    optG.step()
    return grads, float(loss.detach()), float(gp.detach())


def test_one_latent_gan_iteration_vs_fp64(monkeypatch):
    import contextlib
    from mpgan_amd import ext_models, ops
    monkeypatch.setitem(ops.OPTIONS, "set_encode", True)
    calls = count_launches(monkeypatch)
    sd, g = published()
    torch.manual_seed(3)
    lD, lG = ext_models.latent_D(256), ext_models.latent_G(128, 256)
    data = torch.from_numpy(g["x"])
    noise, alpha = torch.randn(8, 128) * 0.2, torch.rand(8, 1)

    def run(dtype, device, route):
        enc = ext_models.load_pcgan_encoder(sd, 3, 256, 256, "max1").to(device=device, dtype=dtype)
        d, gnet = copy.deepcopy(lD).to(device=device, dtype=dtype), copy.deepcopy(lG).to(device=device, dtype=dtype)
        grads, loss, gp = latent_gan_iteration(enc, d, gnet, *(t.to(device=device, dtype=dtype) for t in (data, noise, alpha)), route)
        after = {"D." + k: p.detach().cpu() for k, p in d.named_parameters()}
        after.update({"G." + k: p.detach().cpu() for k, p in gnet.named_parameters()})
        return grads, after, loss, gp

    ref, ref_after, ref_loss, ref_gp = run(torch.float64, "cpu", contextlib.nullcontext)
    control, _, _, _ = run(torch.float32, "cpu", contextlib.nullcontext)
    got, after, loss, gp = run(torch.float32, "cuda", lambda: ops.double_backward_route("cuda"))
    torch.cuda.synchronize()
    assert len(calls) == 1                                           # the real batch went through the one launch
    assert abs(loss - ref_loss) <= TOL * max(abs(ref_loss), 1e-3 * abs(ref_gp)) and abs(gp - ref_gp) <= TOL * abs(ref_gp)
    assert_grads(got, ref, TOL, control=control, what="latent GAN iteration")
    # Adam's first step is -lr g / (|g| + eps): a jump at g = 0.  Where a gradient is within the error ``assert_grads`` can accept
    # (CONTROL_CEILING of its tensor's largest) of zero, the step's sign is not determined; everywhere else the parameters agree.
    before = {**{"D." + k: p for k, p in lD.named_parameters()}, **{"G." + k: p for k, p in lG.named_parameters()}}
    for k, p in after.items():
        g64 = torch.from_numpy(ref[k]).abs()
        if float(g64.max()) == 0.0:      # the critic's last bias: its share of fake - real cancels and the penalty does not see it
            assert k == "D.model.4.bias"
            continue
        sure = g64 > 1.5 * CONTROL_CEILING * g64.max()
        assert bool(sure.any()) and not torch.equal(p, before[k].detach()), k
        assert float((p.double() - ref_after[k])[sure].abs().max()) <= TOL * float(ref_after[k].abs().max()), k
