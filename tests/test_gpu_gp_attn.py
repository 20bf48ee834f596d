"""GPU: the gradient penalty's attention core on the attention kernels (``ops.OPTIONS["gp_attn"]``: ``ops.AttnCoreFn`` /
``ops.AttnCoreVJPFn`` over ``mpg_attn_fwd`` / ``_bwd`` / ``_dd``) -- the op against its fp64 restatement, bit-reproducibility of the
second-order launch, the --gp D step of GAPT against the reference's golden and against the existing route, graph replay, and
peak memory."""
import pytest
import torch

from conftest import load_golden, rel_err, summary_err
from test_gp_attn_cpu import derivatives, make_inputs
from test_gpu_attn import _ref
from test_gpu_mab import launches   # noqa: F401 -- the fixture that counts the calls of every C-ABI entry point

pytestmark = pytest.mark.gpu
TIGHT = 1e-4        # the bar of test_gpu_attn.py for the same arithmetic (the fp32 formulas alone stay at 7.2e-7 on these shapes)
BAR = 1e-3          # the project's parity bar (two fp32 routes around the same GEMMs)

FAST = [(2, 30, 30, 4, 16), (2, 1, 30, 4, 16), (2, 10, 30, 4, 16), (2, 30, 10, 4, 16), (2, 64, 32, 2, 8), (2, 17, 5, 3, 32)]
GENERIC = [(2, 33, 32, 4, 16), (2, 40, 33, 4, 16), (2, 65, 32, 4, 16), (2, 1, 160, 4, 16), (1, 150, 150, 4, 16), (1, 160, 160, 2, 16)]
NAMES = ("o", "dq", "dk", "dv", "dPhi/dq", "dPhi/dk", "dPhi/dv", "dPhi/dG")


def _on_gpu(t, ignore, dims, use=("uq", "uk", "uv"), packed=False):
    from mpgan_amd import ops
    B, L, S, H, d = dims
    dev = torch.device("cuda:0")
    tg = {k: v.float().to(dev) for k, v in t.items()}
    ig = None if ignore is None else ignore.float().to(dev)
    o, first, second = derivatives(lambda q, k, v: ops.AttnCoreFn.apply(q, k, v, ig, B, L, S, H), tg, use, packed)
    torch.cuda.synchronize()
    return [o, *first, *second]


def _compare(dims, dead0, use=("uq", "uk", "uv"), packed=False):
    B, L, S, H, d = dims
    t, ignore = make_inputs(B, L, S, H, d, ignored_tile=True, dead0=dead0)
    got = _on_gpu(t, ignore, dims, use, packed)
    o, first, second = derivatives(lambda q, k, v: _ref(q, k, v, ignore, B, L, S, H), t, use)
    errs = {n: rel_err(g.double().cpu().numpy(), r.numpy()) for n, g, r in zip(NAMES, got, [o, *first, *second])}
    print(dims, "dead jet 0" if dead0 else "every jet live", "uq=None" if "uq" not in use else "", "packed" if packed else "",
          {n: f"{e:.2e}" for n, e in errs.items()})
    for n, g in zip(NAMES, got):
        assert bool(torch.isfinite(g).all()), n
        if dead0:
            assert float(g.reshape(B, -1)[0].abs().max()) == 0.0, ("the jet without a real key is not exactly zero", n)
    assert max(errs.values()) < TIGHT, errs


@pytest.mark.parametrize("dims", FAST + GENERIC)
def test_op_against_fp64(dims):
    """Value, dq / dk / dv and the four second-order outputs against the fp64 restatement on the CPU, per tensor; a random key mask
    (p = 0.3) in which jet 0 has no real key -- its rows are exact zeros in every output -- and, for S > 32, one wholly ignored
    tile of 32 keys.  Where that leaves the batch without a jet of several real keys (it is that one jet, or its other jet keeps one key
    behind the ignored tile), the same shape runs once more with every jet live."""
    _compare(dims, True)
    if dims[0] == 1 or dims[2] == 33:
        _compare(dims, False)


def test_op_without_a_cotangent_on_dq():
    """uq = None: what PMA's seed and ISAB's inducing points give (their queries depend on no input)."""
    _compare((2, 1, 30, 4, 16), True, use=("uk", "uv"))
    _compare((2, 40, 33, 4, 16), True, use=("uk", "uv"))


def test_op_on_column_slices_of_a_packed_projection():
    """q, k, v as column slices of one [rows, 3E] tensor (row stride 3E), both layouts of P."""
    _compare((2, 30, 30, 4, 16), True, packed=True)
    _compare((2, 40, 40, 4, 16), True, packed=True)


@pytest.mark.parametrize("dims", [(2, 30, 30, 4, 16), (2, 40, 33, 4, 16)])
def test_second_order_launch_is_reproducible(dims, launches):
    """Two launches of ``mpg_attn_dd`` on the same inputs: identical bits."""
    from mpgan_amd import ops
    B, L, S, H, d = dims
    t, ignore = make_inputs(B, L, S, H, d, ignored_tile=True)
    dev = torch.device("cuda:0")
    tg = {k: v.float().to(dev) for k, v in t.items()}
    q, k, v, go = (tg[n].clone().requires_grad_(True) for n in ("q", "k", "v", "go"))
    o = ops.AttnCoreFn.apply(q, k, v, ignore.float().to(dev), B, L, S, H)
    first = torch.autograd.grad(o, (q, k, v), go, create_graph=True)
    phi = sum((f * tg[n]).sum() for f, n in zip(first, ("uq", "uk", "uv")))
    launches.clear()
    a = torch.autograd.grad(phi, (q, k, v, go), retain_graph=True)
    b = torch.autograd.grad(phi, (q, k, v, go))
    assert launches.get("mpg_attn_dd") == 2, launches
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def _golden_step(loss, g, **kw):
    from oracle import train_ref as T
    from mpgan_amd import train
    B, N = g["data"].shape[:2]
    G, D = train.default_gapt(N, disc_dropout=0.0)
    G.load_state_dict(T.init_state_dict(T.gapt_param_shapes(True), 41, torch.float32))
    D.load_state_dict(T.init_state_dict(T.gapt_param_shapes(False), 42, torch.float32))
    ts = train.TrainStep(G, D, B, N, latent=64, use_graphs=False, loss=loss, gp_lambda=float(g["gp_lambda"]), lr_disc=0.0, **kw)
    ts.set_batch(torch.from_numpy(g["data"]).float().cuda(), torch.from_numpy(g["labels"]).float().cuda())
    nD = torch.from_numpy(g["noise_D"]).float().cuda()
    ts.fixed_noise = (nD, nD)
    ts.fixed_alpha = torch.from_numpy(g["alpha"]).float().cuda()
    ts._seg_D()
    torch.cuda.synchronize()
    return ts, D


@pytest.mark.parametrize("loss", ["ls", "w"])
def test_gradient_penalty_step_gapt_on_the_attention_route_vs_reference_golden(loss, launches):
    """``test_gradient_penalty_step_gapt_vs_reference_golden`` with ``gp_attn=True``: the same golden, assertions and tolerances, and
    ``mpg_attn_dd`` ran.  With the switch off it did not, and the step is bit-identical to one built without the argument."""
    g = load_golden(f"gp_step_gapt_{loss}.npz")
    launches.clear()
    ts, D = _golden_step(loss, g, gp_attn=True)
    n_mab = sum(1 for m in D.modules() if type(m).__name__ == "MAB")
    assert launches.get("mpg_attn_dd") == n_mab, launches     # (the route was taken, by every block)
    print(loss, "GP", float(ts.GP), "golden", float(g["gp"]))
    assert abs(float(ts.GP) - float(g["gp"])) < 1e-3 * abs(float(g["gp"]))
    assert abs(float(ts.D_loss) - (float(g["Dr"]) + float(g["Df"]))) < 1e-4 * max(abs(float(g["Dr"]) + float(g["Df"])), 1e-3)
    assert abs(float(ts.D_loss) + float(ts.GP) - float(g["D_loss"])) < 1e-3 * abs(float(g["D_loss"]))
    errs = {k: summary_err(k, p.grad, g["gradD__" + k]) for k, p in D.named_parameters()}
    print({k: f"{e:.2e}" for k, e in errs.items()})
    for k, p in D.named_parameters():
        assert bool(torch.isfinite(p.grad).all()), k
        assert errs[k] < 1e-3, (k, errs[k])
    # the one-launch block is first order: a second derivative through it fails loudly
    x = torch.from_numpy(g["data"]).float().cuda().requires_grad_(True)
    (gx,) = torch.autograd.grad(D(x).sum(), x, create_graph=True)
    with pytest.raises(RuntimeError):
        (gx ** 2).sum().backward()
    launches.clear()
    off, D_off = _golden_step(loss, g, gp_attn=False)
    assert "mpg_attn_dd" not in launches, launches
    plain, D_plain = _golden_step(loss, g)
    assert "mpg_attn_dd" not in launches, launches
    assert float(off.GP) == float(plain.GP) and float(off.D_loss) == float(plain.D_loss)
    for (k, a), (_, b) in zip(D_off.named_parameters(), D_plain.named_parameters()):
        assert torch.equal(a.grad, b.grad), k


def _discriminator(kind, N):
    """(G, D) of the three GAPT configurations the goldens do not cover, or the default MPGAN pair; seeded torch initialisation."""
    from mpgan_amd import train
    torch.manual_seed(21)
    if kind == "mpgan":
        return train.default_mpgan(N, disc_dropout=0.0, loss="w"), 32
    G, D = train.default_gapt(N, disc_dropout=0.0, use_isab=(kind == "isab"))
    if kind == "layer_norm":
        from mpgan_amd.gapt import GAPT_D
        lin = {"leaky_relu_alpha": 0.2, "dropout_p": 0.0, "batch_norm": False, "spectral_norm": False}
        D = GAPT_D(sab_layers=2, input_feat_size=3, final_fc_layers=[], dropout_p=0.0, layer_norm=True, num_particles=N, num_heads=4,
                   embed_dim=64, sab_fc_layers=[], use_mask=True, use_isab=False, num_isab_nodes=10, linear_args=lin).cuda()
    return (G, D), 64


def _route_step(kind, gp_attn, B=4, N=30):
    """One ``loss="w"``, ``gp_lambda=10`` D step: (penalty, D's gradients)."""
    from oracle.train_ref import synthetic_batch
    from mpgan_amd import train
    (G, D), lat = _discriminator(kind, N)
    data, labels = synthetic_batch(B, N, seed=13)
    ts = train.TrainStep(G, D, B, N, latent=lat, use_graphs=False, loss="w", gp_lambda=10.0, lr_disc=0.0, gp_attn=gp_attn)
    ts.set_batch(data.cuda(), labels.cuda())
    gen = torch.Generator(device="cuda").manual_seed(2)
    nz = torch.randn(B, N, lat, device="cuda", generator=gen) * 0.2
    ts.fixed_noise = (nz, nz)
    ts.fixed_alpha = torch.rand(B, 1, 1, device="cuda", generator=gen)
    ts._seg_D()
    torch.cuda.synchronize()
    return float(ts.GP), {k: p.grad.clone() for k, p in D.named_parameters()}


@pytest.mark.parametrize("kind, N", [("isab", 30), ("layer_norm", 30), ("default", 40)])
def test_attention_route_agrees_with_the_existing_route(kind, N, launches):
    """ISAB blocks (10 inducing points on either side), LayerNorm blocks, and sets of 40 (the generic kernels): penalty within 1e-3
    relative, every parameter gradient within 1e-3 (``rel_err``) of the existing route's."""
    gp0, g0 = _route_step(kind, False, N=N)
    assert "mpg_attn_dd" not in launches
    gp1, g1 = _route_step(kind, True, N=N)
    assert launches.get("mpg_attn_dd", 0) > 0, launches
    errs = {k: rel_err(g1[k].cpu().numpy(), g0[k].cpu().numpy()) for k in g0}
    print(kind, N, "GP", gp0, gp1, "relative", abs(gp1 - gp0) / abs(gp0), {k: f"{e:.2e}" for k, e in errs.items()})
    assert gp0 > 0 and abs(gp1 - gp0) < BAR * abs(gp0)
    assert max(errs.values()) < BAR, errs


def test_message_passing_discriminator_is_untouched_by_the_option():
    gp0, g0 = _route_step("mpgan", False)
    gp1, g1 = _route_step("mpgan", True)
    assert gp0 == gp1 and gp0 > 0
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k


def test_attention_route_graph_replay_equals_eager():
    """``test_gradient_penalty_under_graphs_equals_eager`` for GAPT with ``gp_attn=True`` (the weight-gradient side stream stays on):
    the captured iteration replays eager execution bit for bit over two steps."""
    from oracle import train_ref as T
    from oracle.train_ref import synthetic_batch
    from mpgan_amd import train
    B, N, lat = 8, 30, 64
    data, labels = synthetic_batch(B, N, seed=13)
    res = []
    for use_graphs in (False, True):
        G, D = train.default_gapt(N, disc_dropout=0.0)
        G.load_state_dict(T.init_state_dict(T.gapt_param_shapes(True), 41, torch.float32))
        D.load_state_dict(T.init_state_dict(T.gapt_param_shapes(False), 42, torch.float32))
        ts = train.TrainStep(G, D, B, N, latent=lat, use_graphs=use_graphs, loss="w", gp_lambda=10.0, gp_attn=True)
        assert ts.gp_attn and ts.wgrad_side
        ts.set_batch(data.cuda(), labels.cuda())
        gen = torch.Generator(device="cuda").manual_seed(2)
        ts.fixed_noise = (torch.randn(B, N, lat, device="cuda", generator=gen) * 0.2,
                          torch.randn(B, N, lat, device="cuda", generator=gen) * 0.2)
        ts.fixed_alpha = torch.rand(B, 1, 1, device="cuda", generator=gen)
        for _ in range(2):
            ts.step()
        torch.cuda.synchronize()
        res.append((ts.fD.flat.clone(), ts.fG.flat.clone(), float(ts.D_loss), float(ts.GP), float(ts.G_loss)))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]) and res[0][2:] == res[1][2:]
    assert res[0][3] > 0


def test_attention_route_takes_less_memory_than_the_existing_route():
    """Peak allocation of one --gp D step of GAPT at B = 16, N = 30, both routes measured here one after the other."""
    peaks = {}
    for gp_attn in (False, True):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        _route_step("default", gp_attn, B=16)
        peaks[gp_attn] = torch.cuda.max_memory_allocated() - base
    print("peak bytes of the D step: existing route", peaks[False], "attention route", peaks[True])
    assert peaks[True] < peaks[False], peaks
