"""GPU: the gradient penalty's LinearNets and discriminator head as twice-differentiable ops (``ops.OPTIONS["gp_chain"]``:
``ops.LinearNetFn`` over ``mpg_chain``, ``ops.DiscHeadDDFn`` over ``mpg_disc_head_fwd`` / ``mpg_disc_head_dd``) -- every output of
all three passes against the fp64 restatement, reproducibility and skipped work, the four penalty goldens, graph replay, and the
ATen launches the switch removes."""
import itertools

import numpy as np
import pytest
import torch

from conftest import load_golden, rel_err, summary_err
import gp_chain_ref as R

pytestmark = pytest.mark.gpu

BAR = 1e-3        # the bar of test_gpu_gp_rows.py / test_gpu_gp_attn.py (the gradient-penalty checks of test_gpu_train.py)
KINK = 1e-3       # every pre-activation of the fp64 restatement stays this far from the LeakyReLU kink
SCALE = 64.0      # of the inputs and biases, and so of every pre-activation: what makes a seed with min |Z| >= KINK likely


def _reset(seed=77, first_tag=300):
    from mpgan_amd import ops
    dev = torch.device("cuda:0")
    ops.set_seed(seed, dev)
    ops.dev_state(dev).tags = itertools.count(first_tag)


def _err(a, b):
    return rel_err(a.detach().double().cpu().numpy(), b.detach().double().cpu().numpy())


def _gpu(t):
    return t.float().cuda()


def _f32_exact(c):
    """The case with every fp64 tensor rounded to a value fp32 holds exactly: the fp64 restatement then sees the very inputs the
    kernels see (a dot product that cancels to 1e-4 of its terms would otherwise differ by the inputs' rounding alone)."""
    rnd = lambda v: v.float().double() if (torch.is_tensor(v) and v.is_floating_point()) else v
    return {k: ([rnd(q) for q in v] if isinstance(v, list) else rnd(v)) for k, v in c.items()}


# ------------------------------------------------------------------------------------------------ LinearNetFn
# name: (widths, columns handed over as the second part, final_linear, residual)
NETS = {"fn_F3": ([195, 256, 256, 32], 3, True, False),        # the default D node network, (192 | F): the MPG_CHAIN_ROUTE_CHAIN2 shape
        "fn_F32": ([224, 256, 256, 32], 32, True, False),
        "ff_resid": ([32, 32], 0, True, True),                # GAPT's 32 -> 32 final-linear with residual
        "loops": ([35, 40, 7], 0, False, False),              # the run-time-loops route; a last layer with an activation
        "split": ([20, 24, 24, 24, 6], 0, True, False)}       # four layers: two consecutive ops
DROPS = {"p0": 0.0, "word": 0.5, "byte": 0.3}                 # thr = 128 draws one bit per element, any other p one byte
CASES = [(n, M, "p0") for n in NETS for M in (1, 31, 33, 70)] + [(n, M, d) for n in NETS for M in (33, 70) for d in ("word", "byte")]
_net_cache = {}


def _net_keeps(widths, M, p, tag0):
    """The keep-and-scale masks of a ``linear_net_dd`` call whose first op drew the tag base ``tag0``, from ``ops.dropout_mask`` dumps:
    layer l of an op is site tag + 1 + l, consecutive ops take consecutive tag bases (8 apart)."""
    from mpgan_amd import ops
    thr, dscale = ops.drop_params(p)
    keeps = []
    for k, (i0, i1) in enumerate(ops.gp_chain_pieces(len(widths) - 1)):
        for l in range(i0, i1):
            keeps.append(ops.dropout_mask(M, widths[l + 1], tag0 + 8 * k + 1 + (l - i0), thr).double().cpu() * dscale)
    return keeps


def _run_net(name, M, drop):
    """One case through the op on the GPU and through the reference composition in fp64, once per session.  The seed is the first
    of the case's own sequence whose fp64 pre-activations all stay KINK clear of zero (under the call's keep masks)."""
    key = (name, M, drop)
    if key in _net_cache:
        return _net_cache[key]
    from mpgan_amd import ops
    widths, two, final_linear, resid = NETS[name]
    p = DROPS[drop]
    dev = torch.device("cuda:0")
    first_tag = 300
    keeps = None
    if p:
        _reset(first_tag=first_tag)     # (the seed the call below will run under; a dump draws no tag)
        keeps = _net_keeps(widths, M, p, first_tag * 8)
    for seed in range(1000 * len(name) + M, 1000 * len(name) + M + 400):
        c = _f32_exact(R.make_net(widths, M, seed, two=two, resid=resid, scale=SCALE))
        c["keeps"] = keeps
        zmin = min(float(z.abs().min()) for z in R.pre_activations(c, final_linear))
        if zmin >= KINK:
            break
    else:
        raise AssertionError(f"{key}: no seed keeps the pre-activations {KINK} clear of the kink")
    _reset(first_tag=first_tag)
    log = ops.dev_state(dev).tag_log = []
    try:
        op = lambda A, A2, W, b, r: ops.linear_net_dd(A, A2, W, b, final_linear=final_linear, alpha=R.ALPHA, p_drop=p, training=True,
                                                      resid=r, param_grads=True)
        got = R.net_derivatives(c, final_linear, op, conv=_gpu)
        got_a2 = R.net_derivatives(c, final_linear, op, conv=_gpu, use_u="A2") if two else None
    finally:
        ops.dev_state(dev).tag_log = None
    torch.cuda.synchronize()
    assert log[0] == ("linear_net", first_tag * 8, ops.drop_params(p)[0]), log[:2]
    ref = R.net_derivatives(c, final_linear)
    _net_cache[key] = dict(case=c, got=got, ref=ref, got_a2=got_a2, zmin=zmin, seed=seed, final_linear=final_linear)
    return _net_cache[key]


@pytest.mark.parametrize("name, M, drop", CASES)
def test_linear_net_against_fp64(name, M, drop):
    """Value, every first-order output (x_bar over both parts, resid_bar, W_bar, b_bar) and every second-order output (dPhi/dY_bar,
    dPhi/dW_l) per tensor as max-abs error over max-abs value; dPhi/db and dPhi/dX_0 are absent or exact zeros.  No element is
    left out: the case's seed keeps every fp64 pre-activation KINK away from the kink."""
    r = _run_net(name, M, drop)
    (y, first, second, _), (ry, rfirst, rsecond, _) = r["got"], r["ref"]
    L = len(r["case"]["W"])
    errs = {"y": _err(y, ry)}
    errs.update({f"first{i}": _err(a, b) for i, (a, b) in enumerate(zip(first, rfirst))})
    errs.update({f"second{i}": _err(a, b) for i, (a, b) in enumerate(zip(second[:L + 1], rsecond[:L + 1]))})
    print(name, M, drop, "seed", r["seed"], "min|Z|", f"{r['zmin']:.2e}", {k: f"{e:.2e}" for k, e in errs.items()})
    assert len(first) == len(rfirst) and r["zmin"] >= KINK
    for a in second[L + 1:]:
        assert a is None or float(a.abs().max()) == 0.0
    assert max(errs.values()) < BAR, errs


@pytest.mark.parametrize("name, M, drop", [("fn_F3", 70, "word"), ("loops", 33, "byte"), ("split", 33, "p0"), ("ff_resid", 31, "p0")])
def test_linear_net_second_order_is_reproducible(name, M, drop):
    """Two launches of the second-order pass (tangent chain + grouped weight gradients) give the same bits."""
    r = _run_net(name, M, drop)
    L = len(r["case"]["W"])
    for a, b in zip(r["got"][2][:L + 1], r["got"][3]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("name", ["fn_F3", "fn_F32"])
def test_linear_net_absent_cotangent_is_zero(name):
    """u on the second input part alone (the first part's cotangent never reaches the op) against the fp64 restatement with zeros there."""
    r = _run_net(name, 33, "p0")
    c = dict(r["case"])
    k = c["x"].shape[1] - c["two"]
    c["u"] = c["u"].clone()
    c["u"][:, :k] = 0
    ref = R.net_derivatives(c, r["final_linear"])
    L = len(c["W"])
    errs = {i: _err(a, b) for i, (a, b) in enumerate(zip(r["got_a2"][2][:L + 1], ref[2][:L + 1]))}
    assert max(errs.values()) < BAR, errs


# ------------------------------------------------------------------------------------------------ DiscHeadDDFn
HEADS = [(N, F, mean, sigmoid, drop) for N in (1, 5, 33) for F in (8, 35) for mean in (False, True) for sigmoid in (False, True)
         for drop in (False, True)]
_head_cache = {}


def _run_head(N, F, mean, sigmoid, drop, use=("U", "mu"), mask=True, B=3):
    key = (N, F, mean, sigmoid, drop, use, mask, B)
    if key in _head_cache:
        return _head_cache[key]
    from mpgan_amd import ops
    dev = torch.device("cuda:0")
    c = _f32_exact(R.make_head(B, N, F, 7 * N + F, mask=mask, zero_jet=mask and not mean and N > 1))
    p = 0.5 if drop else 0.0
    _reset(seed=91)
    op = lambda y, m, w, b: ops.DiscHeadDDFn.apply(y, m, w, b, ops.DiscHeadDDSettings(mean, sigmoid, p, True, None, True))
    got = R.head_derivatives(c, mean, sigmoid, None, op, use, conv=_gpu)
    keep = None
    if drop:
        thr, dscale = ops.drop_params(p)
        keep = ops.dropout_mask(B, 1, ops.last_tag(dev) + ops.TAG_GENERIC, thr).double().cpu().reshape(B) * dscale
    torch.cuda.synchronize()
    # the fp64 restatement: the op's own plain-torch form on fp64 CPU tensors under the kernel's keep.  (tests/test_gp_chain_cpu.py
    # holds it to 1e-10 against autograd's fp64 double backward of the composition, and at N = 1 under the mean with a mask -- where
    # that double backward itself keeps only three digits, 1.6e-3 off on dPhi/dm at F = 35 -- against 60-digit derivatives.)
    restated = lambda y, m, w, b: ops.DiscHeadDDFn.apply(y, m, w, b, ops.DiscHeadDDSettings(mean, sigmoid, 0.0, True, keep, True))
    ref = R.head_derivatives(c, mean, sigmoid, keep, restated, tuple(u for u in use if u != "zeroU"))
    _head_cache[key] = dict(case=c, got=got, ref=ref, keep=keep)
    return _head_cache[key]


def _head_errs(r):
    (out, first, second, _), (rout, rfirst, rsecond, _) = r["got"], r["ref"]
    errs = {"out": _err(out, rout)}
    errs.update({"d" + n: _err(a, b) for n, a, b in zip(("y", "w", "b", "m"), first, rfirst)})
    for n, a, b in zip(("g", "y", "w", "b", "m"), second, rsecond):
        if b is None or float(b.abs().max()) == 0.0:
            assert a is None or float(a.abs().max()) == 0.0, n
        else:
            errs["dPhi/d" + n] = _err(a, b)
    return errs


@pytest.mark.parametrize("N, F, mean, sigmoid, drop", HEADS)
def test_head_against_fp64(N, F, mean, sigmoid, drop):
    """Value, y_bar / w_bar / b_bar / m_bar and dPhi/dg, /dy, /dm, /dw, /db for B = 3 jets: a real-valued mask with a gradient and
    exact zeros, a jet with one real particle and -- under sum pooling -- an all-zero jet, whose rows of y_bar are exact zeros.
    Against the op's plain-torch form in fp64 (``_run_head`` says why); measured worst 1.5e-6, 1.3e-6 at N = 1 under the mean."""
    r = _run_head(N, F, mean, sigmoid, drop)
    errs = _head_errs(r)
    print(N, F, mean, sigmoid, drop, "keep", None if r["keep"] is None else r["keep"].tolist(), {k: f"{e:.2e}" for k, e in errs.items()})
    if not mean and N > 1:
        assert float(r["case"]["mask"][-1].abs().max()) == 0.0 and float(r["got"][1][0][-1].abs().max()) == 0.0
    assert max(errs.values()) < BAR, errs


@pytest.mark.parametrize("drop", [False, True])
def test_head_without_mask_single_particle(drop):
    """GAPT_D's form: N = 1, no mask, sigmoid (``mpg_disc_head_fwd``'s N = 1 form), B = 3 and the E = 64 of the default network."""
    r = _run_head(1, 64, False, True, drop, use=("U",), mask=False)
    errs = _head_errs(r)
    assert max(errs.values()) < BAR, errs


@pytest.mark.parametrize("N, F, mean", [(33, 35, True), (5, 8, False)])
def test_head_second_order_is_reproducible_and_null_cotangents_are_zeros(N, F, mean):
    r = _run_head(N, F, mean, True, True)
    for a, b in zip(r["got"][2], r["got"][3]):      # two launches of mode 1: the same bits
        assert (a is None and b is None) or torch.equal(a, b)
    only_mu = _run_head(N, F, mean, True, True, use=("mu",))["got"][2]           # U = NULL reaches the kernel
    zero_u = _run_head(N, F, mean, True, True, use=("zeroU", "mu"))["got"][2]    # U = a tensor of zeros
    for a, b in zip(only_mu, zero_u):
        assert torch.equal(a, b)
    only_u = _run_head(N, F, mean, True, True, use=("U",))
    assert max(_head_errs(only_u).values()) < BAR                                # mu = NULL


# ------------------------------------------------------------------------------------------------ whole steps
def _models(model, N, disc_dropout, loss):
    from oracle import train_ref as T
    from mpgan_amd import train
    if model == "gapt":
        G, D = train.default_gapt(N, disc_dropout=disc_dropout)
        G.load_state_dict(T.init_state_dict(T.gapt_param_shapes(True), 41, torch.float32))
        D.load_state_dict(T.init_state_dict(T.gapt_param_shapes(False), 42, torch.float32))
        return G, D, 64
    G, D = train.default_mpgan(N, disc_dropout=disc_dropout, loss=loss)
    G.load_state_dict(T.init_state_dict(T.mpgan_param_shapes(True), 41, torch.float32))
    D.load_state_dict(T.init_state_dict(T.mpgan_param_shapes(False), 42, torch.float32))
    return G, D, 32


def _golden_step(model, loss, g, **kw):
    from mpgan_amd import train, ops
    B, N = g["data"].shape[:2]
    G, D, lat = _models(model, N, 0.0, loss)
    ts = train.TrainStep(G, D, B, N, latent=lat, use_graphs=False, loss=loss, gp_lambda=float(g["gp_lambda"]), lr_disc=0.0, **kw)
    ts.set_batch(torch.from_numpy(g["data"]).float().cuda(), torch.from_numpy(g["labels"]).float().cuda())
    nD = torch.from_numpy(g["noise_D"]).float().cuda()
    ts.fixed_noise = (nD, nD)
    ts.fixed_alpha = torch.from_numpy(g["alpha"]).float().cuda()
    dev = torch.device("cuda:0")
    log = ops.dev_state(dev).tag_log = []
    try:
        ts._seg_D()
    finally:
        ops.dev_state(dev).tag_log = None
    torch.cuda.synchronize()
    return ts, D, [kind for kind, *_ in log]


@pytest.mark.parametrize("model", ["mpgan", "gapt"])
@pytest.mark.parametrize("loss", ["w", "ls"])
@pytest.mark.parametrize("others", [False, True])
def test_gradient_penalty_step_with_gp_chain_vs_reference_golden(model, loss, others):
    """The four penalty goldens with ``gp_chain=True`` -- alone and on top of ``gp_rows`` / ``gp_attn`` -- at the assertions and
    tolerances of the existing golden tests, and the route was taken: every LinearNet of the penalty and the head."""
    g = load_golden(f"gp_step_{model}_{loss}.npz")
    ts, D, kinds = _golden_step(model, loss, g, gp_chain=True, gp_rows=others, gp_attn=others)
    assert ts.gp_chain and not ts.wgrad_side
    assert kinds.count("head_dd") == 1
    if model == "mpgan":
        assert kinds.count("linear_net") == len(D.mp_layers) * (1 if others else 2)      # fn of every layer (+ fe on the materialised route)
    else:
        n_mab = sum(1 for m in D.modules() if type(m).__name__ == "MAB")
        assert kinds.count("linear_net") == n_mab + 1                                    # every block's ff + the input embedding
    print(model, loss, others, "GP", float(ts.GP), "golden", float(g["gp"]))
    assert abs(float(ts.GP) - float(g["gp"])) < 1e-3 * abs(float(g["gp"]))
    assert abs(float(ts.D_loss) - (float(g["Dr"]) + float(g["Df"]))) < 1e-4 * max(abs(float(g["Dr"]) + float(g["Df"])), 1e-3)
    assert abs(float(ts.D_loss) + float(ts.GP) - float(g["D_loss"])) < 1e-3 * abs(float(g["D_loss"]))
    errs = {k: summary_err(k, p.grad, g["gradD__" + k]) for k, p in D.named_parameters()}
    print({k: f"{e:.2e}" for k, e in errs.items()})
    for k, p in D.named_parameters():
        assert bool(torch.isfinite(p.grad).all()), k
        assert errs[k] < 1e-3, (k, errs[k])


@pytest.mark.parametrize("model", ["mpgan", "gapt"])
def test_switch_off_is_the_existing_route(model):
    """``gp_chain=False`` and a step built without the argument: no op of the new route is called, and one iteration leaves
    bit-identical gradients and losses."""
    g = load_golden(f"gp_step_{model}_w.npz")
    off, D_off, kinds_off = _golden_step(model, "w", g, gp_chain=False)
    plain, D_plain, kinds_plain = _golden_step(model, "w", g)
    for kinds in (kinds_off, kinds_plain):
        assert "linear_net" not in kinds and "head_dd" not in kinds
    assert not off.gp_chain and not plain.gp_chain
    assert float(off.GP) == float(plain.GP) and float(off.D_loss) == float(plain.D_loss)
    for (k, a), (_, b) in zip(D_off.named_parameters(), D_plain.named_parameters()):
        assert torch.equal(a.grad, b.grad), k


def _dropout_step(model, gp_chain, use_graphs, steps=2, B=4, N=30):
    from oracle.train_ref import synthetic_batch
    from mpgan_amd import train, ops
    dev = torch.device("cuda:0")
    torch.manual_seed(5)
    _reset(seed=4242, first_tag=9000)
    G, D, lat = _models(model, N, 0.5, "w")
    data, labels = synthetic_batch(B, N, seed=13)
    ts = train.TrainStep(G, D, B, N, latent=lat, use_graphs=use_graphs, loss="w", gp_lambda=10.0, gp_chain=gp_chain)
    ts.set_batch(data.cuda(), labels.cuda())
    gen = torch.Generator(device="cuda").manual_seed(2)
    ts.fixed_noise = (torch.randn(B, N, lat, device="cuda", generator=gen) * 0.2, torch.randn(B, N, lat, device="cuda", generator=gen) * 0.2)
    ts.fixed_alpha = torch.rand(B, 1, 1, device="cuda", generator=gen)
    torch.manual_seed(6)
    _reset(seed=4242, first_tag=9000)
    return ts, dev


@pytest.mark.parametrize("model", ["mpgan", "gapt"])
def test_gp_chain_with_dropout_graph_replay_equals_eager(model):
    """The --gp iteration with ``gp_chain=True`` and disc_dropout = 0.5 at N = 30, B = 4: every draw of the penalty comes from the
    device seed and the tag allocator, so the captured iteration replays what eager execution computes, bit for bit."""
    from mpgan_amd import ops
    res = []
    for use_graphs in (False, True):
        ts, dev = _dropout_step(model, True, use_graphs)
        if use_graphs:
            ts.capture(warmup=0)
        for _ in range(2):
            if not use_graphs:   # (a captured step keeps the dropout sites it was captured with: the eager steps take the same ones)
                ops.dev_state(dev).tags = itertools.count(9000)
            ts.step()
        torch.cuda.synchronize()
        res.append((ts.fD.flat.clone(), ts.fG.flat.clone(), float(ts.D_loss), float(ts.GP), float(ts.G_loss)))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]) and res[0][2:] == res[1][2:], (res[0][2:], res[1][2:])
    assert res[0][3] > 0


def _aten_counts(model, gp_chain):
    """Launches of one eager penalty D step by ATen operator, through the profiler hook tools/opcount.py uses."""
    from torch.profiler import profile, ProfilerActivity
    ts, dev = _dropout_step(model, gp_chain, False)
    ts._seg_D()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        ts._seg_D()
        torch.cuda.synchronize()
    return {e.key: e.count for e in prof.key_averages() if e.key.startswith("aten::")}


@pytest.mark.parametrize("model", ["mpgan", "gapt"])
def test_step_with_gp_chain_launches_no_aten_leaky_relu_or_dropout(model):
    """With the switch on (dropout 0.5) a penalty D step calls no ATen ``leaky_relu`` / ``native_dropout`` (forward or backward) and
    draws nothing from torch's generator; with it off it does -- the composites of ``LinearNet._forward_dd``."""
    banned = ("leaky_relu", "native_dropout", "bernoulli")
    on = {k: n for k, n in _aten_counts(model, True).items() if any(b in k for b in banned)}
    off = {k: n for k, n in _aten_counts(model, False).items() if any(b in k for b in banned)}
    print(model, "switch off:", off, "switch on:", on)
    assert off and not on, (off, on)
