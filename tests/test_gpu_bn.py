"""GPU parity of batch norm on the un-fused route: ``mpg_batchnorm_stats / _apply / _bwd`` (csrc/bn.hip) through
``ops.BatchNormFn``, ``ops.batchnorm_eval``, ``LinearNet._bn`` and the C ABI itself, against ``torch.nn.BatchNorm1d`` in float64 on
the CPU (fed the float32 inputs cast up, training mode, its own autograd), and batch norm inside ``LinearNet`` and the un-fused
``MPLayer`` against a float64 stack and the reference's own ``MPLayer`` (tests/golden/mplayer_bn_f64.npz).

The shapes are the smallest that reach each path of the kernels: one chunk and several (``nchunk = max(1, min(256, M // 64))``,
``per = ceil(M / nchunk)`` rows each, the last chunk short, trailing chunks empty), one feature tile of 64 and several with a
ragged last one, and the one workload shape (the 7200 edge rows of B = 8, N = 30 at width 192)."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_golden, rel_err, summary_err

pytestmark = pytest.mark.gpu

TOL = 1e-3       # BASELINE.json north_star (tests/test_gpu_mplayer.py)
TIGHT = 1e-4
SENTINEL = 12345.0


def _dev():
    return torch.device("cuda:0")


def _nchunk(M):
    return max(1, min(256, M // 64))


def _inputs(M, F, seed, sigma=1.0, offset=None):
    """float32 on the CPU: x with a nonzero mean per feature, affine weight and bias, upstream gradient."""
    rs = np.random.RandomState(seed)
    mu = rs.uniform(0.5, 3.0, size=F) * rs.choice([-1.0, 1.0], size=F) if offset is None else np.full(F, offset)
    x = torch.from_numpy(mu + sigma * rs.normal(size=(M, F))).float()
    w = torch.from_numpy(rs.uniform(0.5, 1.5, size=F) * rs.choice([-1.0, 1.0], size=F)).float()
    b = torch.from_numpy(rs.normal(size=F)).float()
    g = torch.from_numpy(rs.normal(size=(M, F))).float()
    return x, w, b, g


def _reference(x, w, b, g, eps, dtype=torch.float64):
    """nn.BatchNorm1d in ``dtype`` on the CPU, training mode: y, dx, dw, db, batch mean, biased batch variance."""
    F = x.shape[1]
    bn = torch.nn.BatchNorm1d(F, eps=eps, momentum=1.0).to(dtype).train()
    with torch.no_grad():
        bn.weight.copy_(w.to(dtype))
        bn.bias.copy_(b.to(dtype))
    xr = x.detach().clone().to(dtype).requires_grad_(True)
    y = bn(xr)
    (y * g.to(dtype)).sum().backward()
    M = x.shape[0]
    # (momentum 1: the running statistics ARE the batch's -- the variance in its unbiased form)
    return {"y": y.detach(), "dx": xr.grad, "dw": bn.weight.grad, "db": bn.bias.grad, "mean": bn.running_mean.clone(),
            "var": bn.running_var * (M - 1) / M}


def _run_fn(x, w, b, g, eps):
    from mpgan_amd import ops
    d = _dev()
    xg, wg, bg = (t.to(d).requires_grad_(True) for t in (x, w, b))
    y, mean, var = ops.BatchNormFn.apply(xg, wg, bg, eps)
    (y * g.to(d)).sum().backward()
    return {"y": y.detach(), "dx": xg.grad, "dw": wg.grad, "db": bg.grad, "mean": mean, "var": var}


def _errs(got, ref):
    return {k: rel_err(got[k].double().cpu().numpy(), ref[k].double().numpy()) for k in ref if got.get(k) is not None}


# (M, F, eps).  At M = 2 the input gradient is  w rstd (g0 - g1) / 2 * eps / (var + eps): with the default eps = 1e-5 and unit
# variance a difference that cancels to 1e-5 of its terms, which no float32 evaluation resolves to 1e-4 of itself (float32
# rounding 6e-8 of the terms = 6e-3 of the result; torch's own float32 batch norm included).  The two-row case checks the
# kernels' row loops and reductions, not that cancellation: it runs with eps = 1, where the difference keeps half of its terms.
CASES = [(2, 1, 1.0), (63, 64, 1e-5), (64, 65, 1e-5), (129, 130, 1e-5), (200, 96, 1e-5), (7200, 192, 1e-5), (16390, 3, 1e-5)]


@pytest.mark.parametrize("M,F,eps", CASES, ids=lambda v: str(v))
def test_batchnorm_fn_vs_fp64(M, F, eps):
    """One chunk (2 and 63 rows), two feature tiles with one live lane in the second (64 x 65), chunks of 65 and 64 rows
    (129 x 130), three chunks of 67, 67, 66 (200 x 96), the workload's 112 chunks (7200 x 192), and the cap of 256 chunks of 65
    rows with chunk 252 short and chunks 253 .. 255 empty (16390 x 3)."""
    nchunk = _nchunk(M)
    per = -(-M // nchunk)
    assert {2: (1, 2), 63: (1, 63), 64: (1, 64), 129: (2, 65), 200: (3, 67), 7200: (112, 65), 16390: (256, 65)}[M] == (nchunk, per)
    if M == 16390:
        assert M - 252 * per == 10 and 253 * per > M
    x, w, b, g = _inputs(M, F, seed=M + F)
    errs = _errs(_run_fn(x, w, b, g, eps), _reference(x, w, b, g, eps))
    print("errs", (M, F), errs)
    assert set(errs) == {"y", "dx", "dw", "db", "mean", "var"}
    assert max(errs.values()) < TIGHT, errs


def test_batchnorm_offset_inputs_two_pass_variance():
    """x = 50 + 0.01 N(0, 1): the variance is 4e-6 of the mean's square, so a one-pass E[x^2] - E[x]^2 in float32 has nothing
    left of it.  No bar can be derived for this input; the yardstick is torch's own float32 batch norm on the same inputs
    against the float64 run: the kernels' error must be at most twice that (the summation order differs) or TIGHT, whichever
    is larger, per tensor."""
    M, F, eps = 7200, 96, 1e-5
    x, w, b, g = _inputs(M, F, seed=5, sigma=0.01, offset=50.0)
    ref = _reference(x, w, b, g, eps)
    yard = _errs(_reference(x, w, b, g, eps, dtype=torch.float32), ref)
    errs = _errs(_run_fn(x, w, b, g, eps), ref)
    print("offset case: kernels", errs, "torch float32", yard)
    assert set(errs) == {"y", "dx", "dw", "db", "mean", "var"}
    bad = {k: (v, yard[k]) for k, v in errs.items() if not v <= max(2.0 * yard[k], TIGHT)}
    assert not bad, (bad, errs, yard)


def test_batchnorm_frozen_norm():
    """Only x requires a gradient (the discriminator's norm inside the generator's step): dx is right, the norm's parameters get
    nothing."""
    from mpgan_amd import ops
    M, F, eps = 129, 70, 1e-5
    x, w, b, g = _inputs(M, F, seed=11)
    d = _dev()
    xg, wg, bg = x.to(d).requires_grad_(True), torch.nn.Parameter(w.to(d), requires_grad=False), torch.nn.Parameter(b.to(d), requires_grad=False)
    y, _, _ = ops.BatchNormFn.apply(xg, wg, bg, eps)
    (y * g.to(d)).sum().backward()
    ref = _reference(x, w, b, g, eps)
    assert rel_err(y.detach().cpu().numpy(), ref["y"].numpy()) < TIGHT
    assert rel_err(xg.grad.cpu().numpy(), ref["dx"].numpy()) < TIGHT
    assert wg.grad is None and bg.grad is None


# ---- the C ABI itself ---------------------------------------------------------------------------------------------------------
def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _abi(x, w, b, g, eps, *, pad=0, accumulate=False, dx=True, dw=True, db=True, affine=True, pre=None):
    """stats + apply + bwd through ``_lib.lib()`` with row strides F + pad; y and dx live in sentinel-filled buffers of that
    stride.  ``pre`` = (dw0, db0): the contents the gradient buffers start with."""
    from mpgan_amd import _lib
    lib, d, st = _lib.lib(), _dev(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    M, F = x.shape
    ld = F + pad
    nchunk = _nchunk(M)

    def wide(t):
        buf = torch.full((M, ld), SENTINEL, device=d)
        if t is not None:
            buf[:, :F] = t.to(d)
        return buf
    xb, gb, yb, dxb = wide(x), wide(g), wide(None), wide(None)
    wd, bd = (w.to(d), b.to(d)) if affine else (None, None)
    part = torch.empty(2 * nchunk * F, device=d)
    mean, var, sums = torch.empty(F, device=d), torch.empty(F, device=d), torch.empty(2 * F, device=d)
    dwb = (pre[0].to(d).clone() if pre else torch.full((F,), SENTINEL, device=d)) if dw else None
    dbb = (pre[1].to(d).clone() if pre else torch.full((F,), SENTINEL, device=d)) if db else None
    assert lib.mpg_batchnorm_stats(_ptr(xb), ld, M, F, _ptr(part), nchunk, _ptr(mean), _ptr(var), st) == 0
    assert lib.mpg_batchnorm_apply(_ptr(xb), ld, _ptr(mean), _ptr(var), _ptr(wd), _ptr(bd), eps, _ptr(yb), ld, M, F, st) == 0
    assert lib.mpg_batchnorm_bwd(_ptr(gb), ld, _ptr(xb), ld, _ptr(mean), _ptr(var), _ptr(wd), eps, _ptr(part), nchunk, _ptr(sums),
                                 _ptr(dxb) if dx else None, ld, _ptr(dwb), _ptr(dbb), int(accumulate), M, F, st) == 0
    torch.cuda.synchronize()
    return {"y": yb, "dx": dxb, "dw": dwb, "db": dbb, "mean": mean, "var": var}


def _pads_intact(buf, F):
    s = int(torch.tensor(SENTINEL).view(torch.int32))
    return bool((buf.view(torch.int32)[:, F:] == s).all())


def test_batchnorm_abi_row_strides():
    """ldx = ldg = ldy = lddx = F + 3 at three chunks and two feature tiles: the three pad columns of y and dx come back untouched."""
    M, F, eps = 200, 70, 1e-5
    x, w, b, g = _inputs(M, F, seed=21)
    out, ref = _abi(x, w, b, g, eps, pad=3), _reference(x, w, b, g, eps)
    assert _pads_intact(out["y"], F) and _pads_intact(out["dx"], F)
    got = dict(out, y=out["y"][:, :F], dx=out["dx"][:, :F])
    errs = _errs(got, ref)
    assert len(errs) == 6 and max(errs.values()) < TIGHT, errs


def test_batchnorm_abi_accumulate():
    """accumulate = 1: dw / db = what the buffers held + the gradient."""
    M, F, eps = 129, 65, 1e-5
    x, w, b, g = _inputs(M, F, seed=22)
    rs = np.random.RandomState(23)
    dw0, db0 = (torch.from_numpy(rs.normal(size=F) * 5).float() for _ in range(2))
    out, ref = _abi(x, w, b, g, eps, accumulate=True, pre=(dw0, db0)), _reference(x, w, b, g, eps)
    assert rel_err(out["dw"].cpu().numpy(), (dw0.double() + ref["dw"]).numpy()) < TIGHT
    assert rel_err(out["db"].cpu().numpy(), (db0.double() + ref["db"]).numpy()) < TIGHT
    assert rel_err(out["dx"].cpu().numpy(), ref["dx"].numpy()) < TIGHT
    # ... and accumulate = 0 overwrites whatever was there
    out = _abi(x, w, b, g, eps, accumulate=False, pre=(dw0, db0))
    assert rel_err(out["dw"].cpu().numpy(), ref["dw"].numpy()) < TIGHT
    assert rel_err(out["db"].cpu().numpy(), ref["db"].numpy()) < TIGHT


@pytest.mark.parametrize("absent", ["dx", "dw", "db"])
def test_batchnorm_abi_null_outputs(absent):
    """dx, dw or db = NULL, one at a time: the other two stay correct (and dx's buffer, when not handed over, is not written)."""
    M, F, eps = 129, 65, 1e-5
    x, w, b, g = _inputs(M, F, seed=24)
    out, ref = _abi(x, w, b, g, eps, **{absent: False}), _reference(x, w, b, g, eps)
    for k in {"dx", "dw", "db"} - {absent}:
        assert rel_err(out[k].cpu().numpy(), ref[k].numpy()) < TIGHT, k
    if absent == "dx":
        assert _pads_intact(out["dx"], 0)
    else:
        assert out[absent] is None


def test_batchnorm_abi_plain_normalisation():
    """w = b = NULL in apply (and w = NULL in the backward): y = xhat, dx that of a weight of ones."""
    M, F, eps = 200, 33, 1e-5
    x, w, b, g = _inputs(M, F, seed=25)
    out = _abi(x, w, b, g, eps, affine=False)
    ref = _reference(x, torch.ones(F), torch.zeros(F), g, eps)
    errs = _errs(out, ref)
    assert len(errs) == 6 and max(errs.values()) < TIGHT, errs


def test_batchnorm_abi_rejects_empty_shapes():
    from mpgan_amd import _lib
    lib, d = _lib.lib(), _dev()
    t = torch.zeros(64, device=d)
    p, st = _ptr(t), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for M, F, nchunk in [(0, 4, 1), (4, 0, 1), (4, 4, 0), (-1, 4, 1)]:
        assert lib.mpg_batchnorm_stats(p, 4, M, F, p, nchunk, p, p, st) == -1, (M, F, nchunk)
        assert lib.mpg_batchnorm_bwd(p, 4, p, 4, p, p, p, 1e-5, p, nchunk, p, p, 4, p, p, 0, M, F, st) == -1, (M, F, nchunk)
    for M, F in [(0, 4), (4, 0)]:
        assert lib.mpg_batchnorm_apply(p, 4, p, p, p, p, 1e-5, p, 4, M, F, st) == -1, (M, F)
    torch.cuda.synchronize()
    assert float(t.abs().max()) == 0.0


# ---- running statistics ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("momentum", [0.1, None])
def test_linearnet_bn_running_statistics(momentum):
    """``LinearNet._bn`` over three training forwards of 40, 129 and 2 rows, then an eval forward (``ops.batchnorm_eval``), against
    nn.BatchNorm1d in float64: running mean, running variance (unbiased: M / (M - 1)), the batch counter, the eval output; with
    momentum 0.1 and with the cumulative average (momentum None)."""
    from mpgan_amd.mpgan import LinearNet
    F = 70
    net = LinearNet([F], input_size=5, batch_norm=True).to(_dev()).train()
    bn = net.bn[0]
    bn.momentum = momentum
    rs = np.random.RandomState(31)
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(rs.uniform(0.5, 1.5, size=F)).float())
        bn.bias.copy_(torch.from_numpy(rs.normal(size=F)).float())
    ref = torch.nn.BatchNorm1d(F, momentum=momentum).double().train()
    with torch.no_grad():
        ref.weight.copy_(bn.weight.double().cpu())
        ref.bias.copy_(bn.bias.double().cpu())
    for M in (40, 129, 2):
        x = torch.from_numpy(1.5 + rs.normal(size=(M, F))).float()
        y = net._bn(0, x.to(_dev()))
        assert rel_err(y.detach().cpu().numpy(), ref(x.double()).detach().numpy()) < TIGHT, M
    assert int(bn.num_batches_tracked) == int(ref.num_batches_tracked) == 3
    assert rel_err(bn.running_mean.cpu().numpy(), ref.running_mean.numpy()) < TIGHT
    assert rel_err(bn.running_var.cpu().numpy(), ref.running_var.numpy()) < TIGHT
    net.eval()
    ref.eval()
    x = torch.from_numpy(1.5 + rs.normal(size=(77, F))).float()
    y = net._bn(0, x.to(_dev()))
    assert rel_err(y.detach().cpu().numpy(), ref(x.double()).detach().numpy()) < TIGHT
    assert int(bn.num_batches_tracked) == 3    # (an eval forward moves nothing)
    assert rel_err(bn.running_mean.cpu().numpy(), ref.running_mean.numpy()) < TIGHT


# ---- batch norm inside the networks ---------------------------------------------------------------------------------------------
WIDTHS, IN, ROWS = [96, 160, 192], 7, 576
MARGIN = 1e-4


def _linearnet_case(seed=0):
    """float32 parameters, input and upstream gradient on the CPU.  576 x (96 + 160 + 192) = 258 048 pre-activations drawn
    around zero would put some ninety of them within MARGIN of zero under ANY seed (a normal density of 0.4 per sigma, the maximum at
    4.5 sigma), and behind a dropout layer the pre-activations depend on keep masks that only the GPU run draws -- no seed can be
    chosen for them beforehand.  So the margin is built in, not searched for: every feature's bias is +-(3.5 .. 4.5) against
    products of standard deviation <= 0.7 (weights N(0, 0.1 / K)), which keeps a feature on one side of the kink for every row
    and every mask -- half of the features on the negative slope.  In the first layer a third of the features change side from
    row to row instead: input column 0 is +-1 per row and enters them with weight +-5 beside a small bias.  The test asserts the
    margin the float64 stack found."""
    rs = np.random.RandomState(100 + seed)
    d = [IN] + WIDTHS
    prm = {}
    for k in range(3):
        prm[f"net.{k}.weight"] = torch.from_numpy(rs.normal(size=(d[k + 1], d[k])) * np.sqrt(0.1 / d[k])).float()
        prm[f"net.{k}.bias"] = torch.from_numpy(rs.uniform(3.5, 4.5, size=d[k + 1]) * rs.choice([-1.0, 1.0], size=d[k + 1])).float()
        prm[f"bn.{k}.weight"] = torch.from_numpy(rs.uniform(0.5, 1.5, size=d[k + 1])).float()
        prm[f"bn.{k}.bias"] = torch.from_numpy(rs.normal(size=d[k + 1]) * 0.3).float()
    x = torch.from_numpy(rs.normal(size=(ROWS, IN))).float()
    x[:, 0] = torch.from_numpy(rs.choice([-1.0, 1.0], size=ROWS)).float()
    n = WIDTHS[0] // 3
    prm["net.0.weight"][:n, 0] = torch.from_numpy(5.0 * rs.choice([-1.0, 1.0], size=n)).float()
    prm["net.0.bias"][:n] = torch.from_numpy(rs.normal(size=n) * 0.3).float()
    g = torch.from_numpy(rs.normal(size=(ROWS, WIDTHS[-1]))).float()
    return prm, x, g


def _linearnet_ref(prm, x, g, alpha, keeps):
    """The float64 stack Linear -> LeakyReLU -> BatchNorm1d -> dropout (``keeps``: keep mask times its scale per layer): output,
    dx, parameter gradients, the smallest |pre-activation| / max|pre-activation| over the layers, and for every bias the
    magnitude of its TERMS -- a bias gradient is the sum over the rows of the gradient at the Linear's / the norm's output; this is
    the largest l2 norm of a column of that."""
    p = {k: v.double().requires_grad_(True) for k, v in prm.items()}
    h = x.double().requires_grad_(True)
    x64, margin, rows = h, float("inf"), {}
    for k in range(3):
        z = h @ p[f"net.{k}.weight"].t() + p[f"net.{k}.bias"]
        margin = min(margin, float(z.detach().abs().min() / z.detach().abs().max()))
        a = torch.nn.functional.leaky_relu(z, alpha)
        n = torch.nn.functional.batch_norm(a, None, None, p[f"bn.{k}.weight"], p[f"bn.{k}.bias"], True, 0.1, 1e-5)
        z.retain_grad()
        n.retain_grad()
        rows[f"net.{k}.bias"], rows[f"bn.{k}.bias"] = z, n
        h = n * keeps[k]
    (h * g.double()).sum().backward()
    terms = {k: float(v.grad.norm(dim=0).max()) for k, v in rows.items()}
    return h.detach(), x64.grad, {k: v.grad for k, v in p.items()}, margin, terms


@pytest.mark.parametrize("alpha", [1.0, 0.2])
@pytest.mark.parametrize("p_drop", [0.0, 0.5, 0.3])
def test_linearnet_batch_norm_vs_fp64(p_drop, alpha):
    """``LinearNet([96, 160, 192], input_size=7, batch_norm=True, dropout_p=p)`` on 576 rows (nine chunks of 64, feature tiles
    of 96 = 64 + 32, 160 = 2 x 64 + 32, 192 = 3 x 64): forward, dx and every parameter gradient against the float64 stack with
    the launches' own keep masks (bit mode at p = 0.5, byte mode at 0.3).  Slope 1 has no kink: TIGHT throughout.  At slope 0.2
    the smallest pre-activation of the float64 stack is more than MARGIN of the largest (asserted; ``_linearnet_case``), far beyond
    what float32 rounding moves, so no element changes side: TIGHT for the forward, TOL for the gradients."""
    from mpgan_amd import ops
    from mpgan_amd.mpgan import LinearNet
    dev = _dev()
    prm, x, g = _linearnet_case()
    net = LinearNet(WIDTHS, input_size=IN, batch_norm=True, dropout_p=p_drop, leaky_relu_alpha=alpha).to(dev).train()
    sd = net.state_dict()
    sd.update({k: v.to(dev) for k, v in prm.items()})
    net.load_state_dict(sd)
    ops.set_seed(77, dev)
    st = ops.dev_state(dev)
    st.tag_log = []
    try:
        xg = x.to(dev).requires_grad_(True)
        y = net(xg)
        log = list(st.tag_log)
    finally:
        st.tag_log = None
    (y * g.to(dev)).sum().backward()
    thr, scale = ops.drop_params(p_drop)
    tags = [t for kind, t, _ in log if kind == "dropout"]
    assert len(tags) == (3 if thr else 0) and (not thr or tags[-1] == ops.last_tag(dev))
    keeps = [ops.dropout_mask(ROWS, wd, tags[k] + ops.TAG_GENERIC, thr, dev).double().cpu() * scale if thr
             else torch.ones(ROWS, wd, dtype=torch.float64) for k, wd in enumerate(WIDTHS)]
    for m in keeps:
        q = 1 - thr / 256.0
        assert abs(float((m != 0).double().mean()) - q) < max(0.01, 5 * (q * (1 - q) / m.numel()) ** 0.5)
    y_ref, dx_ref, grads, margin, terms = _linearnet_ref(prm, x, g, alpha, keeps)
    assert margin > MARGIN, margin
    err_y = rel_err(y.detach().cpu().numpy(), y_ref.numpy())
    got = {"dx": xg.grad.double().cpu(), **{k: q.grad.double().cpu() for k, q in net.named_parameters()}}
    ref = {"dx": dx_ref, **grads}
    assert set(got) == set(ref) and len(ref) == 1 + 12
    # Every tensor against its own maximum -- except that a bias is held to the magnitude of its terms where that is larger.  A
    # norm takes the mean out of its input, so a bias in front of one has no gradient wherever what lies between them is linear
    # over the batch: net.k.bias in every feature at slope 1 and in the one-sided features at slope 0.2, bn.k.bias without dropout.
    # The sum over the rows that cancels there is known to the rounding of its terms, not of itself (as tests/spectral_ref.py
    # measures a dW that cancels: ``terms_scale``): the ones column of the weight-gradient product carries 2^-17 of every term
    # (bf16 hi/lo: 16 bits), independently from row to row, i.e. 2^-17 = 7.6e-6 of the l2 norm of the column it adds up -- TIGHT
    # is 13 of those.  A row left out or counted twice is one term of ~1/24 of that norm: 400 times the bar.
    errs = {k: float((got[k] - ref[k]).abs().max() / max(float(ref[k].abs().max()), terms.get(k, 0.0))) for k in ref}
    print("y", err_y, errs, "l2 of the bias terms", terms)
    assert err_y < TIGHT, err_y
    bar = TIGHT if alpha == 1.0 else TOL
    assert max(errs.values()) < bar, errs


def test_mplayer_batch_norm_vs_reference_golden():
    """``MPLayer(32, [96, 160, 192], [256, 256], 32, batch_norm=True)`` on the un-fused route at B = 3, N = 10 with one empty
    jet, against the reference's own layer in float64 (tests/gen_golden.py: ``mplayer_bn``): the edge network's norms take their
    statistics over ALL B N N edge rows, those of masked senders included (the mask multiplies the edge network's output), the
    node network's over all B N rows.  Bars of the ``edges`` route of test_mplayer_options_vs_reference_golden; the running
    statistics after the one call at TIGHT."""
    from oracle import train_ref as T
    from mpgan_amd.mpgan import MPLayer
    g = load_golden("mplayer_bn_f64.npz")
    layer = MPLayer(32, [96, 160, 192], [256, 256], 32, batch_norm=True).cuda().train()
    assert not layer.fused
    shapes = {k: tuple(v.shape) for k, v in layer.state_dict().items() if "running" not in k and "num_batches" not in k}
    sd = layer.state_dict()
    sd.update({k: v.cuda() for k, v in T.init_state_dict(shapes, seed=int(g["seed"]), dtype=torch.float32).items()})
    layer.load_state_dict(sd)
    mask = torch.from_numpy(g["mask"]).float().cuda()
    assert float(mask.sum(1).min()) == 0.0 and mask.shape == (3, 10, 1)
    x = torch.from_numpy(g["x"]).float().cuda().requires_grad_(True)
    y = layer(x, True, mask)
    (y * torch.from_numpy(g["g"]).float().cuda()).sum().backward()
    assert rel_err(y.detach().cpu().numpy(), g["y"]) < TIGHT
    assert rel_err(x.grad.cpu().numpy(), g["dx"]) < TOL
    unused = [k for k, p in layer.named_parameters() if "grad__" + k not in g]
    assert unused == ["fn.bn.2.weight", "fn.bn.2.bias"]     # (registered for the final linear layer, never run)
    for k, p in layer.named_parameters():
        if k in unused:
            assert p.grad is None, k
        else:
            assert summary_err(k, p.grad, g["grad__" + k]) < TOL, k
    n = 0
    for k, v in layer.state_dict().items():
        if "running" in k or "num_batches" in k:
            assert rel_err(v.double().cpu().numpy(), g["state__" + k]) < TIGHT, k
            n += 1
    assert n == 6 * 3
