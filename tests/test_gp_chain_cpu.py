"""CPU: the gradient penalty's LinearNets and discriminator head as twice-differentiable ops (``ops.OPTIONS["gp_chain"]``) -- the
plain-torch forms of ``ops.LinearNetFn`` and ``ops.DiscHeadDDFn`` in fp64 against autograd's own double backward of the reference
composition, the host-only route predicates, and the switch's plumbing."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from mpgan_amd import ops
from gp_chain_ref import ALPHA, make_net, pre_activations, net_derivatives, make_head, head_derivatives

BAR = 1e-10   # the bar of test_gp_rows_cpu.py / test_gp_attn_cpu.py: fp64 against fp64, the same formulas in another order


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


# ------------------------------------------------------------------------------------------------ LinearNetFn
def _net_op(c, final_linear):
    return lambda A, A2, W, b, r: ops.linear_net_dd(A, A2, W, b, final_linear=final_linear, alpha=ALPHA, p_drop=0.0, training=True, resid=r,
                                                    keeps=c["keeps"], param_grads=True)


def _head_op(mean, sigmoid, keep):
    return lambda y, m, w, b: ops.DiscHeadDDFn.apply(y, m, w, b, ops.DiscHeadDDSettings(mean, sigmoid, 0.0, True, keep, True))


NETS = [([7, 5], 6), ([9, 12, 10, 4], 11), ([6, 8, 8, 8, 5], 9)]   # 1, 3 and 4 layers (the last: two consecutive ops)


@pytest.mark.parametrize("widths,M", NETS)
@pytest.mark.parametrize("final_linear", [True, False])
@pytest.mark.parametrize("form", ["plain", "two_part", "resid", "dropout"])
def test_linear_net_rule_against_autograd_in_fp64(widths, M, final_linear, form):
    """Value, every first-order output and every second-order output, random u: 1, 3 and 4 layers, with and without ``final_linear``,
    the two-part input, the residual form, and keep-and-scale masks.  dPhi/dX_0 and dPhi/db are zero: the op answers None."""
    c = make_net(widths, M, 100 * len(widths) + M, two=3 if form == "two_part" else 0, resid=form == "resid", p=0.5 if form == "dropout" else 0.0)
    got, ref = net_derivatives(c, final_linear, _net_op(c, final_linear)), net_derivatives(c, final_linear)
    assert got[0].dtype == torch.float64 and rel(got[0], ref[0]) <= BAR
    assert len(got[1]) == len(ref[1])
    for i, (a, b) in enumerate(zip(got[1], ref[1])):
        assert a.shape == b.shape and rel(a, b) <= BAR, ("first", i, rel(a, b))
    L = len(widths) - 1
    for i, (a, b) in enumerate(zip(got[2], ref[2])):
        if i <= L:                                  # dPhi/dgo, dPhi/dW_l
            assert a.shape == b.shape and rel(a, b) <= BAR, ("second", i, rel(a, b))
        else:                                       # dPhi/db_l, dPhi/dx: zero (autograd gives None or exact zeros)
            assert a is None or float(a.abs().max()) == 0.0, ("second", i)
            assert b is None or float(b.abs().max()) <= 1e-12, ("second, reference", i)


def test_linear_net_kinks_are_clear_of_zero():
    """The comparison above is between two piecewise-linear functions: no pre-activation of its cases sits on the kink."""
    for widths, M in NETS:
        for z in pre_activations(make_net(widths, M, 100 * len(widths) + M), False):
            assert float(z.abs().min()) > 1e-9


def _first_of_net():
    c = make_net([9, 12, 10, 4], 11, 5)
    x, go = c["x"].clone().requires_grad_(True), c["go"].clone().requires_grad_(True)
    W, b = [w.clone().requires_grad_(True) for w in c["W"]], [v.clone().requires_grad_(True) for v in c["b"]]
    y = ops.linear_net_dd(x, None, W, b, final_linear=True, alpha=ALPHA, p_drop=0.0, training=True, param_grads=True)
    return c, x, go, W, torch.autograd.grad(y, [x] + W, go, create_graph=True)


def test_linear_net_third_derivative_raises():
    c, x, go, W, first = _first_of_net()
    (second,) = torch.autograd.grad((first[0] * c["u"]).sum(), W[1], create_graph=True)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(second.sum(), go)


def test_linear_net_cotangent_on_a_parameter_gradient_raises():
    c, x, go, W, first = _first_of_net()
    with pytest.raises(RuntimeError, match="parameter-gradient"):
        torch.autograd.grad(first[1].sum(), go)


def test_linear_net_first_derivative_with_create_graph_forms_no_parameter_gradients():
    """``param_grads=False`` (what the models pass): the penalty's first derivative is taken with respect to the input alone."""
    c = make_net([9, 12, 4], 7, 3)
    x = c["x"].clone().requires_grad_(True)
    W, b = [w.clone().requires_grad_(True) for w in c["W"]], [v.clone().requires_grad_(True) for v in c["b"]]
    y = ops.linear_net_dd(x, None, W, b, final_linear=True, alpha=ALPHA, p_drop=0.0, training=True)
    xbar, wbar = torch.autograd.grad(y, [x, W[0]], c["go"], create_graph=True, allow_unused=True)
    assert wbar is None and xbar is not None
    assert torch.autograd.grad((xbar ** 2).sum(), W[0])[0].abs().max() > 0    # the penalty's own backward has them


# ------------------------------------------------------------------------------------------------ DiscHeadDDFn
@pytest.mark.parametrize("mean", [False, True])
@pytest.mark.parametrize("sigmoid", [False, True])
@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("use", [("U", "mu"), ("U",), ("mu",)])
def test_head_rule_against_autograd_in_fp64(mean, sigmoid, drop, use):
    """Value, y_bar / w_bar / b_bar / m_bar and the five second-order outputs with random U and mu: sum and mean pooling, with and
    without the sigmoid (its phi'' term) and the output dropout, a mask with exact zeros and a jet with a single real particle;
    once with both cotangents and once with each alone (``None`` reaches the op)."""
    c = make_head(3, 6, 5, 17)
    keep = c["keep"] if drop else None
    got, ref = head_derivatives(c, mean, sigmoid, keep, _head_op(mean, sigmoid, keep), use), head_derivatives(c, mean, sigmoid, keep, None, use)
    assert got[0].dtype == torch.float64 and rel(got[0], ref[0]) <= BAR
    for n, a, b in zip(("y", "w", "b", "m"), got[1], ref[1]):
        assert a.shape == b.shape and rel(a, b) <= BAR, ("first", n, rel(a, b))
    for n, a, b in zip(("g", "y", "w", "b", "m"), got[2], ref[2]):
        if b is None or float(b.abs().max()) == 0.0:
            assert a is None or float(a.abs().max()) <= 1e-12, ("second", n)
        else:
            assert a.shape == b.shape and rel(a, b) <= BAR, ("second", n, rel(a, b))


@pytest.mark.parametrize("mean", [False, True])
def test_head_without_mask_and_single_particle_form(mean):
    """GAPT_D's form: N = 1, no mask, sigmoid."""
    c = make_head(4, 1, 8, 23, mask=False)
    got, ref = head_derivatives(c, mean, True, None, _head_op(mean, True, None)), head_derivatives(c, mean, True, None)
    assert rel(got[0], ref[0]) <= BAR
    for a, b in zip(got[1] + got[2], ref[1] + ref[2]):
        assert a.shape == b.shape and rel(a, b) <= BAR


def test_head_third_derivative_and_parameter_gradient_cotangent_raise():
    c = make_head(3, 6, 5, 17)
    y, w, b, g = (c[n].clone().requires_grad_(True) for n in ("y", "w", "b", "g"))
    m = c["mask"].clone().requires_grad_(True)
    out = ops.DiscHeadDDFn.apply(y, m, w, b, ops.DiscHeadDDSettings(True, True, 0.0, True, None, True))
    first = torch.autograd.grad(out, [y, w], g, create_graph=True)
    with pytest.raises(RuntimeError, match="parameter-gradient"):
        torch.autograd.grad(first[1].sum(), g)
    out = ops.DiscHeadDDFn.apply(y, m, w, b, ops.DiscHeadDDSettings(True, True, 0.0, True, None, True))
    first = torch.autograd.grad(out, [y], g, create_graph=True)
    (second,) = torch.autograd.grad((first[0] * c["U"]).sum(), w, create_graph=True)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(second.sum(), g)


# ------------------------------------------------------------------------------------------------ routes, switch, C ABI
def test_gp_chain_route_over_a_grid():
    on, off = dict(ops.OPTIONS, gp_chain=True), dict(ops.OPTIONS, gp_chain=False)
    assert not ops.OPTIONS["gp_chain"] or "MPG_GP_CHAIN" in os.environ   # off unless asked for
    shapes = ([195, 256, 256, 32], [224, 256, 256, 32], [32, 32], [35, 40, 7], [6, 8, 8, 8, 5], [3, 1])
    for widths in shapes:
        for final_linear in (True, False):
            assert ops.gp_chain_route(widths, final_linear, False, False, True, options=on), widths
            assert not ops.gp_chain_route(widths, final_linear, False, False, True, options=off)
            assert not ops.gp_chain_route(widths, final_linear, False, False, False, options=on)     # outside double_backward_route
            assert not ops.gp_chain_route(widths, final_linear, True, False, True, options=on)      # batch norm
            assert not ops.gp_chain_route(widths, final_linear, False, True, True, options=on)      # spectral norm
    # widths beyond mpg_chain's limits: an input, a hidden or an output width above CHAIN_MAX_K (the input-gradient chain has the
    # output as its first K), also inside the second op of a split net
    for widths in ([257, 32], [32, 257, 8], [32, 257], [8, 8, 8, 8, 300, 4], [8, 8, 8, 8, 300]):
        assert not ops.gp_chain_route(widths, True, False, False, True, options=on), widths
    assert ops.gp_chain_route([256, 256, 256, 256], True, False, False, True, options=on)
    assert ops.gp_chain_pieces(1) == [(0, 1)] and ops.gp_chain_pieces(3) == [(0, 3)] and ops.gp_chain_pieces(4) == [(0, 3), (3, 4)]
    assert ops.gp_head_route(30, True, on) and ops.gp_head_route(1, True, on) and not ops.gp_head_route(30, True, off)
    assert not ops.gp_head_route(30, False, on) and not ops.gp_head_route(ops.DD_HEAD_MAX_N + 1, True, on)


def test_models_follow_the_route():
    from mpgan_amd import train
    from mpgan_amd.mpgan import LinearNet
    on = dict(ops.OPTIONS, gp_chain=True)
    _, D = train.default_mpgan(30, device="cpu")
    assert all(l.fn.gp_chain_ok(True, on) and l.fe.gp_chain_ok(True, on) for l in D.mp_layers) and D.fnd_layer.gp_chain_ok(True, on)
    assert not any(l.fn.gp_chain_ok(True, dict(ops.OPTIONS, gp_chain=False)) for l in D.mp_layers)
    _, Dg = train.default_gapt(30, device="cpu")
    assert Dg.final_fc.gp_chain_ok(True, on) and all(m.ff.gp_chain_ok(True, on) for m in Dg.modules() if hasattr(m, "ff"))
    assert not LinearNet([8, 8], input_size=4, batch_norm=True).gp_chain_ok(True, on)
    assert not LinearNet([8, 8], input_size=4, spectral_norm=True).gp_chain_ok(True, on)
    assert not LinearNet([300, 8], input_size=4).gp_chain_ok(True, on)


def test_train_step_sets_and_restores_the_option():
    """``TrainStep(gp_chain=True).gradient_penalty`` runs D with the option set and puts back what it found, also behind an error."""
    from mpgan_amd import train

    seen = []

    class Probe(torch.nn.Module):
        def forward(self, x):
            seen.append((ops.OPTIONS["gp_chain"], ops.double_backward_on(x.device)))
            return (x ** 2).sum((1, 2)).unsqueeze(1)

    class Fails(torch.nn.Module):
        def forward(self, x):
            seen.append((ops.OPTIONS["gp_chain"], ops.double_backward_on(x.device)))
            raise RuntimeError("no CPU path")

    for flag in (True, False):
        ts = object.__new__(train.TrainStep)     # (the penalty's own attributes: the step's buffers and graphs need a device)
        ts.dev, ts.gp_lambda, ts.fixed_alpha = torch.device("cpu"), 10.0, None
        ts.gp_rows, ts.gp_attn, ts.gp_chain = False, False, flag
        for before in (False, True):
            prev, ops.OPTIONS["gp_chain"] = ops.OPTIONS["gp_chain"], before
            try:
                ts.D = Probe()
                gp = ts.gradient_penalty(torch.randn(2, 5, 4), torch.randn(2, 5, 4))
                assert seen[-1] == (flag, True) and ops.OPTIONS["gp_chain"] is before and float(gp.detach()) > 0
                ts.D = Fails()
                with pytest.raises(RuntimeError):
                    ts.gradient_penalty(torch.randn(2, 5, 4), torch.randn(2, 5, 4))
                assert seen[-1] == (flag, True) and ops.OPTIONS["gp_chain"] is before
            finally:
                ops.OPTIONS["gp_chain"] = prev
    import inspect
    assert inspect.signature(train.TrainStep.__init__).parameters["gp_chain"].default is None


def test_struct_layout_matches_the_header():
    """``sizeof(MpgDiscHeadDD)`` and every field's offset as gcc sees the header equal the ctypes mirror's; ``MpgDiscHead`` has not
    grown."""
    import subprocess
    import tempfile
    from mpgan_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fields = [n for n, _ in _lib.MpgDiscHeadDD._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "mpgan_amd.h"\nint main(){printf("%zu %zu\\n", sizeof(MpgDiscHeadDD), sizeof(MpgDiscHead));'
           + "".join(f'printf("%zu\\n", offsetof(MpgDiscHeadDD, {n}));' for n in fields) + "return 0;}")
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(root, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")], check=True)
        out = subprocess.run([os.path.join(d, "t")], check=True, capture_output=True, text=True).stdout.split()
    assert int(out[0]) == C.sizeof(_lib.MpgDiscHeadDD) and int(out[1]) == C.sizeof(_lib.MpgDiscHead)
    assert [int(v) for v in out[2:]] == [getattr(_lib.MpgDiscHeadDD, n).offset for n in fields]


def _dd_struct():
    from mpgan_amd import _lib
    buf = (C.c_char * 64)()
    p = C.cast(buf, C.c_void_p)
    h = _lib.MpgDiscHeadDD()
    h.y, h.ldy, h.w, h.g, h.mask = p, 8, p, p, p
    h.B, h.N, h.F, h.mode = 2, 4, 8, 1
    return h, buf


@pytest.mark.parametrize("over, code", [({"N": 0}, -1), ({"N": 1025}, -1), ({"mode": 2}, -1), ({"y": None}, -2), ({"g": None}, -2),
                                        ({"gw": 1, "part": None}, -2), ({"gm": 1, "mask": None}, -2), ({"thr": 128, "seed": None}, -2),
                                        ({"ldy": 7}, -5), ({"gy": 1, "ld_gy": 4}, -5), ({"U": 1, "ldu": 3}, -5)])
def test_mpg_disc_head_dd_declines_before_any_launch(over, code):
    from mpgan_amd import _lib
    h, keep = _dd_struct()
    for n, val in over.items():
        setattr(h, n, C.cast(keep, C.c_void_p) if val == 1 else val)
    assert _lib.lib().mpg_disc_head_dd(C.byref(h), None) == code


@pytest.mark.parametrize("F, seed", [(8, 15), (35, 42)])
def test_head_one_particle_mean_against_60_digits(F, seed):
    """N = 1 under the mean with a mask: m_bar, dPhi/dm and dPhi/dy are 1e-12 of the terms they are the difference of, and autograd's
    own fp64 double backward of the composition keeps three to four digits of them there (1.6e-3 off on dPhi/dm of jet 1 at F = 35,
    keep 2, measured against this test's 60-digit value).  The plain-torch form of the op, which sums pairwise terms as the kernel
    does, is held to 1e-10 against the 60-digit derivatives of the composition (mpmath; inputs rounded to fp32-exact values as
    tests/test_gpu_gp_chain.py uses them)."""
    import mpmath as mp
    c = {k: (v.float().double() if torch.is_tensor(v) else v) for k, v in make_head(3, 1, F, seed).items()}
    keep = torch.tensor([0.0, 2.0, 1.0], dtype=torch.float64)
    got = head_derivatives(c, True, True, keep, _head_op(True, True, keep))
    auto = head_derivatives(c, True, True, keep, None)
    with mp.workdps(60):
        f = lambda v: mp.mpf(float(v))
        for b in range(3):
            w = [f(v) for v in c["w"].reshape(-1)]
            t0 = sum(p * q for p, q in zip((f(v) for v in c["y"][b, 0]), w))
            a = sum(p * q for p, q in zip((f(v) for v in c["U"][b, 0]), w))
            mu, m0, g, bias, k = f(c["mu"][b, 0, 0]), f(c["mask"][b, 0, 0]), f(c["g"][b]), f(c["b"][0]), f(keep[b])
            out = lambda m, t: 1 / (1 + mp.exp(-k * (m * t / (m + mp.mpf(1e-12)) + bias)))
            mbar = lambda m, t: g * mp.diff(lambda q: out(q, t), m)
            phi = lambda m, t: g * a * mp.diff(lambda q: out(m, q), t) + mu * mbar(m, t)    # <U, y_bar> + mu m_bar, y_bar = g dout/dt w
            want = {"m_bar": mbar(m0, t0), "dPhi/dm": mp.diff(lambda q: phi(q, t0), m0), "dPhi/dt": mp.diff(lambda q: phi(m0, q), t0)}
            have = {"m_bar": got[1][3][b, 0, 0], "dPhi/dm": got[2][4][b, 0, 0], "dPhi/dt": got[2][1][b, 0, 0] / c["w"][0, 0]}
            for n in want:
                if want[n] == 0:
                    assert float(have[n]) == 0.0, (b, n)
                else:
                    assert abs(f(have[n]) / want[n] - 1) < 1e-10, (b, n, float(have[n]), mp.nstr(want[n], 15))
    print("autograd fp64 against the op, dPhi/dm:", rel(auto[2][4], got[2][4]), "m_bar:", rel(auto[1][3], got[1][3]))
