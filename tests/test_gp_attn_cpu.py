"""CPU: the host side of the gradient penalty's attention route (``ops.OPTIONS["gp_attn"]``): the second-order rule of
``ops.AttnCoreFn`` / ``ops.AttnCoreVJPFn`` in fp64 against torch autograd's own double backward through the plain statement of the
attention core, the declined third derivative, the routing predicate and the layout of ``MpgAttnDD``."""
import ctypes as C

import numpy as np
import pytest
import torch

from mpgan_amd import _lib, ops
from test_gpu_attn import _ref

BAR = 1e-10   # the bar of test_gp_rows_cpu.py: fp64 against fp64, the same formulas in another order


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def make_inputs(B, L, S, H, d, masked=True, dtype=torch.float64, ignored_tile=False, dead0=True):
    """q, k, v, d_o, uq, uk, uv [rows, E] and the key mask [B * S] (1 = ignore): each key ignored with p = 0.3, every jet with at
    least one real key -- except jet 0, which has none (``dead0``); ``ignored_tile``: keys 0-31 of the last jet all ignored."""
    rs = np.random.RandomState(1000 * B + 100 * L + 10 * S + H + d)
    E = H * d
    mk = lambda n: torch.from_numpy(rs.normal(size=(n, E))).to(dtype)
    t = dict(q=mk(B * L), k=mk(B * S), v=mk(B * S), go=mk(B * L), uq=mk(B * L), uk=mk(B * S), uv=mk(B * S))
    ignore = None
    if masked:
        ig = (rs.uniform(size=(B, S)) < 0.3).astype(np.float64)
        ig[:, S - 1] = 0
        if ignored_tile and S > 32:
            ig[B - 1, :32] = 1
        if dead0:
            ig[0] = 1
        ignore = torch.from_numpy(ig.reshape(-1)).to(dtype)
    return t, ignore


def derivatives(f, t, use=("uq", "uk", "uv"), packed=False):
    """(o, [dq, dk, dv], [dPhi/dq, dPhi/dk, dPhi/dv, dPhi/dG]) of o = f(q, k, v) with G = t["go"] and Phi = sum over ``use`` of <u, d.>;
    ``packed``: q, k, v reach f as column slices of one [rows, 3E] tensor (L = S)."""
    q, k, v, go = (t[n].clone().requires_grad_(True) for n in ("q", "k", "v", "go"))
    if packed:
        E = q.shape[1]
        qkv = torch.cat((t["q"], t["k"], t["v"]), 1).requires_grad_(True)
        q, k, v = qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:]
    o = f(q, k, v)
    first = torch.autograd.grad(o, (q, k, v), go, create_graph=True)
    phi = sum((first[i] * t[n]).sum() for i, n in enumerate(("uq", "uk", "uv")) if n in use)
    second = torch.autograd.grad(phi, (q, k, v, go))
    return o.detach(), [x.detach() for x in first], list(second)


SHAPES = [(3, 30, 30, 4, 16), (2, 1, 30, 4, 16), (2, 10, 33, 2, 8), (2, 33, 10, 4, 16)]


@pytest.mark.parametrize("B,L,S,H,d", SHAPES)
@pytest.mark.parametrize("use", [("uq", "uk", "uv"), ("uk", "uv")])
def test_second_order_rule_against_autograd_in_fp64(B, L, S, H, d, use):
    """Value, dq / dk / dv and the four second-order outputs, with a key mask that holds a jet without a real key; once with all
    three cotangents and once with uq absent (``None`` reaches the op: nothing of Phi hangs on dq)."""
    t, ignore = make_inputs(B, L, S, H, d)
    got = derivatives(lambda q, k, v: ops.AttnCoreFn.apply(q, k, v, ignore, B, L, S, H), t, use)
    ref = derivatives(lambda q, k, v: _ref(q, k, v, ignore, B, L, S, H), t, use)
    assert got[0].dtype == torch.float64 and rel(got[0], ref[0]) <= BAR
    for n, a, b in zip(("dq", "dk", "dv"), got[1], ref[1]):
        assert a.shape == b.shape and rel(a, b) <= BAR, ("first", n, rel(a, b))
    for n, a, b in zip(("q", "k", "v", "G"), got[2], ref[2]):
        assert a.shape == b.shape and rel(a, b) <= BAR, ("second", n, rel(a, b))
        assert float(a.reshape(B, -1)[0].abs().max()) == 0.0, ("the jet without a real key", n)


def test_third_derivative_raises():
    B, L, S, H, d = 2, 5, 7, 2, 8
    t, ignore = make_inputs(B, L, S, H, d)
    q, k, v, go = (t[n].clone().requires_grad_(True) for n in ("q", "k", "v", "go"))
    o = ops.AttnCoreFn.apply(q, k, v, ignore, B, L, S, H)
    first = torch.autograd.grad(o, (q, k, v), go, create_graph=True)
    (second,) = torch.autograd.grad((first[1] * t["uk"]).sum(), q, create_graph=True)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(second.sum(), k)


def test_gp_attn_route_follows_the_switch_and_the_kernels_shapes():
    on, off = dict(ops.OPTIONS, gp_attn=True), dict(ops.OPTIONS, gp_attn=False)
    assert not ops.OPTIONS["gp_attn"] or "MPG_GP_ATTN" in __import__("os").environ   # off unless asked for
    assert not ops.gp_attn_route(64, 4, 30, 30, double_backward=True, options=off)
    assert not ops.gp_attn_route(64, 4, 30, 30, double_backward=False, options=on)   # outside double_backward_route
    assert not ops.gp_attn_route(48, 4, 30, 30, double_backward=True, options=on)    # d = 12
    assert not ops.gp_attn_route(64, 4, 30, 161, double_backward=True, options=on)
    assert not ops.gp_attn_route(64, 4, 161, 30, double_backward=True, options=on)
    assert not ops.gp_attn_route(64, 4, 0, 30, double_backward=True, options=on)
    for N in (30, 150):   # the reference's GAPT defaults: SAB, PMA with one seed, ISAB with 10 inducing points on either side
        for L, S in ((N, N), (1, N), (10, N), (N, 10)):
            assert ops.gp_attn_route(64, 4, L, S, double_backward=True, options=on), (L, S)
    assert ops.gp_attn_route(16, 2, 160, 160, double_backward=True, options=on)      # d = 8
    assert ops.gp_attn_route(96, 3, 17, 5, double_backward=True, options=on)         # d = 32


def test_struct_layout_matches_the_header():
    """``sizeof(MpgAttnDD)`` and every field's offset as gcc sees the header equal the ctypes mirror's; ``MpgAttn`` has not grown."""
    import os
    import subprocess
    import tempfile
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    fields = [f[0] for f in _lib.MpgAttnDD._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "mpgan_amd.h"\nint main(){'
           + "".join(f'printf("{f} %zu\\n", offsetof(MpgAttnDD, {f}));' for f in fields)
           + 'printf("sizeof %zu\\n", sizeof(MpgAttnDD));printf("MpgAttn %zu\\n", sizeof(MpgAttn));return 0;}')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-I", inc, c, "-o", os.path.join(d, "t")], check=True)
        out = subprocess.run([os.path.join(d, "t")], check=True, capture_output=True, text=True).stdout
    got = {k: int(v) for k, v in (line.split() for line in out.strip().splitlines())}
    assert got.pop("sizeof") == C.sizeof(_lib.MpgAttnDD)
    assert got.pop("MpgAttn") == C.sizeof(_lib.MpgAttn)
    assert got == {f: getattr(_lib.MpgAttnDD, f).offset for f in fields}
    assert "mpg_attn_dd" in _lib.SIGNATURES


def _dd_struct(B=2, L=30, S=30, H=4, d=16):
    """A well-formed ``MpgAttnDD`` over host dummies (the checks return before anything is read or launched)."""
    E = H * d
    keep = [torch.zeros(max(B * L, B * S) * E) for _ in range(12)]
    e = _lib.MpgAttnDD()
    for n, buf in zip(("q", "k", "v", "d_o", "uq", "uk", "uv", "P", "gq", "gk", "gv", "gdo"), keep):
        setattr(e, n, C.c_void_p(buf.data_ptr()))
    for n in ("ldq", "ldk", "ldv", "ldo", "lduq", "lduk", "lduv", "ldgq", "ldgk", "ldgv", "ldgdo"):
        setattr(e, n, E)
    e.B, e.L, e.S, e.H, e.d = B, L, S, H, d
    return e, keep


@pytest.mark.parametrize("over, code", [(dict(d=12), -1), (dict(S=161), -1), (dict(L=161), -1), (dict(L=0), -1), (dict(B=0), -1),
                                        (dict(q=None), -2), (dict(P=None), -2), (dict(d_o=None), -2), (dict(lduk=63), -5),
                                        (dict(ldgv=0), -5)])
def test_mpg_attn_dd_declines_before_any_launch(over, code):
    e, keep = _dd_struct()
    for n, val in over.items():
        setattr(e, n, val)
    assert _lib.lib().mpg_attn_dd(C.byref(e), None) == code, over
