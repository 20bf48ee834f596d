"""CPU: what mpg_chain refuses, which of its kernels every accepted shape takes (mpg_chain_route), and which MPLayers the
fused route -- whose node network IS an mpg_chain call -- may be given.

mpg_chain_route makes mpg_chain's own decision and returns before any HIP call (struct fields and pointer values only), so
the codes and the route table are pinned on a machine without a GPU."""
import ctypes

import pytest

PTR = 0x1000   # "any non-null, 16-byte aligned value": never dereferenced on these paths


def _chain(layers, *, f16, K1=None, A2=None, M=64, alpha=0.2, nlayers=None, a_slabs=1, in_thr=0, **top):
    """An ``MpgChain`` block from (K, N, {field: value}) triples; the row strides default to the widths."""
    from mpgan_amd import _lib
    c = _lib.MpgChain()   # ctypes zero-initialises
    c.M, c.nlayers, c.alpha, c.f16, c.a_slabs = M, len(layers) if nlayers is None else nlayers, alpha, int(f16), a_slabs
    K0 = layers[0][0] if layers else 0
    c.A, c.lda, c.K1 = PTR, K0, K0 if K1 is None else K1
    c.A2, c.lda2 = A2, (K0 - c.K1 if A2 else 0)
    c.in_thr = in_thr
    for k, v in top.items():
        setattr(c, k, v)
    for L, (K, N, kw) in zip(c.L, layers):
        L.Wimg, L.K, L.N, L.out, L.ldo = PTR, K, N, PTR, N
        for k, v in kw.items():
            setattr(L, k, v)
    return c


def _route(c):
    from mpgan_amd import _lib
    return _lib.lib().mpg_chain_route(ctypes.byref(c))


# ---- the four shapes an MPLayer(F, [96, 160, 192], fn, out) call runs (ops._fn_fwd_chain, _ac_chain, _fn_grad_chain, _dx_chain)
def fn_forward(F=32, fn=(256, 256), out=32, drop=0, **kw):
    d = dict(drop_thr=drop)
    return _chain([(192 + F, fn[0], dict(bias=PTR, act=1, **d)), (fn[0], fn[1], dict(bias=PTR, act=1, **d)), (fn[1], out, dict(bias=PTR))],
                  f16=True, K1=192, A2=PTR, **kw)


def ac_projection(F=32, **kw):
    return _chain([(F, 192, dict(bias=PTR, nbias=96))], f16=True, **kw)


def fn_gradients(F=32, fn=(256, 256), out=32, thr=0, ldh=None, **kw):
    ldh = ldh or (fn[1], fn[0])
    return _chain([(out, fn[1], dict(gateH=PTR, ldh=ldh[0], gate_act=1, gate_thr=thr)),
                   (fn[1], fn[0], dict(gateH=PTR, ldh=ldh[1], gate_act=1, gate_thr=thr)), (fn[0], 192 + F, {})],
                  f16=False, in_thr=thr, **kw)


def dx_from_da_dc(F=32, **kw):
    return _chain([(192, F, dict(resid=PTR, ldr=F))], f16=False, K1=96, A2=PTR, a_slabs=2, **kw)


DEFAULT_SHAPES = [
    ("fn_forward", fn_forward, {}), ("ac_projection", ac_projection, {}), ("fn_gradients", fn_gradients, {}), ("dx", dx_from_da_dc, {}),
    # F = 3: the input rows are staged element by element; the last layer of the gradient chain and of dx are not whole groups
    ("fn_forward-F3", fn_forward, dict(F=3)), ("ac_projection-F3", ac_projection, dict(F=3)),
    ("fn_gradients-F3", fn_gradients, dict(F=3)), ("dx-F3", dx_from_da_dc, dict(F=3)),
    # out = 5: the SL form (last layer stored element by element)
    ("fn_forward-out5", fn_forward, dict(out=5)), ("fn_gradients-out5", fn_gradients, dict(out=5)),
    # hidden widths 228 / 252 with F = out = 20: the same k-steps (14 / 16 / 16 and 2 / 16 / 16), ragged last tiles in every layer
    ("fn_forward-228-252", fn_forward, dict(F=20, fn=(228, 252), out=20)), ("ac_projection-F20", ac_projection, dict(F=20)),
    ("fn_gradients-228-252", fn_gradients, dict(F=20, fn=(228, 252), out=20)), ("dx-F20", dx_from_da_dc, dict(F=20)),
    # one dropout mode per call, either of them
    ("fn_forward-bit", fn_forward, dict(drop=128)), ("fn_forward-byte", fn_forward, dict(drop=77)),
    ("fn_gradients-bit", fn_gradients, dict(thr=128)), ("fn_gradients-byte", fn_gradients, dict(thr=77)),
]


@pytest.mark.parametrize("name,make,kw", DEFAULT_SHAPES, ids=[n for n, _, _ in DEFAULT_SHAPES])
def test_mplayer_shapes_take_chain2_and_the_straight_line_general_kernel_under_the_switch(name, make, kw, monkeypatch):
    from mpgan_amd import _lib
    monkeypatch.delenv("MPG_CHAIN_GENERAL", raising=False)
    assert _route(make(**kw)) == _lib.CHAIN_ROUTE_CHAIN2
    monkeypatch.setenv("MPG_CHAIN_GENERAL", "1")   # read on every call
    assert _route(make(**kw)) == _lib.CHAIN_ROUTE_STRAIGHT
    monkeypatch.delenv("MPG_CHAIN_GENERAL")
    assert _route(make(**kw)) == _lib.CHAIN_ROUTE_CHAIN2


def _mixed_default():
    c = fn_forward(drop=128)
    c.L[1].drop_thr = 77
    return c


def _mixed_gradients(F, fn, out):
    c = fn_gradients(F=F, fn=fn, out=out, thr=128)
    c.in_thr = 77
    return c


def _gate_unaligned():
    c = fn_gradients()
    c.L[0].gateH = PTR + 4
    return c


LOOPS = [
    # shapes that are none of the table's
    ("f16-first-layer-K256", lambda: fn_forward(F=64, fn=(128, 64), out=64)),
    ("two-layers", lambda: _chain([(224, 256, {}), (256, 32, {})], f16=True, K1=192, A2=PTR)),
    ("two-layers-bf16", lambda: _chain([(32, 256, {}), (256, 224, {})], f16=False)),
    ("gate-ldh-not-4", lambda: fn_gradients(F=6, fn=(250, 131), out=7)),               # ldh = 131 and 250, k-steps 2 / 10 / 16
    ("inner-N-not-4", lambda: fn_forward(F=6, fn=(250, 131), out=7)),                  # k-steps 14 / 16 / 10
    ("mixed-dropout", lambda: _mixed_gradients(64, (128, 64), 64)),
    ("N320-bf16", lambda: _chain([(32, 320, dict(bias=PTR))], f16=False)),
    ("N320-f16-K64", lambda: _chain([(64, 320, dict(bias=PTR))], f16=True)),
    ("ac-projection-K64", lambda: ac_projection(F=64)),
    ("ac-projection-K5-bf16", lambda: _chain([(5, 192, {})], f16=False)),
    ("dx-N64-K192-f16", lambda: _chain([(192, 64, dict(resid=PTR, ldr=64))], f16=True, K1=96, A2=PTR)),
    ("fn-gradients-F64", lambda: fn_gradients(F=64, fn=(128, 64), out=64)),
]
# What takes a shape with the table's k-steps off chain2 one condition at a time: the general kernel selects its instantiation by
# k-steps alone, so these run its straight-line code without the environment switch.
STRAIGHT = [
    ("mixed-dropout", _mixed_default),
    ("mixed-dropout-gradients", lambda: _mixed_gradients(32, (256, 256), 32)),
    ("gate-ldh-not-4", lambda: fn_gradients(ldh=(257, 256))),
    ("gate-not-16-byte-aligned", _gate_unaligned),
    ("inner-N-not-4", lambda: fn_forward(fn=(254, 256))),
    ("inner-ldo-not-4", lambda: _chain([(224, 256, dict(ldo=257)), (256, 256, {}), (256, 32, {})], f16=True, K1=192, A2=PTR)),
    ("N320-f16-K32", lambda: _chain([(32, 320, dict(bias=PTR))], f16=True)),
    ("fn-forward-last-N320", lambda: fn_forward(out=320)),
    ("fn-forward-with-residual", lambda: _chain([(224, 256, {}), (256, 256, {}), (256, 32, dict(resid=PTR, ldr=32))], f16=True, K1=192, A2=PTR)),
    ("fn-gradients-one-gate", lambda: _chain([(32, 256, dict(gateH=PTR, ldh=256)), (256, 256, {}), (256, 224, {})], f16=False)),
    ("ac-projection-with-dropout", lambda: _chain([(32, 192, dict(drop_thr=128))], f16=True)),
    ("ac-projection-N-not-4", lambda: _chain([(32, 190, {})], f16=True)),
    ("dx-without-residual", lambda: _chain([(192, 32, {})], f16=False, K1=96, A2=PTR)),
    ("out-of-buffer-offsets", lambda: fn_forward(M=3000000)),                           # M * ldo * 4 beyond 2^31
]


@pytest.mark.parametrize("name,make", LOOPS, ids=[n for n, _ in LOOPS])
def test_other_shapes_take_the_run_time_loops(name, make, monkeypatch):
    from mpgan_amd import _lib
    monkeypatch.delenv("MPG_CHAIN_GENERAL", raising=False)
    assert _route(make()) == _lib.CHAIN_ROUTE_LOOPS
    monkeypatch.setenv("MPG_CHAIN_GENERAL", "1")
    assert _route(make()) == _lib.CHAIN_ROUTE_LOOPS


@pytest.mark.parametrize("name,make", STRAIGHT, ids=[n for n, _ in STRAIGHT])
def test_table_k_steps_off_chain2_take_the_straight_line_general_kernel(name, make, monkeypatch):
    from mpgan_amd import _lib
    monkeypatch.delenv("MPG_CHAIN_GENERAL", raising=False)
    assert _route(make()) == _lib.CHAIN_ROUTE_STRAIGHT


def _one(K, N, **kw):
    return _chain([(K, N, {})], f16=True, **kw)


REFUSALS = [
    ("M=0", lambda: _one(32, 192, M=0), -1),
    ("M<0", lambda: _one(32, 192, M=-5), -1),
    ("nlayers=0", lambda: _one(32, 192, nlayers=0), -1),
    ("nlayers=4", lambda: _one(32, 192, nlayers=4), -1),
    ("alpha=1.5", lambda: _one(32, 192, alpha=1.5), -4),
    ("alpha<0", lambda: _one(32, 192, alpha=-0.1), -4),
    ("alpha=nan", lambda: _one(32, 192, alpha=float("nan")), -4),
    ("K=0", lambda: _one(0, 192), -2),
    ("K=257", lambda: _one(257, 192), -2),
    ("N=0", lambda: _one(32, 0), -2),
    ("inner-N=257", lambda: _chain([(32, 257, {}), (257, 32, {})], f16=True), -2),
    ("second-K=257-alone", lambda: _chain([(32, 256, {}), (257, 32, {})], f16=True), -2),
    ("L1.K!=L0.N", lambda: _chain([(32, 256, {}), (128, 32, {})], f16=True), -2),
    ("L2.K!=L1.N", lambda: _chain([(32, 256, {}), (256, 256, {}), (255, 32, {})], f16=False), -2),
    ("K1>K", lambda: _one(32, 192, K1=33), -2),
    ("K1<K-without-A2", lambda: _one(32, 192, K1=31), -2),
    ("a_slabs=0", lambda: _one(32, 192, a_slabs=0), -2),
    ("M=0-and-alpha", lambda: _one(32, 192, M=0, alpha=1.5), -1),           # two faults at once: the order of the checks
    ("alpha-and-K", lambda: _one(257, 192, alpha=1.5), -4),
    ("MPLayer-F128-V1", lambda: fn_forward(F=128), -2),                      # the shapes MPLayer.fused now keeps away from the chain
    ("MPLayer-fn512", lambda: fn_forward(fn=(512, 256)), -2),
    ("MPLayer-fn300", lambda: fn_forward(fn=(256, 300)), -2),
    ("MPLayer-out300-gradients", lambda: fn_gradients(out=300), -2),
]
ACCEPTED = [
    ("last-N=320", lambda: _one(32, 320)),
    ("last-N=320-of-three", lambda: fn_forward(out=320)),
    ("K=256", lambda: _one(256, 192)),
    ("K=1", lambda: _one(1, 1)),
    ("inner-N=256", lambda: _chain([(32, 256, {}), (256, 32, {})], f16=True)),
    ("K1<K-with-A2", lambda: _one(32, 192, K1=31, A2=PTR)),
    ("K1=0-with-A2", lambda: _one(32, 192, K1=0, A2=PTR)),
    ("alpha=0", lambda: _one(32, 192, alpha=0.0)),
    ("alpha=1", lambda: _one(32, 192, alpha=1.0)),
]


@pytest.mark.parametrize("general", [False, True], ids=["table", "MPG_CHAIN_GENERAL"])
@pytest.mark.parametrize("name,make,code", REFUSALS, ids=[n for n, _, _ in REFUSALS])
def test_chain_refusal_codes(name, make, code, general, monkeypatch):
    """mpg_chain_route's answer, and mpg_chain's own for the same block (a refusal returns before the first HIP call)."""
    from mpgan_amd import _lib
    if general:
        monkeypatch.setenv("MPG_CHAIN_GENERAL", "1")
    else:
        monkeypatch.delenv("MPG_CHAIN_GENERAL", raising=False)
    assert _route(make()) == code
    assert _lib.lib().mpg_chain(ctypes.byref(make()), None) == code


@pytest.mark.parametrize("name,make", ACCEPTED, ids=[n for n, _ in ACCEPTED])
def test_chain_accepts_the_borders(name, make, monkeypatch):
    from mpgan_amd import _lib
    monkeypatch.delenv("MPG_CHAIN_GENERAL", raising=False)
    assert _route(make()) in (_lib.CHAIN_ROUTE_CHAIN2, _lib.CHAIN_ROUTE_STRAIGHT, _lib.CHAIN_ROUTE_LOOPS)


def test_route_constants_match_the_header():
    import os
    import re
    from mpgan_amd import _lib, ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "mpgan_amd.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"^#define\s+MPG_CHAIN_ROUTE_(\w+)\s+(\d+)\s*$", txt, flags=re.M)}
    assert defs == dict(CHAIN2=_lib.CHAIN_ROUTE_CHAIN2, STRAIGHT=_lib.CHAIN_ROUTE_STRAIGHT, LOOPS=_lib.CHAIN_ROUTE_LOOPS)
    src = open(os.path.join(root, "mpgan_amd", "csrc", "chain.hip")).read()
    assert int(re.search(r"constexpr int CH_MAXKS = (\d+);", src).group(1)) * 16 == ops.CHAIN_MAX_K == 256


FE = [96, 160, 192]
FUSED = [(64, [128, 64], 64), (6, [250, 131], 7), (20, [228, 252], 20), (32, [256, 256], 32), (3, [256, 256], 5), (32, [256, 256], 256)]
NOT_FUSED = [(128, [256, 256], 32), (65, [256, 256], 32), (32, [512, 256], 32), (32, [256, 300], 32), (32, [256, 256], 300),
             (32, [257, 256], 32), (32, [256, 256], 257)]


@pytest.mark.parametrize("F,fn,out", FUSED, ids=["F%d-fn%d-%d-out%d" % (F, *fn, out) for F, fn, out in FUSED])
def test_mplayer_is_fused_where_every_chain_input_fits(F, fn, out):
    from mpgan_amd.mpgan import MPLayer
    assert MPLayer(F, FE, fn, out).fused


@pytest.mark.parametrize("F,fn,out", NOT_FUSED, ids=["F%d-fn%d-%d-out%d" % (F, *fn, out) for F, fn, out in NOT_FUSED])
def test_mplayer_is_not_fused_beyond_the_chain_limit(F, fn, out):
    """mpg_chain refuses a layer input beyond 256 columns (-2): such a node network takes the un-fused route."""
    from mpgan_amd.mpgan import MPLayer
    assert not MPLayer(F, FE, fn, out).fused


def test_conditioning_columns_count_towards_the_first_layer_input():
    from mpgan_amd.mpgan import MPLayer
    assert MPLayer(62, FE, [256, 256], 32, clabels=1, mask_fne_np=True).fused         # 192 + 62 + 2 = 256
    assert MPLayer(63, FE, [256, 256], 32, clabels=1).fused                            # 192 + 63 + 1 = 256
    assert not MPLayer(63, FE, [256, 256], 32, clabels=1, mask_fne_np=True).fused      # 257
    assert not MPLayer(64, FE, [256, 256], 32, mask_fne_np=True).fused                 # 257


def test_every_chain_of_a_fused_mplayer_is_accepted():
    """The four descriptors of the fused widths above pass mpg_chain's checks: what ``fused`` promises."""
    for F, fn, out in FUSED:
        for c in (fn_forward(F, tuple(fn), out), ac_projection(F), fn_gradients(F, tuple(fn), out), dx_from_da_dc(F)):
            assert _route(c) > 0, (F, fn, out)
