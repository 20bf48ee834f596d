"""GPU parity of the node-path entry points on their own: mpg_chain, mpg_pack_many, the grouped weight-gradient
GEMM / reduction -- against plain fp64 torch restatements of LinearNet.forward (mpgan/model.py:70-85) and of
autograd's dX = dY W, dW = dY^T X.  Tolerance: 1e-3 relative (north star), asserted at 1e-4.

mpg_chain has two kernels: the MPLayer shapes' own schedule (chain2.hip) and the general one (chain.hip), which also has
straight-line instantiations for those shapes' k-steps.  The tests of the MPLayer shapes run on both (MPG_CHAIN_GENERAL in the
environment), the ``test_general_*`` ones on shapes only the general kernel takes; every chain test asserts the kernel it ran
(``ops.chain_route``), keeps its outputs inside sentinel frames and measures the ragged last tile of rows and columns apart."""
import numpy as np
import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu
TIGHT = 1e-4


def _dev():
    return torch.device("cuda:0")


def _t(rs, *shape, scale=1.0):
    return torch.from_numpy(rs.normal(size=shape) * scale).float().to(_dev())


def _lrelu(v, a):
    return torch.where(v > 0, v, a * v)


# ---- the frame every chain output of this file lives in, and the metric it is held to ----------------------------------------
SENTINEL = 12345.0
GENERAL = [False, True]   # MPG_CHAIN_GENERAL in the environment (the library reads it on every call)
ROUTE_NAMES = {1: "chain2", 2: "general-straight", 3: "general-loops"}


def _framed(M, N, ld=None):
    """An output [M, N] as a view inside a buffer [M + 1, ld > N] filled with a sentinel: whatever the kernel writes beyond its
    rows or columns shows.  The row stride keeps whole 16-byte groups where N has them (the vector stores, the form chain2 takes)
    and is odd against them otherwise (element-wise stores)."""
    if ld is None:
        ld = N + 4 if N % 4 == 0 else N + 1
    assert ld > N
    buf = torch.full((M + 1, ld), SENTINEL, device=_dev())
    return buf, buf[:M, :N]


def _frame_intact(buf, M, N):
    bits = buf.view(torch.int32)
    s = int(torch.tensor(SENTINEL).view(torch.int32))
    return bool((bits[M:] == s).all()) and bool((bits[:M, N:] == s).all())


def _edge_errs(got, ref):
    """rel_err over the whole tensor, and -- each scaled by the whole tensor's max -- over the last N % 32 columns and the last
    M % 32 rows alone (the ragged tile of either direction): an error confined to an edge cannot hide behind the interior."""
    g, r = got.detach().double().cpu().numpy(), ref.detach().double().cpu().numpy()
    assert g.shape == r.shape
    M, N = r.shape
    den = np.abs(r).max()
    den = den if den > 0 else 1.0
    errs = {"all": rel_err(g, r)}
    if N % 32:
        errs["cols"] = float(np.abs(g[:, N - N % 32:] - r[:, N - N % 32:]).max() / den)
    if M % 32:
        errs["rows"] = float(np.abs(g[M - M % 32:] - r[M - M % 32:]).max() / den)
    return errs


class _Case:
    """One chain call of a test: its route, then per output the frame and the errors; ``done`` records and asserts."""

    def __init__(self, what, c, route=None):
        from mpgan_amd import ops
        self.what, self.route, self.errs, self.broken = what, ops.chain_route(c), {}, []
        if route is not None:
            assert self.route == route, (what, "route", self.route, "expected", route)
        ops.run_chain(c)
        torch.cuda.synchronize()

    def check(self, name, buf, view, ref):
        M, N = view.shape
        if not _frame_intact(buf, M, N):
            self.broken.append(name)
        for k, v in _edge_errs(view, ref).items():
            self.errs[name + "." + k] = v

    def done(self):
        from conftest import record_parity
        worst = max(self.errs, key=self.errs.get)
        edges = [v for k, v in self.errs.items() if not k.endswith(".all")]
        record_parity("chain_case", self.what, route=ROUTE_NAMES.get(self.route, str(self.route)), outputs=len({k.split(".")[0] for k in self.errs}),
                      worst=worst, err=float(self.errs[worst]), edge_err=float(max(edges)) if edges else -1.0,
                      sentinel="intact" if not self.broken else "OVERWRITTEN:" + ",".join(self.broken))
        print(self.what, ROUTE_NAMES.get(self.route), self.errs)
        assert not self.broken, (self.what, "sentinel overwritten around", self.broken)
        bad = {k: v for k, v in self.errs.items() if not v < TIGHT}
        assert not bad, (self.what, bad)


def _switch(monkeypatch, general):
    if general:
        monkeypatch.setenv("MPG_CHAIN_GENERAL", "1")
    else:
        monkeypatch.delenv("MPG_CHAIN_GENERAL", raising=False)


def _both_kernels(cases):
    """Every case on chain2 (its id as it was) and, under the switch, on the general kernel (id + "-general")."""
    ids = ["-".join(str(v) for v in (c if isinstance(c, tuple) else (c,))) for c in cases]
    return [pytest.param(*(c if isinstance(c, tuple) else (c,)), g, id=i + ("-general" if g else "")) for g in GENERAL for c, i in zip(cases, ids)]


def _holder(rs, F, out, n1=256, n2=256, dscale=1.0, f16=True):
    from mpgan_amd import ops
    W = dict(W1=_t(rs, 96, 2 * F, scale=0.2), W2=_t(rs, 160, 96, scale=0.1), W3=_t(rs, 192, 160, scale=0.1),
             V1=_t(rs, n1, 192 + F, scale=0.1), V2=_t(rs, n2, n1, scale=0.1), V3=_t(rs, out, n2, scale=0.1))
    pk = ops.PackedMPLayer(tuple(W.values()), F, out, dscale, f16).ensure()
    return W, pk


def _table_route(general):
    from mpgan_amd import _lib
    return _lib.CHAIN_ROUTE_STRAIGHT if general else _lib.CHAIN_ROUTE_CHAIN2


@pytest.mark.parametrize("M,F,out,slabs,general", _both_kernels([(7680, 32, 32, 1), (100, 3, 32, 2), (37, 32, 5, 1), (1, 3, 3, 3)]))
def test_chain_forward_three_layers(M, F, out, slabs, general, monkeypatch):
    """fn = LinearNet([256,256] -> out) on [sum of agg slabs | x], ragged row counts, odd widths."""
    from mpgan_amd import ops
    _switch(monkeypatch, general)
    rs = np.random.RandomState(M + F + out)
    W, pk = _holder(rs, F, out)
    aggp, x = _t(rs, slabs, M, 192), _t(rs, M, F)
    c1, c2, c3 = _t(rs, 256), _t(rs, 256), _t(rs, out)
    (b1, h1), (b2, h2), (b3, y) = (_framed(M, n) for n in (256, 256, out))
    # (the forward images of a PackedMPLayer hold SC_WN * W, the activations are split as SC_ACT * x: exact
    # power-of-two scales that keep the lo halves of the fp16 pairs normal -- the results must not notice)
    c = ops.chain_struct(M, [dict(img=pk.ptr("V1"), K=192 + F, N=256, bias=c1, act=True, out=h1, wscale=ops.SC_WN),
                             dict(img=pk.ptr("V2"), K=256, N=256, bias=c2, act=True, out=h2, wscale=ops.SC_WN),
                             dict(img=pk.ptr("V3"), K=256, N=out, bias=c3, out=y, wscale=ops.SC_WN)],
                         A=aggp, lda=192, K1=192, A2=x, lda2=F, a_slabs=slabs, a_slab_stride=M * 192, alpha=0.2, f16=True,
                         ascale=ops.SC_ACT)
    case = _Case(("fn_forward", M, F, out, slabs), c, _table_route(general))
    inp = torch.cat([aggp.double().sum(0), x.double()], 1)
    r1 = _lrelu(inp @ W["V1"].double().t() + c1.double(), 0.2)
    r2 = _lrelu(r1 @ W["V2"].double().t() + c2.double(), 0.2)
    r3 = r2 @ W["V3"].double().t() + c3.double()
    for got, ref in ((h1, r1), (h2, r2), (y, r3)):
        assert rel_err(got.cpu().numpy(), ref.cpu().numpy()) < TIGHT
    for name, buf, got, ref in (("h1", b1, h1, r1), ("h2", b2, h2, r2), ("y", b3, y, r3)):
        case.check(name, buf, got, ref)
    case.done()


@pytest.mark.parametrize("p_drop,general", _both_kernels([0.0, 0.5, 0.3]))
def test_chain_gradient_chain_with_gates(p_drop, general, monkeypatch):
    """dz3 = gy * keep3 ; dz2 = (dz3 V3) * phi'(h2) keep2 ; dz1 = (dz2 V2) * phi'(h1) keep1 ; dh0 = dz1 V1 -- the keep
    masks are the kernel's own (mpg_dropout_mask), fed to the fp64 restatement."""
    from mpgan_amd import ops
    _switch(monkeypatch, general)
    rs = np.random.RandomState(11)
    M, F, out = 333, 32, 32
    W, pk = _holder(rs, F, out)
    thr, scale = ops.drop_params(p_drop)
    ops.set_seed(99)
    seed = ops.seed_tensor(_dev())
    gy, h1, h2 = _t(rs, M, out), _t(rs, M, 256), _t(rs, M, 256)
    keep = {s: (ops.dropout_mask(M, n, 40 + s, thr).double() if thr else torch.ones(M, n, device=_dev()).double())
            for s, n in ((0, 256), (1, 256), (2, out))}
    if thr:  # dropped activations are exactly zero in the saved tensors
        h1, h2 = h1 * keep[0].float(), h2 * keep[1].float()
    (b3, dz3), (b2, dz2), (b1, dz1), (b0, dh0) = (_framed(M, n) for n in (out, 256, 256, 192 + F))
    c = ops.chain_struct(M, [dict(img=pk.ptr("V3T"), K=out, N=256, gate=(h2, True, 41, thr, scale), out=dz2),
                             dict(img=pk.ptr("V2T"), K=256, N=256, gate=(h1, True, 40, thr, scale), out=dz1),
                             dict(img=pk.ptr("V1T"), K=256, N=192 + F, out=dh0)],
                         A=gy, lda=out, K1=out, in_gate=(42, thr, scale), in_out=dz3 if thr else None, alpha=0.2, seed_t=seed, f16=False)
    case = _Case(("fn_gradients", M, F, out, p_drop), c, _table_route(general))
    sc = scale if thr else 1.0
    r3 = gy.double() * keep[2] * sc
    slope = lambda h: torch.where(h.double() > 0, torch.ones_like(h.double()), 0.2 * torch.ones_like(h.double()))
    r2 = (r3 @ W["V3"].double()) * slope(h2) * keep[1] * sc
    r1 = (r2 @ W["V2"].double()) * slope(h1) * keep[0] * sc
    r0 = r1 @ W["V1"].double()
    pairs = [(dz2, r2), (dz1, r1), (dh0, r0)] + ([(dz3, r3)] if thr else [])
    for got, ref in pairs:
        assert rel_err(got.cpu().numpy(), ref.cpu().numpy()) < TIGHT
    for name, buf, got, ref in (("dz2", b2, dz2, r2), ("dz1", b1, dz1, r1), ("dh0", b0, dh0, r0)) + ((("dz3", b3, dz3, r3),) if thr else ()):
        case.check(name, buf, got, ref)
    if not thr:
        assert _frame_intact(b3, 0, 0)   # no in_out asked for: nothing of it is written
    case.done()


@pytest.mark.parametrize("F,general", _both_kernels([32, 3]))
def test_stacked_layer1_views(F, general, monkeypatch):
    """fe.net.0 on [x_i ; x_j] split as a_i + c_j: the stacked image gives a | c in one launch, its
    transpose gives dx = [da | dc] [W1a ; W1c] + resid."""
    from mpgan_amd import ops
    _switch(monkeypatch, general)
    rs = np.random.RandomState(5 + F)
    M = 450
    W, pk = _holder(rs, F, 32)
    x, b1 = _t(rs, M, F), _t(rs, 96)
    bac, ac = _framed(M, 192)
    c = ops.chain_struct(M, [dict(img=pk.ptr("W1S"), K=F, N=192, bias=b1, nbias=96, out=ac, wscale=ops.SC_WN)], A=x, lda=F, K1=F,
                         f16=True, ascale=ops.SC_ACT)
    case = _Case(("ac_projection", M, F), c, _table_route(general))
    W1 = W["W1"].double()
    ref = torch.cat([x.double() @ W1[:, :F].t() + b1.double(), x.double() @ W1[:, F:].t()], 1)
    assert rel_err(ac.cpu().numpy(), ref.cpu().numpy()) < TIGHT
    case.check("ac", bac, ac, ref)
    case.done()
    da, dc, resid = _t(rs, 2, M, 96), _t(rs, M, 96), _t(rs, M, 40)[:, 8:8 + F]
    bdx, dx = _framed(M, F)
    c = ops.chain_struct(M, [dict(img=pk.ptr("W1ST"), K=192, N=F, resid=resid, out=dx)], A=da, lda=96, K1=96, a_slabs=2,
                         a_slab_stride=M * 96, A2=dc, lda2=96, f16=False)
    case = _Case(("dx", M, F), c, _table_route(general))
    refx = da.double().sum(0) @ W1[:, :F] + dc.double() @ W1[:, F:] + resid.double()
    assert rel_err(dx.cpu().numpy(), refx.cpu().numpy()) < TIGHT
    case.check("dx", bdx, dx, refx)
    case.done()


# ---- the general kernel (chain.hip) on its own: shapes that are none of chain2's table ----------------------------------------
# One row tile is 32 rows: a single row, a ragged tile, a whole tile + 1 row, two tiles + 1 row.
MS = [1, 31, 33, 65]
PS = [0.0, 0.5, 0.3]   # none / bit mode (thr 128) / byte mode


def _images(Ws, f16):
    """``ops.pack_weights`` images of the matrices a chain applies ([N, K] each); fp16 images hold SC_WN * W as MPLayer's do."""
    from mpgan_amd import ops
    return [ops.pack_weights(W, W.shape[0], W.shape[1], scale=ops.SC_WN if f16 else 1.0, f16=f16) for W in Ws]


def _ptr(img):
    import ctypes
    return ctypes.c_void_p(img.data_ptr())


def _keep(M, N, tag, thr):
    from mpgan_amd import ops
    return ops.dropout_mask(M, N, tag, thr).double() if thr else torch.ones(M, N, device=_dev()).double()


def _forward_case(what, M, K1, F2, widths, drops, route, slabs=2, act_last=False):
    """Linear(+LeakyReLU)(+Dropout) layers of ``widths`` on [sum of ``slabs`` slabs of K1 columns | F2 columns], fp16 images with
    MPLayer's operand scales, every layer with bias and output; ``drops``: (thr, scale) per hidden layer."""
    from mpgan_amd import ops
    rs = np.random.RandomState(1000 * M + K1 + F2 + sum(widths))
    dims = [K1 + F2] + list(widths)
    nl = len(widths)
    Ws = [_t(rs, dims[l + 1], dims[l], scale=0.1) for l in range(nl)]
    bs = [_t(rs, n) for n in widths]
    imgs = _images(Ws, True)
    A, A2 = _t(rs, slabs, M, K1), (_t(rs, M, F2) if F2 else None)
    ops.set_seed(99)
    seed = ops.seed_tensor(_dev())
    drops = list(drops) + [(0, 1.0)] * (nl - len(drops))
    keeps = [_keep(M, widths[l], 50 + l, drops[l][0]) for l in range(nl)]
    frames = [_framed(M, n) for n in widths]
    layers = [dict(img=_ptr(imgs[l]), K=dims[l], N=dims[l + 1], bias=bs[l], act=(l + 1 < nl or act_last), drop=(50 + l,) + tuple(drops[l]),
                   out=frames[l][1], wscale=ops.SC_WN) for l in range(nl)]
    c = ops.chain_struct(M, layers, A=A, lda=K1, K1=K1, A2=A2, lda2=F2, a_slabs=slabs, a_slab_stride=M * K1, alpha=0.2, seed_t=seed,
                         f16=True, ascale=ops.SC_ACT)
    case = _Case(what, c, route)
    r = A.double().sum(0)
    if F2:
        r = torch.cat([r, A2.double()], 1)
    for l in range(nl):
        r = r @ Ws[l].double().t() + bs[l].double()
        if layers[l]["act"]:
            r = _lrelu(r, 0.2)
        r = r * keeps[l] * (drops[l][1] if drops[l][0] else 1.0)
        case.check("y%d" % l, frames[l][0], frames[l][1], r)
    case.done()


def _gradient_case(what, M, dims, p_drop, route):
    """The input-gradient chain of three layers, bf16 images: x0 = gy * keep_in ; x_{l+1} = (x_l T_l^T) * phi'(H_l) keep_l for the two
    gated layers, plain for the last; H_l rows are contiguous (row stride = the layer's width), ``in_out`` receives x0."""
    from mpgan_amd import ops
    rs = np.random.RandomState(1000 * M + sum(dims))
    thr, scale = ops.drop_params(p_drop)
    sc = scale if thr else 1.0
    Ts = [_t(rs, dims[l + 1], dims[l], scale=0.1) for l in range(3)]
    imgs = _images(Ts, False)
    ops.set_seed(99)
    seed = ops.seed_tensor(_dev())
    gy = _t(rs, M, dims[0])
    keeps = [_keep(M, dims[1], 41, thr), _keep(M, dims[2], 40, thr)]
    keep_in = _keep(M, dims[0], 42, thr)
    H = [_t(rs, M, dims[1 + l]) * keeps[l].float() for l in range(2)]   # dropped activations are exactly zero in the saved tensors
    assert H[0].stride(0) == dims[1] and H[1].stride(0) == dims[2]
    fin = _framed(M, dims[0])
    frames = [_framed(M, n) for n in dims[1:]]
    layers = [dict(img=_ptr(imgs[l]), K=dims[l], N=dims[l + 1], out=frames[l][1]) for l in range(3)]
    layers[0]["gate"] = (H[0], True, 41, thr, scale)
    layers[1]["gate"] = (H[1], True, 40, thr, scale)
    c = ops.chain_struct(M, layers, A=gy, lda=dims[0], K1=dims[0], in_gate=(42, thr, scale), in_out=fin[1], alpha=0.2, seed_t=seed, f16=False)
    case = _Case(what, c, route)
    slope = lambda h: torch.where(h.double() > 0, torch.ones_like(h.double()), 0.2 * torch.ones_like(h.double()))
    r = gy.double() * keep_in * sc
    case.check("x0", fin[0], fin[1], r)
    for l in range(3):
        r = r @ Ts[l].double().t()
        if l < 2:
            r = r * slope(H[l]) * keeps[l] * sc
        case.check("x%d" % (l + 1), frames[l][0], frames[l][1], r)
    case.done()


def _loops():
    from mpgan_amd import _lib
    return _lib.CHAIN_ROUTE_LOOPS


def _drops(p):
    from mpgan_amd import ops
    return [ops.drop_params(p)] * 2


@pytest.mark.parametrize("p_drop", PS)
@pytest.mark.parametrize("M", MS)
def test_general_forward_three_layers(M, p_drop):
    """fn of MPLayer(64, .., [128, 64], 64): K = 192 + 64 = 256 (two slabs of 192 | 64 columns) -> 128 -> 64 -> 64, fp16."""
    _forward_case(("general_forward", M, p_drop), M, 192, 64, (128, 64, 64), _drops(p_drop), _loops(), act_last=True)


@pytest.mark.parametrize("p_drop", PS)
@pytest.mark.parametrize("M", MS)
def test_general_gradient_chain(M, p_drop):
    """Its input-gradient chain: 64 -> 64 -> 128 -> 256, bf16, gates on layers 0 and 1, the trailing dropout's gate on the input."""
    _gradient_case(("general_gradients", M, p_drop), M, [64, 64, 128, 256], p_drop, _loops())


@pytest.mark.parametrize("p_drop", PS)
@pytest.mark.parametrize("M", MS)
def test_general_forward_widths_not_multiples_of_four(M, p_drop):
    """198 -> 250 -> 131 -> 7 (MPLayer(6, .., [250, 131], 7)): A2 of 6 columns is staged element by element, so are the stores."""
    _forward_case(("general_forward_ragged", M, p_drop), M, 192, 6, (250, 131, 7), _drops(p_drop), _loops())


@pytest.mark.parametrize("p_drop", PS)
@pytest.mark.parametrize("M", MS)
def test_general_gradient_chain_widths_not_multiples_of_four(M, p_drop):
    """7 -> 131 -> 250 -> 198 with gate operands of row stride 131 and 250: the element-wise gate loads and stores."""
    _gradient_case(("general_gradients_ragged", M, p_drop), M, [7, 131, 250, 198], p_drop, _loops())


@pytest.mark.parametrize("M", MS)
def test_general_mixed_dropout_modes_at_the_default_widths(M):
    """224 -> 256 -> 256 -> 32 with bit-mode dropout behind layer 0 and byte-mode dropout behind layer 1: chain2 has one mode per
    call, so these widths reach the general kernel -- its straight-line instantiation -- without the environment switch."""
    from mpgan_amd import _lib, ops
    _forward_case(("general_mixed_dropout", M), M, 192, 32, (256, 256, 32), [ops.drop_params(0.5), ops.drop_params(0.3)],
                  _lib.CHAIN_ROUTE_STRAIGHT, slabs=1)


@pytest.mark.parametrize("K,general", [(64, False), (5, False), (5, True)], ids=["K64", "K5", "K5-general"])
@pytest.mark.parametrize("M", MS)
def test_one_layer_ac_projection_at_other_widths(M, K, general, monkeypatch):
    """a | c = x [W1a ; W1c]^T (+ b1 on the a half: nbias = 96) at F = 64 -- the general kernel's run-time loops -- and at F = 5,
    one of the table's k-steps: chain2, and the general kernel's straight-line form under the switch."""
    from mpgan_amd import ops
    _switch(monkeypatch, general)
    rs = np.random.RandomState(100 * M + K)
    S, b1, x = _t(rs, 192, K, scale=0.2), _t(rs, 96), _t(rs, M, K)
    (img,) = _images([S], True)
    bac, ac = _framed(M, 192)
    c = ops.chain_struct(M, [dict(img=_ptr(img), K=K, N=192, bias=b1, nbias=96, out=ac, wscale=ops.SC_WN)], A=x, lda=K, K1=K,
                         f16=True, ascale=ops.SC_ACT)
    case = _Case(("ac_projection", M, K, general), c, _loops() if K == 64 else _table_route(general))
    ref = x.double() @ S.double().t()
    ref[:, :96] += b1.double()
    case.check("ac", bac, ac, ref)
    case.done()


@pytest.mark.parametrize("general", GENERAL, ids=["chain2", "general"])
@pytest.mark.parametrize("M", MS)
def test_one_layer_dx_at_64_columns(M, general, monkeypatch):
    """dx = [da (two slabs) | dc] T^T + resid at F = 64, bf16, the residual a column slice of a wider tensor: K = 192 is the table's
    dx shape at any width, so chain2 runs it (two output tiles), the general kernel's straight-line form under the switch."""
    from mpgan_amd import ops
    _switch(monkeypatch, general)
    rs = np.random.RandomState(100 * M + 7)
    T, da, dc = _t(rs, 64, 192, scale=0.2), _t(rs, 2, M, 96), _t(rs, M, 96)
    resid = _t(rs, M, 80)[:, 8:72]
    (img,) = _images([T], False)
    bdx, dx = _framed(M, 64)
    c = ops.chain_struct(M, [dict(img=_ptr(img), K=192, N=64, resid=resid, out=dx)], A=da, lda=96, K1=96, a_slabs=2,
                         a_slab_stride=M * 96, A2=dc, lda2=96, f16=False)
    case = _Case(("dx_64", M, general), c, _table_route(general))
    ref = torch.cat([da.double().sum(0), dc.double()], 1) @ T.double().t() + resid.double()
    case.check("dx", bdx, dx, ref)
    case.done()


@pytest.mark.parametrize("f16", [True, False], ids=["f16", "bf16"])
@pytest.mark.parametrize("M", MS)
def test_general_one_layer_with_ten_output_tiles(M, f16):
    """K = 32 -> N = 320 with bias and LeakyReLU: tiles 8 and 9 come from the second trip of a wave's tile loop (late preload) and
    take their bias from global memory.  fp16 has the a | c projection's k-steps (straight-line form), bf16 the run-time loops."""
    from mpgan_amd import _lib, ops
    rs = np.random.RandomState(100 * M + 320 + f16)
    W, b, x = _t(rs, 320, 32, scale=0.2), _t(rs, 320), _t(rs, M, 32)
    (img,) = _images([W], f16)
    by, y = _framed(M, 320)
    c = ops.chain_struct(M, [dict(img=_ptr(img), K=32, N=320, bias=b, act=True, out=y, wscale=ops.SC_WN if f16 else 1.0)], A=x, lda=32, K1=32,
                         alpha=0.2, f16=f16, ascale=ops.SC_ACT if f16 else 1.0)
    case = _Case(("ten_tiles", M, "f16" if f16 else "bf16"), c, _lib.CHAIN_ROUTE_STRAIGHT if f16 else _lib.CHAIN_ROUTE_LOOPS)
    case.check("y", by, y, _lrelu(x.double() @ W.double().t() + b.double(), 0.2))
    case.done()


def test_pack_many_equals_pack_weights():
    """Every image mpg_pack_many builds is bit-identical to mpg_pack_weights' (same fragment order, same split)."""
    from mpgan_amd import ops
    rs = np.random.RandomState(8)
    W, pk = _holder(rs, 32, 32, dscale=2.0)
    singles = {
        # the edge network's images (forward and transposed) carry the power-of-two operand scales on top of the
        # dropout scale and are fp16; the node network's gradient images are plain bf16
        "W2": ops.pack_weights(W["W2"], 160, 96, scale=2.0 * ops.SC_W2, f16=True),
        "W3": ops.pack_weights(W["W3"], 192, 160, scale=2.0 * ops.SC_W3, f16=True),
        "W3T": ops.pack_weights(W["W3"], 192, 160, transpose=True, scale=2.0 * ops.SC_W3, f16=True),
        "W2T": ops.pack_weights(W["W2"], 160, 96, transpose=True, scale=2.0 * ops.SC_W2, f16=True),
        "V2": ops.pack_weights(W["V2"], 256, 256, scale=ops.SC_WN, f16=True), "V1T": ops.pack_weights(W["V1"], 256, 224, transpose=True),
    }
    for k, img in singles.items():
        assert torch.equal(img.view(torch.int16), pk.img[k].view(torch.int16)), k


def test_wgrad_group_and_accumulate():
    """Eleven dW = dY^T X (+ bias sums: every even job) as one grouped launch; a second flush with accumulate doubles the result."""
    from mpgan_amd import ops
    rs = np.random.RandomState(21)
    M = 7680
    # (the node network's own shapes with and without the bias column -- folded into tile column 0 at 256 inputs, inside the last
    # tile at 224 / 192 --, ragged tiles (160 x 130), a single column (96 x 3))
    shapes = [(32, 256), (256, 256), (256, 192), (256, 32), (96, 32), (96, 3), (256, 224), (160, 130), (256, 256), (128, 128), (160, 130)]
    dys = [_t(rs, M, n) for n, _ in shapes]
    xs = [_t(rs, M, k) for _, k in shapes]
    outs = [torch.zeros(n, k + 5, device=_dev()) for n, k in shapes]
    biases = [torch.zeros(n, device=_dev()) if i % 2 == 0 else None for i, (n, _) in enumerate(shapes)]
    for rep in range(2):
        wb = ops.WgradBatch()
        for dy, x, o, b in zip(dys, xs, outs, biases):
            wb.add(dy, x, out=o, out_col0=5, bias_out=b, accumulate=rep == 1)
        wb.flush()
    for dy, x, o, b in zip(dys, xs, outs, biases):
        ref = 2 * (dy.double().t() @ x.double())
        assert rel_err(o[:, 5:].cpu().numpy(), ref.cpu().numpy()) < TIGHT
        assert float(o[:, :5].abs().max()) == 0.0
        if b is not None:
            assert rel_err(b.cpu().numpy(), (2 * dy.double().sum(0)).cpu().numpy()) < TIGHT


def test_chain_rejects_bad_arguments():
    from mpgan_amd import ops
    rs = np.random.RandomState(1)
    W, pk = _holder(rs, 32, 32)
    x = _t(rs, 64, 32)
    y = torch.empty(64, 192, device=_dev())
    with pytest.raises(RuntimeError):  # LeakyReLU slope outside [0, 1]
        ops.chain(64, [dict(img=pk.ptr("W1S"), K=32, N=192, out=y)], A=x, lda=32, K1=32, alpha=1.5, f16=True)
    with pytest.raises(RuntimeError):  # K beyond the 256 features a fragment buffer holds
        ops.chain(64, [dict(img=pk.ptr("W1S"), K=300, N=192, out=y)], A=x, lda=32, K1=300, f16=True)


def test_packed_images_follow_parameter_updates(monkeypatch):
    """MPLayer caches its weight images; an optimizer step (in-place update seen by autograd's version counter) or a
    load_state_dict must be picked up by the next forward, refresh_packed() covers writes torch cannot see."""
    _switch(monkeypatch, False)
    _packed_images_follow_parameter_updates()


def test_packed_images_follow_parameter_updates_on_the_general_kernel(monkeypatch):
    """The same with every mpg_chain call of the layer (a | c projection, input gradients, dx) on the general kernel."""
    _switch(monkeypatch, True)
    _packed_images_follow_parameter_updates()


def _packed_images_follow_parameter_updates():
    from mpgan_amd.mpgan import MPLayer
    torch.manual_seed(0)
    layer = MPLayer(32, [96, 160, 192], [256, 256], 32).to(_dev())
    x = torch.randn(2, 30, 32, device=_dev())
    y0 = layer(x).detach().clone()
    opt = torch.optim.SGD(layer.parameters(), lr=0.05)
    layer(x).pow(2).mean().backward()
    opt.step()
    y1 = layer(x).detach().clone()
    assert torch.isfinite(y1).all() and (y1 - y0).abs().max() > 1e-5   # the update is visible ...
    fresh = MPLayer(32, [96, 160, 192], [256, 256], 32).to(_dev())
    fresh.load_state_dict(layer.state_dict())      # ... and equals a freshly packed layer with the same weights
    assert torch.equal(fresh(x), y1)
    with torch.no_grad():
        for q in layer.parameters():
            q.data.mul_(0.5)                       # a write behind autograd's back (as mpg_rmsprop does) ...
    layer.refresh_packed()                         # ... needs the explicit refresh
    fresh.load_state_dict(layer.state_dict())
    assert torch.equal(fresh(x), layer(x))


def test_linearnet_batch_norm_spectral_norm_vs_reference_golden():
    """LinearNet with both normalisations (mpgan/model.py:55-83, spectral_normalization.py): two training forwards (the power
    iteration and the running statistics move), gradients of the second, then an eval forward -- against the reference's own."""
    from conftest import load_golden
    from oracle import train_ref as T
    from mpgan_amd.mpgan import LinearNet
    g = load_golden("linearnet_bn_sn_f64.npz")
    net = LinearNet([24, 16], input_size=12, output_size=5, final_linear=True, batch_norm=True, spectral_norm=True, dropout_p=0.0).cuda()
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items() if "running" not in k and "num_batches" not in k}
    sd = net.state_dict()
    sd.update({k: v.cuda() for k, v in T.init_state_dict(shapes, seed=int(g["seed"]), dtype=torch.float32).items()})
    net.load_state_dict(sd)
    net.train()
    dev = lambda a: torch.from_numpy(a).float().cuda()
    y1 = net(dev(g["x1"]))
    (y1 * dev(g["g1"])).sum().backward()
    net.zero_grad()
    x2 = dev(g["x2"]).requires_grad_(True)
    y2 = net(x2)
    (y2 * dev(g["g2"])).sum().backward()
    assert rel_err(y1.detach().cpu().numpy(), g["y1"]) < TIGHT
    assert rel_err(y2.detach().cpu().numpy(), g["y2"]) < TIGHT
    assert rel_err(x2.grad.cpu().numpy(), g["dx2"]) < TIGHT
    for k, p in net.named_parameters():
        if "grad__" + k in g:
            assert rel_err(p.grad.cpu().numpy(), g["grad__" + k]) < TIGHT, k
    net.eval()
    assert rel_err(net(x2.detach()).detach().cpu().numpy(), g["y3"]) < TIGHT
    for k, v in net.state_dict().items():
        if "state__" + k in g:
            assert rel_err(v.double().cpu().numpy(), g["state__" + k]) < TIGHT, k
