"""GPU parity of the un-fused route's products: ``mpg_gemm`` in its four operand forms with every epilogue field, split-K with
``mpg_splitk_reduce``, the grouped weight-gradient launch (``ops.WgradBatch``), ``mpg_gate``, and the autograd functions built on
them (``FusedLinearFn``, ``MatMulFn``) -- against the float64 product with the same epilogue in torch, at TIGHT.

Operands are N(0, 1).  Outputs live inside sentinel-filled buffers with a row stride beyond their width (``_framed``): the frame
must come back bit for bit.  Operand buffers are padded with NaN, so a load outside the operand shows in the result.  The shapes
are the smallest that reach each path: tiles are 64 x 64 x 32, four waves of 32 x 32 each, eight k per thread and load."""
import ctypes as C

import numpy as np
import pytest
import torch

import split_ref
from conftest import rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-3       # BASELINE.json north_star (tests/test_gpu_mplayer.py)
TIGHT = 1e-4
SENTINEL = 12345.0
FORMS = [(1, 1), (1, 0), (0, 0), (0, 1)]
SHAPES = [(1, 1, 1), (31, 33, 7), (32, 32, 8), (33, 31, 9), (63, 65, 31), (64, 64, 32), (65, 63, 33), (129, 1, 64), (1, 129, 65),
          (100, 70, 100), (33, 31, 0), (1, 1, 0)]     # (K = 0: bias and epilogue only)


def _dev():
    return torch.device("cuda:0")


def _t(rs, *shape):
    return torch.from_numpy(rs.normal(size=shape)).float().to(_dev())


def _lrelu(v, a):
    return torch.where(v > 0, v, a * v)


def _framed(M, N, c0=3, extra=2, slabs=1):
    """``slabs`` outputs [M, N], each a view at column ``c0`` of a buffer [M + 1, c0 + N + extra] filled with a sentinel
    (tests/test_gpu_chain.py: ``_framed``, with a column offset): buffer, views, row stride, slab stride."""
    ld = c0 + N + extra
    buf = torch.full((slabs, M + 1, ld), SENTINEL, device=_dev())
    return buf, buf[:, :M, c0:c0 + N], ld, (M + 1) * ld


def _frame_intact(buf, M, N, c0=3):
    outside = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    outside[:, :M, c0:c0 + N] = False
    s = int(torch.tensor(SENTINEL).view(torch.int32))
    return bool((buf.view(torch.int32)[outside] == s).all())


def _stored(logical, k_contig, pad=0, off=0):
    """An operand the way the kernel addresses it: ``logical`` [rows, K] laid out with K contiguous (``A[r * ld + k]``) or rows
    contiguous (``A[k * ld + r]``), row stride = width + ``pad``, the base ``off`` elements into an allocation, NaN around it."""
    mat = logical if k_contig else logical.t()
    R, W = mat.shape
    ld = W + pad
    if mat.numel() == 0:
        return torch.empty(0, device=_dev()), max(ld, 1)
    buf = torch.full((off + R * ld,), float("nan"), device=_dev())
    view = buf[off:].view(R, ld)[:, :W]
    view.copy_(mat)
    return view, ld


def _gemm(A, B, ak, bk, f16, *, apad=0, aoff=0, bpad=0, boff=0, c0=3, prefill=None, **epi):
    """C = epi(A B) for logical A [M, K], B [K, N] through ``ops.gemm`` into a framed output; returns (buffer, view [M, N])."""
    from mpgan_amd import ops
    M, K = A.shape
    N = B.shape[1]
    a, lda = _stored(A, bool(ak), apad, aoff)
    b, ldb = _stored(B.t(), bool(bk), bpad, boff)
    buf, view, ldc, _ = _framed(M, N, c0=c0)
    if prefill is not None:
        view[0].copy_(prefill)
    ops.gemm(a, lda, b, ldb, view[0], ldc, M, N, K, ak=bool(ak), bk=bool(bk), f16=bool(f16), **epi)
    return buf, view[0]


def _close(got, ref, what=""):
    err = rel_err(got.detach().double().cpu().numpy(), ref.detach().double().cpu().numpy())
    assert err < TIGHT, (what, err)
    return err


# ---- forms and tile edges -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f16", [0, 1])
@pytest.mark.parametrize("ak,bk", FORMS, ids=lambda v: str(v))
def test_gemm_forms_and_tile_edges(ak, bk, f16):
    """All four (ak, bk) instantiations -- (0, 1) among them, which ``mpg_gemm`` dispatches and nothing else runs -- on both
    operand formats, at one element, around one 32-wide wave tile and one 64-wide workgroup tile in every direction, around one
    and two k-tiles of 32, a single column over three row tiles and the reverse, and K = 0; with a bias and LeakyReLU."""
    for M, N, K in SHAPES:
        rs = np.random.RandomState(1000 * ak + 100 * bk + M + N + K)
        A, B, bias = _t(rs, M, K), _t(rs, K, N), _t(rs, N)
        buf, c = _gemm(A, B, ak, bk, f16, bias=bias, act=True, alpha=0.2)
        ref = _lrelu(A.double() @ B.double() + bias.double(), 0.2)
        _close(c, ref, (M, N, K))
        assert _frame_intact(buf, M, N), (M, N, K)
        if K == 0:   # nothing but the epilogue: exact
            assert torch.equal(c, _lrelu(bias, 0.2).expand(M, N)), (M, N)


# ---- load paths -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f16", [0, 1])
@pytest.mark.parametrize("ak,bk", [(1, 1), (1, 0)], ids=lambda v: str(v))
def test_gemm_load_paths_agree_bit_for_bit(ak, bk, f16):
    """``tile_load`` reads 2 x 16 bytes per thread where the operand's k is contiguous, its row stride a multiple of 4 and its
    base 16-byte aligned, and element by element otherwise: a row stride that is no multiple of 4, and a multiple of 4 behind a
    base one element off, for A and for B.  The staged fragments are the same, so are the results, bit for bit."""
    M, N, K = 65, 63, 64
    rs = np.random.RandomState(7 + ak + bk)
    A, B = _t(rs, M, K), _t(rs, K, N)
    buf, base = _gemm(A, B, ak, bk, f16)
    _close(base, A.double() @ B.double())
    assert _frame_intact(buf, M, N)
    variants = {"lda % 4 = 1": dict(apad=1), "A base off by one element": dict(apad=4, aoff=1),
                "ldb % 4 != 0": dict(bpad=1 if bk else 2), "B base off by one element": dict(bpad=4 if bk else 1, boff=1)}
    for name, kw in variants.items():
        buf, c = _gemm(A, B, ak, bk, f16, **kw)
        assert torch.equal(c, base), name
        assert _frame_intact(buf, M, N), name


# ---- two segments ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f16", [0, 1])
@pytest.mark.parametrize("K1,K2", [(3, 30), (33, 4), (8, 1), (1, 64)])
def test_gemm_two_segments(K1, K2, f16):
    """[A | A2] W[:, c : c + K1 + K2]^T: the seam inside the first group of 8, beyond the first k-tile, on a group boundary, after
    one column; A2 with a row stride of its own (K2 + 3), W entered at column 1 (a base that is not 16-byte aligned)."""
    from mpgan_amd import ops
    M, N = 65, 33
    rs = np.random.RandomState(K1 + 10 * K2)
    A, A2, W, bias = _t(rs, M, K1), _t(rs, M, K2), _t(rs, N, 1 + K1 + K2 + 2), _t(rs, N)
    a2, lda2 = _stored(A2, True, pad=3, off=1)
    buf, view, ldc, _ = _framed(M, N)
    ops.gemm(A, K1, W, W.stride(0), view[0], ldc, M, N, K1 + K2, ak=True, bk=True, b_off=1, A2=a2, lda2=lda2, K1=K1, bias=bias,
             f16=bool(f16))
    ref = torch.cat((A, A2), 1).double() @ W[:, 1:1 + K1 + K2].double().t() + bias.double()
    _close(view[0], ref)
    assert _frame_intact(buf, M, N)
    # ... and through ops.linear_fwd, the form the layer-1 factorisation calls
    y = ops.linear_fwd(A, W, bias, x2=a2, w_col0=1, f16=bool(f16))
    assert torch.equal(y, view[0])


# ---- split-K ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("splitk", [1, 2, 3, 4, 7])
@pytest.mark.parametrize("ak,bk", [(0, 0), (1, 1)], ids=lambda v: str(v))
def test_gemm_splitk_slabs(ak, bk, splitk):
    """K = 100 is four k-tiles; z-slice z of ``splitk`` takes tiles [z per, (z + 1) per), per = ceil(4 / splitk): three slices
    leave the third empty (kbeg = 128 >= K), seven leave three empty, and the last live one is ragged (4 of 32 columns).  Every
    slab against the float64 product over its own k range, slab 0 with the bias, the empty ones exactly zero, the sum at TIGHT."""
    from mpgan_amd import ops
    M, N, K = 65, 33, 100
    rs = np.random.RandomState(splitk)
    A, B, bias = _t(rs, M, K), _t(rs, K, N), _t(rs, N)
    a, lda = _stored(A, bool(ak))
    b, ldb = _stored(B.t(), bool(bk))
    buf, view, ldc, stride = _framed(M, N, slabs=splitk)
    ops.gemm(a, lda, b, ldb, view[0], ldc, M, N, K, ak=bool(ak), bk=bool(bk), bias=bias, splitk=splitk, split_stride=stride)
    assert _frame_intact(buf, M, N)
    per = -(-4 // splitk)
    scale = float((A.double() @ B.double()).abs().max())
    for z in range(splitk):
        k0, k1 = min(K, 32 * per * z), min(K, 32 * per * (z + 1))
        if k0 == k1:
            assert z > 0 and float(view[z].abs().max()) == 0.0, z
            continue
        ref = A[:, k0:k1].double() @ B[k0:k1].double() + (bias.double() if z == 0 else 0.0)
        assert float((view[z].double() - ref).abs().max()) / scale < TIGHT, z
    _close(view.double().sum(0), A.double() @ B.double() + bias.double())


@pytest.mark.parametrize("splitk", [1, 2, 3, 4, 7])
def test_splitk_reduce_offsets_and_bias(splitk):
    """dW = dY^T X with a ones column over 100 rows in ``splitk`` slices, then ``mpg_splitk_reduce`` into columns 5 .. 5 + K of an
    output with row stride K + 9: with a bias output, and with has_bias = 1 and no bias pointer (the ones column is dropped)."""
    from mpgan_amd import ops, _lib
    rows, N, K = 100, 33, 37
    rs = np.random.RandomState(40 + splitk)
    dy, x = _t(rs, rows, N), _t(rs, rows, K)
    part = torch.empty(splitk, N, K + 1, device=_dev())
    ops.gemm(dy, N, x, K, part, K + 1, N, K + 1, rows, ak=False, bk=False, splitk=splitk, split_stride=N * (K + 1), ones_col=True)
    ref, ref_b = dy.double().t() @ x.double(), dy.double().sum(0)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for with_bias in (True, False):
        out = torch.full((N + 1, K + 9), SENTINEL, device=_dev())
        bias = torch.full((N + 2,), SENTINEL, device=_dev())
        code = _lib.lib().mpg_splitk_reduce(C.c_void_p(part.data_ptr()), splitk, N, K, 1, C.c_void_p(out.data_ptr() + 4 * 5), K + 9,
                                            C.c_void_p(bias.data_ptr()) if with_bias else None, st)
        assert code == 0
        _close(out[:N, 5:5 + K], ref)
        frame = out.clone()
        frame[:N, 5:5 + K] = SENTINEL
        assert torch.equal(frame, torch.full_like(frame, SENTINEL))
        if with_bias:
            _close(bias[:N], ref_b)
            assert float(bias[N]) == SENTINEL and float(bias[N + 1]) == SENTINEL
        else:
            assert torch.equal(bias, torch.full_like(bias, SENTINEL))


# ---- the ones column ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 65, 300])
@pytest.mark.parametrize("K", [64, 128, 63, 65])
def test_wgrad_single_launch_ones_column(K, rows):
    """``ops.linear_bwd_weight`` with ``bias_out``: the single launch gives the ones column a tile column of its own when x is 64
    or 128 wide (the grouped launch folds it instead), keeps it inside the last tile at 63 and is one past a tile at 65; dy of
    70 columns = two row tiles of the product; 300 rows = two z-slices."""
    from mpgan_amd import ops
    N = 70
    rs = np.random.RandomState(K + rows)
    dy, x = _t(rs, rows, N), _t(rs, rows, K)
    out = torch.full((N, K + 7), SENTINEL, device=_dev())
    db = torch.full((N,), SENTINEL, device=_dev())
    ops.linear_bwd_weight(dy, x, out=out, out_col0=4, bias_out=db)
    _close(out[:, 4:4 + K], dy.double().t() @ x.double())
    _close(db, dy.double().sum(0))
    assert bool((out[:, :4] == SENTINEL).all()) and bool((out[:, 4 + K:] == SENTINEL).all())


# ---- grouped launch -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 37, 100])
def test_wgrad_group_folded_column_and_two_launches(rows):
    """Eighteen jobs in one queue = two launches (``GROUP_MAX`` = 16): x of 64 and 128 columns with a bias -- the folded ones
    column -- under dy of 1, 65 and 130 columns (the fold at one and at three row tiles), the same without a bias, ragged widths
    with the column inside the last tile, ``out_scale`` = 0.5 on every third job; dy of 1, 37 and 100 rows."""
    from mpgan_amd import ops
    rs = np.random.RandomState(rows)
    shapes = [(n, k, True) for k in (64, 128) for n in (1, 65, 130)] + [(n, k, False) for k in (64, 128) for n in (1, 65, 130)]
    shapes += [(33, 63, True), (33, 65, True), (70, 3, True), (5, 1, True), (96, 32, False), (2, 192, True)]
    assert len(shapes) == 18
    wb = ops.WgradBatch()
    jobs = []
    for i, (n, k, hb) in enumerate(shapes):
        dy, x = _t(rs, rows, n), _t(rs, rows, k)
        out = torch.full((n, k + 6), SENTINEL, device=_dev())
        db = torch.full((n,), SENTINEL, device=_dev()) if hb else None
        scale = 0.5 if i % 3 == 0 else 1.0
        wb.add(dy, x, out=out, out_col0=5, out_scale=scale, bias_out=db)
        jobs.append((dy, x, out, db, scale))
    assert [len(g) for g in wb._groups()] == [16, 2]
    wb.flush()
    for i, (dy, x, out, db, scale) in enumerate(jobs):
        k = x.shape[1]
        _close(out[:, 5:5 + k], scale * (dy.double().t() @ x.double()), shapes[i])
        assert bool((out[:, :5] == SENTINEL).all()) and bool((out[:, 5 + k:] == SENTINEL).all()), shapes[i]
        if db is not None:
            _close(db, scale * dy.double().sum(0), shapes[i])


def test_wgrad_group_two_jobs_on_one_target():
    """Two jobs that add into the same ``out`` / ``bias_out`` (a module applied twice in one backward) land in launches of their
    own -- the grouped reduction reads and writes a target once per element -- and the target holds both sums on top of what it held."""
    from mpgan_amd import ops
    rs = np.random.RandomState(5)
    rows, n, k = 37, 65, 64
    out0, db0 = _t(rs, n, k), _t(rs, n)
    out, db = out0.clone(), db0.clone()
    other = torch.zeros(n, k, device=_dev())
    pairs = [(_t(rs, rows, n), _t(rs, rows, k)) for _ in range(3)]
    wb = ops.WgradBatch()
    wb.add(*pairs[0], out=out, bias_out=db, accumulate=True)
    wb.add(*pairs[1], out=other)
    wb.add(*pairs[2], out=out, bias_out=db, accumulate=True)
    assert [len(g) for g in wb._groups()] == [2, 1]
    wb.flush()
    ref = out0.double() + pairs[0][0].double().t() @ pairs[0][1].double() + pairs[2][0].double().t() @ pairs[2][1].double()
    _close(out, ref)
    _close(db, db0.double() + pairs[0][0].double().sum(0) + pairs[2][0].double().sum(0))
    _close(other, pairs[1][0].double().t() @ pairs[1][1].double())


def test_wgrad_group_rejects_what_it_does_not_compute():
    """``mpg_gemm_wgrad_group`` is the plain dW = scale A^T B form: -2 for a job with a bias pointer, an activation, a gate, a
    residual, ``accumulate`` or dropout, -1 for no job and for more than ``MPG_GROUP_MAX``; nothing is launched."""
    from mpgan_amd import ops, _lib
    from mpgan_amd._lib import MpgGemm
    lib, st = _lib.lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    dy, x = torch.ones(8, 4, device=_dev()), torch.ones(8, 5, device=_dev())
    part = torch.full((4, 5), SENTINEL, device=_dev())
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def jobs(n, **fields):
        gs, sk = (MpgGemm * n)(), (C.c_int * n)()
        for i in range(n):
            g = gs[i]
            g.A, g.lda, g.B, g.ldb, g.C, g.ldc = ptr(dy), 4, ptr(x), 5, ptr(part), 5
            g.M, g.N, g.K, g.split_stride, g.out_scale, g.alpha = 4, 5, 8, 20, 1.0, 0.2
            sk[i] = 1
        for k, v in fields.items():
            setattr(gs[n - 1], k, v)
        return gs, sk
    for fields in (dict(bias=ptr(dy)), dict(act=1), dict(gateH=ptr(dy)), dict(resid=ptr(dy)), dict(accumulate=1), dict(drop_thr=77)):
        gs, sk = jobs(2, **fields)
        assert lib.mpg_gemm_wgrad_group(gs, sk, 2, st) == -2, fields
    gs, sk = jobs(ops.GROUP_MAX + 1)
    assert lib.mpg_gemm_wgrad_group(gs, sk, 0, st) == -1
    assert lib.mpg_gemm_wgrad_group(gs, sk, ops.GROUP_MAX + 1, st) == -1
    torch.cuda.synchronize()
    assert bool((part == SENTINEL).all())
    gs, sk = jobs(1)       # (the same job is taken when nothing is set)
    assert lib.mpg_gemm_wgrad_group(gs, sk, 1, st) == 0
    _close(part, torch.full((4, 5), 8.0))


# ---- epilogue -------------------------------------------------------------------------------------------------------------------
def _keep(M, N, tag, thr):
    """The launch's keep mask times its scale, float64 (ones without dropout)."""
    from mpgan_amd import ops
    if not thr:
        return torch.ones(M, N, dtype=torch.float64, device=_dev())
    return ops.dropout_mask(M, N, tag, thr, _dev()).double() * (256.0 / (256.0 - thr))


EPILOGUES = {
    "bias": dict(bias=True),
    "act0": dict(act=True, alpha=0.0), "act0.2": dict(act=True, alpha=0.2), "act1": dict(act=True, alpha=1.0),
    "scale": dict(out_scale=-0.5),
    "drop_bits": dict(thr=128), "drop_bytes": dict(thr=77),
    "resid": dict(resid=True),
    "accumulate": dict(accumulate=True),
    "all_bits": dict(bias=True, act=True, alpha=0.2, out_scale=-0.5, thr=128, resid=True, accumulate=True),
    "all_bytes": dict(bias=True, act=True, alpha=0.2, out_scale=-0.5, thr=77, resid=True, accumulate=True),
}


@pytest.mark.parametrize("f16", [0, 1])
@pytest.mark.parametrize("name", list(EPILOGUES))
def test_gemm_epilogue_fields(name, f16):
    """(1, 1) at 65 x 70 x 33, each epilogue field on its own and all together, in the kernel's order:
    C = drop(act(scale A B + bias)) + resid (+ C).  Dropout in bit mode (thr = 128) and byte mode (thr = 77): the dropped
    elements are exactly those of ``ops.dropout_mask`` and exactly zero; the residual with a row stride of N + 3."""
    from mpgan_amd import ops
    cfg = dict(bias=False, act=False, alpha=0.2, out_scale=1.0, thr=0, resid=False, accumulate=False)
    cfg.update(EPILOGUES[name])
    M, N, K = 65, 70, 33
    rs = np.random.RandomState(len(name))
    A, B, bias, resid, c_old = _t(rs, M, K), _t(rs, K, N), _t(rs, N), _t(rs, M, N + 3), _t(rs, M, N)
    ops.set_seed(4242, _dev())
    tag, thr = 8 * 321 + ops.TAG_GENERIC, cfg["thr"]
    kw = dict(out_scale=cfg["out_scale"], act=cfg["act"], alpha=cfg["alpha"], accumulate=cfg["accumulate"])
    if cfg["bias"]:
        kw["bias"] = bias
    if thr:
        kw["drop"] = (ops.seed_tensor(_dev()), tag, thr, 256.0 / (256.0 - thr))
    if cfg["resid"]:
        kw.update(resid=resid[:, :N], ldr=N + 3)
    buf, c = _gemm(A, B, 1, 1, f16, prefill=c_old, **kw)
    keep = _keep(M, N, tag, thr)
    v = cfg["out_scale"] * (A.double() @ B.double()) + (bias.double() if cfg["bias"] else 0.0)
    if cfg["act"]:
        v = _lrelu(v, cfg["alpha"])
    v = v * keep
    ref = v + (resid[:, :N].double() if cfg["resid"] else 0.0) + (c_old.double() if cfg["accumulate"] else 0.0)
    _close(c, ref, name)
    assert _frame_intact(buf, M, N), name
    if thr:
        frac = float((keep != 0).double().mean())
        assert abs(frac - (1 - thr / 256.0)) < 0.04, frac
        if not (cfg["resid"] or cfg["accumulate"]):
            assert torch.equal(c == 0, keep == 0), name


@pytest.mark.parametrize("f16", [0, 1])
@pytest.mark.parametrize("gate_act", [0, 1])
@pytest.mark.parametrize("thr", [0, 128, 77])
def test_gemm_gate(thr, gate_act, f16):
    """(1, 0) at 65 x 70 x 33 with ``gateH`` (row stride N + 1): C = (A B) * lrelu'(H) * keep -- the derivative is 1 for H > 0 and the
    slope for H <= 0, zero included (H carries exact zeros of both signs) -- with the gate's dropout in both modes."""
    from mpgan_amd import ops
    M, N, K = 65, 70, 33
    rs = np.random.RandomState(thr + gate_act)
    A, B, H = _t(rs, M, K), _t(rs, K, N), _t(rs, M, N + 1)
    H[::3, ::5] = 0.0
    H[1::3, ::7] = -0.0
    ops.set_seed(4243, _dev())
    tag = 8 * 322 + ops.TAG_GENERIC
    gate = (H, N + 1, gate_act, ops.seed_tensor(_dev()), tag, thr, 256.0 / (256.0 - thr))
    buf, c = _gemm(A, B, 1, 0, f16, gate=gate, alpha=0.2)
    h = H[:, :N].double()
    slope = torch.where(h > 0, torch.ones_like(h), torch.full_like(h, 0.2)) if gate_act else torch.ones_like(h)
    keep = _keep(M, N, tag, thr)
    _close(c, (A.double() @ B.double()) * slope * keep, (thr, gate_act))
    assert _frame_intact(buf, M, N)
    if thr:
        assert torch.equal(c == 0, keep == 0)


# ---- mpg_gate -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thr", [0, 77, 128])
@pytest.mark.parametrize("M,N", [(1, 1), (37, 5), (64, 33), (130, 70)])
def test_gate_bit_identical_to_torch(M, N, thr):
    """``ops.gate`` on column slices of wider tensors (ldi, ldh > N), widths that are no multiples of 4 (the byte groups) or 32
    (the bit words): with H and the activation's derivative, and without H (``gate_act`` = 0, the stand-alone dropout) -- the very
    float32 product in * (lrelu'(H) * scale | 0) that torch forms from ``ops.dropout_mask``."""
    from mpgan_amd import ops
    rs = np.random.RandomState(M + N + thr)
    g_w, H_w = _t(rs, M, N + 3), _t(rs, M, N + 2)
    g, H = g_w[:, 1:1 + N], H_w[:, 2:2 + N]
    H[::2, ::3] = 0.0
    assert g.stride(0) == N + 3 and H.stride(0) == N + 2
    ops.set_seed(4244, _dev())
    tag, scale = 8 * 323 + ops.TAG_GENERIC, 256.0 / (256.0 - thr)
    mask = ops.dropout_mask(M, N, tag, thr, _dev()) if thr else torch.ones(M, N, device=_dev())
    one, sc = torch.ones((), device=_dev()), torch.tensor(scale, dtype=torch.float32, device=_dev())
    for with_h in (True, False):
        out = ops.gate(g, H if with_h else None, gate_act=with_h, alpha=0.2, seed_t=ops.seed_tensor(_dev()), tag=tag, thr=thr,
                       scale=scale)
        gt = torch.where(H > 0, one, 0.2 * one) if with_h else torch.ones(M, N, device=_dev())
        if thr:
            gt = torch.where(mask != 0, gt * sc, 0.0 * one)
        assert torch.equal(out, g * gt), with_h
        assert out.shape == (M, N)
    if thr and M * N > 1000:
        assert abs(float(mask.mean()) - (1 - thr / 256.0)) < 0.03


# ---- the autograd functions -----------------------------------------------------------------------------------------------------
def _fused_linear_case(act, p_drop, resid, sliced, queued):
    from mpgan_amd import ops
    dev = _dev()
    M, K, N, alpha = 65, 33, 70, 0.2
    rs = np.random.RandomState(int(act) + 2 * int(resid) + 4 * int(sliced) + 8 * int(queued))
    xw = _t(rs, 5, 13, K + 1).requires_grad_(True)           # M = 65 rows of K (+ 1) columns
    x = xw[..., :-1] if sliced else xw[..., :K].contiguous()
    W, b = (_t(rs, N, K) / K ** 0.5).requires_grad_(True), _t(rs, N).requires_grad_(True)
    r = _t(rs, 5, 13, N).requires_grad_(True) if resid else None
    up = _t(rs, 5, 13, N)
    st = ops.dev_state(dev)
    ops.set_seed(99, dev)
    y = ops.FusedLinearFn.apply(x, W, b, act, alpha, p_drop, True, r)
    tag = ops.last_tag(dev)
    if queued:
        W.grad, b.grad = torch.zeros_like(W), torch.zeros_like(b)
        st.grad_into_param, st.deferred_wgrad = True, ops.WgradBatch()
    try:
        (y * up).sum().backward()
        if queued:
            assert len(st.deferred_wgrad.jobs) == 1
            st.deferred_wgrad.flush()
    finally:
        st.grad_into_param, st.deferred_wgrad = False, None
    thr, _ = ops.drop_params(p_drop)
    keep = _keep(M, N, tag + ops.TAG_GENERIC, thr).reshape(5, 13, N)
    x64, W64, b64 = (t.detach().double().requires_grad_(True) for t in (xw, W, b))
    z = x64[..., :K] @ W64.t() + b64
    yr = (_lrelu(z, alpha) if act else z) * keep
    if resid:
        r64 = r.detach().double().requires_grad_(True)
        yr = yr + r64
    (yr * up.double()).sum().backward()
    _close(y, yr, "y")
    _close(xw.grad[..., :K], x64.grad[..., :K], "dx")
    assert float(xw.grad[..., K].abs().max()) == 0.0
    _close(W.grad, W64.grad, "dW")
    _close(b.grad, b64.grad, "db")
    if resid:
        _close(r.grad, r64.grad, "dresid")
    return float(z.detach().abs().min() / z.detach().abs().max())


@pytest.mark.parametrize("sliced,queued", [(False, False), (True, False), (False, True)], ids=["plain", "sliced_x", "queued"])
@pytest.mark.parametrize("kind", ["act_dropout", "resid"])
def test_fused_linear_fn_vs_fp64(kind, sliced, queued):
    """``FusedLinearFn`` (Linear -> LeakyReLU -> dropout, and Linear + residual) forward and dx, dW, db (and the residual's gradient)
    against float64 with the launch's own keep mask: from a contiguous x, from x = wider rows without their last column (the
    discriminator's input), and with the weight gradient queued for the grouped launch and added into ``.grad``.  4550
    pre-activations against a kink: the smallest is beyond float32 rounding of the largest (asserted at 1e-6), so no sign differs."""
    act = kind == "act_dropout"
    margin = _fused_linear_case(act, 0.3 if act else 0.0, not act, sliced, queued)
    assert not act or margin > 1e-6, margin


@pytest.mark.parametrize("form", ["nt", "nn", "tn"])
def test_matmul_fn_first_derivatives(form):
    """``MatMulFn`` in its three forms at 65 / 33 / 70: the product and both first derivatives against float64 autograd."""
    from mpgan_amd import ops
    rs = np.random.RandomState(len(form) + ord(form[0]))
    shapes = {"nt": ((65, 70), (33, 70)), "nn": ((65, 33), (33, 70)), "tn": ((65, 33), (65, 70))}[form]
    A, B = (_t(rs, *s).requires_grad_(True) for s in shapes)
    c = ops.MatMulFn.apply(A, B, form)
    A64, B64 = (t.detach().double().requires_grad_(True) for t in (A, B))
    ref = {"nt": lambda: A64 @ B64.t(), "nn": lambda: A64 @ B64, "tn": lambda: A64.t() @ B64}[form]()
    up = _t(rs, *ref.shape)
    (c * up).sum().backward()
    (ref * up.double()).sum().backward()
    _close(c, ref, "C")
    _close(A.grad, A64.grad, "dA")
    _close(B.grad, B64.grad, "dB")


# ---- operand magnitudes ---------------------------------------------------------------------------------------------------------
def _linear_fwd_err(e, f16):
    from mpgan_amd import ops
    A, B = split_ref.operands(e)
    y = ops.linear_fwd(torch.from_numpy(A).to(_dev()), torch.from_numpy(B).to(_dev()), None, f16=f16)
    return split_ref.rel_err(y.cpu().numpy(), split_ref.reference(A, B))


@pytest.mark.parametrize("e", split_ref.E_BF16)
def test_linear_fwd_bf16_route_at_any_magnitude(e):
    """bf16 hi/lo operands have float32's exponents: A scaled by 2^-40 .. 2^40 stays at TIGHT (the emulation: 4.5e-6, flat)."""
    err = _linear_fwd_err(e, False)
    print("bf16 route, A * 2^%d: kernel %.3g, emulated split %.3g" % (e, err, split_ref.split_err(e, False)))
    assert err < TIGHT, (e, err)


@pytest.mark.parametrize("e", split_ref.E_F16)
def test_linear_fwd_fp16_route_per_magnitude(e):
    """fp16 hi/lo operands carry no scales here (the chain and edge kernels do): the pair keeps 22 bits only while lo stays a normal
    fp16 number, so the error grows as the operand shrinks.  The bound comes from the reference side alone (``split_ref.f16_bound``:
    4 x (emulated split error + a plain float32 product's error)); down to 2^-10 the route also meets TIGHT outright."""
    err, bound = _linear_fwd_err(e, True), split_ref.f16_bound(e)
    print("fp16 route, A * 2^%d: kernel %.3g, emulated split %.3g, bound %.3g" % (e, err, split_ref.split_err(e, True), bound))
    assert err <= bound, (e, err, bound)
    if e >= -10:
        assert err < TIGHT, (e, err)
