"""The three ways a parameter gradient leaves a fused backward (``ops.ParamGrads``) give the same gradients: returned to autograd,
added into ``.grad`` by the kernel that forms it (direct), or queued for the grouped weight-gradient launch that adds into ``.grad``.

Every case builds the same inputs from one seed per route and calls the function's backward node itself, so the slots autograd would
get are in hand.  Direct against returned: the same bits (``.grad`` zero-filled: adding into zeros is exact).  Queued against
returned: the two choose different split-K factors, so each is held to the float64 gradients of the same function in torch at TIGHT;
every queued slot is None, the batch holds the expected jobs, the backward issues no weight-gradient launch and the flush exactly
one grouped GEMM + one grouped reduction.  dx: the same bits on every route.  No dropout anywhere: the references need no masks.

Shapes: 65 rows of widths 33 -> 70 for the dense layer; 2 jets of 5 and of 33 tokens (33 crosses the tile of 32) for the attention
blocks, whose kernels take heads of 16 features (E = 32 with 2 heads, and E = 64 with 4 once); 3 jets of 5 x 33 for the head."""
import numpy as np
import pytest
import torch

from conftest import rel_err
from test_gpu_mplayer import _count_calls

pytestmark = pytest.mark.gpu
TIGHT = 1e-4          # tests/test_gpu_gemm.py::_close
SENTINEL = 12345.0
# The launch lists asserted below -- each backward's, and the flush's -- are those of the commit before ``ops.ParamGrads``, recorded in
# profiles/grad_routes_bit_identity.txt.  One group per case here: at most 7 jobs, no target twice.
FLUSH = ["mpg_gemm_wgrad_group", "mpg_splitk_reduce_group"]


def _dev():
    return torch.device("cuda:0")


def _t(rs, *shape, scale=1.0):
    return (torch.from_numpy(rs.normal(size=shape)).float() * scale).to(_dev())


def _lrelu(v, a=0.2):
    return torch.where(v > 0, v, a * v)


class Case:
    """One call ``fn.apply(*args)``: ``params`` {name: index into args} (leaves that want a gradient, or frozen ones), ``xs`` the
    indices of the inputs that want one, ``ref(*args)`` the same function in torch (run in float64), ``jobs`` the queued jobs the
    backward adds and ``returned`` the names whose gradient is returned on every route (a bias alone)."""

    def __init__(self, fn, args, params, xs, ref, jobs, returned=()):
        self.fn, self.args, self.params, self.xs, self.ref, self.jobs, self.returned = fn, args, params, xs, ref, jobs, returned


def _outputs(out):
    return out if isinstance(out, tuple) else (out,)


def _run(build, route, frozen=False):
    """Forward, then the backward node called with fixed upstream gradients, on one route: "returned", "direct" (the flag alone)
    or "queued" (the flag and a batch, flushed here).  Returns dict(slots, grads {name: gradient}, dx [..], jobs, backward, flush)."""
    from mpgan_amd import ops
    st = ops.dev_state(_dev())
    case = build()
    leaves = {k: case.args[i] for k, i in case.params.items()}
    for q in leaves.values():
        q.requires_grad_(not frozen)
        q.grad = None if route == "returned" else torch.full_like(q, SENTINEL if frozen else 0.0)
    out = _outputs(case.fn.apply(*case.args))
    node = next(o.grad_fn for o in out if o is not None)
    rs = np.random.RandomState(77)
    ups = [None if (o is None or o.grad_fn is not node) else _t(rs, *o.shape) for o in out]
    calls = _count_calls(ops)
    st.grad_into_param, st.deferred_wgrad = route != "returned", (ops.WgradBatch() if route == "queued" else None)
    try:
        slots = node.apply(*ups)
        backward, njobs = list(calls.names), (len(st.deferred_wgrad.jobs) if route == "queued" else 0)
        if route == "queued":
            st.deferred_wgrad.flush()
    finally:
        calls.restore()
        st.grad_into_param, st.deferred_wgrad = False, None
    torch.cuda.synchronize()
    grads = {k: (slots[i] if slots[i] is not None else leaves[k].grad) for k, i in case.params.items()}
    return dict(slots={k: slots[i] for k, i in case.params.items()}, grads=grads, dx=[slots[i] for i in case.xs], jobs=njobs,
                backward=backward, flush=calls.names[len(backward):], case=case, ups=ups)


def _ref_grads(run):
    """Float64 autograd of the case's torch form with the same upstream gradients: {name: gradient}."""
    case = run["case"]
    a64 = [a.detach().double().requires_grad_(i in case.params.values()) if (torch.is_tensor(a) and a.is_floating_point()) else a
           for i, a in enumerate(case.args)]
    out = _outputs(case.ref(*a64))
    sum((o * u.double()).sum() for o, u in zip(out, run["ups"]) if u is not None).backward()
    return {k: a64[i].grad for k, i in case.params.items()}


def _same_bits(a, b, what):
    assert len(a) == len(b)
    for u, v in zip(a, b):
        assert (u is None) == (v is None) and (u is None or torch.equal(u, v)), what


def _check_queued(build, backward):
    """Returned against queued (and against the flag alone, which leaves GEMM-shaped gradients and column sums returned)."""
    ret, flag, que = _run(build, "returned"), _run(build, "direct"), _run(build, "queued")
    case, ref = ret["case"], _ref_grads(ret)
    assert que["jobs"] == case.jobs and ret["jobs"] == 0
    for k in case.params:
        if k in case.returned:
            assert que["slots"][k] is not None and torch.equal(que["slots"][k], ret["slots"][k]), k
        else:
            assert que["slots"][k] is None and ret["slots"][k] is not None, k
        assert flag["slots"][k] is not None and torch.equal(flag["slots"][k], ret["slots"][k]), k   # (no batch: as returned, bit for bit)
        for name, run in (("returned", ret), ("queued", que)):
            err = rel_err(run["grads"][k].double().cpu().numpy(), ref[k].cpu().numpy())
            print(name, k, "rel err vs float64: %.3g" % err)
            assert err < TIGHT, (name, k, err)
    _same_bits(ret["dx"], que["dx"], "dx")
    _same_bits(ret["dx"], flag["dx"], "dx")
    assert all(d is not None for d in ret["dx"])
    # the backward itself forms no weight gradient; the flush is one grouped GEMM + one grouped reduction (nothing without a job)
    assert que["backward"] == backward, que["backward"]
    assert que["flush"] == (FLUSH if case.jobs else []), que["flush"]


def _check_direct(build):
    """Returned against direct for a kernel that writes its parameter gradients itself: the same bits, autograd gets None."""
    ret, dire = _run(build, "returned"), _run(build, "direct")
    for k in ret["case"].params:
        assert dire["slots"][k] is None and ret["slots"][k] is not None, k
        assert torch.equal(dire["grads"][k], ret["grads"][k]) and bool((ret["grads"][k] != 0).any()), k
    _same_bits(ret["dx"], dire["dx"], "dx")
    assert dire["backward"] == ret["backward"] and len(ret["backward"]) == 1
    return ret


def _check_frozen(build):
    """No parameter wants a gradient, under ``grad_into_param`` with a batch collecting: ``.grad`` keeps the sentinel written
    beforehand, nothing is queued or returned, and dx is what the trainable node gives."""
    ret, fro = _run(build, "returned"), _run(build, "queued", frozen=True)
    for k, i in fro["case"].params.items():
        assert fro["slots"][k] is None, k
        assert bool((fro["case"].args[i].grad == SENTINEL).all()), k
    assert fro["jobs"] == 0 and fro["flush"] == []
    _same_bits(ret["dx"], fro["dx"], "dx")
    assert all(d is not None for d in ret["dx"])


# ---- FusedLinearFn, GenDiscBridgeFn ------------------------------------------------------------------------------------------
def _linear(bias=True, only_bias=False):
    def build():
        from mpgan_amd import ops
        rs = np.random.RandomState(1)
        M, K, N = 65, 33, 70
        x, W, b = _t(rs, M, K).requires_grad_(True), _t(rs, N, K, scale=K ** -0.5), (_t(rs, N) if bias else None)
        params = {"b": 2} if only_bias else {"W": 1, "b": 2} if bias else {"W": 1}
        return Case(ops.FusedLinearFn, [x, W, b, True, 0.2, 0.0, True], params, [0],
                    lambda x, W, b, *_: _lrelu(x @ W.t() + (0 if b is None else b)), 0 if only_bias else 1,
                    returned=("b",) if only_bias else ())
    return build


@pytest.mark.parametrize("form", ["bias", "no_bias", "only_bias"])
def test_fused_linear_routes(form):
    """``FusedLinearFn``: dW (+ db) as one job; without a bias; the bias alone rides in no GEMM and is returned on every route."""
    _check_queued(_linear(bias=form != "no_bias", only_bias=form == "only_bias"), ["mpg_gate", "mpg_gemm"])


def _bridge(with_buf):
    def build():
        from mpgan_amd import ops
        rs = np.random.RandomState(2)
        Bg, B, N, K, F, E = 2, (3 if with_buf else 2), 5, 64, 3, 64
        pre = _t(rs, Bg, N, K).requires_grad_(True)
        W1, b1, W2, b2 = _t(rs, F, K, scale=K ** -0.5), _t(rs, F), _t(rs, E, F, scale=F ** -0.5), _t(rs, E)
        buf = _t(rs, B, N, F) if with_buf else None
        real = None if buf is None else buf[:B - Bg].clone()

        def ref(pre, W1, b1, _buf, W2, b2, *_):
            feat = torch.tanh(pre @ W1.t() + b1)
            rows = feat if real is None else torch.cat([real.double(), feat], 0)
            return (None if with_buf else feat), _lrelu(rows @ W2.t() + b2)
        return Case(ops.GenDiscBridgeFn, [pre, W1, b1, buf, W2, b2, ops.ACT_CODES["tanh"], True, 0.2, 0.0, True],
                    {"W1": 1, "b1": 2, "W2": 4, "b2": 5}, [0], ref, 2)
    return build


@pytest.mark.parametrize("with_buf", [False, True], ids=["own_feat", "feat_buf"])
def test_bridge_routes(with_buf):
    """``GenDiscBridgeFn``: one job per layer, from one backward launch; alone, and behind a real jet in the caller's batch."""
    _check_queued(_bridge(with_buf), ["mpg_bridge_bwd"])


# ---- FusedMABFn, FusedSABChainFn ---------------------------------------------------------------------------------------------
def _mab_params(rs, E):
    s = E ** -0.5
    return [_t(rs, 3 * E, E, scale=s), _t(rs, 3 * E, scale=0.1), _t(rs, E, E, scale=s), _t(rs, E, scale=0.1), _t(rs, E, E, scale=s),
            _t(rs, E, scale=0.1)]


def _mab_sd(prm, ln=None):
    names = ("attention.in_proj_weight", "attention.in_proj_bias", "attention.out_proj.weight", "attention.out_proj.bias",
             "ff.net.0.weight", "ff.net.0.bias")
    sd = {"mab." + k: v for k, v in zip(names, prm)}
    if ln is not None:
        sd.update({"mab." + k: v for k, v in zip(("norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias"), ln)})
    return sd


def _ignore(rs, B, S):
    ig = (rs.uniform(size=(B, S)) < 0.3).astype(np.float32)
    ig[:, 0] = 0
    return torch.from_numpy(ig).to(_dev())


PRM = {"Win": 3, "bin": 4, "Wo": 5, "bo": 6, "Wf": 7, "bf": 8}
LN = {"n1w": 9, "n1b": 10, "n2w": 11, "n2b": 12}


def _mab(form, L, S, E=32, H=2):
    def build():
        from mpgan_amd import ops
        from oracle import gapt_ref as R
        rs = np.random.RandomState(3)
        B = 2
        cross, ln, seed = form in ("cross", "seed"), form == "layer_norm", form == "seed"
        x = _t(rs, *((1, 1, E) if seed else (B, L, E))).requires_grad_(not seed)
        y = _t(rs, B, S, E).requires_grad_(True) if cross else None
        ig = _ignore(rs, B, S)
        prm = _mab_params(rs, E)
        norms = [1 + _t(rs, E, scale=0.1), _t(rs, E, scale=0.1), 1 + _t(rs, E, scale=0.1), _t(rs, E, scale=0.1)] if ln else [None] * 4
        pk = ops.PackedMAB(prm[0], prm[2], prm[4]).ensure()

        def ref(x, y, ig, Win, bin_, Wo, bo, Wf, bf, n1w, n1b, n2w, n2b, *_):
            xx = x.expand(B, 1, E) if seed else x
            return R.mab_forward(_mab_sd((Win, bin_, Wo, bo, Wf, bf), (n1w, n1b, n2w, n2b) if ln else None), "mab", xx,
                                 xx if y is None else y, ig.reshape(B, S) != 0, num_heads=H, layer_norm=ln)
        params = dict(PRM, **(LN if ln else {}), **({"seed": 0} if seed else {}))
        xs = [1] if seed else [0, 1] if cross else [0]
        return Case(ops.FusedMABFn, [x, y, ig.reshape(-1), *prm, *norms, 1e-5 if ln else None, H, 0.2, True, 0.0, 0.0, True, pk],
                    params, xs, ref, (4 if cross else 3) + (4 if ln else 0) + (1 if seed else 0))
    return build


@pytest.mark.parametrize("form,L,S,E,H", [("self", 5, 5, 32, 2), ("self", 33, 33, 32, 2), ("self", 33, 33, 64, 4), ("cross", 5, 33, 32, 2),
                                           ("cross", 33, 5, 32, 2), ("layer_norm", 33, 33, 32, 2), ("seed", 1, 33, 32, 2)])
def test_mab_routes(form, L, S, E, H):
    """``FusedMABFn``: self-attention (three jobs), cross-attention (four: the two row blocks of the input projection, returned
    one under the other otherwise), with its norms inside (four column sums more) and with the one seed row all jets share as a
    leaf parameter (its gradient, dx summed over the jets, one column sum more)."""
    _check_queued(_mab(form, L, S, E, H), ["mpg_mab_bwd"])


def _sab_chain():
    from mpgan_amd import ops
    from oracle import gapt_ref as R
    rs = np.random.RandomState(4)
    B, N, E, H = 2, 5, 32, 2
    x, ig = _t(rs, B, N, E).requires_grad_(True), _ignore(rs, B, N)
    blocks = [_mab_params(rs, E) for _ in range(2)]
    pks = [ops.PackedMAB(p[0], p[2], p[4]).ensure() for p in blocks]

    def ref(x, ig, *a):
        for prm in (a[7:13], a[13:19]):
            x = R.mab_forward(_mab_sd(prm), "mab", x, x, ig.reshape(B, N) != 0, num_heads=H)
        return x
    names = {"%s%d" % (k, blk): 9 + 6 * blk + j for blk in range(2) for j, k in enumerate(PRM)}
    return Case(ops.FusedSABChainFn, [x, ig.reshape(-1), H, 0.2, True, 0.0, 0.0, True, pks, *blocks[0], *blocks[1]], names, [0], ref, 6)


def test_sab_chain_routes():
    """``FusedSABChainFn`` of two blocks: one backward launch and three jobs per block, the last block's first."""
    _check_queued(_sab_chain, ["mpg_mab_bwd", "mpg_mab_bwd"])


# ---- kernels that write their parameter gradients themselves: DiscHeadFn, BatchNormFn, LayerNormFn ------------------------------
def _head(bias=True):
    def build():
        from mpgan_amd import ops
        rs = np.random.RandomState(5)
        B, N, F = 3, 5, 33
        y, w, b = _t(rs, B, N, F, scale=0.3).requires_grad_(True), _t(rs, 1, F, scale=0.2), (_t(rs, 1) if bias else None)
        mask = torch.from_numpy((rs.uniform(size=(B, N, 1)) < 0.7).astype(np.float32)).to(_dev())
        return Case(ops.DiscHeadFn, [y, mask, w, b, True, True, 0.0, False], {"w": 2, "b": 3} if bias else {"w": 2}, [0], None, 0)
    return build


def _batchnorm():
    from mpgan_amd import ops
    rs = np.random.RandomState(6)
    M, F = 65, 33
    return Case(ops.BatchNormFn, [_t(rs, M, F).requires_grad_(True), 1 + _t(rs, F, scale=0.1), _t(rs, F, scale=0.1), 1e-5],
                {"w": 1, "b": 2}, [0], None, 0)


def _layernorm():
    from mpgan_amd import ops
    rs = np.random.RandomState(7)
    return Case(ops.LayerNormFn, [_t(rs, 2, 33, 32).requires_grad_(True), 1 + _t(rs, 32, scale=0.1), _t(rs, 32, scale=0.1), 1e-5],
                {"w": 1, "b": 2}, [0], None, 0)


DIRECT = {"head": (_head(), "mpg_disc_head_bwd"), "head_no_bias": (_head(False), "mpg_disc_head_bwd"),
          "batchnorm": (_batchnorm, "mpg_batchnorm_bwd"), "layernorm": (_layernorm, "mpg_layernorm_bwd")}


@pytest.mark.parametrize("name", sorted(DIRECT))
def test_kernel_written_routes(name):
    """The head (with and without bias), batch norm and layer norm: their one backward launch adds into zero-filled ``.grad``
    buffers the very bits it writes into fresh tensors otherwise, and the same dx."""
    build, entry = DIRECT[name]
    assert _check_direct(build)["backward"] == [entry]


@pytest.mark.parametrize("name", ["head", "batchnorm", "layernorm"])
def test_frozen_parameters_leave_grad_untouched(name):
    """A frozen norm or head inside a generator step: ``.grad`` is not written, dx is unchanged."""
    _check_frozen(DIRECT[name][0])
