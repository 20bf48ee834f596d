"""GPU: the sparse k-NN route of the fused MPLayer (``ops.OPTIONS["knn_sparse"]``: ``mpg_knn_edge_fwd`` / ``mpg_knn_edge_bwd`` on the
B * N * k rows of the neighbour sets) against the fp64 oracle's k-NN branch, the reference goldens and the dense route.

Bars are those of tests/test_gpu_mplayer.py: TIGHT = 1e-4, TOL = 1e-3, ``_assert_smooth_bars`` for slope 1, ``assert_grads`` with the
fp32 oracle as the kink control for the default slope."""
import contextlib
import itertools

import numpy as np
import pytest
import torch

from conftest import assert_grads, load_golden, rel_err
from test_gpu_mplayer import TIGHT, TOL, _assert_smooth_bars, _fused_node, _mplayer_shapes

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda:0")


@contextlib.contextmanager
def knn_sparse(on=True):
    from mpgan_amd import ops
    old = ops.OPTIONS["knn_sparse"]
    ops.OPTIONS["knn_sparse"] = on
    try:
        yield
    finally:
        ops.OPTIONS["knn_sparse"] = old


def _layer(F, out, k, loops, sm, alpha, sd64, p_drop=0.0):
    from mpgan_amd.mpgan import MPLayer
    layer = MPLayer(F, [96, 160, 192], [256, 256], out, sum=sm, fully_connected=False, num_knn=k, self_loops=loops,
                    leaky_relu_alpha=alpha, dropout_p=p_drop).to(_dev())
    layer.load_state_dict({kk: v.float() for kk, v in sd64.items()})
    return layer


def _run_hip(layer, x64, mask64, g64, sparse=True):
    """One forward + backward of ``layer`` on the sparse (or dense) route: (y, {dx, parameter gradients}) as fp64 numpy, the node."""
    from mpgan_amd import ops
    for p in layer.parameters():
        p.grad = None
    x = x64.float().to(_dev()).requires_grad_(True)
    mask = None if mask64 is None else mask64.float().to(_dev())
    with knn_sparse(sparse):
        y = layer(x, mask is not None, mask)
        node = _fused_node(y)
        assert (ops.knn_saved(node) is not None) == sparse      # the route that was asked for is the route that ran
        (y * g64.float().to(_dev())).sum().backward()
    grads = {"dx": x.grad.double().cpu().numpy(), **{kk: p.grad.double().cpu().numpy() for kk, p in layer.named_parameters()}}
    return y.detach().double().cpu().numpy(), grads


def _run_oracle(sd64, x64, mask64, g64, k, loops, sm, alpha, dt=torch.float64, **kw):
    import oracle
    sdo = {"L." + kk: v.detach().clone().to(dt).requires_grad_(True) for kk, v in sd64.items()}
    xo = x64.detach().clone().to(dt).requires_grad_(True)
    yo = oracle.mplayer_forward(sdo, "L", xo, None if mask64 is None else mask64.to(dt), sum_agg=sm, alpha=alpha, knn=(k, loops), **kw)
    (yo * g64.to(dt)).sum().backward()
    return yo.detach().double().numpy(), {"dx": xo.grad.double().numpy(), **{kk[2:]: v.grad.double().numpy() for kk, v in sdo.items()}}


def _errs(y, grads, yo, go):
    return {"y": rel_err(y, yo), **{kk: rel_err(grads[kk], go[kk]) for kk in go}}


def _sets_agree(x64, mask64, k, loops):
    """The neighbour sets of ``mpg_knn_sets`` (fp32) are the oracle's (fp64) on this input: the comparison below is then about the
    edge kernels alone."""
    from mpgan_amd import ops
    from test_gpu_mplayer import _ref_knn_bits
    B, N, _ = x64.shape
    NW = (N + 31) // 32
    mask = None if mask64 is None else mask64.float().to(_dev())
    words = ops.knn_sets(x64.float().to(_dev()), mask, k, loops).cpu().numpy().astype(np.uint32).reshape(B, N, NW)
    j = np.arange(N)
    got = ((words[:, :, j // 32] >> (j % 32).astype(np.uint32)) & 1).astype(bool)
    return bool((got == _ref_knn_bits(x64, mask64, k, loops).numpy()).all())


# ------------------------------------------------------------------------------------------------------------------ 1. goldens
@pytest.mark.parametrize("name,F", [("knn10", 32), ("knn5nl", 3), ("knn20u", 32)])
def test_sparse_knn_vs_reference_golden(name, F):
    """Forward, dx and all twelve parameter gradients of the three k-NN goldens on the sparse route, as
    test_mplayer_knn_vs_reference_golden holds the dense route to them."""
    from oracle import train_ref as T
    g = load_golden(f"mplayer_{name}_f64.npz")
    k, loops, sm, out = int(g["num_knn"]), bool(g["self_loops"]), bool(g["sum"]), int(g["out"])
    x64, g64 = torch.from_numpy(g["x"]), torch.from_numpy(g["g"])
    mask64 = torch.from_numpy(g["mask"]) if "mask" in g else None
    sd64 = T.init_state_dict(_mplayer_shapes(F, out), seed=int(g["seed"]), dtype=torch.float64)
    assert _sets_agree(x64, mask64, k, loops)
    # slope 1: smooth, against the fp64 oracle
    y, grads = _run_hip(_layer(F, out, k, loops, sm, 1.0, sd64), x64, mask64, g64)
    assert len(grads) == 13
    errs = _errs(y, grads, *_run_oracle(sd64, x64, mask64, g64, k, loops, sm, 1.0))
    print("errs slope 1", name, errs)
    _assert_smooth_bars(errs, name)
    # default slope: forward against the reference's own output, gradients with the fp32 oracle as the kink control
    y, grads = _run_hip(_layer(F, out, k, loops, sm, 0.2, sd64), x64, mask64, g64)
    print("y vs golden", name, rel_err(y, g["y"]))
    assert rel_err(y, g["y"]) < TIGHT
    _, ref = _run_oracle(sd64, x64, mask64, g64, k, loops, sm, 0.2)
    _, c32 = _run_oracle(sd64, x64, mask64, g64, k, loops, sm, 0.2, dt=torch.float32)
    assert rel_err(ref["dx"], g["dx"]) < 1e-9
    assert_grads(grads, ref, TOL, control=c32, what=name)


# --------------------------------------------------------------------------------------------------- 2./3. tile edges, short jets
def _random_case(B, N, F, out, seed, density=None, masks=None):
    from oracle import train_ref as T
    rs = np.random.RandomState(seed)
    x64 = torch.from_numpy(rs.normal(0, 0.5, size=(B, N, F)).astype(np.float32).astype(np.float64))
    g64 = torch.from_numpy(rs.normal(size=(B, N, out)))
    mask64 = None
    if density is not None:
        mask64 = torch.from_numpy((rs.uniform(size=(B, N, 1)) < density).astype(np.float64))
    if masks is not None:
        mask64 = torch.from_numpy(masks)
    sd64 = T.init_state_dict(_mplayer_shapes(F, out), seed=seed + 100, dtype=torch.float64)
    return x64, mask64, g64, sd64


_EDGE_CASES = {  # B, N, k, F, self_loops, mask density
    "N40_k7": (2, 40, 7, 32, True, 0.8),         # two neighbour words, 280 rows: a partial last tile, receivers straddle tiles
    "N150_k20": (2, 150, 20, 32, True, 0.7),     # five words, several receiver blocks
    "k1_loops": (3, 30, 1, 32, True, 0.8),       # every receiver its own (only) sender
    "kNm1_noloops": (2, 9, 8, 32, False, None),  # everyone but oneself
    "N33_k32_mean": (2, 33, 32, 3, False, 0.9),  # a tile per receiver, two words, mean, F = 3
}


@pytest.mark.parametrize("full_blocks", [False, True], ids=["planned", "full_blocks"])
@pytest.mark.parametrize("case", sorted(_EDGE_CASES))
def test_sparse_knn_tile_edges(case, full_blocks, monkeypatch):
    """``full_blocks``: the plan of a launch that has workgroups to spare -- as many receivers per workgroup as fit (about four tiles:
    several tiles per workgroup, receivers straddling them) -- where two jets alone would get a receiver or a tile per workgroup."""
    from mpgan_amd import ops
    B, N, k, F, loops, density = _EDGE_CASES[case]
    if full_blocks:
        monkeypatch.setattr(ops, "NUM_CUS", 1)
        assert ops.knn_plan(B, N, k, True).RW == max(1, min(N, ops.KNN_WG_ROWS // k))
    sm = not case.endswith("mean")
    x64, mask64, g64, sd64 = _random_case(B, N, F, 32, seed=len(case) + N, density=density)
    assert _sets_agree(x64, mask64, k, loops)
    plan = ops.knn_plan(B, N, k, True)
    if case == "N40_k7":
        assert any(n < 32 for _, n in ops.knn_block_tiles(N, k, plan.RW)) and 32 % k != 0
        assert not full_blocks or plan.RW * k > 96       # four tiles on four waves, the last one short
    if case == "N150_k20":
        assert -(-N // plan.RW) > 1
    y, grads = _run_hip(_layer(F, 32, k, loops, sm, 1.0, sd64), x64, mask64, g64)
    errs = _errs(y, grads, *_run_oracle(sd64, x64, mask64, g64, k, loops, sm, 1.0))
    print("errs", case, full_blocks, errs)
    assert all(np.isfinite(v).all() for v in grads.values()) and np.isfinite(y).all()
    _assert_smooth_bars(errs, (case, full_blocks))


@pytest.mark.parametrize("loops", [True, False])
def test_sparse_knn_empty_and_short_jets(loops):
    """The K_knn masks of tests/edge_list_cases.py (an empty jet, a jet of three scattered particles) and jets of the first 3, 11 and
    20 particles at k = 10: the neighbour sets reach into the zero-masked senders, whose rows add exactly nothing."""
    import edge_list_cases as E
    case = E.cases()["K_knn"]
    N, k = case.N, 10
    masks = np.concatenate([E.mask_of(case), np.stack([(np.arange(N) < n).astype(np.float64)[:, None] for n in (3, 11, 20)])])
    B = masks.shape[0]
    x64, mask64, g64, sd64 = _random_case(B, N, 32, 32, seed=31 + int(loops), masks=masks)
    assert _sets_agree(x64, mask64, k, loops)
    y, grads = _run_hip(_layer(32, 32, k, loops, True, 1.0, sd64), x64, mask64, g64)
    assert all(np.isfinite(v).all() for v in grads.values()) and np.isfinite(y).all()
    errs = _errs(y, grads, *_run_oracle(sd64, x64, mask64, g64, k, loops, True, 1.0))
    print("errs", loops, errs)
    _assert_smooth_bars(errs, ("K_knn", loops))


# ----------------------------------------------------------------------------------------------- 4. agreement with the dense route
@pytest.mark.parametrize("B,N,k", [(3, 30, 10), (2, 150, 20)])
def test_sparse_agrees_with_dense_and_repeats_bit_for_bit(B, N, k):
    x64, mask64, g64, sd64 = _random_case(B, N, 32, 32, seed=B * N + k, density=0.8)
    layer = _layer(32, 32, k, True, True, 1.0, sd64)
    yd, gd = _run_hip(layer, x64, mask64, g64, sparse=False)
    ys, gs = _run_hip(layer, x64, mask64, g64, sparse=True)
    ys2, gs2 = _run_hip(layer, x64, mask64, g64, sparse=True)
    errs = _errs(ys, gs, yd, gd)
    print("sparse vs dense", (B, N, k), errs)
    assert errs["y"] < TIGHT
    for kk, e in errs.items():
        if kk != "y":
            assert e < (TOL if (kk == "dx" or kk.startswith("fe.")) else TIGHT), (kk, e)
    # the two routes add a receiver's rows in different orders: no bit identity between them; the sparse route with itself, yes
    assert np.array_equal(ys, ys2) and all(np.array_equal(gs[kk], gs2[kk]) for kk in gs)


# -------------------------------------------------------------------------------------------------------------- 5. dropout exact
@pytest.mark.parametrize("p_drop", [0.5, 0.3])
def test_sparse_knn_dropout_exact(p_drop):
    """The sparse kernels key every draw by the DENSE edge row: ``ops.dropout_mask(B * N * N, width, tag + site, thr)`` describes them,
    gathered along the oracle's own neighbour order."""
    from oracle import train_ref as T
    from mpgan_amd import ops
    B, N, k, F, out = 5, 30, 10, 32, 32
    V = B * N
    sd64 = T.init_state_dict(_mplayer_shapes(F, out), seed=77, dtype=torch.float64)
    rs = np.random.RandomState(5)
    x64 = torch.from_numpy(rs.normal(0, 0.5, size=(B, N, F)).astype(np.float32).astype(np.float64))
    g64 = torch.from_numpy(rs.normal(size=(B, N, out)))
    mask64 = torch.from_numpy((rs.uniform(size=(B, N, 1)) < 0.8).astype(np.float64))
    mask64[:, 0] = 1
    mask64[3] = 0          # a jet without particles
    mask64[4] = 0
    mask64[4, 17] = 1      # a jet with one
    assert _sets_agree(x64, mask64, k, True)
    thr, _ = ops.drop_params(p_drop)
    xs = ((1 - 1e4) * mask64 + 1e4) * x64
    idx = torch.sort(torch.norm(xs.unsqueeze(1) - x64.unsqueeze(2) + 1e-12, dim=3), dim=2)[1][:, :, :k]   # the oracle's own order
    sites = {"e0": ops.TAG_E0, "e1": ops.TAG_E1, "e2": ops.TAG_E2, "n0": ops.TAG_N0, "n1": ops.TAG_N1, "n2": ops.TAG_N2}
    widths = {"e0": 96, "e1": 160, "e2": 192, "n0": 256, "n1": 256, "n2": out}
    for alpha in (1.0, 0.2):
        layer = _layer(F, out, k, True, True, alpha, sd64, p_drop=p_drop)
        layer.train()
        ops.set_seed(4242)
        for p in layer.parameters():
            p.grad = None
        x = x64.float().to(_dev()).requires_grad_(True)
        with knn_sparse():
            y = layer(x, True, mask64.float().to(_dev()))
            tag = ops.last_tag(_dev())
            assert ops.knn_saved(_fused_node(y)) is not None
            (y * g64.float().to(_dev())).sum().backward()
        keeps = {}
        for s, wdt in widths.items():
            if s.startswith("e"):
                dense = ops.dropout_mask(V * N, wdt, tag + sites[s], thr).cpu().double().reshape(B, N, N, wdt)
                keeps[s] = torch.gather(dense, 2, idx.unsqueeze(3).expand(B, N, k, wdt))
            else:
                keeps[s] = ops.dropout_mask(V, wdt, tag + sites[s], thr).cpu().double().reshape(B, N, wdt)
        got = {"dx": x.grad.double().cpu().numpy(), **{kk: p.grad.double().cpu().numpy() for kk, p in layer.named_parameters()}}
        yo, ref = _run_oracle(sd64, x64, mask64, g64, k, True, True, alpha, p=thr / 256.0, keeps=keeps)
        errs = _errs(y.detach().double().cpu().numpy(), got, yo, ref)
        print("errs", p_drop, alpha, errs)
        if alpha == 1.0:
            _assert_smooth_bars(errs, (p_drop, alpha))
            continue
        assert errs["y"] < TIGHT, errs
        _, c32 = _run_oracle(sd64, x64, mask64, g64, k, True, True, alpha, dt=torch.float32, p=thr / 256.0,
                             keeps={s: v.float() for s, v in keeps.items()})
        assert_grads(got, ref, TOL, control=c32, what=(p_drop, alpha))


# ----------------------------------------------------------------------------------------------- 6. no by-products without a backward
def test_sparse_knn_parks_nothing_without_a_backward():
    from mpgan_amd import ops
    B, N, k = 16, 150, 20
    x64, mask64, g64, sd64 = _random_case(B, N, 32, 32, seed=8, density=0.7)
    layer = _layer(32, 32, k, True, True, 0.2, sd64)
    x = x64.float().to(_dev())
    mask = mask64.float().to(_dev())
    plan = ops.knn_plan(B, N, k, True)
    assert plan.parked_bytes == B * N * k * ops.KNN_PARK_ROW_BYTES > 0 and ops.knn_plan(B, N, k, False).parked_bytes == 0
    peaks, ys = {}, {}
    with knn_sparse():
        layer(x, True, mask)   # (warm-up: weight images, allocator pools)
        for mode in ("no_grad", "grad"):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            with torch.no_grad() if mode == "no_grad" else contextlib.nullcontext():
                y = layer(x, True, mask)
            torch.cuda.synchronize()
            peaks[mode] = torch.cuda.max_memory_allocated() - base
            ys[mode] = y.detach().clone()
            assert (y.grad_fn is not None) == (mode == "grad")
            if mode == "grad":
                ks = ops.knn_saved(_fused_node(y))
                assert ks.E1.shape == (B * N * k, 96) and ks.E2.shape == (B * N * k, 160) and ks.sign3.shape == (B * N * k, 6, 2)
                assert sum(t.numel() * t.element_size() for t in ks) == plan.parked_bytes
            del y
    print("peaks", peaks, "parked", plan.parked_bytes)
    assert torch.equal(ys["no_grad"], ys["grad"])
    assert peaks["no_grad"] <= peaks["grad"] - plan.parked_bytes


# ---------------------------------------------------------------------------------------------------------------- 7. captured step
def _knn_train_steps(B, N, k, use_graphs, steps):
    from mpgan_amd import ops, train
    from oracle import train_ref as T
    from oracle.train_ref import synthetic_batch
    dev = torch.device("cuda", torch.cuda.current_device())
    st = ops.dev_state(dev)
    G, D = train.default_mpgan(N, disc_dropout=0.5)
    G.load_state_dict(T.init_state_dict(T.mpgan_param_shapes(True), 41, torch.float32))
    D.load_state_dict(T.init_state_dict(T.mpgan_param_shapes(False), 42, torch.float32))
    for l in (*G.mp_layers, *D.mp_layers):
        l.fully_connected, l.num_knn = False, k
        assert l.fused
    data, labels = synthetic_batch(B, N, seed=3)
    ts = train.TrainStep(G, D, B, N, use_graphs=use_graphs)
    ts.set_batch(data.cuda(), labels.cuda())
    gen = torch.Generator(device="cuda").manual_seed(5)
    ts.fixed_noise = (torch.randn(B, N, 32, device="cuda", generator=gen) * 0.2, torch.randn(B, N, 32, device="cuda", generator=gen) * 0.2)
    ops.set_seed(0x5EED, dev)
    # (the dropout sites of an eager step are numbered anew on every step, a graph keeps those of its capture: the counter is put
    #  back before each eager step and before the capture, as test_gpu_train.py does)
    if use_graphs:
        st.tags = itertools.count(1)
        ts.capture(warmup=0)
    for _ in range(steps):
        if not use_graphs:
            st.tags = itertools.count(1)
        ts.step()
    torch.cuda.synchronize()
    return ts.fD.flat.clone(), ts.fG.flat.clone(), float(ts.D_loss), float(ts.G_loss)


@pytest.mark.parametrize("B,N,k,steps", [(8, 30, 10, 3), (2, 150, 20, 1)])
def test_sparse_knn_captured_step_equals_eager(B, N, k, steps):
    """A k-NN MPGAN (every MPLayer of G and D on the sparse route, dropout 0.5 in D): captured iterations equal eager ones bit for bit
    -- the sparse launches allocate nothing behind a capture and nothing synchronises on the host."""
    from mpgan_amd import ops
    st = ops.dev_state(torch.device("cuda", torch.cuda.current_device()))
    old_log = st.tag_log
    try:
        with knn_sparse():
            st.tag_log = []
            eager = _knn_train_steps(B, N, k, False, steps)
            kinds = [kind for kind, _, _ in st.tag_log]
            graphs = _knn_train_steps(B, N, k, True, steps)
        with knn_sparse(False):
            dense = _knn_train_steps(B, N, k, False, steps)
    finally:
        st.tag_log = old_log
        st.seed_is_default, st.auto_seed_key = True, None
    assert "mplayer" in kinds
    assert torch.equal(eager[0], graphs[0]) and torch.equal(eager[1], graphs[1])
    assert eager[2:] == graphs[2:] and all(np.isfinite(v) for v in eager[2:])
    assert bool(torch.isfinite(eager[0]).all()) and bool(torch.isfinite(eager[1]).all())
    # the option does change the launches: the dense route adds a receiver's rows in another order, so its parameters differ in
    # the last bits (were they equal, the step above would not have been on the sparse route)
    assert not (torch.equal(eager[0], dense[0]) and torch.equal(eager[1], dense[1]))
