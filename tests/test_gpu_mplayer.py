"""GPU parity: HIP path (through the C ABI) vs the CPU oracle, fp32 tolerance 1e-3 relative.

Metric everywhere: max|got - ref| / max|ref| per tensor (conftest.rel_err); the north-star bar is
1e-3, the bf16x3 kernels are expected (and asserted) to sit near 1e-5.
"""
import numpy as np
import pytest
import torch

from conftest import load_golden, rel_err, summarize

pytestmark = pytest.mark.gpu

TOL = 1e-3       # BASELINE.json north_star: "within 1e-3 rel fp32"
TIGHT = 1e-4     # what the three-term split-16-bit products deliver (forward: measured ~1e-6; margin asserted)


def _assert_smooth_bars(errs, what=""):
    """Bars of a case without kinks (slope 1, or margins asserted from the oracle).  The forward and everything the
    three-term products alone produce (the node network's parameter gradients) sit at TIGHT.  The gradients that pass
    through the fused edge backward -- dx and the fe.* parameter gradients -- carry its two-term fp16 products (one
    operand rounded to 11 bits: 2^-12 = 2.4e-4 relative per element, made independent from sender to sender by the
    dither factors): the north-star bar TOL for graphs of a few edges, where nothing averages (measured up to 4e-4 on
    9 edges); <= 9e-5 measured at B = 4 .. 256 (test_mplayer_full_size_smooth pins 2e-4; tests/probe_precision.py)."""
    bad = {k: v for k, v in errs.items() if not v < (TOL if (k == "dx" or k.startswith("fe.")) else TIGHT)}
    assert not bad, (what, bad, errs)


def _dev():
    return torch.device("cuda:0")


def test_library_loaded():
    import mpgan_amd
    lib = mpgan_amd._lib.lib()
    assert lib.mpg_gemm and lib.mpg_edge_fwd and lib.mpg_edge_bwd


@pytest.mark.parametrize("M,N,K", [(64, 64, 32), (7680, 256, 224), (100, 3, 256), (37, 195, 6), (1, 1, 1),
                                   (513, 96, 64)])
def test_gemm_nt(M, N, K):
    from mpgan_amd import ops
    rs = np.random.RandomState(M + N + K)
    x = torch.from_numpy(rs.normal(size=(M, K))).float().to(_dev())
    w = torch.from_numpy(rs.normal(size=(N, K))).float().to(_dev())
    b = torch.from_numpy(rs.normal(size=(N,))).float().to(_dev())
    y = ops.linear_fwd(x, w, b, act=True, alpha=0.2)
    ref = x.double() @ w.double().t() + b.double()
    ref = torch.where(ref > 0, ref, 0.2 * ref)
    assert rel_err(y.cpu().numpy(), ref.cpu().numpy()) < TIGHT


@pytest.mark.parametrize("M,N,K", [(7680, 256, 224), (100, 3, 256), (37, 195, 6), (230400 // 8, 192, 160)])
def test_gemm_bwd_forms(M, N, K):
    from mpgan_amd import ops
    rs = np.random.RandomState(M + N + K + 1)
    dy = torch.from_numpy(rs.normal(size=(M, N))).float().to(_dev())
    w = torch.from_numpy(rs.normal(size=(N, K))).float().to(_dev())
    x = torch.from_numpy(rs.normal(size=(M, K))).float().to(_dev())
    dx = ops.linear_bwd_data(dy, w)
    assert rel_err(dx.cpu().numpy(), (dy.double() @ w.double()).cpu().numpy()) < TIGHT
    dw = ops.linear_bwd_weight(dy, x)
    assert rel_err(dw.cpu().numpy(), (dy.double().t() @ x.double()).cpu().numpy()) < TIGHT


def test_gemm_two_segments_and_slices():
    from mpgan_amd import ops
    rs = np.random.RandomState(3)
    M, K1, K2, N = 300, 192, 3, 256
    a = torch.from_numpy(rs.normal(size=(M, K1))).float().to(_dev())
    x = torch.from_numpy(rs.normal(size=(M, K2))).float().to(_dev())
    w = torch.from_numpy(rs.normal(size=(N, K1 + K2))).float().to(_dev())
    y = ops.linear_fwd(a, w, None, x2=x)
    ref = torch.cat((a, x), 1).double() @ w.double().t()
    assert rel_err(y.cpu().numpy(), ref.cpu().numpy()) < TIGHT
    # column slice of W as the operand (layer-1 factorisation uses W1[:, :F] and W1[:, F:])
    y2 = ops.linear_fwd(x, w, None, w_col0=K1, w_cols=K2)
    assert rel_err(y2.cpu().numpy(), (x.double() @ w[:, K1:].double().t()).cpu().numpy()) < TIGHT


def _mplayer_shapes(F, out, fn=(256, 256)):
    from test_oracle_golden import mplayer_shapes
    return mplayer_shapes(F, out, fn=fn)


def _fused_node(y):
    """The FusedMPLayerFn backward node behind an MPLayer output (its saved tensors hold the forward's by-products)."""
    todo, seen = [y.grad_fn], set()
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        if "FusedMPLayerFn" in type(fn).__name__:
            return fn
        todo.extend(f for f, _ in fn.next_functions)
    raise AssertionError("no FusedMPLayerFn node behind the output")


def _hip_signs(y, B, N):
    """Signs (True = negative) of the pre-activations the HIP forward behind ``y`` saw (``conftest.hip_signs_from``)."""
    from conftest import hip_signs_from
    from mpgan_amd import ops
    saved = ops.mplayer_saved(_fused_node(y))
    return hip_signs_from(saved.ac, saved.stE2, saved.sign3, saved.h1, saved.h2, B, N)


def _sign_disagreements(neg, probe64, mask64):
    """How many pre-activations have another sign than in the fp64 oracle (layers as _hip_signs; fe: unmasked senders)."""
    ref = {"fe1": probe64[0] < 0, "fe2": probe64[1] < 0, "fe3": probe64[2] < 0, "fn1": probe64[3] < 0, "fn2": probe64[4] < 0}
    out = {}
    for k, r in ref.items():
        d = neg[k] != r
        if k.startswith("fe") and mask64 is not None:
            d = d & (mask64.reshape(mask64.shape[0], 1, -1, 1) != 0)
        out[k] = int(d.sum())
    return out


def _run_case(B, N, F, out, use_mask, sum_agg, seed, skip=True, alpha=0.2, control=None, flips=None, conditioned=None, mask=None,
              tensors=None, fn=(256, 256), route=None):
    """HIP MPLayer vs fp64 oracle on the same inputs.  Returns per-tensor
    (max-norm error, fraction of elements off by more than 1e-3 of the max) and the oracle's
    kink margin = min |pre-activation| / max |pre-activation| over all LeakyReLU inputs.
    ``control`` (a dict): also run the oracle in plain fp32 -- the reference's own arithmetic -- on the same inputs
    and store ITS errors / off-fractions against the fp64 run there: the yardstick for kink flips.
    ``flips`` (a dict, needs ``control``): receives the sign-disagreement counts against fp64 of the HIP forward
    (``hip``) and of the fp32 oracle (``fp32``), per layer.
    ``conditioned`` (a dict): receives the errors against the SIGN-CONDITIONED fp64 oracle -- the same oracle with every
    LeakyReLU branch taken as the HIP forward took it (its own sign bits: ``_hip_signs``).  That is the gradient of the
    function the kernels computed: it must match strictly (no kink left to flip), whatever the kink decisions were.
    ``mask`` ([B, N, 1] of 0 / 1, with ``use_mask``): this mask instead of a drawn one -- jets without any particle included.
    ``tensors`` (a dict): receives ``name -> (HIP tensor, oracle tensor)`` as float64 numpy arrays, for checks per jet.
    ``fn``: the node network's hidden widths.  ``route`` (a dict): receives ``fused`` (the layer's own answer) and the C-ABI edge /
    chain entry points its forward (``fwd``) and backward (``bwd``) called, in order."""
    import oracle
    from oracle import train_ref as T
    from mpgan_amd import ops
    from mpgan_amd.mpgan import MPLayer
    ops.OPTIONS["skip_masked"] = skip
    rs = np.random.RandomState(1000 + seed)
    sd64 = T.init_state_dict(_mplayer_shapes(F, out, fn), seed=seed, dtype=torch.float64)
    layer = MPLayer(F, [96, 160, 192], list(fn), out, sum=sum_agg, leaky_relu_alpha=alpha).to(_dev())
    layer.load_state_dict({k: v.float() for k, v in sd64.items()})
    x64 = torch.from_numpy(rs.normal(0, 0.5, size=(B, N, F)))
    g64 = torch.from_numpy(rs.normal(size=(B, N, out)))
    mask64 = None
    if use_mask and mask is not None:
        mask64 = torch.as_tensor(np.asarray(mask), dtype=torch.float64).reshape(B, N, 1).clone()
        assert bool(((mask64 == 0) | (mask64 == 1)).all())
    elif use_mask:
        m = np.zeros((B, N, 1))
        for b in range(B):
            m[b, rs.permutation(N)[: rs.randint(1, N + 1)], 0] = 1
        mask64 = torch.from_numpy(m)
    sdo = {"L." + k: v.clone().requires_grad_(True) for k, v in sd64.items()}
    xo = x64.clone().requires_grad_(True)
    probe = []
    yo = oracle.mplayer_forward(sdo, "L", xo, mask64, sum_agg=sum_agg, alpha=alpha, probe=probe)
    (yo * g64).sum().backward()
    margin = min(float(z.abs().min() / z.abs().max()) for z in probe)
    if control is not None:
        sd32 = {"L." + k: v.float().requires_grad_(True) for k, v in sd64.items()}
        x32 = x64.float().requires_grad_(True)
        probe32 = []
        y32 = oracle.mplayer_forward(sd32, "L", x32, None if mask64 is None else mask64.float(), sum_agg=sum_agg,
                                     alpha=alpha, probe=probe32)
        if flips is not None:
            neg32 = {"fe1": probe32[0] < 0, "fe2": probe32[1] < 0, "fe3": probe32[2] < 0, "fn1": probe32[3] < 0, "fn2": probe32[4] < 0}
            flips["fp32"] = _sign_disagreements(neg32, probe, mask64)
        (y32 * g64.float()).sum().backward()
        cpairs = {"y": (y32.detach(), yo.detach()), "dx": (x32.grad, xo.grad)}
        cpairs.update({k[2:]: (sd32[k].grad, sdo[k].grad) for k in sd32})
        for k, (a, b) in cpairs.items():
            a, b = a.double().numpy(), b.numpy()
            control[k] = (rel_err(a, b), float((np.abs(a - b) > 1e-3 * np.abs(b).max()).mean()))
    x = x64.float().to(_dev()).requires_grad_(True)
    mask = None if mask64 is None else mask64.float().to(_dev())
    calls = _count_calls(ops) if route is not None else None
    try:
        y = layer(x, use_mask, mask)
        if route is not None:
            route["fused"], route["fwd"] = layer.fused, [k for k in calls.names if k in _KEEP]
            del calls.names[:]
        hip_neg = _hip_signs(y, B, N) if (flips is not None or conditioned is not None) else None
        if flips is not None:
            flips["hip"] = _sign_disagreements(hip_neg, probe, mask64)
        (y * g64.float().to(_dev())).sum().backward()
        torch.cuda.synchronize()
        if route is not None:
            route["bwd"] = [k for k in calls.names if k in _KEEP]
    finally:
        if calls is not None:
            calls.restore()
    ops.OPTIONS["skip_masked"] = True
    pairs = {"y": (y.detach(), yo.detach()), "dx": (x.grad, xo.grad)}
    for k, p in layer.named_parameters():
        pairs[k] = (p.grad, sdo["L." + k].grad)
    errs, frac = {}, {}
    for k, (a, b) in pairs.items():
        a = a.double().cpu().numpy()
        b = b.numpy()
        errs[k] = rel_err(a, b)
        frac[k] = float((np.abs(a - b) > 1e-3 * np.abs(b).max()).mean())
        if tensors is not None:
            tensors[k] = (a, b)
    if conditioned is not None:
        sdc = {"L." + k: v.clone().requires_grad_(True) for k, v in sd64.items()}
        xc = x64.clone().requires_grad_(True)
        yc = oracle.mplayer_forward(sdc, "L", xc, mask64, sum_agg=sum_agg, alpha=alpha, signs=hip_neg)
        (yc * g64).sum().backward()
        conditioned["y"] = rel_err(y.detach().double().cpu().numpy(), yc.detach().numpy())
        conditioned["dx"] = rel_err(x.grad.double().cpu().numpy(), xc.grad.numpy())
        for k, p in layer.named_parameters():
            conditioned[k] = rel_err(p.grad.double().cpu().numpy(), sdc["L." + k].grad.numpy())
    return errs, frac, margin


# how the gradient tensors of the kinked cases passed, and the kink decisions seen on the way (test_kink_flips_are_rare)
HATCH = {"outright": 0, "conditioned": 0, "flips_hip": 0, "flips_fp32": 0}


def _assert_gradients_up_to_kink_flips(errs, conditioned, flips, margin, what=""):
    """Gradient bar for the default (kinked) activation.  LeakyReLU' jumps at 0, so an element whose pre-activation
    lies within the forward rounding error of zero may take the other slope -- in the reference's own fp32
    arithmetic just as here.  Two separate questions, two separate bars:
      * the ARITHMETIC: every gradient tensor meets its bar against the fp64 oracle outright, or -- strictly, at the bars of
        the smooth cases -- against the SIGN-CONDITIONED fp64 oracle: the same function with every LeakyReLU branch as the
        HIP forward decided it (``_run_case``).  No tolerance is spent on flips;
      * the DECISIONS: the HIP forward's sign disagreements with fp64, counted from its own sign bits in all five activations,
        stay within 3x of the fp32 oracle's own count on the same input (+3: Poisson noise of a handful of events)."""
    print(what, "errs", errs, "\nconditioned", conditioned, "\nflips", flips, "margin", margin)
    assert conditioned["y"] < TIGHT, conditioned
    bad = {}
    for k in errs:
        if k == "y":
            continue
        if errs[k] < TOL:
            HATCH["outright"] += 1
            continue
        if conditioned[k] < (TOL if (k == "dx" or k.startswith("fe.")) else TIGHT):
            HATCH["conditioned"] += 1
            continue
        bad[k] = (errs[k], conditioned[k])
    n_hip, n_ctl = sum(flips["hip"].values()), sum(flips["fp32"].values())
    HATCH["flips_hip"] += n_hip
    HATCH["flips_fp32"] += n_ctl
    print("passed so far:", HATCH)
    from conftest import record_parity
    grads = [k for k in errs if k != "y"]
    wk = max(grads, key=lambda k: min(errs[k], conditioned[k]))
    record_parity("kink_case", what, tensors=len(grads), outright=sum(errs[k] < TOL for k in grads),
                  conditioned=sum(errs[k] >= TOL for k in grads) - len(bad), failed=len(bad), fwd_err=float(errs["y"]),
                  fwd_err_conditioned=float(conditioned["y"]), worst=wk, err=float(errs[wk]), err_conditioned=float(conditioned[wk]),
                  flips_hip=n_hip, flips_fp32=n_ctl, flips_hip_by_layer=str(flips["hip"]).replace(" ", ""),
                  flips_fp32_by_layer=str(flips["fp32"]).replace(" ", ""), margin=float(margin))
    assert not bad, (bad, margin)
    assert n_hip <= 3 * n_ctl + 3, (flips, margin)


CASES = [  # B, N, F, out, mask, sum
    (4, 30, 32, 32, True, True), (4, 30, 3, 32, True, True), (4, 30, 32, 3, True, True),
    (2, 150, 32, 32, True, True), (3, 30, 32, 32, True, False), (3, 30, 32, 32, False, True),
    (2, 5, 32, 32, True, True), (1, 1, 32, 32, False, True), (2, 33, 32, 32, True, True),
    (2, 32, 3, 32, True, True),
]


@pytest.mark.parametrize("case", CASES)
def test_mplayer_slope1_strict(case):
    """LeakyReLU slope 1 makes the layer smooth: every GEMM orientation, reduction and layout of
    the forward AND backward path must then agree with the fp64 oracle to bf16x3 accuracy."""
    errs, _, _ = _run_case(*case, seed=CASES.index(case), alpha=1.0)
    print("errs", errs)
    _assert_smooth_bars(errs)


@pytest.mark.parametrize("case", CASES)
def test_mplayer_vs_oracle(case):
    """Default slope 0.2.  Forward: strict.  Gradients: LeakyReLU' jumps at 0, so an element
    whose pre-activation lies within the forward rounding error of zero (|z| ~ 1e-5 of the
    scale here, ~1e-7 for the reference's own fp32 arithmetic) may take the other slope; that
    is a property of the function, not an arithmetic error.  Hence: at most a few % of the
    elements of any gradient tensor may differ by more than 1e-3 of its max (each flip touches
    one edge row; here, with a handful of jets, a flipped edge moves the summed gradients by ~1 %,
    at B = 256 by ~1e-4 -- test_mplayer_full_size)."""
    control, flips, cond = {}, {}, {}
    errs, frac, margin = _run_case(*case, seed=CASES.index(case), control=control, flips=flips, conditioned=cond)
    assert errs["y"] < TIGHT, errs
    _assert_gradients_up_to_kink_flips(errs, cond, flips, margin)


WIDTH_CASES = [  # group, B, N, F, fn, out (mask on, sum on)
    # ragged last tiles in every node layer, still the special kernels' k-steps: the node network as the edge launches' epilogue
    ("ragged", 3, 30, 20, (228, 252), 20), ("ragged", 2, 33, 20, (228, 252), 20),
    # none of the special kernels' shapes: mpg_edge_fwd_fn declines, the node network runs on mpg_chain's general kernel
    ("general", 3, 30, 64, (128, 64), 64), ("general", 2, 33, 64, (128, 64), 64), ("general", 2, 5, 64, (128, 64), 64),
    ("general", 3, 30, 6, (250, 131), 7),    # widths that are no multiples of 4
    # a layer input beyond mpg_chain's 256 columns: un-fused
    ("unfused", 2, 5, 128, (256, 256), 32), ("unfused", 2, 5, 32, (512, 256), 32), ("unfused", 2, 5, 32, (256, 256), 300),
]
_WIDTH_IDS = ["%s-B%d-N%d-F%d-fn%d-%d-out%d" % (g, B, N, F, fn[0], fn[1], out) for g, B, N, F, fn, out in WIDTH_CASES]
_default_routes = {}


def _default_route(B, N):
    """The entry points a default-width layer (32, [256, 256], 32) calls at this size, forward and backward."""
    if (B, N) not in _default_routes:
        route = {}
        _run_case(B, N, 32, 32, True, True, seed=0, alpha=1.0, route=route)
        _default_routes[(B, N)] = route
    return _default_routes[(B, N)]


def _follows(names, first, then):
    return any(a == first and b == then for a, b in zip(names, names[1:]))


def _assert_width_route(group, B, N, route):
    """``MPLayer.fused`` and the launches of one WIDTH_CASES run: the ragged widths stay on the epilogue kernels exactly as the default
    widths do at that size; the other fused widths fall back inside the fused route to mpg_edge_fwd + mpg_chain; beyond the chain's
    limits nothing of the fused route runs."""
    assert route["fused"] == (group != "unfused"), route
    if group == "ragged":
        ref = _default_route(B, N)
        assert route["fwd"] == ref["fwd"] and route["bwd"] == ref["bwd"], (route, ref)
        assert "mpg_edge_fwd_fn" in route["fwd"] and "mpg_edge_fwd" not in route["fwd"], route
        assert ("mpg_edge_bwd_fn" in route["bwd"]) == (N == 30) and ("mpg_edge_bwd" in route["bwd"]) == (N != 30), route
    elif group == "general":
        assert _follows(route["fwd"], "mpg_edge_fwd", "mpg_chain"), route   # (mpg_edge_fwd_fn is asked first and answers MPG_FN_NA)
    else:
        assert not route["fwd"] and not route["bwd"], route   # (LinearNet's launches are mpg_gemm)


@pytest.mark.parametrize("case", WIDTH_CASES, ids=_WIDTH_IDS)
def test_mplayer_other_widths_slope1_strict(case, monkeypatch):
    """``test_mplayer_slope1_strict`` at node-network widths other than [256, 256] -> 3 / 5 / 32, and their routes.  One sender chunk
    per jet (at these batch sizes the plan would cut three): the form in which both epilogue kernels run -- the ticketed chunks are
    what ``test_mplayer_other_widths_vs_oracle`` takes."""
    group, B, N, F, fn, out = case
    monkeypatch.setenv("MPG_FORCE_SC", "1")
    route = {}
    errs, _, _ = _run_case(B, N, F, out, True, True, seed=20 + WIDTH_CASES.index(case), alpha=1.0, fn=fn, route=route)
    print("errs", errs, "\nroute", route)
    _assert_width_route(group, B, N, route)
    _assert_smooth_bars(errs, case)


@pytest.mark.parametrize("case", WIDTH_CASES, ids=_WIDTH_IDS)
def test_mplayer_other_widths_vs_oracle(case):
    """``test_mplayer_vs_oracle`` at those widths: forward strict, gradients up to kink flips (the fused layers keep the sign words that
    check needs; the un-fused ones are held to the forward bar here and to the smooth bars above)."""
    group, B, N, F, fn, out = case
    seed = 40 + WIDTH_CASES.index(case)
    if group == "unfused":
        errs, _, _ = _run_case(B, N, F, out, True, True, seed=seed, fn=fn)
        assert errs["y"] < TIGHT, errs
        return
    control, flips, cond = {}, {}, {}
    errs, frac, margin = _run_case(B, N, F, out, True, True, seed=seed, control=control, flips=flips, conditioned=cond, fn=fn)
    assert errs["y"] < TIGHT, errs
    _assert_gradients_up_to_kink_flips(errs, cond, flips, margin, what=case)


@pytest.mark.parametrize("case", [(4, 30, 32, 32, True, True), (3, 30, 3, 32, True, False), (2, 33, 32, 32, False, True)])
def test_mplayer_plain_relu(case):
    """alpha = 0 (plain ReLU): the slope of the negative side is exactly 0, which the kernels get from sign bits
    (v_max(v, -0.0) must keep the sign of a negative pre-activation for the dZ2 gate, edge_bwd.hip).  Forward
    strict; gradients within the bar up to the kink flips fp32 shows on the same input."""
    control, flips, cond = {}, {}, {}
    errs, frac, margin = _run_case(*case, seed=77 + case[0], alpha=0.0, control=control, flips=flips, conditioned=cond)
    assert errs["y"] < TIGHT, errs
    _assert_gradients_up_to_kink_flips(errs, cond, flips, margin)


def test_kink_flips_are_rare():
    """Over the kinked cases above (default slope, plain ReLU): how the gradient tensors passed, and the kink decisions of the
    HIP forward against the fp32 oracle's in total (3x + 10)."""
    n = HATCH["outright"] + HATCH["conditioned"]
    print("gradient tensors of the kinked cases:", HATCH)
    from conftest import record_parity
    record_parity("HATCH", "kinked MPLayer cases of this session, in total", **HATCH)
    if n < 100:
        pytest.skip("the kinked cases did not run in this session")
    assert HATCH["flips_hip"] <= 3 * HATCH["flips_fp32"] + 10, HATCH


def test_mplayer_plain_relu_strict_when_away_from_the_kink():
    found = 0
    for seed in range(300, 360):
        for case in ((1, 4, 32, 32, True, True), (1, 5, 3, 32, False, True)):
            errs, _, margin = _run_case(*case, seed=seed, alpha=0.0)
            if margin < 5e-5:
                continue
            found += 1
            _assert_smooth_bars(errs, (case, seed, margin))
    assert found >= 5, found


def test_mplayer_small_strict_gradients():
    """Small graphs whose every pre-activation is verifiably away from the kink
    (margin asserted from the fp64 oracle): gradients must then match strictly."""
    found = 0
    for seed in range(200, 260):
        for case in ((1, 4, 32, 32, True, True), (1, 5, 3, 32, False, True), (1, 3, 32, 3, True, False)):
            errs, _, margin = _run_case(*case, seed=seed)
            if margin < 5e-5:
                continue
            found += 1
            _assert_smooth_bars(errs, (case, seed, margin))
    assert found >= 5, found


def test_mplayer_noskip():
    errs, _, _ = _run_case(4, 30, 32, 32, True, True, seed=42, skip=False, alpha=1.0)
    _assert_smooth_bars(errs)


@pytest.mark.parametrize("name,F,out,ci", [("g0", 32, 32, 0), ("d0", 3, 32, 1)])
def test_mplayer_vs_reference_golden(name, F, out, ci):
    """Directly against outputs captured from the reference implementation (fp32 goldens)."""
    from oracle import train_ref as T
    from mpgan_amd.mpgan import MPLayer
    g = load_golden(f"mplayer_{name}_f32.npz")
    layer = MPLayer(F, [96, 160, 192], [256, 256], out).to(_dev())
    layer.load_state_dict(T.init_state_dict(_mplayer_shapes(F, out), seed=ci, dtype=torch.float32))
    x = torch.from_numpy(g["x"]).to(_dev()).requires_grad_(True)
    y = layer(x, True, torch.from_numpy(g["mask"]).to(_dev()))
    (y * torch.from_numpy(g["g"]).to(_dev())).sum().backward()
    assert rel_err(y.detach().cpu().numpy(), g["y"]) < TIGHT
    # yardstick: the reference's fp32 run against its own fp64 run on these inputs (both are goldens)
    g64 = load_golden(f"mplayer_{name}_f64.npz")
    off = lambda a, b: float((np.abs(a - b) > 1e-3 * np.abs(b).max()).mean())
    ctrl = off(g["dx"].astype(np.float64), g64["dx"])
    ours = off(x.grad.cpu().numpy().astype(np.float64), g64["dx"])
    print(f"dx off-fraction vs fp64 golden: fp32 reference {ctrl:.2e}, HIP {ours:.2e}")
    assert ours <= max(3 * ctrl, 2.0 / (x.shape[0] * x.shape[1])), (ours, ctrl)
    for k, p in layer.named_parameters():   # parameter gradients: summaries (sum, l2, 64 samples) of the fp64 golden
        from conftest import summarize
        e = rel_err(summarize(k, p.grad), g64["grad__" + k])
        c = rel_err(g["grad__" + k], g64["grad__" + k])
        assert e < max(TOL, 3 * c), (k, e, c)


def _ref_knn_bits(x, mask, k, self_loops):
    """Neighbour sets as the reference picks them (mpgan/model.py:319-381), as a boolean [B, N(i), N(j)] matrix."""
    B, N, _ = x.shape
    xs = x if mask is None else ((1 - 1e4) * mask + 1e4) * x
    d = torch.norm(xs.unsqueeze(1) - x.unsqueeze(2) + 1e-12, dim=3)
    first = 0 if self_loops else 1
    idx = torch.sort(d, dim=2)[1][:, :, first:first + k]
    m = torch.zeros(B, N, N, dtype=torch.bool)
    m.scatter_(2, idx, True)
    return m


@pytest.mark.parametrize("name,F", [("knn10", 32), ("knn5nl", 3), ("knn20u", 32)])
def test_mplayer_knn_vs_reference_golden(name, F):
    """fully_connected=False: the neighbour sets (mpg_knn_sets) are exactly the reference's, and the fused layer with the
    sets as a per-edge factor reproduces the reference's gather / fe / sum (or mean over k) forward and backward."""
    from oracle import train_ref as T
    from conftest import summarize
    from mpgan_amd import ops
    from mpgan_amd.mpgan import MPLayer
    g = load_golden(f"mplayer_{name}_f64.npz")
    k, loops, sm, out = int(g["num_knn"]), bool(g["self_loops"]), bool(g["sum"]), int(g["out"])
    x64 = torch.from_numpy(g["x"])
    mask64 = torch.from_numpy(g["mask"]) if "mask" in g else None
    x = x64.float().to(_dev()).requires_grad_(True)
    mask = None if mask64 is None else mask64.float().to(_dev())
    B, N, _ = x.shape
    bits = ops.knn_sets(x.detach(), mask, k, loops).cpu().numpy().astype(np.uint32).reshape(B, N)   # N <= 32: one word
    got = ((bits[:, :, None] >> np.arange(N, dtype=np.uint32)[None, None, :]) & 1).astype(bool)
    ref = _ref_knn_bits(x64, mask64, k, loops).numpy()
    # zero-masked padded senders coincide after the 1e4 scaling only if their features are identical (not the case for
    # these random features), so the sets must agree exactly
    assert (got == ref).all() and (got.sum(2) == k).all()
    for alpha, strict in ((1.0, True), (0.2, False)):
        sd64 = T.init_state_dict(_mplayer_shapes(F, out), seed=int(g["seed"]), dtype=torch.float64)
        layer = MPLayer(F, [96, 160, 192], [256, 256], out, sum=sm, fully_connected=False, num_knn=k, self_loops=loops,
                        leaky_relu_alpha=alpha).to(_dev())
        layer.load_state_dict({kk: v.float() for kk, v in sd64.items()})
        xx = x64.float().to(_dev()).requires_grad_(True)
        y = layer(xx, mask is not None, mask)
        (y * torch.from_numpy(g["g"]).float().to(_dev())).sum().backward()
        if strict:  # slope 1: smooth, against the oracle's kNN branch (bars: _assert_smooth_bars)
            import oracle
            sdo = {"L." + kk: v.clone().requires_grad_(True) for kk, v in sd64.items()}
            xo = x64.clone().requires_grad_(True)
            yo = oracle.mplayer_forward(sdo, "L", xo, mask64, sum_agg=sm, alpha=1.0, knn=(k, loops))
            (yo * torch.from_numpy(g["g"])).sum().backward()
            errs = {"y": rel_err(y.detach().cpu().numpy(), yo.detach().numpy()), "dx": rel_err(xx.grad.cpu().numpy(), xo.grad.numpy())}
            errs.update({kk: rel_err(p.grad.cpu().numpy(), sdo["L." + kk].grad.numpy()) for kk, p in layer.named_parameters()})
            _assert_smooth_bars(errs, name)
        else:       # default slope: forward against the reference's own fp64 output; gradients against the fp64 oracle
            # (pinned to that golden at 1e-10, test_oracle_golden.py) with the fp32 oracle as the control for kink flips
            import oracle
            assert rel_err(y.detach().cpu().numpy(), g["y"]) < TIGHT
            runs = {}
            for dt in (torch.float64, torch.float32):
                sdo = {"L." + kk: v.detach().clone().to(dt).requires_grad_(True) for kk, v in sd64.items()}
                xo = x64.detach().clone().to(dt).requires_grad_(True)
                yo = oracle.mplayer_forward(sdo, "L", xo, None if mask64 is None else mask64.to(dt), sum_agg=sm, alpha=alpha, knn=(k, loops))
                (yo * torch.from_numpy(g["g"]).to(dt)).sum().backward()
                runs[dt] = {"dx": xo.grad.double().numpy(), **{kk[2:]: v.grad.double().numpy() for kk, v in sdo.items()}}
            ref, c32 = runs[torch.float64], runs[torch.float32]
            assert rel_err(ref["dx"], g["dx"]) < 1e-9   # the oracle's kNN branch IS the reference's here
            got = {"dx": xx.grad.double().cpu().numpy(), **{kk: p.grad.double().cpu().numpy() for kk, p in layer.named_parameters()}}
            # (per tensor: the 1e-3 bar, or 3x what the fp32 oracle itself shows against fp64 on this input -- no wider hatch)
            from conftest import assert_grads
            assert_grads(got, ref, TOL, control=c32, what=name)


def test_mplayer_knn_n150_and_dropout():
    """Five receiver blocks / five neighbour words per row, sender chunks, dropout on: runs, finite, and the graph only
    matters through the sets (k = N with self loops == fully connected, bit for bit)."""
    from mpgan_amd.mpgan import MPLayer
    torch.manual_seed(0)
    B, N, F = 2, 150, 32
    x = (torch.randn(B, N, F, device=_dev()) * 0.5).requires_grad_(True)
    mask = (torch.rand(B, N, 1, device=_dev()) < 0.7).float()
    up = torch.randn(B, N, 32, device=_dev())
    full = MPLayer(F, [96, 160, 192], [256, 256], 32).to(_dev())
    knn_all = MPLayer(F, [96, 160, 192], [256, 256], 32, fully_connected=False, num_knn=N, self_loops=True).to(_dev())
    knn_all.load_state_dict(full.state_dict())
    outs = []
    for lay in (full, knn_all):
        x.grad = None
        y = lay(x, True, mask)
        (y * up).sum().backward()
        outs.append((y.detach().clone(), x.grad.clone(), lay.fe.net[1].weight.grad.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    lay = MPLayer(F, [96, 160, 192], [256, 256], 32, fully_connected=False, num_knn=20, dropout_p=0.5).to(_dev())
    lay.train()
    y = lay(x, True, mask)
    (y * up).sum().backward()
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(lay.fe.net[2].weight.grad).all())


def test_mplayer_full_size_smooth():
    """BASELINE config 2 (B = 256, N = 30, F = 32) with slope 1 (no kink): every product, reduction and layout of
    forward and backward at full size, strict."""
    errs, _, _ = _run_case(256, 30, 32, 32, True, True, seed=7, alpha=1.0)
    print("full-size smooth errors", errs)
    _assert_smooth_bars(errs)
    # over the ~1.4e5 edges of this batch the independent roundings of the two-term products average out: weight
    # gradients of the edge network well inside the bar
    assert max(v for k, v in errs.items() if k == "dx" or k.startswith("fe.")) < 2e-4, errs


def test_mplayer_full_size():
    """BASELINE config 2 with the default slope, three seeds.  Forward strict.  Gradients: LeakyReLU' jumps at 0, and
    a pre-activation within rounding of zero takes the other slope -- in the reference's own fp32 arithmetic as well
    (against fp64 the fp32 oracle disagrees on a few signs per layer at this size, and one such sign in the node
    network moves whole rows of dx and columns of the weight gradients by ~1e-2: fp32 itself shows 3e-3 on dx and
    1e-3 on a bias for seed 8).  So the test pins
      (1) the RATE of such disagreements: counted directly from the signs the HIP forward saw (a|c terms, the packed
          sign words, the node network's outputs) against the fp64 oracle, it must stay within 3x of the fp32
          oracle's own count (+10 for Poisson noise) -- a kernel whose forward were less accurate than fp32 fails;
      (2) the arithmetic, flips apart: every gradient tensor of EVERY seed within the bar of the fp64 oracle outright or,
          strictly (2e-4 on dx and the edge network), of the SIGN-CONDITIONED fp64 oracle -- the same function with every
          LeakyReLU branch as the HIP forward took it (``_run_case``); never a gross error (5e-2), and dx -- where one
          flipped sign in the node network shows at ~1e-2 in that node's rows, for fp32 as for the kernels -- with less
          than 1e-3 of its elements off by more than 1e-3."""
    seeds = (7, 8, 9)
    n_hip, n_ctl = {}, {}
    for seed in seeds:
        control, flips, cond = {}, {}, {}
        errs, frac, margin = _run_case(256, 30, 32, 32, True, True, seed=seed, control=control, flips=flips, conditioned=cond)
        print("full-size seed", seed, "errors", errs, "\nfrac>1e-3", frac, "margin", margin, "\nfp32 control (err, frac)",
              control, "\nsign disagreements vs fp64", flips, "\nagainst the sign-conditioned oracle", cond)
        assert errs["y"] < TIGHT
        assert max(errs.values()) < 5e-2, errs
        assert frac["dx"] < 1e-3, frac["dx"]
        # EVERY seed, every tensor: the bar outright or, strictly, against the oracle with the HIP forward's own kink decisions
        for k in errs:
            if k == "y":
                continue
            assert errs[k] < TOL or cond[k] < (TOL if (k == "dx" or k.startswith("fe.")) else TIGHT), (seed, k, errs[k], cond[k])
        # at this size the independent roundings average out: against the conditioned oracle the edge network's gradients
        # sit where the smooth full-size test has them
        assert max(v for k, v in cond.items() if k == "dx" or k.startswith("fe.")) < 2e-4, cond
        from conftest import record_parity
        grads = [k for k in errs if k != "y"]
        wk = max(grads, key=lambda k: min(errs[k], cond[k]))
        record_parity("kink_case", ("full size B=256 N=30", seed), tensors=len(grads), outright=sum(errs[k] < TOL for k in grads),
                      conditioned=sum(errs[k] >= TOL for k in grads), failed=0, fwd_err=float(errs["y"]),
                      fwd_err_conditioned=float(cond["y"]), worst=wk, err=float(errs[wk]), err_conditioned=float(cond[wk]),
                      worst_conditioned_fe_dx=float(max(v for k, v in cond.items() if k == "dx" or k.startswith("fe."))),
                      flips_hip=sum(flips["hip"].values()), flips_fp32=sum(flips["fp32"].values()),
                      flips_hip_by_layer=str(flips["hip"]).replace(" ", ""), flips_fp32_by_layer=str(flips["fp32"]).replace(" ", ""),
                      margin=float(margin))
        for k in flips["hip"]:
            n_hip[k] = n_hip.get(k, 0) + flips["hip"][k]
            n_ctl[k] = n_ctl.get(k, 0) + flips["fp32"][k]
    print("sign disagreements summed over seeds: HIP", n_hip, "fp32 oracle", n_ctl)
    assert sum(n_hip.values()) <= 3 * sum(n_ctl.values()) + 10, (n_hip, n_ctl)


def test_mplayer_gradient_units_across_binades_and_zero_jets():
    """One launch whose jets' upstream gradients span 2^-20 .. 2^+20 and include jets with an upstream gradient of exactly
    zero (hinge-inactive jets look like that), B = 64, slope 1 (no kink: what is measured is the gradient arithmetic).
    The data-gradient kernel works in a unit per workgroup (2^-e of its own receivers' upstream gradient) and
    ``mpg_edge_dw`` brings the parked dZ2 of all blocks to ONE unit per launch (the minimum exponent, ``gexp``):
      * dx of EVERY jet within the bar relative to that jet's own largest entry -- a jet 2^-40 below the launch's largest
        keeps its full precision -- and exactly zero, finite, for the zero jets;
      * every parameter gradient within the bar of its maximum against the fp64 oracle: the small jets' contributions may
        vanish in the launch-wide unit (they are below 2^-24 of the sum), the large ones' may not be disturbed."""
    import oracle
    from oracle import train_ref as T
    from mpgan_amd.mpgan import MPLayer
    B, N, F, out = 64, 30, 32, 32
    rs = np.random.RandomState(4242)
    sd64 = T.init_state_dict(_mplayer_shapes(F, out), seed=5, dtype=torch.float64)
    layer = MPLayer(F, [96, 160, 192], [256, 256], out, sum=True, leaky_relu_alpha=1.0).to(_dev())
    layer.load_state_dict({k: v.float() for k, v in sd64.items()})
    x64 = torch.from_numpy(rs.normal(0, 0.5, size=(B, N, F)))
    m = np.zeros((B, N, 1))
    for b in range(B):
        m[b, rs.permutation(N)[: rs.randint(4, N + 1)], 0] = 1
    mask64 = torch.from_numpy(m)
    expo = rs.randint(-20, 21, size=B)
    expo[:4] = (20, -20, 19, -19)
    scale = 2.0 ** expo
    scale[4:10] = 0.0                     # six jets with no upstream gradient at all
    g64 = torch.from_numpy(rs.normal(size=(B, N, out)) * scale[:, None, None])
    sdo = {"L." + k: v.clone().requires_grad_(True) for k, v in sd64.items()}
    xo = x64.clone().requires_grad_(True)
    yo = oracle.mplayer_forward(sdo, "L", xo, mask64, sum_agg=True, alpha=1.0)
    (yo * g64).sum().backward()
    x = x64.float().to(_dev()).requires_grad_(True)
    y = layer(x, True, mask64.float().to(_dev()))
    (y * g64.float().to(_dev())).sum().backward()
    torch.cuda.synchronize()
    dx, dxo = x.grad.double().cpu().numpy(), xo.grad.numpy()
    assert np.isfinite(dx).all()
    worst = 0.0
    for b in range(B):
        if scale[b] == 0.0:
            assert np.abs(dx[b]).max() == 0.0, b
        else:
            worst = max(worst, rel_err(dx[b], dxo[b]))
            assert rel_err(dx[b], dxo[b]) < TOL, (b, int(expo[b]), rel_err(dx[b], dxo[b]))
    errs = {k: rel_err(p.grad.double().cpu().numpy(), sdo["L." + k].grad.numpy()) for k, p in layer.named_parameters()}
    print("gradient units across 2^-20 .. 2^20: worst per-jet dx error", worst, "parameter gradients", errs)
    for k, p in layer.named_parameters():
        assert bool(torch.isfinite(p.grad).all()), k
    _assert_smooth_bars(dict(errs, dx=worst))


_DROPOUT_CASES = [pytest.param(p, F, (256, 256), 32, a, id="%s-%s-%s" % (p, F, a))
                  for p, F, a in [(0.5, 32, 1.0), (0.3, 32, 1.0), (0.5, 3, 1.0), (0.3, 3, 1.0), (0.5, 3, 0.2), (0.5, 32, 0.2), (0.3, 3, 0.2)]]
# other widths: the node network on mpg_chain's general kernel (its own choice of dropout words), both modes
_DROPOUT_CASES += [pytest.param(p, 64, (128, 64), 64, 1.0, id="%s-64-128-64-64-1.0" % p) for p in (0.5, 0.3)]


@pytest.mark.parametrize("p_drop,F,fn,out,alpha", _DROPOUT_CASES)
def test_mplayer_dropout_exact(p_drop, F, fn, out, alpha):
    """Dropout on (training mode): the kernels' counter-based keep masks are dumped with
    mpg_dropout_mask and fed to the oracle, so forward AND backward can be compared exactly
    (p = 0.5 takes the one-bit fast path, p = 0.3 the byte-threshold path).  F = 3 is the discriminator's first layer -- the
    layer that carries dropout in the bench -- with x the strided 3-column view of [B, N, 4] jets it gets there.  Slope 1
    keeps the layer smooth (strict bars); the default slope 0.2 is held to the 1e-3 bar with the oracle's own fp32
    evaluation -- same masks -- as the kink-flip control."""
    import oracle
    from conftest import assert_grads
    from oracle import train_ref as T
    from mpgan_amd import ops
    from mpgan_amd.mpgan import MPLayer
    B, N = 5, 30   # (three drawn masks, a jet without any particle, a jet with one)
    V = B * N
    sd64 = T.init_state_dict(_mplayer_shapes(F, out, fn), seed=77, dtype=torch.float64)
    layer = MPLayer(F, [96, 160, 192], list(fn), out, leaky_relu_alpha=alpha, dropout_p=p_drop).to(_dev())
    assert layer.fused
    layer.load_state_dict({k: v.float() for k, v in sd64.items()})
    layer.train()
    rs = np.random.RandomState(5)
    x64 = torch.from_numpy(rs.normal(0, 0.5, size=(B, N, F)))
    g64 = torch.from_numpy(rs.normal(size=(B, N, out)))
    mask64 = torch.from_numpy((rs.uniform(size=(B, N, 1)) < 0.8).astype(np.float64))
    mask64[:, 0] = 1
    # an empty jet and a one-particle jet: workgroups of the dropout kernels without a sender (three sender chunks at this size)
    mask64[3] = 0
    mask64[4] = 0
    mask64[4, 17] = 1
    assert ops.edge_plan(B, N, mask=True, need_grad=True).SC > 1
    ops.set_seed(4242)
    if F == 3:   # as MPDiscriminator hands it over: a column slice of the [B, N, 4] batch
        x4 = torch.cat([x64.float(), mask64.float() - 0.5], 2).to(_dev()).requires_grad_(True)
        x = x4[..., :3]
        assert not x.is_contiguous()
    else:
        x4 = x = x64.float().to(_dev()).requires_grad_(True)
    y = layer(x, True, mask64.float().to(_dev()))
    tag = ops.last_tag(_dev())
    (y * g64.float().to(_dev())).sum().backward()
    dx = x4.grad[..., :F]
    thr, scale = ops.drop_params(p_drop)
    widths = {"e%d" % i: l.out_features for i, l in enumerate(layer.fe.net)}
    widths.update({"n%d" % i: l.out_features for i, l in enumerate(layer.fn.net)})
    assert widths == {"e0": 96, "e1": 160, "e2": 192, "n0": fn[0], "n1": fn[1], "n2": out}
    sites = {"e0": ops.TAG_E0, "e1": ops.TAG_E1, "e2": ops.TAG_E2, "n0": ops.TAG_N0, "n1": ops.TAG_N1, "n2": ops.TAG_N2}
    keeps = {}
    for k, wdt in widths.items():
        rows = V * N if k.startswith("e") else V
        m = ops.dropout_mask(rows, wdt, tag + sites[k], thr).cpu().double()
        keeps[k] = m.reshape(B, N, N, wdt) if k.startswith("e") else m.reshape(B, N, wdt)
        frac, q = float(m.mean()), 1 - thr / 256.0
        # statistical sanity of the counter hash: within 5 sigma of the keep probability (the site tags, hence the
        # realisations, depend on how many fused ops ran before this test)
        assert abs(frac - q) < max(0.01, 5 * (q * (1 - q) / m.numel()) ** 0.5), (k, frac)
    sdo = {"L." + k: v.clone().requires_grad_(True) for k, v in sd64.items()}
    xo = x64.clone().requires_grad_(True)
    yo = oracle.mplayer_forward(sdo, "L", xo, mask64, alpha=alpha, p=thr / 256.0, keeps=keeps)
    (yo * g64).sum().backward()
    errs = {"y": rel_err(y.detach().cpu().numpy(), yo.detach().numpy()), "dx": rel_err(dx.cpu().numpy(), xo.grad.numpy())}
    errs.update({k: rel_err(p.grad.cpu().numpy(), sdo["L." + k].grad.numpy()) for k, p in layer.named_parameters()})
    print("errs", errs)
    if alpha == 1.0:
        _assert_smooth_bars(errs, (p_drop, F))
        return
    assert errs["y"] < TIGHT, errs
    sd32 = {"L." + k: v.float().requires_grad_(True) for k, v in sd64.items()}
    x32 = x64.float().requires_grad_(True)
    y32 = oracle.mplayer_forward(sd32, "L", x32, mask64.float(), alpha=alpha, p=thr / 256.0, keeps={k: v.float() for k, v in keeps.items()})
    (y32 * g64.float()).sum().backward()
    got = {"dx": dx.double().cpu().numpy(), **{k: p.grad.double().cpu().numpy() for k, p in layer.named_parameters()}}
    ref = {"dx": xo.grad.numpy(), **{k: sdo["L." + k].grad.numpy() for k, _ in layer.named_parameters()}}
    ctl = {"dx": x32.grad.double().numpy(), **{k: sd32["L." + k].grad.double().numpy() for k, _ in layer.named_parameters()}}
    assert_grads(got, ref, TOL, control=ctl, what=(p_drop, F, alpha))


def _option_cases():
    from gen_golden import OPTION_CASES
    return OPTION_CASES


# distance column; folded coordinate differences + distance; two row-tiled conditioning columns; k-NN graph with its distances
FUSED_OPTION_CASES = ("ef", "efc", "cl", "knnef")


@pytest.mark.parametrize("route", ["fused", "edges"])
@pytest.mark.parametrize("case", _option_cases(), ids=lambda c: c[0])
def test_mplayer_options_vs_reference_golden(case, route):
    """MPLayer's non-default options -- edge features, conditioning columns tiled as the reference tiles them, k-NN with
    distances, other layer widths -- against the reference's own outputs and gradients (tests/golden/mplayer_opt_*), on both
    routes: the fused kernels (one scalar per edge and option, each with its column of fe.net.0.weight; coordinate
    differences folded into the node terms) where they cover the case, and the un-fused route (edge matrix built as the
    reference builds it), which every case can take."""
    from conftest import option_case_shapes
    from oracle import train_ref as T
    from mpgan_amd.mpgan import MPLayer
    name, B, N, F, out, kw = case
    g = load_golden(f"mplayer_opt_{name}_f64.npz")
    ctor = {k: v for k, v in kw.items() if k not in ("fe", "fn", "use_mask")}
    layer = MPLayer(F, kw.get("fe", [96, 160, 192]), kw.get("fn", [256, 256]), out, **ctor).cuda()
    assert layer.fused == (name in FUSED_OPTION_CASES)
    if route == "fused" and not layer.fused:
        pytest.skip("outside the fused kernels (other widths)")
    if route == "edges":
        layer.fused = False
    layer.load_state_dict(T.init_state_dict(option_case_shapes(F, out, kw), seed=int(g["seed"]), dtype=torch.float32))
    x = torch.from_numpy(g["x"]).float().cuda().requires_grad_(True)
    mask = torch.from_numpy(g["mask"]).float().cuda() if "mask" in g else None
    labels = torch.from_numpy(g["labels"]).float().cuda().requires_grad_(True)
    njp = torch.from_numpy(g["njp"]).float().cuda().requires_grad_(True)
    y = layer(x, mask is not None, mask, labels, njp)
    (y * torch.from_numpy(g["g"]).float().cuda()).sum().backward()
    assert rel_err(y.detach().cpu().numpy(), g["y"]) < TIGHT, name
    assert rel_err(x.grad.cpu().numpy(), g["dx"]) < TOL, name
    if layer.clabels or layer.mask_fne_np:
        # the conditioning inputs get their FULL gradient on either route: through their columns of the edge network (per-edge
        # gathers) and through the columns appended to the node network's input (mpgan/model.py:247-253, :270-276) -- against
        # the oracle (which the goldens pin on this very case)
        from conftest import option_case_oracle_kwargs
        from oracle.mpgan_ref import mplayer_forward_general
        sd64 = {"L." + k: v for k, v in T.init_state_dict(option_case_shapes(F, out, kw), seed=int(g["seed"]), dtype=torch.float64).items()}
        lab64 = torch.from_numpy(g["labels"]).requires_grad_(True)
        njp64 = torch.from_numpy(g["njp"]).requires_grad_(True)
        yo = mplayer_forward_general(sd64, "L", torch.from_numpy(g["x"]), None if mask is None else torch.from_numpy(g["mask"]),
                                     lab64, njp64, **option_case_oracle_kwargs(kw))
        (yo * torch.from_numpy(g["g"])).sum().backward()
        if layer.clabels:
            assert rel_err(labels.grad.cpu().numpy(), lab64.grad.numpy()) < TOL, name
        if layer.mask_fne_np:
            assert rel_err(njp.grad.cpu().numpy(), njp64.grad.numpy()) < TOL, name
    from conftest import summary_err
    for k, p in layer.named_parameters():   # (the summaries' sum entry against the tensor's l1: conftest.summary_err)
        assert summary_err(k, p.grad, g["grad__" + k]) < TOL, (name, k)


@pytest.mark.parametrize("alpha", [1.0, 0.2])
@pytest.mark.parametrize("p_drop,use_mask,N", [(0.0, True, 30), (0.5, True, 30), (0.3, False, 30), (0.5, True, 40)])
def test_edge_scalars_separable_case_equals_node_features(p_drop, use_mask, N, alpha):
    """The edge-scalar kernels in every dropout mode, against the plain kernels: an edge scalar of the form u_i + v_j times a
    column w is  a_i + c_j + (u_i + v_j) w = (a_i + u_i w) + (c_j + v_j w), i.e. the default layer on nodes with two more
    features [x, u, v] and fe.net.0.weight = [W1a | w | 0 | W1c | 0 | w] (zero columns for them in fn.net.0).  Same seed and
    tag, so both runs draw the same dropout masks.  Outputs, dx, d(es) (against du_i = sum_j, dv_j = sum_i of it) and every
    parameter gradient must agree: forward at TIGHT, gradients at the fused backward's bar (both runs round differently).
    Slope 1 is the strict form; at slope 0.2 the two runs add Z1 up in different orders, so a pre-activation within 1e-7 of
    zero may fall on either side (measured: one of 700k elements moved the fe.net.1 gradients by 3e-3 of their maximum) --
    there at most 1 % of a tensor's elements may differ by more than the bar, none by more than 2e-2."""
    import itertools
    from mpgan_amd import ops
    rs = np.random.RandomState(17 + N)
    dev = _dev()
    B, F, out = 3, 30, 32
    t = lambda *s, sc=1.0: torch.from_numpy(rs.normal(size=s) * sc).float().to(dev)
    x, u, v = t(B, N, F, sc=0.5), t(B, N, sc=0.5), t(B, N, sc=0.5)
    mask = None
    if use_mask:
        mask = (torch.from_numpy(rs.uniform(size=(B, N, 1))) < 0.8).float().to(dev)
        mask[:, 0] = 1
        if p_drop == 0.0:   # one case with a jet without any particle: workgroups of the four-wave kernels without a sender
            mask[1] = 0
            assert ops.edge_plan(B, N, es=True, mask=True, need_grad=True).SC > 1
    W1a, W1c, w = t(96, F, sc=0.2), t(96, F, sc=0.2), t(96, 1, sc=0.2)
    b1, W2, b2, W3, b3 = t(96, sc=0.1), t(160, 96, sc=0.1), t(160, sc=0.1), t(192, 160, sc=0.1), t(192, sc=0.1)
    V1a, V1x, c1, V2, c2, V3, c3 = t(256, 192, sc=0.1), t(256, F, sc=0.1), t(256, sc=0.1), t(256, 256, sc=0.1), t(256, sc=0.1), t(out, 256, sc=0.1), t(out, sc=0.1)
    up = t(B, N, out)
    z1, z2 = torch.zeros(96, 1, device=dev), torch.zeros(256, 2, device=dev)

    def run(with_es):
        st = ops.dev_state(dev)
        st.tags = itertools.count(77)      # the same dropout sites for both runs
        ops.set_seed(1234, dev)
        leaves = [q.clone().requires_grad_(True) for q in (x, u, v, W1a, W1c, w, b1, W2, b2, W3, b3, V1a, V1x, c1, V2, c2, V3, c3)]
        X, U, Vv, A, Cc, Ww, B1, w2, bb2, w3, bb3, v1a, v1x, cc1, v2, cc2, v3, cc3 = leaves
        if with_es:
            es = torch.stack((U.unsqueeze(1) + Vv.unsqueeze(2), torch.zeros(B, N, N, device=dev)), dim=2)   # [b, j, q, i] = u_i + v_j
            es.retain_grad()
            y = ops.FusedMPLayerFn.apply(X, mask, torch.cat((A, Cc, Ww), 1), B1, w2, bb2, w3, bb3, torch.cat((v1a, v1x), 1), cc1, v2, cc2,
                                         v3, cc3, es, None, ops.MPLayerSettings(True, alpha, p_drop, True, nq=1))
        else:
            X2 = torch.cat((X, U.unsqueeze(2), Vv.unsqueeze(2)), 2)
            W1 = torch.cat((A, Ww, z1, Cc, z1, Ww), 1)
            y = ops.FusedMPLayerFn.apply(X2, mask, W1, B1, w2, bb2, w3, bb3, torch.cat((v1a, v1x, z2), 1), cc1, v2, cc2, v3, cc3,
                                         None, None, ops.MPLayerSettings(True, alpha, p_drop, True))
        (y * up).sum().backward()
        return y.detach(), [q.grad for q in leaves]

    y_es, g_es = run(True)
    y_nf, g_nf = run(False)
    assert rel_err(y_es.cpu().numpy(), y_nf.cpu().numpy()) < TIGHT
    names = "x u v W1a W1c w b1 W2 b2 W3 b3 V1a V1x c1 V2 c2 V3 c3".split()
    errs = {n: rel_err(a.cpu().numpy(), b.cpu().numpy()) for n, a, b in zip(names, g_es, g_nf)}
    print("errs", errs)
    if alpha == 1.0:
        assert max(errs.values()) < TOL, errs
    else:
        off = {n: float(((a - b).abs() > TOL * b.abs().max()).float().mean()) for n, a, b in zip(names, g_es, g_nf)}
        assert max(errs.values()) < 2e-2 and max(off.values()) < 0.01, (errs, off)


def test_jet_order_and_heaviest_first_launches_change_no_result():
    """mpg_jet_order: a permutation, multiplicities non-increasing, ties in index order.  A layer call with more workgroups
    than CUs hands its jets out in that order (ops.OPTIONS['lpt_order']): outputs and every gradient are BIT-identical to the
    index-order launch -- a jet's workgroup computes the same thing whenever it starts."""
    from mpgan_amd import ops
    from mpgan_amd.mpgan import MPLayer
    dev = _dev()
    rs = np.random.RandomState(5)
    for B, N in ((300, 30), (7, 150), (1, 1), (2048, 30)):
        n = rs.randint(0, N + 1, size=B)
        m = (np.arange(N)[None, :] < n[:, None]).astype(np.float32)
        rs.shuffle(m.T)   # (unmasked particles anywhere in the jet)
        order = torch.empty(B, dtype=torch.int32, device=dev)
        mt = torch.from_numpy(np.ascontiguousarray(m)).to(dev)
        ops.check(ops._lib.lib().mpg_jet_order(ops._p(mt), B, N, ops.C.c_void_p(order.data_ptr()), ops._stream()), "mpg_jet_order")
        o = order.cpu().numpy()
        cnt = m.sum(1)
        assert sorted(o.tolist()) == list(range(B))
        assert np.array_equal(o, np.lexsort((np.arange(B), -cnt)))
    B, N = 300, 30
    torch.manual_seed(3)
    layer = MPLayer(32, [96, 160, 192], [256, 256], 32, dropout_p=0.5).to(dev)
    x0 = torch.randn(B, N, 32, device=dev) * 0.5
    nn_ = torch.from_numpy(rs.randint(1, N + 1, size=B))
    mask = (torch.arange(N)[None, :] < nn_[:, None]).float().unsqueeze(2).to(dev)
    up = torch.randn(B, N, 32, device=dev)
    res = {}
    for lpt in (True, False):
        ops.OPTIONS["lpt_order"] = lpt
        try:
            import itertools
            ops.dev_state(dev).tags = itertools.count(500)
            ops.dev_state(dev).order_cache = None
            ops.set_seed(99, dev)
            x = x0.clone().requires_grad_(True)
            layer.zero_grad(set_to_none=True)
            y = layer(x, True, mask)
            (y * up).sum().backward()
            res[lpt] = [y.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in layer.parameters()]
            assert (ops.dev_state(dev).order_cache is not None) == lpt
        finally:
            ops.OPTIONS["lpt_order"] = True
    for a, b in zip(res[True], res[False]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("B,N,F,out,p_drop,use_mask,train", [
    (5, 30, 32, 32, 0.0, True, True), (5, 30, 32, 32, 0.5, True, True), (5, 30, 32, 32, 0.3, True, True),
    (4, 30, 3, 32, 0.5, True, True),      # D's first layer: x is a 3-column slice of [.., 4] rows
    (4, 30, 32, 3, 0.0, True, True),      # G's last layer: rows of 3 floats (element stores)
    (3, 33, 32, 32, 0.0, True, True),     # two receiver blocks, the second with one receiver
    (6, 30, 32, 32, 0.0, False, False),   # no mask, no gradient (nothing kept for a backward)
    (2, 150, 32, 32, 0.0, True, True),    # N = 150: several sender chunks -- the workgroup that arrives last for a (jet, receiver
                                          # block) adds the chunks up and runs the epilogue (eight-wave form); backward: separate launches
    (3, 150, 32, 32, 0.5, True, True),
    (2, 100, 3, 32, 0.0, True, False),
    (2, 5, 32, 3, 0.5, True, True),       # rows of 3 floats WITH dropout, one bit and byte thresholds: the element-store forms of
    (2, 5, 32, 3, 0.3, True, True),       # the forward's epilogue in the dropout modes (one receiver block of 5)
    (2, 5, 3, 32, 0.3, True, True),       # byte-threshold dropout with a 3-column dx (element stores in the backward's epilogue)
])
@pytest.mark.parametrize("two_term", [0, 1])
def test_node_network_as_edge_epilogue_is_bit_identical(B, N, F, out, p_drop, use_mask, train, two_term):
    """``mpg_edge_fwd_fn`` (fn as the epilogue of the edge forward's workgroups, mpgan/model.py:256-279 in one launch) against
    ``mpg_edge_fwd`` + ``mpg_chain``, and ``mpg_edge_bwd_fn`` (the dx chain as the epilogue of the data-gradient kernel's
    workgroups) against ``mpg_edge_bwd`` + ``mpg_chain``: the layer's output, the by-products kept for the backward (agg, both hidden activations)
    and every gradient must be BIT-identical -- same sums in the same order, same dropout sites -- in all three dropout modes,
    for both output widths, a strided x, two receiver blocks, and without gradients."""
    import itertools
    from mpgan_amd import ops
    from mpgan_amd.mpgan import MPLayer
    from oracle import train_ref as T
    dev = _dev()
    rs = np.random.RandomState(N + F + out)
    layer = MPLayer(F, [96, 160, 192], [256, 256], out, dropout_p=p_drop).to(dev)
    layer.load_state_dict({k: v.float() for k, v in T.init_state_dict(_mplayer_shapes(F, out), seed=9, dtype=torch.float64).items()})
    layer.train(train)
    xfull = torch.from_numpy(rs.normal(0, 0.5, size=(B, N, F + 1))).float().to(dev)
    mask = None
    if use_mask:
        m = np.zeros((B, N, 1))
        for b in range(B):
            m[b, rs.permutation(N)[: rs.randint(1, N + 1)], 0] = 1
        mask = torch.from_numpy(m).float().to(dev)
    up = torch.from_numpy(rs.normal(size=(B, N, out))).float().to(dev)

    def run(fused):
        ops.OPTIONS["fn_epilogue"] = ops.OPTIONS["bwd_epilogue"] = fused
        if fused:
            del calls.names[:]       # (the launches of the fused run are what is checked below)
        else:
            calls.restore()
        st = ops.dev_state(dev)
        st.tags = itertools.count(55)
        ops.set_seed(4321, dev)
        layer.zero_grad()
        x = xfull[..., :F].detach().requires_grad_(train)     # (a column slice: row stride F + 1)
        with torch.set_grad_enabled(train):
            y = layer(x, use_mask, mask)
        res = {"y": y.detach().clone()}
        if train:
            saved = ops.mplayer_saved(_fused_node(y))
            res.update(agg=saved.agg.clone(), h1=saved.h1.clone(), h2=saved.h2.clone())
            (y * up).sum().backward()
            res["dx"] = x.grad.clone()
            res.update({k: q.grad.clone() for k, q in layer.named_parameters()})
        return res

    import os
    from mpgan_amd import ops as _ops
    calls = _count_calls(_ops)
    if N <= 64:
        os.environ["MPG_FORCE_SC"] = "1"     # (a handful of jets would be cut into sender chunks to fill the chip: the whole-jet form)
    saved_opts = (ops.OPTIONS["fn_epilogue"], ops.OPTIONS["bwd_epilogue"])
    # (both sides in ONE product form of the edge layers: three terms, or fe.net.2 on two -- MpgEdgeFwd.two_term)
    prev_tt, ops.OPTIONS["fwd_two_term"] = ops.OPTIONS["fwd_two_term"], two_term
    try:
        a, b_ = run(True), run(False)
    finally:
        ops.OPTIONS["fwd_two_term"] = prev_tt
        ops.OPTIONS["fn_epilogue"], ops.OPTIONS["bwd_epilogue"] = saved_opts
        os.environ.pop("MPG_FORCE_SC", None)
        calls.restore()
    want = ["mpg_chain", "mpg_edge_fwd_fn"]
    names = [k for k in calls.names if k != "mpg_pack_many"]   # (the first call builds the weight images)
    assert names[:len(want)] == want, names[:4]
    if train:   # ... and the backward: the dx chain as the epilogue of the data-gradient kernel (a whole jet per workgroup: N <= 32)
        nb = [k for k in names[len(want):] if k in ("mpg_chain", "mpg_edge_bwd", "mpg_edge_bwd_fn")]
        assert nb == (["mpg_chain", "mpg_edge_bwd_fn"] if N <= 32 else ["mpg_chain", "mpg_edge_bwd", "mpg_chain"]), nb
    assert bool(torch.isfinite(a["y"]).all())
    for k in a:
        assert torch.equal(a[k], b_[k]), (k, float((a[k] - b_[k]).abs().max()))


class _count_calls:
    """Records the names of the C-ABI entry points called while it is installed."""

    def __init__(self, ops):
        from mpgan_amd import _lib
        self._lib, self.names, self.args = _lib, [], []   # (args: each call's arguments, beside its name)
        real = _lib.lib()
        outer = self

        class Spy:
            def __getattr__(self, k):
                fn = getattr(real, k)
                if not k.startswith("mpg_"):
                    return fn

                def f(*a):
                    outer.names.append(k)
                    outer.args.append(a)
                    return fn(*a)
                return f
        self.saved = _lib._lib
        _lib._lib = Spy()

    def restore(self):
        self._lib._lib = self.saved


def test_node_network_epilogue_takes_one_launch():
    """The default layer at the headline batch really runs as ONE launch (mpg_edge_fwd_fn) + the a|c projection, not three."""
    from mpgan_amd import ops
    from mpgan_amd.mpgan import MPLayer
    dev = _dev()
    layer = MPLayer(32, [96, 160, 192], [256, 256], 32).to(dev)
    x = torch.randn(256, 30, 32, device=dev)
    mask = torch.ones(256, 30, 1, device=dev)
    layer(x, True, mask)   # (weight images built)
    calls = _count_calls(ops)
    try:
        with torch.no_grad():
            layer(x, True, mask)
    finally:
        calls.restore()
    assert calls.names == ["mpg_chain", "mpg_edge_fwd_fn"], calls.names


@pytest.mark.parametrize("which,train", [("G", True), ("D", True), ("G", False)])
@pytest.mark.parametrize("two_term", [0, 1])
def test_layers_hand_over_their_node_terms(which, train, two_term):
    """A whole network at the headline batch: every layer's edge launch runs the node network as its epilogue AND, for all
    layers but the last, the next layer's a | c projection behind it (``ops.LayerHandoff``) -- one ``mpg_chain`` launch per
    network forward (the first layer's projection) instead of four -- and, in the backward, every data-gradient launch carries
    its layer's dx chain and the lower layer's input-gradient chain as its epilogue (one ``mpg_chain`` launch instead of five);
    outputs and gradients bit-identical to the launches taken one by one, dropout on in D."""
    import itertools
    from mpgan_amd import ops, train as mtrain
    dev = _dev()
    B, N = 256, 30
    torch.manual_seed(3)
    G, D = mtrain.default_mpgan(N, disc_dropout=0.5)
    net = G if which == "G" else D
    net.train(train)
    rs = np.random.RandomState(5)
    labels = torch.from_numpy(rs.randint(10, N + 1, size=(B, 1)) / N).float().to(dev)
    if which == "G":
        xin = torch.from_numpy(rs.normal(0, 0.2, size=(B, N, 32))).float().to(dev)
    else:
        from oracle.train_ref import synthetic_batch
        xin = synthetic_batch(B, N, seed=3)[0].to(dev)

    def run(fused):
        ops.OPTIONS["fn_epilogue"] = ops.OPTIONS["bwd_epilogue"] = fused
        st = ops.dev_state(dev)
        st.tags = itertools.count(91)
        ops.set_seed(99, dev)
        net.zero_grad()
        x = xin.clone().requires_grad_(train)
        calls = _count_calls(ops)
        keep = ("mpg_chain", "mpg_edge_fwd", "mpg_edge_fwd_fn", "mpg_edge_bwd", "mpg_edge_bwd_fn")
        try:
            with torch.set_grad_enabled(train):
                y = net(x, labels)
            names = [k for k in calls.names if k in keep]
            del calls.names[:]
            res = {"y": y.detach().clone()}
            if train:
                y.sum().backward()
                res["dx"] = x.grad.clone()
                res.update({k: q.grad.clone() for k, q in net.named_parameters() if q.grad is not None})
        finally:
            calls.restore()
        return res, names, [k for k in calls.names if k in keep]

    saved = (ops.OPTIONS["fn_epilogue"], ops.OPTIONS["bwd_epilogue"])
    prev_tt, ops.OPTIONS["fwd_two_term"] = ops.OPTIONS["fwd_two_term"], two_term   # (see test_node_network_as_edge_epilogue_is_bit_identical)
    try:
        net(xin, labels)   # (weight images built)
        (a, na, ba), (b_, nb, bb) = run(True), run(False)
    finally:
        ops.OPTIONS["fwd_two_term"] = prev_tt
        ops.OPTIONS["fn_epilogue"], ops.OPTIONS["bwd_epilogue"] = saved
    assert na == ["mpg_chain", "mpg_edge_fwd_fn", "mpg_edge_fwd_fn"], na
    assert nb == ["mpg_chain", "mpg_edge_fwd", "mpg_chain"] * 2, nb
    if train:
        # backward: the top layer's input-gradient chain is the only mpg_chain launch; its data-gradient launch carries its dx
        # and the lower layer's chain, the lower layer's data-gradient launch its own dx
        assert ba == ["mpg_chain", "mpg_edge_bwd_fn", "mpg_edge_bwd_fn"], ba
        assert bb == ["mpg_chain", "mpg_edge_bwd", "mpg_chain", "mpg_chain", "mpg_edge_bwd", "mpg_chain"], bb
    for k in a:
        assert torch.equal(a[k], b_[k]), (k, float((a[k] - b_[k]).abs().max()))


_KEEP = ("mpg_chain", "mpg_edge_fwd", "mpg_edge_fwd_fn", "mpg_edge_bwd", "mpg_edge_bwd_fn")


def _layer_pair_runs(N, shift=None, F=32):
    """Two fused MPLayers F -> F -> F (F = 32: default widths; dropout 0.5, training mode) on B = 2 jets, one sender chunk: the pair
    run through ``MPNet._run_layers`` (each layer with its ``ops.LayerHandoff``) and called by hand (no handoff), same seed and
    tags.  ``shift``: a forward pre-hook on the second layer replaces its x by x + shift in the coupled pass; the by-hand pass
    is given that input.  Returns ((results, forward launches, backward launches) coupled, the same by hand)."""
    import itertools
    import os
    from mpgan_amd import ops
    from mpgan_amd.mpgan import MPNet
    dev = _dev()
    B = 2
    torch.manual_seed(11)
    net = MPNet(N, F, mp_iters=2, hidden_node_size=F, linear_args={"dropout_p": 0.5}).to(dev).train()
    lo, hi = net.mp_layers
    assert lo.fused and hi.fused
    rs = np.random.RandomState(40 + N)
    x0 = torch.from_numpy(rs.normal(0, 0.5, size=(B, N, F))).float().to(dev)
    m = np.zeros((B, N, 1))
    for b in range(B):
        m[b, rs.permutation(N)[: rs.randint(N // 2, N + 1)], 0] = 1
    mask = torch.from_numpy(m).float().to(dev)
    up = torch.from_numpy(rs.normal(size=(B, N, F))).float().to(dev)

    def run(coupled):
        ops.dev_state(dev).tags = itertools.count(123)
        ops.set_seed(2024, dev)
        net.zero_grad()
        x = x0.clone().requires_grad_(True)
        hook = hi.register_forward_pre_hook(lambda mod, args: (args[0] + shift,) + tuple(args[1:])) if (coupled and shift is not None) else None
        calls = _count_calls(ops)
        try:
            if coupled:
                y = net._run_layers(x, True, mask, None, None)
            else:
                y = lo(x, True, mask)
                y = hi(y if shift is None else y + shift, True, mask)
            fwd = [k for k in calls.names if k in _KEEP]
            del calls.names[:]
            (y * up).sum().backward()
        finally:
            calls.restore()
            if hook is not None:
                hook.remove()
        res = {"y": y.detach().clone(), "dx": x.grad.clone()}
        res.update({k: q.grad.clone() for k, q in net.named_parameters()})
        assert len(res) == 2 + 24 and all(bool(torch.isfinite(v).all()) for v in res.values())
        return res, fwd, [k for k in calls.names if k in _KEEP]

    os.environ["MPG_FORCE_SC"] = "1"
    try:
        y = lo(x0, True, mask)
        hi(y, True, mask)     # (weight images built)
        return run(True), run(False)
    finally:
        os.environ.pop("MPG_FORCE_SC", None)


@pytest.mark.parametrize("N", [30, 33])
def test_coupled_and_uncoupled_layer_pairs_give_the_same_bits(N):
    """Output, dx and the twelve parameter gradients of both layers: bit-identical with and without the hand-off.  N = 30 (one
    receiver block, one sender chunk): the only form in which both epilogues and both halves of the hand-off run -- the launch
    sequences say so.  N = 33 (two receiver blocks): the data-gradient launch takes no epilogue, so the lower layer's pending
    chain that was handed over is quietly not used."""
    (a, fa, ba), (b_, fb, bb) = _layer_pair_runs(N)
    for k in a:
        assert torch.equal(a[k], b_[k]), (k, float((a[k] - b_[k]).abs().max()))
    if N == 30:
        assert fa == ["mpg_chain", "mpg_edge_fwd_fn", "mpg_edge_fwd_fn"], fa
        assert fb == ["mpg_chain", "mpg_edge_fwd_fn"] * 2, fb
        assert ba == ["mpg_chain", "mpg_edge_bwd_fn", "mpg_edge_bwd_fn"], ba
        assert bb == ["mpg_chain", "mpg_edge_bwd_fn"] * 2, bb


def test_layer_pair_at_64_features_declines_the_hand_off_with_the_same_bits():
    """``MPNet(N, 64, mp_iters=2, hidden_node_size=64)``: both layers are fused, but none of the epilogue kernels' shapes (the node
    network's first layer has 192 + 64 = 256 columns, dx 64) -- ``_next_node_terms`` declines (out_f > 32), every piece takes its own
    launch with the node network on mpg_chain's general kernel, coupled and by hand alike, and the bits agree."""
    (a, fa, ba), (b_, fb, bb) = _layer_pair_runs(30, F=64)
    for k in a:
        assert torch.equal(a[k], b_[k]), (k, float((a[k] - b_[k]).abs().max()))
    ran = lambda names: [k for k in names if not k.endswith("_fn")]   # (the epilogue entry points are asked, and answer MPG_FN_NA)
    assert ran(fa) == ran(fb) == ["mpg_chain", "mpg_edge_fwd", "mpg_chain"] * 2, (fa, fb)
    assert ran(ba) == ran(bb) == ["mpg_chain", "mpg_edge_bwd", "mpg_chain"] * 2, (ba, bb)


def test_forward_pre_hook_between_layers_breaks_the_coupling_safely():
    """A forward pre-hook on the second layer makes another tensor of x (x + 0.25): the a | c terms the lower layer's launch
    projected (of the rows before the shift) and that layer's pending input-gradient chain are refused by the validity checks --
    every piece takes its own launch, and all results equal the by-hand pass on the shifted input bit for bit."""
    (a, fa, ba), (b_, fb, bb) = _layer_pair_runs(30, shift=0.25)
    for k in a:
        assert torch.equal(a[k], b_[k]), (k, float((a[k] - b_[k]).abs().max()))
    assert fa == fb == ["mpg_chain", "mpg_edge_fwd_fn"] * 2, (fa, fb)
    assert ba == bb == ["mpg_chain", "mpg_edge_bwd_fn"] * 2, (ba, bb)


@pytest.mark.parametrize("alpha", [0.2, 1.0])
@pytest.mark.parametrize("B,N,p_drop", [(6, 30, 0.0), (5, 30, 0.5), (4, 30, 0.3), (2, 150, 0.5), (3, 33, 0.0), (256, 30, 0.5)])
def test_two_term_layer3_agrees_with_three_terms(B, N, p_drop, alpha):
    """The fused forward with fe.net.2 on TWO 16-bit terms (``MpgEdgeFwd.two_term = 1``: its input E2 as the one fp16 value that is
    parked for the backward anyway, times W3 hi + lo) against the three-term form, same seed and tags, so the same dropout masks.
    Layer 2 is untouched: the parked E2 fragments (and with them every kink decision of fe.net.0 / fe.net.1) agree BIT FOR BIT.
    fe.net.2's pre-activations carry the rounding of E2 -- 2^-12 rms per element, independent from edge to edge --: the layer's
    output within 2e-4 of the three-term one.  Gradients: with slope 1 (no kink) every tensor within 5e-4 of the three-term form's;
    with the default slope both forms take the backward's branches from their own forward's sign bits, and a pre-activation
    within ~1e-4 of zero -- of fe.net.2 itself, and of the node network behind the perturbed aggregate -- may sit on the other
    side of the kink: the branch differences of fe.net.2 are counted (<= 1e-3 of its pre-activations; measured 3-8e-5) and the
    gradient differences recorded, not bounded (one flipped node-network sign moves that node's dx rows by ~1e-2, in fp32 as
    here; against the fp64 oracle the form meets the bars of the sign-conditioned evaluation:
    test_train_iteration_with_dropout_vs_oracle run under MPG_FWD_TWO_TERM=1, profiles/r06_*_parity_bars_two_term.txt)."""
    import itertools
    from mpgan_amd import ops
    from mpgan_amd.mpgan import MPLayer
    from conftest import record_parity
    dev = _dev()
    rs = np.random.RandomState(31 + N)
    F, out = 32, 32
    layer = MPLayer(F, [96, 160, 192], [256, 256], out, dropout_p=p_drop, leaky_relu_alpha=alpha).to(dev).train()
    x0 = torch.from_numpy(rs.normal(0, 0.5, size=(B, N, F))).float().to(dev)
    m = np.zeros((B, N, 1))
    for b in range(B):
        m[b, rs.permutation(N)[: rs.randint(1, N + 1)], 0] = 1
    mask = torch.from_numpy(m).float().to(dev)
    up = torch.from_numpy(rs.normal(size=(B, N, out))).float().to(dev)
    prev = ops.OPTIONS["fwd_two_term"]

    def run(tt):
        ops.OPTIONS["fwd_two_term"] = tt
        ops.dev_state(dev).tags = itertools.count(4000)
        ops.set_seed(777, dev)
        layer.zero_grad()
        x = x0.clone().requires_grad_(True)
        y = layer(x, True, mask)
        saved = ops.mplayer_saved(_fused_node(y))
        res = {"sign3": saved.sign3.clone(), "stE2": saved.stE2.clone(), "y": y.detach().clone()}
        (y * up).sum().backward()
        res["dx"] = x.grad.clone()
        res.update({k: q.grad.clone() for k, q in layer.named_parameters()})
        return res

    try:
        a, b_ = run(0), run(1)
    finally:
        ops.OPTIONS["fwd_two_term"] = prev
    # (blocks of masked senders are never written: compare the unmasked senders' blocks)
    RB = (N + 31) // 32
    live = (mask.reshape(B, 1, N) != 0).expand(B, RB, N).reshape(-1)
    assert torch.equal(a["stE2"].reshape(B * RB * N, -1)[live].view(torch.int16), b_["stE2"].reshape(B * RB * N, -1)[live].view(torch.int16))
    sa, sb = a["sign3"].reshape(B * RB * N, -1)[live], b_["sign3"].reshape(B * RB * N, -1)[live]
    diff = (sa ^ sb).cpu().numpy().astype(np.uint32)
    flips = int(np.unpackbits(diff.view(np.uint8)).sum())
    n_pre = int(live.sum()) * 32 * 192     # (32 lanes of receivers per block, padded ones included)
    errs = {k: rel_err(b_[k].cpu().numpy(), a[k].cpu().numpy()) for k in a if k not in ("sign3", "stE2")}
    print("two-term layer 3 against three terms", errs, "sign words differ in", flips, "of", n_pre, "pre-activations of fe.net.2")
    record_parity("two_term", (B, N, p_drop, alpha), fwd_err=float(errs["y"]), worst_grad=max((k for k in errs if k != "y"), key=errs.get),
                  grad_err=float(max(v for k, v in errs.items() if k != "y")), fe3_branch_differences=flips, fe3_preactivations=n_pre,
                  fraction=flips / max(n_pre, 1))
    assert errs["y"] < 2e-4, errs
    if alpha == 1.0:
        assert max(v for k, v in errs.items() if k != "y") < 5e-4, errs
    assert flips <= 1e-3 * n_pre, (flips, n_pre)


def _one_layer_run(N, kw=None, force_sc=None, mode="train", direct=False):
    """One ``MPLayer(32, [96, 160, 192], [256, 256], 32, dropout_p=0.5)`` in training mode on B = 2 jets with some particles masked
    out: a first call builds the weight images, then ONE forward (+ backward) under a fixed seed and tag counter with every ``mpg_*``
    entry point recorded (``_count_calls``).  ``mode``: "train", "frozen" (no parameter wants a gradient, x does) or "nograd"; ``direct``: the backward
    adds into zero-filled ``.grad`` buffers (``DeviceState.grad_into_param``; asserted: ``MpgEdgeDw.accumulate`` says which route ran).
    Returns (results by name, launches)."""
    import itertools
    import os
    from mpgan_amd import ops
    from mpgan_amd.mpgan import MPLayer
    dev = _dev()
    B, F = 2, 32
    torch.manual_seed(7)
    layer = MPLayer(F, [96, 160, 192], [256, 256], 32, dropout_p=0.5, **(kw or {})).to(dev).train()
    rs = np.random.RandomState(100 + N)
    x0 = torch.from_numpy(rs.normal(0, 0.5, size=(B, N, F))).float().to(dev)
    m = np.zeros((B, N, 1))
    for b in range(B):
        m[b, rs.permutation(N)[: rs.randint(N // 2, N)], 0] = 1
    mask = torch.from_numpy(m).float().to(dev)
    up = torch.from_numpy(rs.normal(size=(B, N, 32))).float().to(dev)
    if mode == "frozen":
        for q in layer.parameters():
            q.requires_grad_(False)
    st = ops.dev_state(dev)
    env_sc = os.environ.get("MPG_FORCE_SC")
    if force_sc:
        os.environ["MPG_FORCE_SC"] = force_sc
    try:
        with torch.no_grad():
            layer(x0, True, mask)   # (weight images built)
        st.tags = itertools.count(51)
        ops.set_seed(4242, dev)
        for q in layer.parameters():
            q.grad = torch.zeros_like(q) if direct else None
        x = x0.clone().requires_grad_(mode != "nograd")
        st.grad_into_param = direct
        calls = _count_calls(ops)
        try:
            with torch.set_grad_enabled(mode != "nograd"):
                y = layer(x, True, mask)
            res = {"y": y.detach().clone()}
            if mode != "nograd":
                (y * up).sum().backward()
                res["dx"] = x.grad.clone()
                res.update({k: q.grad.clone() for k, q in layer.named_parameters() if q.grad is not None})
        finally:
            calls.restore()
            st.grad_into_param = False
    finally:
        if env_sc is None:
            os.environ.pop("MPG_FORCE_SC", None)
        else:
            os.environ["MPG_FORCE_SC"] = env_sc
    if mode == "train":   # which route the gradients took: added into .grad by the launches themselves, or handed to autograd
        acc = [a[0]._obj.accumulate for k, a in zip(calls.names, calls.args) if k == "mpg_edge_dw"]
        assert acc == [int(direct)], acc
    return res, calls.names


@pytest.mark.parametrize("N", [30, 33])
def test_direct_accumulation_equals_returned_gradients(N):
    """``grad_into_param``: adding the twelve parameter gradients into zero-filled ``.grad`` buffers gives the bits autograd is
    handed otherwise (adding into zeros is exact), and the same dx.  N = 30: both epilogues; N = 33: two receiver blocks, slab sums."""
    (a, _), (b_, _) = _one_layer_run(N, force_sc="1"), _one_layer_run(N, force_sc="1", direct=True)
    assert len(a) == len(b_) == 2 + 12
    for k in a:
        assert torch.equal(a[k], b_[k]), (k, float((a[k] - b_[k]).abs().max()))
    assert all(bool(torch.isfinite(v).all()) and bool((v != 0).any()) for v in a.values())


# Every ``mpg_*`` call of ONE forward + backward of ``_one_layer_run``, in order, as the host path made them before it was split into named
# steps (recorded on that commit: profiles/mplayer_host_bit_identity.txt)
_LAYER_CASES = {"N30_sc1": (30, None, "1", "train"), "N33_sc1": (33, None, "1", "train"), "N150": (150, None, None, "train"),
                "N30_es": (30, dict(pos_diffs=True, delta_r=True), None, "train"),
                "N30_knn": (30, dict(fully_connected=False, num_knn=10), None, "train"),
                "N30_frozen": (30, None, None, "frozen"), "N30_nograd": (30, None, None, "nograd"),
                # frozen parameters on the whole-jet form (the data-gradient kernel parks nothing, dx is its epilogue) and with edge scalars
                "N5_frozen_sc1": (5, None, "1", "frozen"), "N30_es_frozen": (30, dict(pos_diffs=True, delta_r=True), None, "frozen")}
_LAUNCHES = {
    "N30_sc1": ["mpg_chain", "mpg_edge_fwd_fn", "mpg_chain", "mpg_edge_bwd_fn", "mpg_edge_dw", "mpg_gemm_wgrad_group",
               "mpg_splitk_reduce_group_dw"],
    "N33_sc1": ["mpg_chain", "mpg_edge_fwd_fn", "mpg_chain", "mpg_edge_bwd", "mpg_slab_sums", "mpg_edge_dw", "mpg_gemm_wgrad_group",
               "mpg_splitk_reduce_group_dw", "mpg_chain"],
    "N150": ["mpg_chain", "mpg_edge_fwd_fn", "mpg_chain", "mpg_edge_bwd", "mpg_slab_sums", "mpg_edge_dw", "mpg_gemm_wgrad_group",
            "mpg_splitk_reduce_group_dw", "mpg_chain"],
    "N30_es": ["mpg_chain", "mpg_edge_fwd", "mpg_chain", "mpg_chain", "mpg_edge_bwd", "mpg_slab_sums", "mpg_edge_dw",
              "mpg_gemm_wgrad_group", "mpg_splitk_reduce_group_dw", "mpg_chain"],
    "N30_knn": ["mpg_knn_sets", "mpg_chain", "mpg_edge_fwd_fn", "mpg_chain", "mpg_edge_bwd", "mpg_slab_sums", "mpg_edge_dw",
               "mpg_gemm_wgrad_group", "mpg_splitk_reduce_group_dw", "mpg_chain"],
    "N30_frozen": ["mpg_chain", "mpg_edge_fwd_fn", "mpg_chain", "mpg_edge_bwd", "mpg_slab_sums", "mpg_chain"],
    "N30_nograd": ["mpg_chain", "mpg_edge_fwd_fn"],
    # (N30_sc1 and N30_es without their three weight-gradient launches, as N30_frozen is N33_sc1 without them)
    "N5_frozen_sc1": ["mpg_chain", "mpg_edge_fwd_fn", "mpg_chain", "mpg_edge_bwd_fn"],
    "N30_es_frozen": ["mpg_chain", "mpg_edge_fwd", "mpg_chain", "mpg_chain", "mpg_edge_bwd", "mpg_slab_sums", "mpg_chain"],
}


@pytest.mark.parametrize("case", sorted(_LAYER_CASES))
def test_complete_launch_sequences(case):
    """No launch added, dropped or reordered on any route: whole-jet forms (N = 30, 33 with one sender chunk), sender chunks with
    tickets (N = 150), edge scalars, k-NN sets, the G-step form (frozen parameters: no weight-gradient launches) and no_grad."""
    _, names = _one_layer_run(*_LAYER_CASES[case])
    assert names == _LAUNCHES[case], names
