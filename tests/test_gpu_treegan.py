"""GPU: the TreeGCN launches (mpg_tree_gcn_fwd / _bwd, ``ops.TreeGcnFn``) against the fp64 restatement of tests/treegan_ref.py, and
``ext_models.TreeGANG`` against the reference's own results (tests/golden/treegan.npz, published_treegan_g.npz).

Bars: TIGHT = 1e-4 on forward values, TOL = 1e-3 on gradients (BASELINE.json's), metric ``conftest.rel_err``, gradients through
``conftest.assert_grads`` with the fp32 evaluation of the literal layer as its control.  Inputs of the gradient cases come from the
first seed whose fp64 pre-activations all stay 1e-4 of their layer's largest away from zero: two orders above fp32 rounding, so both
arithmetics take the same LeakyReLU slopes."""
import types

import numpy as np
import pytest
import torch

import treegan_ref as R
from conftest import assert_grads, load_golden, rel_err

pytestmark = pytest.mark.gpu

TIGHT, TOL = 1e-4, 1e-3
POISON = -77.0
PAD = 3          # poisoned columns on either side of an output's rows
SMALL = dict(features=[5, 7, 4, 6, 3], degrees=[3, 1, 2, 2], support=3)
DEFAULT = dict(features=[96, 64, 64, 64, 64, 3], degrees=[2, 2, 2, 2, 2], support=10)


def dev(t):
    return None if t is None else t.float().cuda()


def dev_layer(w):
    return {k: [dev(t) for t in v] if isinstance(v, list) else dev(v) for k, v in w.items()}


def poisoned(rows, cols):
    """A [rows, cols] view in the middle of a wider poisoned array with a poisoned row above and below."""
    wide = torch.full((rows + 2, cols + 2 * PAD), POISON, device="cuda")
    return wide, wide[1:-1, PAD:PAD + cols]


def intact(wide, cols):
    mask = torch.ones_like(wide, dtype=torch.bool)
    mask[1:-1, PAD:PAD + cols] = False
    return bool((wide[mask] == POISON).all()) and not bool((wide[1:-1, PAD:PAD + cols] == POISON).any())


def launch(levels, w, want_u=True):
    """The forward launch into poisoned arrays: (y [B, P g, out], u [B, P g, in] or None), after the poison check."""
    from mpgan_amd import ops
    B, P, inn = levels[-1].shape
    g, out = w["W_branch"].shape[2] // inn, w["W1"].shape[0]
    d = dev_layer(w)
    Wc = (w["W1"] @ w["W0"]).float().cuda()
    ywide, y = poisoned(B * P * g, out)
    uwide, u = poisoned(B * P * g, inn) if want_u else (None, None)
    ops.tree_gcn_launch([dev(t) for t in levels], d["W_root"], d["W_branch"], Wc, None if d["bias"] is None else d["bias"].reshape(-1),
                        act=w["bias"] is not None, alpha=R.ALPHA, y=y, u=u)
    torch.cuda.synchronize()
    assert intact(ywide, out) and (u is None or intact(uwide, inn))
    return y.reshape(B, P * g, out).clone(), None if u is None else u.reshape(B, P * g, inn).clone()


#         features,                  degrees,         d,  B, act
LAYERS = [([3, 1],                   [1],             0,  1, True),     # in 3, out 1, g 1, one jet
          ([5, 3],                   [3],             0, 15, True),     # g in = 15
          ([7, 16, 33],              [3, 2],          1, 17, True),     # P 3, out 33: two column tiles, the second of one column
          ([5, 7, 4, 6, 17, 64],     [3, 1, 2, 1, 3], 4, 31, True),     # d 4 under degrees [3, 1, 2]: anc_i, in 17: two k-steps
          ([9, 17, 64, 12, 64, 3],   [2, 2, 2, 2, 2], 4, 33, False),    # P 16, g in = 128, the last layer, two jet tiles
          ([96, 64],                 [2],             0, 65, True),     # in 96, g in = 192: six branch tiles, three jet tiles
          ([128, 128],               [2],             0, 33, True),     # the limits: width 128, g in = 256
          ([1, 2],                   [160],           0,  2, True)]     # 160 children of one node, in 1


@pytest.mark.parametrize("features, degrees, d, B, act", LAYERS)
def test_layer_forward_vs_fp64(features, degrees, d, B, act):
    gen_ = torch.Generator().manual_seed(100 * d + B)
    w = R.random_layer(features, degrees, d, 3, act, gen_)
    levels = R.random_levels(features, degrees, d, B, gen_)
    ref_y, ref_u = R.collapsed(levels, w)
    assert rel_err(ref_y, R.literal(levels, w)) <= 1e-12
    y, u = launch(levels, w)
    ey, eu = rel_err(y.cpu(), ref_y), rel_err(u.cpu(), ref_u)
    print(f"y {ey:.3g} u {eu:.3g}")
    assert ey <= TIGHT and eu <= TIGHT
    y2, none = launch(levels, w, want_u=False)
    assert none is None and torch.equal(y, y2)


def test_a_jets_values_do_not_depend_on_the_batch():
    """Jet b's rows are bit-identical alone (B = 1), at another position of a batch of 65, and on a rerun."""
    features, degrees, d = [7, 16, 33], [3, 2], 1
    gen_ = torch.Generator().manual_seed(1)
    w = R.random_layer(features, degrees, d, 3, True, gen_)
    big = R.random_levels(features, degrees, d, 65, gen_)
    for t in big:
        t[40] = t[0]
    one = [t[:1].clone() for t in big]
    y1, u1 = launch(one, w)
    yb, ub = launch(big, w)
    yb2, ub2 = launch(big, w)
    assert torch.equal(yb, yb2) and torch.equal(ub, ub2)
    for pos in (0, 40):
        assert torch.equal(y1[0], yb[pos]) and torch.equal(u1[0], ub[pos])
    assert not torch.equal(yb[0], yb[1])


def _decided(features, degrees, d, B, act):
    """(weights, levels, cotangent) of the first seed of range(40) whose pre-activations all stay 1e-4 max|z| away from zero."""
    P = int(np.prod(degrees[:d + 1]))
    for seed in range(40):
        gen_ = torch.Generator().manual_seed(seed)
        w = R.random_layer(features, degrees, d, 3, act, gen_)
        levels = R.random_levels(features, degrees, d, B, gen_)
        probe = {}
        R.collapsed(levels, w, probe=probe)
        if min(float(z.abs().min() / z.abs().max()) for z in probe["z"]) >= 1e-4:
            return w, levels, torch.randn(B, P, features[d + 1], generator=gen_, dtype=torch.float64)
    raise AssertionError("no decided seed in range(40)")


def _names(d, act):
    return [f"level{i}" for i in range(d + 1)] + [f"W_root{i}" for i in range(d + 1)] + ["W_branch", "W0", "W1"] + (["bias"] if act else [])


def _leaves(levels, w, cast):
    return [cast(t).requires_grad_(True) for t in levels + w["W_root"] + [w["W_branch"], w["W0"], w["W1"]]
            + ([w["bias"]] if w["bias"] is not None else [])]


def _literal_grads(levels, w, dy, cast):
    d, act = len(levels) - 1, w["bias"] is not None
    lv = _leaves(levels, w, cast)
    ww = {"W_root": lv[d + 1:2 * d + 2], "W_branch": lv[2 * d + 2], "W0": lv[2 * d + 3], "W1": lv[2 * d + 4], "bias": lv[-1] if act else None}
    y = R.literal(lv[:d + 1], ww)
    grads = torch.autograd.grad((y * cast(dy)).sum(), lv)
    return y.detach(), dict(zip(_names(d, act), (g.numpy() for g in grads)))


@pytest.mark.parametrize("d, act", [(2, True), (3, False)])
def test_tree_gcn_fn_gradients_vs_fp64_autograd(d, act):
    """Every parameter, every level and u's path, for a middle layer and the last layer of the small configuration at B = 33."""
    from mpgan_amd import ops
    B = 33
    w, levels, dy = _decided(SMALL["features"], SMALL["degrees"], d, B, act)
    ref_y, ref = _literal_grads(levels, w, dy, lambda t: t.clone())
    _, control = _literal_grads(levels, w, dy, lambda t: t.float())
    lv = _leaves(levels, w, lambda t: t.float().cuda())
    out = ops.tree_gcn(lv[:d + 1], lv[d + 1:2 * d + 2], lv[2 * d + 2], lv[2 * d + 3], lv[2 * d + 4], lv[-1] if act else None, act=act)
    (out * dy.float().cuda()).sum().backward()
    torch.cuda.synchronize()
    assert rel_err(out.detach().cpu(), ref_y) <= TIGHT
    got = {k: t.grad.cpu().numpy() for k, t in zip(_names(d, act), lv)}
    for k in ref:
        print(k, f"{rel_err(got[k], ref[k]):.3g}")
    assert_grads(got, ref, TOL, control=control, what=f"TreeGcnFn d={d} act={act}")


@pytest.mark.parametrize("route", ["queued", "direct"])
def test_tree_gcn_fn_gradient_routes(route):
    """Under ``grad_into_param`` the parameter gradients go into existing .grad buffers (queued: by the collecting batch's grouped
    launch at its flush; direct without one: returned and accumulated by autograd) and add to what is there: twice the returned
    route's values on buffers that held them already.  Bar 2^-16: the routes differ in which launch forms a sum (the bias is an fp32
    ``sum`` when returned, a ones column of the grouped bf16 hi / lo GEMM when queued), and a bf16 hi / lo operand keeps its value to
    2^-17, two operands per product."""
    from mpgan_amd import ops
    d, act, B = 2, True, 33
    w, levels, dy = _decided(SMALL["features"], SMALL["degrees"], d, B, act)

    def run(lv):
        out = ops.tree_gcn(lv[:d + 1], lv[d + 1:2 * d + 2], lv[2 * d + 2], lv[2 * d + 3], lv[2 * d + 4], lv[-1], act=act)
        (out * dy.float().cuda()).sum().backward()

    lv = _leaves(levels, w, lambda t: t.float().cuda())
    run(lv)
    torch.cuda.synchronize()
    first = [t.grad.clone() for t in lv]
    st = ops.dev_state(lv[0].device)
    st.grad_into_param, st.deferred_wgrad = True, (ops.WgradBatch() if route == "queued" else None)
    try:
        run(lv)
        if route == "queued":
            assert len(st.deferred_wgrad.jobs) == 3 + 3 + 3       # W_branch per node, W_loop.0, W_loop.1 and the bias, the roots
            st.deferred_wgrad.flush()
    finally:
        st.grad_into_param, st.deferred_wgrad = False, None
    torch.cuda.synchronize()
    for name, t, g1 in zip(_names(d, act), lv, first):
        assert rel_err(t.grad.cpu(), 2 * g1.cpu()) <= 2.0 ** -16, name


def test_backward_launch_vs_formula():
    """dz, S, du and dx of the launch on the y and u THE FORWARD PRODUCED, against the fp64 formulas on the same y and u."""
    from mpgan_amd import ops
    features, degrees, d, B = [7, 16, 33], [3, 2], 1, 33
    gen_ = torch.Generator().manual_seed(3)
    w = R.random_layer(features, degrees, d, 3, True, gen_)
    levels = R.random_levels(features, degrees, d, B, gen_)
    y, u = launch(levels, w)
    P, g, inn, out = 3, 2, 16, 33
    dy = torch.randn(B * P * g, out, generator=gen_).cuda()
    Wc = (w["W1"] @ w["W0"]).float().cuda()
    dz, S, du, dx = ops.tree_gcn_bwd_launch(dy, y.reshape(-1, out), u.reshape(-1, inn), [t.shape[1:] for t in levels],
                                            dev(w["W_branch"]), Wc, act=True, alpha=R.ALPHA)
    torch.cuda.synchronize()
    y64, u64, dy64, Wc64 = y.cpu().double(), u.cpu().double(), dy.cpu().double().reshape(B, P * g, out), Wc.cpu().double()
    rdz = dy64 * R.slope(y64)
    rdu = (rdz @ Wc64).reshape(B, P, g * inn) * R.slope(u64.reshape(B, P, g * inn))
    rdx = torch.einsum("bpn,pkn->bpk", rdu, w["W_branch"].float().double())
    assert rel_err(dz.cpu().reshape(B, P * g, out), rdz) <= 1e-6
    assert rel_err(S.cpu().reshape(B, P, out), rdz.reshape(B, P, g, out).sum(2)) <= 1e-6
    assert rel_err(du.cpu().reshape(B, P, g * inn), rdu) <= TOL and rel_err(dx.cpu().reshape(B, P, inn), rdx) <= TOL
    none = ops.tree_gcn_bwd_launch(dy, y.reshape(-1, out), u.reshape(-1, inn), [t.shape[1:] for t in levels], dev(w["W_branch"]), Wc,
                                   act=True, alpha=R.ALPHA, need_dx=False)
    assert none[3] is None and torch.equal(none[2], du)


def test_no_grad_call_writes_no_u(monkeypatch):
    from mpgan_amd import ops
    w, levels, _ = _decided(SMALL["features"], SMALL["degrees"], 2, 5, True)
    seen = []
    real = ops.tree_gcn_launch
    monkeypatch.setattr(ops, "tree_gcn_launch", lambda *a, **k: (seen.append(k["u"]), real(*a, **k))[1])
    lv = _leaves(levels, w, lambda t: t.float().cuda())
    args = (lv[:3], lv[3:6], lv[6], lv[7], lv[8], lv[9])
    with torch.no_grad():
        y0 = ops.tree_gcn(*args)
    y1 = ops.tree_gcn(*args)
    assert seen[0] is None and seen[1] is not None and torch.equal(y0, y1.detach())


# ------------------------------------------------------------------------------------------------ the generator
@pytest.fixture(scope="module")
def golden():
    return {k: torch.from_numpy(np.asarray(v)) for k, v in load_golden("treegan.npz").items()}


def _net(cfg, sd=None, seed=0):
    from mpgan_amd import ext_models
    torch.manual_seed(seed)
    net = ext_models.TreeGANG(**cfg)
    if sd is not None:
        net.load_state_dict({k: v.float() for k, v in sd.items()}, strict=True)
    return net


def test_small_generator_vs_reference_golden(golden, monkeypatch):
    from mpgan_amd import ops
    sd = {k[3:]: v for k, v in golden.items() if k.startswith("sd.")}
    net = _net(SMALL, sd).cuda()
    calls = []
    real = ops.tree_gcn_launch
    monkeypatch.setattr(ops, "tree_gcn_launch", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    noise = golden["noise"].float().cuda().requires_grad_(True)
    out = net([noise])
    (out * golden["cot"].float().cuda()).sum().backward()
    torch.cuda.synchronize()
    assert len(calls) == 4                                  # every layer on the fused launch
    assert rel_err(out.detach().cpu(), golden["out"]) <= TIGHT
    last = "gcn.TreeGCN_3.bias"
    assert dict(net.named_parameters())[last].grad is None
    # the control: the literal net in fp32 (the reference's arithmetic)
    leaves = {k: v.float().requires_grad_(True) for k, v in sd.items()}
    n32 = golden["noise"].float().requires_grad_(True)
    (R.generator(leaves, n32, 4, fn=R.literal) * golden["cot"].float()).sum().backward()
    keys = [k for k in sd if k != last]
    got = {"dnoise": noise.grad.cpu().numpy(), **{k: p.grad.cpu().numpy() for k, p in net.named_parameters() if k != last}}
    ref = {"dnoise": golden["dnoise"].numpy(), **{k: golden["grad." + k].numpy() for k in keys}}
    control = {"dnoise": n32.grad.numpy(), **{k: leaves[k].grad.numpy() for k in keys}}
    assert_grads(got, ref, TOL, control=control, what="ext_models TreeGANG")


def test_default_generator_fused_unfused_and_fp64(monkeypatch):
    """The default configuration at B = 4: the fused route against the fp64 CPU module; the un-fused route (MPG_TREE_GCN=0) agrees
    and never calls the new launch."""
    from mpgan_amd import ops
    cpu = _net(DEFAULT, seed=3)
    noise = torch.randn(4, 1, 96, generator=torch.Generator().manual_seed(1)) * 0.2
    with torch.no_grad():
        ref = cpu.double()([noise.double()])
    net = _net(DEFAULT, seed=3).cuda()
    calls = []
    real = ops.tree_gcn_launch
    monkeypatch.setattr(ops, "tree_gcn_launch", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    with torch.no_grad():
        fused = net([noise.cuda()])
    assert len(calls) == 5 and fused.shape == (4, 32, 3)
    monkeypatch.setitem(ops.OPTIONS, "tree_gcn", False)
    with torch.no_grad():
        plain = net([noise.cuda()])
    assert len(calls) == 5
    e1, e2, e3 = rel_err(fused.cpu(), ref), rel_err(plain.cpu(), ref), rel_err(fused.cpu(), plain.cpu())
    print(f"fused {e1:.3g} un-fused {e2:.3g} fused vs un-fused {e3:.3g}")
    assert e1 <= TIGHT and e2 <= TIGHT and e3 <= TIGHT


def test_double_backward_route_is_twice_differentiable(golden, monkeypatch):
    """Inside ``ops.double_backward_route`` the literal layer runs on ``MatMulFn`` / ATen and never on the fused launch: the output
    meets the golden one, and the gradient of |d out / d noise|^2 with respect to every parameter meets the fp64 CPU module's."""
    from mpgan_amd import ops
    sd = {k[3:]: v for k, v in golden.items() if k.startswith("sd.")}
    calls = []
    real = ops.tree_gcn_launch
    monkeypatch.setattr(ops, "tree_gcn_launch", lambda *a, **k: (calls.append(1), real(*a, **k))[1])

    def penalty(net, noise, cot):
        out = net([noise])
        (g,) = torch.autograd.grad((out * cot).sum(), noise, create_graph=True)
        (g ** 2).sum().backward()
        return out.detach(), {k: p.grad.cpu().numpy() for k, p in net.named_parameters() if p.grad is not None}

    from mpgan_amd import ext_models
    net64 = ext_models.TreeGANG(**SMALL).double()
    net64.load_state_dict(sd, strict=True)
    ref_out, ref = penalty(net64, golden["noise"].clone().requires_grad_(True), golden["cot"])
    _, control = penalty(_net(SMALL, sd), golden["noise"].float().requires_grad_(True), golden["cot"].float())
    net = _net(SMALL, sd).cuda()
    with ops.double_backward_route("cuda"):
        out, got = penalty(net, golden["noise"].float().cuda().requires_grad_(True), golden["cot"].float().cuda())
    torch.cuda.synchronize()
    assert not calls and set(got) == set(ref)
    assert rel_err(out.cpu(), ref_out) <= TIGHT and rel_err(ref_out, golden["out"]) <= 1e-12
    assert_grads(got, ref, TOL, control=control, what="ext_models TreeGANG double backward")


def test_published_generator_on_the_gpu():
    from mpgan_amd import gen
    sd = {k: torch.from_numpy(v) for k, v in load_golden("published_treegan_g_weights.npz").items()}
    G = _net(DEFAULT, sd).cuda().eval()
    g = load_golden("published_treegan_g.npz")
    margs = {"treegang_features": DEFAULT["features"]}
    out = gen.gen(margs, G, 8, 30, model="treegan", noise=[torch.from_numpy(g["noise"]).cuda()])
    err = rel_err(out.detach().cpu(), g["out"])
    print(f"published generator {err:.3g}")
    assert out.shape == (8, 32, 3) and err <= TIGHT
    assert gen.gen_multi_batch(margs, G, 4, 6, 30, out_device="cuda", detach=True, model="treegan").shape == (6, 32, 3)


def test_captured_forward_follows_in_place_weight_updates():
    """The forward of the default generator captured with torch.cuda.graph replays to the eager result, and after an in-place
    change of W_loop.0.weight to the new eager result: Wc is formed on the device inside the captured region."""
    net = _net(DEFAULT, seed=5).cuda()
    noise = (torch.randn(4, 1, 96, generator=torch.Generator().manual_seed(2)) * 0.2).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.no_grad():
        with torch.cuda.stream(side):
            for _ in range(2):
                net([noise])
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = net([noise])
        graph.replay()
        torch.cuda.synchronize()
        eager = net([noise])
        assert torch.equal(out, eager)
        net.gcn.TreeGCN_2.W_loop[0].weight.mul_(-1.5)
        graph.replay()
        torch.cuda.synchronize()
        eager2 = net([noise])
        assert torch.equal(out, eager2) and not torch.equal(eager, eager2)


def test_one_adam_step_against_rgand():
    from mpgan_amd import ext_models
    torch.manual_seed(11)
    G = ext_models.TreeGANG(**DEFAULT).cuda()
    D = ext_models.rGAND(types.SimpleNamespace(rgand_sfc=[64, 128], rgand_fc=[64], num_hits=32, node_feat_size=3,
                                               leaky_relu_alpha=0.2)).cuda()
    opt = torch.optim.Adam(G.parameters(), lr=1e-4)
    before = {k: p.detach().clone() for k, p in G.named_parameters()}
    noise = torch.randn(8, 1, 96, device="cuda") * 0.2
    loss = ((D(G([noise])) - 1.0) ** 2).mean()
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss))
    last = "gcn.TreeGCN_4.bias"
    for k, p in G.named_parameters():
        if k == last:
            assert p.grad is None and torch.equal(p, before[k])
        else:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, k
            assert not torch.equal(p, before[k]), k
