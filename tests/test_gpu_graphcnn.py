"""GPU: the NNConv launches (mpg_nnconv_fwd / _bwd, ``ops.NNConvFn``) against the fp64 restatement of tests/nnconv_ref.py, and
``ext_models.GraphCNNGANG`` against the reference's own results (tests/golden/graphcnn.npz, published_graphcnn_g.npz).

Bars: TIGHT = 1e-4 on forward values, TOL = 1e-3 on gradients (BASELINE.json's), metric ``conftest.rel_err``, gradients through
``conftest.assert_grads`` with the fp32 evaluation of the literal layer as its control.  The layer tests hand the graph in from the
fp64 restatement and evaluate the fp64 reference on the inputs AS ROUNDED TO fp32 (what the launch is given: on a clustered jet the
rounding of x itself moves x_j - x_i by 1e-3 of its size, which is no property of the kernel).  Generator tests use inputs whose
neighbour sets are decided (rank margin >= 1e-4, two orders above fp32 rounding of a distance)."""
import types

import numpy as np
import pytest
import torch

import nnconv_ref as R
from conftest import assert_grads, load_golden, rel_err

pytestmark = pytest.mark.gpu

TIGHT, TOL = 1e-4, 1e-3
POISON = -77.0
PAD = 3          # poisoned columns on either side of an output's rows
SMALL = dict(latent_dim=7, num_hits=10, graphcnng_layers=[6, 5], node_feat_size=3, num_knn=4, leaky_relu_alpha=0.2,
             graphcnng_tanh=True, device="cuda")
PUBLISHED = dict(latent_dim=128, num_hits=30, graphcnng_layers=[32, 24], node_feat_size=3, num_knn=20, leaky_relu_alpha=0.2,
                 graphcnng_tanh=False, device="cuda")
NAMES = ("nn_weight", "nn_bias", "root", "bias")


def args_of(d):
    return types.SimpleNamespace(**{k: (list(v) if isinstance(v, list) else v) for k, v in d.items()})


def poisoned(rows, cols):
    """A [rows, cols] view in the middle of a wider poisoned array with a poisoned row above and below."""
    wide = torch.full((rows + 2, cols + 2 * PAD), POISON, device="cuda")
    return wide, wide[1:-1, PAD:PAD + cols]


def intact(wide, cols):
    mask = torch.ones_like(wide, dtype=torch.bool)
    mask[1:-1, PAD:PAD + cols] = False
    return bool((wide[mask] == POISON).all()) and not bool((wide[1:-1, PAD:PAD + cols] == POISON).any())


def random_layer(Cin, Cout, N, B, seed, x=None):
    """fp64 values that are exact in fp32."""
    gen_ = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen_, dtype=torch.float64)
    w = dict(x=r(B, N, Cin) if x is None else x, nn_weight=r(Cin * Cout, Cin) / Cin ** 0.5, nn_bias=r(Cin * Cout) / Cin ** 0.5,
             root=r(Cin, Cout) / Cin ** 0.5, bias=r(Cout))
    return {k: v.float().double() for k, v in w.items()}


def launch(w, adj, want_pm=True):
    """The forward launch into poisoned arrays: (y [B, N, Cout], pm [B N, Cin (Cin + 1)] or None), after the poison check."""
    from mpgan_amd import ops
    B, N, Cin = w["x"].shape
    Cout = w["root"].shape[1]
    xwide, x2 = poisoned(B * N, Cin)             # a strided input as well
    x2.copy_(w["x"].reshape(B * N, Cin).float())
    ywide, y = poisoned(B * N, Cout)
    pm = torch.full((B * N + 2, Cin * (Cin + 1)), POISON, device="cuda") if want_pm else None
    ops.nnconv_launch(x2, R.pack_bits(adj).cuda(), *(w[n].float().cuda() for n in NAMES), B, N, y=y, pm=None if pm is None else pm[1:-1])
    torch.cuda.synchronize()
    assert intact(ywide, Cout)
    if pm is not None:
        assert bool((pm[0] == POISON).all()) and bool((pm[-1] == POISON).all()) and not bool((pm[1:-1] == POISON).any())
    return y.reshape(B, N, Cout).clone(), None if pm is None else pm[1:-1].clone()


def check_forward(w, adj, bar=TIGHT):
    B, N, Cin = w["x"].shape
    Cout = w["root"].shape[1]
    ref_y, P, m = R.factorised(w["x"], adj, *(w[n] for n in NAMES))
    if B * N * N * Cin * Cout <= 5_000_000:
        assert rel_err(ref_y, R.literal(w["x"], adj, *(w[n] for n in NAMES))) <= 1e-11
    y, pm = launch(w, adj)
    ref_pm = torch.cat([P.reshape(B * N, Cin * Cin), m.reshape(B * N, Cin)], 1)
    ey, ep = rel_err(y.cpu(), ref_y), rel_err(pm.cpu(), ref_pm)
    print(f"y {ey:.3g} [P | m] {ep:.3g}")
    assert ey <= bar and ep <= bar
    y2, none = launch(w, adj, want_pm=False)
    assert none is None and torch.equal(y, y2)
    return y


#          Cin, Cout, N,  k, loop, B
SHAPES = [(1,   1,    2,  1, False, 1),
          (5,   3,   10,  4, False, 3),
          (32, 24,   30, 20, False, 5),      # the published layers
          (24,  3,   30, 20, False, 5),
          (8,   8,   30, 30, True,  2),      # loop: every node lists all 30, itself included
          (7,  33,   33,  9, False, 2),      # two receiver tiles, the second of one row; Cout beyond one column tile
          (64, 64,   65, 20, False, 2),      # the widths' limits, three receiver tiles, three neighbour words
          (16,  8,  160, 20, False, 1),      # the limit of N: five receiver tiles, five neighbour words
          (4,   4,    8, 12, False, 2)]      # k = 12 > N - 1 = 7: n_i = 7 < k


@pytest.mark.parametrize("Cin, Cout, N, k, loop, B", SHAPES)
def test_layer_forward_vs_fp64(Cin, Cout, N, k, loop, B):
    w = random_layer(Cin, Cout, N, B, 100 * Cin + N)
    adj = R.knn_adjacency(w["x"], k, loop)
    assert int(adj.sum(2).max()) == int(adj.sum(2).min()) == min(k, N if loop else N - 1)
    check_forward(w, adj)


def test_layer_forward_on_hand_made_sets():
    """An empty row (a zero message: y = x root + bias), a row of one bit, a row that lists itself only, rows of different counts."""
    w = random_layer(6, 5, 35, 2, 7)
    adj = R.knn_adjacency(w["x"], 3, False)
    adj[0, 4] = 0
    adj[0, 5] = 0
    adj[0, 5, 34] = 1
    adj[1, 33] = 0
    adj[1, 33, 33] = 1
    adj[1, 34] = 1
    y = check_forward(w, adj)
    assert rel_err(y[0, 4].cpu(), w["x"][0, 4] @ w["root"] + w["bias"]) <= TIGHT


def test_clustered_jet():
    """x = 32 + 1e-3 noise, root = nn.bias = bias = 0: the moment form mean(x_j x_j^T) - m_i x_i^T evaluated in fp32 is 3e-3 from fp64
    here; the differences taken first keep it at fp32 rounding."""
    gen_ = torch.Generator().manual_seed(5)
    x = 32.0 + 1e-3 * torch.randn(3, 30, 32, generator=gen_, dtype=torch.float64)
    w = random_layer(32, 24, 30, 3, 6, x=x)
    for n in ("nn_bias", "root", "bias"):
        w[n] = torch.zeros_like(w[n])
    check_forward(w, R.knn_adjacency(w["x"], 20, False))


def _sd(golden):
    return {k[3:]: v for k, v in golden.items() if k.startswith("sd.")}


@pytest.fixture(scope="module")
def golden():
    return {k: torch.from_numpy(np.asarray(v)) for k, v in load_golden("graphcnn.npz").items()}


@pytest.fixture(scope="module")
def published():
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in load_golden("published_graphcnn_g_weights.npz").items()}
    return sd, load_golden("published_graphcnn_g.npz")


def test_knn_sets_equal_the_fp64_graph_on_the_golden_inputs(golden, published):
    """``ops.knn_sets`` on the fp32 layer inputs of both golden cases gives the fp64 restatement's sets bit for bit, without self
    loops at the nets' k and with them at k = N (the reference's only loop case); the stored margins say the sets are decided."""
    from mpgan_amd import ops
    assert float(golden["margin_rank"]) >= 1e-4 and float(published[1]["margin_rank"]) >= 1e-4
    cases = []
    probe = {}
    R.generator(_sd(golden), golden["noise"], 10, 4, 0.2, tanh=True, training=True, probe=probe)
    cases += [(x, 4) for x in probe["x"]]
    probe = {}
    R.generator({k: v.double() for k, v in published[0].items()}, torch.from_numpy(published[1]["noise"]).double(), 30, 20, 0.2, probe=probe)
    cases += [(x, 20) for x in probe["x"]]
    assert len(cases) == 4
    for x, k in cases:
        B, N, _ = x.shape
        for kk, loop in ((k, False), (N, True)):
            got = ops.knn_sets(x.float().cuda(), None, kk, self_loops=loop)
            assert torch.equal(got.cpu(), R.pack_bits(R.knn_adjacency(x, kk, loop))), (tuple(x.shape), kk, loop)


def test_a_jets_values_do_not_depend_on_the_batch():
    """Jet b's rows are bit-identical alone (B = 1), at another position of a batch of 33, and on a rerun."""
    w = random_layer(7, 33, 33, 33, 1)
    w["x"][20] = w["x"][0]
    adj = R.knn_adjacency(w["x"], 9, False)
    one = dict(w, x=w["x"][:1].clone())
    y1, p1 = launch(one, adj[:1])
    yb, pb = launch(w, adj)
    yb2, pb2 = launch(w, adj)
    assert torch.equal(yb, yb2) and torch.equal(pb, pb2)
    for pos in (0, 20):
        assert torch.equal(y1[0], yb[pos]) and torch.equal(p1, pb[33 * pos:33 * (pos + 1)])
    assert not torch.equal(yb[0], yb[1])


# ------------------------------------------------------------------------------------------------ gradients
def _literal_grads(w, adj, dy, cast):
    lv = {k: cast(v).requires_grad_(True) for k, v in w.items()}
    y = R.literal(lv["x"], cast(adj), *(lv[n] for n in NAMES))
    grads = torch.autograd.grad((y * cast(dy)).sum(), list(lv.values()))
    return y.detach(), dict(zip(lv, (g.numpy() for g in grads)))


def _case(Cin, Cout, N, k, B, seed):
    w = random_layer(Cin, Cout, N, B, seed)
    adj = R.knn_adjacency(w["x"], k, False)
    dy = torch.randn(B, N, Cout, generator=torch.Generator().manual_seed(seed + 1), dtype=torch.float64).float().double()
    return w, adj, dy


@pytest.mark.parametrize("Cin, Cout, N, k, B", [(5, 3, 10, 4, 3), (32, 24, 30, 20, 5)])
def test_nnconv_fn_gradients_vs_fp64_autograd(Cin, Cout, N, k, B):
    from mpgan_amd import ops
    w, adj, dy = _case(Cin, Cout, N, k, B, 11 * Cin)
    ref_y, ref = _literal_grads(w, adj, dy, lambda t: t.clone())
    _, control = _literal_grads(w, adj, dy, lambda t: t.float())
    closed = R.backward(w["x"], adj, *(w[n] for n in NAMES), dy)
    for n in ref:
        assert rel_err(closed[n], ref[n]) <= 1e-11
    lv = {n: t.float().cuda().requires_grad_(True) for n, t in w.items()}
    out = ops.nnconv(lv["x"], R.pack_bits(adj).cuda(), *(lv[n] for n in NAMES))
    assert type(out.grad_fn).__name__ == "NNConvFnBackward" and out.shape == (B * N, Cout)
    (out * dy.float().cuda().reshape(B * N, Cout)).sum().backward()
    torch.cuda.synchronize()
    assert rel_err(out.detach().cpu().reshape(B, N, Cout), ref_y) <= TIGHT
    got = {n: t.grad.cpu().numpy() for n, t in lv.items()}
    for n in ref:
        print(n, f"{rel_err(got[n], ref[n]):.3g}")
    assert_grads(got, ref, TOL, control=control, what=f"NNConvFn {Cin}->{Cout}")


def test_backward_launch_vs_closed_form():
    """dx of the launch (into a poisoned, padded array) on the [P | m] THE FORWARD PARKED, against the fp64 closed form; the
    workspace's [G | dm]; a rerun is bit-identical."""
    from mpgan_amd import ops
    Cin, Cout, N, B = 7, 33, 33, 2
    w, adj, dy = _case(Cin, Cout, N, 9, B, 3)
    adj[1, 2] = 0                                   # an empty row: it sends, and receives its own shares only
    _, pm = launch(w, adj)
    nbr = R.pack_bits(adj).cuda()
    dev = {n: w[n].float().cuda() for n in w}
    x2 = dev["x"].reshape(B * N, Cin)
    dyd = dy.float().cuda().reshape(B * N, Cout)
    wide, dx = poisoned(B * N, Cin)
    g = torch.full((B * N + 1, Cin * (Cin + 1)), POISON, device="cuda")
    ops.nnconv_bwd_launch(dyd, x2, nbr, pm, dev["nn_weight"], dev["nn_bias"], dev["root"], B, N, dx=dx, g=g[:-1])
    torch.cuda.synchronize()
    assert intact(wide, Cin) and bool((g[-1] == POISON).all())
    ref = R.backward(w["x"], adj, *(w[n] for n in NAMES), dy)
    G = torch.einsum("bio,cod->bicd", dy, w["nn_weight"].view(Cin, Cout, Cin)).reshape(B * N, Cin * Cin)
    dm = (dy @ w["nn_bias"].view(Cin, Cout).t()).reshape(B * N, Cin)
    eg, ex = rel_err(g[:-1].cpu(), torch.cat([G, dm], 1)), rel_err(dx.cpu().reshape(B, N, Cin), ref["x"])
    print(f"[G | dm] {eg:.3g} dx {ex:.3g}")
    assert eg <= 1e-5 and ex <= TOL
    dx2 = ops.nnconv_bwd_launch(dyd, x2, nbr, pm, dev["nn_weight"], dev["nn_bias"], dev["root"], B, N)
    assert torch.equal(dx2, dx)


@pytest.mark.parametrize("wanted", [("x",), NAMES, ("x", "root"), ("nn_weight",), ("bias",)])
def test_needs_input_grad_subsets(wanted):
    """Only what asks for a gradient gets one, and it equals the all-gradients call's bit for bit."""
    from mpgan_amd import ops
    w, adj, dy = _case(5, 3, 10, 4, 3, 21)
    nbr = R.pack_bits(adj).cuda()

    def run(names):
        lv = {n: t.float().cuda().requires_grad_(n in names) for n, t in w.items()}
        out = ops.nnconv(lv["x"], nbr, *(lv[n] for n in NAMES))
        (out * dy.float().cuda().reshape(30, 3)).sum().backward()
        torch.cuda.synchronize()
        return out.detach(), {n: t.grad for n, t in lv.items()}

    y_all, full = run(tuple(w))
    y, part = run(wanted)
    assert torch.equal(y, y_all)
    for n in w:
        assert (part[n] is None) == (n not in wanted), n
        if n in wanted:
            assert torch.equal(part[n], full[n]), n


@pytest.mark.parametrize("route", ["queued", "direct"])
def test_nnconv_fn_gradient_routes(route):
    """Under ``grad_into_param`` the parameter gradients go into existing .grad buffers (queued: by the collecting batch's grouped
    launch at its flush; direct without one: returned and accumulated by autograd) and add to what is there: twice the returned
    route's values on buffers that held them already.  Bar 2^-16: the routes differ in which launch forms a sum (the bias is an fp32
    ``sum`` when returned, a ones column of the grouped bf16 hi / lo GEMM when queued), and a bf16 hi / lo operand keeps its value to
    2^-17, two operands per product."""
    from mpgan_amd import ops
    Cin = 5
    w, adj, dy = _case(Cin, 3, 10, 4, 3, 31)
    nbr = R.pack_bits(adj).cuda()
    lv = {n: t.float().cuda().requires_grad_(True) for n, t in w.items()}

    def run():
        out = ops.nnconv(lv["x"], nbr, *(lv[n] for n in NAMES))
        (out * dy.float().cuda().reshape(30, 3)).sum().backward()

    run()
    torch.cuda.synchronize()
    first = {n: t.grad.clone() for n, t in lv.items()}
    st = ops.dev_state(lv["x"].device)
    st.grad_into_param, st.deferred_wgrad = True, (ops.WgradBatch() if route == "queued" else None)
    try:
        run()
        if route == "queued":
            assert len(st.deferred_wgrad.jobs) == Cin + 3       # nn.weight per c, nn.bias, root, the bias sum
            st.deferred_wgrad.flush()
    finally:
        st.grad_into_param, st.deferred_wgrad = False, None
    torch.cuda.synchronize()
    for n, t in lv.items():
        assert rel_err(t.grad.cpu(), 2 * first[n].cpu()) <= 2.0 ** -16, n


def test_no_grad_call_parks_nothing(monkeypatch):
    from mpgan_amd import ops
    w, adj, _ = _case(5, 3, 10, 4, 3, 41)
    seen = []
    real = ops.nnconv_launch
    monkeypatch.setattr(ops, "nnconv_launch", lambda *a, **k: (seen.append(k["pm"]), real(*a, **k))[1])
    lv = {n: t.float().cuda().requires_grad_(True) for n, t in w.items()}
    args = (lv["x"], R.pack_bits(adj).cuda(), *(lv[n] for n in NAMES))
    with torch.no_grad():
        y0 = ops.nnconv(*args)
    y1 = ops.nnconv(*args)
    assert seen[0] is None and seen[1] is not None and torch.equal(y0, y1.detach())


# ------------------------------------------------------------------------------------------------ the generator
def _net(cfg, sd=None, seed=0):
    from mpgan_amd import ext_models
    torch.manual_seed(seed)
    net = ext_models.GraphCNNGANG(args_of(dict(cfg, device="cpu")))
    if sd is not None:
        net.load_state_dict({k: (v.float() if v.is_floating_point() else v) for k, v in sd.items()}, strict=True)
    return net


def _spy(monkeypatch):
    from mpgan_amd import ops
    calls = []
    real = ops.nnconv_launch
    monkeypatch.setattr(ops, "nnconv_launch", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


@pytest.mark.parametrize("fused", [True, False])
def test_small_generator_vs_reference_golden(golden, monkeypatch, fused):
    """Training mode: output, noise gradient, every parameter gradient and the running statistics after the forward, on the fused
    route and on the un-fused one (which never calls the new launch)."""
    from mpgan_amd import ops
    monkeypatch.setitem(ops.OPTIONS, "nnconv", fused)
    calls = _spy(monkeypatch)
    sd = _sd(golden)
    net = _net(SMALL, sd).cuda().train()
    noise = golden["noise"].float().cuda().requires_grad_(True)
    out = net(noise)
    (out * golden["cot"].float().cuda()).sum().backward()
    torch.cuda.synchronize()
    assert len(calls) == (2 if fused else 0)
    err = rel_err(out.detach().cpu(), golden["out"])
    print(f"fused {fused}: out {err:.3g}")
    assert err <= TIGHT
    for k, v in net.state_dict().items():
        if "after." + k in golden:
            assert rel_err(v.cpu(), golden["after." + k]) <= TIGHT, k
    # the control: the module on the CPU in fp32 (the reference's arithmetic)
    cpu = _net(SMALL, sd).train()
    n32 = golden["noise"].float().requires_grad_(True)
    (cpu(n32) * golden["cot"].float()).sum().backward()
    keys = [k for k, _ in net.named_parameters()]
    got = {"dnoise": noise.grad.cpu().numpy(), **{k: p.grad.cpu().numpy() for k, p in net.named_parameters()}}
    ref = {"dnoise": golden["dnoise"].numpy(), **{k: golden["grad." + k].numpy() for k in keys}}
    control = {"dnoise": n32.grad.numpy(), **{k: p.grad.numpy() for k, p in cpu.named_parameters()}}
    assert_grads(got, ref, TOL, control=control, what=f"ext_models GraphCNNGANG fused={fused}")


def test_published_generator_on_the_gpu(published, monkeypatch):
    from mpgan_amd import gen
    calls = _spy(monkeypatch)
    sd, g = published
    G = _net(PUBLISHED, sd).cuda().eval()
    margs = {"latent_dim": 128}
    out = gen.gen(margs, G, 4, 30, model="graphcnngan", noise=torch.from_numpy(g["noise"]).cuda())
    err = rel_err(out.detach().cpu(), g["out"])
    print(f"published generator {err:.3g}")
    assert len(calls) == 2 and out.shape == (4, 30, 3) and err <= TIGHT
    assert gen.gen_multi_batch(margs, G, 4, 6, 30, out_device="cuda", detach=True, model="graphcnngan").shape == (6, 30, 3)


def test_double_backward_route_is_twice_differentiable(golden, monkeypatch):
    """Inside ``ops.double_backward_route`` the literal layer runs on ``MatMulFn`` / ATen and never on the fused launch: the output
    meets the golden one, and the gradient of |d out / d noise|^2 with respect to every parameter meets the fp64 CPU module's."""
    from mpgan_amd import ops
    sd = _sd(golden)
    calls = _spy(monkeypatch)

    def penalty(net, noise, cot):
        out = net(noise)
        (g,) = torch.autograd.grad((out * cot).sum(), noise, create_graph=True)
        (g ** 2).sum().backward()
        return out.detach(), {k: p.grad.cpu().numpy() for k, p in net.named_parameters() if p.grad is not None}

    net64 = _net(SMALL).double().train()
    net64.load_state_dict(sd, strict=True)
    ref_out, ref = penalty(net64, golden["noise"].clone().requires_grad_(True), golden["cot"])
    _, control = penalty(_net(SMALL, sd).train(), golden["noise"].float().requires_grad_(True), golden["cot"].float())
    net = _net(SMALL, sd).cuda().train()
    with ops.double_backward_route("cuda"):
        out, got = penalty(net, golden["noise"].float().cuda().requires_grad_(True), golden["cot"].float().cuda())
    torch.cuda.synchronize()
    assert not calls and set(got) == set(ref) == {k for k, _ in net.named_parameters()}
    assert rel_err(out.cpu(), ref_out) <= TIGHT and rel_err(ref_out, golden["out"]) <= 1e-12
    assert_grads(got, ref, TOL, control=control, what="ext_models GraphCNNGANG double backward")


def test_captured_forward_follows_in_place_weight_updates(published):
    """The eval-mode forward of the published generator captured with torch.cuda.graph replays to the eager result, and after an
    in-place change of the first edge network's weight and of a root to the new eager result: the launches read the raw parameters."""
    sd, g = published
    net = _net(PUBLISHED, sd).cuda().eval()
    noise = torch.from_numpy(g["noise"]).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.no_grad():
        with torch.cuda.stream(side):
            for _ in range(2):
                net(noise)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = net(noise)
        graph.replay()
        torch.cuda.synchronize()
        eager = net(noise)
        assert torch.equal(out, eager)
        net.edge_weights[0].weight.mul_(1.0 + 2.0 ** -6)
        net.layers[1].root.mul_(1.0 - 2.0 ** -6)
        graph.replay()
        torch.cuda.synchronize()
        eager2 = net(noise)
        assert torch.equal(out, eager2) and not torch.equal(eager, eager2)


def _decided_seed(B):
    """The first seed of range(100) whose randomly initialised published-shape net, in training mode on its noise, has neighbour
    sets and LeakyReLU signs that are decided (both margins >= 1e-4 in fp64): both routes then take the same ones."""
    for seed in range(100):
        net = _net(PUBLISHED, seed=seed).double().train()
        noise = torch.randn(B, 128, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 0.2
        probe = {}
        R.generator({k: v.detach() for k, v in net.state_dict().items()}, noise, 30, 20, 0.2, training=True, probe=probe)
        mz = min(float(z.abs().min() / z.abs().max()) for z in probe["z"])
        if R.rank_margin(probe["x"], 20, False) >= 1e-4 and mz >= 1e-4:
            return seed, noise.float()
    raise AssertionError("no decided seed in range(100)")


def test_one_rmsprop_step_against_rgand_equals_the_unfused_route(monkeypatch):
    """One eager RMSprop step of the generator against rGAND (the reference's default pairing), fused and un-fused.

    A convolution's bias sits in front of a training-mode batch norm, so its true gradient is zero and what either route returns for
    it is the fp32 rounding of a column sum that cancels: two such values have nothing to agree on.  Each route's gradients are
    therefore held to the fp64 CPU module's through ``assert_grads`` with TOL and the fp32 CPU module as control (the project's rule
    for a gradient that vanishes by symmetry), and every other parameter's gradient agrees between the routes within TOL directly.
    The stepped parameters agree within TOL wherever the step is decided: RMSprop's first step is lr g / (sqrt(0.01 g^2) + eps),
    +-10 lr whatever |g|, so an element whose gradient is below TOL of its tensor's largest may take either sign on either route,
    and the two biases throughout."""
    from mpgan_amd import ext_models, ops
    B = 4
    seed, noise = _decided_seed(B)
    calls = _spy(monkeypatch)
    vanishing = ("layers.0.bias", "layers.1.bias")

    def nets(cast):
        G = cast(_net(PUBLISHED, seed=seed)).train()
        torch.manual_seed(99)
        D = cast(ext_models.rGAND(types.SimpleNamespace(rgand_sfc=[64, 128], rgand_fc=[64], num_hits=30, node_feat_size=3,
                                                        leaky_relu_alpha=0.2)))
        return G, D

    def step(cast, z, fused=True):
        monkeypatch.setitem(ops.OPTIONS, "nnconv", fused)
        G, D = nets(cast)
        opt = torch.optim.RMSprop(G.parameters(), lr=1e-4)
        loss = ((D(G(z)) - 1.0) ** 2).mean()
        loss.backward()
        grads = {k: p.grad.cpu().numpy().copy() for k, p in G.named_parameters()}
        opt.step()
        assert bool(torch.isfinite(loss))
        return grads, {k: p.detach().cpu().numpy() for k, p in G.named_parameters()}

    ref, _ = step(lambda m: m.double(), noise.double())
    control, _ = step(lambda m: m, noise)
    g1, p1 = step(lambda m: m.cuda(), noise.cuda(), True)
    assert len(calls) == 2
    g0, p0 = step(lambda m: m.cuda(), noise.cuda(), False)
    torch.cuda.synchronize()
    assert len(calls) == 2
    assert_grads(g1, ref, TOL, control=control, what="GraphCNNGANG RMSprop step, fused")
    assert_grads(g0, ref, TOL, control=control, what="GraphCNNGANG RMSprop step, un-fused")
    for k in p0:
        if k in vanishing:
            continue
        err = rel_err(g1[k], g0[k])
        print(k, f"fused vs un-fused {err:.3g}")
        assert err <= TOL, k
        decided = np.abs(g0[k]) > TOL * np.abs(g0[k]).max()
        assert np.abs(p1[k] - p0[k])[decided].max() <= TOL * np.abs(p0[k]).max(), k
