"""CPU: the GraphCNN-GAN generator (``mpgan_amd.ext_models``: NNConv, GraphBatchNorm, GraphCNNGANG) in fp64 against the reference's
own outputs and gradients (tests/golden/graphcnn.npz, published_graphcnn_g.npz; tests/gen_golden_graphcnn.py), the factorised form
that ``ops.nnconv`` computes and its closed-form backward (tests/nnconv_ref.py) against the literal layer and autograd, the
state-dict layout, the published generator's weights, generation with ``model="graphcnngan"``, and the host side of the op:
``MpgNNConv``'s layout, the argument checks of mpg_nnconv_fwd / _bwd (which return before any launch) and the routing predicate."""
import ctypes as C
import os
import subprocess
import tempfile
import types

import numpy as np
import pytest
import torch

import nnconv_ref as R
from conftest import assert_grads, load_golden, rel_err
from mpgan_amd import _lib, ext_models, gen, ops

BAR = 1e-12   # fp64 against the reference's own fp64 results
SMALL = dict(latent_dim=7, num_hits=10, graphcnng_layers=[6, 5], node_feat_size=3, num_knn=4, leaky_relu_alpha=0.2,
             graphcnng_tanh=True, device="cpu")
PUBLISHED = dict(latent_dim=128, num_hits=30, graphcnng_layers=[32, 24], node_feat_size=3, num_knn=20, leaky_relu_alpha=0.2,
                 graphcnng_tanh=False, device="cpu")
KEYS = (["dense.weight", "dense.bias"]
        + [f"layers.{i}.{n}" for i in range(2) for n in ("root", "bias", "nn.weight", "nn.bias")]
        + [f"edge_weights.{i}.{n}" for i in range(2) for n in ("weight", "bias")]
        + [f"bn_layers.{i}.module.{n}" for i in range(2) for n in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")])


def args_of(d):
    return types.SimpleNamespace(**{k: (list(v) if isinstance(v, list) else v) for k, v in d.items()})


@pytest.fixture(scope="module")
def golden():
    return {k: torch.from_numpy(np.asarray(v)) for k, v in load_golden("graphcnn.npz").items()}


def random_layer(Cin, Cout, N, B, gen_, scale=1.0):
    r = lambda *s: torch.randn(*s, generator=gen_, dtype=torch.float64)
    return dict(x=r(B, N, Cin) * scale, nn_weight=r(Cin * Cout, Cin) / Cin ** 0.5, nn_bias=r(Cin * Cout) / Cin ** 0.5,
                root=r(Cin, Cout) / Cin ** 0.5, bias=r(Cout))


@pytest.mark.parametrize("Cin, Cout, N, k, loop", [(5, 3, 10, 4, False), (3, 4, 6, 6, True), (2, 2, 4, 7, False), (1, 1, 2, 1, False)])
def test_factorised_equals_literal_and_the_closed_form_backward_equals_autograd(Cin, Cout, N, k, loop):
    gen_ = torch.Generator().manual_seed(Cin + N)
    w = random_layer(Cin, Cout, N, 3, gen_)
    adj = R.knn_adjacency(w["x"], k, loop)
    assert adj.sum(2).max() == min(k, N if loop else N - 1)
    assert bool((torch.diagonal(adj, dim1=1, dim2=2) == (1.0 if loop else 0.0)).all())
    leaves = {n: t.clone().requires_grad_(True) for n, t in w.items()}
    y_lit = R.literal(leaves["x"], adj, *(leaves[n] for n in ("nn_weight", "nn_bias", "root", "bias")))
    dy = torch.randn(y_lit.shape, generator=gen_, dtype=torch.float64)
    ref = dict(zip(leaves, torch.autograd.grad((y_lit * dy).sum(), list(leaves.values()))))
    y, P, m = R.factorised(w["x"], adj, w["nn_weight"], w["nn_bias"], w["root"], w["bias"])
    assert rel_err(y, y_lit.detach()) <= BAR
    got = R.backward(w["x"], adj, w["nn_weight"], w["nn_bias"], w["root"], w["bias"], dy)
    for n in ref:
        assert got[n].shape == ref[n].shape and rel_err(got[n], ref[n]) <= BAR, n
    # the un-fused route's formulas on the CPU, and the packed words
    y_ops = ops.nnconv_literal(w["x"], adj, w["nn_weight"], w["nn_bias"], w["root"], w["bias"], 3, N, int(adj.sum(2).max()))
    assert rel_err(y_ops.reshape(3, N, Cout), y_lit.detach()) <= BAR
    assert torch.equal(R.unpack_bits(R.pack_bits(adj), 3, N), adj)
    assert torch.equal(ext_models.knn_adjacency(w["x"], k, loop), adj)


def test_an_empty_row_gets_a_zero_message_and_the_mean_is_over_the_listed():
    gen_ = torch.Generator().manual_seed(0)
    w = random_layer(4, 3, 5, 1, gen_)
    adj = torch.zeros(1, 5, 5, dtype=torch.float64)
    adj[0, 1, 3] = 1
    adj[0, 2, [0, 4]] = 1
    y = R.literal(w["x"], adj, w["nn_weight"], w["nn_bias"], w["root"], w["bias"])
    yf, P, m = R.factorised(w["x"], adj, w["nn_weight"], w["nn_bias"], w["root"], w["bias"])
    assert rel_err(yf, y) <= BAR
    assert torch.equal(y[0, 0], (w["x"][0, 0] @ w["root"] + w["bias"])) and float(P[0, 0].abs().max()) == 0.0
    assert rel_err(m[0, 2], w["x"][0, [0, 4]].mean(0)) <= BAR and rel_err(m[0, 1], w["x"][0, 3]) <= BAR
    y_ops = ops.nnconv_literal(w["x"], adj, w["nn_weight"], w["nn_bias"], w["root"], w["bias"], 1, 5, 2)
    assert rel_err(y_ops.reshape(1, 5, 3), y) <= BAR


def small_net(golden):
    net = ext_models.GraphCNNGANG(args_of(SMALL)).double()
    net.load_state_dict({k[3:]: v for k, v in golden.items() if k.startswith("sd.")}, strict=True)
    return net.train()


def test_module_fp64_matches_the_reference(golden):
    net = small_net(golden)
    noise = golden["noise"].clone().requires_grad_(True)
    out = net(noise)
    (out * golden["cot"]).sum().backward()
    assert out.shape == golden["out"].shape == (4, 10, 3)
    assert rel_err(out.detach(), golden["out"]) <= BAR and rel_err(noise.grad, golden["dnoise"]) <= BAR
    names = [k for k, _ in net.named_parameters()]
    assert sorted("grad." + k for k in names) == sorted(k for k in golden if k.startswith("grad."))
    # (a convolution's bias in front of a training-mode batch norm has a gradient that vanishes by symmetry: ``assert_grads`` holds
    # it to the net's largest gradient; 1e-10 = fp64 rounding of a sum of ~100 terms of the largest gradient's size over that 1e-3)
    assert_grads({k: p.grad for k, p in net.named_parameters()}, {k: golden["grad." + k] for k in names}, 1e-10, what="graphcnn.npz fp64")
    for k, v in net.state_dict().items():
        if "after." + k in golden:
            assert rel_err(v, golden["after." + k]) <= BAR, k


def test_restated_net_matches_the_reference_and_its_stored_margins(golden):
    sd = {k[3:]: v for k, v in golden.items() if k.startswith("sd.")}
    probe = {}
    out = R.generator(sd, golden["noise"], 10, 4, 0.2, tanh=True, training=True, probe=probe)
    assert rel_err(out, golden["out"]) <= BAR
    mr = R.rank_margin(probe["x"], 4, False)
    mz = min(float(z.abs().min() / z.abs().max()) for z in probe["z"])
    assert abs(mr - float(golden["margin_rank"])) <= 1e-12 and mr >= 1e-4
    assert abs(mz - float(golden["margin_z"])) <= 1e-12 and mz >= 1e-4


def test_published_generator_loads_and_reproduces_the_reference():
    G = ext_models.GraphCNNGANG(args_of(PUBLISHED))
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in load_golden("published_graphcnn_g_weights.npz").items()}
    assert sorted(sd) == sorted(KEYS) and len(KEYS) == 24 and sorted(G.state_dict()) == sorted(KEYS)
    G.load_state_dict(sd, strict=True)
    g = load_golden("published_graphcnn_g.npz")
    assert float(g["margin_rank"]) >= 1e-4
    with torch.no_grad():
        out = G.double().eval()(torch.from_numpy(g["noise"]).double())
    assert out.shape == (4, 30, 3) and rel_err(out, g["out"]) <= BAR


def test_the_edge_network_is_one_module_under_two_names():
    G = ext_models.GraphCNNGANG(args_of(PUBLISHED))
    for i in range(2):
        assert G.edge_weights[i] is G.layers[i].nn and G.edge_weights[i].weight is G.layers[i].nn.weight
        assert isinstance(G.bn_layers[i].module, torch.nn.BatchNorm1d)
    # dense 2, per layer root, bias, nn.weight, nn.bias, bn weight, bn bias
    assert len(list(G.parameters())) == 2 + 2 * 6
    assert sum(p.numel() for p in G.parameters()) == 128 * 960 + 960 + (32 * 24 + 24 + 768 * 32 + 768 + 48) + (24 * 3 + 3 + 72 * 24 + 72 + 6)


def test_root_and_bias_initialisation_and_the_refusals():
    torch.manual_seed(0)
    conv = ext_models.NNConv(64, 40, torch.nn.Linear(64, 64 * 40))
    assert conv.root.shape == (64, 40) and conv.bias.shape == (40,)
    bound = 1.0 / 8.0
    assert 0.95 * bound < float(conv.root.detach().abs().max()) <= bound and float(conv.bias.detach().abs().max()) <= bound
    assert abs(float(conv.root.detach().mean())) <= 5 * bound / (3 * 64 * 40) ** 0.5
    for kw, word in [(dict(aggr="add"), "add"), (dict(aggr="max"), "max"), (dict(root_weight=False), "root_weight"),
                     (dict(bias=False), "bias"), (dict(flow="target_to_source"), "flow")]:
        with pytest.raises(NotImplementedError, match=word):
            ext_models.NNConv(4, 3, torch.nn.Linear(4, 12), **kw)


def test_running_statistics_follow_batchnorm1d():
    torch.manual_seed(1)
    bn, ref = ext_models.GraphBatchNorm(5), torch.nn.BatchNorm1d(5)
    assert sorted(bn.state_dict()) == sorted("module." + k for k in ref.state_dict())
    for _ in range(2):
        x = torch.randn(40, 5) * 3 + 1
        assert torch.equal(bn(x), ref(x))
    for k, v in ref.state_dict().items():
        assert torch.equal(bn.state_dict()["module." + k], v), k
    assert int(bn.module.num_batches_tracked) == 2
    bn.eval(), ref.eval()
    assert torch.equal(bn(x), ref(x))


def test_graphcnngan_noise_and_generation():
    margs = {"latent_dim": 128}
    torch.manual_seed(0)
    noise, extra = gen.get_gen_noise(margs, 4000, 30, model="graphcnngan", device="cpu", noise_std=0.3)
    assert extra is None and noise.shape == (4000, 128)
    n = noise.numel()
    # sampling error of a standard deviation over n draws is std / sqrt(2 n); five of them
    assert abs(float(noise.std()) - 0.3) <= 5 * 0.3 / (2 * n) ** 0.5 and abs(float(noise.mean())) <= 5 * 0.3 / n ** 0.5
    G = ext_models.GraphCNNGANG(args_of(PUBLISHED))
    out = gen.gen(margs, G, 5, 30, model="graphcnngan")
    assert out.shape == (5, 30, 3) and out.requires_grad
    out = gen.gen_multi_batch(margs, G, 3, 7, 30, out_device="cpu", detach=True, model="graphcnngan")
    assert out.shape == (7, 30, 3) and not out.requires_grad
    with pytest.raises(NotImplementedError):
        gen.get_gen_noise_shape(margs, 7, 30, model="graphcnngan")


def test_struct_layout_matches_the_header():
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    fields = [f[0] for f in _lib.MpgNNConv._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "mpgan_amd.h"\nint main(){'
           + "".join(f'printf("{f} %zu\\n", offsetof(MpgNNConv, {f}));' for f in fields)
           + 'printf("sizeof %zu\\n", sizeof(MpgNNConv));'
           + 'printf("limits %d %d %d\\n", MPG_NNCONV_MAX_N, MPG_NNCONV_MAX_C, MPG_NNCONV_MAX_B);return 0;}')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-I", inc, c, "-o", os.path.join(d, "t")], check=True)
        out = subprocess.run([os.path.join(d, "t")], check=True, capture_output=True, text=True).stdout
    lines = [line.split() for line in out.strip().splitlines()]
    limits = [int(v) for v in lines.pop()[1:]]
    got = {k: int(v) for k, v in lines}
    assert got.pop("sizeof") == C.sizeof(_lib.MpgNNConv)
    assert got == {f: getattr(_lib.MpgNNConv, f).offset for f in fields}
    assert tuple(limits) == (_lib.NNCONV_MAX_N, _lib.NNCONV_MAX_C, _lib.NNCONV_MAX_B) == (160, 64, 1 << 20)
    assert ops.NNCONV_MAX == (160, 64, 64)
    assert "mpg_nnconv_fwd" in _lib.SIGNATURES and "mpg_nnconv_bwd" in _lib.SIGNATURES


def _desc(B=4, N=30, Cin=32, Cout=24):
    """A well-formed ``MpgNNConv`` over host dummies (the checks return before anything is read or launched)."""
    keep = torch.zeros(1 << 12)
    ptr = C.c_void_p(keep.data_ptr())
    e = _lib.MpgNNConv()
    for name in ("x", "nbr", "nn_weight", "nn_bias", "root", "bias", "y", "pm", "dy", "g", "dx"):
        setattr(e, name, ptr)
    e.B, e.N, e.Cin, e.Cout = B, N, Cin, Cout
    e.ld_x = e.ld_dx = Cin
    e.ld_y = e.ld_dy = Cout
    return e, keep


SIZES = [({"B": 0}, -1), ({"B": (1 << 20) + 1}, -1), ({"N": 0}, -1), ({"N": 161}, -1), ({"Cin": 0}, -1), ({"Cin": 65, "ld_x": 65, "ld_dx": 65}, -1),
         ({"Cout": 0}, -1), ({"Cout": 65, "ld_y": 65, "ld_dy": 65}, -1),
         ({"x": None}, -2), ({"nbr": None}, -2), ({"nn_weight": None}, -2), ({"nn_bias": None}, -2), ({"root": None}, -2), ({"ld_x": 31}, -5)]


@pytest.mark.parametrize("over, code", SIZES + [({"bias": None}, -2), ({"y": None}, -2), ({"ld_y": 23}, -5)])
def test_mpg_nnconv_fwd_declines_before_any_launch(over, code):
    e, keep = _desc()
    for n, v in over.items():
        setattr(e, n, v)
    assert _lib.lib().mpg_nnconv_fwd(C.byref(e), None) == code, over


@pytest.mark.parametrize("over, code", SIZES + [({"pm": None}, -2), ({"dy": None}, -2), ({"g": None}, -2), ({"dx": None}, -2),
                                                ({"ld_dy": 23}, -5), ({"ld_dx": 31}, -5)])
def test_mpg_nnconv_bwd_declines_before_any_launch(over, code):
    e, keep = _desc()
    for n, v in over.items():
        setattr(e, n, v)
    assert _lib.lib().mpg_nnconv_bwd(C.byref(e), None) == code, over


def test_null_descriptor_and_the_limits_themselves():
    assert _lib.lib().mpg_nnconv_fwd(None, None) == -2 and _lib.lib().mpg_nnconv_bwd(None, None) == -2
    # N = 160 and both widths 64 pass the size checks: the next refusal is the NULL y / dx
    e, keep = _desc(B=1 << 20, N=160, Cin=64, Cout=64)
    e.y = e.dx = None
    assert _lib.lib().mpg_nnconv_fwd(C.byref(e), None) == -2 and _lib.lib().mpg_nnconv_bwd(C.byref(e), None) == -2


def test_nnconv_route_at_the_limits():
    on, off = {"nnconv": True}, {"nnconv": False}
    assert ops.OPTIONS["nnconv"] is (os.environ.get("MPG_NNCONV", "1") != "0")
    for shape in [(30, 32, 24), (30, 24, 3), (160, 64, 64), (1, 1, 1)]:
        assert ops.nnconv_route(*shape, False, options=on)
        assert not ops.nnconv_route(*shape, True, options=on)       # the launch pair is once differentiable
        assert not ops.nnconv_route(*shape, False, options=off)
    for shape in [(161, 64, 64), (160, 65, 64), (160, 64, 65), (0, 4, 4), (4, 0, 4), (4, 4, 0)]:
        assert not ops.nnconv_route(*shape, False, options=on)
