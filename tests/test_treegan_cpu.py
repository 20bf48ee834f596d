"""CPU: the TreeGAN generator (``mpgan_amd.ext_models``: TreeGCN, TreeGANG) in fp64 against the reference's own outputs and gradients
(tests/golden/treegan.npz, tests/gen_golden_treegan.py), the restatement that ``ops.tree_gcn`` computes (tests/treegan_ref.py)
against autograd of the literal layer, the state-dict layout, the published generator's weights, the deliberate difference from the
reference (the caller's list is not grown), generation with ``model="treegan"``, and the host side of the op: ``MpgTreeGcn``'s
layout, the argument checks of mpg_tree_gcn_fwd / _bwd (which return before any launch) and the routing predicate."""
import ctypes as C
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import treegan_ref as R
from conftest import GOLDEN, load_golden, rel_err
from mpgan_amd import _lib, ext_models, gen, ops

BAR = 1e-12   # fp64 against the reference's own fp64 results


@pytest.fixture(scope="module")
def manifest():
    with open(os.path.join(GOLDEN, "treegan_manifest.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def golden():
    return {k: torch.from_numpy(np.asarray(v)) for k, v in load_golden("treegan.npz").items()}


@pytest.mark.parametrize("features, degrees, d, act", [([5, 7, 4, 6, 3], [3, 1, 2, 2], 2, True), ([5, 7, 4, 6, 3], [3, 1, 2, 2], 3, False),
                                                       ([5, 7, 4, 3], [3, 1, 2], 0, True)])
def test_restatement_equals_autograd_of_the_literal_layer(features, degrees, d, act):
    gen_ = torch.Generator().manual_seed(d)
    w = R.random_layer(features, degrees, d, 3, act, gen_)
    levels = R.random_levels(features, degrees, d, 4, gen_)
    leaves = [t.requires_grad_(True) for t in levels + w["W_root"] + [w["W_branch"], w["W0"], w["W1"]] + ([w["bias"]] if act else [])]
    y_lit = R.literal(levels, w)
    dy = torch.randn(y_lit.shape, generator=gen_, dtype=torch.float64)
    ref = torch.autograd.grad((y_lit * dy).sum(), leaves)
    with torch.no_grad():
        y, u = R.collapsed(levels, w)
        dlev, g = R.backward(levels, w, y, u, dy)
    assert rel_err(y, y_lit.detach()) <= BAR
    got = dlev + g["W_root"] + [g["W_branch"], g["W0"], g["W1"]] + ([g["bias"]] if act else [])
    assert g["bias"] is not None or not act
    for a, b in zip(got, ref):
        assert a.shape == b.shape and rel_err(a, b) <= BAR


def small_net(golden, manifest):
    net = ext_models.TreeGANG(**manifest["small"]).double()
    res = net.load_state_dict({k[3:]: v for k, v in golden.items() if k.startswith("sd.")})
    assert not res.missing_keys and not res.unexpected_keys
    return net


def test_module_fp64_matches_the_reference(golden, manifest):
    net = small_net(golden, manifest)
    noise = golden["noise"].clone().requires_grad_(True)
    tree = [noise]
    out = net(tree)
    (out * golden["cot"]).sum().backward()
    assert len(tree) == 1 and tree[0] is noise            # the caller's list is not grown
    assert out.shape == golden["out"].shape and net.pointcloud is out and torch.equal(net.getPointcloud(), out[-1])
    assert rel_err(out.detach(), golden["out"]) <= BAR and rel_err(noise.grad, golden["dnoise"]) <= BAR
    last = f"gcn.TreeGCN_{len(manifest['small']['degrees']) - 1}.bias"
    for k, p in net.named_parameters():
        if k == last:
            assert p.grad is None and "grad." + k not in golden    # never read by the forward
        else:
            assert rel_err(p.grad, golden["grad." + k]) <= BAR, k
    # a second call on the same list runs on the same one-level tree
    with torch.no_grad():
        assert torch.equal(net(tree), out.detach())


def test_restated_net_matches_the_reference_and_its_stored_margin(golden, manifest):
    sd = {k[3:]: v for k, v in golden.items() if k.startswith("sd.")}
    n = len(manifest["small"]["degrees"])
    assert rel_err(R.generator(sd, golden["noise"], n), golden["out"]) <= BAR
    assert rel_err(R.generator(sd, golden["noise"], n, fn=R.literal), golden["out"]) <= BAR
    probe, levels = {}, [golden["noise"]]
    for d in range(n):
        levels.append(R.collapsed(levels, R.layer_weights(sd, d, act=d < n - 1), probe=probe)[0])
    m = min(float(z.abs().min() / z.abs().max()) for z in probe["z"])
    assert abs(m - float(golden["margin_z"])) <= 1e-12 and m > 1e-4


def test_state_dict_shapes_equal_the_manifest(manifest):
    net = ext_models.TreeGANG(**manifest["args"])
    assert {k: list(v.shape) for k, v in net.state_dict().items()} == manifest["shapes"]
    layer = net.gcn.TreeGCN_2
    assert isinstance(layer, ext_models.TreeGCN) and (layer.depth, layer.node, layer.degree) == (2, 4, 2)
    # the reference's initialisation: xavier with relu gain on W_branch, uniform +-1 / sqrt(out) on the bias
    fan_in, fan_out = layer.W_branch.shape[1] * layer.W_branch.shape[2], layer.W_branch.shape[0] * layer.W_branch.shape[2]
    bound = 2 ** 0.5 * (6.0 / (fan_in + fan_out)) ** 0.5
    top = float(layer.W_branch.detach().abs().max())
    assert 0.9 * bound < top <= bound
    assert float(layer.bias.detach().abs().max()) <= 1.0 / 8.0


def test_published_generator_loads_and_reproduces_the_reference(manifest):
    G = ext_models.TreeGANG(**manifest["args"])
    sd = {k: torch.from_numpy(v) for k, v in load_golden("published_treegan_g_weights.npz").items()}
    assert sum(v.numel() for v in sd.values()) == 757158
    G.load_state_dict(sd, strict=True)
    g = load_golden("published_treegan_g.npz")
    with torch.no_grad():
        out = G.double()([torch.from_numpy(g["noise"]).double()])
    assert out.shape == (8, 32, 3) and rel_err(out, g["out"]) <= BAR


def test_treegan_noise_and_generation(manifest):
    margs = {"treegang_features": manifest["args"]["features"]}
    torch.manual_seed(0)
    noise, extra = gen.get_gen_noise(margs, 4000, 30, model="treegan", device="cpu", noise_std=0.3)
    assert isinstance(noise, list) and len(noise) == 1 and extra is None and noise[0].shape == (4000, 1, 96)
    n = noise[0].numel()
    # sampling error of a standard deviation over n draws is std / sqrt(2 n); five of them
    assert abs(float(noise[0].std()) - 0.3) <= 5 * 0.3 / (2 * n) ** 0.5 and abs(float(noise[0].mean())) <= 5 * 0.3 / n ** 0.5
    G = ext_models.TreeGANG(**manifest["args"])
    out = gen.gen(margs, G, 5, 30, model="treegan")
    assert out.shape == (5, 32, 3) and out.requires_grad
    out = gen.gen_multi_batch(margs, G, 3, 7, 30, out_device="cpu", detach=True, model="treegan")
    assert out.shape == (7, 32, 3) and not out.requires_grad
    with pytest.raises(NotImplementedError):
        gen.get_gen_noise_shape(margs, 7, 30, model="treegan")


def test_struct_layout_matches_the_header():
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    fields = [f[0] for f in _lib.MpgTreeGcn._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "mpgan_amd.h"\nint main(){'
           + "".join(f'printf("{f} %zu\\n", offsetof(MpgTreeGcn, {f}));' for f in fields)
           + 'printf("sizeof %zu\\n", sizeof(MpgTreeGcn));'
           + 'printf("limits %d %d %d %d\\n", MPG_TREE_GCN_MAX_LEVELS, MPG_TREE_GCN_MAX_WIDTH, MPG_TREE_GCN_MAX_BRANCH, '
             'MPG_TREE_GCN_MAX_NODES);return 0;}')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-I", inc, c, "-o", os.path.join(d, "t")], check=True)
        out = subprocess.run([os.path.join(d, "t")], check=True, capture_output=True, text=True).stdout
    lines = [line.split() for line in out.strip().splitlines()]
    limits = [int(v) for v in lines.pop()[1:]]
    got = {k: int(v) for k, v in lines}
    assert got.pop("sizeof") == C.sizeof(_lib.MpgTreeGcn)
    assert got == {f: getattr(_lib.MpgTreeGcn, f).offset for f in fields}
    assert tuple(limits) == ops.TREE_GCN_MAX == (8, 128, 256, 160)
    assert "mpg_tree_gcn_fwd" in _lib.SIGNATURES and "mpg_tree_gcn_bwd" in _lib.SIGNATURES


def _desc(B=4, nodes=(1, 3, 3), widths=(5, 7, 4), g=2, out=6):
    """A well-formed ``MpgTreeGcn`` over host dummies (the checks return before anything is read or launched)."""
    keep = torch.zeros(1 << 16)
    ptr = C.c_void_p(keep.data_ptr())
    e = _lib.MpgTreeGcn()
    for i, (n, w) in enumerate(zip(nodes, widths)):
        e.level[i], e.W_root[i], e.nodes[i], e.width[i] = keep.data_ptr(), keep.data_ptr(), n, w
    for name in ("W_branch", "Wc", "bias", "y", "u", "dy", "dz", "S", "du", "dx"):
        setattr(e, name, ptr)
    e.B, e.P, e.g, e.out, e.d, e.act, e.alpha = B, nodes[-1], g, out, len(nodes) - 1, 1, 0.2
    setattr(e, "in", widths[-1])
    e.ld_y = e.ld_dy = e.ld_dz = out
    e.ld_u = widths[-1]
    return e, keep


def _apply(e, over):
    for n, val in over.items():
        if isinstance(n, tuple):
            getattr(e, n[0])[n[1]] = val
        else:
            setattr(e, n, val)


SIZES = [({"B": 0}, -1), ({"out": 129}, -1), ({"in": 129, ("width", 2): 129}, -1), ({("width", 0): 129}, -1), ({"out": 0}, -1),
         ({"g": 65}, -1),                       # g in = 260 > 256
         ({"g": 54}, -1),                       # P g = 162 > 160
         ({"g": 0}, -1), ({"d": 8}, -1), ({"d": -1}, -1),
         ({("nodes", 1): 2}, -3),               # P = 3 is no multiple of 2
         ({("nodes", 2): 1}, -3), ({("width", 2): 5}, -3), ({"alpha": 1.5}, -4), ({"alpha": -0.1}, -4)]


@pytest.mark.parametrize("over, code", SIZES + [({"W_branch": None}, -2), ({"Wc": None}, -2), ({"y": None}, -2),
                                                ({("level", 1): None}, -2), ({("W_root", 0): None}, -2), ({"ld_y": 5}, -5),
                                                ({"ld_u": 3}, -5)])
def test_mpg_tree_gcn_fwd_declines_before_any_launch(over, code):
    e, keep = _desc()
    _apply(e, over)
    assert _lib.lib().mpg_tree_gcn_fwd(C.byref(e), None) == code, over


@pytest.mark.parametrize("over, code", SIZES + [({"W_branch": None}, -2), ({"Wc": None}, -2), ({"y": None}, -2), ({"u": None}, -2),
                                                ({"dy": None}, -2), ({"dz": None}, -2), ({"S": None}, -2), ({"du": None}, -2),
                                                ({"ld_dy": 5}, -5), ({"ld_dz": 5}, -5), ({"ld_u": 3}, -5), ({"ld_y": 5}, -5)])
def test_mpg_tree_gcn_bwd_declines_before_any_launch(over, code):
    e, keep = _desc()
    _apply(e, over)
    assert _lib.lib().mpg_tree_gcn_bwd(C.byref(e), None) == code, over


def test_null_descriptor_and_the_limits_themselves():
    assert _lib.lib().mpg_tree_gcn_fwd(None, None) == -2 and _lib.lib().mpg_tree_gcn_bwd(None, None) == -2
    # eight levels, width 128, g in = 256, P g = 160 pass the size checks: the next refusal is the NULL y
    e, keep = _desc(nodes=(1, 1, 1, 1, 1, 1, 1, 80), widths=(128,) * 8, g=2, out=128)
    e.ld_y = e.ld_dy = e.ld_dz = e.ld_u = 128
    e.y = None
    assert _lib.lib().mpg_tree_gcn_fwd(C.byref(e), None) == -2
    e, keep = _desc(nodes=(1, 3, 3), widths=(5, 7, 4), g=53, out=6)      # P g = 159, g in = 212
    e.y = None
    assert _lib.lib().mpg_tree_gcn_fwd(C.byref(e), None) == -2


def test_tree_gcn_route_at_the_limits():
    on, off = {"tree_gcn": True}, {"tree_gcn": False}
    assert ops.OPTIONS["tree_gcn"] is (os.environ.get("MPG_TREE_GCN", "1") != "0")
    F, D = [96, 64, 64, 64, 64, 3], [2, 2, 2, 2, 2]
    assert all(ops.tree_gcn_route(F, D, d, False, options=on) for d in range(5))
    assert not any(ops.tree_gcn_route(F, D, d, True, options=on) for d in range(5))      # the launch pair is once differentiable
    assert not any(ops.tree_gcn_route(F, D, d, False, options=off) for d in range(5))
    assert ops.tree_gcn_route([128, 128], [2], 0, False, options=on) and not ops.tree_gcn_route([128, 129], [2], 0, False, options=on)
    assert not ops.tree_gcn_route([129, 128], [1], 0, False, options=on)
    assert not ops.tree_gcn_route([129, 8, 8], [1, 1], 1, False, options=on)             # an ancestor level's width
    assert ops.tree_gcn_route([64, 8], [4], 0, False, options=on) and not ops.tree_gcn_route([65, 8], [4], 0, False, options=on)
    assert ops.tree_gcn_route([4, 4, 4], [80, 2], 1, False, options=on) and not ops.tree_gcn_route([4, 4, 4], [81, 2], 1, False, options=on)
    assert ops.tree_gcn_route([1, 1], [160], 0, False, options=on) and not ops.tree_gcn_route([1, 1], [161], 0, False, options=on)
    assert ops.tree_gcn_route([4] * 9, [1] * 8, 7, False, options=on) and not ops.tree_gcn_route([4] * 10, [1] * 9, 8, False, options=on)
    assert ops.tree_gcn_route([4, 4, 4], [3, 1], 1, False, options=on) and not ops.tree_gcn_route([4, 4], [0], 0, False, options=on)
    assert not ops.tree_gcn_route([4, 4], [2], 1, False, options=on)                     # no such layer
