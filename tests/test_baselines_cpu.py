"""CPU: the set-pooling baselines (``mpgan_amd.ext_models``: rGANG, rGAND, PointNetMixD) in fp64 against the reference's own outputs
and gradients (tests/golden/baselines.npz, tests/gen_golden_baselines.py), their state-dict layout, the published FC generator's
weights, the two deliberate differences from the reference (nothing of the caller's is modified), and the host side of the
layer-and-pool op: ``MpgPointPool``'s layout, the argument checks of mpg_point_pool_fwd / _bwd (which return before any launch), the
routing predicate and the rgan noise shape."""
import copy
import ctypes as C
import json
import os
import subprocess
import tempfile
import types

import numpy as np
import pytest
import torch

import baselines_ref as R
from conftest import GOLDEN, load_golden, rel_err
from mpgan_amd import _lib, ext_models, gen, ops

BAR = 1e-10   # the bar of test_oracle_golden.py: fp64 against fp64
N, FS = 30, 3
SMALL = dict(latent_dim=16, rgang_fc=[24, 32], rgand_sfc=[32, 48, 96], rgand_fc=[40, 24], pointnetd_pointfc=[32, 48, 160],
             pointnetd_fc=[64], num_hits=N, node_feat_size=FS, leaky_relu_alpha=0.2, mask=True)


def small_args():
    return types.SimpleNamespace(**copy.deepcopy(SMALL))


@pytest.fixture(scope="module")
def golden():
    return load_golden("baselines.npz")


def case(g, name):
    """(state dict, x, cot, out, dx, grads) of one net of baselines.npz as fp64 tensors."""
    t = lambda a: torch.from_numpy(np.asarray(a))
    sd = {k[len(name) + 4:]: t(v) for k, v in g.items() if k.startswith(name + ".sd.")}
    gr = {k[len(name) + 6:]: t(v) for k, v in g.items() if k.startswith(name + ".grad.")}
    return sd, t(g[name + ".x"]), t(g["cot"]), t(g[name + ".out"]), t(g[name + ".dx"]), gr


RESTATED = {"rgand": lambda sd, x: R.rgand(sd, x, N, FS), "pnet": lambda sd, x: R.pointnet_mix(sd, x, N, FS, mask=True)}
MODULES = {"rgand": ext_models.rGAND, "pnet": ext_models.PointNetMixD}


@pytest.mark.parametrize("name", ["rgand", "pnet"])
def test_restatement_matches_the_reference(golden, name):
    sd, x, cot, out, dx, gr = case(golden, name)
    o, gx, gp = R.grads(RESTATED[name], sd, x, cot)
    assert rel_err(o, out) <= BAR and rel_err(gx, dx) <= BAR
    assert set(gp) == set(gr)
    for k in gr:
        assert rel_err(gp[k], gr[k]) <= BAR, k


@pytest.mark.parametrize("name", ["rgand", "pnet"])
def test_modules_fp64_match_the_reference(golden, name):
    sd, x, cot, out, dx, gr = case(golden, name)
    net = MODULES[name](small_args()).double()
    res = net.load_state_dict(sd)
    assert not res.missing_keys and not res.unexpected_keys
    xi = x.clone().requires_grad_(True)
    o = net(xi)
    (o * cot).sum().backward()
    assert o.shape == out.shape
    assert rel_err(o.detach(), out) <= BAR and rel_err(xi.grad, dx) <= BAR
    for k, p in net.named_parameters():
        assert rel_err(p.grad, gr[k]) <= BAR, k


def test_margins_of_the_fixture_are_those_stored(golden):
    """The stored margins are the restatement's on the stored input: what the GPU tests' bars lean on."""
    mz, gap = [], []
    for name, real in (("rgand", (N,) * 4), ("pnet", tuple(int(v) for v in golden["real"]))):
        sd, x = case(golden, name)[:2]
        probe = {}
        (R.rgand if name == "rgand" else R.pointnet_mix)(sd, x, N, FS, probe=probe)
        mz.append(min(float(z.abs().min() / z.abs().max()) for z in probe["z"]))
        y = probe["pool_y"]
        gap.append(min(float(R.top_two_gap(y[b:b + 1, :min(n + 1, N)]).min()) for b, n in enumerate(real)) / float(y.abs().max()))
    assert abs(min(mz) - float(golden["margin_z"])) <= 1e-12 and abs(min(gap) - float(golden["margin_gap"])) <= 1e-12
    assert min(mz) > 1e-5 and min(gap) > 1e-5


def test_state_dict_shapes_equal_the_manifest():
    with open(os.path.join(GOLDEN, "baselines_manifest.json")) as f:
        man = json.load(f)
    for cls, shapes in man["shapes"].items():
        net = getattr(ext_models, cls)(types.SimpleNamespace(**copy.deepcopy(man["args"])))
        assert {k: list(v.shape) for k, v in net.state_dict().items()} == shapes, cls


def test_published_fc_generator_loads_and_reproduces_the_reference():
    with open(os.path.join(GOLDEN, "baselines_manifest.json")) as f:
        args = types.SimpleNamespace(**json.load(f)["args"])
    G = ext_models.rGANG(args)
    res = G.load_state_dict({k: torch.from_numpy(v) for k, v in load_golden("published_fc_g_weights.npz").items()})
    assert not res.missing_keys and not res.unexpected_keys
    g = load_golden("published_fc_g.npz")
    with torch.no_grad():
        out = G.double()(torch.from_numpy(g["noise"]).double())
    assert out.shape == (8, N, FS) and rel_err(out, g["out"]) <= BAR
    sd = {k: v.double() for k, v in G.state_dict().items()}
    assert rel_err(R.rgang(sd, torch.from_numpy(g["noise"]).double(), N, FS), g["out"]) <= BAR


def test_nothing_of_the_callers_is_modified(golden):
    """The two deliberate differences: ``args``' lists and the input tensor are bit-identical after construction and a call."""
    args = small_args()
    before = copy.deepcopy(vars(args))
    nets = [ext_models.rGANG(args), ext_models.rGAND(args), ext_models.PointNetMixD(args)]
    assert vars(args) == before
    x = torch.from_numpy(golden["pnet.x"]).float()
    x0 = x.clone()
    with torch.no_grad():
        nets[2](x)
        nets[1](x[:, :, :3])
    assert torch.equal(x, x0) and vars(args) == before
    assert "_shift" not in nets[2].state_dict()


def test_struct_layout_matches_the_header():
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    fields = [f[0] for f in _lib.MpgPointPool._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "mpgan_amd.h"\nint main(){'
           + "".join(f'printf("{f} %zu\\n", offsetof(MpgPointPool, {f}));' for f in fields)
           + 'printf("sizeof %zu\\n", sizeof(MpgPointPool));'
           + 'printf("limits %d %d %d\\n", MPG_POINT_POOL_MAX_N, MPG_POINT_POOL_MAX_K, MPG_POINT_POOL_MAX_C);return 0;}')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-I", inc, c, "-o", os.path.join(d, "t")], check=True)
        out = subprocess.run([os.path.join(d, "t")], check=True, capture_output=True, text=True).stdout
    lines = [line.split() for line in out.strip().splitlines()]
    limits = [int(v) for v in lines.pop()[1:]]
    got = {k: int(v) for k, v in lines}
    assert got.pop("sizeof") == C.sizeof(_lib.MpgPointPool)
    assert got == {f: getattr(_lib.MpgPointPool, f).offset for f in fields}
    assert tuple(limits) == ops.POINT_POOL_MAX == (160, 256, 1024)
    assert "mpg_point_pool_fwd" in _lib.SIGNATURES and "mpg_point_pool_bwd" in _lib.SIGNATURES


def _desc(B=2, N=30, K=20, Cn=40, mode=3):
    """A well-formed ``MpgPointPool`` over host dummies (the checks return before anything is read or launched)."""
    keep = [torch.zeros(B * N * max(K, Cn, 64)) for _ in range(8)]
    e = _lib.MpgPointPool()
    for n, buf in zip(("x", "W", "bias", "pooled", "argmax", "neg", "gpooled", "dz"), keep):
        setattr(e, n, C.c_void_p(buf.data_ptr()))
    e.ldx, e.ldw, e.ld_pooled, e.ld_gpooled, e.ld_dz = K, K, 2 * Cn, 2 * Cn, Cn
    e.B, e.N, e.K, e.C, e.act, e.alpha, e.mode, e.f16 = B, N, K, Cn, 1, 0.2, mode, 1
    return e, keep


FWD_REFUSALS = [(dict(B=0), -1), (dict(N=161), -1), (dict(N=0), -1), (dict(K=257), -1), (dict(K=0), -1), (dict(C=1025), -1),
                (dict(C=0), -1), (dict(mode=0), -3), (dict(mode=4), -3), (dict(alpha=2.0), -4), (dict(alpha=-0.1), -4),
                (dict(f16=0), -6), (dict(x=None), -2), (dict(W=None), -2), (dict(pooled=None), -2), (dict(ldx=19), -5),
                (dict(ldw=19), -5), (dict(ld_pooled=79), -5)]


@pytest.mark.parametrize("over, code", FWD_REFUSALS)
def test_mpg_point_pool_fwd_declines_before_any_launch(over, code):
    e, keep = _desc()
    for n, val in over.items():
        setattr(e, n, val)
    assert _lib.lib().mpg_point_pool_fwd(C.byref(e), None) == code, over


@pytest.mark.parametrize("over, code", [(dict(B=0), -1), (dict(N=161), -1), (dict(C=1025), -1), (dict(mode=0), -3),
                                        (dict(alpha=2.0), -4), (dict(f16=0), -6), (dict(gpooled=None), -2), (dict(dz=None), -2),
                                        (dict(argmax=None), -2), (dict(neg=None), -2), (dict(ld_dz=39), -5),
                                        (dict(ld_gpooled=79), -5)])
def test_mpg_point_pool_bwd_declines_before_any_launch(over, code):
    e, keep = _desc()
    for n, val in over.items():
        setattr(e, n, val)
    assert _lib.lib().mpg_point_pool_bwd(C.byref(e), None) == code, over


def test_point_pool_route_at_the_limits():
    on, off = {"point_pool": True}, {"point_pool": False}
    assert ops.OPTIONS["point_pool"] is (os.environ.get("MPG_POINT_POOL", "1") != "0")
    assert ops.point_pool_route(30, 128, 1024, False, options=on)
    assert ops.point_pool_route(1, 1, 1, False, options=on) and ops.point_pool_route(160, 256, 1024, False, options=on)
    for n, k, c in ((161, 128, 512), (0, 128, 512), (30, 257, 512), (30, 0, 512), (30, 128, 1025), (30, 128, 0)):
        assert not ops.point_pool_route(n, k, c, False, options=on), (n, k, c)
    assert not ops.point_pool_route(30, 128, 512, True, options=on)       # the launch pair is once differentiable
    assert not ops.point_pool_route(30, 128, 512, False, options=off)


def test_rgan_noise_shape():
    assert gen.get_gen_noise_shape({"latent_dim": 128}, 7, 30, model="rgan") == (7, 128)
    noise, extra = gen.get_gen_noise({"latent_dim": 16}, 5, 30, model="rgan", device="cpu")
    assert noise.shape == (5, 16) and extra is None
    G = ext_models.rGANG(small_args())
    out = gen.gen_multi_batch({"latent_dim": 16}, G, 3, 7, 30, out_device="cpu", detach=True, model="rgan")
    assert out.shape == (7, N, FS)
    for other in ("treegan", "graphcnngan", "pcgan"):
        with pytest.raises(NotImplementedError):
            gen.get_gen_noise_shape({"latent_dim": 128}, 7, 30, model=other)
