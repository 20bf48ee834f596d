"""CPU: PCGAN's networks (``mpgan_amd.ext_models``: the equivariant layers, G_inv_Tanh, G_inv, G, latent_G, latent_D) in fp64 against
the reference's own outputs and gradients (tests/golden/pcgan*.npz, tests/gen_golden_pcgan.py), the restatement that
``ops.set_encode_launch`` computes (tests/pcgan_ref.py) against the same fixtures, the state-dict layout, the published encoder's
weights, ``load_pcgan_encoder``, generation with ``model="pcgan"``, and the host side of the op: ``MpgSetEncode``'s layout, the
argument checks of mpg_set_encode_fwd (which return before any HIP call) and the routing predicate."""
import ctypes as C
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import pcgan_ref as R
from conftest import GOLDEN, load_golden, rel_err
from mpgan_amd import _lib, ext_models, gen, ops

BAR = 1e-12   # fp64 against the reference's own fp64 results


@pytest.fixture(scope="module")
def manifest():
    with open(os.path.join(GOLDEN, "pcgan_manifest.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def golden():
    return {k: torch.from_numpy(np.asarray(v)) for k, v in load_golden("pcgan.npz").items()}


NETS = ["enc_max1", "enc_max", "enc_mean", "enc_max1_x4", "encsp_mean", "dec", "latent_G", "latent_D"]


def small_net(name, golden, manifest):
    spec = manifest["small"][name]
    net = getattr(ext_models, spec["class"])(*spec["args"])
    sd = {k[len(name) + 4:]: v for k, v in golden.items() if k.startswith(name + ".sd.")}
    net.load_state_dict(sd, strict=True)
    return net, sd


def test_the_fixture_has_every_net_the_pipeline_uses(manifest):
    assert sorted(manifest["small"]) == sorted(NETS)
    assert {v["class"] for v in manifest["small"].values()} == {"G_inv_Tanh", "G_inv", "G", "latent_G", "latent_D"}
    pools = {tuple(v["args"][::3]) for v in manifest["small"].values() if v["class"] == "G_inv_Tanh"}
    assert pools == {(3, "max1"), (3, "max"), (3, "mean"), (4, "max1")}


@pytest.mark.parametrize("name", NETS)
def test_module_fp64_matches_the_reference(name, golden, manifest, capsys):
    net, _ = small_net(name, golden, manifest)
    assert capsys.readouterr().out == ""                                   # the constructors do not print the module
    net = net.double()
    xs = [golden[f"{name}.{t}"].double().requires_grad_(True) for t in ("x", "x2") if f"{name}.{t}" in golden]
    out = net(*xs)
    (out * golden[f"{name}.cot"]).sum().backward()
    assert out.shape == golden[f"{name}.out"].shape and rel_err(out.detach(), golden[f"{name}.out"]) <= BAR
    for t, x in zip(("dx", "dx2"), xs):
        assert rel_err(x.grad, golden[f"{name}.{t}"]) <= BAR, t
    params = dict(net.named_parameters())
    grads = {k[len(name) + 6:] for k in golden if k.startswith(name + ".grad.")}
    assert grads == set(params)
    for k, p in params.items():
        assert rel_err(p.grad, golden[f"{name}.grad.{k}"]) <= BAR, k


@pytest.mark.parametrize("name", [n for n in NETS if n.startswith("enc")])
def test_restatement_matches_the_reference(name, golden, manifest):
    spec = manifest["small"][name]
    sd = {k[len(name) + 4:]: v.double() for k, v in golden.items() if k.startswith(name + ".sd.")}
    pool, act = R.POOLS[spec["args"][3]], R.ACTS["tanh" if spec["class"] == "G_inv_Tanh" else "softplus"]
    x = golden[f"{name}.x"].double()
    assert rel_err(R.encoder(sd, x, pool, act), golden[f"{name}.out"]) <= BAR
    # what the restated stack returns is what the module's own route computes in front of ``ro``
    net, _ = small_net(name, golden, manifest)
    with torch.no_grad():
        assert rel_err(R.stack(x, *R.stack_weights(sd, pool), pool, act), net.double().pooled(x)) <= BAR
    assert float(x.max()) <= -1.0


def test_state_dict_shapes_equal_the_manifest(manifest):
    for cls, args in manifest["args"].items():
        net = getattr(ext_models, cls)(*args)
        assert {k: list(v.shape) for k, v in net.state_dict().items()} == manifest["shapes"][cls], cls
    enc = ext_models.G_inv_Tanh(3, 8, 5, "max")
    assert isinstance(enc.phi[0], ext_models.PermEqui2_max) and isinstance(enc.phi[1], torch.nn.Tanh)
    assert isinstance(ext_models.G_inv(3, 8, 5, "mean").phi[4], ext_models.PermEqui2_mean)
    assert isinstance(ext_models.G_inv(3, 8, 5, "max1").phi[2], ext_models.PermEqui1_max)
    assert isinstance(ext_models.G_inv(3, 8, 5).ro[1], torch.nn.Softplus) and ext_models.G_inv(3, 8, 5).pool == "mean"
    assert len(enc.faster_parameters) == len(list(enc.parameters()))
    for missing in ("D", "skipD", "skipG", "ALPHA"):
        assert not hasattr(ext_models, missing)


def published():
    sd = {k: torch.from_numpy(v) for k, v in load_golden("published_pcgan_g_inv_t_weights.npz").items()}
    return sd, load_golden("published_pcgan_g_inv_t.npz")


def test_published_encoder_loads_and_reproduces_the_reference(manifest):
    sd, g = published()
    assert sum(v.numel() for v in sd.values()) == 264192
    assert abs(max(float(v.abs().max()) for v in sd.values()) - 6.598) < 1e-3
    enc = ext_models.G_inv_Tanh(*manifest["args"]["G_inv_Tanh"])
    enc.load_state_dict(sd, strict=True)
    with torch.no_grad():
        out = enc.double()(torch.from_numpy(g["x"]).double())
    assert out.shape == (8, 256) and rel_err(out, g["out"]) <= BAR


def test_load_pcgan_encoder_leaves_nothing_requiring_grad(tmp_path):
    sd, g = published()
    enc = ext_models.load_pcgan_encoder(sd, 3, 256, 256, "max1")
    assert isinstance(enc, ext_models.G_inv_Tanh) and not enc.training
    assert not any(p.requires_grad for p in enc.parameters()) and not any(p.requires_grad for p in enc.faster_parameters)
    out = enc(torch.from_numpy(g["x"]))            # grad mode on: nothing to differentiate
    assert not out.requires_grad and rel_err(out, g["out"]) <= 1e-4
    path = os.path.join(tmp_path, "enc.pt")
    torch.save(sd, path)
    again = ext_models.load_pcgan_encoder(path, 3, 256, 256, "max1")
    assert all(torch.equal(a, b) for a, b in zip(again.state_dict().values(), enc.state_dict().values()))
    with pytest.raises(RuntimeError):
        ext_models.load_pcgan_encoder(sd, 3, 256, 256, "max")       # strict: no Lambda in the file
    with pytest.raises(ValueError):
        ext_models.G_inv_Tanh(3, 8, 8, "sum")


def test_struct_layout_matches_the_header():
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    fields = [f[0] for f in _lib.MpgSetEncode._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "mpgan_amd.h"\nint main(){'
           + "".join(f'printf("{f} %zu\\n", offsetof(MpgSetEncode, {f}));' for f in fields)
           + 'printf("sizeof %zu\\n", sizeof(MpgSetEncode));'
           + 'printf("limits %d %d %d\\n", MPG_SET_ENC_MAX_N, MPG_SET_ENC_MAX_D, MPG_SET_ENC_MAX_LAYERS);return 0;}')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-I", inc, c, "-o", os.path.join(d, "t")], check=True)
        out = subprocess.run([os.path.join(d, "t")], check=True, capture_output=True, text=True).stdout
    lines = [line.split() for line in out.strip().splitlines()]
    limits = [int(v) for v in lines.pop()[1:]]
    got = {k: int(v) for k, v in lines}
    assert got.pop("sizeof") == C.sizeof(_lib.MpgSetEncode)
    assert got == {f: getattr(_lib.MpgSetEncode, f).offset for f in fields}
    assert tuple(limits) == ops.SET_ENC_MAX == (128, 256, 4)
    assert "mpg_set_encode_fwd" in _lib.SIGNATURES


def _desc(B=4, N=30, widths=(3, 40, 40, 24), pool=2, act=2):
    """A well-formed ``MpgSetEncode`` over host dummies (the checks return before anything is read or launched)."""
    keep = torch.zeros(1 << 16)
    e = _lib.MpgSetEncode()
    e.x = e.pooled = C.c_void_p(keep.data_ptr())
    e.B, e.N, e.L, e.pool, e.act = B, N, len(widths) - 1, pool, act
    for l in range(len(widths) - 1):
        e.K[l], e.D[l] = widths[l], widths[l + 1]
        e.Gamma[l] = e.bias[l] = e.Lambda[l] = keep.data_ptr()
    e.ldx, e.ld_pooled = widths[0], widths[-1]
    return e, keep


def _apply(e, over):
    for n, val in over.items():
        if isinstance(n, tuple):
            getattr(e, n[0])[n[1]] = val
        else:
            setattr(e, n, val)


@pytest.mark.parametrize("over, code", [
    ({"B": 0}, -1), ({"N": 0}, -1), ({"N": 129}, -1), ({"L": 0}, -1), ({"L": 5}, -1),
    ({("K", 0): 0}, -1), ({("K", 0): 257, "ldx": 257}, -1), ({("D", 2): 0}, -1), ({("D", 2): 257, "ld_pooled": 257}, -1),
    ({("D", 0): 257, ("K", 1): 257}, -1),
    ({("K", 1): 39}, -1), ({("D", 1): 41}, -1),               # widths that do not chain
    ({"x": None}, -2), ({"pooled": None}, -2), ({("Gamma", 1): None}, -2), ({("Lambda", 2): None}, -2),
    ({"pool": 0}, -3), ({"pool": 4}, -3), ({"act": 1}, -3), ({"act": 4}, -3), ({"act": 0}, -3),
    ({"ldx": 2}, -5), ({"ld_pooled": 23}, -5)])
def test_mpg_set_encode_fwd_declines_before_any_hip_call(over, code):
    e, keep = _desc()
    _apply(e, over)
    assert _lib.lib().mpg_set_encode_fwd(C.byref(e), None) == code, over


def test_null_descriptor_the_limits_themselves_and_what_is_not_needed():
    fwd = _lib.lib().mpg_set_encode_fwd
    assert fwd(None, None) == -2
    # N = 128, four layers of 256 pass the size checks: the next refusal is the NULL pooled
    e, keep = _desc(N=128, widths=(256,) * 5)
    e.pooled = None
    assert fwd(C.byref(e), None) == -2
    # pool 1 reads no Lambda, and a bias may be absent: the next refusal is the short stride
    e, keep = _desc(pool=1)
    for l in range(3):
        e.Lambda[l] = e.bias[l] = None
    e.ldx = 2
    assert fwd(C.byref(e), None) == -5
    # the slots behind L are not looked at
    e, keep = _desc(widths=(3, 40))
    e.K[1], e.D[1], e.ld_pooled = 7, 999, 39
    assert fwd(C.byref(e), None) == -5


def test_set_encode_route_at_the_limits():
    on, off = {"set_encode": True}, {"set_encode": False}
    assert ops.OPTIONS["set_encode"] is (os.environ.get("MPG_SET_ENCODE", "1") != "0")
    W = [3, 256, 256, 256]
    route = lambda N=30, widths=W, pool=1, act=2, grad=False, dbl=False, options=on: ops.set_encode_route(N, widths, pool, act, grad, dbl,
                                                                                                      options=options)
    assert route() and route(pool="max1", act="tanh") and route(pool="mean", act="softplus") and route(pool=3, act=3)
    assert route(N=128) and not route(N=129) and route(N=1) and not route(N=0)
    assert route(widths=[256, 256]) and not route(widths=[3, 257, 256]) and not route(widths=[257, 8]) and not route(widths=[3, 0])
    assert route(widths=[3, 8, 8, 8, 8]) and not route(widths=[3, 8, 8, 8, 8, 8]) and not route(widths=[3])       # L 4 / 5 / 0
    assert not route(options=off)
    assert not route(grad=True)
    assert not route(dbl=True)
    assert not route(pool=0) and not route(pool=4) and not route(pool="sum") and not route(act=1) and not route(act="relu")


def test_pcgan_noise_and_generation():
    margs = {"pcgan_latent_dim": 16, "pcgan_z2_dim": 10, "sample_points": False}
    torch.manual_seed(0)
    noise, extra = gen.get_gen_noise(margs, 4000, 30, model="pcgan", device="cpu", noise_std=0.3)
    assert noise.shape == (4000, 16) and extra is None
    n = noise.numel()
    # sampling error of a standard deviation over n draws is std / sqrt(2 n); five of them
    assert abs(float(noise.std()) - 0.3) <= 5 * 0.3 / (2 * n) ** 0.5 and abs(float(noise.mean())) <= 5 * 0.3 / n ** 0.5
    lG, dec = ext_models.latent_G(16, 24, [32, 48]), ext_models.G(3, 24, 10)
    out = gen.gen(margs, lG, 5, 30, model="pcgan")
    assert out.shape == (5, 24) and out.requires_grad                     # sample_points off: the latent rows (training)
    margs = dict(margs, sample_points=True, G_pc=dec)
    noise, pn = gen.get_gen_noise(margs, 4000, 30, model="pcgan", device="cpu", noise_std=0.3)
    assert noise.shape == (4000, 16) and pn.shape == (4000, 30, 10)
    n = pn.numel()
    assert abs(float(pn.std()) - 1.0) <= 5 / (2 * n) ** 0.5 and abs(float(pn.mean())) <= 5 / n ** 0.5
    assert abs(float(noise.std()) - 0.3) <= 5 * 0.3 / (2 * noise.numel()) ** 0.5
    out = gen.gen(margs, lG, 5, 30, model="pcgan")
    assert out.shape == (5, 30, 3)
    # caller-supplied noise: with the caller's point noise the result is a function of both; without, point noise is drawn
    z, pn = gen.get_gen_noise(margs, 5, 30, model="pcgan", device="cpu")
    with torch.no_grad():
        a = gen.gen(margs, lG, 5, 30, model="pcgan", noise=z, point_noise=pn)
        assert torch.equal(a, dec(lG(z).unsqueeze(1), pn))
        b = gen.gen(margs, lG, 5, 30, model="pcgan", noise=z)
    assert b.shape == (5, 30, 3) and not torch.equal(a, b)
    out = gen.gen_multi_batch(margs, lG, 3, 7, 30, out_device="cpu", detach=True, model="pcgan")
    assert out.shape == (7, 30, 3) and not out.requires_grad
    with pytest.raises(NotImplementedError):
        gen.get_gen_noise_shape(margs, 7, 30, model="pcgan")
