"""CPU: the spectral-norm kernels' per-layer routines compiled for the host (``mpg_spectral_norm_host`` /
``mpg_spectral_norm_bwd_host``: one body with the device kernels, csrc/spectral.hip) against the fp64 torch statement of
include/mpgan_amd.h, the backward formula against autograd, the refusals, and what spectral norm changes at construction."""
import ctypes as C
import os
import re

import pytest
import torch

from spectral_ref import (ITERATIONS, SHAPES, TIGHT, backward_ref, check_forward, forward_ref, make_layer, rel_err, scaled_err,
                          terms_scale)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mpgan_amd.h")


def run_group(shapes, P, seed=1):
    """One grouped host call over ``shapes``; per layer (inputs before the call, what the call left) checked against fp64, then
    the backward on the call's own outputs: G random and G = W_eff, accumulate off and on."""
    from mpgan_amd import ops
    layers = [make_layer(R, C, P, seed + k) for k, (R, C) in enumerate(shapes)]
    before = [(W.clone(), u.clone(), v.clone()) for W, u, v in layers]
    outs = ops.spectral_norm_launch(layers, P, host=True)
    assert len(outs) == len(shapes)
    for (R, C), (W, u, v), (W0, u0, v0), out in zip(shapes, layers, before, outs):
        assert torch.equal(W, W0)
        check_forward((*out, u, v), W0, u0, v0, P, what=(R, C, P))
    g = torch.Generator().manual_seed(seed)
    for cancelling in (False, True):
        for accumulate in (False, True):
            jobs, refs = [], []
            for (R, C), (W_eff, u_out, v_out, inv) in zip(shapes, outs):
                G = W_eff.clone() if cancelling else torch.randn(R, C, generator=g)
                dW0 = torch.randn(R, C, generator=g)
                dW = dW0.clone()
                jobs.append((G, W_eff, u_out, v_out, inv, dW, accumulate))
                refs.append((backward_ref(G, W_eff, u_out, v_out, inv, dW0 if accumulate else None),
                             terms_scale(G, W_eff, u_out, v_out, inv, dW0 if accumulate else None)))
            ops.spectral_norm_bwd_launch(jobs, host=True)
            for (R, C), job, (ref, scale) in zip(shapes, jobs, refs):
                # (a rank-one W -- R or C of 1 -- has W_eff = u v^T: dW vanishes identically, for every G)
                err = scaled_err(job[5], ref, scale) if (cancelling or min(R, C) == 1) else rel_err(job[5], ref)
                assert err < TIGHT, ((R, C, P), "cancelling" if cancelling else "random", accumulate, err)


@pytest.mark.parametrize("P", ITERATIONS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_host_twin_one_layer_vs_fp64(shape, P):
    run_group([shape], P)


@pytest.mark.parametrize("P", ITERATIONS)
def test_host_twin_all_shapes_in_one_group_vs_fp64(P):
    run_group(SHAPES, P, seed=3)


def test_launch_helper_splits_a_group_beyond_the_job_limit():
    from mpgan_amd import ops
    txt = open(HEADER).read()
    assert int(re.search(r"^#define\s+MPG_SPECTRAL_MAX_JOBS\s+(\d+)\s*$", txt, flags=re.M).group(1)) == ops.SPECTRAL_MAX
    run_group([(5 + k, 3 + (k % 4)) for k in range(2 * ops.SPECTRAL_MAX + 3)], 1, seed=5)


def test_second_call_moves_the_state_on_and_leaves_the_first_calls_copies():
    """Two forwards before one backward: the second call iterates from where the first left u and v, and what the first call
    returned for its backward is untouched."""
    from mpgan_amd import ops
    W, u, v = make_layer(96, 6, 1, 9)
    u0, v0 = u.clone(), v.clone()
    first = ops.spectral_norm_launch([(W, u, v)], 1, host=True)[0]
    kept = [t.clone() for t in first]
    u1, v1 = u.clone(), v.clone()
    second = ops.spectral_norm_launch([(W, u, v)], 1, host=True)[0]
    check_forward((*second, u, v), W, u1, v1, 1)
    assert not torch.equal(u, u1) and not torch.equal(u1, u0)
    assert all(torch.equal(a, b) for a, b in zip(first, kept))
    two = forward_ref(W, u0, v0, 2)
    assert rel_err(u, two["u"]) < TIGHT and rel_err(second[0], two["W_eff"]) < TIGHT


@pytest.mark.parametrize("P", [0, 1, 2])
def test_backward_formula_is_autograd_of_the_fp64_statement(P):
    g = torch.Generator().manual_seed(4)
    for R, C in ((1, 1), (8, 5), (6, 8), (40, 33)):
        W, u, v = (t.double() for t in make_layer(R, C, 1, 2))
        W.requires_grad_(True)
        with torch.no_grad():
            from spectral_ref import power_iteration
            un, vn, _ = power_iteration(W, u, v, P)
        inv = 1.0 / (un.dot(torch.mv(W, vn)) + 1e-12)
        W_eff = W * inv
        G = torch.randn(R, C, generator=g, dtype=torch.float64)
        (dW,) = torch.autograd.grad((G * W_eff).sum(), W)
        args = (G, W_eff.detach(), un, vn, inv.detach().reshape(1))
        # (over the terms' magnitude: the 1 x 1 layer's gradient vanishes identically)
        assert scaled_err(backward_ref(*args), dW, terms_scale(*args)) < 1e-12, (R, C, P)


def _job(W, u, v, outs):
    from mpgan_amd import _lib
    j = _lib.MpgSpectralJob()
    j.W, j.u, j.v, j.R, j.C = W.data_ptr(), u.data_ptr(), v.data_ptr(), W.shape[0], W.shape[1]
    j.W_eff, j.u_out, j.v_out, j.inv_sigma = (t.data_ptr() for t in outs)
    return j


def test_refusals():
    from mpgan_amd import _lib, ops
    lib = _lib.lib()
    W, u, v = make_layer(8, 5, 1, 1)
    W2, u2, v2 = make_layer(8, 5, 1, 2)
    fresh = lambda: (torch.empty(8, 5), torch.empty(8), torch.empty(5), torch.empty(1))   # noqa: E731
    keep = [fresh(), fresh()]
    before = (u.clone(), v.clone(), u2.clone(), v2.clone())
    for a, b in (((W, u, v), (W2, u, v2)), ((W, u, v), (W2, u2, v))):      # one u, one v in two jobs of a launch
        jobs = (_lib.MpgSpectralJob * 2)(_job(*a, keep[0]), _job(*b, keep[1]))
        assert lib.mpg_spectral_norm_host(jobs, 2, 1) == -2
        assert lib.mpg_spectral_norm(jobs, 2, 1, None) == -2               # (refused before anything is launched)
    with pytest.raises(ValueError):
        ops.spectral_norm_launch([(W, u, v), (W2, u, v2)], 1, host=True)
    one = (_lib.MpgSpectralJob * 1)(_job(W, u, v, keep[0]))
    assert lib.mpg_spectral_norm_host(one, 0, 1) == -1 and lib.mpg_spectral_norm_host(one, _lib_max() + 1, 1) == -1
    assert lib.mpg_spectral_norm_host(one, 1, -1) == -1 and lib.mpg_spectral_norm_host(None, 1, 1) == -1
    one[0].R = 0
    assert lib.mpg_spectral_norm_host(one, 1, 1) == -1
    one[0].R, one[0].u_out = 8, u.data_ptr()
    assert lib.mpg_spectral_norm_host(one, 1, 1) == -3
    bj = (_lib.MpgSpectralBwdJob * 1)()
    assert lib.mpg_spectral_norm_bwd_host(bj, 1) == -1 and lib.mpg_spectral_norm_bwd(bj, 1, None) == -1
    assert all(torch.equal(a, b) for a, b in zip(before, (u, v, u2, v2)))   # a refused call writes nothing


def _lib_max():
    from mpgan_amd import ops
    return ops.SPECTRAL_MAX


def test_zero_iterations_write_neither_vector():
    from mpgan_amd import ops
    W, u, v = make_layer(16, 300, 0, 1)
    u0, v0 = u.clone(), v.clone()
    W_eff, u_out, v_out, inv = ops.spectral_norm_launch([(W, u, v)], 0, host=True)[0]
    assert torch.equal(u, u0) and torch.equal(v, v0) and torch.equal(u_out, u0) and torch.equal(v_out, v0)
    assert rel_err(W_eff, forward_ref(W, u0, v0, 0)["W_eff"]) < TIGHT


def test_header_and_signature_table_agree():
    from mpgan_amd import _lib
    txt = open(HEADER).read()
    for name in ("mpg_spectral_norm", "mpg_spectral_norm_bwd", "mpg_spectral_norm_host", "mpg_spectral_norm_bwd_host"):
        decl = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", txt, flags=re.M | re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(_lib.lib(), name)
    import subprocess
    import tempfile
    structs = ["MpgSpectralJob", "MpgSpectralBwdJob"]
    src = '#include <stdio.h>\n#include "mpgan_amd.h"\nint main(){' + "".join(
        f'printf("{s} %zu\\n", sizeof({s}));' for s in structs) + "return 0;}"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.run(["gcc", "-I", os.path.dirname(HEADER), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")], check=True)
        out = subprocess.run([os.path.join(d, "t")], check=True, capture_output=True, text=True).stdout
    sizes = dict(line.split() for line in out.strip().splitlines())
    for s in structs:
        assert int(sizes[s]) == C.sizeof(getattr(_lib, s)), s


def test_spectral_norm_layers_are_built_for_the_fused_kernels():
    from mpgan_amd import ops, train
    from mpgan_amd.mpgan import MPLayer
    from mpgan_amd.mpgan.model import SpectralNorm
    assert "sn_fused" in ops.OPTIONS and ops.OPTIONS["sn_fused"] is True
    layer = MPLayer(32, [96, 160, 192], [256, 256], 32, spectral_norm=True)
    assert layer.fused is True and layer.spectral_norm
    assert MPLayer(32, [96, 160, 192], [256, 256], 32, batch_norm=True, spectral_norm=True).fused is False
    assert MPLayer(32, [96, 160, 192], [256, 256], 32, batch_norm=True).fused is False
    assert not MPLayer(32, [96, 160, 192], [256, 256], 32).spectral_norm
    # which layers are wrapped, their keys and the frozen vectors: as before
    wrapped = [isinstance(l, SpectralNorm) for l in (*layer.fe.net, *layer.fn.net)]
    assert wrapped == [True] * 5 + [False]
    keys = set(layer.state_dict())
    assert {"fe.net.0.module.weight_bar", "fe.net.0.module.weight_u", "fe.net.0.module.weight_v", "fe.net.0.module.bias",
            "fn.net.2.weight", "fn.net.2.bias"} <= keys and "fe.net.0.weight" not in keys
    assert all(p.requires_grad != k.endswith(("weight_u", "weight_v")) for k, p in layer.named_parameters())
    assert layer.packed_sets() == []
    # a spectral-norm generator still writes state in its forward (no generator-ahead stream), its discriminator has no fused head
    G, D = train.default_mpgan(30, device="cpu", spectral_norm_gen=True, spectral_norm_disc=True)
    assert all(l.fused for l in (*G.mp_layers, *D.mp_layers))
    assert not train._forward_writes_no_state(G) and D.fused_head() is None
    # the host formula of SpectralNorm.weight() is what CPU tensors keep
    sn = layer.fe.net[0]
    u0 = sn.module.weight_u.detach().clone()
    ref = forward_ref(sn.module.weight_bar.detach(), u0, sn.module.weight_v.detach().clone(), 1)
    w = sn.weight()
    assert w.grad_fn is not None and rel_err(w.detach(), ref["W_eff"]) < TIGHT and not torch.equal(sn.module.weight_u, u0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        layer(torch.randn(2, 30, 32))
