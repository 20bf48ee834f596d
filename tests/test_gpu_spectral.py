"""GPU: spectral norm on the grouped kernels (``mpg_spectral_norm`` / ``mpg_spectral_norm_bwd``) and spectral-norm MPLayers on
the fused edge kernels -- the kernels against the fp64 statement, two forwards before one backward, a layer against the fp64
oracle, whole networks and captured TrainSteps against the un-fused route (``ops.OPTIONS["sn_fused"] = False``)."""
import copy

import numpy as np
import pytest
import torch

from conftest import assert_grads, rel_err
from spectral_ref import (ITERATIONS, SHAPES, TIGHT, backward_ref, check_forward, forward_ref, make_layer, scaled_err, terms_scale)

pytestmark = pytest.mark.gpu
TOL = 1e-3       # BASELINE.json north_star: "within 1e-3 rel fp32"
SN_KEYS = ("fe.net.0", "fe.net.1", "fe.net.2", "fn.net.0", "fn.net.1")   # the wrapped layers of an MPLayer (fn.net.2 is not)


def _dev():
    return torch.device("cuda:0")


class sn_fused:
    """``ops.OPTIONS["sn_fused"]`` set for a block, restored behind it."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from mpgan_amd import ops
        self.old, ops.OPTIONS["sn_fused"] = ops.OPTIONS["sn_fused"], self.on

    def __exit__(self, *exc):
        from mpgan_amd import ops
        ops.OPTIONS["sn_fused"] = self.old


# ------------------------------------------------------------------------------------------------------------------ 1. kernels
def _group_on_device(shapes, P, seed, odd_offset=False):
    layers, host = [], []
    for k, (R, C) in enumerate(shapes):
        W, u, v = make_layer(R, C, P, seed + k)
        host.append((W, u, v))
        if odd_offset:   # a view at an odd float offset into a larger buffer: the start is 4-byte aligned only
            buf = torch.zeros(R * C + 8, device=_dev())
            Wd = buf[3:3 + R * C].view(R, C)
            Wd.copy_(W)
            assert Wd.is_contiguous() and Wd.data_ptr() % 8 == 4
        else:
            Wd = W.to(_dev())
        layers.append((Wd, u.to(_dev()), v.to(_dev())))
    return layers, host


def _check_group(shapes, P, seed, odd_offset=False):
    from mpgan_amd import ops
    layers, host = _group_on_device(shapes, P, seed, odd_offset)
    outs = ops.spectral_norm_launch(layers, P)
    again, _ = _group_on_device(shapes, P, seed, odd_offset)
    outs_again = ops.spectral_norm_launch(again, P)
    torch.cuda.synchronize()
    for (W, u, v), (W0, u0, v0), out, (_, ua, va), outa in zip(layers, host, outs, again, outs_again):
        assert torch.equal(W.cpu(), W0)
        check_forward((*out, u, v), W0, u0, v0, P, what=(tuple(W0.shape), P))
        # two runs from the same inputs: the same bits
        assert all(torch.equal(a, b) for a, b in zip((*out, u, v), (*outa, ua, va))), (tuple(W0.shape), P)
    # a second call on the updated vectors: the state in place really advances
    mid = [(u.cpu().clone(), v.cpu().clone()) for _, u, v in layers]
    outs2 = ops.spectral_norm_launch(layers, P)
    torch.cuda.synchronize()
    for (W, u, v), (W0, _, _), (u1, v1), out, out1 in zip(layers, host, mid, outs2, outs):
        check_forward((*out, u, v), W0, u1, v1, P, what=("second call", tuple(W0.shape), P))
        if P and min(W0.shape) > 1:
            assert not torch.equal(u.cpu(), u1)
            assert torch.equal(out1[1].cpu(), u1)   # what the first call kept for its backward is untouched
    # the backward on the first call's outputs
    g = torch.Generator().manual_seed(seed)
    for cancelling in (False, True):
        for accumulate in (False, True):
            jobs, refs = [], []
            for (W0, _, _), (W_eff, u_out, v_out, inv) in zip(host, outs):
                G = W_eff.clone() if cancelling else torch.randn(W0.shape, generator=g).to(_dev())
                dW0 = torch.randn(W0.shape, generator=g).to(_dev())
                dW = dW0.clone()
                jobs.append((G, W_eff, u_out, v_out, inv, dW, accumulate))
                args = tuple(t.cpu() for t in (G, W_eff, u_out, v_out, inv)) + ((dW0.cpu() if accumulate else None),)
                refs.append((backward_ref(*args), terms_scale(*args)))
            ops.spectral_norm_bwd_launch(jobs)
            torch.cuda.synchronize()
            for (W0, _, _), job, (ref, scale) in zip(host, jobs, refs):
                got = job[5].cpu()
                err = scaled_err(got, ref, scale) if (cancelling or min(W0.shape) == 1) else rel_err(got, ref)
                assert err < TIGHT, (tuple(W0.shape), P, "cancelling" if cancelling else "random", accumulate, err)


@pytest.mark.parametrize("P", ITERATIONS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_kernel_one_layer_vs_fp64(shape, P):
    _check_group([shape], P, seed=1)


@pytest.mark.parametrize("P", ITERATIONS)
def test_kernel_all_shapes_in_one_group_vs_fp64(P):
    _check_group(SHAPES, P, seed=3)


def test_kernel_weight_at_an_odd_float_offset():
    _check_group([(96, 6), (256, 224), (8, 5)], 1, seed=4, odd_offset=True)


def test_kernel_group_beyond_the_job_limit():
    from mpgan_amd import ops
    _check_group([(5 + k, 3 + (k % 4)) for k in range(2 * ops.SPECTRAL_MAX + 3)], 1, seed=5)


# ------------------------------------------------------------------------------------------- 2. two forwards, one backward
def test_backward_through_the_first_of_two_forwards_uses_its_own_vectors():
    from mpgan_amd import ops
    W0, u0, v0 = make_layer(96, 6, 1, 11)
    W = W0.to(_dev()).requires_grad_(True)
    u, v = u0.to(_dev()), v0.to(_dev())
    w1 = ops.spectral_weights([(W, u, v)], 1)[0]
    u1, v1 = u.cpu().clone(), v.cpu().clone()
    w2 = ops.spectral_weights([(W, u, v)], 1)[0]
    assert w1.grad_fn is not None and not torch.equal(u.cpu(), u1)
    G = torch.randn(96, 6, generator=torch.Generator().manual_seed(2))
    (w1 * G.to(_dev())).sum().backward()
    torch.cuda.synchronize()
    first, second = forward_ref(W0, u0, v0, 1), forward_ref(W0, u1, v1, 1)
    assert rel_err(w1.detach().cpu(), first["W_eff"]) < TIGHT and rel_err(w2.detach().cpu(), second["W_eff"]) < TIGHT
    then = backward_ref(G, first["W_eff"], first["u"], first["v"], first["inv_sigma"])
    assert rel_err(W.grad.cpu(), then) < TIGHT
    # (the live vectors would give another gradient: the check tells the two apart)
    now = backward_ref(G, second["W_eff"], second["u"], second["v"], second["inv_sigma"])
    assert rel_err(now, then) > 10 * TIGHT
    assert u.grad is None and v.grad is None


# ------------------------------------------------------------------------------------------------------------------ 3. MPLayer
def _sn_layer(F, out, sum_agg, seed):
    """(the layer on the GPU, fp64 leaves {key: tensor} of its trained parameters, {layer: (u, v)} float32)."""
    from oracle import train_ref as T
    from test_oracle_golden import mplayer_shapes
    from mpgan_amd.mpgan import MPLayer
    sd64 = T.init_state_dict(mplayer_shapes(F, out), seed=seed, dtype=torch.float64)
    g = torch.Generator().manual_seed(100 + seed)
    state, leaves, uv = {}, {}, {}
    for k, t in sd64.items():
        base, kind = k.rsplit(".", 1)
        t = t.float()
        if base in SN_KEYS:
            key = base + (".module.weight_bar" if kind == "weight" else ".module.bias")
            if kind == "weight":
                uv[base] = tuple(torch.nn.functional.normalize(torch.randn(n, generator=g), dim=0, eps=1e-12) for n in t.shape)
                state[base + ".module.weight_u"], state[base + ".module.weight_v"] = uv[base]
        else:
            key = k
        state[key] = t
        leaves[key] = t.double().requires_grad_(True)
    layer = MPLayer(F, [96, 160, 192], [256, 256], out, sum=sum_agg, spectral_norm=True, dropout_p=0.0)
    layer.load_state_dict(state)
    return layer.to(_dev()).train(), leaves, uv


def _run_layer(layer, x, mask, up):
    x = x.clone().requires_grad_(True)
    y = layer(x, True, mask)
    (y * up).sum().backward()
    torch.cuda.synchronize()
    grads = {"dx": x.grad.cpu().numpy()}
    grads.update({k: p.grad.cpu().numpy() for k, p in layer.named_parameters() if p.requires_grad})
    state = {k: p.detach().cpu().clone() for k, p in layer.named_parameters() if not p.requires_grad}
    assert all(p.grad is None for p in layer.parameters() if not p.requires_grad)
    return y.detach().cpu(), grads, state


@pytest.mark.parametrize("B,N,F,out,sum_agg", [(3, 30, 32, 32, True), (2, 33, 3, 32, False)], ids=["3x30x32-sum", "2x33x3-mean"])
def test_mplayer_spectral_norm_vs_fp64_oracle(B, N, F, out, sum_agg):
    import oracle
    layer, leaves, uv = _sn_layer(F, out, sum_agg, seed=B)
    assert layer.fused and layer.spectral_norm
    control_layer = copy.deepcopy(layer)
    rs = np.random.RandomState(50 + B)
    x64 = torch.from_numpy(rs.normal(0, 0.5, size=(B, N, F)))
    up64 = torch.from_numpy(rs.normal(size=(B, N, out)))
    m = (rs.uniform(size=(B, N, 1)) < 0.8).astype(np.float64)
    m[:, 0] = 1
    m[B - 1, :, 0] = 0
    m[B - 1, [4, N - 1], 0] = 1            # one jet with 2 live particles
    mask64 = torch.from_numpy(m)
    # fp64: W_eff from (weight_bar, u, v) with the vectors constant, autograd through weight_bar
    sdo, vec64 = {}, {}
    for key, leaf in leaves.items():
        if key.endswith(".module.weight_bar"):
            base = key[:-len(".module.weight_bar")]
            with torch.no_grad():
                from spectral_ref import power_iteration
                un, vn, _ = power_iteration(leaf, uv[base][0].double(), uv[base][1].double(), 1)
            vec64[base] = (un, vn)
            sdo["L." + base + ".weight"] = leaf / (un.dot(torch.mv(leaf, vn)) + 1e-12)
        else:
            sdo["L." + key.replace(".module.bias", ".bias")] = leaf
    xo = x64.clone().requires_grad_(True)
    yo = oracle.mplayer_forward(sdo, "L", xo, mask64, sum_agg=sum_agg)
    (yo * up64).sum().backward()
    ref = {"dx": xo.grad.numpy()}
    ref.update({k: leaf.grad.numpy() for k, leaf in leaves.items()})

    x, mask, up = x64.float().to(_dev()), mask64.float().to(_dev()), up64.float().to(_dev())
    with sn_fused(True):
        y, got, state = _run_layer(layer, x, mask, up)
    with sn_fused(False):
        yc, control, state_c = _run_layer(control_layer, x, mask, up)
    assert set(got) == set(ref) == set(control)
    assert rel_err(y.numpy(), yo.detach().numpy()) < TIGHT
    assert rel_err(yc.numpy(), yo.detach().numpy()) < TIGHT
    assert_grads(got, ref, TOL, control=control, what=("sn mplayer", B, N, F, out))
    for base, (un, vn) in vec64.items():
        ku, kv = base + ".module.weight_u", base + ".module.weight_v"
        assert rel_err(state[ku], un) < TIGHT and rel_err(state[kv], vn) < TIGHT, base
        assert torch.equal(state[ku], state_c[ku]) and torch.equal(state[kv], state_c[kv]), base   # the same kernel either way
        assert not torch.equal(state[ku], uv[base][0])


# ----------------------------------------------------------------------------------------------------------------- 4. networks
def _net_run(net, call):
    net.zero_grad()
    y = call(net)
    torch.cuda.synchronize()
    grads = {k: p.grad.cpu().numpy() for k, p in net.named_parameters() if p.requires_grad}
    frozen = [k for k, p in net.named_parameters() if not p.requires_grad]
    assert frozen and all(k.endswith(("weight_u", "weight_v")) for k in frozen)
    assert all(p.grad is None for k, p in net.named_parameters() if not p.requires_grad)
    return y, grads, {k: v.detach().cpu().clone() for k, v in net.state_dict().items() if k.endswith(("weight_u", "weight_v"))}


def test_spectral_norm_networks_fused_vs_unfused_route():
    from mpgan_amd import train
    from oracle.train_ref import synthetic_batch
    B, N = 4, 30
    torch.manual_seed(21)
    G, D = train.default_mpgan(N, disc_dropout=0.0, spectral_norm_gen=True, spectral_norm_disc=True)
    assert all(l.fused and l.spectral_norm for l in (*G.mp_layers, *D.mp_layers))
    data, labels = synthetic_batch(B, N, seed=7)
    data, labels = data.to(_dev()), labels.to(_dev())
    gen = torch.Generator().manual_seed(8)
    noise = (torch.randn(B, N, 32, generator=gen) * 0.2).to(_dev())
    up = torch.randn(B, N, 4, generator=gen).to(_dev())

    def run_D(net):
        y = net(data.clone(), labels)
        y.sum().backward()
        return y.detach().cpu()

    def run_G(net):
        y = net(noise.clone(), labels)
        (y * up).sum().backward()
        return y.detach().cpu()

    for name, net, call in (("D", D, run_D), ("G", G, run_G)):
        other = copy.deepcopy(net)
        with sn_fused(True):
            y, got, vecs = _net_run(net, call)
        with sn_fused(False):
            yr, ref, vecs_r = _net_run(other, call)
        assert rel_err(y.numpy(), yr.numpy()) < TIGHT, name
        assert set(got) == set(ref)
        assert_grads(got, ref, TOL, what=("sn network", name))
        assert vecs.keys() == vecs_r.keys() and all(torch.equal(vecs[k], vecs_r[k]) for k in vecs), name


# ---------------------------------------------------------------------------------------------------------------- 5. TrainStep
def _train_steps(use_graphs, steps):
    from mpgan_amd import train
    from oracle.train_ref import synthetic_batch
    B, N = 8, 30
    torch.manual_seed(11)
    G, D = train.default_mpgan(N, disc_dropout=0.0, spectral_norm_gen=True, spectral_norm_disc=True)
    data, labels = synthetic_batch(B, N, seed=5)
    ts = train.TrainStep(G, D, B, N, use_graphs=use_graphs, lr_disc=1e-3, lr_gen=1e-3)
    ts.set_batch(data.cuda(), labels.cuda())
    gen = torch.Generator(device="cuda").manual_seed(6)
    ts.fixed_noise = (torch.randn(B, N, 32, device="cuda", generator=gen) * 0.2,
                      torch.randn(B, N, 32, device="cuda", generator=gen) * 0.2)
    for _ in range(steps):
        ts.step()
    torch.cuda.synchronize()
    state = {"flatD": ts.fD.flat.clone(), "flatG": ts.fG.flat.clone()}
    for name, net in (("G", G), ("D", D)):
        state.update({f"{name}.{k}": v.clone() for k, v in net.state_dict().items() if k.endswith(("weight_u", "weight_v"))})
    return state, ts


def test_captured_spectral_norm_steps_equal_eager_ones():
    from mpgan_amd import ops
    ops.range_status(_dev(), clear=True)
    with sn_fused(True):
        eager, ts_e = _train_steps(False, 3)
        graphs, ts_g = _train_steps(True, 3)
    assert all(l.fused for l in (*ts_g.G.mp_layers, *ts_g.D.mp_layers)) and not ts_g.gen_ahead and not ts_e.gen_ahead
    assert sum(k.endswith("weight_u") for k in eager) == 20
    for k in eager:
        assert torch.equal(eager[k], graphs[k]), k
    assert bool(torch.isfinite(ts_g.fD.flat).all()) and bool(torch.isfinite(ts_g.fG.flat).all())
    assert ops.range_status(_dev()) == 0
