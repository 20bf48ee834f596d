"""GPU: label smoothing / label noise of the D step -- ``mpg_label_targets`` against a numpy restatement of the draws written from
include/mpgan_amd.h, the fused head reading per-jet targets against fp64 autograd, and ``TrainStep(label_smoothing=...,
label_noise=...)``: captured against eager, the fused routes against the "module" route, resume, and the default step unchanged."""
import contextlib

import numpy as np
import pytest
import torch

from conftest import assert_grads, rel_err
from test_gpu_head import _ref_head
from test_gpu_schedule import _all_equal, _device_seed, _named, _state, _step, _watch
from test_loader_cpu import _word

pytestmark = pytest.mark.gpu

SEED = 0x9E3779B97F4A7C15      # (both halves of the 64-bit seed in use, the top bit set)


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


@contextlib.contextmanager
def _seed_at(value_tensor):
    """The device seed holds ``value_tensor`` for the block and what it held before afterwards (no host flag is touched)."""
    from mpgan_amd import ops
    s = ops.seed_tensor(_dev())
    keep = s.clone()
    s.copy_(value_tensor)
    try:
        yield
    finally:
        s.copy_(keep)


def _drawn_numpy(seed, B, smoothing, noise, site=0):
    """Y [2B] as the header states it: u_s, u_n from groups 0 and 1 of the hash word of (seed, MPG_LABEL_TAG + site, jet b), every
    operation in fp32."""
    from mpgan_amd import ops
    tag = ops.LABEL_TAG + site
    row = np.arange(2 * B, dtype=np.uint64)
    u = lambda grp: (_word(seed, tag, row, grp) >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    us, un = u(0), u(1)
    real = np.arange(2 * B) < B
    if smoothing:
        y = np.where(real, np.float32(0.7) + np.float32(0.5) * us, np.float32(0.3) * us).astype(np.float32)
    else:
        y = real.astype(np.float32)
    flip = un < np.float32(noise)
    return np.where(flip, np.where(real, np.float32(0), np.float32(1)), y).astype(np.float32)


def _targets_fp64(drawn, B, smoothing):
    y = drawn.astype(np.float64)
    if not smoothing:
        return y, 0.0
    t = np.concatenate([np.full(B, y[:B].mean()), np.full(B, y[B:].mean())])
    return t, float(y[:B].var() + y[B:].var())


@pytest.mark.parametrize("noise", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("smoothing", [False, True])
@pytest.mark.parametrize("B", [1, 5, 64, 257])
def test_draws_against_the_headers_statement(B, smoothing, noise):
    from mpgan_amd import ops
    with _device_seed(SEED) as seed:
        seed()
        assert ops.get_seed(_dev()) == SEED
        targets, extra, drawn = ops.label_targets(B, smoothing, noise, _dev())
        torch.cuda.synchronize()
    d, t, e = drawn.cpu().numpy(), targets.cpu().numpy(), float(extra)
    want = _drawn_numpy(SEED, B, smoothing, noise)
    assert d.dtype == np.float32 and np.array_equal(d.view(np.uint32), want.view(np.uint32))       # bit for bit
    wt, we = _targets_fp64(d, B, smoothing)
    print(B, smoothing, noise, "targets rel", rel_err(t, wt), "extra", e, "want", we)
    assert rel_err(t, wt) <= 1e-5
    assert abs(e - we) <= 1e-5 * max(abs(we), 1e-3)
    if not smoothing:
        assert np.array_equal(t, d) and e == 0.0
        if noise == 0.0:
            assert np.array_equal(t, (np.arange(2 * B) < B).astype(np.float32))
    if noise == 1.0:
        assert not d[:B].any() and (d[B:] == 1).all() and not t[:B].any() and (t[B:] == 1).all()
    elif smoothing and noise == 0.0:
        assert (d[:B] >= 0.7).all() and (d[:B] <= 1.2).all() and (d[B:] >= 0.0).all() and (d[B:] <= 0.3).all()
    if B == 1 and smoothing:      # one label per half: it is its own mean, and nothing varies
        assert e == 0.0 and np.array_equal(t, d)
    # another site, another seed: other draws (where anything is drawn at all)
    if smoothing and noise < 1.0:
        with _device_seed(SEED) as seed:
            seed()
            other = ops.label_targets(B, smoothing, noise, _dev(), site=1)[2].cpu().numpy()
        assert not np.array_equal(other, d) and np.array_equal(other, _drawn_numpy(SEED, B, smoothing, noise, site=1))


def test_flipped_share_at_2048():
    """noise = 0.3 over 2048 labels per half: the flipped share within 0.3 +- 0.05 (five standard deviations of the binomial,
    sqrt(0.3 * 0.7 / 2048) = 0.0101); the seed is fixed, so the outcome is too."""
    from mpgan_amd import ops
    B = 2048
    with _device_seed(SEED) as seed:
        seed()
        targets, extra, drawn = ops.label_targets(B, False, 0.3, _dev())
        d = drawn.cpu().numpy()
    share_r, share_f = float((d[:B] == 0).mean()), float((d[B:] == 1).mean())
    print("flipped share: real", share_r, "generated", share_f)
    assert abs(share_r - 0.3) <= 0.05 and abs(share_f - 0.3) <= 0.05
    assert np.array_equal(d, _drawn_numpy(SEED, B, False, 0.3))


# ---- the head reading targets ---------------------------------------------------------------------------------------------------
def _loss_fp64(loss, out, t, extra, count):
    if loss == "ls":
        terms = (out - t) ** 2
    else:      # nn.BCELoss's formula (logarithms clamped at -100) with a target that need not be 0 / 1
        terms = -(t * torch.clamp(torch.log(out), min=-100.0) + (1 - t) * torch.clamp(torch.log(1 - out), min=-100.0))
    return terms.sum() / count + extra


@pytest.mark.parametrize("loss,sigmoid", [("ls", False), ("og", True)])
@pytest.mark.parametrize("mean", [False, True])
def test_disc_head_loss_with_targets(mean, loss, sigmoid):
    """10 jets (5 + 5) of 3 particles, 33 features (the feature loop passes 32), arbitrary targets in [0, 1.2] with an exact 0 and
    an exact 1 among them, loss_extra = 0.0173: value, out, dy, dw, db against fp64 autograd, 1e-5 relative."""
    from mpgan_amd import ops
    g = torch.Generator(device="cuda").manual_seed(29)
    B, N, F = 5, 3, 33
    nj = 2 * B
    y = torch.randn(nj, N, F, device="cuda", generator=g).mul_(0.3)
    mask = (torch.rand(nj, N, 1, device="cuda", generator=g) < 0.7).float()
    mask[:, 0] = 1.0                                  # (no empty jet: mean pooling divides by the mask's sum)
    w = torch.randn(1, F, device="cuda", generator=g).mul_(0.2)
    b = torch.randn(1, device="cuda", generator=g)
    targets = torch.rand(nj, device="cuda", generator=g) * 1.2
    targets[2], targets[7] = 0.0, 1.0
    extra = torch.full((1,), 0.0173, device="cuda")
    kw = dict(mean=mean, sigmoid=sigmoid, p_drop=0.0, training=True, loss=loss, n_real=B, gen_step=False, count=B)
    loss_out = torch.zeros((), device="cuda")
    dw, db = torch.zeros(1, F, device="cuda"), torch.zeros(1, device="cuda")
    out, dy = ops.disc_head_loss(y, mask, w, b, loss_out=loss_out, wgrad=(dw, db), targets=targets, loss_extra=extra, **kw)
    yr, wr, br = (t.double().requires_grad_(True) for t in (y, w, b))
    o = _ref_head(yr, mask.double(), wr, br, mean, sigmoid).reshape(-1)
    L = _loss_fp64(loss, o, targets.double(), 0.0173, B)
    L.backward()
    errs = {"out": rel_err(out.cpu().numpy(), o.detach().cpu().numpy()), "dy": rel_err(dy.cpu().numpy(), yr.grad.cpu().numpy()),
            "dw": rel_err(dw.cpu().numpy(), wr.grad.cpu().numpy()), "db": rel_err(db.cpu().numpy(), br.grad.cpu().numpy())}
    print(loss, mean, "loss", float(loss_out), float(L.detach()), errs)
    assert abs(float(loss_out) - float(L.detach())) < 1e-5 * max(abs(float(L.detach())), 1e-3)
    assert all(e < 1e-5 for e in errs.values()), errs
    # without the two pointers: the call as it was, bit for bit -- and not the call with them
    res = []
    for extra_kw in ({}, dict(targets=None, loss_extra=None)):
        lo = torch.zeros((), device="cuda")
        dw2, db2 = torch.zeros(1, F, device="cuda"), torch.zeros(1, device="cuda")
        o2, dy2 = ops.disc_head_loss(y, mask, w, b, loss_out=lo, wgrad=(dw2, db2), **kw, **extra_kw)
        res.append((o2, dy2, dw2, db2, lo))
    assert _all_equal(res[0], res[1])
    assert torch.equal(res[0][0], out) and not torch.equal(res[0][1], dy) and not torch.equal(res[0][4], loss_out)
    # ... which scores against 1 / 0: the same as handing those in as targets, with nothing to add
    hard = torch.cat([torch.ones(B, device="cuda"), torch.zeros(B, device="cuda")])
    lo = torch.zeros((), device="cuda")
    dw3, db3 = torch.zeros(1, F, device="cuda"), torch.zeros(1, device="cuda")
    o3, dy3 = ops.disc_head_loss(y, mask, w, b, loss_out=lo, wgrad=(dw3, db3), targets=hard, **kw)
    assert _all_equal(res[0], (o3, dy3, dw3, db3, lo))


# ---- the step -------------------------------------------------------------------------------------------------------------------
LABELS = dict(label_smoothing=True, label_noise=0.3)


def _labels_of(ts):
    return [ts.label_drawn.clone(), ts.label_targets.clone(), ts.label_extra.clone()]


@pytest.mark.parametrize("model,B", [("mpgan", 6), ("gapt", 4)])
def test_captured_equals_eager_and_every_replay_draws_fresh_labels(model, B):
    """Three steps from one device seed, ``ls`` with smoothing and noise 0.3, fixed generator noise: the captured run equals the
    eager one bit for bit after every step (training state and the label buffers); the labels differ from replay to replay and
    are ``ops.label_targets`` under the seed the iteration started from."""
    from mpgan_amd import ops
    res = []
    with _device_seed() as seed:
        for use_graphs in (False, True):
            seed()
            ts = _step(model, B, use_graphs=use_graphs, **LABELS)
            assert ts.labels_on and ts._route() != "module"
            seen = []
            for _ in range(3):
                before = ops.seed_tensor(ts.dev).clone()
                ts.step()
                torch.cuda.synchronize()
                with _seed_at(before):
                    want = ops.label_targets(B, True, 0.3, ts.dev)
                    torch.cuda.synchronize()
                assert torch.equal(ts.label_drawn, want[2]) and torch.equal(ts.label_targets, want[0])
                assert torch.equal(ts.label_extra, want[1])
                seen.append(_state(ts) + _labels_of(ts))
            if use_graphs:
                assert len(ts._graphs) == 1
            res.append(seen)
    for k, (a, c) in enumerate(zip(*res)):
        assert _all_equal(a, c), (k, [i for i, (x, y) in enumerate(zip(a, c)) if not torch.equal(x, y)])
    for seen in res:
        drawn = [s[-3] for s in seen]
        assert not torch.equal(drawn[0], drawn[1]) and not torch.equal(drawn[1], drawn[2])
        assert float(drawn[0][:B].max()) <= 1.2 and float(drawn[0][B:].min()) >= 0.0
    assert all(np.isfinite(float(s[0])) for s in res[0]) and float(res[0][0][-1]) > 0      # (D_loss; extra = the two variances)


@pytest.mark.parametrize("model,B", [("mpgan", 6), ("gapt", 4)])
def test_fused_route_equals_the_module_route(model, B):
    """One D step from one device seed on the fused route and on the "module" route (``batch_real_fake=False``: D's two passes,
    ``d_loss`` on the label buffers): the same labels, D_loss to 1e-4 and D's parameter gradients to 1e-3 of each tensor's largest
    entry -- the bars tests/test_gpu_train.py holds a step to against another evaluation of the same iteration
    (``test_train_step_other_losses_vs_oracle``)."""
    got = {}
    with _device_seed() as seed:
        for route, kw in (("fused", {}), ("module", dict(batch_real_fake=False))):
            seed()
            ts = _step(model, B, use_graphs=False, **LABELS, **kw)
            assert (ts._route() == "module") == (route == "module")
            log = {}
            _watch(ts.fD, log, "D")
            ts.step()
            torch.cuda.synchronize()
            got[route] = (float(ts.D_loss), _named(ts.fD, log["D"]), _labels_of(ts))
    assert _all_equal(got["fused"][2], got["module"][2])
    a, m = got["fused"][0], got["module"][0]
    print(model, "D_loss fused", a, "module", m)
    assert abs(a - m) <= 1e-4 * max(abs(m), 1e-3)
    assert_grads({k: v.numpy() for k, v in got["fused"][1].items()}, {k: v.numpy() for k, v in got["module"][1].items()}, 1e-3,
                 what=f"labels: fused vs module route, {model}")


def test_resume_equals_the_uninterrupted_run(tmp_path):
    """Saved after two steps, loaded into fresh objects, two more: the state and the labels of four uninterrupted steps, bit for
    bit -- the labels hang on the device seed, which travels with G's optimizer state."""
    from mpgan_amd import checkpoint as ck
    tmp = str(tmp_path / "models")
    B = 6
    with _device_seed() as seed:
        seed()
        ts = _step("mpgan", B, **LABELS)
        mid = None
        for b in range(4):
            ts.step()
            if b == 1:
                torch.cuda.synchronize()
                ck.save_models(ts.D, ts.G, ts.fD, ts.fG, tmp, 2)
                mid = ts.label_drawn.clone()
        whole = _state(ts, device_counters=False) + _labels_of(ts)
        seed()
        again = _step("mpgan", B, seeds=(77, 78), **LABELS)      # other weights: everything comes from the files
        ck.load_models(again.D, again.G, tmp, 2)
        ck.load_optimizers(again.fD, again.fG, tmp, 2)
        for b in range(2, 4):
            again.step()
        got = _state(again, device_counters=False) + _labels_of(again)
    assert _all_equal(whole, got), [i for i, (x, y) in enumerate(zip(whole, got)) if not torch.equal(x, y)]
    assert not torch.equal(mid, whole[-3])


def test_options_off_are_the_default_step():
    res = []
    with _device_seed() as seed:
        for kw in ({}, dict(label_smoothing=False, label_noise=0.0)):
            seed()
            ts = _step("mpgan", 6, fixed=False, **kw)
            for _ in range(2):
                ts.step()
            assert not ts.labels_on and not hasattr(ts, "label_targets") and len(ts._graphs) == 1
            res.append(_state(ts))
    assert _all_equal(res[0], res[1])
