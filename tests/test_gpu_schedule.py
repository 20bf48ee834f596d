"""GPU: the num_critic / num_gen schedule of ``TrainStep`` -- batches on which only the discriminator or only the generator trains
(train.py:841, :864) -- against the fp64 oracle one batch at a time, captured against eager bit for bit, and what has to hold
around them: fresh noise on consecutive critic steps, no generator-ahead branch left open, resume in the middle of a cycle, one
batch of the data stream per ``step()``, and the default step unchanged."""
import contextlib
import itertools

import numpy as np
import pytest
import torch

from conftest import assert_grads

pytestmark = pytest.mark.gpu

N = 30
DG, D_, G_ = ("D", "G"), ("D",), ("G",)
# (num_critic, num_gen) -> what batches 0, 1, 2, ... of an epoch run, written out from train.py:841 / :864
RAN = {(3, 1): [D_, DG, D_, D_, DG, D_, D_], (2, 1): [D_, DG, D_, DG], (1, 2): [DG, DG, G_, DG, G_], (1, 1): [DG] * 3}


def _nets(model="mpgan", disc_dropout=0.0, loss="ls", seeds=(41, 42)):
    """(G, D, latent, (lr_disc, lr_gen)) with the oracle's name-keyed initial values."""
    from oracle import train_ref as T
    from mpgan_amd import train
    if model == "mpgan":
        G, D = train.default_mpgan(N, disc_dropout=disc_dropout, loss=loss)
        shapes, latent, lrs = T.mpgan_param_shapes, 32, train.LR["g"]
    else:
        G, D = train.default_gapt(N, disc_dropout=disc_dropout)
        shapes, latent, lrs = T.gapt_param_shapes, 64, train.LR_GAPT
    G.load_state_dict(T.init_state_dict(shapes(True), seeds[0], torch.float32))
    D.load_state_dict(T.init_state_dict(shapes(False), seeds[1], torch.float32))
    return G, D, latent, lrs


def _fixed_noise(B, latent, seed=5):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(B, N, latent, device="cuda", generator=gen) * 0.2, torch.randn(B, N, latent, device="cuda", generator=gen) * 0.2)


def _step(model="mpgan", B=8, disc_dropout=0.0, loss="ls", fixed=True, seeds=(41, 42), data_seed=3, **kw):
    from mpgan_amd import train
    from oracle.train_ref import synthetic_batch
    G, D, latent, lrs = _nets(model, disc_dropout, loss, seeds)
    ts = train.TrainStep(G, D, B, N, latent=latent, lr_disc=lrs[0], lr_gen=lrs[1], loss=loss, **kw)
    if ts.loader is None:
        data, labels = synthetic_batch(B, N, seed=data_seed)
        ts.set_batch(data.cuda(), labels.cuda())
    if fixed:
        ts.fixed_noise = _fixed_noise(B, latent)
    return ts


@contextlib.contextmanager
def _device_seed(value=0x5EED):
    """The device's noise / dropout seed set to ``value`` for a run, and the device handed back as one nobody has seeded."""
    from mpgan_amd import ops
    dev = torch.device("cuda", torch.cuda.current_device())
    st = ops.dev_state(dev)
    try:
        yield lambda: ops.set_seed(value, dev)
    finally:
        st.seed_is_default, st.auto_seed_key = True, None


def _state(ts, device_counters=True):
    """Everything ``_training_state`` lists, the optimizers' step counts and ``batch_ndx``.  ``device_counters=False``: without
    ``FlatParams.step_count``, which only Adam's launch reads and writes -- under RMSprop an uninterrupted run leaves it at zero and
    ``load_state_dict`` fills it with the saved count (``FlatParams.steps``, compared below, is the host's count there)."""
    torch.cuda.synchronize()
    skip = () if device_counters else (ts.fD.step_count, ts.fG.step_count)
    return [t.clone() for t in ts._training_state() if not any(t is c for c in skip)] + \
        [torch.tensor([ts.fD.steps, ts.fG.steps, float(ts.batch_ndx)])]


def _all_equal(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


# ---- 1. against the fp64 oracle, one batch at a time ------------------------------------------------------------------------
def _named(flat, buf, dtype=torch.float64):
    names = [k for k, p in flat.module.named_parameters() if p.requires_grad]
    assert len(names) == len(flat._spans)
    return {k: buf[off:off + n].view(shape).detach().to("cpu", dtype).clone() for k, (off, n, shape) in zip(names, flat._spans)}


def _watch(flat, log, key):
    """``log[key]``: the gradient buffer as the optimizer launch of ``flat`` found it (the launch clears it)."""
    import weakref
    ref = weakref.ref(flat)      # (no cycle through the instance attribute: the step and its buffers go when the test ends)

    def step(*args, **kwargs):
        f = ref()
        log[key] = f.grad.clone()
        return type(f).step(f, *args, **kwargs)
    flat.step = step


@pytest.mark.parametrize("loss", ["w", "ls"])
@pytest.mark.parametrize("num_critic,num_gen", [(3, 1), (1, 2)])
def test_each_batch_of_a_cycle_vs_oracle(loss, num_critic, num_gen):
    """num_critic = 3: batches D / D+G / D; num_gen = 2: batches 0..3 = D+G / D+G / G / D+G (train.py:841: (3 - 1) % 2 == 0, batch 3
    trains D again).  Before each batch the step's parameters and RMSprop state go into the oracle's dicts, so every comparison
    covers one batch.  A D-only batch is the oracle's iteration with lr_gen = 0 on a throw-away copy of G's state, a G-only batch
    the one with lr_disc = 0 on a throw-away copy of D's; a D+G batch is both, the second from D's parameters as the step's own
    update left them -- the existing test keeps lr_disc at 0 for the same reason: under ``w`` D's last biases have a gradient that
    vanishes by symmetry, RMSprop turns its rounding noise into a full-size step of either sign, and the last bias shifts every
    output, G_loss with them (measured with the oracle's own D update in that place: G_loss -0.21002 against -0.20906).
    Compared, with the bars of
    ``test_gpu_train.py::test_train_step_other_losses_vs_oracle`` and ``conftest.assert_grads`` as it uses it: the losses the batch
    wrote (1e-4) and the gradients its optimizer launches consumed (1e-3, or the fp32 oracle's own error) -- the quantities those
    bars were made for; RMSprop turns a gradient within rounding of zero into a full-size step of either sign, so the parameters
    are held to the step's own gradient instead: p - lr g / (sqrt(0.99 v + 0.01 g^2) + 1e-8) in fp64, to fp32's rounding of p plus
    1e-5 of the largest update (``test_fused_optimizers_vs_torch``'s bar).  The network that does not train is ``torch.equal`` to
    what it was: parameters, optimizer state, step counter, its loss."""
    from oracle import train_ref as T
    B = 8
    ts = _step("mpgan", B, loss=loss, use_graphs=False, num_critic=num_critic, num_gen=num_gen)
    assert ts._route() in ("parts", "into")
    cfg = {"D": {"sigmoid": loss not in ("w", "hinge")}}
    data, labels = ts.data.cpu(), ts.labels.cpu()
    nD, nG = (z.cpu() for z in ts.fixed_noise)
    log = {}
    _watch(ts.fD, log, "D")
    _watch(ts.fG, log, "G")
    nets = {"D": (ts.fD, ts.lr_disc, ts.D_loss), "G": (ts.fG, ts.lr_gen, ts.G_loss)}
    for b, ran in enumerate(RAN[(num_critic, num_gen)][:3 if num_critic > 1 else 4]):
        before = {k: (_named(f, f.flat), _named(f, f.sq), f.steps, float(l)) for k, (f, _, l) in nets.items()}
        frozen = {k: (f.flat.clone(), f.sq.clone(), f.grad.clone()) for k, (f, _, _) in nets.items()}
        log.clear()
        ts.step()
        torch.cuda.synchronize()
        assert ts.last_ran == ran and set(log) == set(ran), (b, ts.last_ran, sorted(log))
        # train_D's half: the oracle's iteration from the parameters before the batch with lr_gen = 0; train_G's half: the one from
        # D's parameters as the batch left them (the ones before it where D did not train) with lr_disc = 0
        halves = {"D": (before["D"][0], ts.lr_disc, 0.0), "G": (_named(ts.fD, ts.fD.flat), 0.0, ts.lr_gen)}
        oracle = {"fp32": [None] * 4, "fp64": [None] * 4}
        for i, k in enumerate(("D", "G")):
            if k not in ran:
                continue
            sdD, lr_d, lr_g = halves[k]
            for name, dt in (("fp32", torch.float32), ("fp64", torch.float64)):
                cast = lambda d: {k: v.to(dt).clone() for k, v in d.items()}     # (the oracle updates its dicts in place)
                out = T.train_iteration("mpgan", cast(sdD), cast(before["G"][0]), cast(before["D"][1]), cast(before["G"][1]), data.to(dt),
                                        labels.to(dt), nD.to(dt), nG.to(dt), lr_d, lr_g, return_grads=True, loss=loss, cfg=cfg)
                oracle[name][i], oracle[name][2 + i] = out[i], out[2 + i]
        num = lambda d: {k: v.detach().double().numpy() for k, v in d.items()}
        for i, (k, (f, lr, l)) in enumerate(nets.items()):
            p0, v0, steps0, loss0 = before[k]
            if k not in ran:
                assert torch.equal(f.flat, frozen[k][0]) and torch.equal(f.sq, frozen[k][1]) and torch.equal(f.grad, frozen[k][2]), (b, k)
                assert f.steps == steps0 and float(l) == loss0, (b, k)
                continue
            want = oracle["fp64"][i]
            print("batch", b, ran, k, "loss", float(l), "oracle", want)
            assert abs(float(l) - want) < 1e-4 * max(abs(want), 1e-3), (b, k, float(l), want)
            assert_grads(num(_named(f, log[k])), num(oracle["fp64"][2 + i]), 1e-3, control=num(oracle["fp32"][2 + i]),
                         what=("schedule", loss, num_critic, num_gen, b, k))
            assert f.steps == steps0 + 1 and not bool(f.grad.any()), (b, k)
            g, p1 = _named(f, log[k]), _named(f, f.flat)
            for name in p0:
                v = 0.99 * v0[name] + 0.01 * g[name] ** 2
                upd = -lr * g[name] / (v.sqrt() + 1e-8)
                err = float((p1[name] - p0[name] - upd).abs().max())
                assert err <= 2.0 ** -23 * float(p0[name].abs().max()) + 1e-5 * float(upd.abs().max()), (b, k, name, err)


# ---- 2. graphs equal eager, bit for bit ---------------------------------------------------------------------------------------
TAG_BASE = {"DG": 1000, "D": 2000, "G": 3000}


@pytest.mark.parametrize("model,num_critic,num_gen,split", [("mpgan", 3, 1, False), ("mpgan", 3, 1, True), ("mpgan", 1, 2, False),
                                                            ("gapt", 3, 1, False), ("gapt", 1, 2, False)])
def test_captured_kinds_equal_eager_bit_for_bit(monkeypatch, model, num_critic, num_gen, split):
    """Two full cycles with D's dropout at 0.5 and fresh noise: parameters, optimizer state, step counters, the seed and the losses
    of the captured run equal the eager run's after every batch.  The seed is set to one value before each run.  Dropout sites are
    numbered in host order (``ops.next_tag``) and a capture freezes the numbers it saw, so both runs are given the same ones: each
    kind of batch starts from a base of its own -- before its capture (without warm-up iterations, which would move the counter)
    and before every eager batch."""
    from mpgan_amd import ops
    ran = RAN[(num_critic, num_gen)]
    kinds = ["".join(r) for r in ran]
    if split:
        monkeypatch.setenv("MPG_SPLIT_GRAPHS", "1")
    res = []
    with _device_seed() as seed:
        for use_graphs in (False, True):
            seed()
            ts = _step(model, 8, disc_dropout=0.5, fixed=False, use_graphs=use_graphs, num_critic=num_critic, num_gen=num_gen)
            st = ops.dev_state(ts.dev)
            if use_graphs:
                for kind in dict.fromkeys(kinds):     # (in the order of first use)
                    st.tags = itertools.count(TAG_BASE[kind])
                    ts.capture(warmup=0, kind=kind)
                n = {k: len(ts._graphs if k == "DG" else ts._alone_graphs[k]) for k in set(kinds)}
                assert n == {k: ({"DG": 3, "D": 2, "G": 2}[k] if split else 1) for k in set(kinds)}, n
            seen = []
            for b, kind in enumerate(kinds):
                st.tags = itertools.count(TAG_BASE[kind])
                ts.step()
                assert ts.last_ran == ran[b]
                seen.append(_state(ts))
            res.append(seen)
    for b, (a, c) in enumerate(zip(*res)):
        assert _all_equal(a, c), (b, kinds[b], [i for i, (x, y) in enumerate(zip(a, c)) if not torch.equal(x, y)])
    losses = [float(s[0]) for s in res[0]]
    assert all(np.isfinite(v) for v in losses) and len(set(losses)) > 1


# ---- 3. consecutive critic steps draw fresh noise; the seed moves once per batch -----------------------------------------------
def test_consecutive_critic_steps_generate_different_jets():
    from mpgan_amd import ops
    B = 8
    with _device_seed() as seed:
        seed()
        ts = _step("mpgan", B, fixed=False, num_critic=5)
        start = ops.get_seed(ts.dev)
        jets = []
        for b in range(6):                      # D, D+G, D, D, D, D: the real batch stays the one set once
            ts.step()
            torch.cuda.synchronize()
            jets.append((ts._x3 if ts.parts else ts._dcat)[B:, :, :3].clone())
        assert ts.last_ran == ("D",) and ts._alone_graphs.keys() == {"D"}
        assert bool(jets[2].abs().sum() > 0)
        for a, c in itertools.combinations(jets[2:], 2):      # batches 2..5 are D alone
            assert not torch.equal(a, c)
        assert ops.get_seed(ts.dev) == (start + 6 * ops.SEED_STEP) & 0xFFFFFFFFFFFFFFFF
        for num_critic, num_gen, eager in ((1, 1, False), (3, 1, True), (1, 2, False), (1, 2, True)):
            seed()
            ts = _step("mpgan", B, fixed=False, num_critic=num_critic, num_gen=num_gen, use_graphs=not eager)
            for _ in range(5):
                ts.step()
            assert ops.get_seed(ts.dev) == (start + 5 * ops.SEED_STEP) & 0xFFFFFFFFFFFFFFFF, (num_critic, num_gen, eager)


# ---- 4. a D-only batch opens no generator-ahead branch --------------------------------------------------------------------------
@pytest.mark.parametrize("use_graphs", [True, False])
def test_no_branch_is_opened_without_a_generator_step_to_join_it(monkeypatch, use_graphs):
    def run(env=()):
        with monkeypatch.context() as m, _device_seed() as seed:
            for name, value in env:
                m.setenv(name, value)
            seed()
            ts = _step("mpgan", 8, num_critic=2, use_graphs=use_graphs)
        joins = []
        for b, ran in enumerate(RAN[(2, 1)]):
            before = ts.gen_join
            ts.step()
            torch.cuda.synchronize()
            assert ts.last_ran == ran and not ts._ahead.open and ts._ahead.jets is None
            if ran == D_:
                assert ts.gen_join == before, (b, before, ts.gen_join)
            joins.append(ts.gen_join)
        return ts, joins, _state(ts)

    ts, joins, res = run()
    assert ts.gen_ahead and ts.gen_ahead_late
    assert joins == [None, "seg_G", "seg_G", "seg_G"], joins
    off, joins_off, res_off = run((("MPG_GEN_AHEAD", "0"),))
    assert off.gen_ahead is False and joins_off == [None] * 4
    assert _all_equal(res, res_off)


# ---- 5. the gradient penalty's route ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["mpgan", "gapt"])
def test_gradient_penalty_schedule_under_graphs_equals_eager(model):
    """``test_gradient_penalty_under_graphs_equals_eager`` with num_critic = 2 (D / D+G / D / D+G) at B = 4: dropout off, fixed noise
    and interpolation weights; parameters and the three losses bit for bit."""
    B = 4
    res = []
    for use_graphs in (False, True):
        ts = _step(model, B, loss="w", data_seed=13, use_graphs=use_graphs, gp_lambda=10.0, num_critic=2)
        assert ts._route() == "module"
        ts.fixed_alpha = torch.rand(B, 1, 1, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
        for ran in RAN[(2, 1)]:
            ts.step()
            assert ts.last_ran == ran
        torch.cuda.synchronize()
        res.append((ts.fD.flat.clone(), ts.fG.flat.clone(), float(ts.D_loss), float(ts.GP), float(ts.G_loss)))
        assert (ts.fD.steps, ts.fG.steps) == (4, 2)
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]) and res[0][2:] == res[1][2:]
    assert res[0][3] > 0


# ---- 6. resume in the middle of a cycle ---------------------------------------------------------------------------------------
def test_resume_mid_cycle_equals_the_uninterrupted_run(tmp_path):
    from mpgan_amd import checkpoint as ck
    tmp = str(tmp_path / "models")
    ran = RAN[(3, 1)][:6]
    with _device_seed() as seed:
        seed()
        ts = _step("mpgan", 8, num_critic=3)
        for b in range(6):
            ts.step()
            assert ts.last_ran == ran[b]
            if b == 1:
                torch.cuda.synchronize()
                ck.save_models(ts.D, ts.G, ts.fD, ts.fG, tmp, 2)
        whole = _state(ts, device_counters=False)
        seed()
        again = _step("mpgan", 8, num_critic=3, seeds=(77, 78))      # other weights: everything comes from the files
        ck.load_models(again.D, again.G, tmp, 2)
        ck.load_optimizers(again.fD, again.fG, tmp, 2)
        assert again.batch_ndx == 2
        for b in range(2, 6):
            again.step()
            assert again.last_ran == ran[b], b
        got = _state(again, device_counters=False)
        assert _all_equal(whole, got), [i for i, (x, y) in enumerate(zip(whole, got)) if not torch.equal(x, y)]
        assert (again.fD.steps, again.fG.steps) == (6, 2)


# ---- 7. one batch of the data stream per step(), whichever kind ------------------------------------------------------------------
@pytest.mark.parametrize("use_graphs", [True, False])
def test_every_step_consumes_one_batch_of_the_loader(use_graphs):
    from mpgan_amd.data import DeviceJetLoader, synthetic_jets
    B, n = 4, 10
    particles, labels = synthetic_jets(n, N, seed=3, dist="uniform")
    loader = DeviceJetLoader((particles, labels), B, "cuda", seed=21)
    ts = _step("mpgan", B, num_gen=2, use_graphs=use_graphs, loader=loader)
    for step, ran in enumerate(RAN[(1, 2)]):
        ts.step()
        torch.cuda.synchronize()
        assert ts.last_ran == ran
        assert loader.position == (step + 1) * loader.stride, (step, ran, loader.position)
        idx = loader.indices(step)
        assert torch.equal(ts.labels.cpu(), labels[idx].reshape(B, 1)), (step, ran)
        assert torch.equal(ts.data.cpu(), particles[idx]), (step, ran)
    assert bool(torch.isfinite(ts.fG.flat).all()) and np.isfinite(float(ts.G_loss))


# ---- 8. the defaults are the step as it was -----------------------------------------------------------------------------------
def test_counts_of_one_are_the_default_step():
    res = []
    with _device_seed() as seed:
        for kw in ({}, dict(num_critic=1, num_gen=1)):
            seed()
            ts = _step("mpgan", 8, fixed=False, **kw)
            for _ in range(3):
                ts.step()
                assert ts.last_ran == ("D", "G")
            three = _state(ts)
            ts.start_epoch()          # (nothing depends on the batch index)
            ts.step()
            assert len(ts._graphs) == 1 and not ts._alone_graphs and ts.epoch_sums is None
            res.append(three + _state(ts)[:-1])
    assert _all_equal(*res)
