"""The num_critic / num_gen update schedule of ``TrainStep`` on the CPU (toy modules, torch RMSprop in place of the fused step):
which of train_D / train_G a batch runs (train.py:841, :864), that a batch on which a network does not train leaves it alone, what
travels with a checkpoint, and how the epoch's loss sums are divided (train.py:960-962)."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from test_dist_cpu import ToyG, ToyD, ToyD2, _torch_rmsprop, _inputs, N, LAT  # noqa: E402

B = 4
DG, D_, G_ = ("D", "G"), ("D",), ("G",)
# batches 0..12 of an epoch, read off train.py:841 (train_D: num_critic > 1, or batch 0, or (batch - 1) % num_gen == 0) and :864
# (train_G: num_critic == 1, or (batch - 1) % num_critic == 0) by hand
TABLE = {
    (1, 1): [DG, DG, DG, DG, DG, DG, DG, DG, DG, DG, DG, DG, DG],
    (2, 1): [D_, DG, D_, DG, D_, DG, D_, DG, D_, DG, D_, DG, D_],          # G on 1, 3, 5, ...
    (5, 1): [D_, DG, D_, D_, D_, D_, DG, D_, D_, D_, D_, DG, D_],          # G on 1, 6, 11
    (1, 2): [DG, DG, G_, DG, G_, DG, G_, DG, G_, DG, G_, DG, G_],          # D on 0, 1, 3, 5, ...
    (1, 3): [DG, DG, G_, G_, DG, G_, G_, DG, G_, G_, DG, G_, G_],          # D on 0, 1, 4, 7, 10
}


def _toy(monkeypatch, D=None, **kw):
    from mpgan_amd import train
    monkeypatch.setattr(train.FlatParams, "step", _torch_rmsprop)
    torch.manual_seed(3)
    ts = train.TrainStep(ToyG(), D if D is not None else ToyD(), B, N, latent=LAT, lr_disc=1e-2, lr_gen=2e-2, use_graphs=False, **kw)
    data, labels, _, _ = _inputs(B)
    ts.set_batch(data, labels)
    return ts


@pytest.mark.parametrize("num_critic,num_gen", sorted(TABLE))
def test_batches_run_what_the_references_two_conditions_say(monkeypatch, num_critic, num_gen):
    ts = _toy(monkeypatch, num_critic=num_critic, num_gen=num_gen)
    want = TABLE[(num_critic, num_gen)]
    assert ts.batch_ndx == 0 and ts.last_ran == ()
    for epoch in range(2):
        for b in range(13):
            assert ts.batch_ndx == b
            steps = (ts.fD.steps, ts.fG.steps)
            ts.step()
            assert ts.last_ran == want[b], (epoch, b, ts.last_ran)
            # ... and the optimizers that stepped are the ones it names
            assert (ts.fD.steps - steps[0], ts.fG.steps - steps[1]) == ("D" in want[b], "G" in want[b]), (epoch, b)
        assert ts.batch_ndx == 13
        ts.start_epoch()          # (enumerate restarts: batch 0 again)
        assert ts.batch_ndx == 0


def test_counts_that_are_no_schedule_are_refused(monkeypatch):
    from mpgan_amd import train
    for kw in (dict(num_critic=0), dict(num_gen=0), dict(num_critic=-1), dict(num_critic=2.0), dict(num_gen=True)):
        with pytest.raises(ValueError, match="integer >= 1"):
            train.TrainStep(ToyG(), ToyD(), B, N, latent=LAT, use_graphs=False, **kw)
    with pytest.raises(ValueError, match="num-critic must be 1 for this to apply"):
        train.TrainStep(ToyG(), ToyD(), B, N, latent=LAT, use_graphs=False, num_critic=2, num_gen=2)


def _net_state(f):
    return [f.flat.clone(), f.sq.clone(), f.grad.clone(), f.step_count.clone(), torch.tensor(float(f.steps))] + \
        ([f.aux.clone()] if f.aux is not None else [])


def test_a_batch_on_which_a_network_does_not_train_leaves_it_alone(monkeypatch):
    """D only (num_critic = 2, batch 0): G's parameters, optimizer state, step counter and G_loss stay; the seed moves on.  G only
    (num_gen = 2, batch 2): D's parameters, optimizer state, step counter, gradient buffer and D_loss stay; the seed moves on."""
    from mpgan_amd import ops
    cpu = torch.device("cpu")
    ts = _toy(monkeypatch, num_critic=2)
    seed = ops.get_seed(cpu)
    before_G, before_D, g_loss = _net_state(ts.fG), _net_state(ts.fD), ts.G_loss.clone()
    ts.step()
    assert ts.last_ran == ("D",)
    assert all(torch.equal(a, b) for a, b in zip(before_G, _net_state(ts.fG))) and torch.equal(ts.G_loss, g_loss)
    assert not torch.equal(before_D[0], ts.fD.flat) and ts.fD.steps == 1 and not bool(ts.fD.grad.any())
    assert ops.get_seed(cpu) == (seed + ops.SEED_STEP) & 0xFFFFFFFFFFFFFFFF
    assert ts.gen_join is None

    ts = _toy(monkeypatch, num_gen=2)
    ts.step(); ts.step()
    seed = ops.get_seed(cpu)
    before_G, before_D, d_loss = _net_state(ts.fG), _net_state(ts.fD), ts.D_loss.clone()
    ts.step()
    assert ts.last_ran == ("G",)
    assert all(torch.equal(a, b) for a, b in zip(before_D, _net_state(ts.fD))) and torch.equal(ts.D_loss, d_loss)
    assert not torch.equal(before_G[0], ts.fG.flat) and ts.fG.steps == 3 and not bool(ts.fG.grad.any())
    assert ops.get_seed(cpu) == (seed + ops.SEED_STEP) & 0xFFFFFFFFFFFFFFFF


def test_batch_ndx_travels_with_the_generators_optimizer_state(monkeypatch):
    from mpgan_amd import train
    ts = _toy(monkeypatch, num_critic=3)
    for _ in range(2):
        ts.step()
    sdD, sdG = ts.optimizer_state_dicts()
    assert sdG["param_groups"][0][train.FlatParams.BATCH_KEY] == 2 and train.FlatParams.BATCH_KEY not in sdD["param_groups"][0]
    torch.optim.RMSprop([torch.zeros(tuple(p.shape)) for p in ts.G.parameters()], lr=1.0).load_state_dict(sdG)   # torch reads it
    again = _toy(monkeypatch, num_critic=3)
    again.load_optimizer_state_dicts(sdD, sdG)
    assert again.batch_ndx == 2
    again.step()
    assert again.last_ran == ("D",)         # (batch 2 of num_critic = 3; batch 0 would be D alone as well, batch 1 both:)
    again.load_optimizer_state_dicts(sdD, sdG)
    again.batch_ndx = 1
    again.step()
    assert again.last_ran == ("D", "G")
    del sdG["param_groups"][0][train.FlatParams.BATCH_KEY]     # a file without the field: the top of an epoch
    again.load_optimizer_state_dicts(sdD, sdG)
    assert again.batch_ndx == 0


@pytest.mark.parametrize("num_critic,num_gen,gp", [(1, 1, 0.0), (2, 1, 10.0), (1, 2, 0.0)])
def test_epoch_losses_divide_as_the_reference_does(monkeypatch, num_critic, num_gen, gp):
    """Seven batches whose losses are read after each: the D side's sums over 7 / num_gen, G's over 7 / num_critic
    (train.py:960-962), whatever the number of times each ran; reading resets, and so does ``start_epoch``."""
    kw = dict(loss="w", gp_lambda=gp, D=ToyD2()) if gp else {}
    ts = _toy(monkeypatch, num_critic=num_critic, num_gen=num_gen, track_epoch_losses=True, **kw)
    n = 7
    for epoch in range(2):
        terms = {"D": [], "gp": [], "G": []}
        for b in range(n):
            ts.step()
            if "D" in ts.last_ran:
                terms["D"].append(float(ts.D_loss))
                terms["gp"].append(float(ts.GP))
            if "G" in ts.last_ran:
                terms["G"].append(float(ts.G_loss))
        assert (len(terms["D"]), len(terms["G"])) == {(1, 1): (7, 7), (2, 1): (7, 3), (1, 2): (4, 7)}[(num_critic, num_gen)]
        over = {"D": n / num_gen, "gp": n / num_gen, "G": n / num_critic}
        got = ts.epoch_losses(reset=epoch == 1)
        assert set(got) == {"D", "gp", "G"}
        for k, v in terms.items():
            # (the sums are fp32: n additions, each within 2^-24 of the running sum, which sum |term| bounds)
            assert abs(got[k] - sum(v) / over[k]) <= n * 2.0 ** -24 * sum(abs(t) for t in v) / over[k], (k, got, v)
        assert (got["gp"] > 0) == bool(gp)
        if epoch == 0:
            assert ts.epoch_losses(reset=False) == got      # (not reset: read again)
            ts.start_epoch()                                # ... which the top of the next epoch does
    with pytest.raises(RuntimeError, match="no step"):
        ts.epoch_losses()
    with pytest.raises(RuntimeError, match="track_epoch_losses"):
        _toy(monkeypatch).epoch_losses()


def test_a_step_is_freed_when_its_last_reference_goes(monkeypatch):
    """No reference cycle through the step: its graphs and buffers are released where the caller drops it, not by a garbage
    collection that may run in the middle of another step's capture (where destroying a hipGraph aborts the process)."""
    import gc
    import weakref
    gc.collect()
    gc.disable()
    try:
        for kw in (dict(), dict(num_critic=2), dict(num_gen=2, track_epoch_losses=True)):
            ts = _toy(monkeypatch, **kw)
            for _ in range(4):
                ts.step()
            ts.fG.load_state_dict(ts.fG.state_dict())
            refs = [weakref.ref(ts), weakref.ref(ts.fG), weakref.ref(ts.fD)]
            del ts
            assert all(r() is None for r in refs), kw
    finally:
        gc.enable()
