"""CPU: the carried state of ``TrainStep`` (``train.SeedState`` / ``Schedule`` / ``AdaController`` / ``DeviceWords``) on toy networks --
which optimizer file holds which key, what a missing key loads, and that every carried device word is part of what ``capture``
puts back behind its warm-up."""
import copy

import pytest
import torch

from test_dist_cpu import ToyG, _torch_rmsprop, _inputs, N, LAT
from test_ada_cpu import LabelFreeD

B = 4
AUG = dict(aug_r90=True, aug_f=True, aug_t=True, aug_s=True, adaptive_prob=True, aug_prob=0.25, ada_target=0.5, ada_interval=2,
           ada_kimg=0.064)


def _step(seed=3):
    from mpgan_amd import train
    torch.manual_seed(seed)
    data, labels, nD, nG = _inputs(B)
    ts = train.TrainStep(ToyG(), LabelFreeD(), B, N, latent=LAT, lr_disc=1e-2, lr_gen=2e-2, use_graphs=False,
                         augment=train.Augment(**AUG), label_noise=0.1, num_critic=2, track_epoch_losses=True)
    ts.set_batch(data, labels)
    ts.fixed_noise = (nD, nG)
    return ts


def _custom(group):
    return {k for k in group if k.startswith("mpgan_amd_")}


def test_keys_are_in_the_right_file(monkeypatch):
    from mpgan_amd import train
    monkeypatch.setattr(train.FlatParams, "step", _torch_rmsprop)
    ts = _step()
    for _ in range(3):
        ts.step()
    gD, gG = (sd["param_groups"][0] for sd in ts.optimizer_state_dicts())
    assert _custom(gD) == {"mpgan_amd_ada"} and _custom(gG) == {"mpgan_amd_batch_ndx"}     # (the seed's two keys: GPU only)
    assert gD["mpgan_amd_ada"] == ts.ada and gG["mpgan_amd_batch_ndx"] == ts.batch_ndx == 3
    assert ts.ada["steps"] == 1                                                            # three D steps: an interval and a half


def test_missing_keys_give_the_defaults():
    ada = {"p": 0.375, "r": 0.5, "sign_sum": -2, "steps": 1}
    gD = {"lr": 1e-2, "params": list(range(len(list(LabelFreeD().parameters())))), "mpgan_amd_ada": dict(ada)}
    gG = {"lr": 2e-2, "params": list(range(len(list(ToyG().parameters())))), "mpgan_amd_batch_ndx": 5, "mpgan_amd_seed": 123,
          "mpgan_amd_seed_rank": 0}

    def load(gD, gG):
        ts = _step(seed=9)
        ts.batch_ndx = 2
        ts.set_aug_prob(0.75)
        ts.load_optimizer_state_dicts({"state": {}, "param_groups": [copy.deepcopy(gD)]}, {"state": {}, "param_groups": [copy.deepcopy(gG)]})
        return ts

    ts = load(gD, gG)
    assert ts.ada == ada and ts.batch_ndx == 5
    assert ts.optimizer_state_dicts()[0]["param_groups"][0]["mpgan_amd_ada"] == ada
    assert ts.optimizer_state_dicts()[1]["param_groups"][0]["mpgan_amd_batch_ndx"] == 5
    bare = load({k: v for k, v in gD.items() if k != "mpgan_amd_ada"}, gG)
    assert bare.ada == {"p": 0.25, "r": 0.0, "sign_sum": 0, "steps": 0} and bare.batch_ndx == 5
    bare = load(gD, {k: v for k, v in gG.items() if k != "mpgan_amd_batch_ndx"})
    assert bare.batch_ndx == 0 and bare.ada == ada
    # the seed: left alone without its key -- and, on a device that carries one, set from it
    from mpgan_amd import ops, train
    cpu = torch.device("cpu")
    st = ops.dev_state(cpu)
    before, flags = ops.get_seed(cpu), (st.seed_is_default, st.auto_seed_key)
    try:
        seeded = _step(seed=9)
        seeded.fG.carried.insert(0, train.SeedState(cpu, 0))
        ops.set_seed(77, cpu)
        seeded.load_optimizer_state_dicts({"state": {}, "param_groups": [dict(gD)]},
                                          {"state": {}, "param_groups": [{k: v for k, v in gG.items() if "seed" not in k}]})
        assert ops.get_seed(cpu) == 77
        seeded.load_optimizer_state_dicts({"state": {}, "param_groups": [dict(gD)]}, {"state": {}, "param_groups": [dict(gG)]})
        assert ops.get_seed(cpu) == 123
    finally:
        ops.set_seed(before, cpu)
        st.seed_is_default, st.auto_seed_key = flags
    with pytest.raises(ValueError, match="counts 2 D steps into an interval of 2"):
        load(dict(gD, mpgan_amd_ada=dict(ada, steps=2)), gG)


def test_the_protocol_is_complete():
    from mpgan_amd import train
    ts = _step()
    state = ts._training_state()
    carried = ts.fD.carried + ts.fG.carried
    words = [t for c in carried for t in c.tensors()]
    assert all(any(t is s for s in state) for t in words)
    # ... and they are the words the options own: the probability and the controller's two, the epoch's three sums
    for t in [ts.aug_p, ts._ada.state, ts._ada.r] + list(ts.epoch_sums.values()):
        assert any(t is w for w in words)
    assert all(hasattr(c, "save") and hasattr(c, "load") for c in carried)
    flat = train.FlatParams(ToyG())
    assert flat.carried == [] and not _custom(flat.state_dict()["param_groups"][0])
