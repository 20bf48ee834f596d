"""Host-side pieces around the hot path that need no GPU: synthetic data, (un)normalisation, checkpoint / loss-history
formats of a reference run, optimiser state dicts in torch.optim layout, per-device op state."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_synthetic_jets_match_the_oracle_generator():
    from mpgan_amd.data import synthetic_jets
    from oracle.train_ref import synthetic_batch
    for B, N, d in ((64, 30, "gluon"), (64, 30, "uniform"), (16, 150, "gluon")):
        a, b = synthetic_jets(B, N, 5, d), synthetic_batch(B, N, 5, d)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        data, labels = a
        n = (labels[:, 0] * N).int()                       # the round trip the generator's mask_c relies on
        assert torch.equal(n, (data[..., 3] > 0).sum(1).int())
    with pytest.raises(ValueError):
        synthetic_jets(4, 30, dist="nope")


def test_normalise_unnormalise_round_trip_and_dataset():
    from mpgan_amd.data import JetArrayDataset, unnormalise_jets, FEATURE_MAXES
    rs = np.random.RandomState(0)
    raw = rs.uniform(0, 1, size=(20, 30, 4)).astype(np.float32) * np.array(FEATURE_MAXES["t"], dtype=np.float32)
    raw[..., 3] = (rs.uniform(size=(20, 30)) > 0.3)
    raw[..., :3] *= raw[..., 3:]
    ds = JetArrayDataset(raw, jet_type="t", split="all")
    x, lab = ds[3]
    assert x.shape == (30, 4) and abs(float(lab) - raw[3, :, 3].sum() / 30) < 1e-6
    assert float(ds.particle_data[..., 2].min()) >= -0.5 - 1e-6 and float(ds.particle_data[..., 2].max()) <= 0.5 + 1e-6
    back = unnormalise_jets(ds.particle_data, "t")
    assert torch.allclose(back, torch.from_numpy(raw[..., :3]), atol=1e-6)
    tr, va = JetArrayDataset(raw, split="train"), JetArrayDataset(raw, split="valid")
    assert len(tr) == 14 and len(va) == 6


def test_checkpoint_formats_round_trip(tmp_path):
    from mpgan_amd import checkpoint as ck
    D, G = torch.nn.Linear(3, 2), torch.nn.Linear(4, 3)
    oD, oG = torch.optim.RMSprop(D.parameters(), lr=3e-5), torch.optim.RMSprop(G.parameters(), lr=1e-5)
    D(torch.randn(5, 3)).sum().backward(); oD.step()
    G(torch.randn(5, 4)).sum().backward(); oG.step()
    mp = str(tmp_path / "models")
    assert ck.latest_epoch(mp) == 0
    ck.save_models(D, G, oD, oG, mp, 5)
    ck.save_models(D, G, oD, oG, mp, 10)
    torch.save(D.state_dict(), os.path.join(mp, "D_15.pt"))      # G_15 missing: epoch 15 does not count
    assert sorted(os.listdir(mp))[:4] == ["D_10.pt", "D_15.pt", "D_5.pt", "D_optim_10.pt"]
    assert ck.latest_epoch(mp) == 10
    D2, G2 = torch.nn.Linear(3, 2), torch.nn.Linear(4, 3)
    ck.load_models(D2, G2, mp, 10)
    assert torch.equal(D2.weight, D.weight) and torch.equal(G2.bias, G.bias)
    o2D, o2G = torch.optim.RMSprop(D2.parameters(), lr=1.0), torch.optim.RMSprop(G2.parameters(), lr=1.0)
    ck.load_optimizers(o2D, o2G, mp, 10)
    assert o2D.state_dict()["param_groups"][0]["lr"] == 3e-5
    assert torch.equal(o2G.state_dict()["state"][0]["square_avg"], oG.state_dict()["state"][0]["square_avg"])
    # loss histories
    keys, eval_keys = ck.loss_keys(gp=False, fpnd=False, fpd=True, efp=False)
    assert keys == ["D", "Dr", "Df", "G", "w1p", "w1m", "fpd"]
    losses = {"D": [0.5, 0.4, 0.3], "Dr": [0.2, 0.2, 0.1], "Df": [0.3, 0.2, 0.2], "G": [0.9, 0.8, 0.7],
              "w1p": [[1e-3, 1e-4]], "w1m": [[2e-3, 2e-4]], "fpd": [[0.5, 0.01]]}
    lp = str(tmp_path / "losses")
    ck.save_losses(losses, lp)
    back = ck.load_losses(lp, keys, eval_keys, start_epoch=1, save_epochs=5)
    assert back["D"] == [0.5, 0.4] and back["w1p"] == [[1e-3, 1e-4]] and back["fpd"] == [[0.5, 0.01]]
    assert ck.load_losses(lp, ["nope"])["nope"] == []


@pytest.mark.parametrize("opt", ["rmsprop", "adam", "adadelta"])
def test_flat_params_speak_torch_optim_state_dicts(opt):
    """FlatParams.state_dict() loads into the matching torch.optim class and vice versa (the reference's
    *_optim_<epoch>.pt files, train.py:534-535 / setup_training.py:1525-1535)."""
    from mpgan_amd.train import FlatParams
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.Linear(5, 2))
    ref = torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.Linear(5, 2))
    ref.load_state_dict(net.state_dict())
    cls = {"rmsprop": torch.optim.RMSprop, "adam": torch.optim.Adam, "adadelta": torch.optim.Adadelta}[opt]
    kw = {"weight_decay": 5e-4, "betas": (0.5, 0.9)} if opt == "adam" else {}
    to = cls(ref.parameters(), lr=1e-3, **kw)
    for _ in range(3):
        to.zero_grad()
        ref(torch.randn(4, 6)).pow(2).sum().backward()
        to.step()
    fp = FlatParams(net, opt, betas=(0.5, 0.9))
    assert fp.state_dict()["state"] == {}                      # no step taken yet: empty, like torch
    lr = fp.load_state_dict(to.state_dict())
    assert lr == 1e-3 and fp.steps == 3
    sd = fp.state_dict()
    tsd = to.state_dict()
    assert sd["param_groups"][0].keys() == tsd["param_groups"][0].keys()
    assert sd["param_groups"][0]["params"] == tsd["param_groups"][0]["params"]
    for i, ent in tsd["state"].items():
        assert sd["state"][i].keys() == ent.keys(), (sd["state"][i].keys(), ent.keys())
        for k, v in ent.items():
            assert torch.allclose(sd["state"][i][k].float().cpu(), torch.as_tensor(v).float()), (i, k)
    fresh = cls(ref.parameters(), lr=5.0, **kw)
    fresh.load_state_dict(sd)                                  # and torch accepts what we write
    assert fresh.state_dict()["param_groups"][0]["lr"] == 1e-3
    with pytest.raises(ValueError):
        fp.load_state_dict({"state": {0: {"nope": torch.zeros(5, 6)}, 1: {}, 2: {}, 3: {}}, "param_groups": [{}]})


def test_device_state_is_per_device_not_global():
    from mpgan_amd import ops
    a, b = ops.dev_state(0), ops.dev_state(1)
    assert a is not b and a is ops.dev_state("cuda:0") and ops.dev_state("cpu").index == -1
    a.grad_into_param = True
    assert b.grad_into_param is False
    a.grad_into_param = False
    t0 = ops.next_tag(0); t1 = ops.next_tag(1); t0b = ops.next_tag(0)
    assert t0b - t0 == 8 and ops.last_tag(1) == t1 and ops.last_tag(0) == t0b
    for name in ("DEFERRED_WGRAD", "LAST_TAG", "_seed", "_tag_counter"):
        assert not hasattr(ops, name), name                    # no step state at module level
    assert "grad_into_param" not in ops.OPTIONS


def test_fused_backwards_decline_double_backward():
    """Every fused autograd Function is marked once_differentiable: a create_graph=True pass through it raises
    instead of silently dropping second-order terms (reference train.py:304-311 would do exactly that)."""
    import inspect
    from mpgan_amd import ops
    for fn in (ops.FusedMPLayerFn, ops.FusedLinearFn, ops.FusedDropoutFn, ops.FusedPackedAttnFn, ops.FusedAttnFn):
        src = inspect.getsource(fn)
        assert "@once_differentiable\n    def backward" in src, fn


def test_mab_key_mask_is_a_view_of_the_mask_it_is_given():
    """``MAB._ignore_of``: the float [B*S] key mask the attention kernels take, derived from the mask alone (nothing rides on
    the tensor).  A float contiguous [B, S] mask and the slice ``[:, :, 0]`` of a [B, S, 1] one -- what travels through a
    network pass -- come back as views (same storage: no copy, no launch); a [B, L, S] mask gives its first query row's keys;
    a bool mask its float form."""
    from mpgan_amd.gapt import MAB
    B, S, L = 3, 5, 2
    gen = torch.Generator().manual_seed(0)
    m2 = (torch.rand(B, S, generator=gen) < 0.5).float()
    got = MAB._ignore_of(m2, B, S)
    assert got.shape == (B * S,) and torch.equal(got, m2.reshape(B * S)) and got.data_ptr() == m2.data_ptr()
    m3 = (torch.rand(B, S, 1, generator=gen) < 0.5).float()
    km = m3[:, :, 0]
    got = MAB._ignore_of(km, B, S)
    assert got.shape == (B * S,) and torch.equal(got, m3.reshape(B * S)) and got.data_ptr() == km.data_ptr() == m3.data_ptr()
    mq = (torch.rand(B, 1, S, generator=gen) < 0.5).float().expand(B, L, S).contiguous()
    got = MAB._ignore_of(mq, B, S)
    assert got.shape == (B * S,) and got.is_contiguous() and torch.equal(got, mq[:, 0, :].reshape(B * S))
    mb = torch.rand(B, S, generator=gen) < 0.5
    got = MAB._ignore_of(mb, B, S)
    assert got.dtype == torch.float32 and torch.equal(got, mb.float().reshape(B * S))
    assert MAB._ignore_of(None, B, S) is None


def test_jetnet_file_reader(tmp_path):
    """JetNet's on-disk layout (particle_features [n, N, 4], jet_features [n, 4] = pt, eta, mass, num_particles) read
    from a file the test writes itself, normalised as train.py:41-67 configures JetNet: x / max + shift per particle
    feature, num_particles * (1 / num_hits) as the label, 70 / 30 train / valid split."""
    from mpgan_amd.data import JetArrayDataset, read_jetnet_file, FEATURE_MAXES, FEATURE_SHIFTS
    rs = np.random.RandomState(1)
    n, N = 40, 30
    mult = rs.randint(1, N + 1, size=n)
    pf = rs.uniform(-1, 1, size=(n, N, 4)).astype(np.float32)
    pf[..., 3] = np.arange(N)[None] < mult[:, None]
    pf[..., :3] *= pf[..., 3:]
    jf = np.stack([rs.uniform(800, 1600, n), rs.normal(0, 1, n), rs.uniform(0, 200, n), mult], axis=1).astype(np.float32)
    np.savez(tmp_path / "g.npz", particle_features=pf, jet_features=jf)
    a, b = read_jetnet_file(str(tmp_path / "g.npz"))
    assert np.array_equal(a, pf) and np.array_equal(b, jf)
    tr = JetArrayDataset.from_jetnet_file(str(tmp_path), "g", 30, split="train")
    va = JetArrayDataset.from_jetnet_file(str(tmp_path), "g", 30, split="valid")
    assert len(tr) == 28 and len(va) == 12
    x, lab = va[2]
    want = pf[30] / np.array(FEATURE_MAXES["g"], dtype=np.float32) + np.array(FEATURE_SHIFTS, dtype=np.float32)
    assert np.allclose(x.numpy(), want, atol=1e-7) and x.dtype == torch.float32
    assert float(lab) == float(np.float32(mult[30]) * np.float32(1.0 / 30))     # the product with the reciprocal
    assert int(float(lab) * 30) == mult[30]
    # a shorter particle axis takes the first (pT-ordered) particles and counts the multiplicity again
    cut = JetArrayDataset.from_jetnet_file(str(tmp_path), "g", 10, split="all")
    assert cut.particle_data.shape == (n, 10, 4)
    assert np.allclose(cut.jet_features[:, 0].numpy() * 10, np.minimum(mult, 10))
    # the 150-particle file name, a missing file, a malformed array
    np.savez(tmp_path / "t150.npz", particle_features=np.zeros((3, 150, 4), np.float32))
    assert JetArrayDataset.from_jetnet_file(str(tmp_path), "t", 150, split="all").particle_data.shape == (3, 150, 4)
    with pytest.raises(FileNotFoundError):
        JetArrayDataset.from_jetnet_file(str(tmp_path), "q", 30)
    np.savez(tmp_path / "q.npz", particle_features=np.zeros((3, 30, 3), np.float32))
    with pytest.raises(ValueError):
        JetArrayDataset.from_jetnet_file(str(tmp_path), "q", 30)


def test_flat_params_leave_frozen_parameters_alone():
    """Spectral norm's power-iteration vectors (requires_grad = False) are not part of the flat buffers, never stepped,
    and optimiser state dicts come and go in both index conventions of the reference's optimizers
    (setup_training.py:1500-1523: filtered by requires_grad, or all of module.parameters())."""
    from mpgan_amd.mpgan import LinearNet
    from mpgan_amd.train import FlatParams
    net = LinearNet([8, 6], input_size=5, output_size=2, final_linear=True, spectral_norm=True)
    names = [k for k, _ in net.named_parameters()]
    frozen = [i for i, (k, p) in enumerate(net.named_parameters()) if not p.requires_grad]
    assert frozen and all(("weight_u" in names[i]) or ("weight_v" in names[i]) for i in frozen)
    u_before = [p.detach().clone() for p in net.parameters() if not p.requires_grad]
    fp = FlatParams(net, "adam", betas=(0.5, 0.9))
    assert fp.n == sum(p.numel() for p in net.parameters() if p.requires_grad)
    assert all(p.grad is None for p in net.parameters() if not p.requires_grad)
    assert all(torch.equal(a, b) for a, b in zip(u_before, [p for p in net.parameters() if not p.requires_grad]))
    trained = [p for p in net.parameters() if p.requires_grad]
    for ref in (torch.optim.Adam(trained, lr=1e-3, weight_decay=5e-4, betas=(0.5, 0.9)),
                torch.optim.Adam(net.parameters(), lr=1e-3, weight_decay=5e-4, betas=(0.5, 0.9))):
        for p in trained:
            p.grad.fill_(0.25)
        ref.step()
        sd = ref.state_dict()
        fp.load_state_dict(sd)                                           # the reference's file, either convention
        assert fp.steps == 1.0
        filtered = len(sd["param_groups"][0]["params"]) == len(trained)
        ours = fp.state_dict(1e-3, filtered=filtered)
        assert list(ours["state"].keys()) == list(sd["state"].keys())
        for i in sd["state"]:
            assert torch.equal(ours["state"][i]["exp_avg_sq"].cpu(), sd["state"][i]["exp_avg_sq"])
        ref.load_state_dict(ours)                                        # ... and torch.optim reads ours
    with pytest.raises(ValueError):
        fp.load_state_dict({"state": {}, "param_groups": [{"params": list(range(fp._n_all + 3))}]})


def test_spectral_norm_two_forwards_before_one_backward():
    """train_D runs D(real) and D(fake) and backpropagates once (train.py:432-460): the power iteration of the second
    forward must not invalidate what autograd saved for the first."""
    from mpgan_amd.mpgan.model import SpectralNorm
    torch.manual_seed(0)
    sn = SpectralNorm(torch.nn.Linear(6, 4))
    u0 = sn.module.weight_u.detach().clone()
    w1 = sn.weight()
    w2 = sn.weight()
    (w1.sum() + (w2 * w2).sum()).backward()
    assert sn.module.weight_bar.grad is not None and bool(torch.isfinite(sn.module.weight_bar.grad).all())
    assert not torch.equal(sn.module.weight_u, u0) and not sn.module.weight_u.requires_grad
    # one power iteration as the reference does it (spectral_normalization.py:29-39)
    ref = torch.nn.Linear(6, 4)
    torch.manual_seed(0)
    sn2 = SpectralNorm(torch.nn.Linear(6, 4))
    w, u = sn2.module.weight_bar.detach(), sn2.module.weight_u.detach().clone()
    v = torch.mv(w.t(), u); v = v / (v.norm() + 1e-12)
    u = torch.mv(w, v); u = u / (u.norm() + 1e-12)
    assert torch.allclose(sn2.weight(), w / (u.dot(w.mv(v)) + 1e-12), atol=1e-7)


def test_synthetic_jet_laws_and_learning_rates_per_jet_type():
    """``bench.py --jets {g,t,q}``: the learning rates of setup_training.py:848-872 and the synthetic multiplicity laws standing in for
    the three JetNet jet types (top jets nearly fill their 30 slots, quark jets are lighter than gluon jets)."""
    import bench
    from mpgan_amd import train
    from mpgan_amd.data import synthetic_jets
    assert train.LR == {"g": (3e-5, 1e-5), "t": (6e-5, 2e-5), "q": (1.5e-5, 0.5e-5)}
    assert bench.JET_LAW == {"g": "gluon", "t": "top", "q": "quark"}
    mean = {}
    for law in ("gluon", "top", "quark", "uniform"):
        data, labels = synthetic_jets(512, 30, seed=3, dist=law)
        n = (data[..., 3] > 0).sum(1)
        assert int(n.min()) >= 1 and int(n.max()) <= 30
        assert torch.equal((labels[:, 0] * 30).round().long(), n)          # labels = multiplicity / N
        assert bool(((data[..., 3] > 0)[:, :-1] >= (data[..., 3] > 0)[:, 1:]).all())   # real particles first
        mean[law] = float(n.float().mean())
    assert mean["top"] > 27 > mean["gluon"] > mean["quark"] > mean["uniform"]


def test_packed_sets_share_one_job_layout_and_see_parameter_changes():
    """``PackedMPLayer`` / ``PackedMAB`` on CPU tensors (construction launches nothing): twelve and six pack jobs of one tuple
    length -- what ``refresh_many`` unpacks --, and a key that moves with an in-place update and with a new storage."""
    from mpgan_amd import ops
    F, out, E = 6, 8, 32
    W1, W2, W3 = torch.randn(ops.H1, 2 * F + 1), torch.randn(ops.H2, ops.H1), torch.randn(ops.H3, ops.H2)
    V1, V2, V3 = torch.randn(16, ops.H3 + F), torch.randn(16, 16), torch.randn(out, 16)
    Win, Wo, Wf = torch.randn(3 * E, E), torch.randn(E, E), torch.randn(E, E)
    for pk, n in ((ops.PackedMPLayer((W1, W2, W3, V1, V2, V3), F, out, 2.0, True), 12), (ops.PackedMAB(Win, Wo, Wf), 6)):
        jobs = pk.jobs()
        assert len(jobs) == n and {len(j) for j in jobs} == {9}
        assert set(pk.img) == set(pk._spec) and len(pk.img) == n
        for W, rows, cols, tr, scale, f16, row_split, split_cols, img in jobs:
            assert any(W is q for q in pk.params) and tr in (0, 1) and img.numel() == ops._img_elems(rows, cols)
            assert (row_split, split_cols) == (0, 0) or (row_split, split_cols) == (ops.H1, F)
        key = pk._current_key()
        assert pk._key is None and key == pk._current_key()
        last = pk.params[-1]
        last.add_(1.0)
        key2 = pk._current_key()
        assert key2 != key and key2[:-1] == key[:-1]
        pk.params[0].data = pk.params[0].data.clone()
        key3 = pk._current_key()
        assert key3 != key2 and key3[1:] == key2[1:]
    assert sum(1 for j in ops.PackedMPLayer((W1, W2, W3, V1, V2, V3), F, out, 2.0, True).jobs() if j[6]) == 2   # W1S, W1ST


def test_deferred_targets_only_inside_a_collecting_backward_with_every_target():
    """``ops._deferred_targets``: the ``.grad`` targets in order plus the batch while ``grad_into_param`` is on, a batch is
    collecting and EVERY parameter has a target; None otherwise."""
    from mpgan_amd import ops
    st = ops.DeviceState(-1)
    W = torch.nn.Parameter(torch.randn(6, 4))
    b = torch.nn.Parameter(torch.randn(6))
    bare = torch.nn.Parameter(torch.randn(3))          # no .grad buffer
    W.grad, b.grad = torch.zeros_like(W), torch.zeros_like(b)
    batch = object()
    assert ops._deferred_targets(st, [W, b]) is None                       # nothing switched on
    st.deferred_wgrad = batch
    assert ops._deferred_targets(st, [W, b]) is None                       # grad_into_param off
    st.grad_into_param, st.deferred_wgrad = True, None
    assert ops._deferred_targets(st, [W, b]) is None                       # no batch
    st.deferred_wgrad = batch
    assert ops._deferred_targets(st, [W, bare]) is None                    # one parameter without a target
    assert ops._deferred_targets(st, [W, None]) is None
    targets, got = ops._deferred_targets(st, [W, b])
    assert got is batch and len(targets) == 2 and targets[0] is W.grad and targets[1] is b.grad
    rows = W[2:5]                                                          # a row slice of a leaf: the matching view of its .grad
    (t,), _ = ops._deferred_targets(st, [rows])
    assert t.shape == (3, 4) and t.data_ptr() == W.grad[2:5].data_ptr()
    assert ops._deferred_targets(st, [b, W])[0][0] is b.grad


def test_param_grads_queue_only_inside_a_collecting_backward_with_every_target():
    """``ops.ParamGrads`` queues -- the ``.grad`` targets in order plus the batch -- while ``grad_into_param`` is on, a batch is
    collecting and EVERY wanted parameter has a target; not otherwise."""
    from mpgan_amd import ops
    st = ops.DeviceState(-1)
    W = torch.nn.Parameter(torch.randn(6, 4))
    b = torch.nn.Parameter(torch.randn(6))
    bare = torch.nn.Parameter(torch.randn(3))          # no .grad buffer
    W.grad, b.grad = torch.zeros_like(W), torch.zeros_like(b)
    batch = object()

    def queued(params):
        pg = ops.ParamGrads(st, params, (True,) * len(params))
        assert (pg.batch is None) or (pg.targets is not None)     # (a batch only ever beside every target)
        return None if pg.batch is None else (pg.targets, pg.batch)
    assert queued([W, b]) is None                       # nothing switched on
    st.deferred_wgrad = batch
    assert queued([W, b]) is None                       # grad_into_param off
    st.grad_into_param, st.deferred_wgrad = True, None
    assert queued([W, b]) is None                       # no batch
    st.deferred_wgrad = batch
    assert queued([W, bare]) is None                    # one parameter without a target
    assert queued([W, None]) is None
    targets, got = queued([W, b])
    assert got is batch and len(targets) == 2 and targets[0] is W.grad and targets[1] is b.grad
    rows = W[2:5]                                                          # a row slice of a leaf: the matching view of its .grad
    (t,), _ = queued([rows])
    assert t.shape == (3, 4) and t.data_ptr() == W.grad[2:5].data_ptr()
    assert queued([b, W])[0][0] is b.grad


class _RecordingBatch:
    """Stands in for ``ops.WgradBatch``: keeps the arguments of every ``add``."""

    def __init__(self):
        self.jobs = []

    def add(self, dy, x, **kw):
        self.jobs.append((dy, x, kw))


def _route(pg):
    # which way the gradients of one ``ops.ParamGrads`` go, read off its decision
    if not any(pg.wanted):
        return "none"
    return "returned" if pg.targets is None else "direct" if pg.batch is None else "queued"


def _linear_params(with_b=True, grads=True):
    W = torch.nn.Parameter(torch.randn(6, 4))
    b = torch.nn.Parameter(torch.randn(6)) if with_b else None
    if grads:
        W.grad = torch.zeros_like(W)
        if with_b:
            b.grad = torch.zeros_like(b)
    return W, b


@pytest.mark.parametrize("flag", [False, True])
@pytest.mark.parametrize("has_batch", [False, True])
@pytest.mark.parametrize("grads", [False, True])
@pytest.mark.parametrize("with_b", [False, True])
def test_param_grads_decision_table(flag, has_batch, grads, with_b):
    """The route of ``ops.ParamGrads`` for every combination of (flag, batch present, targets present, b is None), and nothing
    wanted; ``written`` and ``slots`` on each: None for autograd exactly where the gradient goes into .grad."""
    from mpgan_amd import ops
    st = ops.DeviceState(-1)
    st.grad_into_param, st.deferred_wgrad = flag, (_RecordingBatch() if has_batch else None)
    W, b = _linear_params(with_b, grads)
    wanted = (True, with_b)                               # (as DiscHeadFn asks: a head without bias has one target)
    pg = ops.ParamGrads(st, (W, b), wanted)
    expect = "returned" if not (flag and grads) else "queued" if has_batch else "direct"
    assert _route(pg) == expect
    fresh = (torch.empty(6, 4), torch.empty(6) if with_b else None)
    (tw, tb), acc = pg.written(lambda: fresh)
    if expect == "returned":
        assert acc == 0 and tw is fresh[0] and tb is fresh[1]
        assert pg.slots()[0] is fresh[0] and pg.slots()[1] is fresh[1]
    else:                                                 # (a kernel that writes the gradients itself adds into .grad, batch or not)
        assert acc == 1 and tw is W.grad and (tb is b.grad if with_b else tb is None)
        assert pg.slots() == (None, None)
    # nothing wanted: no target is looked up, nothing is allocated, nothing is returned -- a frozen norm's .grad stays as it is
    calls = []
    none = ops.ParamGrads(st, (W, b), (False, False))
    assert _route(none) == "none" and none.targets is None and none.batch is None
    assert none.written(lambda: calls.append(1)) == ([None, None], 0) and not calls and none.slots() == (None, None)
    none.gemm(0, 1, None, None)
    none.colsum(1, None)
    assert none.slots() == (None, None) and (not has_batch or not st.deferred_wgrad.jobs)
    # a wanted parameter that is None has no target: returned, whatever is switched on (FusedMABFn's seed row that is no leaf)
    assert _route(ops.ParamGrads(st, (None,), (True,))) == "returned"
    # ``eligible``: what else a node needs (FusedMPLayerFn: its PackedMPLayer knows the twelve Parameters)
    assert _route(ops.ParamGrads(st, (W, b), wanted, eligible=False)) == "returned"


def test_param_grads_queued_jobs_and_autograd_slots():
    """The jobs ``gemm`` and ``colsum`` add on the queued route -- with and without bias, a row block, ``out_col0``, a column
    sum -- and the tuple autograd gets: None for everything queued."""
    from mpgan_amd import ops
    st = ops.DeviceState(-1)
    st.grad_into_param, st.deferred_wgrad = True, _RecordingBatch()
    jobs = st.deferred_wgrad.jobs
    W, b = _linear_params()
    dy, x = torch.randn(9, 6), torch.randn(9, 4)
    pg = ops.ParamGrads(st, (W, b), (True, True))
    pg.gemm(0, 1, dy, x)
    assert len(jobs) == 1 and jobs[0][0] is dy and jobs[0][1] is x
    kw = jobs[0][2]
    assert sorted(kw) == ["accumulate", "bias_out", "out", "out_col0"]
    assert kw["out"] is W.grad and kw["bias_out"] is b.grad and kw["out_col0"] == 0 and kw["accumulate"] is True
    assert pg.slots() == (None, None)
    pg = ops.ParamGrads(st, (W, b), (True, False))         # the bias is not wanted: no bias_out, no target looked up for it
    pg.gemm(0, 1, dy, x[:, :2], col0=2)
    assert jobs[1][2]["out"] is W.grad and jobs[1][2]["bias_out"] is None and jobs[1][2]["out_col0"] == 2 and jobs[1][2]["accumulate"] is True
    assert pg.targets[1] is None and pg.slots() == (None, None)
    pg = ops.ParamGrads(st, (W, b), (True, True))          # a row block (cross-attention's Win[:E] / Win[E:]): the same rows of both targets
    pg.gemm(0, 1, dy[:, :2], x, rows=slice(4, None))
    kw = jobs[2][2]
    assert kw["out"].shape == (2, 4) and kw["out"].data_ptr() == W.grad[4:].data_ptr()
    assert kw["bias_out"].shape == (2,) and kw["bias_out"].data_ptr() == b.grad[4:].data_ptr() and kw["accumulate"] is True
    pg = ops.ParamGrads(st, (W, b), (False, True))         # a bias alone rides in no GEMM: summed at once and returned
    pg.gemm(0, 1, dy, x)
    assert len(jobs) == 3 and pg.slots()[0] is None and torch.equal(pg.slots()[1], dy.sum(0))
    # a column sum: the bias-sum job -- a one-column GEMM into a throw-away out, the sums into the flattened target
    g = torch.nn.Parameter(torch.randn(1, 1, 6))
    g.grad = torch.zeros_like(g)
    rows = torch.randn(9, 6)
    pg = ops.ParamGrads(st, (g,), (True,))
    pg.colsum(0, rows)
    dy4, x4, kw = jobs[3]
    assert dy4 is rows and x4.shape == (9, 1) and x4.data_ptr() == rows.data_ptr() and x4.stride() == rows[:, :1].stride()
    assert kw["out"].shape == (6, 1) and kw["bias_out"].shape == (6,) and kw["bias_out"].data_ptr() == g.grad.data_ptr()
    assert kw["accumulate"] is True and pg.slots() == (None,)
    # not queued (no batch): summed here and returned, whatever the flag says
    st.deferred_wgrad = None
    pg = ops.ParamGrads(st, (g,), (True,))
    pg.colsum(0, rows)
    assert torch.equal(pg.slots()[0], rows.sum(0)) and not g.grad.any()


@pytest.mark.parametrize("switches", ["1", "0"])
def test_cpu_and_gradient_penalty_steps_take_the_module_route(monkeypatch, switches):
    """``TrainStep._route()`` names how the generator's jets reach the discriminator.  A step on the CPU (toy modules) and a
    step with a gradient penalty -- whose D(interpolated) needs the modules' own graph -- go by the plain modules with a torch
    loss, whatever the route switches say; the switches are read when the step is built, never after."""
    from mpgan_amd import train
    from test_dist_cpu import ToyG, ToyD, ToyD2, N as TN, LAT
    for name in ("MPG_PARTS", "MPG_BRIDGE", "MPG_GEN_AHEAD", "MPG_GEN_AHEAD_LATE", "MPG_WGRAD_SIDE", "MPG_NOISE_MASK"):
        monkeypatch.setenv(name, switches)
    monkeypatch.delenv("MPG_SPLIT_GRAPHS", raising=False)
    torch.manual_seed(3)
    plain = train.TrainStep(ToyG(), ToyD(), 4, TN, latent=LAT, use_graphs=False)
    gp = train.TrainStep(ToyG(), ToyD2(), 4, TN, latent=LAT, use_graphs=False, loss="w", gp_lambda=10.0)
    for ts in (plain, gp):
        assert ts._route() == "module" and ts._route(rows_ok=False) == "module"
        assert not ts._bridge() and not ts._fused_ends()
        # nothing of the device-only arrangements is on for a CPU step, and there is no branch to join
        assert not (ts.parts or ts.gen_ahead or ts.gen_ahead_late or ts.wgrad_side or ts.bridge or ts.noise_mask)
        assert ts.gen_join is None and ts.split_graphs is False
    # sampled at construction: the environment changing afterwards reaches nothing
    monkeypatch.setenv("MPG_SPLIT_GRAPHS", "1")
    assert plain.split_graphs is False
    assert train.TrainStep(ToyG(), ToyD(), 4, TN, latent=LAT, use_graphs=False).split_graphs is True


# ---- the fused MPLayer's host path (ops.FusedMPLayerFn): descriptors, plan and dx layer from CPU tensors, nothing launched
def _mp_call(B, N, F, extras, thr):
    """An ``ops.MPCall`` over CPU tensors as ``FusedMPLayerFn.forward`` would save them, with its gradient buffers: (call, dh0, bufs)."""
    import ctypes as C
    from mpgan_amd import ops
    H1, H2, H3 = ops.H1, ops.H2, ops.H3
    V, RB, nq = B * N, (N + 31) // 32, 2 if extras else 0
    f = lambda *s: torch.zeros(s)
    W1, W2, W3, V1, V2, V3 = f(H1, 2 * F + nq), f(H2, H1), f(H3, H2), f(64, H3 + F), f(48, 64), f(F, 48)
    pk = ops.PackedMPLayer((W1, W2, W3, V1, V2, V3), F, F, 2.0 if thr else 1.0, True)
    sv = ops.MPLayerSaved(
        x2=f(V, F), m1=f(V), ac=f(V, 2 * H1), agg=f(V, H3), h1=f(V, 64), h2=f(V, 48), W1=W1, b2=f(H2), b3=f(H3), W2=W2, W3=W3,
        V1=V1, V2=V2, V3=V3, sign3=torch.zeros(B * RB * N * 192, dtype=torch.int32), nbr=torch.zeros(V, 8, dtype=torch.int32) if extras else None,
        stE2=torch.zeros(B * RB * N, H2, 32, dtype=torch.float16), es=f(B, N, ops.EDGE_SCALARS, N) if extras else None,
        wq=f(ops.EDGE_SCALARS, H1) if extras else None, xf2=f(V, F), order=torch.zeros(B, dtype=torch.int32) if extras else None)
    cfg = ops.MPLayerCfg(B, N, F, 0.125, 0.25, thr, 2.0 if thr else 1.0, 7 if thr else 0, 2 if extras else 1, True, nq)
    call = ops.MPCall(sv, cfg, pk, torch.zeros(1, dtype=torch.int64))
    return call, f(V, H3 + F), ops._edge_grad_bufs(call, True)


@pytest.mark.parametrize("extras,thr", [(True, 128), (False, 0)])
def test_mplayer_edge_descriptors_agree(extras, thr):
    """Every field that two or three of MpgEdgeFwd / MpgEdgeBwd / MpgEdgeDw have carries the same value in each, and the shared
    fields are what the call holds: with k-NN sets, edge scalars and dropout, and with none of them."""
    from mpgan_amd import ops, _lib
    B, N, F = 3, 40, 8
    call, dh0, bufs = _mp_call(B, N, F, extras, thr)
    sv, cfg, pk, seed_t = call
    tg = ops.MPGradTargets(*(torch.zeros(3) for _ in range(12)), direct=True)
    descs = {"fwd": ops._edge_fwd_desc(call, torch.zeros(cfg.SC, B * N, ops.H3)), "bwd": ops._edge_bwd_desc(call, dh0, bufs),
             "dw": ops._edge_dw_desc(call, dh0, bufs, tg, torch.zeros(5, 7))}
    fields = {k: [f[0] for f in type(d)._fields_] for k, d in descs.items()}
    shared = {n for a in fields for b in fields if a < b for n in set(fields[a]) & set(fields[b])}
    ptr = lambda t, off=0: None if t is None else t.data_ptr() + 4 * off
    want = dict(a=ptr(sv.ac), c=ptr(sv.ac, ops.H1), ld_ac=2 * ops.H1, mask=ptr(sv.m1), B=B, N=N, alpha=0.25, agg_scale=0.125,
                nbr=ptr(sv.nbr), seed=ptr(seed_t), tag_base=cfg.tag, thr=thr, dscale=cfg.dscale, f16=1, es=ptr(sv.es), wq=ptr(sv.wq),
                dagg=ptr(dh0), ld_dagg=dh0.stride(0), sign3=ptr(sv.sign3), stageE2=ptr(sv.stE2), stageZ2=ptr(bufs.stZ2), gexp=ptr(bufs.gexp))
    assert set(want) <= shared, sorted(set(want) - shared)
    assert (want["nbr"] is not None) == extras and (want["es"] is not None) == extras
    for name in sorted(shared):
        vals = {k: getattr(d, name) for k, d in descs.items() if name in fields[k]}
        assert len(vals) >= 2 and len(set(vals.values())) == 1, (name, vals)
        if name in want:
            assert next(iter(vals.values())) == want[name], (name, vals, want[name])


def test_mplayer_edge_plan(monkeypatch):
    from mpgan_amd import ops
    monkeypatch.delenv("MPG_FORCE_SC", raising=False)
    on = dict(ops.OPTIONS, fn_epilogue=True, fn_chunks=True, lpt_order=True)
    p = ops.edge_plan(256, 30, need_grad=True, options=on)
    assert (p.SC, p.RB, p.epilogue, p.tickets, p.lpt, p.write_agg) == (1, 1, True, False, False, True)
    assert not ops.edge_plan(256, 30, mask=True, options=on).lpt      # (every CU has one workgroup: nothing to order)
    assert ops.edge_plan(512, 30, mask=True, options=on).lpt and not ops.edge_plan(512, 30, mask=False, options=on).lpt
    p = ops.edge_plan(16, 150, need_grad=True, options=on)
    assert (p.SC, p.RB, p.epilogue, p.tickets, p.write_agg) == (3, 5, True, True, True)
    assert ops.edge_plan(16, 150, need_grad=False, options=on).write_agg   # (the chunks' partial sums travel through agg)
    p = ops.edge_plan(2, 30, es=True, options=on)
    assert not p.epilogue and -(-30 // p.SC) <= ops.MAX_CHUNK_SENDERS_ES
    assert -(-150 // ops.edge_plan(1, 150, es=True, options=on).SC) <= ops.MAX_CHUNK_SENDERS_ES
    p = ops.edge_plan(256, 30, need_grad=False, options=on)
    assert p.SC == 1 and p.epilogue and not p.write_agg
    assert not ops.edge_plan(256, 30, options=dict(on, fn_epilogue=False)).epilogue
    assert not ops.edge_plan(16, 150, options=dict(on, fn_chunks=False)).epilogue
    assert ops.edge_plan(256, 30, options=dict(on, fn_chunks=False)).epilogue
    saved = ops.OPTIONS["fn_epilogue"]
    try:   # (without ``options``: the module's switches as they are at the call)
        ops.OPTIONS["fn_epilogue"] = False
        assert not ops.edge_plan(256, 30).epilogue
        ops.OPTIONS["fn_epilogue"] = True
        assert ops.edge_plan(256, 30).epilogue
    finally:
        ops.OPTIONS["fn_epilogue"] = saved
    monkeypatch.setenv("MPG_FORCE_SC", "1")
    p = ops.edge_plan(16, 150, options=on)
    assert p.SC == 1 and not p.tickets
    monkeypatch.setenv("MPG_FORCE_SC", "2")
    assert ops.edge_plan(256, 30, options=on).SC == 2


def test_mplayer_park_limit_raises_before_anything_runs():
    """32-bit offsets into the parked fragments: with a backward pending N = 30 takes 0x7fffffff // (1 * 30 * 10240) = 6990 jets."""
    from mpgan_amd import ops
    assert 0x7fffffff // (1 * 30 * ops.PARK_BYTES_PER_BLOCK) == 6990
    ops.edge_plan(6990, 30, need_grad=True)
    with pytest.raises(RuntimeError, match="at most 6990 jets"):
        ops.edge_plan(6991, 30, need_grad=True)
    ops.edge_plan(6991, 30, need_grad=False)


def test_mplayer_dx_layer_is_one_definition():
    """The dx chain's three feeds describe the same layer; only where its [da | dc] rows come from differs."""
    from mpgan_amd import ops
    H1, H3 = ops.H1, ops.H3
    B, N, F = 3, 40, 8
    call, dh0, bufs = _mp_call(B, N, F, False, 0)
    V = B * N
    dx, dadc = torch.zeros(V, F), torch.zeros(V, 2 * H1)
    da, dc = bufs.dap[0], bufs.dcp[0]
    chains = [ops._dx_chain(call, dh0, dx, bufs.dap, bufs.dcp), ops._dx_chain(call, dh0, dx, dadc), ops._dx_chain(call, dh0, dx, da, dc)]
    feeds = [(bufs.dap.data_ptr(), H1, H1, bufs.dcp.data_ptr(), H1), (dadc.data_ptr(), 2 * H1, 2 * H1, None, 0),
             (bufs.dap.data_ptr(), H1, H1, dc.data_ptr(), dc.stride(0))]
    for c, feed in zip(chains, feeds):
        assert (c.A, c.lda, c.K1, c.A2, c.lda2) == feed
        L = c.L[0]
        assert (c.M, c.nlayers, c.f16, c.alpha, c.seed) == (V, 1, 0, 0.25, None)
        assert (L.Wimg, L.K, L.N) == (call.pk.img["W1ST"].data_ptr(), 2 * H1, F)
        assert (L.resid, L.ldr, L.out, L.ldo) == (dh0.data_ptr() + 4 * H3, dh0.stride(0), dx.data_ptr(), F)
        assert (L.bias, L.act, L.gateH, L.drop_thr) == (None, 0, None, 0)
