"""GPU: the one-launch batch feed (csrc/loader.hip) against ``TrainStep.set_batch`` bit for bit, and ``TrainStep(loader=...)``
captured, eager, resumed and against the hand-fed step.  Parameter comparisons run with D's dropout off and fixed noise, as the
eager-against-captured tests of test_gpu_train.py do (dropout sites are numbered in host order, which a capture's warm-up
moves): everything else of an iteration is deterministic, so the bar is bit equality."""
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu


def _jets(n, N, seed=1):
    from mpgan_amd.data import synthetic_jets
    return synthetic_jets(n, N, seed=seed, dist="uniform")


def _buffers(B, N, fill=-7.0):
    """TrainStep's batch buffers, filled with a value no jet holds (a row the launch should not write stays visible)."""
    dev = "cuda"
    f = lambda *s: torch.full(s, fill, device=dev)
    return SimpleNamespace(B=B, loader=None, data=f(B, N, 4), labels=f(B, 1), _dcat=f(2 * B, N, 4), _labels2=f(2 * B, 1),
                           _x3=f(2 * B, N, 3), _mask2=f(2 * B, N, 1), _ign2=f(2 * B, N))


NAMES = ("data", "labels", "_dcat", "_labels2", "_x3", "_mask2", "_ign2")


@pytest.mark.parametrize("n,N,B,launches,rank,world,drop", [
    (37, 30, 8, 6, 0, 1, ()),                # batches straddle the epoch boundary; the cursor advances by itself
    (37, 30, 8, 3, 1, 2, ()),                # a rank's slice: starts at B, strides by 2B
    (5, 30, 8, 3, 0, 1, ()),                 # n < B: a batch is longer than an epoch
    (9, 150, 4, 3, 0, 1, ("data", "_x3", "_labels2")),   # five lanes' worth of particles per lane pair; some destinations NULL
    (3, 1, 2, 3, 0, 1, ()),
    (70, 33, 9, 2, 0, 1, ("_dcat", "labels")),           # first N on the one-jet-per-wave path; B no multiple of a workgroup's jets
])
def test_feed_equals_set_batch_bit_for_bit(n, N, B, launches, rank, world, drop):
    from mpgan_amd import train
    from mpgan_amd.data import DeviceJetLoader
    particles, labels = _jets(n, N)
    loader = DeviceJetLoader((particles, labels), B, "cuda", seed=11, rank=rank, world_size=world)
    assert loader.position == rank * B
    want, got = _buffers(B, N), _buffers(B, N)
    for name in drop:
        setattr(got, name, None)
    for k in range(launches):
        idx = loader.indices(k)
        assert idx.shape == (B,) and int(idx.min()) >= 0 and int(idx.max()) < n
        train.TrainStep.set_batch(want, particles[idx].cuda(), labels[idx].cuda())
        loader.feed(got)
        torch.cuda.synchronize()
        assert int(loader._ticket.item()) == 0, k                       # the arrival counter is left as it was found
        assert loader.position == rank * B + (k + 1) * world * B, k      # ... and the cursor moved by the stride
        for name in NAMES:
            if name in drop:
                continue
            a, b = getattr(got, name), getattr(want, name)
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (name, k)   # (bits: -0.0 and 0.0 differ)
    assert loader.epoch == loader.position // n


def test_entry_point_refuses_what_the_header_says():
    import ctypes as C
    from mpgan_amd import _lib
    L = _lib.lib()
    x, l = torch.zeros(3, 2, 4, device="cuda"), torch.zeros(3, device="cuda")
    cur, tk = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    out = torch.zeros(2, 2, 4, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    args = lambda **kw: [kw.get("x", p(x)), p(l), kw.get("n", 3), kw.get("N", 2), 1, kw.get("cur", p(cur)), p(tk), kw.get("B", 2), 2,
                         p(out), None, None, None, None, None, None, None]
    for bad in (dict(n=0), dict(B=0), dict(N=0), dict(cur=None), dict(x=None)):
        assert L.mpg_batch_feed(*args(**bad)) == -1, bad
    assert L.mpg_batch_feed(*args(x=C.c_void_p(x.data_ptr() + 4))) == -2
    torch.cuda.synchronize()
    assert int(cur.item()) == 0 and int(tk.item()) == 0 and not bool(out.any())


# ---- the training step with a loader ----------------------------------------------------------------------------------------
B_, N_, n_ = 4, 30, 10


def _nets():
    from oracle import train_ref as T
    from mpgan_amd import train
    G, D = train.default_mpgan(N_, disc_dropout=0.0)
    G.load_state_dict(T.init_state_dict(T.mpgan_param_shapes(True), 41, torch.float32))
    D.load_state_dict(T.init_state_dict(T.mpgan_param_shapes(False), 42, torch.float32))
    return G, D


def _step(G, D, loader, use_graphs=True):
    from mpgan_amd import train
    ts = train.TrainStep(G, D, B_, N_, use_graphs=use_graphs, loader=loader)
    gen = torch.Generator(device="cuda").manual_seed(5)
    ts.fixed_noise = (torch.randn(B_, N_, 32, device="cuda", generator=gen) * 0.2,
                      torch.randn(B_, N_, 32, device="cuda", generator=gen) * 0.2)
    return ts


def _params(ts):
    torch.cuda.synchronize()
    return ts.fD.flat.clone(), ts.fG.flat.clone()


@pytest.fixture(scope="module")
def run():
    """ONE captured run of eight iterations with the loader (default capture: three warm-up iterations, which must consume no
    jets); what the tests below compare against: the batch buffers after every step, the parameters after steps 4, 5 and 8, and
    everything a resume needs after step 5."""
    from mpgan_amd.data import DeviceJetLoader
    particles, labels = _jets(n_, N_, seed=3)
    G, D = _nets()
    loader = DeviceJetLoader((particles, labels), B_, "cuda", seed=21)
    ts = _step(G, D, loader)
    r = SimpleNamespace(particles=particles, labels=labels, key_seed=21, data=[], x3=[], lab=[], idx=[], params={}, loader=loader, ts=ts)
    for step in range(8):
        ts.step()
        torch.cuda.synchronize()
        r.data.append(ts.data.clone()); r.x3.append(ts._x3[:B_].clone()); r.lab.append(ts.labels.clone())
        r.idx.append(loader.indices(step))
        if step + 1 in (4, 5, 8):
            r.params[step + 1] = _params(ts)
        if step + 1 == 5:
            r.position5 = loader.position
            clone = lambda sd: {k: v.clone() for k, v in sd.items()}
            r.saved = (loader.state_dict(), ts.optimizer_state_dicts(), clone(G.state_dict()), clone(D.state_dict()))
    assert len(ts._graphs) == 1
    return r


def test_captured_iteration_feeds_itself(run):
    for step in range(8):
        idx = run.idx[step]
        assert torch.equal(run.data[step].cpu(), run.particles[idx]), step
        assert torch.equal(run.x3[step].cpu(), run.particles[idx][..., :3]), step
        assert torch.equal(run.lab[step].cpu(), run.labels[idx]), step
    assert run.position5 == 5 * B_ and run.loader.position == 8 * B_ and run.loader.epoch == 3
    with pytest.raises(RuntimeError):
        run.ts.attach_loader(run.loader)            # (captured: the feed launch is part of the graph)
    with pytest.raises(RuntimeError):
        run.ts.set_batch(run.data[0], run.lab[0])


def test_eager_equals_captured(run):
    from mpgan_amd.data import DeviceJetLoader
    G, D = _nets()
    loader = DeviceJetLoader((run.particles, run.labels), B_, "cuda", seed=run.key_seed)
    ts = _step(G, D, loader, use_graphs=False)
    for _ in range(5):
        ts.step()
    fD, fG = _params(ts)
    assert torch.equal(fD, run.params[5][0]) and torch.equal(fG, run.params[5][1])
    assert torch.equal(ts.data, run.data[4]) and loader.position == 5 * B_


def test_resume_equals_the_uninterrupted_run(run):
    from mpgan_amd.data import DeviceJetLoader
    sd_loader, (sd_D, sd_G), g_state, d_state = run.saved
    G, D = _nets()
    G.load_state_dict(g_state); D.load_state_dict(d_state)
    loader = DeviceJetLoader((run.particles, run.labels), B_, "cuda", seed=99)     # (another key: the saved one takes over)
    loader.load_state_dict(sd_loader)
    ts = _step(G, D, loader)
    ts.load_optimizer_state_dicts(sd_D, sd_G)
    for step in range(5, 8):
        ts.step()
        torch.cuda.synchronize()
        assert torch.equal(ts.data, run.data[step]), step
    fD, fG = _params(ts)
    assert torch.equal(fD, run.params[8][0]) and torch.equal(fG, run.params[8][1])
    assert loader.position == 8 * B_
    with pytest.raises(RuntimeError):               # another key cannot reach the captured launch
        loader.load_state_dict(dict(sd_loader, key=sd_loader["key"] ^ 1))


def test_loader_equals_the_hand_fed_step(run):
    """The old way in -- ``set_batch`` of the same rows before every step -- gives the same parameters bit for bit."""
    G, D = _nets()
    ts = _step(G, D, None)
    for step in range(4):
        idx = run.idx[step]
        ts.set_batch(run.particles[idx].cuda(), run.labels[idx].cuda())
        ts.step()
    fD, fG = _params(ts)
    assert torch.equal(fD, run.params[4][0]) and torch.equal(fG, run.params[4][1])


def test_gapt_captured_iteration_feeds_itself():
    """The default GAPT step (dropout on, the one-launch bridge between the networks), captured."""
    from mpgan_amd import train
    from mpgan_amd.data import DeviceJetLoader
    particles, labels = _jets(n_, N_, seed=4)
    torch.manual_seed(0)
    G, D = train.default_gapt(N_)
    loader = DeviceJetLoader((particles, labels), B_, "cuda", seed=8)
    ts = train.TrainStep(G, D, B_, N_, latent=64, lr_disc=train.LR_GAPT[0], lr_gen=train.LR_GAPT[1], loader=loader)
    for step in range(5):
        ts.step()
        torch.cuda.synchronize()
        idx = loader.indices(step)
        assert torch.equal(ts.data.cpu(), particles[idx]) and torch.equal(ts._x3[:B_].cpu(), particles[idx][..., :3]), step
        assert torch.equal(ts._labels2.cpu(), torch.cat([labels[idx], labels[idx]])), step
        assert bool(torch.isfinite(ts.D_loss)) and bool(torch.isfinite(ts.G_loss))
    assert ts._graphs is not None and loader.position == 5 * B_
