"""GPU: the averaged generator -- the three ``mpg_*_ema`` launches against the numpy restatement of tests/test_ema_cpu.py bit for bit
(and everything else they write against the launches without the average), and ``TrainStep(ema=Ema(...))``: the average after
every step against the fold of the weights' own snapshots, the step without the option unchanged, captured against eager, the
num_critic schedule, resume, and the twin module of ``ema_generator()`` with its packed weight images.  The reference has no
averaged generator: the restatement of include/mpgan_amd.h is the specification."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from test_ema_cpu import F32, bits, mixed, restate
from test_gpu_schedule import N, RAN, _device_seed, _step

pytestmark = pytest.mark.gpu

SEED_STEP = 0x9E3779B97F4A7C15        # (any odd 64-bit stride: the launch adds what it is given)


def _words(t):
    return torch.tensor([t, 0], dtype=torch.int64).to(torch.uint32).cuda()


def _t(state):
    torch.cuda.synchronize()
    return state.cpu().tolist()


def _same(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Bit for bit (a NaN equals itself, +0 differs from -0)."""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    as_int = {4: torch.int32, 8: torch.int64}[a.element_size()]
    return torch.equal(a.view(as_int), b.view(as_int))


# ---- 1. one launch ----------------------------------------------------------------------------------------------------------------
class _Bufs:
    """p, g and the optimizer's moments of one flat buffer of n values, the seed word and Adam's step count."""

    def __init__(self, n, seed):
        self.n = n
        self.p = torch.from_numpy(mixed(n, seed)).cuda()
        self.v = torch.from_numpy(np.abs(mixed(n, seed + 1))).cuda()
        self.aux = torch.from_numpy(np.abs(mixed(n, seed + 2)) * F32(1e-3)).cuda()
        self.g = torch.zeros(n, device="cuda")
        self.count = torch.full((), 2.0, device="cuda")
        self.seed = torch.tensor([12345], dtype=torch.int64, device="cuda")

    def launch(self, opt, grad, block=None):
        from mpgan_amd import _lib
        L = _lib.lib()
        self.g.copy_(grad)
        vp = lambda t: C.c_void_p(t.data_ptr())
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        tail = (st,) if block is None else (C.byref(block), st)
        if opt == "rmsprop":
            args = (vp(self.p), vp(self.g), vp(self.v), self.n, 1e-2, 0.99, 1e-8, 0.5, 1, vp(self.seed), SEED_STEP)
        elif opt == "adam":
            args = (vp(self.p), vp(self.g), vp(self.aux), vp(self.v), vp(self.count), self.n, 1e-2, 0.9, 0.999, 1e-8, 5e-4, 0.5, 1,
                    vp(self.seed), SEED_STEP)
        else:
            args = (vp(self.p), vp(self.g), vp(self.v), vp(self.aux), self.n, 1.0, 0.9, 1e-6, 0.5, 1, vp(self.seed), SEED_STEP)
        name = "mpg_" + opt + ("" if block is None else "_ema")
        _lib.check(getattr(L, name)(*args, *tail), name)

    def all(self):
        return [self.p, self.g, self.v, self.aux, self.count, self.seed]


# (t before the first launch, beta, start, warmup): from the start without warm-up; across t = start - 1 -> start + 1 with it
RUNS = [(0, 0.999, 0, False), (1, 0.9, 2, True)]


# (one workgroup, its edges, two; the first size at which a thread of the averaged launch -- at most 256 workgroups -- takes a second
# element; beyond the grid cap of the launch without the average as well, where its stride loop runs twice)
@pytest.mark.parametrize("n", [1, 255, 256, 257, 256 * 256 + 1, 2048 * 256 + 3])
@pytest.mark.parametrize("opt", ["rmsprop", "adam", "adadelta"])
def test_one_launch_against_the_restatement(opt, n):
    from mpgan_amd import _lib
    for t0, beta, start, warmup in RUNS:
        with_avg, without = _Bufs(n, 7 * n), _Bufs(n, 7 * n)
        e0 = mixed(n, 3 * n + 1)
        ema, state = torch.from_numpy(e0).cuda(), _words(t0)
        block = _lib.MpgEma(C.c_void_p(ema.data_ptr()), C.c_void_p(state.data_ptr()), beta, start, int(warmup))
        want = e0
        for k in range(3):       # three consecutive launches on one state
            grad = torch.from_numpy(mixed(n, 100 * k + n)).cuda()
            with_avg.launch(opt, grad, block)
            without.launch(opt, grad)
            assert _t(state) == [t0 + k + 1, 0], (k, _t(state))                  # t moved by exactly one, the ticket reads 0
            for name, a, b in zip(("p", "g", "v", "aux", "count", "seed"), with_avg.all(), without.all()):
                assert _same(a, b), (k, name)                                   # the launch without the average, bit for bit
            assert int(with_avg.seed) % (1 << 64) == (12345 + (k + 1) * SEED_STEP) % (1 << 64)      # (the seed word, moved on)
            assert float(with_avg.g.abs().max()) == 0.0
            want = restate(want, with_avg.p.cpu().numpy(), t0 + k, F32(beta), start, warmup)    # fed with the launch's own p
            got = ema.cpu().numpy()
            assert np.array_equal(bits(got), bits(want)), (t0, k, int((bits(got) != bits(want)).sum()))
        assert not np.array_equal(bits(want), bits(with_avg.p.cpu().numpy()))      # (an average, not a copy)


def test_launch_argument_checks():
    """What tests/test_ema_cpu.py refuses comes back before the launch here as well: nothing is written."""
    from mpgan_amd import _lib
    b = _Bufs(16, 1)
    before = [t.clone() for t in b.all()]
    ema, state = torch.zeros(16, device="cuda"), _words(0)
    for kw in (dict(beta=1.0), dict(beta=float("nan")), dict(start=-1)):
        block = _lib.MpgEma(**dict(dict(ema=ema.data_ptr(), state=state.data_ptr(), beta=0.5, start=0, warmup=0), **kw))
        with pytest.raises(RuntimeError):
            b.launch("rmsprop", torch.ones(16, device="cuda"), block)
    b.g.zero_()
    assert all(_same(x, y) for x, y in zip(b.all(), before)) and _t(state) == [0, 0] and float(ema.abs().max()) == 0.0


# ---- 2. the step ------------------------------------------------------------------------------------------------------------------
B = 4


def _ema_step(model="mpgan", ema="default", **kw):
    from mpgan_amd.step_options import Ema
    kw.setdefault("use_graphs", False)
    return _step(model, B, ema=Ema(beta=0.9) if ema == "default" else ema, **kw)


def _fold(snapshots, e0, beta, start=0, warmup=False, t0=0):
    e = e0
    for k, p in enumerate(snapshots):
        e = restate(e, p, t0 + k, F32(beta), start, warmup)
    return e


def _run(ts, steps):
    """(G's weights after every step that trained G, [(D_loss, G_loss)] after every step)."""
    snaps, losses = [], []
    for _ in range(steps):
        ts.step()
        torch.cuda.synchronize()
        if "G" in ts.last_ran:
            snaps.append(ts.fG.flat.cpu().numpy().copy())
        losses.append((ts.D_loss.clone(), ts.G_loss.clone()))
    return snaps, losses


@pytest.mark.parametrize("model", ["mpgan", "gapt"])
def test_the_average_is_the_fold_of_the_weights_own_snapshots(model):
    with _device_seed() as seed:
        seed()
        ts = _ema_step(model)
        e0 = ts.fG.flat.cpu().numpy().copy()
        assert _same(ts.fG.ema, ts.fG.flat)
        snaps, _ = _run(ts, 5)
        assert len(snaps) == 5 and not np.array_equal(bits(snaps[0]), bits(snaps[4]))
        got, want = ts.fG.ema.cpu().numpy(), _fold(snaps, e0, 0.9)
        assert np.array_equal(bits(got), bits(want)), int((bits(got) != bits(want)).sum())
        assert _t(ts.fG.ema_state) == [5, 0]
        assert not np.array_equal(bits(got), bits(snaps[4]))


def test_the_step_without_the_option_is_unchanged():
    """Losses, G's and D's weights and optimizer moments after every one of five steps, with the average and without."""
    runs = []
    with _device_seed() as seed:
        for ema in ("default", None):
            seed()
            ts = _ema_step(ema=ema)
            seen = []
            for _ in range(5):
                ts.step()
                seen.append([t.clone() for t in (ts.D_loss, ts.G_loss, ts.fG.flat, ts.fD.flat, ts.fG.sq, ts.fD.sq, ts.fG.grad, ts.fD.grad)])
            runs.append(seen)
            if ema is None:
                assert ts.fG.ema is None and ts.fG.ema_state is None
    for k, (a, b) in enumerate(zip(*runs)):
        assert all(_same(x, y) for x, y in zip(a, b)), (k, [i for i, (x, y) in enumerate(zip(a, b)) if not _same(x, y)])


@pytest.mark.parametrize("optimizer", ["adam", "adadelta"])
def test_the_other_optimizers_fold_the_same_way(optimizer):
    from mpgan_amd.step_options import Ema
    with _device_seed() as seed:
        seed()
        ts = _ema_step(ema=Ema(beta=0.5, start=1, warmup=True), optimizer=optimizer)
        e0 = ts.fG.flat.cpu().numpy().copy()
        snaps, _ = _run(ts, 3)
        got, want = ts.fG.ema.cpu().numpy(), _fold(snaps, e0, 0.5, start=1, warmup=True)
        assert np.array_equal(bits(got), bits(want)) and _t(ts.fG.ema_state) == [3, 0]


# ---- 3. captured against eager ----------------------------------------------------------------------------------------------------
def test_captured_equals_eager_and_capture_leaves_the_average_alone():
    res = []
    with _device_seed() as seed:
        for use_graphs in (False, True):
            seed()
            ts = _ema_step(use_graphs=use_graphs)
            if use_graphs:
                flat0 = ts.fG.flat.clone()
                ts.capture()                       # (three real warm-up iterations, then put back)
                assert _same(ts.fG.ema, ts.fG.flat) and _same(ts.fG.flat, flat0) and _t(ts.fG.ema_state) == [0, 0]
            for _ in range(5):
                ts.step()
            res.append((ts.fG.ema.clone(), _t(ts.fG.ema_state), ts.fG.flat.clone()))
    (e_a, t_a, f_a), (e_c, t_c, f_c) = res
    assert t_a == t_c == [5, 0] and _same(f_a, f_c) and _same(e_a, e_c)
    assert not _same(e_a, f_a)


# ---- 4. the schedule --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_graphs", [False, True], ids=["eager", "captured"])
def test_the_average_moves_only_with_the_generator(use_graphs):
    ran = RAN[(2, 1)]
    with _device_seed() as seed:
        seed()
        ts = _ema_step(num_critic=2, use_graphs=use_graphs)
        e0 = ts.fG.flat.cpu().numpy().copy()
        snaps, t = [], 0
        for b in range(len(ran)):
            before = ts.fG.ema.clone()
            ts.step()
            assert ts.last_ran == ran[b]
            if "G" in ts.last_ran:
                t += 1
                snaps.append(ts.fG.flat.cpu().numpy().copy())
                assert not _same(ts.fG.ema, before), b
            else:                                  # a D-only batch: neither the average nor its step word
                assert _same(ts.fG.ema, before), b
            assert _t(ts.fG.ema_state) == [t, 0], b
        assert t == 2 and np.array_equal(bits(ts.fG.ema.cpu().numpy()), bits(_fold(snaps, e0, 0.9)))


def test_a_generator_only_batch_moves_the_average():
    ran = RAN[(1, 2)]
    with _device_seed() as seed:
        seed()
        ts = _ema_step(num_gen=2)
        for b in range(3):
            before = ts.fG.ema.clone()
            ts.step()
            assert ts.last_ran == ran[b]
        assert ts.last_ran == ("G",) and not _same(ts.fG.ema, before) and _t(ts.fG.ema_state) == [3, 0]


# ---- 5. resume --------------------------------------------------------------------------------------------------------------------
def test_resume_equals_the_uninterrupted_run(tmp_path):
    from mpgan_amd import checkpoint as ck
    from mpgan_amd.step_options import Ema
    tmp = str(tmp_path / "models")
    ema = Ema(beta=0.9, start=1, warmup=True)
    with _device_seed() as seed:
        seed()
        ts = _ema_step(ema=ema)
        for k in range(5):
            ts.step()
            if k == 2:
                torch.cuda.synchronize()
                ck.save_models(ts.D, ts.G, ts.fD, ts.fG, tmp, 3, G_ema=ts.ema_generator())
        whole = (ts.fG.ema.clone(), _t(ts.fG.ema_state), ts.fG.flat.clone())
        assert sorted(os.listdir(tmp)) == ["D_3.pt", "D_optim_3.pt", "G_3.pt", "G_ema_3.pt", "G_optim_3.pt"] and ck.latest_epoch(tmp) == 3
        seed()
        again = _ema_step(ema=ema, seeds=(77, 78))           # other weights: everything comes from the files
        ck.load_models(again.D, again.G, tmp, 3)
        ck.load_optimizers(again.fD, again.fG, tmp, 3)
        assert ck.load_ema(again, tmp, 3) is True
        assert _t(again.fG.ema_state) == [3, 0] and not _same(again.fG.ema, again.fG.flat)
        for _ in range(2):
            again.step()
        assert _t(again.fG.ema_state) == whole[1] == [5, 0]
        assert _same(again.fG.flat, whole[2]) and _same(again.fG.ema, whole[0])
        # without the average's file: the average restarts from the loaded weights at t = 0
        os.remove(os.path.join(tmp, "G_ema_3.pt"))
        seed()
        third = _ema_step(ema=ema, seeds=(5, 6))
        ck.load_models(third.D, third.G, tmp, 3)
        ck.load_optimizers(third.fD, third.fG, tmp, 3)
        assert ck.load_ema(third, tmp, 3) is False
        assert _t(third.fG.ema_state) == [0, 0] and _same(third.fG.ema, third.fG.flat)
        loaded = third.fG.flat.cpu().numpy().copy()
        snaps, _ = _run(third, 2)
        assert _same(third.fG.flat, whole[2])            # (the weights go on as they would have)
        assert np.array_equal(bits(third.fG.ema.cpu().numpy()), bits(_fold(snaps, loaded, 0.9, start=1, warmup=True)))


# ---- 6. the twin ------------------------------------------------------------------------------------------------------------------
def _fresh_generator(state_dict):
    from mpgan_amd import train
    G = train.default_mpgan(N)[0]
    G.load_state_dict({k: v.clone() for k, v in state_dict.items()})
    return G.eval()


def test_the_twin_is_a_generator_holding_the_average():
    from mpgan_amd import gen
    with _device_seed() as seed:
        seed()
        ts = _ema_step()
        for _ in range(3):
            ts.step()
        twin = ts.ema_generator()
        assert type(twin) is type(ts.G) and not twin.training and list(twin.state_dict()) == list(ts.G.state_dict())
        g = torch.Generator(device="cuda").manual_seed(11)
        noise = torch.randn(B, N, 32, device="cuda", generator=g) * 0.2
        labels = torch.full((B, 1), 20 / N, device="cuda")
        table = np.arange(5, N + 1, dtype=np.float32) / N
        sampler = gen.JetSampler(twin, table, N, chunk=8, seed=123)
        for round_ in range(2):
            flat = torch.cat([p.detach().reshape(-1) for p in twin.parameters() if p.requires_grad])
            assert _same(flat, ts.fG.ema) and not _same(flat, ts.fG.flat)
            with torch.no_grad():
                got = twin(noise, labels)
                want = _fresh_generator(twin.state_dict())(noise, labels)
            assert _same(got, want), round_               # (round 1: fails on weight images left from round 0)
            position = sampler.state_dict()
            jets = sampler.sample(8).clone()
            fresh = gen.JetSampler(_fresh_generator(twin.state_dict()), table, N, chunk=8, seed=123)
            fresh.load_state_dict(position)
            assert _same(jets, fresh.sample(8)), round_
            if round_ == 0:
                first = got.clone()
                for _ in range(2):
                    ts.step()
                assert ts.ema_generator() is twin
        assert not _same(first, got)                   # (the average has moved between the rounds)
