"""GPU: the optimizer-step control -- ``mpg_step_control`` against its host twin (norm against the fp64 sum; factor, lr_eff, gmul and s
bit for bit from the device's own norm; two launches, the same bits), the ``mpg_*_ctl`` optimizer launches against the plain and
averaged ones called with the control's words, ``FlatParams(control=...)`` against torch's ``clip_grad_norm_`` + ``LambdaLR``, and
``TrainStep(lr_schedule=..., grad_clip=...)``: the null control changes nothing, captured equals eager and capture moves no
state, the num_critic schedule, ``set_lr``, resume, and two data-parallel ranks that clip by the norm of the averaged gradient."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from conftest import rel_err
from spawn_util import spawn_joined
from test_ema_cpu import bits, mixed
from test_gpu_ema import SEED_STEP, _Bufs, _same, _words
from test_gpu_schedule import N, RAN, _device_seed, _step
from test_step_control_cpu import F32, NORM_RTOL, host_control, knots32, norm64, restate

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KNOTS = [(0, 0.0), (2, 1.0), (5, 1.0), (9, 0.25)]      # warm-up over two steps, a plateau, a decay


# ---- 1. one launch ----------------------------------------------------------------------------------------------------------------
def _device_block(knots=(), max_norm=0.0, want_norm=0, t=0, base=1e-3):
    """(block, state, base, out, partials) over device tensors, which the caller keeps alive."""
    from mpgan_amd import _lib
    state, base_t = _words(t), torch.full((1,), base, device="cuda")
    out, partials = torch.full((4,), -7.0, device="cuda"), torch.zeros(256, device="cuda", dtype=torch.float64)
    b = _lib.MpgStepCtl()
    b.state, b.base, b.out, b.partials = (x.data_ptr() for x in (state, base_t, out, partials))
    b.nknots = len(knots)
    for k, (step, f) in enumerate(knots):
        b.knot_step[k], b.knot_f[k] = step, f
    b.max_norm, b.want_norm = max_norm, want_norm
    return b, state, base_t, out, partials


def _launch(g, gscale, block):
    from mpgan_amd import _lib
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    return _lib.lib().mpg_step_control(C.c_void_p(g.data_ptr()), g.numel(), gscale, C.byref(block), st)


# (one element, the workgroup's edges, two workgroups; one past the capped grid of 256 workgroups, where a thread takes a second
# element; a ragged tail far beyond it)
@pytest.mark.parametrize("n", [1, 255, 256, 257, 256 * 256 + 1, 2048 * 256 + 3])
def test_one_launch_against_the_host_twin(n):
    g_host = mixed(n, 5 * n + 1) * F32(1e-2)
    g_host[0] = F32(0.75)                      # (n = 1: not one of ``mixed``'s zeros)
    g = torch.from_numpy(g_host).cuda()
    guard = g.clone()
    gscale, base = F32(0.5), F32(3e-5)
    ref = norm64(g_host, gscale)
    for clip, max_norm in (("binding", float(F32(ref) * F32(0.37))), ("slack", float(F32(ref) * F32(1.5))), ("off", 0.0)):
        for t0 in (1, 7):                      # on a warm-up segment and on the decay
            b, state, _base, out, _partials = _device_block(KNOTS, max_norm, want_norm=1, t=t0, base=float(base))
            assert _launch(g, float(gscale), b) == 0
            torch.cuda.synchronize()
            first = out.cpu().numpy().copy()
            assert state.cpu().tolist() == [t0 + 1, 0]                                # t moved by one, the ticket reads 0
            lr_eff, s, norm, factor = (F32(v) for v in first)
            assert abs(float(norm) - float(ref)) <= NORM_RTOL * float(ref), (n, float(norm), float(ref))
            # the host twin, fed the device's norm through the restatement it is tested against, and run itself on the same data
            w_factor, w_lr, w_gmul, w_s = restate(t0, base, knots32(KNOTS), gscale, F32(max_norm) if max_norm else None, norm)
            assert bits(factor) == bits(w_factor) and bits(lr_eff) == bits(w_lr) and bits(s) == bits(w_s), (n, clip, t0, first)
            assert (float(w_gmul) < 1.0) == (clip == "binding")
            code, h_out, h_state = host_control(g_host, gscale, knots=KNOTS, max_norm=max_norm, want_norm=1, t=t0, base=float(base))
            assert code == 0 and h_state.tolist() == [t0 + 1, 0]
            if bits(h_out[2]) == bits(norm):   # (the same order of summation: the same bits throughout whenever the norms agree)
                assert np.array_equal(bits(h_out), bits(first))
            assert abs(float(h_out[2]) - float(norm)) <= NORM_RTOL * float(ref)
            # a second launch on the same data: the same bits
            state.copy_(_words(t0))
            out.fill_(-7.0)
            assert _launch(g, float(gscale), b) == 0
            torch.cuda.synchronize()
            assert np.array_equal(bits(out.cpu().numpy()), bits(first)) and state.cpu().tolist() == [t0 + 1, 0]
    assert _same(g, guard)                     # (the launch reads the gradient and writes none of it)


def test_without_a_norm_the_launch_reads_no_gradient():
    b, state, _base, out, partials = _device_block(KNOTS, 0.0, want_norm=0, t=3, base=2e-4)
    from mpgan_amd import _lib
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert _lib.lib().mpg_step_control(None, 0, 0.5, C.byref(b), st) == 0
    torch.cuda.synchronize()
    assert state.cpu().tolist() == [4, 0] and float(partials.abs().max()) == 0.0
    assert [bits(F32(v)) for v in out.cpu().numpy()] == [bits(F32(2e-4)), bits(F32(0.5)), bits(F32(0)), bits(F32(1))]


def test_launch_argument_checks_write_nothing():
    g = torch.ones(16, device="cuda")
    for kw in (dict(knots=[(5, 1.0), (5, 0.5)]), dict(knots=[(0, -1.0)]), dict(max_norm=float("nan"))):
        b, state, _base, out, _partials = _device_block(**kw)
        assert _launch(g, 1.0, b) == -1
        torch.cuda.synchronize()
        assert state.cpu().tolist() == [0, 0] and float(out[0]) == -7.0


# ---- 2. the controlled optimizer launches -----------------------------------------------------------------------------------------
class _CtlBufs(_Bufs):
    """``_Bufs`` whose launch can go through the ``_ctl`` entry point, or through the plain one with given lr and gscale."""

    def launch_ctl(self, opt, grad, ctl, ema=None):
        from mpgan_amd import _lib
        self.g.copy_(grad)
        vp = lambda t: C.c_void_p(t.data_ptr())
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        lr, gs = 123.0, 456.0                  # (the arguments a controlled launch must not look at)
        if opt == "rmsprop":
            args = (vp(self.p), vp(self.g), vp(self.v), self.n, lr, 0.99, 1e-8, gs, 1, vp(self.seed), SEED_STEP)
        elif opt == "adam":
            args = (vp(self.p), vp(self.g), vp(self.aux), vp(self.v), vp(self.count), self.n, lr, 0.9, 0.999, 1e-8, 5e-4, gs, 1,
                    vp(self.seed), SEED_STEP)
        else:
            args = (vp(self.p), vp(self.g), vp(self.v), vp(self.aux), self.n, lr, 0.9, 1e-6, gs, 1, vp(self.seed), SEED_STEP)
        name = "mpg_" + opt + "_ctl"
        _lib.check(getattr(_lib.lib(), name)(*args, C.byref(ctl), None if ema is None else C.byref(ema), st), name)

    def launch_plain(self, opt, grad, lr, gscale, ema=None):
        from mpgan_amd import _lib
        self.g.copy_(grad)
        vp = lambda t: C.c_void_p(t.data_ptr())
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        tail = (st,) if ema is None else (C.byref(ema), st)
        if opt == "rmsprop":
            args = (vp(self.p), vp(self.g), vp(self.v), self.n, lr, 0.99, 1e-8, gscale, 1, vp(self.seed), SEED_STEP)
        elif opt == "adam":
            args = (vp(self.p), vp(self.g), vp(self.aux), vp(self.v), vp(self.count), self.n, lr, 0.9, 0.999, 1e-8, 5e-4, gscale, 1,
                    vp(self.seed), SEED_STEP)
        else:
            args = (vp(self.p), vp(self.g), vp(self.v), vp(self.aux), self.n, lr, 0.9, 1e-6, gscale, 1, vp(self.seed), SEED_STEP)
        name = "mpg_" + opt + ("" if ema is None else "_ema")
        _lib.check(getattr(_lib.lib(), name)(*args, *tail), name)


@pytest.mark.parametrize("n", [257, 256 * 256 + 1])
@pytest.mark.parametrize("with_ema", [False, True], ids=["plain", "ema"])
@pytest.mark.parametrize("opt", ["rmsprop", "adam", "adadelta"])
def test_ctl_launch_equals_the_plain_launch_with_the_controls_words(opt, with_ema, n):
    """Two launches on one state, a binding clip on a warm-up segment: parameters, moments, average and its words, the cleared
    gradient, Adam's count and the seed word, bit for bit."""
    from mpgan_amd import _lib
    a, b = _CtlBufs(n, 7 * n), _CtlBufs(n, 7 * n)
    emas = []
    for _ in range(2):
        e, st = torch.from_numpy(mixed(n, 3 * n + 1)).cuda(), _words(1)
        emas.append((e, st, _lib.MpgEma(C.c_void_p(e.data_ptr()), C.c_void_p(st.data_ptr()), 0.9, 0, 1) if with_ema else None))
    for k in range(2):
        grad = torch.from_numpy(mixed(n, 100 * k + n)).cuda()
        ref = norm64(grad.cpu().numpy(), 0.5)
        ctl, state, _base, out, _partials = _device_block(KNOTS, float(ref) * 0.5, want_norm=0, t=1 + k, base=1e-2)
        assert _launch(grad, 0.5, ctl) == 0
        torch.cuda.synchronize()
        lr_eff, s = (float(v) for v in out.cpu().numpy()[:2])
        assert 0.0 < lr_eff <= 1e-2 and 0.2 < s < 0.3                                  # (scheduled and clipped: neither is the argument)
        a.launch_ctl(opt, grad, ctl, emas[0][2])
        b.launch_plain(opt, grad, lr_eff, s, emas[1][2])
        torch.cuda.synchronize()
        for name, x, y in zip(("p", "g", "v", "aux", "count", "seed"), a.all(), b.all()):
            assert _same(x, y), (k, name)
        assert _same(emas[0][0], emas[1][0]) and _same(emas[0][1], emas[1][1])
        assert float(a.g.abs().max()) == 0.0 and int(a.seed) % (1 << 64) == (12345 + (k + 1) * SEED_STEP) % (1 << 64)
        assert emas[0][1].cpu().tolist() == ([2 + k, 0] if with_ema else [1, 0])
    assert not _same(a.p, torch.from_numpy(mixed(n, 7 * n)).cuda())


# ---- 3. against torch -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt", ["rmsprop", "adam", "adadelta"])
def test_controlled_optimizers_vs_torch(opt):
    """``test_fused_optimizers_vs_torch`` with ``clip_grad_norm_`` and a ``LambdaLR`` over the same knots on the fp64 twin; the
    gradients' scale alternates so that max_norm = 1 binds on steps 0, 2, 4 (norm ~ 38) and not on steps 1, 3 (norm ~ 0.4)."""
    from mpgan_amd.step_options import GradClip, LrSchedule, StepControl
    from mpgan_amd.train import FlatParams
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(40, 30), torch.nn.Linear(30, 7)).cuda()
    ref = torch.nn.Sequential(torch.nn.Linear(40, 30), torch.nn.Linear(30, 7)).cuda().double()
    ref.load_state_dict({k: v.double() for k, v in net.state_dict().items()})
    cls = {"rmsprop": torch.optim.RMSprop, "adam": torch.optim.Adam, "adadelta": torch.optim.Adadelta}[opt]
    kw = {"weight_decay": 5e-4, "betas": (0.5, 0.9)} if opt == "adam" else {}
    lr = {"rmsprop": 1e-3, "adam": 1e-3, "adadelta": 1.0}[opt]
    knots = [(0, 0.25), (2, 1.0), (3, 1.0), (6, 0.5)]
    sched, max_norm = LrSchedule(knots), 1.0
    to = cls(ref.parameters(), lr=lr, **kw)

    def factor64(t):       # the knots in fp64
        if t <= knots[0][0]:
            return knots[0][1]
        if t >= knots[-1][0]:
            return knots[-1][1]
        k = max(i for i in range(len(knots) - 1) if knots[i][0] <= t)
        return knots[k][1] + (t - knots[k][0]) / (knots[k + 1][0] - knots[k][0]) * (knots[k + 1][1] - knots[k][1])
    lam = torch.optim.lr_scheduler.LambdaLR(to, factor64)
    ctl = StepControl(lr, sched, GradClip(max_norm), "cuda")
    fp = FlatParams(net, opt, betas=(0.5, 0.9), control=ctl)
    for it in range(5):
        scale = 1.0 if it % 2 == 0 else 0.01
        grads = [scale * torch.randn_like(p) for p in net.parameters()]
        for p, q, gr in zip(net.parameters(), ref.parameters(), grads):
            p.grad.copy_(2.0 * gr)          # "summed over 2 ranks"
            q.grad = gr.double()
        assert abs(to.param_groups[0]["lr"] - ctl.next_lr()) <= 1e-6 * lr
        fp.step(lr, gscale=0.5, zero_grad=it % 2 == 1)
        assert (float(fp.grad.abs().max()) == 0.0) == (it % 2 == 1)
        total = float(torch.nn.utils.clip_grad_norm_(ref.parameters(), max_norm))
        to.step()
        lam.step()
        r = ctl.read()
        assert r["t"] == it + 1 and abs(r["norm"] - total) <= 1e-6 * total and abs(r["factor"] - factor64(it)) <= 1e-6
        assert (r["clip"] < 1.0) == (it % 2 == 0) == (total > max_norm), (it, r, total)
    assert fp.steps == 5.0
    for p, q in zip(net.parameters(), ref.parameters()):
        assert rel_err(p.detach().cpu().numpy(), q.detach().cpu().numpy()) < 1e-5


# ---- 4. the step ------------------------------------------------------------------------------------------------------------------
B = 4
CLIP = 1e-5           # (far below the gradient norms of the smallest MPGAN step: binds on every step, which the tests assert)


def _ctl_step(sched="default", clip="default", **kw):
    from mpgan_amd.step_options import GradClip, LrSchedule
    kw.setdefault("use_graphs", False)
    return _step("mpgan", B, lr_schedule=LrSchedule(KNOTS) if sched == "default" else sched,
                 grad_clip=GradClip(CLIP) if clip == "default" else clip, **kw)


def _weights(ts):
    torch.cuda.synchronize()
    return [t.clone() for t in (ts.D_loss, ts.G_loss, ts.fD.flat, ts.fG.flat, ts.fD.sq, ts.fG.sq, ts.fD.grad, ts.fG.grad)]


class _Calls:
    """The library with the names of the entry points called through it, in order."""

    def __init__(self, real):
        self._real, self.names = real, []

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name.startswith("mpg_"):
            self.names.append(name)
        return fn


def _recorded(ts):
    """The entry points one eager ``step()`` calls, in order."""
    from mpgan_amd import _lib
    real = _lib.lib()
    _lib._lib = rec = _Calls(real)
    try:
        ts.step()
    finally:
        _lib._lib = real
    return rec.names


@pytest.mark.parametrize("use_graphs", [False, True], ids=["eager", "captured"])
def test_the_null_control_changes_nothing(use_graphs):
    """``LrSchedule([])`` + ``GradClip(None)`` -- factor 1, no clipping, the norm read out -- against the step built without the
    options: losses, weights, moments and cleared gradients of D and G after each of three steps, bit for bit."""
    from mpgan_amd.step_options import GradClip, LrSchedule
    runs = []
    with _device_seed() as seed:
        for null in (True, False):
            seed()
            ts = _ctl_step(LrSchedule([]), GradClip(None), use_graphs=use_graphs) if null else _step("mpgan", B, use_graphs=use_graphs)
            seen = []
            for _ in range(3):
                ts.step()
                seen.append(_weights(ts))
            runs.append(seen)
            if null:
                sc = ts.step_control
                assert sc["D"]["t"] == sc["G"]["t"] == 3 and sc["D"]["factor"] == sc["G"]["factor"] == 1.0
                assert sc["D"]["clip"] == sc["G"]["clip"] == 1.0 and sc["D"]["norm"] > 0.0 and sc["G"]["norm"] > 0.0
                assert bits(F32(sc["D"]["lr"])) == bits(F32(ts.lr_disc)) and bits(F32(sc["G"]["lr"])) == bits(F32(ts.lr_gen))
            else:
                assert ts.fD.control is None and ts.fG.control is None and ts.fD.carried == []
                with pytest.raises(RuntimeError):
                    ts.step_control
    for k, (a, b) in enumerate(zip(*runs)):
        assert all(_same(x, y) for x, y in zip(a, b)), (k, [i for i, (x, y) in enumerate(zip(a, b)) if not _same(x, y)])


def test_the_default_step_launches_what_it_did_and_the_control_adds_two():
    """The entry points of one eager step: the default step calls neither ``mpg_step_control`` nor a ``_ctl`` optimizer -- its two
    optimizer launches are ``mpg_rmsprop`` -- and the controlled step is the same sequence with ``mpg_step_control`` in front of
    each optimizer launch, which goes through ``mpg_rmsprop_ctl``."""
    with _device_seed() as seed:
        seed()
        plain = _step("mpgan", B, use_graphs=False)
        plain.step()
        default = _recorded(plain)
        seed()
        ts = _ctl_step()
        ts.step()
        controlled = _recorded(ts)
    assert not [n for n in default if "step_control" in n or n.endswith("_ctl")]
    assert [n for n in default if n in ("mpg_rmsprop", "mpg_adam", "mpg_adadelta") or n.endswith("_ema")] == ["mpg_rmsprop"] * 2
    want = []
    for n in default:
        want += ["mpg_step_control", "mpg_rmsprop_ctl"] if n == "mpg_rmsprop" else [n]
    assert controlled == want and len(controlled) == len(default) + 2
    # one network alone: the other's launch stays the plain one
    from mpgan_amd.step_options import GradClip
    with _device_seed() as seed:
        seed()
        only_d = _ctl_step(None, (GradClip(CLIP), None))
        only_d.step()
        names = _recorded(only_d)
    assert [n for n in names if "rmsprop" in n or "step_control" in n] == ["mpg_step_control", "mpg_rmsprop_ctl", "mpg_rmsprop"]
    assert only_d.fG.control is None and only_d.step_control["G"] is None and only_d.step_control["D"]["t"] == 2


def test_captured_equals_eager_and_capture_moves_no_state():
    res = []
    with _device_seed() as seed:
        for use_graphs in (False, True):
            seed()
            ts = _ctl_step(use_graphs=use_graphs)
            if use_graphs:
                flat0 = ts.fD.flat.clone()
                before = [t.clone() for f in (ts.fD, ts.fG) for t in f.control.tensors()]
                ts.capture()                       # (three real warm-up iterations, then put back)
                after = [t for f in (ts.fD, ts.fG) for t in f.control.tensors()]
                assert all(_same(x, y) for x, y in zip(before, after)) and _same(ts.fD.flat, flat0)
                assert ts.fD.control in ts.fD.carried and ts.fG.control in ts.fG.carried
            for _ in range(4):
                ts.step()
            res.append((_weights(ts), ts.step_control, [ts.fD.control.out.clone(), ts.fG.control.out.clone()]))
    (w_e, sc_e, out_e), (w_c, sc_c, out_c) = res
    assert all(_same(x, y) for x, y in zip(w_e, w_c)) and all(_same(x, y) for x, y in zip(out_e, out_c)) and sc_e == sc_c
    from mpgan_amd.step_options import LrSchedule
    for net, lr in (("D", ts.lr_disc), ("G", ts.lr_gen)):
        r = sc_c[net]
        assert r["t"] == 4                                          # (the warm-up's iterations did not advance it)
        want = restate(3, F32(lr), knots32(KNOTS), F32(1), F32(CLIP), F32(r["norm"]))     # the last step taken was t = 3
        assert bits(F32(r["factor"])) == bits(want[0]) == bits(F32(LrSchedule(KNOTS).factor(3))) and r["factor"] == 1.0
        assert bits(F32(r["lr"])) == bits(want[1]) and bits(F32(r["clip"])) == bits(want[2])
        assert r["norm"] > CLIP and r["clip"] < 1.0                 # (the clip binds)


@pytest.mark.parametrize("use_graphs", [False, True], ids=["eager", "captured"])
def test_each_control_counts_its_own_optimizers_steps(use_graphs):
    ran = RAN[(2, 1)]
    with _device_seed() as seed:
        seed()
        ts = _ctl_step(num_critic=2, use_graphs=use_graphs)
        t_d = t_g = 0
        for b in range(len(ran)):
            g_words = [t.clone() for t in ts.fG.control.tensors()]
            ts.step()
            assert ts.last_ran == ran[b]
            t_d += "D" in ts.last_ran
            t_g += "G" in ts.last_ran
            sc = ts.step_control
            assert (sc["D"]["t"], sc["G"]["t"]) == (t_d, t_g), b
            if "G" not in ts.last_ran:            # a D-only batch: G's control words untouched
                assert all(_same(x, y) for x, y in zip(g_words, ts.fG.control.tensors())), b
            want = restate(t_d - 1, F32(ts.lr_disc), knots32(KNOTS), F32(1), None, F32(0))
            assert bits(F32(sc["D"]["factor"])) == bits(want[0]) and bits(F32(sc["D"]["lr"])) == bits(want[1]), b
        assert (t_d, t_g) == (4, 2)
        assert bits(F32(sc["G"]["factor"])) == bits(restate(1, F32(1), knots32(KNOTS), F32(1), None, F32(0))[0])


def test_set_lr_on_a_captured_step():
    """A captured controlled step follows ``set_lr`` without a recapture: from one saved state, one step at the base rates and one
    at twice them -- out[0] is the fp32 product bit for bit, and D's update (its gradient does not depend on the rate) doubles to
    within the roundings of the two stored weights; G's differs as D's weights do.  Without control ``set_lr`` sets the attributes
    before a capture and raises after it."""
    from mpgan_amd.step_options import LrSchedule
    with _device_seed() as seed:
        seed()
        ts = _ctl_step(LrSchedule(KNOTS), None, use_graphs=True)
        ts.step()                                # t = 0 -> 1: captured here; the next step is on the warm-up segment (factor 0.5)
        torch.cuda.synchronize()
        saved = [t.clone() for t in ts._training_state()]
        graphs = list(ts._graphs)
        lr_d, lr_g = ts.lr_disc, ts.lr_gen
        p0 = ts.fD.flat.clone()
        seen = {}
        for mul in (1.0, 2.0):
            for t, v in zip(ts._training_state(), saved):
                t.copy_(v)
            ts._refresh_packed(ts.D)
            ts._refresh_packed(ts.G)
            ts.set_lr(lr_disc=mul * lr_d, lr_gen=mul * lr_g)
            ts.step()
            torch.cuda.synchronize()
            seen[mul] = (ts.fD.flat.clone(), ts.fD.control.out.clone(), ts.fG.control.out.clone(), ts.step_control)
        assert ts._graphs == graphs and (ts.lr_disc, ts.lr_gen) == (2.0 * lr_d, 2.0 * lr_g)      # (no recapture)
        half = F32(LrSchedule(KNOTS).factor(1))
        assert half == F32(0.5)
        for mul in (1.0, 2.0):
            _, out_d, out_g, sc = seen[mul]
            assert sc["D"]["t"] == sc["G"]["t"] == 2
            assert bits(out_d.cpu().numpy()[0]) == bits(F32(mul * lr_d) * half) and bits(out_g.cpu().numpy()[0]) == bits(F32(mul * lr_g) * half)
        d1, d2 = (seen[1.0][0] - p0).double(), (seen[2.0][0] - p0).double()
        assert float(d1.abs().max()) > 0.0
        bound = 2.0 ** -22 * torch.maximum(p0.abs(), torch.maximum(seen[1.0][0].abs(), seen[2.0][0].abs())).double()
        assert bool(((d2 - 2.0 * d1).abs() <= bound).all()), float(((d2 - 2.0 * d1).abs() - bound).max())
        # without control
        seed()
        plain = _step("mpgan", B, use_graphs=True)
        plain.set_lr(lr_disc=1e-4)
        assert plain.lr_disc == 1e-4 and plain.lr_gen == lr_g
        plain.step()
        with pytest.raises(RuntimeError) as e:
            plain.set_lr(lr_gen=1e-4)
        assert "lr_schedule=" in str(e.value) and plain.lr_gen == lr_g
        plain.set_lr()                           # (nothing asked for: nothing to refuse)


def test_resume_equals_the_uninterrupted_run(tmp_path):
    from mpgan_amd import checkpoint as ck
    from mpgan_amd.step_options import StepControl
    tmp = str(tmp_path / "models")
    with _device_seed() as seed:
        seed()
        ts = _ctl_step()
        for k in range(5):
            ts.step()
            if k == 2:
                torch.cuda.synchronize()
                ck.save_models(ts.D, ts.G, ts.fD, ts.fG, tmp, 3)
        whole = (_weights(ts), ts.step_control)
        for tag, flat, lr in (("D", ts.fD, ts.lr_disc), ("G", ts.fG, ts.lr_gen)):
            group = torch.load(os.path.join(tmp, f"{tag}_optim_3.pt"))["param_groups"][0]
            ent = group[StepControl.KEY]
            assert ent == {"t": 3, "base": float(F32(lr)), "knots": [list(k) for k in knots32(KNOTS)], "max_norm": float(F32(CLIP))}
            # the effective rate of the step to come (t = 3: the plateau), where a torch scheduler leaves it
            assert bits(F32(group["lr"])) == bits(restate(3, F32(lr), knots32(KNOTS), F32(1), None, F32(0))[1])
        seed()
        again = _ctl_step(seeds=(77, 78))                    # other weights: everything comes from the files
        again.set_lr(1.0, 1.0)                               # (and other base rates: the files' are restored)
        ck.load_models(again.D, again.G, tmp, 3)
        ck.load_optimizers(again.fD, again.fG, tmp, 3)
        sc = again.step_control
        assert sc["D"]["t"] == sc["G"]["t"] == 3
        for _ in range(2):
            again.step()
        assert again.step_control == whole[1] and whole[1]["D"]["t"] == 5
        assert all(_same(x, y) for x, y in zip(_weights(again), whole[0]))


# ---- 5. data parallel -------------------------------------------------------------------------------------------------------------
DP_STEPS = 2


def _rank_main(rank, world, port, out):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    from mpgan_amd import dist as mdist, train
    from mpgan_amd.step_options import GradClip, LrSchedule
    from oracle import train_ref as T
    from oracle.train_ref import synthetic_batch
    torch.cuda.set_device(0)
    r, w, pg = mdist.init_from_env("gloo")
    Br = 4
    G, D = train.default_mpgan(N, disc_dropout=0.0)
    if rank == 0:
        G.load_state_dict(T.init_state_dict(T.mpgan_param_shapes(True), 41, torch.float32))
        D.load_state_dict(T.init_state_dict(T.mpgan_param_shapes(False), 42, torch.float32))
    mdist.broadcast_module(G, 0, pg)
    mdist.broadcast_module(D, 0, pg)
    data, labels = synthetic_batch(Br * world, N, seed=3)
    sl = slice(rank * Br, (rank + 1) * Br)
    ts = train.TrainStep(G, D, Br, N, lr_disc=train.LR["g"][0], lr_gen=train.LR["g"][1], use_graphs=True, process_group=pg,
                         world_size=world, lr_schedule=LrSchedule(KNOTS), grad_clip=GradClip(CLIP))
    ts.set_batch(data[sl].cuda(), labels[sl].cuda())
    dumps = []
    reduce = ts._allreduce

    def dumping(flat):       # (an ordinary call between the graphs of a batch: the gradient as this rank's backward left it)
        torch.cuda.synchronize()
        dumps.append(flat.grad.detach().cpu().clone())
        reduce(flat)
    ts._allreduce = dumping
    ts.capture(warmup=0)
    assert len(ts._graphs) == 3
    trace = []
    for _ in range(DP_STEPS):
        ts.step()
        torch.cuda.synchronize()
        trace.append(ts.step_control)
    out[rank] = (trace, dumps, ts.fD.flat.cpu(), ts.fG.flat.cpu())
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_clip_by_the_norm_of_the_averaged_gradient():
    """B = 4 per rank, captured (three graphs, the all-reduces between them), a binding clip: the ranks end with the same weights
    bit for bit and report the same norms -- those of the mean of the two ranks' gradients, dumped in front of each all-reduce and
    averaged here in fp64."""
    import torch.multiprocessing as mp
    world = 2
    out = mp.get_context("spawn").Manager().dict()
    spawn_joined(_rank_main, (world, 29581, out), world)
    (tr0, dumps0, fD0, fG0), (tr1, dumps1, fD1, fG1) = out[0], out[1]
    assert _same(fD0, fD1) and _same(fG0, fG1) and tr0 == tr1
    assert len(dumps0) == len(dumps1) == 2 * DP_STEPS           # D's and G's, every step
    for k in range(DP_STEPS):
        for j, net in enumerate(("D", "G")):
            a, b = dumps0[2 * k + j].double(), dumps1[2 * k + j].double()
            assert not torch.equal(a, b)                        # (the ranks' own batches)
            want = float(torch.sqrt((((a + b) * 0.5) ** 2).sum()))
            got = tr0[k][net]
            assert abs(got["norm"] - want) <= NORM_RTOL * want, (k, net, got["norm"], want)
            assert got["clip"] < 1.0 and got["t"] == k + 1
