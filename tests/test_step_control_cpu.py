"""CPU: the optimizer-step control (``TrainStep(lr_schedule=..., grad_clip=...)``) -- the rule of ``mpg_step_control`` restated in
numpy from include/mpgan_amd.h (``restate`` below; the reference has neither a schedule nor clipping, so this restatement is the
specification) against ``mpg_step_control_host``, the kernel's own body compiled for the host: factor, lr_eff, gmul and s bit for
bit given the function's own norm, the norm against the fp64 sum; the C ABI's refusals; ``LrSchedule`` / ``GradClip``; and the
control's key in an optimizer file."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from test_ema_cpu import bits, mixed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mpgan_amd.h")
F32 = np.float32
NORM_RTOL = 2.0 ** -23      # both sides are an fp32 rounding of fp64 sums that differ by fp64 ulps


def restate(t, base, knots, gscale, max_norm, norm):
    """(factor, lr_eff, gmul, s) of the step at step word ``t`` as include/mpgan_amd.h states them.  ``base``, ``gscale``, ``norm``
    and the knots' factors: np.float32; ``max_norm``: np.float32 or None (no clipping).  Every operation below is one numpy
    float32 operation: one rounding each, nothing fused."""
    assert all(isinstance(v, np.float32) for v in (base, gscale, norm)) and all(isinstance(f, np.float32) for _, f in knots)
    factor = F32(1)
    if knots:
        if t <= knots[0][0]:
            factor = knots[0][1]
        elif t >= knots[-1][0]:
            factor = knots[-1][1]
        else:
            k = max(i for i in range(len(knots) - 1) if knots[i][0] <= t)
            (s0, f0), (s1, f1) = knots[k], knots[k + 1]
            w = F32(t - s0) / F32(s1 - s0)
            d = f1 - f0
            m = w * d
            factor = f0 + m
            assert w.dtype == np.float32 and factor.dtype == np.float32
    lr_eff = base * factor
    gmul = F32(1)
    if max_norm is not None and 0 < max_norm < np.inf:
        q = max_norm / (norm + F32(1e-6))
        assert q.dtype == np.float32
        gmul = F32(1) if q > 1 else q
    s = gscale * gmul
    assert lr_eff.dtype == np.float32 and s.dtype == np.float32
    return factor, lr_eff, gmul, s


def norm64(g, gscale):
    """The norm in fp64 from the fp32 products, rounded to fp32 once."""
    return np.float32(np.sqrt(np.sum((F32(gscale) * np.asarray(g, dtype=np.float32)).astype(np.float64) ** 2)))


def make_block(knots=(), max_norm=0.0, want_norm=0, t=0, base=1e-3):
    """(block, state, base, out, partials): an ``MpgStepCtl`` over host arrays, which the caller keeps alive."""
    from mpgan_amd import _lib
    state = np.array([t, 0], dtype=np.uint32)
    base_a, out, partials = np.array([base], dtype=np.float32), np.full(4, -7.0, dtype=np.float32), np.zeros(256, dtype=np.float64)
    b = _lib.MpgStepCtl()
    b.state, b.base, b.out, b.partials = (a.ctypes.data for a in (state, base_a, out, partials))
    b.nknots = len(knots)
    for k, (step, f) in enumerate(knots):
        b.knot_step[k], b.knot_f[k] = step, f
    b.max_norm, b.want_norm = max_norm, want_norm
    return b, state, base_a, out, partials


def host_control(g, gscale, **kw):
    """(code, out [4], state [2]) of one ``mpg_step_control_host`` call."""
    from mpgan_amd import _lib
    b, state, _, out, _ = make_block(**kw)
    g = None if g is None else np.ascontiguousarray(g, dtype=np.float32)
    ptr = None if g is None else g.ctypes.data_as(C.c_void_p)
    code = _lib.lib().mpg_step_control_host(ptr, 0 if g is None else g.size, float(gscale), C.byref(b))
    return code, out, state


def knots32(knots):
    return [(s, F32(f)) for s, f in knots]


KNOTS8 = [(0, 0.0), (3, 0.3), (10, 1.0), (11, 1.0), (1000, 0.7), (1001, 0.25), (100000, 0.125), (1 << 24, 0.0)]
KNOT_SETS = {"none": [], "one": [(5, 0.37)], "eight": KNOTS8}
# (at, before, between and beyond the knots: every knot of the eight, both neighbours of each, the far end of the 32-bit count)
STEPS = sorted({0, 1, 2, 4, 5, 6, 500, 50000, (1 << 24) - 1, (1 << 24) + 1, 0xFFFFFFFE} | {s + d for s, _ in KNOTS8 for d in (-1, 0, 1)
                                                                                     if s + d >= 0})


@pytest.mark.parametrize("clip", ["off", "binding", "slack"])
@pytest.mark.parametrize("which", list(KNOT_SETS))
def test_host_twin_against_the_restatement(which, clip):
    knots = KNOT_SETS[which]
    g, gscale, base = mixed(1000, 21) * F32(1e-3), F32(0.5), F32(3e-5)
    ref = norm64(g, gscale)
    max_norm = {"off": None, "binding": F32(ref) * F32(0.37), "slack": F32(ref) * F32(1.5)}[clip]
    for t in STEPS:
        code, out, state = host_control(g, gscale, knots=knots, max_norm=0.0 if max_norm is None else float(max_norm),
                                        want_norm=1, t=t, base=float(base))
        assert code == 0 and state.tolist() == [t + 1, 0]
        lr_eff, s, norm, factor = (F32(v) for v in out)
        assert abs(float(norm) - float(ref)) <= NORM_RTOL * float(ref), (float(norm), float(ref))
        w_factor, w_lr, w_gmul, w_s = restate(t, base, knots32(knots), gscale, max_norm, norm)
        assert bits(factor) == bits(w_factor) and bits(lr_eff) == bits(w_lr) and bits(s) == bits(w_s), (t, out, w_factor, w_lr, w_s)
        # gmul is not stored: s = gscale * gmul with gscale = 0.5 is exact, so s says it bit for bit
        assert bits(F32(s / gscale)) == bits(w_gmul)
        assert (float(w_gmul) < 1.0) == (clip == "binding")


def test_the_rule_in_words():
    """No knots and no clip: lr_eff = base and s = gscale exactly; a schedule's ends; the step count stops at 2^32 - 1; without a
    norm wanted none is computed (0 is written, the gradient is not read); ``GradClip(None)``'s block writes the norm and s = gscale."""
    g = mixed(300, 5)
    code, out, state = host_control(None, 0.25, t=7, base=1e-3)
    assert code == 0 and state.tolist() == [8, 0]
    assert [bits(F32(v)) for v in out] == [bits(F32(1e-3)), bits(F32(0.25)), bits(F32(0)), bits(F32(1))]
    code, out, state = host_control(None, 1.0, t=0xFFFFFFFF, base=1e-3, knots=[(0, 0.0), (10, 1.0)])
    assert code == 0 and state.tolist() == [0xFFFFFFFF, 0] and out[0] == F32(1e-3)
    assert host_control(None, 1.0, t=0, base=1e-3, knots=[(0, 0.0), (10, 1.0)])[1][0] == 0.0
    assert host_control(None, 1.0, t=5, base=1.0, knots=[(0, 0.0), (10, 1.0)])[1][3] == F32(0.5)
    code, out, _ = host_control(g, 0.5, want_norm=1)
    assert code == 0 and out[2] == norm64(g, 0.5) and bits(out[1]) == bits(F32(0.5))
    # the sum's order depends on n alone: the same bits from a second call, and for an n beyond one workgroup's 256 elements
    big = mixed(256 * 256 + 1, 9)
    a, b = host_control(big, 0.5, want_norm=1)[1], host_control(big, 0.5, want_norm=1)[1]
    assert np.array_equal(bits(a), bits(b)) and abs(float(a[2]) - float(norm64(big, 0.5))) <= NORM_RTOL * float(a[2])


def test_symbols_struct_and_documented_signatures():
    from mpgan_amd import _lib
    lib = _lib.lib()
    txt = open(HEADER).read()
    decl = lambda sym: [a.split()[-1].lstrip("*") for a in
                        re.search(r"^int\s+" + sym + r"\s*\(([^;]*)\);", txt, flags=re.M | re.S).group(1).split(",")]
    assert decl("mpg_step_control") == ["g", "n", "gscale", "ctl", "stream"]
    assert decl("mpg_step_control_host") == ["g", "n", "gscale", "ctl"]
    for base in ("mpg_rmsprop", "mpg_adam", "mpg_adadelta"):
        assert hasattr(lib, base + "_ctl") and decl(base + "_ctl") == decl(base)[:-1] + ["ctl", "ema", "stream"]
        assert _lib.SIGNATURES[base + "_ctl"][1] == _lib.SIGNATURES[base][1][:-1] + [C.POINTER(_lib.MpgStepCtl), C.POINTER(_lib.MpgEma),
                                                                                  C.c_void_p]
    assert int(re.search(r"^#define\s+MPG_LR_KNOTS\s+(\d+)\s*$", txt, flags=re.M).group(1)) == _lib.LR_KNOTS == 8
    assert [n for n, _ in _lib.MpgStepCtl._fields_] == ["state", "base", "out", "partials", "nknots", "knot_step", "knot_f", "max_norm",
                                                        "want_norm"]
    src = '#include <stdio.h>\n#include "mpgan_amd.h"\nint main(){printf("%zu\\n", sizeof(MpgStepCtl));return 0;}'
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-I", os.path.dirname(HEADER), c, "-o", exe], check=True)
        size = int(subprocess.run([exe], check=True, capture_output=True, text=True).stdout)
    assert size == C.sizeof(_lib.MpgStepCtl)


BAD_BLOCKS = [
    ("knots out of order", dict(knots=[(5, 1.0), (5, 0.5)])),
    ("knots descending", dict(knots=[(5, 1.0), (4, 0.5)])),
    ("knot step above 2^24", dict(knots=[(0, 1.0), ((1 << 24) + 1, 0.5)])),
    ("negative factor", dict(knots=[(0, -0.5)])),
    ("infinite factor", dict(knots=[(0, float("inf"))])),
    ("NaN factor", dict(knots=[(0, 1.0), (3, float("nan"))])),
    ("NaN max_norm", dict(max_norm=float("nan"))),
]


def test_argument_checks():
    from mpgan_amd import _lib
    L = _lib.lib()
    g = np.ones(16, dtype=np.float32)
    gp = g.ctypes.data_as(C.c_void_p)
    for host in (True, False):      # (the launch refuses before it touches the device: host pointers never reach a kernel)
        call = (lambda *a: L.mpg_step_control_host(*a)) if host else (lambda *a: L.mpg_step_control(*a, None))
        ok, state, _, out, _ = make_block(knots=[(0, 0.5), (4, 1.0)], max_norm=1.0)
        if host:
            assert call(gp, 16, 1.0, C.byref(ok)) == 0 and state.tolist() == [1, 0]
        assert call(gp, 16, 1.0, None) == -1
        for field in ("state", "base", "out", "partials"):
            b = make_block(max_norm=1.0)
            setattr(b[0], field, None)
            assert call(gp, 16, 1.0, C.byref(b[0])) == -1, field
        for name, kw in BAD_BLOCKS:
            b = make_block(**kw)
            assert call(gp, 16, 1.0, C.byref(b[0])) == -1, name
            assert b[1].tolist() == [0, 0] and float(b[3][0]) == -7.0, name      # (nothing was written)
        b = make_block()
        b[0].nknots = 9
        assert call(gp, 16, 1.0, C.byref(b[0])) == -1
        b[0].nknots = -1
        assert call(gp, 16, 1.0, C.byref(b[0])) == -1
        for kw in (dict(max_norm=1.0), dict(want_norm=1)):      # a norm to compute: n == 0 and a NULL gradient
            b = make_block(**kw)
            assert call(gp, 0, 1.0, C.byref(b[0])) == -1 and call(None, 16, 1.0, C.byref(b[0])) == -1
    # +inf and <= 0 are "no clipping", not refusals: no norm is wanted then and n == 0 goes through
    for max_norm in (float("inf"), 0.0, -1.0):
        b = make_block(max_norm=max_norm)
        assert L.mpg_step_control_host(None, 0, 0.5, C.byref(b[0])) == 0 and bits(b[3][1]) == bits(F32(0.5))
    # the controlled optimizer entry points: a NULL control, a control without out, n == 0, a bad averaged-generator block
    some = C.c_void_p(64)       # (never dereferenced: every call below is refused before the launch)
    ok = make_block()
    no_out = make_block()
    no_out[0].out = None
    bad_ema = _lib.MpgEma(ema=64, state=64, beta=1.5, start=0, warmup=0)
    calls = {
        "mpg_rmsprop_ctl": lambda n, c, e: L.mpg_rmsprop_ctl(some, some, some, n, 1e-3, 0.99, 1e-8, 1.0, 0, None, 0, c, e, None),
        "mpg_adam_ctl": lambda n, c, e: L.mpg_adam_ctl(some, some, some, some, some, n, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 0, None, 0, c, e,
                                                       None),
        "mpg_adadelta_ctl": lambda n, c, e: L.mpg_adadelta_ctl(some, some, some, some, n, 1.0, 0.9, 1e-6, 1.0, 0, None, 0, c, e, None),
    }
    for name, f in calls.items():
        assert f(16, None, None) == -1, name
        assert f(16, C.byref(no_out[0]), None) == -1, name
        assert f(0, C.byref(ok[0]), None) == -1, name
        assert f(16, C.byref(ok[0]), C.byref(bad_ema)) == -1, name
    assert L.mpg_adam_ctl(some, some, some, some, None, 16, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 0, None, 0, C.byref(ok[0]), None, None) == -1


# ---- the option objects -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [[(0, 1.0)] * 2, [(3, 1.0), (2, 1.0)], [(-1, 1.0)], [((1 << 24) + 1, 1.0)], [(1.5, 1.0)], [(True, 1.0)],
                                 [(0, -0.1)], [(0, float("nan"))], [(0, float("inf"))], [(0, 1e39)], [(0, True)], [5],
                                 [(k, 1.0) for k in range(9)]])
def test_lr_schedule_validation(bad):
    from mpgan_amd.step_options import LrSchedule
    with pytest.raises(ValueError) as e:
        LrSchedule(bad)
    assert "LrSchedule" in str(e.value)


def test_lr_schedule_constructors():
    from mpgan_amd import train
    from mpgan_amd.step_options import GradClip, LrSchedule
    assert train.LrSchedule is LrSchedule and train.GradClip is GradClip
    assert LrSchedule().knots == LrSchedule([]).knots == ()
    assert LrSchedule.warmup(100).knots == ((0, 0.0), (100, 1.0))
    assert LrSchedule.warmup_decay(100, 5000, 6000, 0.1).knots == ((0, 0.0), (100, 1.0), (5000, 1.0), (6000, float(F32(0.1))))
    assert LrSchedule.warmup_decay(0, 50, 60, 0.0).knots == ((0, 1.0), (50, 1.0), (60, 0.0))
    assert LrSchedule.warmup_decay(10, 10, 20, 0.5).knots == ((0, 0.0), (10, 1.0), (20, 0.5))
    assert LrSchedule([(k, 1.0) for k in range(8)]).knots[-1] == (7, 1.0)
    for bad in (dict(warmup=5, hold_until=4, end=10), dict(warmup=0, hold_until=10, end=10), dict(warmup=-1, hold_until=4, end=10),
                dict(warmup=1.0, hold_until=4, end=10), dict(warmup=1, hold_until=4, end=10, final=-1.0)):
        with pytest.raises(ValueError):
            LrSchedule.warmup_decay(**bad)
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError):
            LrSchedule.warmup(bad)
    # ``factor`` is the rule: the host twin's bits at every step of the catalogue
    sched = LrSchedule(KNOTS8)
    for t in STEPS:
        want = host_control(None, 1.0, knots=KNOTS8, t=t)[1][3]
        assert bits(F32(sched.factor(t))) == bits(want), t


@pytest.mark.parametrize("bad", [0, 0.0, -1.0, float("nan"), float("inf"), True, 1e39])
def test_grad_clip_validation(bad):
    from mpgan_amd.step_options import GradClip
    with pytest.raises(ValueError) as e:
        GradClip(bad)
    assert "max_norm" in str(e.value) and repr(bad) in str(e.value)


def test_grad_clip_values():
    from mpgan_amd.step_options import GradClip
    assert GradClip(None).max_norm is None and GradClip().max_norm is None
    assert GradClip(0.1).max_norm == float(F32(0.1)) and GradClip(2).max_norm == 2.0


# ---- the control and its key in an optimizer file ---------------------------------------------------------------------------------
def test_the_control_on_host_tensors_is_the_host_twin():
    from mpgan_amd.step_options import GradClip, LrSchedule, StepControl
    g = mixed(700, 3)
    sc = StepControl(3e-5, LrSchedule.warmup_decay(2, 4, 8, 0.1), GradClip(0.5))
    assert sc.tensors() == [sc.state, sc.base, sc.out] and sc.read() == {"t": 0, "lr": float(F32(3e-5)), "factor": 1.0, "norm": 0.0,
                                                                          "clip": 1.0}
    for t in range(10):
        assert bits(F32(sc.next_lr())) == bits(restate(t, F32(3e-5), knots32(sc.knots), F32(1), None, F32(0))[1])
        sc.launch(torch.from_numpy(g), 0.5)
        code, out, _ = host_control(g, 0.5, knots=sc.knots, max_norm=0.5, t=t, base=3e-5)
        assert code == 0 and np.array_equal(bits(sc.out.numpy()), bits(out)), t
        r = sc.read()
        assert r["t"] == t + 1 and bits(F32(r["clip"])) == bits(F32(out[1] / F32(0.5))) and r["clip"] < 1.0
    sc.set_base(6e-5)
    sc.launch(torch.from_numpy(g), 0.5)
    assert bits(sc.out.numpy()[0]) == bits(F32(6e-5) * F32(0.1))
    for bad in (-1.0, float("nan"), float("inf"), True):
        with pytest.raises(ValueError):
            sc.set_base(bad)
    with pytest.raises(TypeError):
        StepControl(1e-3, [(0, 1.0)])
    with pytest.raises(TypeError):
        StepControl(1e-3, None, 1.0)


def test_save_load_round_trip_through_torch_optim():
    """The key survives ``torch.optim.RMSprop.load_state_dict`` / ``state_dict`` as the seed's does; loading restores t and base;
    a group without the key takes t from the loaded optimizer's step count and leaves base alone."""
    from mpgan_amd.step_options import GradClip, LrSchedule, StepControl
    sched, clip = LrSchedule.warmup_decay(2, 4, 8, 0.1), GradClip(0.5)
    sc = StepControl(3e-5, sched, clip)
    g = torch.from_numpy(mixed(64, 1))
    for _ in range(5):
        sc.launch(g, 1.0)
    sc.set_base(4e-5)
    w = [torch.zeros(3, requires_grad=True)]
    opt = torch.optim.RMSprop(w, lr=1e-3)
    sd = opt.state_dict()
    sc.save(sd["param_groups"][0])
    ent = sd["param_groups"][0][StepControl.KEY]
    assert ent == {"t": 5, "base": float(F32(4e-5)), "knots": [list(k) for k in sched.knots], "max_norm": 0.5}
    again = torch.optim.RMSprop([torch.zeros(3, requires_grad=True)], lr=1e-3)
    again.load_state_dict(sd)
    back = again.state_dict()["param_groups"][0]
    assert back[StepControl.KEY] == ent
    fresh = StepControl(1e-3, sched, clip)
    fresh.load(back)
    assert fresh.t == 5 and fresh.state.tolist() == [5, 0] and bits(fresh.base.numpy()[0]) == bits(F32(4e-5))
    fresh.launch(g, 1.0)
    sc.launch(g, 1.0)
    assert np.array_equal(bits(fresh.out.numpy()), bits(sc.out.numpy()))
    # without the key: t from the step count the optimizer file holds, base as built
    other = StepControl(1e-3, sched, clip)
    other.loaded_steps = 7
    other.load({"lr": 1e-3})
    assert other.state.tolist() == [7, 0] and bits(other.base.numpy()[0]) == bits(F32(1e-3))
    with pytest.raises(ValueError):
        other.set_t(1 << 32)


def test_flat_params_carry_the_control_through_an_optimizer_file():
    """``FlatParams(control=...)`` on host tensors: a real ``torch.optim.RMSprop`` file without the key resumes the schedule at the
    optimizer's step count; ``state_dict`` records the effective rate of the step to come and the key; a round trip restores t."""
    from mpgan_amd.step_options import GradClip, LrSchedule, StepControl
    from mpgan_amd.train import FlatParams
    torch.manual_seed(0)
    sched = LrSchedule.warmup_decay(2, 4, 8, 0.1)
    ref = torch.nn.Linear(5, 3)
    opt = torch.optim.RMSprop(ref.parameters(), lr=1e-3)
    for _ in range(6):
        for p in ref.parameters():
            p.grad = torch.ones_like(p)
        opt.step()
    net = torch.nn.Linear(5, 3)
    fp = FlatParams(net, "rmsprop", control=StepControl(1e-3, sched, GradClip(None)))
    fp.carried = [fp.control]
    fp.load_state_dict(opt.state_dict())
    assert fp.control.t == 6 and fp.steps == 6.0
    sd = fp.state_dict()
    group = sd["param_groups"][0]
    assert bits(F32(group["lr"])) == bits(F32(1e-3) * F32(sched.factor(6))) and 0.1e-3 < group["lr"] < 1e-3
    assert group[StepControl.KEY]["t"] == 6 and group[StepControl.KEY]["max_norm"] is None
    torch.optim.RMSprop(ref.parameters(), lr=1e-3).load_state_dict(sd)      # (torch reads the file as its own)
    other = FlatParams(torch.nn.Linear(5, 3), "rmsprop", control=StepControl(5e-4, sched, GradClip(None)))
    other.carried = [other.control]
    group[StepControl.KEY]["t"] = 3
    other.load_state_dict(sd)
    assert other.control.t == 3 and bits(other.control.base.numpy()[0]) == bits(F32(1e-3))
    with pytest.raises(TypeError):
        FlatParams(torch.nn.Linear(5, 3), "rmsprop", control=object())
