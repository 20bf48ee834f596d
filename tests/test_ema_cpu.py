"""CPU: the averaged generator (``TrainStep(ema=Ema(...))``) -- the update rule of ``mpg_*_ema`` restated in numpy from
include/mpgan_amd.h (``restate`` below; the reference has no averaged generator, so this restatement is the specification) against
``mpg_ema_update_host``, the kernels' own body compiled for the host, bit for bit; ``step_options.Ema``'s validation; the C ABI's
refusals; and the files: ``G_ema_<epoch>.pt``, ``latest_epoch``, the average's key in G's optimizer file."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from test_dist_cpu import ToyD, ToyG, N, LAT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mpgan_amd.h")
F32 = np.float32


def restate(e, p_new, t, beta, start, warmup):
    """The average after one launch at step word ``t``, as include/mpgan_amd.h states it.  ``e``, ``p_new``: float32 arrays;
    ``beta``: np.float32.  Every operation below is one numpy float32 operation: one rounding each, nothing fused."""
    assert e.dtype == p_new.dtype == np.float32 and isinstance(beta, np.float32)
    if t < start:
        return p_new.copy()
    k = F32(min(t - start, 1 << 24))
    beta_t = beta
    if warmup:
        ramp = (F32(1) + k) / (F32(10) + k)
        assert ramp.dtype == np.float32
        beta_t = min(beta, ramp)
    om = F32(1) - beta_t
    d = p_new - e
    m = om * d
    out = e + m
    assert om.dtype == np.float32 and out.dtype == np.float32
    return out


def mixed(n, seed):
    """n float32 values of mixed magnitude (1e-6 .. 1e3, both signs), with exact zeros among every fifty or more."""
    g = np.random.default_rng(seed)
    v = (g.standard_normal(n) * 10.0 ** g.uniform(-6, 3, n)).astype(np.float32)
    v[g.integers(0, n, size=n // 50)] = 0
    return v


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def kimg_beta(kimg=10, batch=256):
    from mpgan_amd.step_options import Ema
    return F32(Ema(kimg=kimg).beta_for(batch))


def host_update(e, p_new, t, beta, start, warmup):
    from mpgan_amd import _lib
    e = np.array(e, dtype=np.float32)
    p = np.ascontiguousarray(p_new, dtype=np.float32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    code = _lib.lib().mpg_ema_update_host(ptr(e), ptr(p), e.size, t, float(beta), start, int(warmup))
    return code, e


START = 3
STEPS = (0, START - 1, START, START + 1, START + 9, START + 10 ** 6, (1 << 24) + 5)


@pytest.mark.parametrize("warmup", [False, True], ids=["plain", "warmup"])
@pytest.mark.parametrize("beta", [0.0, 0.5, 0.999, "kimg"])
def test_host_twin_against_the_restatement(beta, warmup):
    beta = kimg_beta() if beta == "kimg" else F32(beta)
    e0, p = mixed(1000, 11), mixed(1000, 12)
    p[:100] = e0[:100] * F32(1.0001)          # (weights close to their average, as in training)
    for start in (0, START):
        for t in STEPS + ((1 << 24) + 5 + START,):
            want = restate(e0, p, t, beta, start, warmup)
            code, got = host_update(e0, p, t, beta, start, warmup)
            assert code == 0 and np.array_equal(bits(got), bits(want)), (start, t, int((bits(got) != bits(want)).sum()))


def test_the_rule_in_words():
    """Before ``start`` the average is the weights; beta = 0 follows them as well wherever the sum is exact; without warm-up t
    plays no part beyond ``start``; the warm-up's first step takes beta_t = 1 / 10 and it is over once (1 + k) / (10 + k) >= beta."""
    e0, p = mixed(64, 1), mixed(64, 2)
    assert np.array_equal(bits(host_update(e0, p, 2, 0.999, 3, True)[1]), bits(p))
    assert np.array_equal(bits(host_update(e0, p, 3, 0.5, 3, False)[1]), bits(host_update(e0, p, 10 ** 6, 0.5, 3, False)[1]))
    zero = np.zeros(64, dtype=np.float32)
    assert np.array_equal(bits(host_update(zero, p, 0, 0.0, 0, False)[1]), bits(p))
    first = host_update(zero, p, 3, 0.999, 3, True)[1]
    assert np.array_equal(bits(first), bits((F32(1) - F32(1) / F32(10)) * p))
    late = host_update(e0, p, 3 + 10 ** 6, 0.999, 3, True)[1]
    assert np.array_equal(bits(late), bits(host_update(e0, p, 3, 0.999, 3, False)[1]))
    assert not np.array_equal(bits(first), bits(host_update(zero, p, 3, 0.999, 3, False)[1]))


def test_kimg_is_stylegans_half_life():
    from mpgan_amd.step_options import Ema
    b = Ema(kimg=10).beta_for(256)
    assert b == float(F32(0.5 ** (256 / 10000.0))) and 0.98 < b < 0.983
    assert abs(b ** (10000 / 256) - 0.5) < 1e-5                    # (half of the average is 10 thousand jets old)
    assert Ema(beta=0.999).beta_for(None) == float(F32(0.999))
    e = Ema(kimg=2.5, start=7, warmup=True)
    assert (e.beta, e.kimg, e.start, e.warmup) == (None, 2.5, 7, True)
    with pytest.raises(ValueError):
        Ema(kimg=10).beta_for(None)
    with pytest.raises(ValueError):
        Ema(kimg=1e12).beta_for(1)                                  # (rounds to a decay of 1 in fp32)


@pytest.mark.parametrize("bad", [dict(), dict(beta=0.9, kimg=10), dict(beta=1.0), dict(beta=-0.1), dict(beta=float("nan")),
                                 dict(beta=True), dict(kimg=0), dict(kimg=-1.0), dict(kimg=float("nan")), dict(beta=0.9, start=-1),
                                 dict(beta=0.9, start=1.5), dict(beta=0.9, start=True)])
def test_ema_validation(bad):
    from mpgan_amd.step_options import Ema
    with pytest.raises(ValueError):
        Ema(**bad)


def test_ema_is_exported_and_refused_by_type():
    from mpgan_amd import train
    from mpgan_amd.step_options import Ema
    assert train.Ema is Ema
    assert Ema(beta=0.0).beta == 0.0 and Ema(beta=0.5).start == 0 and Ema(beta=0.5).warmup is False
    with pytest.raises(TypeError):
        train.TrainStep(ToyG(), ToyD(), 4, N, latent=LAT, use_graphs=False, ema=0.999)


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------
def test_symbols_struct_and_documented_signatures():
    from mpgan_amd import _lib
    lib = _lib.lib()
    txt = open(HEADER).read()
    for base in ("mpg_rmsprop", "mpg_adam", "mpg_adadelta"):
        decl = lambda sym: [a.split()[-1].lstrip("*") for a in
                            re.search(r"^int\s+" + sym + r"\s*\(([^;]*)\);", txt, flags=re.M | re.S).group(1).split(",")]
        plain, ema = decl(base), decl(base + "_ema")
        assert hasattr(lib, base + "_ema") and ema == plain[:-1] + ["ema", "stream"]      # (the block in front of the stream)
        args, args_ema = _lib.SIGNATURES[base][1], _lib.SIGNATURES[base + "_ema"][1]
        assert args_ema == args[:-1] + [C.POINTER(_lib.MpgEma), C.c_void_p]
    assert [n for n, _ in _lib.MpgEma._fields_] == ["ema", "state", "beta", "start", "warmup"]
    src = '#include <stdio.h>\n#include "mpgan_amd.h"\nint main(){printf("%zu\\n", sizeof(MpgEma));return 0;}'
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-I", os.path.dirname(HEADER), c, "-o", exe], check=True)
        size = int(subprocess.run([exe], check=True, capture_output=True, text=True).stdout)
    assert size == C.sizeof(_lib.MpgEma)


def _blocks():
    """(name, block or None) that the averaged entry points refuse; the pointers are never followed."""
    from mpgan_amd import _lib
    some = C.c_void_p(4096)
    ok = dict(ema=some, state=some, beta=0.5, start=0, warmup=0)
    bad = [("null ema", dict(ema=None)), ("null state", dict(state=None)), ("beta 1", dict(beta=1.0)), ("beta < 0", dict(beta=-0.1)),
           ("beta nan", dict(beta=float("nan"))), ("start < 0", dict(start=-1))]
    return [("null block", None)] + [(name, _lib.MpgEma(**dict(ok, **kw))) for name, kw in bad], _lib.MpgEma(**ok)


def test_cabi_refusals():
    """Every refusal comes back before any launch (this machine has no GPU to launch on)."""
    from mpgan_amd import _lib
    L = _lib.lib()
    some = C.c_void_p(4096)
    blocks, ok = _blocks()
    calls = {
        "mpg_rmsprop_ema": lambda n, b: L.mpg_rmsprop_ema(some, some, some, n, 1e-3, 0.99, 1e-8, 1.0, 0, None, 0, b, None),
        "mpg_adam_ema": lambda n, b: L.mpg_adam_ema(some, some, some, some, some, n, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 0, None, 0, b, None),
        "mpg_adadelta_ema": lambda n, b: L.mpg_adadelta_ema(some, some, some, some, n, 1.0, 0.9, 1e-6, 1.0, 0, None, 0, b, None),
    }
    for sym, call in calls.items():
        for name, blk in blocks:
            assert call(16, None if blk is None else C.byref(blk)) == -1, (sym, name)
        assert call(0, C.byref(ok)) == -1, (sym, "n == 0 with a block")
    assert L.mpg_adam_ema(some, some, some, some, None, 16, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 0, None, 0, C.byref(ok), None) == -1
    # the entry points without the average keep their own answers for n == 0
    assert L.mpg_rmsprop(some, some, some, 0, 1e-3, 0.99, 1e-8, 1.0, 0, None, 0, None) == 0
    assert L.mpg_rmsprop(some, some, some, 0, 1e-3, 0.99, 1e-8, 1.0, 0, some, 1, None) == -1
    e, p = np.zeros(4, dtype=np.float32), np.ones(4, dtype=np.float32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    H = L.mpg_ema_update_host
    assert H(ptr(e), ptr(p), 4, 0, 0.5, 0, 0) == 0 and e.tolist() == [0.5] * 4
    for args in ((None, ptr(p), 4, 0, 0.5, 0, 0), (ptr(e), None, 4, 0, 0.5, 0, 0), (ptr(e), ptr(p), 0, 0, 0.5, 0, 0),
                 (ptr(e), ptr(p), 4, 0, 1.0, 0, 0), (ptr(e), ptr(p), 4, 0, -0.1, 0, 0), (ptr(e), ptr(p), 4, 0, float("nan"), 0, 0),
                 (ptr(e), ptr(p), 4, 0, 0.5, -1, 0)):
        assert H(*args) == -1, args
    assert e.tolist() == [0.5] * 4


# ---- files ------------------------------------------------------------------------------------------------------------------------
def _toy_step(ema, seed=0, **kw):
    from mpgan_amd import train
    torch.manual_seed(seed)
    return train.TrainStep(ToyG(), ToyD(), 4, N, latent=LAT, lr_disc=1e-2, lr_gen=2e-2, use_graphs=False, ema=ema, **kw)


def test_flat_params_own_the_average():
    from mpgan_amd import train
    from mpgan_amd.step_options import Ema, EmaState
    ts = _toy_step(Ema(beta=0.9, start=2, warmup=True))
    fG = ts.fG
    assert torch.equal(fG.ema, fG.flat) and fG.ema.data_ptr() != fG.flat.data_ptr()
    assert fG.ema_state.dtype == torch.uint32 and fG.ema_state.tolist() == [0, 0]
    blk = fG._ema_block
    assert (blk.ema, blk.state, blk.start, blk.warmup) == (fG.ema.data_ptr(), fG.ema_state.data_ptr(), 2, 1)
    assert blk.beta == float(F32(0.9))
    ent = [c for c in fG.carried if isinstance(c, EmaState)]
    assert len(ent) == 1 and [t.data_ptr() for t in ent[0].tensors()] == [fG.ema.data_ptr(), fG.ema_state.data_ptr()]
    state = ts._training_state()
    assert any(t is fG.ema for t in state) and any(t is fG.ema_state for t in state)
    assert ts.fD.ema is None and ts.fD.ema_state is None and not any(isinstance(c, EmaState) for c in ts.fD.carried)
    off = _toy_step(None)
    assert off.fG.ema is None and off.fG.ema_state is None and off.fG._ema_block is None
    assert not any(isinstance(c, EmaState) for c in off.fG.carried)
    with pytest.raises(RuntimeError):
        off.ema_generator()
    assert train.FlatParams(ToyG(), ema=Ema(kimg=10), batch_size=256).ema_carried.beta == float(kimg_beta())


def test_twin_has_gs_keys_and_views_the_average():
    from mpgan_amd.step_options import Ema
    ts = _toy_step(Ema(beta=0.9))
    twin = ts.ema_generator()
    assert type(twin) is type(ts.G) and twin is not ts.G and twin is ts.ema_generator() and not twin.training and ts.G.training
    assert list(twin.state_dict()) == list(ts.G.state_dict())
    ts.fG.ema.mul_(2.0)                                      # (what the launch does: a write into the flat average)
    for (k, a), b in zip(twin.state_dict().items(), ts.G.state_dict().values()):
        assert torch.equal(a, 2.0 * b), k
    lo, hi = ts.fG.ema.data_ptr(), ts.fG.ema.data_ptr() + 4 * ts.fG.n
    assert all(lo <= p.data_ptr() < hi and p.grad is None for p in twin.parameters())


class NormedG(ToyG):
    """ToyG with what a forward writes behind the optimizer's back: a batch norm's running statistics and a frozen parameter."""

    def __init__(self):
        super().__init__()
        self.bn = torch.nn.BatchNorm1d(3)
        self.u = torch.nn.Parameter(torch.ones(3), requires_grad=False)


def test_every_call_brings_the_twins_buffers_and_frozen_parameters_up_to_date():
    from mpgan_amd import train
    from mpgan_amd.step_options import Ema
    G = NormedG()
    ts = train.TrainStep(G, ToyD(), 4, N, latent=LAT, use_graphs=False, ema=Ema(beta=0.9))
    twin = ts.ema_generator()
    assert list(twin.state_dict()) == list(G.state_dict()) and not twin.u.requires_grad
    with torch.no_grad():
        G.bn.running_mean.add_(0.25)
        G.bn.num_batches_tracked.add_(3)
        G.u.mul_(-2.0)
        G.lin.weight.add_(1.0)                     # (a trained parameter: the twin's is the average, not G's)
    assert not torch.equal(twin.bn.running_mean, G.bn.running_mean) and twin.u.data_ptr() != G.u.data_ptr()
    assert ts.ema_generator() is twin and not twin.training
    assert torch.equal(twin.bn.running_mean, G.bn.running_mean) and int(twin.bn.num_batches_tracked) == 3
    assert torch.equal(twin.u, G.u) and not torch.equal(twin.lin.weight, G.lin.weight)
    assert ts.fG.n == sum(p.numel() for p in G.parameters() if p.requires_grad) == ts.fG.ema.numel()


def test_optimizer_file_carries_the_step_word(tmp_path):
    from mpgan_amd.step_options import Ema
    ts = _toy_step(Ema(beta=0.9, start=2, warmup=True))
    ts.fG.ema.add_(1.0)
    ts.fG.ema_state.copy_(torch.tensor([7, 0], dtype=torch.int64).to(torch.uint32))
    _, sd = ts.optimizer_state_dicts()
    assert sd["param_groups"][0]["mpgan_amd_ema"] == {"t": 7, "beta": float(F32(0.9)), "start": 2, "warmup": True}
    path = str(tmp_path / "G_optim.pt")
    torch.save(sd, path)
    again = _toy_step(Ema(beta=0.9, start=2, warmup=True), seed=5)
    again.fG.load_state_dict(torch.load(path, weights_only=False))
    assert again.fG.ema_state.tolist() == [7, 0] and torch.equal(again.fG.ema, again.fG.flat)    # (until load_ema: the weights)
    # a file without the key: the reference's own, or one written by a step without the average
    del sd["param_groups"][0]["mpgan_amd_ema"]
    again.fG.ema.add_(1.0)
    again.fG.load_state_dict(sd)
    assert again.fG.ema_state.tolist() == [0, 0] and torch.equal(again.fG.ema, again.fG.flat)
    # ... and a step without the average reads a file that has the key
    _toy_step(None).fG.load_state_dict(torch.load(path, weights_only=False))
    # torch.optim's own loader carries the unknown key along
    opt = torch.optim.RMSprop(ToyG().parameters(), lr=1e-2)
    opt.load_state_dict(torch.load(path, weights_only=False))
    assert opt.state_dict()["param_groups"][0]["mpgan_amd_ema"]["t"] == 7


def test_save_models_and_load_ema_round_trip(tmp_path):
    from mpgan_amd import checkpoint as ck
    from mpgan_amd.step_options import Ema
    tmp = str(tmp_path / "models")
    ts = _toy_step(Ema(beta=0.9))
    ts.fG.ema.copy_(torch.arange(ts.fG.n, dtype=torch.float32) / 7)
    ts.fG.ema_state.copy_(torch.tensor([3, 0], dtype=torch.int64).to(torch.uint32))
    ck.save_models(ts.D, ts.G, ts.fD, ts.fG, tmp, 4, G_ema=ts.ema_generator())
    assert sorted(os.listdir(tmp)) == ["D_4.pt", "D_optim_4.pt", "G_4.pt", "G_ema_4.pt", "G_optim_4.pt"]
    # a plain generator state dict: any generator module loads it
    G = ToyG()
    G.load_state_dict(torch.load(os.path.join(tmp, "G_ema_4.pt")))
    assert torch.equal(torch.cat([p.reshape(-1) for p in G.parameters()]), ts.fG.ema)
    G2 = ToyG()
    assert ck.load_ema(G2, tmp, 4) is True
    assert all(torch.equal(a, b) for a, b in zip(G2.state_dict().values(), G.state_dict().values()))
    # into a fresh step: the weights, the optimizer files, then the average
    again = _toy_step(Ema(beta=0.9), seed=9)
    ck.load_models(again.D, again.G, tmp, 4)
    ck.load_optimizers(again.fD, again.fG, tmp, 4)
    assert torch.equal(again.fG.flat, ts.fG.flat) and torch.equal(again.fG.ema, again.fG.flat)
    assert ck.load_ema(again, tmp, 4) is True
    assert torch.equal(again.fG.ema, ts.fG.ema) and again.fG.ema_state.tolist() == [3, 0]
    assert torch.equal(again.fG.flat, ts.fG.flat)                      # (the weights are not the average's to touch)
    # without the file: the restart of a file without the key
    os.remove(os.path.join(tmp, "G_ema_4.pt"))
    again.fG.ema.add_(1.0)
    assert ck.load_ema(again, tmp, 4) is False
    assert torch.equal(again.fG.ema, again.fG.flat) and again.fG.ema_state.tolist() == [0, 0]
    assert ck.load_ema(ToyG(), tmp, 4) is False
    # save_models without the twin writes the reference's four files
    ck.save_models(ts.D, ts.G, ts.fD, ts.fG, str(tmp_path / "plain"), 1)
    assert sorted(os.listdir(str(tmp_path / "plain"))) == ["D_1.pt", "D_optim_1.pt", "G_1.pt", "G_optim_1.pt"]


def test_latest_epoch_ignores_the_averaged_generators_files(tmp_path):
    from mpgan_amd import checkpoint as ck
    tmp = str(tmp_path)
    for name in ("D_3.pt", "G_3.pt", "D_optim_3.pt", "G_optim_3.pt", "G_ema_3.pt"):
        open(os.path.join(tmp, name), "w").close()
    assert ck.latest_epoch(tmp) == 3
    for name in ("G_ema_9.pt", "G_9.pt", "G_ema_12.pt"):      # (no D_9.pt: an averaged generator never stands in for a network)
        open(os.path.join(tmp, name), "w").close()
    assert ck.latest_epoch(tmp) == 3
    open(os.path.join(tmp, "D_9.pt"), "w").close()
    assert ck.latest_epoch(tmp) == 9
