"""CPU: label smoothing / label noise of calc_D_loss -- the C ABI of ``mpg_label_targets``, ``train.effective_targets`` + ``train.d_loss``
against calc_D_loss EXECUTED from the reference's source (tests/golden/label_losses.npz, tests/gen_golden_labels.py), and the host
logic of ``TrainStep(label_smoothing=..., label_noise=...)`` on toy networks (torch's generator stands in for the device stream)."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_dist_cpu import ToyG, ToyD, _torch_rmsprop, _inputs, N, LAT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mpgan_amd.h")

CASES = ("ls_smooth", "ls_noise", "ls_smooth_noise", "og_noise")


def test_symbol_is_exported_with_the_documented_signature_and_a_tag_family_of_its_own():
    import ctypes as C
    from mpgan_amd import _lib, ops
    lib = _lib.lib()
    txt = open(HEADER).read()
    assert hasattr(lib, "mpg_label_targets")
    decl = re.search(r"^int\s+mpg_label_targets\s*\(([^;]*)\);", txt, flags=re.M | re.S).group(1)
    res, args = _lib.SIGNATURES["mpg_label_targets"]
    assert res is C.c_int and len(args) == 9 == len(decl.split(","))
    assert [a.split()[-1].lstrip("*") for a in decl.split(",")] == ["B", "smoothing", "noise", "seed", "tag", "targets", "extra", "drawn",
                                                                    "stream"]
    assert args[:3] == [C.c_int, C.c_int, C.c_float] and args[4] is C.c_uint32 and args[-1] is C.c_void_p
    tag = int(re.search(r"^#define\s+MPG_LABEL_TAG\s+(0x[0-9A-Fa-f]+)\s*$", txt, flags=re.M).group(1), 16)
    assert tag == ops.LABEL_TAG == 0x4C000000
    # the head's struct ends with the two fields the launch feeds
    assert [f[0] for f in _lib.MpgDiscHead._fields_[-2:]] == ["targets", "loss_extra"]
    # (that the family stays clear of every other one: test_cabi_cpu.py::test_tag_table)


def _golden_case(g, name):
    t = lambda k: torch.from_numpy(np.asarray(g[f"{name}_{k}"], dtype=np.float64))
    return str(g[f"{name}_loss"]), bool(g[f"{name}_smoothing"]), t("out_r"), t("out_f"), t("Y_real"), t("Y_fake")


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("name", CASES)
def test_effective_targets_and_d_loss_reproduce_the_reference(name):
    """Values and gradients with respect to D's outputs, fp64, 1e-12 relative: the broadcast quirk of ``ls`` + smoothing included."""
    from mpgan_amd import train
    g = load_golden("label_losses.npz")
    assert sorted(CASES) == list(g["cases"])
    loss, smoothing, out_r, out_f, y_r, y_f = _golden_case(g, name)
    B = int(g["B"])
    assert out_r.shape == (B, 1) and y_r.shape == (B,)
    t, extra = train.effective_targets(y_r, y_f, smoothing)
    assert t.dtype == torch.float64 and t.shape == (2 * B,) and extra.shape == ()
    if not smoothing:
        assert float(extra) == 0.0 and torch.equal(t, torch.cat([y_r, y_f]))
        assert set(t.tolist()) <= {0.0, 1.0} and (bool((y_r == 0).any()) or bool((y_f == 1).any()))     # (something flipped)
    out = torch.cat([out_r, out_f]).reshape(-1).requires_grad_(True)
    D = train.d_loss(loss, out, B, t, extra)
    D.backward()
    got, want = float(D.detach()), float(g[f"{name}_D"])
    print(name, "D", got, "golden", want, "rel", abs(got - want) / abs(want))
    assert abs(got - want) <= 1e-12 * abs(want)
    want_g = np.concatenate([g[f"{name}_dD_dr"].reshape(-1), g[f"{name}_dD_df"].reshape(-1)])
    print(name, "grad rel", _rel(out.grad.numpy(), want_g))
    assert _rel(out.grad.numpy(), want_g) <= 1e-12
    assert abs(float(g[f"{name}_Dr"]) + float(g[f"{name}_Df"]) - want) <= 1e-12 * abs(want)     # (D is the two halves' sum)


def test_golden_tells_the_broadcast_rule_from_the_per_jet_rule():
    """``ls`` + smoothing: the per-jet mean_i (out_i - Y_i)^2 is NOT what the reference computes -- it differs by about popvar(Y)."""
    g = load_golden("label_losses.npz")
    _, smoothing, out_r, out_f, y_r, y_f = _golden_case(g, "ls_smooth")
    assert smoothing
    naive = float(((out_r.reshape(-1) - y_r) ** 2).mean() + ((out_f.reshape(-1) - y_f) ** 2).mean())
    want = float(g["ls_smooth_D"])
    print("naive", naive, "golden", want, "popvar", float(y_r.var(unbiased=False) + y_f.var(unbiased=False)))
    assert abs(naive - want) > 1e-6
    assert bool(g["og_smooth_raises_ValueError"]) and "target size" in str(g["og_smooth_message"])


# ---- TrainStep on the CPU ------------------------------------------------------------------------------------------------------
class LabelFreeD(ToyD):
    def forward(self, x, labels=None):      # (gradient_penalty calls D(interpolated) without labels, train.py:301)
        return super().forward(x, 0.0 if labels is None else labels)


def _toy_step(B=4, seed=3, **kw):
    from mpgan_amd import train
    torch.manual_seed(seed)
    G, D = ToyG(), LabelFreeD()
    data, labels, nD, nG = _inputs(B)
    ts = train.TrainStep(G, D, B, N, latent=LAT, lr_disc=1e-2, lr_gen=2e-2, use_graphs=False, **kw)
    ts.set_batch(data, labels)
    ts.fixed_noise = (nD, nG)
    return ts, G, D, data, labels, nD, nG


def _plain_loop(B, steps, smoothing, noise, seed=3, draw_seed=21):
    """train_D / train_G of the reference on the toy networks in plain torch (``ls``): its labels by its four calls, its criterion
    with its shapes (MSELoss of [B, 1] against [B] under smoothing), torch's RMSprop."""
    import warnings
    torch.manual_seed(seed)
    G, D = ToyG(), ToyD()
    data, labels, nD, nG = _inputs(B)
    oD, oG = torch.optim.RMSprop(D.parameters(), lr=1e-2), torch.optim.RMSprop(G.parameters(), lr=2e-2)
    mse = torch.nn.MSELoss()
    torch.manual_seed(draw_seed)
    losses = []
    for _ in range(steps):
        oD.zero_grad()
        out_r = D(data, labels)
        with torch.no_grad():
            fake = G(nD, labels)
        out_f = D(fake, labels)
        if smoothing:
            y_r, y_f = torch.empty(B).uniform_(0.7, 1.2), torch.empty(B).uniform_(0.0, 0.3)
        else:
            y_r, y_f = torch.ones(B, 1), torch.zeros(B, 1)
        if noise:
            y_r[torch.rand(B) < noise] = 0
            y_f[torch.rand(B) < noise] = 1
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            loss = mse(out_r, y_r) + mse(out_f, y_f)
        loss.backward()
        oD.step()
        losses.append(float(loss.detach()))
        oG.zero_grad()
        g_loss = mse(D(G(nG, labels), labels), torch.ones(B, 1))
        g_loss.backward()
        oG.step()
    flat = lambda m: torch.cat([p.detach().reshape(-1) for p in m.parameters()])
    return flat(D), flat(G), losses


@pytest.mark.parametrize("smoothing,noise", [(True, 0.0), (False, 0.4), (True, 0.4)], ids=["smoothing", "noise", "both"])
def test_cpu_step_equals_a_plain_torch_loop_that_makes_the_same_draws(monkeypatch, smoothing, noise):
    from mpgan_amd import train
    monkeypatch.setattr(train.FlatParams, "step", _torch_rmsprop)
    B = 4
    ts, *_ = _toy_step(B, label_smoothing=smoothing, label_noise=noise)
    assert ts.labels_on and ts._route() == "module"
    torch.manual_seed(21)
    got_losses, drawn = [], []
    for _ in range(2):
        ts.step()
        got_losses.append(float(ts.D_loss))
        drawn.append(ts.label_drawn.clone())
    wD, wG, want_losses = _plain_loop(B, 2, smoothing, noise)
    if noise:      # (0.4 over 2 x 2 x 4 labels under this seed: something flipped)
        assert any(bool((d[:B] == 0).any()) or bool((d[B:] == 1).any()) for d in drawn)
    if smoothing:
        assert all(float(d[:B].max()) <= 1.2 and float(d[B:].max()) <= 1.0 for d in drawn) and not torch.equal(drawn[0], drawn[1])
    print("D", float((ts.fD.flat - wD).abs().max()), "G", float((ts.fG.flat - wG).abs().max()), got_losses, want_losses)
    assert float((ts.fD.flat - wD).abs().max()) <= 1e-6 and float((ts.fG.flat - wG).abs().max()) <= 1e-6
    assert all(abs(a - b) <= 1e-6 for a, b in zip(got_losses, want_losses))


def test_validation():
    from mpgan_amd import train
    with pytest.raises(ValueError, match="BCELoss"):
        _toy_step(loss="og", label_smoothing=True)
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match="label_noise"):
            _toy_step(label_noise=bad)
        with pytest.raises(ValueError, match="label_noise"):
            _toy_step(loss="w", label_noise=bad)
    ts, *_ = _toy_step(loss="og", label_noise=1.0)       # (noise alone runs with og; the ends of the range are in it)
    assert ts.labels_on
    assert not _toy_step(label_noise=0.0)[0].labels_on


def _run(steps=3, **kw):
    ts, *_ = _toy_step(**kw)
    torch.manual_seed(4)
    rng = torch.get_rng_state()
    for _ in range(steps):
        ts.step()
    return ts, (ts.fD.flat.clone(), ts.fG.flat.clone(), float(ts.D_loss), float(ts.G_loss)), torch.equal(torch.get_rng_state(), rng)


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2:] == b[2:]


@pytest.mark.parametrize("loss", ["w", "hinge"])
def test_w_and_hinge_ignore_both_options(monkeypatch, loss):
    from mpgan_amd import train
    monkeypatch.setattr(train.FlatParams, "step", _torch_rmsprop)
    _, plain, _ = _run(loss=loss)
    ts, opt, untouched = _run(loss=loss, label_smoothing=True, label_noise=0.3)
    assert not ts.labels_on and not hasattr(ts, "label_targets") and untouched      # (no buffer, no draw)
    assert _same(plain, opt)


def test_options_off_are_the_default_step(monkeypatch):
    from mpgan_amd import train
    monkeypatch.setattr(train.FlatParams, "step", _torch_rmsprop)
    _, plain, _ = _run()
    ts, off, untouched = _run(label_smoothing=False, label_noise=0.0)
    assert not ts.labels_on and not hasattr(ts, "label_targets") and untouched
    assert _same(plain, off)
    _, on, untouched = _run(label_smoothing=True)
    assert not untouched and not _same(plain, on)


def test_options_run_beside_the_gradient_penalty(monkeypatch):
    """``ls`` with gp_lambda > 0 on the toy networks: the labels enter D_loss, the penalty stays what it was on its own."""
    from mpgan_amd import train
    monkeypatch.setattr(train.FlatParams, "step", _torch_rmsprop)
    alpha = torch.rand(4, 1, 1, generator=torch.Generator().manual_seed(2))
    res = {}
    for key, kw in (("plain", {}), ("labels", dict(label_smoothing=True, label_noise=0.3))):
        ts, G, D, data, labels, nD, nG = _toy_step(gp_lambda=10.0, **kw)
        ts.fixed_alpha = alpha
        torch.manual_seed(9)
        ts.step()
        res[key] = (float(ts.D_loss), float(ts.GP), ts)
    assert res["plain"][1] == res["labels"][1] > 0          # (first step: the same weights, the same interpolation)
    ts = res["labels"][2]
    assert ts.labels_on and res["labels"][0] != res["plain"][0] and np.isfinite(res["labels"][0])
    # D_loss is the loss of the labels the step kept, from the outputs of the weights it started from
    torch.manual_seed(3)
    G0, D0 = ToyG(), ToyD()
    data, labels, nD, nG = _inputs(4)
    with torch.no_grad():
        out = torch.cat([D0(data, labels), D0(G0(nD, labels), labels)]).reshape(-1)
        t, extra = train.effective_targets(ts.label_drawn[:4], ts.label_drawn[4:], True)
        want = float(train.d_loss("ls", out, 4, t, extra))
    assert torch.equal(t, ts.label_targets) and abs(res["labels"][0] - want) <= 1e-6


def test_grouped_weight_gradients_never_add_twice_into_one_buffer_in_one_launch():
    """The "module" route with ``batch_real_fake=False`` applies D twice in one backward, so every parameter is the target of two
    queued weight-gradient jobs.  The grouped reduction adds with a plain read and write: ``WgradBatch`` cuts the queue so that no
    launch holds two jobs on the same target -- and leaves a queue without repeats in runs of GROUP_MAX, as before."""
    from mpgan_amd import ops
    W = [torch.zeros(4, 6) for _ in range(13)]
    b = [torch.zeros(4) for _ in range(13)]

    def queue(order):
        wb = ops.WgradBatch()
        for k, col0 in order:
            wb.add(torch.zeros(3, 4), torch.zeros(3, 3), out=W[k], out_col0=col0, bias_out=b[k] if col0 == 0 else None, accumulate=True)
        return wb
    one_pass = [(k, c) for k in range(13) for c in (0, 3)]        # 26 jobs, every (buffer, column block) once
    sizes = [len(g) for g in queue(one_pass)._groups()]
    assert sizes == [16, 10] == [len(one_pass[i:i + ops.GROUP_MAX]) for i in range(0, 26, ops.GROUP_MAX)]
    two_passes = [(k, 0) for k in range(13)] * 2                  # job 13 + k repeats job k: 13 + 3 would share a launch
    wb = queue(two_passes)
    groups = wb._groups()
    assert [len(g) for g in groups] == [13, 13]
    assert [id(j) for g in groups for j in g] == [id(j) for j in wb.jobs]      # (every job once, in the order queued)
    for g in groups:
        targets = [(j[2].data_ptr(), j[3]) for j in g] + [(j[5].data_ptr(), 0) for j in g if j[5] is not None]
        assert len(set(targets)) == len(targets) and len(g) <= ops.GROUP_MAX
    assert queue([])._groups() == []
