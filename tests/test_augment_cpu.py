"""CPU: the augmentation's C ABI, the torch statement of its per-jet map against the stages of ``mpgan.augment``, and the
host logic of ``TrainStep(augment=...)`` on toy networks (torch's generator stands in for the device stream there)."""
import os
import re
from types import SimpleNamespace

import pytest
import torch

from test_dist_cpu import ToyG, ToyD, _torch_rmsprop, _inputs, N, LAT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mpgan_amd.h")


def test_symbols_are_exported_with_the_documented_signatures():
    import ctypes as C
    from mpgan_amd import _lib, ops
    lib = _lib.lib()
    txt = open(HEADER).read()
    for name, n_args in (("mpg_augment", 15), ("mpg_augment_bwd", 9)):
        assert hasattr(lib, name), name
        decl = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", txt, flags=re.M | re.S).group(1)
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == n_args == len(decl.split(",")), name
        assert args[-1] is C.c_void_p and "void* stream" in decl.split(",")[-1]
    decl = re.search(r"^int\s+mpg_augment\s*\(([^;]*)\);", txt, flags=re.M | re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in decl.split(",")] == [
        "x", "y", "jet_stride", "ld", "F", "B", "N", "seed", "tag", "p", "flags", "translate_ratio", "scale_sd", "params", "stream"]
    defs = dict(re.findall(r"^#define\s+(MPG_AUG_\w+)\s+(\d+)\s*$", txt, flags=re.M))
    assert {k: int(v) for k, v in defs.items()} == {"MPG_AUG_R90": ops.AUG_R90, "MPG_AUG_FLIP": ops.AUG_FLIP,
                                                    "MPG_AUG_TRANSLATE": ops.AUG_TRANSLATE, "MPG_AUG_SCALE": ops.AUG_SCALE}
    assert (ops.AUG_R90, ops.AUG_FLIP, ops.AUG_TRANSLATE, ops.AUG_SCALE) == (1, 2, 4, 8)
    assert ops.augment_flags(aug_r90=True, aug_s=True) == 9 and ops.augment_flags() == 0
    # (the site tags: test_cabi_cpu.py::test_tag_table)


ARGS = SimpleNamespace(device="cpu", aug_r90=True, aug_f=True, aug_t=True, aug_s=True, translate_ratio=0.3, scale_sd=0.2)


@pytest.fixture
def f64():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)     # (the stages' draws, their sin / cos and the jets: all fp64)
    yield
    torch.set_default_dtype(old)


def _ident(B):
    return torch.tensor([1.0, 0, 0, 1, 0, 0]).repeat(B, 1)


def _r90(q, k):
    """A <- R^k A, t <- R^k t with R = [[0, -1], [1, 0]]."""
    c = torch.tensor([1.0, 0, -1, 0])[k].reshape(-1, 1)
    s = torch.tensor([0.0, 1, 0, -1])[k].reshape(-1, 1)
    top, bot = q[:, (0, 1, 4)], q[:, (2, 3, 5)]
    nt, nb = c * top - s * bot, s * top + c * bot
    return torch.stack((nt[:, 0], nt[:, 1], nb[:, 0], nb[:, 1], nt[:, 2], nb[:, 2]), 1)


def _flip(q, sign):
    return q * torch.stack((sign[:, 0], sign[:, 0], sign[:, 1], sign[:, 1], sign[:, 0], sign[:, 1]), 1)


def _translate(q, shift):
    return q + torch.cat((torch.zeros(q.shape[0], 4), shift), 1)


def _scale(q, f):
    return q * f.reshape(-1, 1)


def _law():
    return torch.distributions.log_normal.LogNormal(torch.tensor([0.0]), torch.tensor([ARGS.scale_sd]))


def test_reference_statement_reproduces_each_stage(f64):
    """Each stage of mpgan.augment under a known generator state against ``augment_apply_reference`` with the map built by hand
    from the stage's own draws (drawn again from the same state)."""
    from mpgan_amd import ops
    from mpgan_amd.mpgan import augment as A
    B = 33
    X = torch.randn(B, 7, 4, generator=torch.Generator().manual_seed(1))
    cases = (
        (A.rand_90_rotation, lambda: _r90(_ident(B), torch.floor(torch.rand(B, 1, 1) * 4).long().reshape(-1))),
        (A.rand_flip, lambda: _flip(_ident(B), (torch.round(torch.rand(B, 1, 2)) * 2 - 1).reshape(B, 2))),
        (A.rand_translate, lambda: _translate(_ident(B), ((torch.rand(B, 1, 2) - 0.5) * ARGS.translate_ratio).reshape(B, 2))),
        (A.rand_scale, lambda: _scale(_ident(B), _law().sample((B, 1)).reshape(-1))),
    )
    for stage, by_hand in cases:
        torch.manual_seed(11)
        want = stage(ARGS, X)
        torch.manual_seed(11)
        q = by_hand()
        assert not torch.equal(q, _ident(B))
        got = ops.augment_apply_reference(X, q)
        assert got.dtype == torch.float64 and float((got - want).abs().max()) < 1e-12, stage.__name__
        assert torch.equal(got[..., 2:], X[..., 2:])


@pytest.mark.parametrize("p", [0.5, 0.25, 1.0])
def test_reference_statement_reproduces_the_composition(f64, p):
    """``augment`` (rotation, flip, translation, scaling; each mixed in per jet with probability p, a stage's own draw in front
    of its mix draw) against ONE map per jet composed by hand from the same decisions -- p == 1 takes nothing."""
    from mpgan_amd import ops
    from mpgan_amd.mpgan import augment as A
    B = 64
    X = torch.randn(B, 5, 3, generator=torch.Generator().manual_seed(2))
    torch.manual_seed(5)
    want = A.augment(ARGS, X, p)
    torch.manual_seed(5)
    q = _ident(B)

    def mix(new):
        if p == 1:
            return q
        take = (torch.rand(B, 1, 1) < p).reshape(-1, 1)
        return torch.where(take, new, q)
    q = mix(_r90(q, torch.floor(torch.rand(B, 1, 1) * 4).long().reshape(-1)))
    q = mix(_flip(q, (torch.round(torch.rand(B, 1, 2)) * 2 - 1).reshape(B, 2)))
    q = mix(_translate(q, ((torch.rand(B, 1, 2) - 0.5) * ARGS.translate_ratio).reshape(B, 2)))
    q = mix(_scale(q, _law().sample((B, 1)).reshape(-1)))
    if p == 1:
        assert torch.equal(q, _ident(B)) and torch.equal(want, X)
    else:
        assert int((q != _ident(B)).any(1).sum()) > B // 2
    got = ops.augment_apply_reference(X, q)
    assert float((got - want).abs().max()) < 1e-12


class RecordingD(ToyD):
    def __init__(self):
        super().__init__()
        self.seen = []

    def forward(self, x, labels=None):      # (gradient_penalty calls D(interpolated) without labels, train.py:301)
        self.seen.append(x.detach().clone())
        return super().forward(x, 0.0 if labels is None else labels)


def _toy_step(augment, B=4, **kw):
    from mpgan_amd import train
    torch.manual_seed(3)
    G, D = ToyG(), RecordingD()
    data, labels, nD, nG = _inputs(B)
    ts = train.TrainStep(G, D, B, N, latent=LAT, lr_disc=1e-2, lr_gen=2e-2, use_graphs=False, **kw) if augment == "absent" else \
        train.TrainStep(G, D, B, N, latent=LAT, lr_disc=1e-2, lr_gen=2e-2, use_graphs=False, augment=augment, **kw)
    ts.set_batch(data, labels)
    ts.fixed_noise = (nD, nG)
    return ts, G, D, data, labels, nD, nG


def test_cpu_step_feeds_D_the_real_batch_as_it_is_and_the_generated_batch_augmented(monkeypatch):
    from mpgan_amd import train
    from mpgan_amd.mpgan import augment as A
    monkeypatch.setattr(train.FlatParams, "step", _torch_rmsprop)
    cfg = train.Augment(aug_r90=True, aug_f=True, aug_t=True, aug_s=True, translate_ratio=0.3, scale_sd=0.2, aug_prob=0.5)
    ts, G, D, data, labels, nD, nG = _toy_step(cfg)
    assert ts.aug is not None and not ts._bridge()
    with torch.no_grad():
        fake_D, fake_G = G(nD, labels), G(nG, labels)      # (G moves only at the end of the iteration)
    torch.manual_seed(21)
    ts.step()
    assert len(D.seen) == 2                                   # train_D on real + generated, train_G on generated
    torch.manual_seed(21)                                     # the step's draws again: train_D's augmentation, then train_G's
    args = SimpleNamespace(device="cpu", **{k: getattr(cfg, k) for k in ("aug_r90", "aug_f", "aug_t", "aug_s", "translate_ratio", "scale_sd")})
    want_D, want_G = A.augment(args, fake_D, 0.5), A.augment(args, fake_G, 0.5)
    assert torch.equal(D.seen[0][:4], data)                   # D(real): train.py:425 runs before the augmentation
    assert torch.equal(D.seen[0][4:], want_D) and not torch.equal(want_D, fake_D)
    assert torch.equal(D.seen[1], want_G) and not torch.equal(want_G, fake_G)
    assert torch.equal(ts.data, data)
    # the probability is the step's to change; at 1 nothing is taken (rand_mix)
    ts.set_aug_prob(1.0)
    D.seen.clear()
    with torch.no_grad():
        fake_D = G(nD, labels)
    ts.step()
    assert torch.equal(D.seen[0][4:], fake_D)


def test_cpu_step_hands_the_gradient_penalty_the_augmented_real_batch(monkeypatch):
    from mpgan_amd import train
    monkeypatch.setattr(train.FlatParams, "step", _torch_rmsprop)
    cfg = train.Augment(aug_t=True, translate_ratio=0.3, aug_prob=0.5)
    ts, G, D, data, *_ = _toy_step(cfg, loss="w", gp_lambda=10.0)
    seen = []
    inner = ts.gradient_penalty
    ts.gradient_penalty = lambda real, fake: (seen.append(real.clone()), inner(real, fake))[1]
    torch.manual_seed(8)
    ts.step()
    real = seen[0]
    moved = (real != data).reshape(4, -1).any(1)
    assert bool(moved.any()) and not bool(moved.all())       # (p = 0.5 over 4 jets under this seed: some taken, some not)
    assert torch.equal(real[..., 2:], data[..., 2:]) and torch.equal(D.seen[0][:4], data)
    shift = (real - data)[..., :2]
    assert float((shift - shift[:, :1]).abs().max()) < 1e-6 and float(shift.abs().max()) <= 0.15 + 1e-6   # one shift per jet


def test_augment_none_changes_nothing_on_cpu(monkeypatch):
    from mpgan_amd import train
    monkeypatch.setattr(train.FlatParams, "step", _torch_rmsprop)
    res = []
    for augment in ("absent", None, train.Augment(aug_prob=0.5)):      # (the last: every switch off)
        ts, *_ = _toy_step(augment)
        assert ts.aug is None
        torch.manual_seed(4)
        rng = torch.get_rng_state()
        for _ in range(3):
            ts.step()
        assert torch.equal(torch.get_rng_state(), rng)          # (no draw made)
        res.append((ts.fD.flat.clone(), ts.fG.flat.clone(), float(ts.D_loss), float(ts.G_loss)))
    for r in res[1:]:
        assert torch.equal(r[0], res[0][0]) and torch.equal(r[1], res[0][1]) and r[2:] == res[0][2:]
    with pytest.raises(RuntimeError):
        _toy_step(None)[0].set_aug_prob(0.5)
