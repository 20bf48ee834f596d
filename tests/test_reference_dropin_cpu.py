"""Drop-in boundary, checked against records of the reference stored under tests/golden/
(tests/gen_golden.py: fixtures, generated where the reference can be imported):

* the reference's ``setup_training`` with ``install_as_reference_packages()`` in force builds OUR classes, with its own
  default arguments (reference_setup.json: class, structure and state-dict shapes of the four networks it built), and the
  import line of the reference's ``train.py:7`` resolves;
* the published ``trained_models/mp_g`` generator checkpoint loads (all keys matched);
* ``augment`` / ``mask_manual`` reproduce the reference functions under the same RNG state (reference_augment.npz).
"""
import json
import os
import sys
import types

import torch

from conftest import GOLDEN, load_golden
from test_oracle_golden import published_weights


def test_train_py_import_line_resolves():
    """``from mpgan import augment, mask_manual`` (reference train.py:7) with our package installed."""
    import mpgan_amd
    saved = {k: sys.modules.get(k) for k in ("mpgan", "gapt")}
    try:
        mpgan_amd.install_as_reference_packages()
        ns = {}
        exec("from mpgan import augment, mask_manual\nfrom mpgan import MPGenerator, MPDiscriminator, MPNet, MPLayer, LinearNet\n"
             "from gapt import GAPT_G, GAPT_D, MAB, SAB, ISAB, PMA, LinearNet as L2", ns)
        assert isinstance(ns["augment"], types.ModuleType) and callable(ns["augment"].augment)
        assert callable(ns["mask_manual"])
        assert ns["MPGenerator"].__module__.startswith("mpgan_amd")
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def test_reference_setup_builds_our_classes_and_loads_published_weights():
    """What the reference's ``setup_mpgan`` / ``setup_gapt`` built from their default arguments with our packages installed
    (recorded) is what ``train.default_mpgan`` / ``default_gapt`` build: the same classes, module structure and state-dict
    shapes; the published generator checkpoint loads into it with every key matched."""
    import mpgan_amd
    from mpgan_amd import train
    with open(os.path.join(GOLDEN, "reference_setup.json")) as f:
        rec = json.load(f)
    G, D = train.default_mpgan(30, device="cpu")
    Gg, Dg = train.default_gapt(30, device="cpu")
    assert type(G) is mpgan_amd.MPGenerator and type(D) is mpgan_amd.MPDiscriminator
    assert type(Gg) is mpgan_amd.GAPT_G and type(Dg) is mpgan_amd.GAPT_D
    for key, m in (("mpgan_G", G), ("mpgan_D", D), ("gapt_G", Gg), ("gapt_D", Dg)):
        r = rec[key]
        assert f"{type(m).__module__}.{type(m).__qualname__}" == r["class"], key
        assert repr(m) == r["repr"], key
        assert {k: list(v.shape) for k, v in m.state_dict().items()} == r["state_dict"], key
    res = G.load_state_dict(published_weights("g"))
    assert not res.missing_keys and not res.unexpected_keys


class _Args:
    device = "cpu"
    num_hits = 30
    aug_r90 = aug_f = aug_t = aug_s = True
    translate_ratio = 0.125
    translate_pn_ratio = 0.05
    scale_sd = 0.125
    mask_real_only = False
    mask_exp = False


def test_augment_and_mask_manual_match_reference():
    from mpgan_amd.mpgan import augment as ours, mask_manual as ours_mask
    ref = load_golden("reference_augment.npz")
    args = _Args()
    X = torch.from_numpy(ref["X"])
    for p in (0.3, 0.8, 1):
        torch.manual_seed(11)
        a = ours.augment(args, X.clone(), p)
        assert torch.allclose(a, torch.from_numpy(ref[f"augment_p{p}"]), atol=1e-6), p
    for fn in ("rand_flip", "rand_90_rotation", "rand_translate", "rand_translate_per_node", "rand_scale"):
        torch.manual_seed(5)
        a = getattr(ours, fn)(args, X.clone())
        assert torch.allclose(a, torch.from_numpy(ref[fn]), atol=1e-6), fn
    for tag, flags in (("plain", {}), ("mask_exp", {"mask_exp": True}), ("mask_real_only", {"mask_real_only": True})):
        a2 = _Args()
        for k, v in flags.items():
            setattr(a2, k, v)
        assert torch.equal(ours_mask(a2, X, -0.2), torch.from_numpy(ref[f"mask_manual_{tag}"])), flags


def test_augment_without_reference():
    """Shape / invariants on their own (runs everywhere)."""
    from mpgan_amd.mpgan import augment as A, mask_manual
    args = _Args()
    torch.manual_seed(0)
    X = torch.randn(8, 30, 4)
    Y = A.augment(args, X, 0.5)
    assert Y.shape == X.shape and torch.equal(Y[..., 2:], X[..., 2:])      # pT and mask untouched
    assert torch.equal(A.augment(args, X, 1), X)                           # the reference's p == 1 shortcut
    r = A.rand_90_rotation(args, X)
    assert torch.allclose((r[..., :2] ** 2).sum(-1), (X[..., :2] ** 2).sum(-1), atol=1e-5)
    m = mask_manual(args, X[..., :3], 0.0)
    assert m.shape == (8, 30, 4) and set(m[..., 3].unique().tolist()) <= {-0.5, 0.5}
