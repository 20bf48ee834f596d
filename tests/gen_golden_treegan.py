"""Fixtures of the TreeGAN generator, from the reference's own ``TreeGANG`` (``ext_models/ext_models.py:211-333``):

  tests/golden/treegan.npz                  features [5, 7, 4, 6, 3], degrees [3, 1, 2, 2], support 3 at B = 4 in fp64: state dict,
                                            noise, output, noise gradient and every parameter gradient for a stored cotangent
  tests/golden/treegan_manifest.json        state-dict shapes at the default [96, 64, 64, 64, 64, 3] / [2, 2, 2, 2, 2] / 10
  tests/golden/published_treegan_g_weights*.npz   the published generator's state dict (trained_models/treeganfc_g), and
  tests/golden/published_treegan_g.npz      the reference's fp64 output for 8 jets on stored noise

The seed of ``treegan.npz`` is the one of ``range(200)`` that keeps every LeakyReLU pre-activation (the branch product's and the
layer's) furthest from zero relative to its layer's largest: the smallest |z| / max|z| over all of them is the largest.  That margin
is stored.  The last layer's ``bias`` gets no gradient in the reference (its forward never reads it): no ``grad.`` entry.

    python tests/gen_golden_treegan.py        (needs the reference checkout: MPGAN_REFERENCE)
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from gen_golden import OUT, REF, save_parts  # noqa: E402
from gen_golden_baselines import reference_module  # noqa: E402
import treegan_ref as R  # noqa: E402

B = 4
SMALL = dict(features=[5, 7, 4, 6, 3], degrees=[3, 1, 2, 2], support=3)
DEFAULT = dict(features=[96, 64, 64, 64, 64, 3], degrees=[2, 2, 2, 2, 2], support=10)


def build(ref, seed):
    torch.manual_seed(seed)
    net = ref.TreeGANG(SMALL["features"], SMALL["degrees"], SMALL["support"]).double()
    g = torch.Generator().manual_seed(seed)
    noise = torch.randn(B, 1, SMALL["features"][0], generator=g, dtype=torch.float64)
    cot = torch.randn(B, int(np.prod(SMALL["degrees"])), SMALL["features"][-1], generator=g, dtype=torch.float64)
    return net, noise, cot


def margin(sd, noise):
    """The smallest |z| / max|z| over every LeakyReLU pre-activation of the restated net."""
    n = len(SMALL["degrees"])
    probe, levels = {}, [noise]
    for d in range(n):
        levels.append(R.collapsed(levels, R.layer_weights(sd, d, act=d < n - 1), probe=probe)[0])
    return min(float(z.abs().min() / z.abs().max()) for z in probe["z"])


def main():
    if not os.path.isdir(REF):
        print(f"reference not found at {REF}; nothing generated")
        return 0
    ref = reference_module()
    os.makedirs(OUT, exist_ok=True)

    best = None
    for seed in range(200):
        net, noise, _ = build(ref, seed)
        m = margin(dict(net.state_dict()), noise)
        if best is None or m > best[0]:
            best = (m, seed)
    m, seed = best
    print("seed", seed, "min |z| / max|z|", m)
    net, noise, cot = build(ref, seed)
    xi = noise.clone().requires_grad_(True)
    out = net([xi])                  # (the reference appends to the list it is given: a fresh one)
    (out * cot).sum().backward()
    arrays = {"seed": np.array(seed), "margin_z": np.array(m), "noise": noise.numpy(), "cot": cot.numpy(),
              "out": out.detach().numpy(), "dnoise": xi.grad.numpy()}
    for k, p in net.named_parameters():
        arrays[f"sd.{k}"] = p.detach().numpy()
        if p.grad is not None:
            arrays[f"grad.{k}"] = p.grad.numpy()
    np.savez_compressed(os.path.join(OUT, "treegan.npz"), **arrays)

    shapes = {k: list(v.shape) for k, v in ref.TreeGANG(DEFAULT["features"], DEFAULT["degrees"], DEFAULT["support"]).state_dict().items()}
    with open(os.path.join(OUT, "treegan_manifest.json"), "w") as f:
        json.dump({"args": DEFAULT, "small": SMALL, "shapes": shapes}, f, indent=1, sort_keys=True)
        f.write("\n")

    sd = torch.load(os.path.join(REF, "trained_models", "treeganfc_g", "G_best_epoch.pt"), map_location="cpu")
    G = ref.TreeGANG(DEFAULT["features"], DEFAULT["degrees"], DEFAULT["support"])
    print("treeganfc_g", G.load_state_dict(sd), sum(v.numel() for v in sd.values()), "floats")
    save_parts("published_treegan_g_weights", {k: v.numpy() for k, v in sd.items()})
    noise = torch.randn(8, 1, DEFAULT["features"][0], generator=torch.Generator().manual_seed(0)) * 0.2
    with torch.no_grad():
        out = G.double()([noise.double()])
    np.savez_compressed(os.path.join(OUT, "published_treegan_g.npz"), noise=noise.numpy(), out=out.numpy())
    return 0


if __name__ == "__main__":
    sys.exit(main())
