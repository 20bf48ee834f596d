"""Fixtures of the set-pooling baselines, from the reference's own classes (``ext_models/ext_models.py``: rGANG, rGAND, PointNetMixD):

  tests/golden/baselines.npz              rGAND (sfc [32, 48, 96], fc [40, 24]) and PointNetMixD (pointfc [32, 48, 160], fc [64],
                                          mask) at B = 4, N = 30 in fp64: state dict, input, output, dx and every parameter gradient
                                          for a stored cotangent; PointNet-Mix jets with 30, 20, 7 and 1 real particles
  tests/golden/baselines_manifest.json    state-dict shapes of the three classes at their default widths
  tests/golden/published_fc_g_weights.npz the published FC generator's state dict (trained_models/fc_g), and
  tests/golden/published_fc_g.npz         the reference's output for 8 jets on stored noise

The reference's module imports ``torch_geometric`` and ``torch_cluster`` at its top; the three classes use neither, so stubs stand in
for the two libraries.  The seed of ``baselines.npz`` is the one of ``range(200)`` that keeps the decisions of the nets furthest from
their kinks: the smaller of (a) the smallest |z| / max|z| over every LeakyReLU layer's pre-activations and (b) the smallest top-two
gap of the pooled layer per (jet, channel) relative to max|y| is the largest.  Masked rows of a jet are identical and count as ONE
row in (b).  Both margins are stored.

    python tests/gen_golden_baselines.py        (needs the reference checkout: MPGAN_REFERENCE)
"""
import copy
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from gen_golden import OUT, REF, save_parts  # noqa: E402
import baselines_ref as R  # noqa: E402

B, N = 4, 30
REAL = (30, 20, 7, 1)
SMALL = dict(latent_dim=16, rgang_fc=[24, 32], rgand_sfc=[32, 48, 96], rgand_fc=[40, 24], pointnetd_pointfc=[32, 48, 160],
             pointnetd_fc=[64], num_hits=N, node_feat_size=3, leaky_relu_alpha=0.2, mask=True)
DEFAULT = dict(latent_dim=128, rgang_fc=[64, 128], rgand_sfc=[64, 128, 256, 256, 512], rgand_fc=[128, 64],
               pointnetd_pointfc=[64, 128, 1024], pointnetd_fc=[512], num_hits=N, node_feat_size=3, leaky_relu_alpha=0.2, mask=True)


def reference_module():
    for name in ("torch_geometric", "torch_geometric.nn", "torch_cluster"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["torch_geometric"].nn = sys.modules["torch_geometric.nn"]
    sys.modules["torch_geometric.nn"].NNConv = None
    sys.modules["torch_cluster"].knn_graph = None
    spec = importlib.util.spec_from_file_location("reference_ext_models", os.path.join(REF, "ext_models", "ext_models.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def args_of(d):
    return types.SimpleNamespace(**copy.deepcopy(d))


def inputs(seed):
    g = torch.Generator().manual_seed(seed)
    xr = torch.randn(B, N, 3, generator=g, dtype=torch.float64)
    xp = torch.randn(B, N, 4, generator=g, dtype=torch.float64)
    for b, n in enumerate(REAL):
        xp[b, :, 3] = -0.5
        xp[b, :n, 3] = 0.5
    cot = torch.randn(B, 1, generator=g, dtype=torch.float64)
    return xr, xp, cot


def margins(sd, x, which):
    """(smallest |z| / max|z| over the LeakyReLU layers, smallest top-two gap / max|y| of the pooled layer), identical rows once."""
    probe = {}
    if which == "rgand":
        R.rgand(sd, x, N, 3, probe=probe)
        keep = [list(range(N))] * B
    else:
        R.pointnet_mix(sd, x, N, 3, probe=probe)
        keep = [list(range(min(n + 1, N))) for n in REAL]      # the real rows and ONE of the masked ones
    mz = min(float(z.abs().min() / z.abs().max()) for z in probe["z"])
    y = probe["pool_y"]
    gap = min(float(R.top_two_gap(y[b:b + 1, rows]).min()) for b, rows in enumerate(keep)) / float(y.abs().max())
    return mz, gap


def build(ref, seed):
    torch.manual_seed(seed)
    nets = {"rgand": ref.rGAND(args_of(SMALL)).double(), "pnet": ref.PointNetMixD(args_of(SMALL)).double()}
    return nets, inputs(seed)


def main():
    if not os.path.isdir(REF):
        print(f"reference not found at {REF}; nothing generated")
        return 0
    ref = reference_module()
    os.makedirs(OUT, exist_ok=True)

    best = None
    for seed in range(200):
        nets, (xr, xp, _) = build(ref, seed)
        m = [margins(dict(nets["rgand"].state_dict()), xr, "rgand"), margins(dict(nets["pnet"].state_dict()), xp, "pnet")]
        score = min(min(a) for a in m)
        if best is None or score > best[0]:
            best = (score, seed, min(a[0] for a in m), min(a[1] for a in m))
    _, seed, mz, gap = best
    print("seed", seed, "min |z| / max|z|", mz, "min top-two gap / max|y|", gap)
    nets, (xr, xp, cot) = build(ref, seed)
    arrays = {"seed": np.array(seed), "margin_z": np.array(mz), "margin_gap": np.array(gap), "cot": cot.numpy(),
              "real": np.array(REAL)}
    for name, x in (("rgand", xr), ("pnet", xp)):
        net = nets[name]
        xi = x.clone().requires_grad_(True)
        out = net(xi.clone())       # (the reference's PointNetMixD writes into the tensor it is given)
        (out * cot).sum().backward()
        arrays[f"{name}.x"], arrays[f"{name}.out"], arrays[f"{name}.dx"] = x.numpy(), out.detach().numpy(), xi.grad.numpy()
        for k, p in net.named_parameters():
            arrays[f"{name}.sd.{k}"], arrays[f"{name}.grad.{k}"] = p.detach().numpy(), p.grad.numpy()
    np.savez_compressed(os.path.join(OUT, "baselines.npz"), **arrays)

    manifest = {}
    for cls in ("rGANG", "rGAND", "PointNetMixD"):
        manifest[cls] = {k: list(v.shape) for k, v in getattr(ref, cls)(args_of(DEFAULT)).state_dict().items()}
    with open(os.path.join(OUT, "baselines_manifest.json"), "w") as f:
        json.dump({"args": DEFAULT, "shapes": manifest}, f, indent=1, sort_keys=True)
        f.write("\n")

    sd = torch.load(os.path.join(REF, "trained_models", "fc_g", "G_best_epoch.pt"), map_location="cpu")
    G = ref.rGANG(args_of(DEFAULT))
    print("fc_g", G.load_state_dict(sd))
    save_parts("published_fc_g_weights", {k: v.numpy() for k, v in sd.items()})
    noise = torch.randn(8, DEFAULT["latent_dim"], generator=torch.Generator().manual_seed(0)) * 0.2
    with torch.no_grad():
        out = G.double()(noise.double())
    np.savez_compressed(os.path.join(OUT, "published_fc_g.npz"), noise=noise.numpy(), out=out.numpy())
    return 0


if __name__ == "__main__":
    sys.exit(main())
