"""Fixtures of PCGAN's networks, from the reference's own classes (``ext_models/pcgan_model.py``) in fp64:

  tests/golden/pcgan*.npz                    small nets at B = 4, N = 30 (``NETS`` below): per net ``<net>.sd.<key>`` (fp32 values),
                                             the input(s) ``<net>.x`` (``.x2``), output ``<net>.out``, a stored cotangent
                                             ``<net>.cot`` and for it ``<net>.dx`` (``.dx2``) and ``<net>.grad.<key>``; the
                                             reference ran in fp64 on exactly the stored fp32 weight values
  tests/golden/pcgan_manifest.json           state-dict shapes at the defaults (setup_training.py:684-714) and the small nets' args
  tests/golden/published_pcgan_g_inv_t_weights*.npz   the published inference network of the top-quark data set
                                             (ext_models/pcgan_models/pcgan_G_inv_t.pt: pool max1, x_dim 3, d_dim = z1_dim = 256;
                                             of the three it has the largest weights), and
  tests/golden/published_pcgan_g_inv_t.npz   its fp64 output for 8 stored synthetic jets in the reference's normalisation
                                             (eta_rel, phi_rel in +-0.5 around 0, pT_rel in -0.5 .. 0.5)

    python tests/gen_golden_pcgan.py          (needs the reference checkout: MPGAN_REFERENCE)
"""
import contextlib
import importlib.util
import io
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from gen_golden import OUT, REF, save_parts  # noqa: E402
import pcgan_ref as R  # noqa: E402

B, N = 4, 30
D_DIM, Z1, Z2, LATENT = 40, 24, 10, 16
# name -> (class, constructor arguments)
NETS = {
    "enc_max1": ("G_inv_Tanh", [3, D_DIM, Z1, "max1"]),
    "enc_max": ("G_inv_Tanh", [3, D_DIM, Z1, "max"]),
    "enc_mean": ("G_inv_Tanh", [3, D_DIM, Z1, "mean"]),
    "enc_max1_x4": ("G_inv_Tanh", [4, D_DIM, Z1, "max1"]),
    "encsp_mean": ("G_inv", [3, D_DIM, Z1, "mean"]),
    "dec": ("G", [3, Z1, Z2]),
    "latent_G": ("latent_G", [LATENT, Z1, [32, 48]]),
    "latent_D": ("latent_D", [Z1, [32, 48]]),
}
DEFAULTS = {
    "G_inv_Tanh": [3, 256, 256, "max1"],
    "G": [3, 256, 10],
    "latent_G": [128, 256],
    "latent_D": [256],
}


def reference_module():
    spec = importlib.util.spec_from_file_location("reference_pcgan_model", os.path.join(REF, "ext_models", "pcgan_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def quiet(cls, *args):
    """The reference's constructors print the module."""
    with contextlib.redirect_stdout(io.StringIO()):
        return cls(*args)


def inputs(name, args, g):
    if name.startswith("enc"):
        return [R.negative_jets(B, N, args[0], g)]
    if name == "dec":
        return [torch.randn(B, 1, Z1, generator=g, dtype=torch.float64), torch.randn(B, N, Z2, generator=g, dtype=torch.float64)]
    return [torch.randn(B, args[0], generator=g, dtype=torch.float64)]


def main():
    if not os.path.isdir(REF):
        print(f"reference not found at {REF}; nothing generated")
        return 0
    ref = reference_module()
    os.makedirs(OUT, exist_ok=True)

    arrays = {}
    for seed, (name, (cls, args)) in enumerate(NETS.items()):
        torch.manual_seed(100 + seed)
        net = quiet(getattr(ref, cls), *args)           # fp32 initialisation: the stored weights are fp32 values
        sd32 = {k: v.clone() for k, v in net.state_dict().items()}
        net = net.double()
        g = torch.Generator().manual_seed(200 + seed)
        xs = [x.float().double().requires_grad_(True) for x in inputs(name, args, g)]   # (fp32 values as well)
        out = net(*xs)
        cot = torch.randn(out.shape, generator=g, dtype=torch.float64)
        (out * cot).sum().backward()
        for k, v in sd32.items():
            arrays[f"{name}.sd.{k}"] = v.numpy()
        for tag, x in zip(("x", "x2"), xs):
            arrays[f"{name}.{tag}"] = x.detach().float().numpy()
            arrays[f"{name}.d{tag}"] = x.grad.numpy()
        arrays[f"{name}.out"], arrays[f"{name}.cot"] = out.detach().numpy(), cot.numpy()
        for k, p in net.named_parameters():
            arrays[f"{name}.grad.{k}"] = p.grad.numpy()
    save_parts("pcgan", arrays)       # (the decoder's four 250 x 250 weights and their fp64 gradients: several parts)

    shapes = {cls: {k: list(v.shape) for k, v in quiet(getattr(ref, cls), *args).state_dict().items()} for cls, args in DEFAULTS.items()}
    with open(os.path.join(OUT, "pcgan_manifest.json"), "w") as f:
        json.dump({"args": DEFAULTS, "small": {k: {"class": c, "args": a} for k, (c, a) in NETS.items()}, "shapes": shapes,
                   "B": B, "N": N}, f, indent=1, sort_keys=True)
        f.write("\n")

    sd = torch.load(os.path.join(REF, "ext_models", "pcgan_models", "pcgan_G_inv_t.pt"), map_location="cpu")
    enc = quiet(ref.G_inv_Tanh, *DEFAULTS["G_inv_Tanh"])
    print("pcgan_G_inv_t", enc.load_state_dict(sd), sum(v.numel() for v in sd.values()), "floats, max |w|",
          max(float(v.abs().max()) for v in sd.values()))
    save_parts("published_pcgan_g_inv_t_weights", {k: v.numpy() for k, v in sd.items()})
    g = torch.Generator().manual_seed(0)
    ang = (torch.randn(8, N, 2, generator=g) * 0.1).clamp(-0.5, 0.5)
    pt = torch.rand(8, N, 1, generator=g).pow(4).sort(1, descending=True)[0] - 0.5
    x = torch.cat((ang, pt), 2)
    with torch.no_grad():
        out = enc.double()(x.double())
    np.savez_compressed(os.path.join(OUT, "published_pcgan_g_inv_t.npz"), x=x.numpy(), out=out.numpy())
    return 0


if __name__ == "__main__":
    sys.exit(main())
