#!/usr/bin/env python3
"""Golden vectors of calc_D_loss under label smoothing / label noise, from the REFERENCE implementation (build container only).

``calc_D_loss`` (with ``bce`` / ``mse``) is taken out of the reference's ``train.py`` with ``ast`` and EXECUTED here as it is, the
way tests/gen_golden.py takes it -- never copied.  It runs on CPU in fp64 with B = 6 under a fixed ``torch.manual_seed``; the
labels it drew are recorded by repeating its own torch calls, in its order, under the same seed, and the repetition is proved
right before anything is written: the loss recomputed from the recorded labels equals the value the reference returned.

Run:  python tests/gen_golden_labels.py      (no-op with a message if the reference is absent)
Writes tests/golden/label_losses.npz.
"""
import ast
import os
import sys

import numpy as np
import torch

REF = os.environ.get("MPGAN_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "golden")

B = 6
SEED = 20240607
NOISE = 0.3
# name -> (loss, label_smoothing, label_noise)
CASES = {"ls_smooth": ("ls", True, False), "ls_noise": ("ls", False, NOISE), "ls_smooth_noise": ("ls", True, NOISE),
         "og_noise": ("og", False, NOISE)}


def reference_calc_D_loss():
    with open(os.path.join(REF, "train.py")) as f:
        tree = ast.parse(f.read())
    wanted = [n for n in tree.body
              if (isinstance(n, ast.FunctionDef) and n.name == "calc_D_loss")
              or (isinstance(n, ast.Assign) and getattr(n.targets[0], "id", "") in ("bce", "mse"))]
    assert len(wanted) == 3, [getattr(n, "name", None) for n in wanted]
    ns = {"torch": torch}
    exec(compile(ast.Module(body=wanted, type_ignores=[]), os.path.join(REF, "train.py"), "exec"), ns)
    return ns["calc_D_loss"]


def redraw(smoothing, noise):
    """The labels calc_D_loss draws (train.py:353-363), by its own calls in its own order."""
    if smoothing:
        y_real = torch.empty(B).uniform_(0.7, 1.2)
        y_fake = torch.empty(B).uniform_(0.0, 0.3)
    else:
        y_real = torch.ones(B, 1)
        y_fake = torch.zeros(B, 1)
    if noise:
        y_real[torch.rand(B) < noise] = 0
        y_fake[torch.rand(B) < noise] = 1
    return y_real, y_fake


def main():
    if not os.path.isfile(os.path.join(REF, "train.py")):
        print("gen_golden_labels: no reference at", REF, "-- nothing written")
        return
    calc_D_loss = reference_calc_D_loss()
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)     # (the reference draws its labels in the default dtype)
    try:
        rs = np.random.RandomState(17)
        rec = {"B": np.array(B), "seed": np.array(SEED), "noise": np.array(NOISE), "cases": np.array(sorted(CASES))}
        for name, (loss, smoothing, noise) in CASES.items():
            out_r = torch.from_numpy(rs.uniform(0.05, 0.95, size=(B, 1))).requires_grad_(True)
            out_f = torch.from_numpy(rs.uniform(0.05, 0.95, size=(B, 1))).requires_grad_(True)
            torch.manual_seed(SEED)
            D, parts = calc_D_loss(loss, None, out_r.detach(), None, out_r, out_f, B, label_smoothing=smoothing, label_noise=noise)
            D.backward()
            torch.manual_seed(SEED)
            y_real, y_fake = redraw(smoothing, noise)
            # the repetition drew what the reference used: its loss from the recorded labels, by torch's own criterion
            crit = torch.nn.MSELoss() if loss == "ls" else torch.nn.BCELoss()
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")     # (MSELoss says what it thinks of [B, 1] against [B])
                again = crit(out_r.detach(), y_real) + crit(out_f.detach(), y_fake)
            assert float(again) == float(D.detach()), (name, float(again), float(D))
            if noise:
                assert bool(((y_real == 0).any() or (y_fake == 1).any())), name       # (the seed flips something)
            rec.update({f"{name}_out_r": out_r.detach().numpy(), f"{name}_out_f": out_f.detach().numpy(),
                        f"{name}_Y_real": y_real.reshape(-1).numpy(), f"{name}_Y_fake": y_fake.reshape(-1).numpy(),
                        f"{name}_Dr": np.array(parts["Dr"]), f"{name}_Df": np.array(parts["Df"]), f"{name}_D": np.array(parts["D"]),
                        f"{name}_dD_dr": out_r.grad.numpy(), f"{name}_dD_df": out_f.grad.numpy(),
                        f"{name}_smoothing": np.array(bool(smoothing)), f"{name}_loss": np.array(loss)})
            print(name, parts["D"], y_real.reshape(-1).tolist(), y_fake.reshape(-1).tolist())
        # og + smoothing: the reference does not run
        o = torch.full((B, 1), 0.5)
        torch.manual_seed(SEED)
        try:
            calc_D_loss("og", None, o, None, o, o, B, label_smoothing=True, label_noise=False)
            raised, msg = False, ""
        except ValueError as e:
            raised, msg = True, str(e)
        assert raised and "target size" in msg, msg
        rec["og_smooth_raises_ValueError"] = np.array(raised)
        rec["og_smooth_message"] = np.array(msg)
    finally:
        torch.set_default_dtype(prev)
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, "label_losses.npz"), **rec)
    print("wrote", os.path.join(OUT, "label_losses.npz"))


if __name__ == "__main__":
    sys.exit(main())
