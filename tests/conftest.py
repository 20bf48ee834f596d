import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the HIP runtime says why it aborts (a faulting kernel's queue error, an invalid launch) only at this log level; errors only
os.environ.setdefault("AMD_LOG_LEVEL", "1")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


def pytest_collection_modifyitems(config, items):
    # GPU tests are skipped (not failed) where no GPU is visible
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except Exception:  # pragma: no cover
        has_gpu = False
    if has_gpu:
        return
    skip = pytest.mark.skip(reason="no GPU visible")
    for it in items:
        if "gpu" in it.keywords:
            it.add_marker(skip)


def load_golden(name):
    """``tests/golden/<name>``, merged with its parts ``<stem>.part1.npz``, ... where a fixture is larger than one committed
    file may be (tests/gen_golden.py: save_parts)."""
    d = dict(np.load(os.path.join(GOLDEN, name), allow_pickle=False))
    stem, k = os.path.splitext(name)[0], 1
    while os.path.isfile(os.path.join(GOLDEN, f"{stem}.part{k}.npz")):
        d.update(np.load(os.path.join(GOLDEN, f"{stem}.part{k}.npz"), allow_pickle=False))
        k += 1
    return d


def summarize(name, t):
    """Same summary as tests/gen_golden.py: sum, l2, 64 sampled entries."""
    import zlib
    flat = t.detach().double().reshape(-1).cpu()
    rs = np.random.RandomState(zlib.crc32(name.encode()) % (2**31))
    idx = rs.randint(0, flat.numel(), size=64)
    return np.concatenate([[flat.sum().item(), flat.norm().item()], flat[idx].numpy()])


def rel_err(a, b):
    """max|a-b| / max|b|  -- the parity metric used throughout (per tensor)."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    den = np.abs(b).max()
    return float(np.abs(a - b).max() / (den if den > 0 else 1.0))


def summary_err(name, t, golden):
    """Error of a tensor against a golden SUMMARY (sum, l2, 64 sampled entries; tests/gen_golden.py) as a fraction of
    each entry's natural scale: the l2 norm and the sampled entries over max|golden[1:]| (the tensor's own magnitude),
    the sum over the l1 norm of the tensor -- a sum of n entries that each carry a relative error eps is only known
    to eps * sum|x_i|; against |sum x_i|, which cancellation makes arbitrarily smaller, the same eps looks like a
    multiple of itself (a weight gradient whose entries cancel to 1.5 % of their l1 turned 3e-5 into 2e-3)."""
    s = summarize(name, t)
    g = np.asarray(golden, dtype=np.float64)
    scale = np.abs(g[1:]).max()
    scale = scale if scale > 0 else 1.0
    l1 = float(t.detach().double().abs().sum().item())
    return float(max(np.abs(s[1:] - g[1:]).max() / scale, abs(s[0] - g[0]) / (l1 if l1 > 0 else 1.0)))


# ---- parity evidence: what the gradient checks of a session measured, kept for profiles/  -------------------
# Every check that lets a tensor pass on something else than its plain bar -- the fp32 control of ``assert_grads``, the
# sign-conditioned oracle of the kinked MPLayer cases -- records what it measured here; a ``-m gpu`` session writes the records
# to gpurun_out/parity_bars.txt when it ends (copied to profiles/ by whoever ran it).
PARITY_LOG = []
CONTROL_CEILING = 2e-2   # no tensor passes on the fp32 control beyond this, whatever fp32's own error on the input was


def record_parity(kind, what, **fields):
    test = os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0]
    PARITY_LOG.append((kind, test, str(what), fields))


def pytest_sessionfinish(session, exitstatus):
    if not PARITY_LOG:
        return
    out = os.path.join(ROOT, "gpurun_out")
    try:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "parity_bars.txt"), "w") as f:
            f.write("# parity evidence of one pytest session (tests/conftest.py: PARITY_LOG); exit status %s\n" % exitstatus)
            f.write("# assert_grads: per call the tensor with the largest err = max|got - fp64| / max|fp64| (fp32_err: the fp32 oracle's own error "
                    "against fp64 there, err_vs_fp32: got against the fp32 oracle) and how many tensors passed on which route: within tol "
                    "of fp64 / within tol of the fp32 evaluation / within control_bar = max(tol, 3 x fp32_err) capped at %g\n" % CONTROL_CEILING)
            for kind, test, what, fields in PARITY_LOG:
                f.write("%s | %s | %s | %s\n" % (kind, test, what, " ".join("%s=%s" % (k, _fmt(v)) for k, v in fields.items())))
    except OSError:   # (a read-only tree: the evidence is a by-product, never a reason to fail)
        pass


def _fmt(v):
    return "%.3g" % v if isinstance(v, float) else str(v)


def assert_grads(got, ref, tol, control=None, what=""):
    """Per-parameter gradient check against the fp64 oracle: max|got - ref| <= tol * max|ref|; a parameter whose true
    gradient vanishes by symmetry is held to tol * 1e-3 of the network's largest gradient instead of to its own
    rounding noise.  ``control`` = the SAME oracle evaluated in plain fp32 (the reference's arithmetic).  LeakyReLU' jumps at
    0, so a pre-activation within rounding of zero takes the other slope in any finite arithmetic, fp32 included, and in a
    short sum (few jets) one such edge is visible at ~1e-2.  A parameter beyond ``tol`` of fp64 passes
      * when it is within ``tol`` of the fp32 evaluation itself (the reference's own arithmetic made the same decisions:
        "within 1e-3 of the reference's fp32 result" is BASELINE.json's bar), or
      * within 3x of fp32's own error against fp64 on this input -- but never beyond ``CONTROL_CEILING``.
    Every call leaves in ``PARITY_LOG`` its worst tensor and how many tensors passed on which route."""
    scale = max(float(np.abs(np.asarray(v)).max()) for v in ref.values())
    bad, worst = {}, None
    routes = {"fp64": 0, "fp32": 0, "control": 0}
    for k, r in ref.items():
        r = np.asarray(r, dtype=np.float64)
        g = np.asarray(got[k], dtype=np.float64)
        den = max(np.abs(r).max(), 1e-3 * scale)
        err = float(np.abs(g - r).max() / den)
        bar, ctl, e32 = tol, None, None
        if control is not None:
            c = np.asarray(control[k], dtype=np.float64)
            ctl = float(np.abs(c - r).max() / den)
            e32 = float(np.abs(g - c).max() / den)
            bar = min(max(tol, 3.0 * ctl), max(tol, CONTROL_CEILING))
        if err <= tol:
            routes["fp64"] += 1
        elif e32 is not None and e32 <= tol:
            routes["fp32"] += 1
        elif err <= bar:
            routes["control"] += 1
        else:
            bad[k] = (err, bar, e32)
        if worst is None or err > worst[1]:
            worst = (k, err, bar, ctl, e32)
    record_parity("assert_grads", what, tensors=len(ref), tol=float(tol), worst=worst[0], err=worst[1], control_bar=worst[2],
                  fp32_err=(-1.0 if worst[3] is None else worst[3]), err_vs_fp32=(-1.0 if worst[4] is None else worst[4]),
                  passed_vs_fp64=routes["fp64"], passed_vs_fp32=routes["fp32"], passed_on_control=routes["control"], failed=len(bad))
    assert not bad, (what, bad)


def option_case_shapes(F, out, kw):
    """State-dict shapes of an MPLayer built with the option keywords of ``gen_golden.OPTION_CASES`` (edge features,
    conditioning columns and layer widths change the first Linear of fe / fn; mpgan/model.py:169-204)."""
    nc = 3 if kw.get("coords", "polarrel") == "cartesian" else 2
    num_ef = 0
    if kw.get("pos_diffs"):
        if kw.get("delta_coords"):
            num_ef += nc
        if kw.get("delta_r", True) or kw.get("all_ef", True):
            num_ef += 1
    extra = int(kw.get("clabels", 0)) + int(bool(kw.get("mask_fne_np")))
    fe, fn = list(kw.get("fe", [96, 160, 192])), list(kw.get("fn", [256, 256]))
    sh = {}
    d = [2 * F + num_ef + extra] + fe
    for k in range(len(fe)):
        sh[f"fe.net.{k}.weight"], sh[f"fe.net.{k}.bias"] = (d[k + 1], d[k]), (d[k + 1],)
    d = [fe[-1] + F + extra] + fn + [out]
    for k in range(len(fn) + 1):
        sh[f"fn.net.{k}.weight"], sh[f"fn.net.{k}.bias"] = (d[k + 1], d[k]), (d[k + 1],)
    return sh


def option_case_oracle_kwargs(kw):
    """The keywords of ``oracle.mpgan_ref.mplayer_forward_general`` for one ``OPTION_CASES`` entry."""
    o = {k: kw[k] for k in ("pos_diffs", "all_ef", "coords", "delta_coords", "delta_r", "clabels", "mask_fne_np") if k in kw}
    if not kw.get("fully_connected", True):
        o["knn"] = (kw["num_knn"], kw.get("self_loops", True))
    o["sum_agg"] = kw.get("sum", True)
    return o


def hip_signs_from(ac, stE2, sign3, h1, h2, B, N):
    """Signs (True = negative) of the pre-activations a fused MPLayer forward saw, where it keeps them: fe layer 1 from the
    saved a|c terms (z1 = a_i + c_j in fp32, as the kernel adds them), fe layer 2 from the sign bits of the parked E2
    fragments (edge_fwd2_impl.h: block (b, rb, j) = 10 fragments x 64 lanes x 8 halves; fragment 2 mm + s, lane (r, h),
    element jj <-> feature 32 mm + 16 s + 8 (jj >> 2) + 4 h + (jj & 3) of receiver 32 rb + r; LeakyReLU keeps the sign, -0.0
    for plain ReLU), fe layer 3 from the packed sign words (word q of lane (r, h), bit 31 - (16 (tile & 1) + reg) for
    tile >> 1 == q; reg 4g+t <-> feature 32 tile + 8g + 4h + t), the node network from the sign bits of its saved outputs.
    [B,N,N,*] / [B,N,*] like the oracle's probes; the fe layers are only defined for unmasked senders (skipped blocks are
    never written) and, under dropout, for kept elements (a dropped one is +0: its branch multiplies a zero)."""
    import torch
    a, c = ac[:, :96].reshape(B, N, 96), ac[:, 96:].reshape(B, N, 96)
    z1neg = ((a.unsqueeze(2) + c.unsqueeze(1)) < 0).cpu()
    RB = (N + 31) // 32
    e2 = torch.signbit(stE2.reshape(B, RB, N, 5, 2, 2, 32, 2, 4)).cpu()          # [b, rb, j, mm, s, h, r, u, t]
    z2neg = e2.permute(0, 1, 6, 2, 3, 4, 7, 5, 8).reshape(B, RB * 32, N, 160)[:, :N].contiguous()   # [b, i, j, 32mm+16s+8u+4h+t]
    w = sign3.reshape(B, RB, N, 3, 64).cpu().numpy().astype(np.uint32)           # [b, rb, j, q, lane]
    z3neg = np.zeros((B, N, N, 192), dtype=bool)
    for tile in range(6):
        for reg in range(16):
            bit = (w[:, :, :, tile >> 1, :] >> np.uint32(31 - (16 * (tile & 1) + reg))) & 1   # [b, rb, j, lane]
            g, t = reg >> 2, reg & 3
            for hh in range(2):
                f = 32 * tile + 8 * g + 4 * hh + t
                for rb in range(RB):
                    n_i = min(32, N - 32 * rb)
                    z3neg[:, 32 * rb:32 * rb + n_i, :, f] = bit[:, rb, :, 32 * hh:32 * hh + n_i].transpose(0, 2, 1) != 0
    return {"fe1": z1neg, "fe2": z2neg, "fe3": torch.from_numpy(z3neg), "fn1": torch.signbit(h1.reshape(B, N, -1)).cpu(),
            "fn2": torch.signbit(h2.reshape(B, N, -1)).cpu()}
