"""The one-launch attention blocks (mpg_mab_fwd / mpg_mab_bwd / mpg_mab_chain_fwd, csrc/mab_fwd.hip and mab_bwd.hip) on the key masks a network
meets in use -- whole key tiles of 32 without a real key (leading, middle, last), single real keys at a tile's first and last
slot, the jet with no real key at all -- at every tile and route edge, through every schedule that can take the shape.

Every case is held against autograd on ``oracle.gapt_ref.mab_forward`` in fp64, fed the very dropout masks the kernels drew
(``ops.dropout_mask``), with the catalogue of tests/test_mab_masks_cpu.py as ONE batch (dead and sparse jets beside full ones):
  * out, dx, dy PER JET: max|got_b - ref_b| <= TIGHT * max(max|ref_b|, 1e-3 max|ref|) -- a sparse or dead jet that is wrong by
    its own magnitude cannot hide behind the batch's largest rows; the offending pattern is named in the failure;
  * every parameter gradient per tensor at TIGHT; everything finite;
  * the all-ignored jet: zero attention weights (torch's ``_safe_softmax`` meaning, oracle/gapt_ref._mha), i.e. its output is
    x + out_proj.bias pushed through the second half of the block and its rows of dy (cross attention) are zero;
  * the worst per-jet error of each (shape, schedule) and the pattern that gave it go to ``conftest.record_parity``.
TIGHT = 1e-4 is tests/test_gpu_mab.py's bar; the oracle's own fp32 evaluation stays below 1e-5 under the same metric
(tests/test_mab_masks_cpu.py)."""
import os

import numpy as np
import pytest
import torch

from conftest import rel_err, record_parity, assert_grads
from test_mab_masks_cpu import (catalogue, tiled_catalogue, worst_jet, DEAD, FLOOR, SELF_SIZES, POOL_KEYS,
                                ISAB_KEYS, EDGE_SHAPES)

pytestmark = pytest.mark.gpu
TIGHT = 1e-4
LA = {"leaky_relu_alpha": 0.2, "dropout_p": 0.0, "batch_norm": False, "spectral_norm": False}
SCHEDULES = {   # (read at every launch, csrc/mab_common.h: mab_split_mode; mpg_mab_fwd)
    "default": {},
    "split0": {"MPG_MAB_SPLIT": "0"},     # one wave per jet
    "split1": {"MPG_MAB_SPLIT": "1"},     # two waves per jet up to 512 jets (the default, spelled out)
    "split2": {"MPG_MAB_SPLIT": "2"},     # two waves per jet at any size
    "big": {"MPG_MAB_BIG": "1"},          # the large-set kernels on a small set
}


class _env:
    def __init__(self, values):
        self.values = values

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in ("MPG_MAB_SPLIT", "MPG_MAB_BIG")}
        for k in self.saved:
            os.environ.pop(k, None)
        os.environ.update(self.values)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _shapes(E, ln, prefix="mab"):
    from oracle import train_ref as T
    sh = dict(T._mab_shapes(prefix, E))
    if ln:
        for n in ("norm1", "norm2"):
            sh[f"{prefix}.{n}.weight"], sh[f"{prefix}.{n}.bias"] = (E,), (E,)
    return sh


def _params(E, ln, seed, prefix="mab"):
    from oracle import train_ref as T
    sd = T.init_state_dict(_shapes(E, ln, prefix), seed, torch.float32)
    for k in list(sd):
        if k.endswith(("norm1.weight", "norm2.weight")):   # (around 1, as a trained norm's)
            sd[k] = 1.0 + 0.3 * sd[k] / sd[k].abs().max()
    return sd


def _fixed_dropout_stream(dev):
    """The same seed and dropout-site tags whatever ran before: a case draws the same masks alone and inside the whole suite."""
    import itertools
    from mpgan_amd import ops
    ops.set_seed(20261, dev)
    ops.dev_state(dev).tags = itertools.count(7000)


def _keeps(B, L, E, tag, thr):
    from mpgan_amd import ops
    if not thr:
        return None
    return {k: ops.dropout_mask(B * L, E, tag + site, thr).double().cpu().reshape(B, L, E) for site, k in enumerate(("a", "f", "o"))}


def _without_attention(sd64, prefix, x, keeps, p, ln):
    """The block with zero attention weights: x + out_proj.bias through the norms, dropout sites and feed-forward layer."""
    from oracle import gapt_ref as R
    from oracle.mpgan_ref import leaky, _drop
    k = keeps or {}
    z = x + sd64[f"{prefix}.attention.out_proj.bias"]
    if ln:
        z = R._layer_norm(sd64, f"{prefix}.norm1", z)
    z = _drop(z, k.get("a"), p)
    f = _drop(leaky(z @ sd64[f"{prefix}.ff.net.0.weight"].t() + sd64[f"{prefix}.ff.net.0.bias"], 0.2), k.get("f"), p)
    o = z + f
    if ln:
        o = R._layer_norm(sd64, f"{prefix}.norm2", o)
    return _drop(o, k.get("o"), p)


def _compare(got, ref, ggrads, rgrads, names, what, dead_out=None):
    """The assertions of one case; every figure is printed before anything is asserted.  Returns the worst per-jet error."""
    bad, worst = [], (0.0, "", -1, "")
    for k in ("out", "dx", "dy"):
        if k not in ref:
            continue
        if not np.isfinite(got[k]).all():
            rows = np.flatnonzero(~np.isfinite(got[k].reshape(len(names), -1)).all(1))
            bad.append(f"{k}: not finite in jets {[(int(b), names[b]) for b in rows[:8]]}")
        err, name, b = worst_jet(got[k], ref[k], names)
        print(f"{what} {k}: worst per-jet {err:.3g} ({name}, jet {b}); per tensor {rel_err(np.nan_to_num(got[k]), ref[k]):.3g}")
        if err > worst[0]:
            worst = (err, name, b, k)
        if not err <= TIGHT:
            bad.append(f"{k}: per-jet error {err:.3g} > {TIGHT:g} in pattern {name!r} (jet {b})")
    gworst = (0.0, "")
    for k, r in rgrads.items():
        g = ggrads[k]
        e = rel_err(g, r) if np.isfinite(g).all() else float("inf")
        if e > gworst[0]:
            gworst = (e, k)
        if not e < TIGHT:
            bad.append(f"grad {k}: {e:.3g}")
    print(f"{what} parameter gradients: worst {gworst[0]:.3g} ({gworst[1]})")
    # the all-ignored jets: attention contributes nothing
    for b, n in enumerate(names):
        if not n.startswith(DEAD):
            continue
        if dead_out is not None:
            want = dead_out(b)
            e = float(np.abs(got["out"][b] - want).max() / max(np.abs(want).max(), FLOOR * np.abs(ref["out"]).max()))
            if not e <= TIGHT:
                bad.append(f"out of the all-ignored jet {b} is not x + bo through the second half: {e:.3g}")
        if "dy" in ref:
            e = float(np.abs(got["dy"][b]).max())
            if not e <= TIGHT * FLOOR * np.abs(ref["dy"]).max():
                bad.append(f"dy of the all-ignored jet {b} is not zero: max {e:.3g}")
    record_parity("mab_masks", what, jets=len(names), worst_err=worst[0], tensor=worst[3], pattern=worst[1], jet=worst[2],
                  worst_param_grad=gworst[0], param=gworst[1], failed=len(bad))
    assert not bad, (what, bad)
    return worst[0]


def run_block(E, H, L, S, ln, p, route, names, ign, schedule="default", seed=11):
    """One forward + backward of a block on ``names`` / ``ign`` (None: ``ignore = None``) against the fp64 oracle.
    route: "mab" (self-attention when L == S, cross otherwise), "pma" (PMA's shared seed row, B > 1), "seeds" (plain MAB with
    the seed row copied B times)."""
    from oracle import gapt_ref as R
    from mpgan_amd import ops
    from mpgan_amd.gapt import MAB, PMA, _attn_mask
    B = len(names)
    dev = torch.device("cuda:0")
    la = dict(LA, dropout_p=p)
    args = dict(embed_dim=E, num_heads=H, ff_layers=[], final_linear=False, layer_norm=ln, dropout_p=p, linear_args=la)
    sd = _params(E, ln, seed)
    gen = torch.Generator().manual_seed(5 + L + 7 * S)
    yk = torch.randn(B, S, E, generator=gen)
    self_attn = route == "mab" and L == S
    if route in ("pma", "seeds"):
        assert L == 1
        seed_row = 0.5 * torch.randn(1, 1, E, generator=gen)
        xq = seed_row.expand(B, 1, E).contiguous()
    else:
        xq = yk if self_attn else torch.randn(B, L, E, generator=gen)
    gy = torch.randn(B, L, E, generator=gen)
    what = f"{route} {L}x{S} E={E} ln={int(ln)} p={p} B={B} {schedule}" + ("" if ign is not None else " ignore=None")
    _fixed_dropout_stream(dev)
    with _env(SCHEDULES[schedule]):
        if route == "pma":
            blk = PMA(num_seeds=1, **args).to(dev).train()
            blk.mab.load_state_dict({k[len("mab."):]: v for k, v in sd.items()})
            with torch.no_grad():
                blk.S.copy_(seed_row)
            yg = yk.to(dev).requires_grad_(True)
            mask = None if ign is None else _attn_mask((~ign).float().reshape(B, S, 1).to(dev))
            out = blk(yg, mask)
            xg = None
        else:
            blk = MAB(**args).to(dev).train()
            blk.load_state_dict({k[len("mab."):]: v for k, v in sd.items()})
            assert blk._fused_ok(torch.empty(1, device=dev), L, S)
            xg = xq.to(dev).requires_grad_(True)
            yg = xg if self_attn else yk.to(dev).requires_grad_(True)
            out = blk(xg, yg, None if ign is None else ign.to(dev))
        tag = ops.last_tag()
        (out * gy.to(dev)).sum().backward()
        torch.cuda.synchronize()
    thr, _ = ops.drop_params(p)
    keeps = _keeps(B, L, E, tag, thr)
    pe = thr / 256.0    # (byte-mode dropout quantises p to thr / 256)
    sd64 = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    yo = yk.double().requires_grad_(True)
    if route == "pma":
        so = seed_row.double().requires_grad_(True)
        xo = so.expand(B, 1, E)
    else:
        xo = xq.double().requires_grad_(True)
        if self_attn:
            yo = xo
    ref = R.mab_forward(sd64, "mab", xo, yo, ign, num_heads=H, p=pe, keeps=keeps, layer_norm=ln)
    (ref * gy.double()).sum().backward()
    num = lambda t: t.detach().double().cpu().numpy()
    got, want = {"out": num(out)}, {"out": num(ref)}
    if route != "pma":
        got["dx"], want["dx"] = num(xg.grad), num(xo.grad)
    if not self_attn:
        got["dy"], want["dy"] = num(yg.grad), num(yo.grad)
    ggrads, rgrads = {}, {}
    for k, q in blk.named_parameters():
        if route == "pma":
            ggrads[k], rgrads[k] = num(q.grad), num(so.grad if k == "S" else sd64[k].grad)
        else:
            ggrads[k], rgrads[k] = num(q.grad), num(sd64["mab." + k].grad)
    sdd = {k: v.detach() for k, v in sd64.items()}

    def dead_out(b):
        kb = None if keeps is None else {k: v[b] for k, v in keeps.items()}
        return _without_attention(sdd, "mab", xo.detach()[b], kb, pe, ln).numpy()
    return _compare(got, want, ggrads, rgrads, names, what, dead_out)


def run_catalogue(E, H, L, S, ln, p, route, schedule="default"):
    names, ign = catalogue(S)
    run_block(E, H, L, S, ln, p, route, names, ign, schedule)
    if schedule == "default":    # ``ignore = None``: a call of its own (the kernels take a null pointer)
        run_block(E, H, L, S, ln, p, route, ["ignore_None"] * 3, None, schedule)


BASE = dict(E=64, H=4, ln=False, p=0.5)
OPTIONS = [dict(E=64, H=4, ln=True, p=0.0), dict(E=32, H=2, ln=False, p=0.0), dict(E=32, H=2, ln=True, p=0.5)]
OPTION_SUBSET = [("mab", n, n) for n in (31, 32, 33, 64, 65, 129, 160)] + [("pma", 1, 160), ("mab", 10, 150), ("mab", 150, 10),
                                                                         ("mab", 32, 33)]
_id = lambda v: f"{v[0]}-{v[1]}x{v[2]}" if isinstance(v, tuple) else (f"E{v['E']}-ln{int(v['ln'])}-p{v['p']}" if isinstance(v, dict) else str(v))


@pytest.mark.parametrize("N", SELF_SIZES)
def test_self_attention_on_the_mask_catalogue(N):
    """Self-attention at every tile edge: last lane of the one-wave kernels (31, 32), first size of the large-set kernels (33),
    and each side of every further tile boundary up to 160."""
    run_catalogue(L=N, S=N, route="mab", **BASE)


@pytest.mark.parametrize("route", ["pma", "seeds"])
@pytest.mark.parametrize("S", POOL_KEYS)
def test_pooling_shape_on_the_mask_catalogue(S, route):
    """One query, S keys: through PMA's shared seed row (row stride 0, its gradient summed over the jets) and through a plain
    MAB given B copies of the row."""
    run_catalogue(L=1, S=S, route=route, **BASE)


@pytest.mark.parametrize("L,S", [(10, s) for s in ISAB_KEYS] + [(s, 10) for s in ISAB_KEYS] + list(EDGE_SHAPES))
def test_cross_attention_on_the_mask_catalogue(L, S):
    """Both cross shapes of an ISAB, and the shapes where only one of L, S is past 32 (either picks the large-set kernels; the
    workgroup is sized by the larger)."""
    run_catalogue(L=L, S=S, route="mab", **BASE)


@pytest.mark.parametrize("opt", OPTIONS, ids=_id)
@pytest.mark.parametrize("shape", OPTION_SUBSET, ids=_id)
def test_other_widths_norms_and_dropout_on_the_mask_catalogue(shape, opt):
    """E = 32 / 2 heads, ``layer_norm=True`` (a dead jet's rows still pass both norms), dropout off."""
    route, L, S = shape
    run_catalogue(L=L, S=S, route=route, **opt)
    if max(L, S) <= 32:
        run_catalogue(L=L, S=S, route=route, schedule="big", **opt)


@pytest.mark.parametrize("schedule", ["split0", "split1", "split2", "big"])
@pytest.mark.parametrize("shape", [("mab", n, n) for n in (1, 2, 31, 32)] + [("pma", 1, s) for s in (1, 31, 32)]
                         + [("seeds", 1, 32), ("mab", 10, 30)], ids=_id)
def test_every_schedule_of_a_small_set_against_the_oracle(shape, schedule):
    """Sets of at most 32 tokens through every kernel that can take them -- one wave per jet, two waves per jet, the large-set
    kernels -- each against the oracle, not against each other."""
    route, L, S = shape
    run_catalogue(L=L, S=S, route=route, schedule=schedule, **BASE)


@pytest.mark.parametrize("B,opt", [(255, BASE), (300, BASE), (300, OPTIONS[0]), (700, BASE), (700, OPTIONS[1]), (1100, BASE),
                                   (1100, OPTIONS[2])], ids=_id)
def test_batch_size_branches_of_the_launcher(B, opt):
    """N = 30 with the catalogue tiled to an odd batch below 256 (one wave per workgroup), 257 ... 512 (two waves per jet both
    ways / two one-wave jets per workgroup), 513 ... 1,024 (``mab_fwd2_kernel<.., 8>`` forward, one-wave backward) and beyond
    1,024 (four jets per workgroup, grid capped): self-attention and the 10 x 30 cross shape."""
    for L in (30, 10):
        names, ign = tiled_catalogue(30, B)
        run_block(L=L, S=30, route="mab", names=names, ign=ign, **opt)


@pytest.mark.parametrize("training", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("E,H,schedule", [(64, 4, "default"), (64, 4, "split0"), (32, 2, "default")])
@pytest.mark.parametrize("N", [1, 31, 32])
@pytest.mark.parametrize("nblk", [2, 4])
def test_sab_chain_on_the_mask_catalogue(nblk, N, E, H, schedule, training):
    """``mpg_mab_chain_fwd`` (a wave keeps its jet's rows in registers from block to block: an error in one block's dead or
    sparse jet would feed the next) against the oracle applied block after block, with each block's own dropout masks; the
    block-by-block backward behind it against autograd on the same."""
    from oracle import gapt_ref as R
    from mpgan_amd import ops, _lib
    from mpgan_amd.gapt import SAB, _attn_mask
    from mpgan_amd.gapt.model import _run_sabs
    dev = torch.device("cuda:0")
    p = 0.5
    names, ign = catalogue(N)
    B = len(names)
    args = dict(embed_dim=E, num_heads=H, ff_layers=[], final_linear=False, layer_norm=False, dropout_p=p, linear_args=dict(LA, dropout_p=p))
    sds = [_params(E, False, 20 + i) for i in range(nblk)]
    sabs = []
    for sd in sds:
        s = SAB(**args).to(dev)
        s.load_state_dict(sd)
        sabs.append(s.train(training))
    gen = torch.Generator().manual_seed(9 + N)
    x = torch.randn(B, N, E, generator=gen)
    gy = torch.randn(B, N, E, generator=gen)
    st = ops.dev_state(dev)
    real, calls = _lib.lib(), []

    class Spy:
        def __getattr__(self, k):
            fn = getattr(real, k)
            if not k.startswith("mpg_mab"):
                return fn

            def f(*a):
                calls.append(k)
                return fn(*a)
            return f
    _fixed_dropout_stream(dev)
    saved, _lib._lib = _lib._lib, Spy()
    st.tag_log = []
    try:
        with _env(SCHEDULES[schedule]):
            xg = x.to(dev).requires_grad_(True)
            out = _run_sabs(sabs, xg, _attn_mask((~ign).float().reshape(B, N, 1).to(dev)))
            tags = [t for kind, t, _ in st.tag_log if kind == "mab"]
            (out * gy.to(dev)).sum().backward()
            torch.cuda.synchronize()
    finally:
        st.tag_log = None
        _lib._lib = saved
    assert calls[0] == "mpg_mab_chain_fwd" and calls.count("mpg_mab_chain_fwd") == 1 and "mpg_mab_fwd" not in calls, calls
    assert calls.count("mpg_mab_bwd") == nblk and len(tags) == nblk, (calls, tags)
    thr = ops.drop_params(p)[0] if training else 0
    pe = thr / 256.0
    xo = x.double().requires_grad_(True)
    sd64 = [{k: v.double().requires_grad_(True) for k, v in sd.items()} for sd in sds]
    h = xo
    for i in range(nblk):
        h = R.mab_forward(sd64[i], "mab", h, h, ign, num_heads=H, p=pe, keeps=_keeps(B, N, E, tags[i], thr))
    (h * gy.double()).sum().backward()
    num = lambda t: t.detach().double().cpu().numpy()
    ggrads = {f"{i}.{k}": num(q.grad) for i, s in enumerate(sabs) for k, q in s.named_parameters()}
    rgrads = {f"{i}.{k}": num(v.grad) for i, sd in enumerate(sd64) for k, v in sd.items()}
    what = f"chain of {nblk} {N}x{N} E={E} {'train' if training else 'eval'} {schedule}"
    _compare({"out": num(out), "dx": num(xg.grad)}, {"out": num(h), "dx": num(xo.grad)}, ggrads, rgrads, names, what)


def test_gapt_networks_n150_with_sparse_and_full_jets_vs_oracle():
    """GAPT_G and GAPT_D, one train_D + train_G at N = 150, B = 8, multiplicities 1, 2, 31, 33 and 150 among them: the only place
    the scattered masks of ``mpg_rank_mask`` (a jet of one particle: every key tile but one wholly ignored, usually the leading
    ones) meet the large-set kernels end to end.  Gradients of both networks against the oracle's iteration in fp64 at 1e-3
    with its own fp32 evaluation as the control (as test_gapt_train_step_n150_vs_oracle); the generated jets per jet at TIGHT."""
    from oracle import train_ref as T, gapt_ref as R
    from mpgan_amd import train
    B, N = 8, 150
    rs = np.random.RandomState(14)
    n = T.synthetic_batch(B, N, seed=14, dist="uniform")[1].numpy().reshape(-1) * N
    n = np.rint(n).astype(np.int64)
    n[:5] = (1, 2, 31, 33, 150)
    real = np.arange(N)[None, :] < n[:, None]
    eta, phi = (np.clip(rs.normal(0, 0.15, size=(B, N)), -1, 1) for _ in range(2))
    pt = rs.uniform(-0.5, 0.5, size=(B, N))
    data = torch.from_numpy(np.stack([np.where(real, eta, 0.0), np.where(real, phi, 0.0), np.where(real, pt, -0.5),
                                      np.where(real, 0.5, -0.5)], axis=2)).float()
    labels = torch.from_numpy((n.astype(np.float32) * np.float32(1.0 / N)).reshape(B, 1))
    G, D = train.default_gapt(N, disc_dropout=0.0)
    sdG = T.init_state_dict(T.gapt_param_shapes(True), 41, torch.float64)
    sdD = T.init_state_dict(T.gapt_param_shapes(False), 42, torch.float64)
    G.load_state_dict({k: v.float() for k, v in sdG.items()})
    D.load_state_dict({k: v.float() for k, v in sdD.items()})
    gen = torch.Generator().manual_seed(7)
    nD, nG = torch.randn(B, N, 64, generator=gen) * 0.2, torch.randn(B, N, 64, generator=gen) * 0.2
    # the generated jets themselves, per jet
    G.eval()
    with torch.no_grad():
        fake = G(nG.cuda(), labels.cuda()).double().cpu()
    G.train()
    with torch.no_grad():
        # (float32(n) * float32(1 / N) times N truncates to n in fp32, the reference's arithmetic, but for some n falls a hair
        # below n in fp64: the oracle gets the fp32 meaning, as in test_train_step_n150_vs_oracle)
        want = R.gapt_g_forward(sdG, nG.double(), labels.double() + 1e-7, num_particles=N)
    assert torch.equal(fake[..., 3], want[..., 3]) and [int(v) for v in (want[..., 3] > 0).sum(1)] == n.tolist()
    names = [f"n={v}" for v in n]
    err, name, b = worst_jet(fake.numpy(), want.numpy(), names)
    print(f"GAPT_G N=150 generated jets: worst per-jet {err:.3g} ({name}, jet {b})")
    record_parity("mab_masks", "GAPT_G 150 generated jets", jets=B, worst_err=err, pattern=name, jet=b)
    assert bool(torch.isfinite(fake).all()) and err <= TIGHT, (name, b, err)
    # one iteration's gradients
    ts = train.TrainStep(G, D, B, N, latent=64, use_graphs=False, lr_disc=0.0, lr_gen=train.LR_GAPT[1])
    ts.set_batch(data.cuda(), labels.cuda())
    ts.fixed_noise = (nD.cuda(), nG.cuda())
    ts._seg_D()
    gradD = {k: q.grad.detach().double().cpu().numpy().copy() for k, q in D.named_parameters()}
    ts._seg_G()
    gradG = {k: q.grad.detach().double().cpu().numpy().copy() for k, q in G.named_parameters()}
    ts._seg_end()
    torch.cuda.synchronize()
    c32 = lambda sd: {k: v.float() for k, v in sd.items()}
    c64 = lambda sd: {k: v.clone() for k, v in sd.items()}
    _, _, cD, cG = T.train_iteration("gapt", c32(sdD), c32(sdG), {}, {}, data.float(), labels.float(), nD.float(), nG.float(),
                                     0.0, train.LR_GAPT[1], return_grads=True)
    dl, gl, gD, gG = T.train_iteration("gapt", c64(sdD), c64(sdG), {}, {}, data.double(), labels.double() + 1e-7, nD.double(),
                                       nG.double(), 0.0, train.LR_GAPT[1], return_grads=True)
    num = lambda d: {k: v.detach().double().numpy() for k, v in d.items()}
    assert all(np.isfinite(v).all() for v in list(gradD.values()) + list(gradG.values()))
    assert abs(float(ts.D_loss) - dl) < 1e-4 * abs(dl) and abs(float(ts.G_loss) - gl) < 1e-4 * abs(gl)
    assert_grads(gradD, num(gD), 1e-3, control=num(cD), what=("gapt masks", N, "D"))
    assert_grads(gradG, num(gG), 1e-3, control=num(cG), what=("gapt masks", N, "G"))
