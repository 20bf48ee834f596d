"""The key-mask catalogue of the attention-block tests, and the meaning those tests hold the kernels to, pinned without a GPU.

``catalogue(S)`` names the key masks a GAPT network meets in use and a Bernoulli draw never produces: whole key tiles of 32 with
no real key (a pT-sorted jet of 40 particles out of 150 leaves tiles 2 ... 4 ignored; a sparse generated jet, whose real
particles ``mpg_rank_mask`` scatters, leaves its LEADING tiles ignored), single real keys at the first and last slot of a tile,
and the jet with no real key at all (the gradient penalty's interpolated jets; a label of 0).  One jet per pattern, all in one
batch, so that dead and sparse jets sit beside full ones.  tests/test_gpu_mab_masks.py and tests/test_gpu_attn.py import the
catalogue and the per-jet metric from here.

The contract (oracle/gapt_ref._mha): a query whose keys are all ignored gets zero attention weights -- torch's
``_safe_softmax`` meaning; every output and gradient stays finite."""
import numpy as np
import pytest
import torch

TILE = 32
# token counts of the GPU modules: self-attention sizes, pooled / induced key counts, route edges
SELF_SIZES = (1, 2, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128, 129, 159, 160)
POOL_KEYS = (1, 31, 32, 33, 64, 65, 128, 129, 160)
ISAB_KEYS = (33, 64, 150, 160)
EDGE_SHAPES = ((32, 33), (33, 32), (33, 1), (160, 33), (33, 160))
ALL_KEY_COUNTS = tuple(sorted(set(SELF_SIZES) | set(POOL_KEYS) | set(ISAB_KEYS) | {10, 30, 70} | {s for _, s in EDGE_SHAPES}))
DEAD = "all_ignored"
FLOOR = 1e-3    # a jet's error is taken against max(its own reference magnitude, FLOOR x the batch's)


def expected_real(name, S):
    """The real keys a pattern's NAME promises, as a sorted index array (the catalogue's specification)."""
    nt = (S + TILE - 1) // TILE
    every = np.arange(S)
    if name == "none_ignored":
        return every
    if name == "real_prefix":
        return every[:20 if S >= 40 else max(1, S // 2)]
    if name == "only_last":
        return every[S - 1:]
    if name == "only_first":
        return every[:1]
    if name.startswith("only_tile"):
        kt = int(name[len("only_tile"):])
        return every[TILE * kt:TILE * (kt + 1)]
    if name.startswith("all_but_tile"):
        kt = int(name[len("all_but_tile"):])
        return np.concatenate([every[:TILE * kt], every[TILE * (kt + 1):]])
    if name == "one_per_tile_slot0":
        return np.array([TILE * kt for kt in range(nt)])
    if name == "one_per_tile_slot31":
        return np.array([min(TILE * kt + TILE - 1, S - 1) for kt in range(nt)])
    if name == "scattered3":
        return np.sort(np.random.RandomState(1000 + S).permutation(S)[:3])
    if name == "every_second":
        return every[::2]
    if name == "bernoulli02":
        keep = np.random.RandomState(2000 + S).uniform(size=S) >= 0.2
        keep[np.random.RandomState(3000 + S).randint(S)] = True   # (the dead jet is a pattern of its own)
        return every[keep]
    if name == DEAD:
        return every[:0]
    raise KeyError(name)


def pattern_names(S):
    nt = (S + TILE - 1) // TILE
    names = ["none_ignored", "real_prefix", "only_last", "only_first"]
    if nt > 1:   # (one tile: "only tile 0" is no key ignored, "all but tile 0" is the dead jet)
        names += [f"only_tile{kt}" for kt in range(nt)] + [f"all_but_tile{kt}" for kt in range(nt)]
    names += ["one_per_tile_slot0", "one_per_tile_slot31", "scattered3", "every_second", "bernoulli02", DEAD]
    return names


def catalogue(S):
    """(names, ignore [P, S] bool; True = do not attend): one row per pattern that exists at S keys.  Patterns that coincide at
    a small S (one key: every pattern is "the key" or "nothing") are kept once, under the first name; the unmasked jet and the
    dead jet are always there.  ``ignore = None`` is not a row: the GPU tests run it as a call of its own."""
    names, rows, seen = [], [], set()
    for name in pattern_names(S):
        ign = np.ones(S, dtype=bool)
        ign[expected_real(name, S)] = False
        key = ign.tobytes()
        if key in seen:
            continue
        seen.add(key)
        names.append(name)
        rows.append(ign)
    return names, torch.from_numpy(np.stack(rows))


def tiled_catalogue(S, B):
    """The catalogue repeated to B jets (the launcher's batch-size branches): names carry their copy's number."""
    names, ign = catalogue(S)
    idx = [i % len(names) for i in range(B)]
    return [f"{names[i]}#{k // len(names)}" for k, i in enumerate(idx)], ign[idx]


def per_jet_err(got, ref, B):
    """err[b] = max|got_b - ref_b| / max(max|ref_b|, FLOOR * max|ref|): a sparse or dead jet is measured against its own rows,
    not against the largest jet of the batch; the floor serves jets whose reference is identically zero."""
    g = np.asarray(got, dtype=np.float64).reshape(B, -1)
    r = np.asarray(ref, dtype=np.float64).reshape(B, -1)
    top = np.abs(r).max()
    den = np.maximum(np.abs(r).max(1), FLOOR * (top if top > 0 else 1.0))
    return np.abs(g - r).max(1) / den


def worst_jet(got, ref, names):
    """(worst per-jet error, its pattern's name, its jet index)."""
    e = per_jet_err(got, ref, len(names))
    e = np.where(np.isfinite(e), e, np.inf)
    b = int(np.argmax(e))
    return float(e[b]), names[b], b


# ---- the catalogue does what it says --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", ALL_KEY_COUNTS)
def test_catalogue_patterns_have_the_real_keys_their_names_promise(S):
    names, ign = catalogue(S)
    nt = (S + TILE - 1) // TILE
    assert len(set(names)) == len(names) and ign.shape == (len(names), S) and ign.dtype == torch.bool
    real = {n: set(np.flatnonzero(~ign[i].numpy()).tolist()) for i, n in enumerate(names)}
    assert len({frozenset(v) for v in real.values()}) == len(names)          # (no two jets alike)
    assert real["none_ignored"] == set(range(S)) and real[DEAD] == set()
    # every pattern of the full list is present, under its own name or (where patterns coincide) another's
    for n in pattern_names(S):
        want = set(expected_real(n, S).tolist())
        assert want in real.values(), (S, n)
        if n in real:
            assert real[n] == want, (S, n)
    # spelled out once more, independently of ``expected_real`` (a pattern that coincides with an earlier one lives under that name)
    def holds(n, want):
        assert want in real.values() and real.get(n, want) == want, (S, n)

    holds("only_last", {S - 1})
    holds("only_first", {0})
    holds("every_second", set(range(0, S, 2)))
    if S >= 40:
        holds("real_prefix", set(range(20)))
    if S >= 8:
        assert len(real["scattered3"]) == 3
    if S >= 30:
        assert 0.5 * S < len(real["bernoulli02"]) < S
    if nt > 1:
        for kt in range(nt):
            tile = set(range(TILE * kt, min(TILE * (kt + 1), S)))
            holds(f"only_tile{kt}", tile)
            holds(f"all_but_tile{kt}", set(range(S)) - tile)
        holds("one_per_tile_slot0", {TILE * kt for kt in range(nt)})
        holds("one_per_tile_slot31", {min(TILE * kt + 31, S - 1) for kt in range(nt)})
        # a running maximum must survive a wholly ignored LEADING tile and a wholly ignored LAST tile
        first, last = set(range(TILE)), set(range(TILE * (nt - 1), S))
        live = [n for n in names if real[n]]
        assert any(not (real[n] & first) for n in live) and any(not (real[n] & last) for n in live)
        if S - TILE > 1:    # (... and with more than one real key behind it)
            assert any(not (real[n] & first) and len(real[n]) > 1 for n in live)


def test_tiled_catalogue_and_metric():
    names, ign = tiled_catalogue(30, 301)
    base, ign0 = catalogue(30)
    assert len(names) == 301 and ign.shape == (301, 30) and torch.equal(ign[:len(base)], ign0)
    assert names[0] == base[0] + "#0" and names[len(base)] == base[0] + "#1" and torch.equal(ign[len(base)], ign0[0])
    # the per-jet metric sees a small jet that is wrong by its own magnitude; the per-tensor metric does not
    ref = np.ones((3, 4, 2))
    ref[1] *= 1e-2
    got = ref.copy()
    got[1] *= 2.0
    e = per_jet_err(got, ref, 3)
    assert e[0] == 0 and e[2] == 0 and abs(e[1] - 1.0) < 1e-12
    assert np.abs(got - ref).max() / np.abs(ref).max() < 2e-2
    ref[2] = 0.0                                       # an identically-zero jet: the floor
    got[2] = 5e-4
    assert abs(per_jet_err(got, ref, 3)[2] - 0.5) < 1e-12
    got[0, 0, 0] = np.nan
    assert worst_jet(got, ref, ["a", "b", "c"])[1:] == ("a", 0)


# ---- the oracle itself on the catalogue: fp32 against fp64, per jet -------------------------------------------------------------
def _oracle_run(dt, E, H, L, S, names, ign, seed=11):
    from oracle import train_ref as T, gapt_ref as R
    B = len(names)
    sd = {k: v.to(dt).requires_grad_(True) for k, v in T.init_state_dict(T._mab_shapes("mab", E), seed, torch.float64).items()}
    gen = torch.Generator().manual_seed(5)
    yk = torch.randn(B, S, E, generator=gen)
    xq = yk if L == S else torch.randn(B, L, E, generator=gen)
    gy = torch.randn(B, L, E, generator=gen)
    xo = xq.to(dt).requires_grad_(True)
    yo = xo if L == S else yk.to(dt).requires_grad_(True)
    out = R.mab_forward(sd, "mab", xo, yo, ign, num_heads=H)
    (out * gy.to(dt)).sum().backward()
    res = {"out": out.detach(), "dx": xo.grad}
    if L != S:
        res["dy"] = yo.grad
    return res, {k: v.grad for k, v in sd.items()}, (xq, sd)


@pytest.mark.parametrize("E,H,L,S", [(64, 4, 150, 150), (64, 4, 10, 150), (64, 4, 30, 30), (32, 2, 97, 97), (64, 4, 1, 160),
                                     (64, 4, 160, 33)])
def test_oracle_fp32_vs_fp64_on_the_catalogue(E, H, L, S):
    """``oracle.gapt_ref.mab_forward`` in fp32 against itself in fp64, per jet, at 1e-5 (measured: 5.4e-7 worst on outputs and
    input gradients, 6.2e-7 on parameter gradients -- the reference's own arithmetic leaves the GPU bar of 1e-4 a margin above
    100x under the per-jet metric); everything finite, the dead jet included; the dead jet's attention contributes nothing."""
    names, ign = catalogue(S)
    r64, g64, (xq, sd) = _oracle_run(torch.float64, E, H, L, S, names, ign)
    r32, g32, _ = _oracle_run(torch.float32, E, H, L, S, names, ign)
    for k in r64:
        assert bool(torch.isfinite(r64[k]).all()) and bool(torch.isfinite(r32[k]).all()), k
        err, name, b = worst_jet(r32[k].numpy(), r64[k].numpy(), names)
        print(f"oracle fp32 vs fp64 {L}x{S} E={E} {k}: worst per-jet {err:.3g} ({name}, jet {b})")
        assert err <= 1e-5, (k, name, b, err)
    for k in g64:
        assert bool(torch.isfinite(g32[k]).all()), k
        e = float((g32[k].double() - g64[k]).abs().max() / g64[k].abs().max())
        assert e <= 1e-5, (k, e)
    d = names.index(DEAD)
    from oracle.mpgan_ref import leaky
    z = xq[d].double() + sd["mab.attention.out_proj.bias"].detach()
    want = z + leaky(z @ sd["mab.ff.net.0.weight"].detach().t() + sd["mab.ff.net.0.bias"].detach(), 0.2)
    assert float((r64["out"][d] - want).abs().max()) <= 1e-12 * float(want.abs().max())
    if "dy" in r64:
        assert float(r64["dy"][d].abs().max()) == 0.0
