"""GPU: bulk generation as a row stream (``gen.JetSampler``, csrc/sampler.hip).  Every row is recomputed on the test's side from
(key, row) -- the label by the host twin of the draw, the noise under the chunk's seed word, the jet by an eager
``generate_parts`` and ``data.unnormalise_jets`` -- and compared bit for bit; the stream's state (cursor, ticket, seed) is read
back after the launches.  Generators at their real widths, chunks of 3 or 4 jets: the smallest shapes at which a chunk is short,
the cursor moves more than once and a jet crosses a 32-receiver block (N = 33)."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu

CHUNK, TOTAL = 3, 8        # three chunks, the last one short by one jet


def _table(N):
    """[0, 1/N, ..., 1] as ``JetArrayDataset.jet_features`` forms its values (the product with the reciprocal): entry k is a jet
    of k real particles -- none, one, ..., all N."""
    return torch.from_numpy(np.arange(N + 1, dtype=np.float32) * np.float32(1.0 / N))


def _nets(model, N):
    from mpgan_amd import train
    torch.manual_seed(0)
    G, _ = (train.default_mpgan if model == "mpgan" else train.default_gapt)(N)
    return G.eval(), (32 if model == "mpgan" else 64)


def _seed_with_both_ends(N, rows=TOTAL):
    """A sampler seed under which the first ``rows`` rows draw a label 0 and a label 1 (host twin; a fixed search order)."""
    from mpgan_amd import gen, ops
    for seed in range(1, 4000):
        idx = ops.label_pick_indices(gen.sampler_key(seed), 0, rows, N + 1).tolist()
        if 0 in idx and N in idx:
            return seed
    raise AssertionError("no seed below 4000 draws both ends of the table")


def _rebuild_chunk(G, latent, N, table, key, c, jet_type):
    """Chunk c of the stream as the header states it, from the module path: (jets [CHUNK, N, 3], mask [CHUNK, N], the module's
    own G(noise, labels) un-normalised)."""
    from mpgan_amd import data, ops
    idx = ops.label_pick_indices(key, c * CHUNK, CHUNK, table.numel())
    labels = table[idx].reshape(CHUNK, 1).cuda()
    seed_t = torch.tensor([ops.u64_as_i64(ops.chunk_seed(key, c))], dtype=torch.int64, device="cuda")
    noise, mask, ign = ops.normal_noise_masked((CHUNK, N, latent), 0.2, labels, seed_t=seed_t)
    with torch.no_grad():
        feat, _, _ = G.generate_parts(noise, labels, feat_out=torch.empty(CHUNK, N, 3, device="cuda"), premask=(mask, ign))
        want = data.unnormalise_jets(torch.cat((feat, mask.unsqueeze(2) - 0.5), 2), jet_type)
        module = data.unnormalise_jets(G(noise, labels), jet_type)
    return want, mask, module, idx


@pytest.mark.parametrize("model,N", [("mpgan", 1), ("mpgan", 30), ("mpgan", 33), ("gapt", 30)])
def test_rows_equal_the_module_path(model, N):
    from mpgan_amd import gen
    G, latent = _nets(model, N)
    table = _table(N)
    seed = _seed_with_both_ends(N)
    s = gen.JetSampler(G, table, N, jet_type="t", chunk=CHUNK, model=model, seed=seed, with_mask=True)
    assert s.key == gen.sampler_key(seed) and s.parts and s.premask
    jets, masks = s.sample(TOTAL)
    torch.cuda.synchronize()
    assert jets.shape == (TOTAL, N, 3) and masks.shape == (TOTAL, N)
    drawn = []
    for c in range(-(-TOTAL // CHUNK)):
        want, mask, module, idx = _rebuild_chunk(G, latent, N, table, s.key, c, "t")
        k = min(CHUNK, TOTAL - c * CHUNK)
        rows = slice(c * CHUNK, c * CHUNK + k)
        assert torch.equal(jets[rows], want[:k]), (c, float((jets[rows] - want[:k]).abs().max()))
        assert torch.equal(masks[rows], mask[:k]), c
        err = rel_err(jets[rows].cpu().numpy(), module[:k].cpu().numpy())
        print(f"{model} N={N} chunk {c}: rel err against G(noise, labels) = {err:.3g}")
        assert err < 1e-6, (c, err)
        assert torch.equal(masks[rows].sum(1).cpu(), idx[:k].float()), c       # table entry k: k real particles
        drawn += idx[:k].tolist()
    assert 0 in drawn and N in drawn            # a jet without a real particle and a full one were among the rows
    empty = drawn.index(0)
    assert not bool(jets[empty].any()) and not bool(masks[empty].any())
    assert bool((jets[..., 2] >= 0).all())


def test_short_last_chunk_writes_nothing_beyond_total():
    from mpgan_amd import gen
    N = 30
    G, _ = _nets("mpgan", N)
    s = gen.JetSampler(G, _table(N), N, chunk=CHUNK, seed=5, with_mask=True)
    buf, mbuf = torch.full((11, N, 3), -7.0, device="cuda"), torch.full((11, N), -7.0, device="cuda")
    jets, masks = s.sample(TOTAL, out=buf[:TOTAL], mask_out=mbuf[:TOTAL])
    torch.cuda.synchronize()
    assert jets.data_ptr() == buf.data_ptr() and masks.data_ptr() == mbuf.data_ptr()
    assert bool((buf[TOTAL:] == -7.0).all()) and bool((mbuf[TOTAL:] == -7.0).all())      # the three rows behind: intact
    assert not bool((mbuf[:TOTAL] == -7.0).any()) and bool(((mbuf[:TOTAL] == 0) | (mbuf[:TOTAL] == 1)).all())
    assert s.position == 9 and int(s._ticket.item()) == 0                              # three chunks of 3
    from mpgan_amd import ops
    assert int(s.seed.item()) & (2**64 - 1) == ops.chunk_seed(s.key, 3)                # ... and the next chunk's seed word


def test_captured_equals_eager_and_a_new_out_needs_no_recapture():
    from mpgan_amd import gen
    N = 30
    G, _ = _nets("mpgan", N)
    cap = gen.JetSampler(G, _table(N), N, chunk=CHUNK, seed=9, use_graphs=True)
    eag = gen.JetSampler(G, _table(N), N, chunk=CHUNK, seed=9, use_graphs=False)
    a, b = cap.sample(9), eag.sample(9)
    torch.cuda.synchronize()
    assert cap._graph is not None and eag._graph is None
    assert torch.equal(a, b) and bool(a.any())
    graph = cap._graph
    mine = torch.full((5, N, 3), -7.0, device="cuda")                # caller-owned, another address, another length
    a2 = cap.sample(5, out=mine)
    b2 = eag.sample(5)
    torch.cuda.synchronize()
    assert cap._graph is graph                                       # no recapture
    assert a2.data_ptr() == mine.data_ptr() and torch.equal(a2, b2)
    assert not torch.equal(a2, a[:5])                                # the stream went on: rows 9 .. 13
    assert cap.position == eag.position == 15
    assert G.training is False


def test_labels_are_a_function_of_the_row():
    from mpgan_amd import gen, ops
    N = 30
    G, _ = _nets("mpgan", N)
    want = ops.label_pick_indices(gen.sampler_key(3), 0, 12, N + 1)
    for chunk in (3, 4):
        s = gen.JetSampler(G, _table(N), N, chunk=chunk, seed=3, with_mask=True)
        jets, masks = s.sample(12)
        torch.cuda.synchronize()
        assert torch.equal(masks.sum(1).long().cpu(), want), chunk
        # particles that are not real are three zeros, real ones are not (eta_rel = tanh(.) * max is zero for no real particle)
        assert torch.equal((jets != 0).any(2).sum(1).cpu(), want), chunk
        assert bool((((jets[..., 2] != 0).sum(1)).cpu() <= want).all()), chunk     # pT: clamped at zero, so at most as many


def test_resume():
    from mpgan_amd import gen
    N = 30
    G, _ = _nets("mpgan", N)
    whole = gen.JetSampler(G, _table(N), N, chunk=CHUNK, seed=21).sample(12)
    first = gen.JetSampler(G, _table(N), N, chunk=CHUNK, seed=21)
    head = first.sample(6)
    sd = first.state_dict()
    assert sd == {"key": gen.sampler_key(21), "cursor": 6, "chunk": CHUNK, "n": N + 1}
    second = gen.JetSampler(G, _table(N), N, chunk=CHUNK, seed=99)          # (another key: the saved one takes over)
    second.load_state_dict(sd)
    tail = second.sample(6)
    torch.cuda.synchronize()
    assert torch.equal(torch.cat((head, tail)), whole)
    assert second.state_dict() == dict(sd, cursor=12)
    with pytest.raises(ValueError):
        gen.JetSampler(G, _table(N - 1), N, chunk=CHUNK, seed=21).load_state_dict(sd)      # another n
    with pytest.raises(ValueError):
        gen.JetSampler(G, _table(N), N, chunk=4, seed=21).load_state_dict(sd)              # another chunk


def test_entry_points_refuse_what_the_header_says():
    from mpgan_amd import _lib
    L = _lib.lib()
    table, labels = torch.zeros(3, device="cuda"), torch.zeros(2, device="cuda")
    feat, mask, out = torch.ones(2, 2, 3, device="cuda"), torch.ones(2, 2, device="cuda"), torch.zeros(2, 2, 3, device="cuda")
    cur, seed = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    tk = torch.zeros(1, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    pick = lambda **kw: L.mpg_label_pick(kw.get("table", p(table)), kw.get("n", 3), 1, kw.get("cur", p(cur)), kw.get("B", 2),
                                         kw.get("labels", p(labels)), None)
    for bad in (dict(n=0), dict(n=2**31), dict(B=0), dict(table=None), dict(cur=None), dict(labels=None)):
        assert pick(**bad) == -1, bad
    f3 = (C.c_float * 3)(1.0, 1.0, 1.0)
    fin = lambda **kw: L.mpg_jets_finish(kw.get("feat", p(feat)), kw.get("ld", 3), p(mask), kw.get("B", 2), kw.get("N", 2),
                                         kw.get("maxes", f3), f3, f3, kw.get("out", p(out)), None, 0, kw.get("total", 2), 1,
                                         kw.get("cur", p(cur)), kw.get("seed", p(seed)), kw.get("tk", p(tk)), None)
    for bad in (dict(B=0), dict(N=0), dict(total=-1), dict(feat=None), dict(out=None), dict(cur=None), dict(seed=None), dict(tk=None),
                dict(ld=2), dict(maxes=None)):
        assert fin(**bad) == -1, bad
    torch.cuda.synchronize()
    assert int(cur.item()) == 0 and int(seed.item()) == 0 and int(tk.item()) == 0 and not bool(out.any()) and not bool(labels.any())


def test_finish_is_unnormalise_jets_bit_for_bit():
    """``ops.jets_finish`` alone on values a generator does not reach -- pT on both sides of the clamp, masks on both sides of the
    threshold, a [B, N, 4] input read in place, B N no multiple of a workgroup, several workgroups -- against
    ``data.unnormalise_jets`` for every jet type."""
    from mpgan_amd import data, ops
    g = torch.Generator(device="cuda").manual_seed(2)
    B, N = 7, 41                      # 287 particles: two workgroups, the second partly empty
    x4 = torch.rand(B, N, 4, device="cuda", generator=g) * 2 - 1
    mask = (torch.rand(B, N, device="cuda", generator=g) < 0.6).float()
    mask[0, :4] = torch.tensor([0.99999994, 1.0, 1.5, 0.0], device="cuda")    # (the next float below 1 is not real)
    mask[1, :3] = 1.0
    x4[..., 3] = mask - 0.5                                                   # the generator's mask column
    x4[1, :3, 2] = torch.tensor([-0.5, -0.50000006, -0.49999997], device="cuda")   # pT at the clamp and on either side of it
    for jt in ("g", "q", "t"):
        want = data.unnormalise_jets(x4, jt)
        for feat in (x4, x4[..., :3].contiguous()):
            cur, seed = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
            tk = torch.zeros(1, dtype=torch.int32, device="cuda")
            out, mo = torch.full((B, N, 3), -7.0, device="cuda"), torch.full((B, N), -7.0, device="cuda")
            ops.jets_finish(feat, mask.contiguous(), out, maxes=data.FEATURE_MAXES[jt], norms=data.FEATURE_NORMS,
                            shifts=data.FEATURE_SHIFTS, key=77, cursor=cur, seed=seed, ticket=tk, mask_out=mo)
            torch.cuda.synchronize()
            assert torch.equal(out, want), (jt, feat.shape)
            assert torch.equal(mo, (x4[..., 3] >= 0.5).float())
            assert int(cur.item()) == B and int(tk.item()) == 0 and int(seed.item()) & (2**64 - 1) == ops.chunk_seed(77, 1)
    # no mask: all real
    out = torch.empty(B, N, 3, device="cuda")
    ops.jets_finish(x4, None, out, maxes=data.FEATURE_MAXES["g"], norms=data.FEATURE_NORMS, shifts=data.FEATURE_SHIFTS, key=77,
                    cursor=cur, seed=seed, ticket=tk, row0=B)
    assert torch.equal(out, data.unnormalise_jets(x4, "g", mask=False))


def test_seed_word_argument_of_the_noise_launches():
    """``seed_t=`` is the device seed's stand-in: a tensor holding the device seed's value draws the default call's values (the
    device seed itself is only read here), another value draws others; ``out=`` is written in place."""
    from mpgan_amd import ops
    mine = torch.tensor([ops.u64_as_i64(ops.get_seed("cuda"))], dtype=torch.int64, device="cuda")
    other = torch.tensor([ops.u64_as_i64(ops.get_seed("cuda") + 1)], dtype=torch.int64, device="cuda")
    labels = torch.tensor([[0.5], [1.0]], device="cuda")
    a = ops.normal_noise((2, 5, 4), 0.2, site=3)
    buf = torch.empty(2, 5, 4, device="cuda")
    b = ops.normal_noise((2, 5, 4), 0.2, site=3, seed_t=mine, out=buf)
    assert b.data_ptr() == buf.data_ptr() and torch.equal(a, b)
    assert not torch.equal(a, ops.normal_noise((2, 5, 4), 0.2, site=3, seed_t=other))
    za, ma, ia = ops.normal_noise_masked((2, 5, 4), 0.2, labels, site=3)
    zb, mb, ib = ops.normal_noise_masked((2, 5, 4), 0.2, labels, site=3, seed_t=mine, out=buf)
    assert zb.data_ptr() == buf.data_ptr() and torch.equal(za, zb) and torch.equal(ma, mb) and torch.equal(ia, ib)
    assert torch.equal(za, a) and ma.sum(1).tolist() == [2.0, 5.0]
    with pytest.raises(ValueError):
        ops.normal_noise((2, 5, 4), 0.2, seed_t=mine.int())
    with pytest.raises(ValueError):
        ops.normal_noise((2, 5, 4), 0.2, out=torch.empty(2, 5, 3, device="cuda"))


def test_a_generator_without_generate_parts_runs_as_a_module():
    """The fallback: ``G(noise, labels)`` and ``jets_finish`` on its [chunk, N, 4] rows -- the same stream, the same jets."""
    from mpgan_amd import gen

    class Plain(torch.nn.Module):
        def __init__(self, G):
            super().__init__()
            self.G = G

        def forward(self, x, labels):
            return self.G(x, labels)

    N = 30
    G, _ = _nets("mpgan", N)
    a = gen.JetSampler(G, _table(N), N, chunk=CHUNK, seed=4).sample(TOTAL)
    s = gen.JetSampler(Plain(G), _table(N), N, chunk=CHUNK, seed=4, with_mask=True)
    assert not s.parts and not s.premask
    b, m = s.sample(TOTAL)
    torch.cuda.synchronize()
    assert rel_err(b.cpu().numpy(), a.cpu().numpy()) < 1e-6
    assert torch.equal((b != 0).any(2), m.bool())


def test_evaluate_generator_with_a_sampler():
    from mpgan_amd import data, evaluation as ev, gen
    N = 30
    G, _ = _nets("mpgan", N)
    x, labels = data.synthetic_jets(200, N, seed=4)
    real = data.unnormalise_jets(x, "g").cuda()
    keys = ("w1p", "w1m", "w1efp")
    kw = dict(num_samples=200, keys=keys, num_w1_eval_samples=100)
    plain = ev.evaluate_generator(G, real, "g", rng=np.random.RandomState(0), **kw)
    s = gen.JetSampler(G, labels, N, chunk=64, seed=1)
    mine = ev.evaluate_generator(G, real, "g", rng=np.random.RandomState(0), sampler=s, **kw)
    assert sorted(mine) == sorted(plain) == sorted(keys)
    for k in keys:
        assert len(mine[k]) == len(plain[k]) == 1 and np.shape(mine[k][0]) == np.shape(plain[k][0]), k
        assert np.all(np.isfinite(mine[k][0])), k
    assert s.position == 256                                                   # four chunks of 64
    with pytest.raises(ValueError):
        ev.evaluate_generator(G, real, "q", sampler=s, **kw)                   # the sampler un-normalises for its own jet type
