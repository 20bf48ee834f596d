"""GPU: the fused MPLayer on masks that leave workgroups of the edge kernels WITHOUT senders -- jets with no particle at all,
fewer unmasked senders than sender chunks, whole chunks masked -- and on N > 160, where every chunk lists its own index range.

The masks live in tests/edge_list_cases.py; tests/test_edge_partition_cpu.py asserts (without a GPU) that each of them reaches
the path it is named for under the plan ``ops.edge_plan`` makes today.  Slope 1 unless stated: the layer is smooth and the
fp64 oracle a strict reference.  Bars: ``_assert_smooth_bars`` of tests/test_gpu_mplayer.py (TIGHT on y and the node network's
gradients, TOL on dx and the edge network's), with y and dx judged PER JET against that jet's own largest entry -- an empty
jet's rows (the node path alone) must not hide under a full jet's scale."""
import numpy as np
import pytest
import torch

import edge_list_cases as E
from conftest import rel_err
from test_gpu_mplayer import TIGHT, TOL, _assert_smooth_bars, _dev, _mplayer_shapes, _ref_knn_bits, _run_case

pytestmark = pytest.mark.gpu

CASES = E.cases()


def _options(**kw):
    """Context: ``ops.OPTIONS`` entries set for the block, restored behind it."""
    import contextlib
    from mpgan_amd import ops

    @contextlib.contextmanager
    def cm():
        old = {k: ops.OPTIONS[k] for k in kw}
        ops.OPTIONS.update(kw)
        try:
            yield
        finally:
            ops.OPTIONS.update(old)
    return cm()


def _per_jet(pair):
    got, ref = pair
    return max(rel_err(got[b], ref[b]) for b in range(ref.shape[0]))


def _check(case, F=32, out=32, sum_agg=True, skip=True, alpha=1.0, seed=11, forward_only=False):
    """One case through ``_run_case``: everything finite, y and dx per jet, parameter gradients per tensor.  Returns the tensors."""
    t = {}
    with _options(skip_masked=True):   # (``_run_case`` sets it; restored whatever happens in there)
        errs, _, _ = _run_case(case.B, case.N, F, out, True, sum_agg, seed=seed, skip=skip, alpha=alpha, mask=E.mask_of(case), tensors=t)
    for k, (got, _) in t.items():
        assert np.isfinite(got).all(), (case.name, k)
    errs = dict(errs, y=_per_jet(t["y"]), dx=_per_jet(t["dx"]))
    print(case.name, "F", F, "sum", sum_agg, "skip", skip, "alpha", alpha, "errs (y, dx per jet)", errs)
    if forward_only:
        assert errs["y"] < TIGHT, (case.name, errs["y"])
    else:
        _assert_smooth_bars(errs, case.name)
    return t


# ---- A: empty jets beside full ones (N = 30, B = 4: three sender chunks, whole-list mode)
@pytest.mark.parametrize("skip", [True, False])
@pytest.mark.parametrize("F,out", [(32, 32), (3, 32)])
@pytest.mark.parametrize("sum_agg", [True, False])
def test_empty_jets_beside_full_ones(sum_agg, F, out, skip):
    """Jets with 0, 30, 1 (the last index) and 8 particles.  The mean divides by N, not by the count; the empty jet's y and dx
    are the node path's alone.  ``skip_masked`` off makes the forward list the masked senders too (they add exact zeros)."""
    with _options(fn_epilogue=True):
        _check(CASES["A_empty_beside_full"], F=F, out=out, sum_agg=sum_agg, skip=skip)


def test_empty_jets_on_the_plain_route():
    """The same without the node network as the edge launch's epilogue: mpg_edge_fwd, the chunks' sum, mpg_chain."""
    with _options(fn_epilogue=False):
        _check(CASES["A_empty_beside_full"])


# ---- B: a launch with no sender at all
def test_launch_without_any_sender():
    """Both jets empty: no workgroup of any edge launch has a sender, mpg_edge_dw finds no valid block.  The edge network's
    parameter gradients are exactly zero (and finite: the launch's gradient unit comes from workgroups that had nothing to scale);
    y, dx and the node network's gradients meet the oracle's."""
    t = _check(CASES["B_no_sender"])
    for k, (got, ref) in t.items():
        if k.startswith("fe."):
            assert np.abs(ref).max() == 0.0 and np.abs(got).max() == 0.0, k


# ---- C: one receiver in the last receiver block, senders only in the last tile, beside empty shares
@pytest.mark.parametrize("name", ["C33_last_receiver", "C64_last_tile", "C65_last_receiver"])
def test_last_receiver_block_and_last_tile(name):
    _check(CASES[name])


# ---- D: N = 150
_D16 = {}


def _d16():
    if not _D16:
        _D16.update(_check(CASES["D16_n150"]))
    return _D16


def test_n150_few_senders_in_sixteen_jets():
    """B = 16 (three chunks): jets of 0, 1, 2, 4, 5 and 150 particles at the head and at the tail of the index range."""
    assert _d16()


def test_n150_fewer_senders_than_chunks():
    """B = 2 (seventeen chunks): one particle, and sixteen."""
    _check(CASES["D2_n150"])


# ---- E: index mode, N > 160
@pytest.mark.parametrize("name", ["E161_index_mode", "E192_index_mode"])
def test_index_mode_chunks(name):
    """N = 161: a jet unmasked only in the last (shorter) chunk, a jet with one whole chunk masked; N = 192 (six receiver blocks):
    an empty jet and a jet with one sender per chunk.  Every chunk lists its own index range here."""
    _check(CASES[name])


# ---- F: kNN over an empty jet and over fewer particles than neighbours
@pytest.mark.parametrize("self_loops", [True, False])
def test_knn_with_an_empty_jet_and_fewer_particles_than_neighbours(self_loops):
    import oracle
    from oracle import train_ref as T
    from mpgan_amd import ops
    from mpgan_amd.mpgan import MPLayer
    case, k, F, out = CASES["K_knn"], 10, 32, 32
    B, N = case.B, case.N
    rs = np.random.RandomState(31)
    x64 = torch.from_numpy(rs.normal(0, 0.5, size=(B, N, F))).float().double()   # (fp32 values: both sides sort the same distances)
    g64 = torch.from_numpy(rs.normal(size=(B, N, out)))
    mask64 = torch.from_numpy(E.mask_of(case))
    x = x64.float().to(_dev()).requires_grad_(True)
    mask = mask64.float().to(_dev())
    bits = ops.knn_sets(x.detach(), mask, k, self_loops).cpu().numpy().astype(np.uint32).reshape(B, N)   # N <= 32: one word
    got = ((bits[:, :, None] >> np.arange(N, dtype=np.uint32)[None, None, :]) & 1).astype(bool)
    ref = _ref_knn_bits(x64, mask64, k, self_loops).numpy()
    assert (got == ref).all() and (got.sum(2) == k).all()
    sd64 = T.init_state_dict(_mplayer_shapes(F, out), seed=13, dtype=torch.float64)
    layer = MPLayer(F, [96, 160, 192], [256, 256], out, fully_connected=False, num_knn=k, self_loops=self_loops,
                    leaky_relu_alpha=1.0).to(_dev())
    layer.load_state_dict({kk: v.float() for kk, v in sd64.items()})
    y = layer(x, True, mask)
    (y * g64.float().to(_dev())).sum().backward()
    sdo = {"L." + kk: v.clone().requires_grad_(True) for kk, v in sd64.items()}
    xo = x64.clone().requires_grad_(True)
    yo = oracle.mplayer_forward(sdo, "L", xo, mask64, alpha=1.0, knn=(k, self_loops))
    (yo * g64).sum().backward()
    pairs = {"y": (y.detach(), yo.detach()), "dx": (x.grad, xo.grad)}
    pairs.update({kk: (p.grad, sdo["L." + kk].grad) for kk, p in layer.named_parameters()})
    pairs = {kk: (a.double().cpu().numpy(), b.numpy()) for kk, (a, b) in pairs.items()}
    for kk, (a, _) in pairs.items():
        assert np.isfinite(a).all(), kk
    errs = {kk: rel_err(a, b) for kk, (a, b) in pairs.items()}
    errs.update(y=_per_jet(pairs["y"]), dx=_per_jet(pairs["dx"]))
    print("knn, self loops", self_loops, errs)
    _assert_smooth_bars(errs, ("knn", self_loops))


# ---- G: no contamination across jets
def _hip_rows(case, seed=11):
    """y and dx of the HIP layer alone (no oracle), on the inputs ``_check`` draws for this shape and seed."""
    from oracle import train_ref as T
    from mpgan_amd.mpgan import MPLayer
    B, N, F, out = case.B, case.N, 32, 32
    rs = np.random.RandomState(1000 + seed)
    layer = MPLayer(F, [96, 160, 192], [256, 256], out, leaky_relu_alpha=1.0).to(_dev())
    layer.load_state_dict({k: v.float() for k, v in T.init_state_dict(_mplayer_shapes(F, out), seed=seed, dtype=torch.float64).items()})
    x = torch.from_numpy(rs.normal(0, 0.5, size=(B, N, F))).float().to(_dev()).requires_grad_(True)
    g = torch.from_numpy(rs.normal(size=(B, N, out))).float().to(_dev())
    y = layer(x, True, torch.from_numpy(E.mask_of(case)).float().to(_dev()))
    (y * g).sum().backward()
    torch.cuda.synchronize()
    return y.detach().cpu(), x.grad.cpu()


@pytest.mark.parametrize("name", ["A_empty_beside_full", "D16_n150"])
def test_other_jets_do_not_notice_an_empty_jet(name):
    """The same launch with the empty jets given exactly one particle: the same shape, so the same plan.  The y and dx rows of
    every OTHER jet are bit-identical between the two runs -- a ticket, slab or order mix-up would move them."""
    case = CASES[name]
    filled = E.one_particle_instead_of_none(case)
    assert E.plan(filled.B, filled.N) == E.plan(case.B, case.N)
    y0, dx0 = _hip_rows(case)
    y1, dx1 = _hip_rows(filled)
    same = [b for b in range(case.B) if case.sets[b] == filled.sets[b]]
    changed = [b for b in range(case.B) if b not in same]
    assert same and changed
    for b in same:
        assert torch.equal(y0[b], y1[b]) and torch.equal(dx0[b], dx1[b]), (name, b)
    for b in changed:   # (and the particle is seen where it was put)
        assert not torch.equal(y0[b], y1[b]), (name, b)
    if name == "D16_n150":   # the rows G compares are the rows D judged against the oracle
        assert np.array_equal(_d16()["y"][0], y0.double().numpy())


# ---- H: default slope, once
def test_empty_jets_default_slope_forward():
    """alpha = 0.2 on case A: the forward per jet.  (The gradients of kinked cases stay with tests/test_gpu_mplayer.py.)"""
    _check(CASES["A_empty_beside_full"], alpha=0.2, forward_only=True)
