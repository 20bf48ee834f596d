"""CPU: the host side of the gradient penalty's row route (``ops.OPTIONS["gp_rows"]``): the second-order rule of ``ops.EdgeRowsFn`` /
``ops.EdgeRowsVJPFn`` in fp64 against torch autograd's own double backward through a plain restatement of the edge network, the
routing predicate, the argument checks of ``mpg_knn_edge_jvp`` (which return before any launch) and the declined third derivative."""
import ctypes as C

import pytest
import torch

from mpgan_amd import _lib, ops

H1, H2, H3 = ops.H1, ops.H2, ops.H3
BAR = 1e-10   # the bar of test_oracle_golden.py: fp64 against fp64, the same formulas in another order


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def edge_ref(x, m, P, alpha, keeps, s):
    """agg_i = s sum_j m_j fe([x_i ; x_j]) as MPLayer.forward states it (mpgan/model.py:206-267), keeps explicit."""
    W1, b1, W2, b2, W3, b3 = P
    B, N, F = x.shape
    lre = torch.nn.functional.leaky_relu
    A = torch.cat((x.unsqueeze(2).expand(B, N, N, F), x.unsqueeze(1).expand(B, N, N, F)), 3)
    E = keeps[0] * lre(A @ W1.t() + b1, alpha)
    E = keeps[1] * lre(E @ W2.t() + b2, alpha)
    E = keeps[2] * lre(E @ W3.t() + b3, alpha)
    return s * (E * m.reshape(B, 1, N, 1)).sum(2)


def _case(seed, B=2, N=5, F=3, p=0.5):
    g = torch.Generator().manual_seed(seed)
    r = lambda *shape, sc=1.0: (torch.randn(*shape, generator=g, dtype=torch.float64) * sc)
    P = [r(H1, 2 * F, sc=0.5), r(H1, sc=0.1), r(H2, H1, sc=0.1), r(H2, sc=0.1), r(H3, H2, sc=0.1), r(H3, sc=0.1)]
    x, m = r(B, N, F), torch.rand(B, N, generator=g, dtype=torch.float64) * 0.9 + 0.05
    keeps = [(torch.rand(B, N, N, h, generator=g) >= p).double() / (1 - p) for h in (H1, H2, H3)]
    abar, u, mu = r(B, N, H3), r(B, N, F), r(B, N)
    return P, x, m, keeps, abar, u, mu


def _derivatives(f, P, x, m, abar, u, mu):
    """(value, first-order outputs, gradients of Phi = <u, x_bar> + <mu, m_bar>) of agg = f(x, m, P)."""
    leaves = [t.clone().requires_grad_(True) for t in (abar, x, m, *P)]
    ab, xx, mm, *PP = leaves
    agg = f(xx, mm, PP)
    first = torch.autograd.grad(agg, (xx, mm, *PP), ab, create_graph=True)
    phi = (first[0] * u).sum() + (first[1] * mu).sum()
    second = torch.autograd.grad(phi, leaves)
    return agg.detach(), [t.detach() for t in first], second


@pytest.mark.parametrize("sum_agg", [True, False])
def test_second_order_rule_against_autograd_in_fp64(sum_agg):
    alpha = 0.2
    P, x, m, keeps, abar, u, mu = _case(5)
    s = 1.0 if sum_agg else 1.0 / x.shape[1]
    st = ops.EdgeRowsSettings(sum_agg, alpha, keeps=keeps)
    got = _derivatives(lambda xx, mm, PP: ops.EdgeRowsFn.apply(xx, mm, *PP, st), P, x, m, abar, u, mu)
    ref = _derivatives(lambda xx, mm, PP: edge_ref(xx, mm, PP, alpha, keeps, s), P, x, m, abar, u, mu)
    assert rel(got[0], ref[0]) <= BAR
    names = ["x", "m", "W1", "b1", "W2", "b2", "W3", "b3"]
    for n, a, b in zip(names, got[1], ref[1]):
        assert a.shape == b.shape and rel(a, b) <= BAR, ("first", n, rel(a, b))
    for n, a, b in zip(["abar"] + names, got[2], ref[2]):
        assert a.shape == b.shape and rel(a, b) <= BAR, ("second", n, rel(a, b))


def test_rule_without_a_mask_and_with_one_cotangent_only():
    """No mask (every sender counts once): m_bar is None and Phi = <u, x_bar>; and mu alone (u absent) on the masked op."""
    alpha = 0.2
    P, x, m, keeps, abar, u, mu = _case(7)
    st = ops.EdgeRowsSettings(True, alpha, keeps=keeps)
    ones = torch.ones_like(m)

    def run(f):
        leaves = [t.clone().requires_grad_(True) for t in (abar, x, *P)]
        ab, xx, *PP = leaves
        (xb,) = torch.autograd.grad(f(xx, PP), xx, ab, create_graph=True)
        # (without mu nothing of Phi depends on x or the biases: such a gradient may come back as None, which stands for zeros)
        return [torch.zeros_like(t) if g is None else g for g, t in zip(torch.autograd.grad((xb * u).sum(), leaves, allow_unused=True), leaves)]
    for a, b in zip(run(lambda xx, PP: ops.EdgeRowsFn.apply(xx, None, *PP, st)), run(lambda xx, PP: edge_ref(xx, ones, PP, alpha, keeps, 1.0))):
        assert float((a - b).abs().max()) <= BAR * max(float(b.abs().max()), 1.0)

    def run_mu(f):
        leaves = [t.clone().requires_grad_(True) for t in (abar, x, m, *P)]
        ab, xx, mm, *PP = leaves
        (mb,) = torch.autograd.grad(f(xx, mm, PP), mm, ab, create_graph=True)
        return torch.autograd.grad((mb * mu).sum(), [ab, xx, *PP])
    for a, b in zip(run_mu(lambda xx, mm, PP: ops.EdgeRowsFn.apply(xx, mm, *PP, st)), run_mu(lambda xx, mm, PP: edge_ref(xx, mm, PP, alpha, keeps, 1.0))):
        assert rel(a, b) <= BAR


def _ref_agg(c, keeps, alpha):
    """agg of the case ``c`` of gp_rows_ref with LeakyReLU's own signs: senders weighted by the adjacency and (where there is one) the mask."""
    import gp_rows_ref as R

    def f(xx, mm, PP):
        Z3 = R.pre_activations(xx, PP, keeps, torch.float64)[2]
        E3 = keeps[2] * torch.nn.functional.leaky_relu(Z3, alpha)
        w = c["adj"].double().unsqueeze(3)
        return c["s"] * (E3 * (w if mm is None else w * mm.reshape(c["B"], 1, c["N"], 1))).sum(2)
    return f


@pytest.mark.parametrize("what", ["none", "tail", "tail_constant", "k1"])
def test_rule_with_the_mask_kinds_and_sets_of_the_plan_cases(what):
    """The CPU statement of the rule against autograd in fp64 on what ``gp_rows_ref.PLAN_CASES`` adds to the case table: no mask,
    the jet-like mask (its exact zeros take an m_bar and a dPhi/dm; as a constant they take none) and one neighbour per receiver."""
    import gp_rows_ref as R
    alpha = R.ALPHA
    pc = {"none": R.PlanCase(3, 2, 9, 3, "none", 0.5, True, None, False, False, {}),
          "tail": R.PlanCase(4, 2, 9, 3, "tail", 0.5, False, None, True, False, {}),
          "tail_constant": R.PlanCase(5, 2, 9, 3, "tail", 0.0, True, None, False, False, {}),
          "k1": R.PlanCase(6, 2, 9, 3, "frac", 0.5, True, 1, True, False, {})}[what]
    c = R.make_case(pc)
    B, N = c["B"], c["N"]
    assert (c["m"] is None) == (what == "none")
    if what.startswith("tail"):
        assert bool((c["m"][:, N - N // 3:] == 0).all()) and bool((c["m"][:, :N - N // 3] > 0).all())
    if what == "k1":
        assert bool((c["adj"].sum(2) == 1).all())
    g = torch.Generator().manual_seed(pc.seed)
    keeps = [(torch.rand(B, N, N, h, generator=g) >= pc.p).double() / (1 - pc.p) for h in (H1, H2, H3)]
    st = ops.EdgeRowsSettings(pc.sum_agg, alpha, nbr=None if pc.k is None else c["adj"].double(), k=pc.k or 0, keeps=keeps)
    got = R.derivatives(lambda xx, mm, PP: ops.EdgeRowsFn.apply(xx, mm, *PP, st), c, pc.mask_grad)
    ref = R.derivatives(_ref_agg(c, keeps, alpha), c, pc.mask_grad)
    assert rel(got[0], ref[0]) <= BAR
    for order, a, b in (("first", got[1], ref[1]), ("second", got[2], ref[2])):
        assert list(a) == list(b) and ("m" in a) == pc.mask_grad
        for n in b:
            assert a[n].shape == b[n].shape and rel(a[n], b[n]) <= BAR, (order, n, rel(a[n], b[n]))


def _plan_case_names():
    import gp_rows_ref as R
    return R.PLAN_RUNS


@pytest.mark.parametrize("name, plan", _plan_case_names(), ids=[f"{n}-{p}" for n, p in _plan_case_names()])
def test_plan_case_reaches_what_it_is_there_for(name, plan, monkeypatch):
    """Every ``there_for`` property of a ``gp_rows_ref.PLAN_CASES`` entry, from ``ops.knn_plan`` / ``ops.knn_block_tiles`` as they are
    (and, where the property is one of the data, from the case's own mask and neighbour sets): after a change of the plan this says
    which case stopped covering its path.  No launch, no large tensor."""
    import gp_rows_ref as R
    pc = R.PLAN_CASES[name]
    B, N, k = pc.B, pc.N, pc.k or pc.N
    training_rw = ops.knn_plan(256, N, k, True).RW if "training_rw" in pc.there_for[plan] else None      # (on the chip as it is)
    if plan == "full_blocks":
        monkeypatch.setattr(ops, "NUM_CUS", 1)
    kp = ops.knn_plan(B, N, k, True)
    RW, NW = kp.RW, (N + 31) // 32
    wgs = {}      # workgroup of the jet -> its tiles (first edge row, rows)
    for r0, n in ops.knn_block_tiles(N, k, RW):
        wgs.setdefault(r0 // (RW * k), []).append((r0, n))
    wgs = [wgs[i] for i in sorted(wgs)]
    assert len(wgs) == -(-N // RW) and sum(n for t in wgs for _, n in t) == N * k
    stage = RW * k * ops.KNN_STAGE_BYTES
    assert stage <= ops.KNN_LDS_BYTES
    thr = ops.drop_params(pc.p)[0] if pc.p > 0 else 0
    assert pc.there_for[plan]
    for what in pc.there_for[plan]:
        if what == "tiles_gt4":
            assert max(len(t) for t in wgs) > 4
        elif what == "tiles_eq4_short":
            assert len(wgs[0]) == 4 and wgs[0][-1][1] < 32
        elif what == "training_rw":
            assert RW == training_rw
        elif what == "straddle":
            assert any(r0 // k != (r0 + n - 1) // k for t in wgs for r0, n in t)
        elif what == "short_tile":
            assert any(n < 32 for t in wgs for _, n in t)
        elif what == "short_workgroup":
            assert len(wgs) > 1 and N % RW != 0
        elif what == "receiver_blocks":
            assert len(wgs) > 1
        elif what == "one_tile":
            assert RW == N and all(len(t) == 1 for t in wgs)
        elif what.startswith("words_"):
            assert NW == int(what[6:])
        elif what == "sparse_words":
            assert k < N and NW > 1
        elif what == "k_not_dividing_32":
            assert 32 % k != 0
        elif what == "k1":
            assert k == 1
        elif what == "stage_gt_100k":
            assert stage > 100 * 1024
        elif what == "dmask_three_waves":
            assert N > 128 and pc.mask_grad
        elif what == "dmask_all_threads":
            assert N == 192 and pc.mask_grad
        elif what == "dmask_hits_three_waves":
            adj = R.make_case(name)["adj"]      # [b, receiver, sender]
            hit = [adj[:, lo:hi].any(1) for lo, hi in ((0, 64), (64, 128), (128, N))]
            assert pc.mask_grad and bool((hit[0] & hit[1] & hit[2]).any())
        elif what == "skipped_tile":
            m = R.make_case(name)["m"]
            assert pc.k is None and not pc.mask_grad      # (fully connected: row r of a workgroup has sender r % N; no mu reaches it)
            assert any(bool((m[b, [(r0 + q) % N for q in range(n)]] == 0).all()) for b in range(B) for t in wgs for r0, n in t[4:])
        elif what == "byte_drop":      # (edge_drop_mode of csrc/edge_units.h: bit mode at thr = 128 alone)
            assert thr not in (0, 128)
        elif what == "bit_drop":
            assert thr == 128
        elif what == "no_mask":
            assert pc.kind == "none" and not pc.mask_grad
        elif what == "slice_x":
            assert pc.slice_x
        else:
            raise AssertionError(what)


def test_the_six_first_cases_are_what_they_were():
    """``B`` became a field of the case: the six cases of ``CASES`` keep B = 3, their seeds and their draws."""
    import gp_rows_ref as R
    assert list(R.CASES) == ["n5_sum", "n33_mean_drop", "n40_sparse_jets_drop", "n40_sparse_jets_skipped", "n9_knn4_drop",
                             "n30_two_receivers_per_workgroup"]
    for name in R.CASES:
        c = R.make_case(name)
        assert c["B"] == 3 and c["x"].shape[0] == 3 and not c["slice_x"] and c["m"] is not None
    c = R.make_case("n5_sum")
    g = torch.Generator().manual_seed(1000)
    assert torch.equal(c["P"][0], (torch.randn(H1, 6, generator=g, dtype=torch.float64) * 0.5).float().double())


def test_third_derivative_and_parameter_gradient_cotangents_raise():
    alpha = 0.2
    P, x, m, keeps, abar, u, mu = _case(9)
    st = ops.EdgeRowsSettings(True, alpha, keeps=keeps)
    leaves = [t.clone().requires_grad_(True) for t in (abar, x, m, *P)]
    ab, xx, mm, *PP = leaves
    agg = ops.EdgeRowsFn.apply(xx, mm, *PP, st)
    first = torch.autograd.grad(agg, (xx, mm, *PP), ab, create_graph=True)
    (second,) = torch.autograd.grad((first[0] * u).sum(), ab, create_graph=True)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(second.sum(), xx)
    with pytest.raises(RuntimeError, match="parameter-gradient"):
        torch.autograd.grad((first[2] ** 2).sum(), xx)


def test_gp_rows_route_covers_the_default_discriminator_only():
    from mpgan_amd import train
    on = dict(ops.OPTIONS, gp_rows=True)

    def layers(**kw):
        return train.default_mpgan(30, device="cpu", **kw)[1].mp_layers

    for N in (30, 150):
        assert all(l.gp_rows_ok(16, N, True, on) for l in layers())
    assert not any(l.gp_rows_ok(16, 30, True, dict(ops.OPTIONS, gp_rows=False)) for l in layers())
    assert not any(l.gp_rows_ok(16, 30, False, on) for l in layers())      # outside double_backward_route
    assert not any(l.gp_rows_ok(16, 200, True, on) for l in layers())      # beyond KNN_MAX_N
    assert not ops.OPTIONS["gp_rows"] or "MPG_GP_ROWS" in __import__("os").environ   # off unless asked for
    from mpgan_amd.mpgan import MPLayer
    base = dict(input_node_size=3, fe_layers=[96, 160, 192], fn_layers=[256, 256], output_node_size=32)
    assert MPLayer(**base).gp_rows_ok(4, 30, True, on)
    assert MPLayer(**base, fully_connected=False, num_knn=10).gp_rows_ok(4, 30, True, on)
    for kw in (dict(pos_diffs=True), dict(clabels=1), dict(spectral_norm=True), dict(batch_norm=True), dict(mask_fne_np=True),
               dict(pos_diffs=True, delta_coords=True, delta_r=False, all_ef=False)):
        assert not MPLayer(**base, **kw).gp_rows_ok(4, 30, True, on), kw
    assert not MPLayer(**dict(base, fe_layers=[64, 160, 192])).gp_rows_ok(4, 30, True, on)
    assert not MPLayer(**dict(base, fn_layers=[256])).gp_rows_ok(4, 30, True, on)
    assert not MPLayer(**base, fully_connected=False, num_knn=40).gp_rows_ok(4, 30, True, on)   # k > N


def _jvp_args(**over):
    """A well-formed ``MpgKnnEdgeJvp`` over host dummies (the checks return before anything is read or launched)."""
    buf = (C.c_char * 64)()
    ptr = C.c_void_p((C.addressof(buf) + 15) & ~15)   # (16-byte aligned, as the tangent rows have to be)
    e = _lib.MpgKnnEdgeJvp()
    for f in ("nbr", "mask", "dagg", "ta", "tc", "W2img", "W3img", "b3", "E1", "E2", "sign3", "T1", "T2", "aggt", "rowdot", "dmask"):
        setattr(e, f, ptr)
    e.ld_dagg, e.ld_t, e.B, e.N, e.k, e.RW = H3, H1, 2, 30, 30, 4
    e.alpha, e.agg_scale, e.thr, e.dscale = 0.2, 1.0, 0, 1.0
    for k, v in over.items():
        setattr(e, k, v)
    return e, buf


@pytest.mark.parametrize("over, code", [
    (dict(B=0), -1), (dict(k=31), -1), (dict(N=193, k=5), -1), (dict(RW=0), -1),
    (dict(nbr=None), -2), (dict(dagg=None), -2), (dict(W3img=None), -2), (dict(b3=None), -2), (dict(W2img=None), -2),
    (dict(E1=None, E2=None, sign3=None), -2), (dict(ta=None, tc=None, rowdot=None, dmask=None), -2), (dict(thr=128, seed=None), -2),
    (dict(E1=None), -3), (dict(sign3=None), -3), (dict(tc=None), -3), (dict(rowdot=None), -3),
    (dict(alpha=1.5), -4), (dict(alpha=-0.1), -4),
    (dict(ld_dagg=191), -5), (dict(ld_t=95), -5), (dict(ld_t=98), -5),
    (dict(RW=7), -6),                   # 7 * 30 rows * 784 bytes > 160 KiB
    (dict(B=60000, N=192, k=4, RW=1), -7),   # B * N * N beyond the 32-bit dropout key
])
def test_knn_edge_jvp_refuses_bad_arguments_before_launching(over, code):
    assert "mpg_knn_edge_jvp" in _lib.SIGNATURES
    e, keep = _jvp_args(**over)
    assert _lib.lib().mpg_knn_edge_jvp(C.byref(e), None) == code, over


def test_struct_layout_matches_the_header():
    """Every field of ``MpgKnnEdgeJvp`` at the offset gcc gives it in the header, and the struct's size."""
    import os
    import subprocess
    import tempfile
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    fields = [f[0] for f in _lib.MpgKnnEdgeJvp._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "mpgan_amd.h"\nint main(){'
           + "".join(f'printf("{f} %zu\\n", offsetof(MpgKnnEdgeJvp, {f}));' for f in fields)
           + 'printf("sizeof %zu\\n", sizeof(MpgKnnEdgeJvp));return 0;}')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-I", inc, c, "-o", os.path.join(d, "t")], check=True)
        out = subprocess.run([os.path.join(d, "t")], check=True, capture_output=True, text=True).stdout
    got = {k: int(v) for k, v in (line.split() for line in out.strip().splitlines())}
    assert got.pop("sizeof") == C.sizeof(_lib.MpgKnnEdgeJvp)
    assert got == {f: getattr(_lib.MpgKnnEdgeJvp, f).offset for f in fields}
