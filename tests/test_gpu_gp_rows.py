"""GPU: the gradient penalty's edge aggregation on the row kernels (``ops.OPTIONS["gp_rows"]``: ``ops.EdgeRowsFn`` /
``ops.EdgeRowsVJPFn`` over ``mpg_knn_edge_fwd`` / ``_bwd`` / ``_jvp``) -- the op against fp64 under the kernel's own kink decisions (six
small cases, then every launch plan, word count and N up to 192: ``gp_rows_ref.PLAN_CASES``; what they print is kept in
profiles/gp_rows_plan_cases.txt), at other cotangent magnitudes, run twice and with another jet beside it, the --gp D step against the reference's golden and against the existing route, graph replay, and peak memory."""
import itertools

import numpy as np
import pytest
import torch

from conftest import load_golden, summarize, summary_err
import gp_rows_ref as R

pytestmark = pytest.mark.gpu

BAR = 1e-3          # the existing bar of the gradient-penalty checks (test_gpu_train.py)
FLIP_SHARE = 1e-3   # kink decisions of the kernel that differ from fp64's own, as a share of the live, kept elements


def _reset(seed=77, first_tag=300):
    from mpgan_amd import ops
    dev = torch.device("cuda:0")
    ops.set_seed(seed, dev)
    ops.dev_state(dev).tags = itertools.count(first_tag)


def _dense(rows, adj):
    """Row-major edge rows [B * N * k, H] -> [B, N, N, H] (zeros where receiver i does not list sender j; rows ascend in j)."""
    out = torch.zeros(*adj.shape, rows.shape[-1], dtype=torch.float64)
    out[adj] = rows.double().cpu()
    return out


def _sign3_bits(sign3):
    """The parked sign words [rows, 6, 2] -> [rows, 192] bool, True where Z3 <= 0 (bit 4g + t of word (m, h) <-> feature 32m + 8g + 4h + t)."""
    w = sign3.cpu().to(torch.int32) & 0xffff
    bits = ((w.unsqueeze(-1) >> torch.arange(16)) & 1).bool()           # [rows, m, h, (g, t)]
    return bits.reshape(-1, 6, 2, 4, 4).permute(0, 1, 3, 2, 4).reshape(-1, 192)


_op_cache = {}


def _hip(c):
    """The case ``c`` through the op on the GPU, from the same device seed and tag every time: ((value, first-order outputs,
    second-order outputs), the call's ``_RowsState``)."""
    from mpgan_amd import ops
    B, N, F, p = c["B"], c["N"], c["F"], c["p"]
    dev = torch.device("cuda:0")
    _reset()
    nbr = None if c["k"] is None else R.adjacency_words(c["adj"]).to(dev)
    st = ops.EdgeRowsSettings(c["sum_agg"], R.ALPHA, p, p > 0, None, nbr, c["k"] or 0, None, True)
    holder = {}

    def f(xx, mm, PP):
        if c["slice_x"]:   # D's own call: the features of a [B, N, F + 1] tensor without its last column, a view of row stride F + 1
            xx = torch.cat((xx, xx.new_ones(B, N, 1)), 2)[..., :F]
            assert not xx.is_contiguous() and xx.stride(1) == F + 1
        agg = ops.EdgeRowsFn.apply(xx, mm, *PP, st)
        holder["st"] = agg.grad_fn.st
        return agg
    g = {k: (v.float().to(dev) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in c.items()}
    g["P"] = [t.float().to(dev) for t in c["P"]]
    got = R.derivatives(f, g, c["mask_grad"])
    torch.cuda.synchronize()
    assert holder["st"].kp.RW == ops.knn_plan(B, N, c["k"] or N, True).RW
    return got, holder["st"]


def _run_op(name, plan="planned"):
    """One case through the op on the GPU and through the gated fp64 statement on the CPU, once per session and launch plan (the
    caller has patched ``ops.NUM_CUS`` for "full_blocks")."""
    if (name, plan) in _op_cache:
        return _op_cache[name, plan]
    from mpgan_amd import ops
    c = R.make_case(name)
    B, N, p = c["B"], c["N"], c["p"]
    got, s = _hip(c)
    thr, dscale = ops.drop_params(p) if p > 0 else (0, 1.0)
    keeps = [torch.ones(B, N, N, h, dtype=torch.float64) for h in (R.H1, R.H2, R.H3)]
    if thr:
        keeps = [ops.dropout_mask(B * N * N, h, s.tag + t, thr).double().cpu().reshape(B, N, N, h) * dscale
                 for h, t in zip((R.H1, R.H2, R.H3), (ops.TAG_E0, ops.TAG_E1, ops.TAG_E2))]
    torch.cuda.synchronize()
    adj = c["adj"]
    neg = [_dense(s.E1, adj) <= 0, _dense(s.E2, adj) <= 0, _dense(_sign3_bits(s.sign3).double(), adj) > 0]
    G = [k * torch.where(n, torch.full_like(k, R.ALPHA), torch.ones_like(k)) for k, n in zip(keeps, neg)]
    ref = R.derivatives(lambda xx, mm, PP: R.gated_agg(xx, mm, PP, G, c["s"], adj), c, c["mask_grad"])
    # the kernel's kink decisions against fp64's own, on the elements where a decision exists
    z64 = R.pre_activations(c["x"], c["P"], keeps, torch.float64)
    where = R.live_kept(c, keeps)
    flips = sum(int((((z <= 0) != n) & w).sum()) for z, n, w in zip(z64, neg, where))
    total = sum(int(w.sum()) for w in where)
    _op_cache[name, plan] = dict(case=c, got=got, ref=ref, flips=flips, total=total, fp32_flips=R.fp32_flips(c, keeps), RW=s.kp.RW)
    return _op_cache[name, plan]


def _second_errs(second, rsecond):
    return {"dPhi/d" + k: summary_err(k, second[k], summarize(k, rsecond[k])) for k in rsecond}


def _check_against_fp64(r, what):
    (v, first, second), (rv, rfirst, rsecond) = r["got"], r["ref"]
    errs = {"agg": summary_err("agg", v, summarize("agg", rv))}
    errs.update({"d" + k: summary_err(k, first[k], summarize(k, rfirst[k])) for k in rfirst})
    errs.update(_second_errs(second, rsecond))
    print(what, {k: f"{e:.2e}" for k, e in errs.items()}, "flips", r["flips"], "of", r["total"], "fp32 flips", r["fp32_flips"])
    for k in rsecond:
        assert bool(torch.isfinite(second[k]).all()), k
    assert max(errs.values()) < BAR, errs
    assert r["flips"] <= FLIP_SHARE * r["total"], (r["flips"], r["total"])
    assert r["fp32_flips"] == 0, "the case's seed: torch fp32 on the CPU flips a sign against fp64"


@pytest.mark.parametrize("name", list(R.CASES))
def test_op_against_fp64_under_the_kernels_own_gates(name):
    """Value, first-order outputs and every second-order output of ``EdgeRowsFn`` against the fp64 restatement evaluated with the gates
    the kernels took (read back from the parked E1 / E2 / sign3 and the call's keep masks).  Where the mask takes a gradient its
    exact zeros still have an m_bar and a dPhi/dm -- whole jets of them here --; where it takes none their tiles are skipped."""
    _check_against_fp64(_run_op(name), name)


@pytest.mark.parametrize("name, plan", R.PLAN_RUNS, ids=[f"{n}-{p}" for n, p in R.PLAN_RUNS])
def test_op_against_fp64_at_every_plan_word_count_and_n_to_192(name, plan, monkeypatch):
    """The same check, bars included, on ``gp_rows_ref.PLAN_CASES``: the launch shapes the six cases above never take -- more than
    four tiles per workgroup, the training batch's RW, N = 150 and 192, sparse sets over several words, byte-mode dropout, no mask, x
    as a strided view.  tests/test_gp_rows_cpu.py asserts from the plan that each case reaches what it is there for."""
    from mpgan_amd import ops
    pc = R.PLAN_CASES[name]
    k = pc.k or pc.N
    if plan == "full_blocks":
        monkeypatch.setattr(ops, "NUM_CUS", 1)
        assert ops.knn_plan(pc.B, pc.N, k, True).RW == max(1, min(pc.N, ops.KNN_WG_ROWS // k))
    r = _run_op(name, plan)
    assert r["RW"] == ops.knn_plan(pc.B, pc.N, k, True).RW
    _check_against_fp64(r, f"{name} {plan} RW {r['RW']}")


@pytest.mark.parametrize("exp", [-30, 12])
@pytest.mark.parametrize("name", ["n33_mean_drop", "n9_knn4_drop"])
def test_second_order_outputs_at_other_cotangent_magnitudes(name, exp):
    """``u`` and ``mu`` times 2^exp (a cotangent has no fixed scale: the tangent rows are split hi + lo in a power-of-two unit of
    their own row).  The first-order outputs do not depend on them and come out bit-identical; Phi is linear in them and the gates
    are those of the unscaled run, so the fp64 reference is the unscaled one times 2^exp, exactly, and every second-order output meets
    the same relative bar against it."""
    base = _run_op(name)
    c = dict(base["case"])
    c["u"], c["mu"] = c["u"] * 2.0 ** exp, c["mu"] * 2.0 ** exp
    assert torch.equal(c["u"].float().double(), c["u"]) and torch.equal(c["mu"].float().double(), c["mu"])   # (fp32-representable)
    (v, first, second), _ = _hip(c)
    assert torch.equal(v, base["got"][0])
    for k, t in base["got"][1].items():
        assert torch.equal(first[k], t), k
    errs = _second_errs(second, {k: t * 2.0 ** exp for k, t in base["ref"][2].items()})
    print(name, "2^%d" % exp, {k: f"{e:.2e}" for k, e in errs.items()})
    for k in second:
        assert bool(torch.isfinite(second[k]).all()), k
    assert max(errs.values()) < BAR, errs


def _all_outputs(got):
    v, first, second = got
    return {"agg": v, **{"d" + k: t for k, t in first.items()}, **{"dPhi/d" + k: t for k, t in second.items()}}


@pytest.mark.parametrize("name", ["n30_training_plan", "n150_knn20"])
def test_op_repeats_itself_bit_for_bit(name, monkeypatch):
    """Two runs from the same seeds and tags under the full-blocks plan: every sum is taken in a fixed order, without atomics."""
    from mpgan_amd import ops
    monkeypatch.setattr(ops, "NUM_CUS", 1)
    c = R.make_case(name)
    one, two = _all_outputs(_hip(c)[0]), _all_outputs(_hip(c)[0])
    for k in one:
        assert torch.equal(one[k], two[k]), k


PER_NODE = ("agg", "dx", "dm", "dPhi/dabar", "dPhi/dx", "dPhi/dm")   # (parameter gradients are sums over the jets)


@pytest.mark.parametrize("name, plan", [("n150_knn20", "full_blocks"), ("n150_fc", "planned")])
def test_a_jets_rows_are_unmoved_by_its_neighbour_in_the_launch(name, plan, monkeypatch):
    """B = 2, then jet 0's x, m, a_bar, u and mu redrawn (with x its neighbour sets) and jet 1 untouched: jet 1's per-node outputs
    of both orders are bit-identical, jet 0's are not.  HIP against HIP: no reference takes part."""
    from mpgan_amd import ops
    if plan == "full_blocks":
        monkeypatch.setattr(ops, "NUM_CUS", 1)
    c1, other = R.make_case(name, B=2), R.make_case(name, seed=R.case_fields(name)[0] + 1, B=2)
    c2 = dict(c1)
    for key in ("x", "m", "abar", "u", "mu", "adj"):
        c2[key] = torch.cat((other[key][:1], c1[key][1:]))
        assert torch.equal(c2[key][1], c1[key][1])
    assert not torch.equal(c2["x"][0], c1["x"][0])
    (got1, st1), (got2, st2) = _hip(c1), _hip(c2)
    assert st1.kp.RW == st2.kp.RW == ops.knn_plan(2, c1["N"], c1["k"] or c1["N"], True).RW
    one, two = _all_outputs(got1), _all_outputs(got2)
    for k in PER_NODE:
        assert torch.equal(one[k][1], two[k][1]), k
        assert not torch.equal(one[k][0], two[k][0]), k


def _gp_step(loss, g, gp_rows):
    from oracle import train_ref as T
    from mpgan_amd import train
    B, N = g["data"].shape[:2]
    G, D = train.default_mpgan(N, disc_dropout=0.0, loss=loss)
    G.load_state_dict(T.init_state_dict(T.mpgan_param_shapes(True), 41, torch.float32))
    D.load_state_dict(T.init_state_dict(T.mpgan_param_shapes(False), 42, torch.float32))
    ts = train.TrainStep(G, D, B, N, use_graphs=False, loss=loss, gp_lambda=float(g["gp_lambda"]), lr_disc=0.0, gp_rows=gp_rows)
    ts.set_batch(torch.from_numpy(g["data"]).float().cuda(), torch.from_numpy(g["labels"]).float().cuda())
    nD = torch.from_numpy(g["noise_D"]).float().cuda()
    ts.fixed_noise = (nD, nD)
    ts.fixed_alpha = torch.from_numpy(g["alpha"]).float().cuda()
    ts._seg_D()
    torch.cuda.synchronize()
    return ts, D


@pytest.mark.parametrize("loss", ["w", "ls"])
def test_gradient_penalty_step_on_the_rows_route_vs_reference_golden(loss):
    """``test_gradient_penalty_step_vs_reference_golden`` with ``gp_rows=True``: the same golden, assertions and tolerances."""
    from mpgan_amd import ops
    g = load_golden(f"gp_step_mpgan_{loss}.npz")
    log = ops.dev_state(torch.device("cuda:0")).tag_log = []
    try:
        ts, D = _gp_step(loss, g, True)
    finally:
        ops.dev_state(torch.device("cuda:0")).tag_log = None
    assert sum(1 for kind, *_ in log if kind == "edge_rows") == len(D.mp_layers)     # (the route was taken, by every layer)
    print(loss, "GP", float(ts.GP), "golden", float(g["gp"]))
    assert abs(float(ts.GP) - float(g["gp"])) < 1e-3 * abs(float(g["gp"]))
    assert abs(float(ts.D_loss) - (float(g["Dr"]) + float(g["Df"]))) < 1e-4 * max(abs(float(g["Dr"]) + float(g["Df"])), 1e-3)
    assert abs(float(ts.D_loss) + float(ts.GP) - float(g["D_loss"])) < 1e-3 * abs(float(g["D_loss"]))
    errs = {k: summary_err(k, p.grad, g["gradD__" + k]) for k, p in D.named_parameters()}
    print({k: f"{e:.2e}" for k, e in errs.items()})
    for k, e in errs.items():
        assert e < 1e-3, (k, e)


def _route_step(model, loss, gp_rows, B=4, N=30, pos_diffs=False):
    from oracle import train_ref as T
    from oracle.train_ref import synthetic_batch
    from mpgan_amd import train
    lat = 32
    if model == "gapt":
        G, D = train.default_gapt(N, disc_dropout=0.0)
        G.load_state_dict(T.init_state_dict(T.gapt_param_shapes(True), 41, torch.float32))
        D.load_state_dict(T.init_state_dict(T.gapt_param_shapes(False), 42, torch.float32))
        lat = 64
    else:
        G, D = train.default_mpgan(N, disc_dropout=0.0, loss=loss)
        G.load_state_dict(T.init_state_dict(T.mpgan_param_shapes(True), 41, torch.float32))
        if pos_diffs:
            from mpgan_amd.mpgan import MPDiscriminator
            torch.manual_seed(11)
            D = MPDiscriminator(mp_iters=2, num_particles=N, hidden_node_size=32, input_node_size=3, fe_layers=[96, 160, 192],
                                fn_layers=[256, 256], final_activation="", dea=True, dea_sum=True, fnd=[],
                                mp_args=dict(pos_diffs=True, delta_r=True, all_ef=False, delta_coords=False, sum=True),
                                linear_args=dict(leaky_relu_alpha=0.2, dropout_p=0.0), mask_args=dict(mask_c=True)).cuda()
        else:
            D.load_state_dict(T.init_state_dict(T.mpgan_param_shapes(False), 42, torch.float32))
    data, labels = synthetic_batch(B, N, seed=13)
    ts = train.TrainStep(G, D, B, N, latent=lat, use_graphs=False, loss=loss, gp_lambda=10.0, lr_disc=0.0, gp_rows=gp_rows)
    ts.set_batch(data.cuda(), labels.cuda())
    gen = torch.Generator(device="cuda").manual_seed(2)
    nz = torch.randn(B, N, lat, device="cuda", generator=gen) * 0.2
    ts.fixed_noise = (nz, nz)
    ts.fixed_alpha = torch.rand(B, 1, 1, device="cuda", generator=gen)
    ts._seg_D()
    torch.cuda.synchronize()
    return float(ts.GP), {k: p.grad.clone() for k, p in D.named_parameters()}


@pytest.mark.parametrize("loss", ["w", "ls"])
def test_rows_route_agrees_with_the_existing_route(loss):
    gp0, g0 = _route_step("mpgan", loss, False)
    gp1, g1 = _route_step("mpgan", loss, True)
    print(loss, "GP", gp0, gp1)
    assert gp0 > 0 and abs(gp1 - gp0) < 1e-3 * abs(gp0)
    errs = {k: summary_err(k, g1[k], summarize(k, g0[k])) for k in g0}
    print({k: f"{e:.2e}" for k, e in errs.items()})
    assert max(errs.values()) < BAR, errs


@pytest.mark.parametrize("model, pos_diffs", [("mpgan", True), ("gapt", False)])
def test_layers_the_route_does_not_cover_are_untouched_by_the_option(model, pos_diffs):
    """A ``pos_diffs`` discriminator and the attention discriminator: bit-identical with the option on and off."""
    gp0, g0 = _route_step(model, "w", False, pos_diffs=pos_diffs)
    gp1, g1 = _route_step(model, "w", True, pos_diffs=pos_diffs)
    assert gp0 == gp1 and gp0 > 0
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k


def _two_steps(use_graphs):
    from oracle import train_ref as T
    from oracle.train_ref import synthetic_batch
    from mpgan_amd import train, ops
    B, N = 8, 30
    dev = torch.device("cuda:0")
    torch.manual_seed(5)
    _reset(seed=4242, first_tag=9000)
    G, D = train.default_mpgan(N, disc_dropout=0.5, loss="w")
    G.load_state_dict(T.init_state_dict(T.mpgan_param_shapes(True), 41, torch.float32))
    D.load_state_dict(T.init_state_dict(T.mpgan_param_shapes(False), 42, torch.float32))
    data, labels = synthetic_batch(B, N, seed=13)
    ts = train.TrainStep(G, D, B, N, use_graphs=use_graphs, loss="w", gp_lambda=10.0, gp_rows=True)
    ts.set_batch(data.cuda(), labels.cuda())
    gen = torch.Generator(device="cuda").manual_seed(2)
    ts.fixed_noise = (torch.randn(B, N, 32, device="cuda", generator=gen) * 0.2, torch.randn(B, N, 32, device="cuda", generator=gen) * 0.2)
    ts.fixed_alpha = torch.rand(B, 1, 1, device="cuda", generator=gen)
    torch.manual_seed(6)
    _reset(seed=4242, first_tag=9000)
    if use_graphs:
        ts.capture(warmup=0)
    for _ in range(2):
        if not use_graphs:   # (a captured step keeps the dropout sites it was captured with: the eager steps take the same ones)
            ops.dev_state(dev).tags = itertools.count(9000)
        ts.step()
    torch.cuda.synchronize()
    return ts.fD.flat.clone(), ts.fG.flat.clone(), float(ts.D_loss), float(ts.GP), float(ts.G_loss)


def test_rows_route_with_dropout_graph_replay_equals_eager_and_reruns():
    """The --gp iteration on the rows route with disc_dropout = 0.5: the penalty's edge dropout comes from the device seed and the
    tag allocator, so the captured iteration replays what eager execution computes, and a second run from the same seeds repeats it."""
    eager, graph, again = _two_steps(False), _two_steps(True), _two_steps(True)
    for a, b in ((eager, graph), (graph, again)):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2:] == b[2:], (a[2:], b[2:])
    assert eager[3] > 0


def test_rows_route_takes_less_memory_than_the_existing_route():
    """Peak allocation of one --gp D step at B = 16, N = 30, both routes measured here one after the other."""
    peaks = {}
    for gp_rows in (False, True):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        _route_step("mpgan", "w", gp_rows, B=16)
        peaks[gp_rows] = torch.cuda.max_memory_allocated() - base
    print("peak bytes of the D step: existing route", peaks[False], "rows route", peaks[True])
    assert peaks[True] < peaks[False], peaks
