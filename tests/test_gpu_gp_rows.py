"""GPU: the gradient penalty's edge aggregation on the row kernels (``ops.OPTIONS["gp_rows"]``: ``ops.EdgeRowsFn`` /
``ops.EdgeRowsVJPFn`` over ``mpg_knn_edge_fwd`` / ``_bwd`` / ``_jvp``) -- the op against fp64 under the kernel's own kink decisions, the
--gp D step against the reference's golden and against the existing route, graph replay, and peak memory."""
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


def _run_op(name):
    """One case through the op on the GPU and through the gated fp64 statement on the CPU, once per session."""
    if name in _op_cache:
        return _op_cache[name]
    from mpgan_amd import ops
    c = R.make_case(name)
    N, F, p = c["N"], c["F"], c["p"]
    dev = torch.device("cuda:0")
    _reset()
    nbr = None if c["k"] is None else R.adjacency_words(c["adj"]).to(dev)
    st = ops.EdgeRowsSettings(c["sum_agg"], R.ALPHA, p, p > 0, None, nbr, c["k"] or 0, None, True)
    holder = {}

    def f(xx, mm, PP):
        agg = ops.EdgeRowsFn.apply(xx, mm, *PP, st)
        holder["st"] = agg.grad_fn.st
        return agg
    g = {k: (v.float().to(dev) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in c.items()}
    g["P"] = [t.float().to(dev) for t in c["P"]]
    got = R.derivatives(f, g, c["mask_grad"])
    s = holder["st"]
    thr, dscale = ops.drop_params(p) if p > 0 else (0, 1.0)
    keeps = [torch.ones(R.B, N, N, h, dtype=torch.float64) for h in (R.H1, R.H2, R.H3)]
    if thr:
        keeps = [ops.dropout_mask(R.B * N * N, h, s.tag + t, thr).double().cpu().reshape(R.B, N, N, h) * dscale
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
    _op_cache[name] = dict(case=c, got=got, ref=ref, flips=flips, total=total, fp32_flips=R.fp32_flips(c, keeps))
    return _op_cache[name]


@pytest.mark.parametrize("name", list(R.CASES))
def test_op_against_fp64_under_the_kernels_own_gates(name):
    """Value, first-order outputs and every second-order output of ``EdgeRowsFn`` against the fp64 restatement evaluated with the gates
    the kernels took (read back from the parked E1 / E2 / sign3 and the call's keep masks).  Where the mask takes a gradient its
    exact zeros still have an m_bar and a dPhi/dm -- whole jets of them here --; where it takes none their tiles are skipped."""
    r = _run_op(name)
    (v, first, second), (rv, rfirst, rsecond) = r["got"], r["ref"]
    errs = {"agg": summary_err("agg", v, summarize("agg", rv))}
    errs.update({"d" + k: summary_err(k, first[k], summarize(k, rfirst[k])) for k in rfirst})
    errs.update({"dPhi/d" + k: summary_err(k, second[k], summarize(k, rsecond[k])) for k in rsecond})
    print(name, {k: f"{e:.2e}" for k, e in errs.items()}, "flips", r["flips"], "of", r["total"], "fp32 flips", r["fp32_flips"])
    for k in rsecond:
        assert bool(torch.isfinite(second[k]).all()), k
    assert max(errs.values()) < BAR, errs
    assert r["flips"] <= FLIP_SHARE * r["total"], (r["flips"], r["total"])
    assert r["fp32_flips"] == 0, "the case's seed: torch fp32 on the CPU flips a sign against fp64"


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
