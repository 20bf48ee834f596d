"""GPU: the full G+D iteration on the fused path vs goldens captured from the reference modules."""
import numpy as np
import pytest
import torch

from conftest import load_golden, summarize, rel_err, summary_err, assert_grads

pytestmark = pytest.mark.gpu


def _setup(B, N, disc_dropout=0.0, use_graphs=False, seedG=41, seedD=42):
    from oracle import train_ref as T
    from mpgan_amd import train
    G, D = train.default_mpgan(N, disc_dropout=disc_dropout)
    G.load_state_dict(T.init_state_dict(T.mpgan_param_shapes(True), seedG, torch.float32))
    D.load_state_dict(T.init_state_dict(T.mpgan_param_shapes(False), seedD, torch.float32))
    return G, D


def test_state_dict_manifest_matches_reference():
    import json, os
    from conftest import GOLDEN
    G, D = _setup(4, 30)
    with open(os.path.join(GOLDEN, "manifests.json")) as f:
        m = json.load(f)
    assert {k: list(v.shape) for k, v in G.state_dict().items()} == m["mpgan_G"]
    assert {k: list(v.shape) for k, v in D.state_dict().items()} == m["mpgan_D"]


def test_nets_forward_vs_reference_golden():
    from oracle import train_ref as T
    g = load_golden("mpgan_nets_f32.npz")
    G, D = _setup(6, 30, seedG=11, seedD=12)
    G.eval(); D.eval()
    dev = "cuda"
    gout = G(torch.from_numpy(g["noise"]).to(dev), torch.from_numpy(g["labels"]).to(dev))
    dout = D(torch.from_numpy(g["data"]).to(dev), torch.from_numpy(g["labels"]).to(dev))
    assert rel_err(gout.detach().cpu().numpy(), g["gout"]) < 1e-4
    assert rel_err(dout.detach().cpu().numpy(), g["dout"]) < 1e-4


def test_train_step_vs_reference_golden():
    """Two iterations, dropout 0, the reference's learning rates: losses, first-iteration gradients
    and parameter UPDATES match what the reference modules + torch RMSprop produced (fp64 golden)."""
    from mpgan_amd import train
    g = load_golden("train_step_mpgan.npz")
    B, N = g["data"].shape[:2]
    G, D = _setup(B, N)
    init = {("G", k): v.detach().clone() for k, v in G.state_dict().items()}
    init.update({("D", k): v.detach().clone() for k, v in D.state_dict().items()})
    ts = train.TrainStep(G, D, B, N, lr_disc=float(g["lr_d"]), lr_gen=float(g["lr_g"]), use_graphs=False)
    ts.set_batch(torch.from_numpy(g["data"]).float().cuda(), torch.from_numpy(g["labels"]).float().cuda())
    ts.fixed_noise = (torch.from_numpy(g["noise_D"]).float().cuda(), torch.from_numpy(g["noise_G"]).float().cuda())
    for it in range(2):
        ts._seg_D()
        if it == 0:
            for k, p in D.named_parameters():
                assert summary_err(k, p.grad, g["gradD__" + k]) < 1e-3, k
        ts._seg_G()
        if it == 0:
            for k, p in G.named_parameters():
                assert summary_err(k, p.grad, g["gradG__" + k]) < 1e-3, k
        ts._seg_end()
        assert abs(float(ts.D_loss) - float(g[f"D_loss{it}"])) < 1e-4 * abs(float(g[f"D_loss{it}"]))
        assert abs(float(ts.G_loss) - float(g[f"G_loss{it}"])) < 1e-4 * abs(float(g[f"G_loss{it}"]))
    # parameter values after both iterations (summaries: sum, l2, 64 samples) ...
    for net, mod in (("D", D), ("G", G)):
        for k, p in mod.named_parameters():
            assert rel_err(summarize(k, p.data), g[f"post{net}__" + k]) < 1e-4, (net, k)
    # ... and the UPDATES themselves (post - initial on the sum and the 64 samples; the l2 entry is not linear):
    # a value check at 1e-4 of max|w| would let a 10 % error of a ~1e-4 step through
    # yardstick for the updates: the oracle's own two iterations in plain fp32 (the reference's arithmetic)
    from oracle import train_ref as T
    sdD = T.init_state_dict(T.mpgan_param_shapes(False), 42, torch.float32)
    sdG = T.init_state_dict(T.mpgan_param_shapes(True), 41, torch.float32)
    stD, stG = {}, {}
    f32 = lambda a: torch.from_numpy(np.asarray(a)).float()
    for it in range(2):
        T.train_iteration("mpgan", sdD, sdG, stD, stG, f32(g["data"]), f32(g["labels"]), f32(g["noise_D"]), f32(g["noise_G"]),
                          float(g["lr_d"]), float(g["lr_g"]))
    _assert_updates_match(init, {"D": dict(D.named_parameters()), "G": dict(G.named_parameters())}, g, control={"D": sdD, "G": sdG})


def _count_update_outliers(init, nets, g, tol, k_excl=100.0):
    """(entries beyond ``tol``, entries compared, entries excluded) over the 64 sampled entries of every tensor.  An entry
    is EXCLUDED when the reference's own first-iteration gradient there (the golden's ``grad{net}__*`` summary holds the
    same sampled positions) is within ``k_excl * tol`` of zero relative to the tensor's largest sampled gradient."""
    n_bad = n_all = n_excl = 0
    worst = (0.0, None)
    for net, params in nets.items():
        for k, p in params.items():
            d_ours = (summarize(k, p.data) - summarize(k, init[(net, k)]))[2:66]
            d_ref = (g[f"post{net}__" + k] - summarize(k, init[(net, k)]))[2:66]
            # (the golden's initial values are the same tensors: init_state_dict is a function of name and seed;
            # fp32 rounding of the initial weights enters both differences alike)
            g1 = np.abs(g[f"grad{net}__" + k][2:66])
            keep = g1 > k_excl * tol * g1.max()
            scale = np.abs(d_ref).max()
            err = np.abs(d_ours - d_ref) / scale
            bad = (err > tol) & keep
            n_bad += int(bad.sum()); n_all += int(keep.sum()); n_excl += int((~keep).sum())
            if keep.any() and err[keep].max() > worst[0]:
                worst = (float(err[keep].max()), (net, k))
    return n_bad, n_all, n_excl, worst


def _assert_updates_match(init, nets, g, control, tol=1e-3):
    """Parameter UPDATES of two iterations against the reference's (fp64 golden), sampled entries, at the north-star
    1e-3 of the largest update of each tensor.  Two RMSprop steps move an entry by
        -10 lr [ sign(g1) + r / sqrt(0.99 + r^2) ],   r = g2 / |g1|
    (first step: +-lr / sqrt(1 - alpha) whatever the gradient's size).  Where g1 is within rounding of zero its SIGN decides a
    full-size step, and a gradient error of e (relative to the tensor's largest gradient) moves the second term by about
    kappa * e of the largest update with  kappa = 0.2 / (|g1| / max|g1|)  -- the map's condition number, in ANY finite
    arithmetic.  The entries compared are the well-conditioned ones, kappa <= 2: reference gradient at least 0.1 of the
    tensor's largest (taken out EXPLICITLY otherwise; about half of the sample stays).  There the update error is at most
    kappa times the gradient error, so with the gradient bar at 1e-3 the bar for the updates is 2e-3, and NO entry may be
    beyond it -- for the HIP path and, as a check of the instrument itself, for the oracle's own two iterations in plain
    fp32 (``control``).  Measured on the MPGAN golden (8 jets, where the kernels' gradient errors are largest: <= 5.9e-4
    against 1.4 - 3.6e-4 for plain fp32): worst compared entry HIP 1.3e-3, fp32 4.5e-4.  The counts beyond 1e-3 with smaller
    exclusion zones are printed: they follow kappa (zone 0.03: HIP 5 / fp32 0 of 2,351; zone 0.01: 9 / 2 of 2,798)."""
    bar = 2.0 * tol   # kappa <= 2 in the compared zone
    n_bad, n_all, n_excl, worst = _count_update_outliers(init, nets, g, bar, 100.0 * tol / bar)
    c_bad, _, _, c_worst = _count_update_outliers(init, {n: {k: v for k, v in control[n].items() if k in nets[n]} for n in nets}, g,
                                                  bar, 100.0 * tol / bar)
    for kx in (10.0, 30.0):   # informational: the same count with smaller exclusion zones
        print("  exclusion", kx, "* tol: HIP", _count_update_outliers(init, nets, g, tol, kx)[:2], "fp32",
              _count_update_outliers(init, {n: {k: v for k, v in control[n].items() if k in nets[n]} for n in nets}, g, tol, kx)[:2])
    print("update entries beyond", bar, ": HIP", n_bad, "(worst %.2e at %s)" % worst, "fp32 oracle", c_bad,
          "(worst %.2e at %s)" % c_worst, "of", n_all, "compared,", n_excl, "excluded (near-zero reference gradient)")
    assert n_all > 0.4 * (n_all + n_excl), (n_excl, n_all)   # (half of the sampled entries are well-conditioned)
    assert c_bad == 0, (c_bad, c_worst)
    assert n_bad == 0, (n_bad, worst)


def test_graph_replay_equals_eager():
    """Dropout off: kernels and RMSprop are deterministic, so three hipGraph replays must give
    bit-identical parameters to three eager iterations.  Dropout on: replays stay finite and
    every replay draws new masks (the seed lives in device memory)."""
    from mpgan_amd import train, ops
    from oracle.train_ref import synthetic_batch
    B, N = 16, 30
    data, labels = synthetic_batch(B, N, seed=3)
    res = []
    for use_graphs in (False, True):
        G, D = _setup(B, N, disc_dropout=0.0)
        ts = train.TrainStep(G, D, B, N, use_graphs=use_graphs)
        ts.set_batch(data.cuda(), labels.cuda())
        gen = torch.Generator(device="cuda").manual_seed(5)
        ts.fixed_noise = (torch.randn(B, N, 32, device="cuda", generator=gen) * 0.2,
                          torch.randn(B, N, 32, device="cuda", generator=gen) * 0.2)
        if use_graphs:
            ts.capture(warmup=0)
        for _ in range(3):
            ts.step()
        torch.cuda.synchronize()
        res.append((ts.fD.flat.clone(), ts.fG.flat.clone(), float(ts.D_loss), float(ts.G_loss)))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert res[0][2] == res[1][2] and res[0][3] == res[1][3]

    G, D = _setup(B, N, disc_dropout=0.5)
    ts = train.TrainStep(G, D, B, N, use_graphs=True)
    ts.set_batch(data.cuda(), labels.cuda())
    losses = []
    for _ in range(4):
        ts.step()
        losses.append(float(ts.D_loss))
    assert all(np.isfinite(l) for l in losses)
    assert len(set(losses)) == 4  # fresh noise and fresh dropout masks on every replay


def _three_steps(B, N, use_graphs, split=False, pg=None, model="mpgan", disc_dropout=0.0, steps=3, seed=3, n_graphs=None,
                 gen_join=None):
    """Parameters after `steps` iterations from fixed weights / data / noise."""
    import os
    from mpgan_amd import train
    from oracle import train_ref as T
    from oracle.train_ref import synthetic_batch
    if model == "mpgan":
        G, D = _setup(B, N, disc_dropout=disc_dropout)
        latent, lrs = 32, train.LR["g"]
    else:
        G, D = train.default_gapt(N, disc_dropout=disc_dropout)
        G.load_state_dict(T.init_state_dict(T.gapt_param_shapes(True), 41, torch.float32))
        D.load_state_dict(T.init_state_dict(T.gapt_param_shapes(False), 42, torch.float32))
        latent, lrs = 64, train.LR_GAPT
    data, labels = synthetic_batch(B, N, seed=seed)
    if split:
        os.environ["MPG_SPLIT_GRAPHS"] = "1"
    try:
        ts = train.TrainStep(G, D, B, N, latent=latent, lr_disc=lrs[0], lr_gen=lrs[1], use_graphs=use_graphs,
                             process_group=pg)
        ts.set_batch(data.cuda(), labels.cuda())
        gen = torch.Generator(device="cuda").manual_seed(5)
        ts.fixed_noise = (torch.randn(B, N, latent, device="cuda", generator=gen) * 0.2,
                          torch.randn(B, N, latent, device="cuda", generator=gen) * 0.2)
        if use_graphs:
            ts.capture(warmup=0)
            assert len(ts._graphs) == (n_graphs if n_graphs is not None else (3 if (split or pg is not None) else 1))
        for _ in range(steps):
            ts.step()
        torch.cuda.synchronize()
        if gen_join is not None and ts.gen_ahead:    # where the generator-ahead branch joined (TrainStep.gen_join)
            assert ts.gen_join == gen_join, (ts.gen_join, gen_join)
    finally:
        os.environ.pop("MPG_SPLIT_GRAPHS", None)
    return ts.fD.flat.clone(), ts.fG.flat.clone(), float(ts.D_loss), float(ts.G_loss)


def test_three_segment_graphs_equal_eager():
    """The multi-rank shape of the iteration -- three hipGraphs with the gradient exchange between them -- replayed
    without a process group (MPG_SPLIT_GRAPHS): bit-identical to eager execution."""
    a = _three_steps(16, 30, use_graphs=False)
    b = _three_steps(16, 30, use_graphs=True, split=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2:] == b[2:]


def test_train_step_n150_shard():
    """BASELINE config 5's per-GPU shard (N = 150, B = 16): five receiver blocks per jet, sender chunks > 1.
    Graph replay == eager bit for bit (dropout off), losses finite with dropout on."""
    a = _three_steps(16, 150, use_graphs=False, steps=2)
    b = _three_steps(16, 150, use_graphs=True, steps=2)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2:] == b[2:]
    c = _three_steps(16, 150, use_graphs=True, disc_dropout=0.5, steps=2)
    assert all(np.isfinite(v) for v in c[2:]) and bool(torch.isfinite(c[0]).all()) and bool(torch.isfinite(c[1]).all())


def test_train_step_n150_vs_oracle():
    """Parameter motion at N = 150 against the oracle's iteration (B = 2: what the CPU restatement can afford)."""
    from oracle import train_ref as T
    from oracle.train_ref import synthetic_batch
    from mpgan_amd import train
    B, N = 2, 150
    G, D = _setup(B, N)
    sdG = T.init_state_dict(T.mpgan_param_shapes(True), 41, torch.float64)
    sdD = T.init_state_dict(T.mpgan_param_shapes(False), 42, torch.float64)
    # D sums 150 particles before its sigmoid: with unit-scale head weights the logit is ~ +-17, where fp32's
    # 1 - sigmoid is exactly 0 (fp64's is 4e-8) and every gradient vanishes -- an fp32 artefact the reference has
    # too.  Shrink the head so the comparison happens where both arithmetics have a gradient.
    sdD["fnd_layer.net.0.weight"] = sdD["fnd_layer.net.0.weight"] * 0.02
    D.load_state_dict({k: v.float() for k, v in sdD.items()})
    data, labels = synthetic_batch(B, N, seed=11)
    gen = torch.Generator().manual_seed(6)
    nD, nG = torch.randn(B, N, 32, generator=gen) * 0.2, torch.randn(B, N, 32, generator=gen) * 0.2
    # (learning rate 0 for D: RMSprop's first step is ~ -10 lr sign(g) wherever |g| >> 1e-7, so rounding noise on a
    # gradient entry that is zero by symmetry would move D differently here and in the oracle before the G step)
    ts = train.TrainStep(G, D, B, N, use_graphs=False, lr_disc=0.0)
    ts.set_batch(data.cuda(), labels.cuda())
    ts.fixed_noise = (nD.cuda(), nG.cuda())
    ts._seg_D()
    # (labels: float32(n) * float32(1/N) times N truncates to n in fp32 -- the reference's arithmetic -- but for some n
    # falls a hair below n in fp64; the oracle gets the fp32 meaning)
    # control: the same oracle iteration in plain fp32 (the reference's arithmetic) from the same parameters
    c32 = lambda sd: {k: v.float() for k, v in sd.items()}
    _, _, cD, cG = T.train_iteration("mpgan", c32(sdD), c32(sdG), {}, {}, data.float(), labels.float(), nD.float(), nG.float(),
                                     0.0, train.LR["g"][1], return_grads=True)
    dl, gl, gD, gG = T.train_iteration("mpgan", sdD, sdG, {}, {}, data.double(), labels.double() + 1e-7, nD.double(),
                                       nG.double(), 0.0, train.LR["g"][1], return_grads=True)
    # B = 2: every LeakyReLU sign that fp32-level rounding decides differently from fp64 shows at ~1e-2 in these
    # short sums -- for the fp32 control as for the kernels, hence the bar max(1e-3, 3x fp32's own error) per parameter
    _assert_grads(D, gD, 1e-3, control=cD)
    ts._seg_G()
    _assert_grads(G, gG, 1e-3, control=cG)
    ts._seg_end()
    assert abs(float(ts.D_loss) - dl) < 1e-4 * abs(dl) and abs(float(ts.G_loss) - gl) < 1e-4 * abs(gl)


def test_gapt_train_step_n150_vs_oracle():
    """GAPT at --num-hits 150 (setup_training.py:415): one train_D + train_G against the oracle's iteration, B = 3, D dropout off.
    Every attention block -- 4 + 2 SABs of 150 x 150 tokens, D's pooling block 1 x 150 -- runs as ONE launch each way on the
    large-set kernels (asserted: no mpg_gemm / mpg_attn_* launch in the iteration); losses 1e-4, first-iteration gradients of both
    networks 1e-3 with the oracle's own fp32 evaluation as the control."""
    from oracle import train_ref as T
    from oracle.train_ref import synthetic_batch
    from mpgan_amd import train, _lib
    B, N = 3, 150
    G, D = train.default_gapt(N, disc_dropout=0.0)
    sdG = T.init_state_dict(T.gapt_param_shapes(True), 41, torch.float64)
    sdD = T.init_state_dict(T.gapt_param_shapes(False), 42, torch.float64)
    G.load_state_dict({k: v.float() for k, v in sdG.items()})
    D.load_state_dict({k: v.float() for k, v in sdD.items()})
    data, labels = synthetic_batch(B, N, seed=12)
    gen = torch.Generator().manual_seed(7)
    nD, nG = torch.randn(B, N, 64, generator=gen) * 0.2, torch.randn(B, N, 64, generator=gen) * 0.2
    ts = train.TrainStep(G, D, B, N, latent=64, use_graphs=False, lr_disc=0.0, lr_gen=train.LR_GAPT[1])
    ts.set_batch(data.cuda(), labels.cuda())
    ts.fixed_noise = (nD.cuda(), nG.cuda())
    counts = {}
    real = _lib.lib()

    class Spy:
        def __getattr__(self, name):
            f = getattr(real, name)
            if not name.startswith("mpg_"):
                return f
            def g(*a):
                counts[name] = counts.get(name, 0) + 1
                return f(*a)
            return g
    saved, _lib._lib = _lib._lib, Spy()
    try:
        ts._seg_D()
        gradD = {k: p.grad.detach().double().cpu().numpy().copy() for k, p in D.named_parameters()}
        ts._seg_G()
        gradG = {k: p.grad.detach().double().cpu().numpy().copy() for k, p in G.named_parameters()}
        ts._seg_end()
    finally:
        _lib._lib = saved
    torch.cuda.synchronize()
    print(counts)
    assert counts.get("mpg_mab_fwd", 0) + 2 * counts.get("mpg_mab_chain_fwd", 0) >= 7 and counts.get("mpg_mab_bwd", 0) >= 7, counts
    assert not any(k in counts for k in ("mpg_gemm", "mpg_attn_fwd", "mpg_attn_bwd", "mpg_gate")), counts
    c32 = lambda sd: {k: v.float() for k, v in sd.items()}
    c64 = lambda sd: {k: v.clone() for k, v in sd.items()}
    _, _, cD, cG = T.train_iteration("gapt", c32(sdD), c32(sdG), {}, {}, data.float(), labels.float(), nD.float(), nG.float(),
                                     0.0, train.LR_GAPT[1], return_grads=True)
    dl, gl, gD, gG = T.train_iteration("gapt", c64(sdD), c64(sdG), {}, {}, data.double(), labels.double(), nD.double(),
                                       nG.double(), 0.0, train.LR_GAPT[1], return_grads=True)
    num = lambda d: {k: v.detach().double().numpy() for k, v in d.items()}
    assert abs(float(ts.D_loss) - dl) < 1e-4 * abs(dl) and abs(float(ts.G_loss) - gl) < 1e-4 * abs(gl)
    assert_grads(gradD, num(gD), 1e-3, control=num(cD), what=("gapt", N, "D"))
    assert_grads(gradG, num(gG), 1e-3, control=num(cG), what=("gapt", N, "G"))


def _assert_grads(module, ref, tol, control=None):
    """conftest.assert_grads on a module's .grad buffers (e.g. the last node-layer bias of D under the w / hinge
    losses has a gradient that vanishes by symmetry: real and generated jets have the same multiplicities and opposite
    loss gradients)."""
    assert_grads({k: p.grad.double().cpu().numpy() for k, p in module.named_parameters()},
                 {k: v.detach().numpy() for k, v in ref.items()}, tol,
                 control=None if control is None else {k: v.detach().double().numpy() for k, v in control.items()})


@pytest.mark.parametrize("loss,B,head", [("og", 8, None), ("w", 8, None), ("hinge", 8, None), ("hinge", 64, (10.0, 0.28))],
                         ids=["og", "w", "hinge", "hinge-B64-inactive-jets"])
def test_train_step_other_losses_vs_oracle(loss, B, head):
    """--loss og / w / hinge (train.py:331-395, :465-476): losses and first-iteration gradients vs the oracle.
    ``head`` = (s, shift): D's last Linear scaled and shifted (out -> s * (out - shift)) so that its outputs straddle the
    hinge margins -- at B = 64 with (10, 0.28) the oracle finds 14 real and 3 generated jets beyond them (asserted below,
    with the smallest distance to a margin): whole jets whose upstream gradient is EXACTLY zero ride in the same launches
    as active ones, through the fused head, the data-gradient kernels' per-workgroup gradient units and the
    weight-gradient kernel's launch-wide unit."""
    from oracle import train_ref as T
    from oracle.train_ref import synthetic_batch
    from mpgan_amd import train
    N = 30
    G, D = train.default_mpgan(N, disc_dropout=0.0, loss=loss)
    sdG = T.init_state_dict(T.mpgan_param_shapes(True), 41, torch.float64)
    sdD = T.init_state_dict(T.mpgan_param_shapes(False), 42, torch.float64)
    if head is not None:
        s_, shift = head
        sdD["fnd_layer.net.0.bias"] = sdD["fnd_layer.net.0.bias"] * s_ - s_ * shift
        sdD["fnd_layer.net.0.weight"] = sdD["fnd_layer.net.0.weight"] * s_
    G.load_state_dict({k: v.float() for k, v in sdG.items()})
    D.load_state_dict({k: v.float() for k, v in sdD.items()})
    data, labels = synthetic_batch(B, N, seed=12)
    gen = torch.Generator().manual_seed(7)
    nD, nG = torch.randn(B, N, 32, generator=gen) * 0.2, torch.randn(B, N, 32, generator=gen) * 0.2
    # (lr_disc = 0, see test_train_step_n150_vs_oracle: under w / hinge the last node-layer bias of D has a gradient
    # that vanishes by symmetry, and RMSprop would turn its rounding noise into a full-size step)
    ts = train.TrainStep(G, D, B, N, use_graphs=False, loss=loss, lr_disc=0.0)
    ts.set_batch(data.cuda(), labels.cuda())
    ts.fixed_noise = (nD.cuda(), nG.cuda())
    cfg = {"D": {"sigmoid": loss not in ("w", "hinge")}}
    if head is not None:
        with torch.no_grad():
            fake = T._fwd_G("mpgan", sdG, nD.double(), labels.double(), N, cfg)
            o_r = T._fwd_D("mpgan", sdD, data.double(), labels.double(), 0.0, None, cfg)
            o_f = T._fwd_D("mpgan", sdD, fake, labels.double(), 0.0, None, cfg)
        n_r, n_f = int(((1 - o_r) <= 0).sum()), int(((1 + o_f) <= 0).sum())
        margin = float(torch.minimum((1 - o_r).abs().min(), (1 + o_f).abs().min()))
        print("hinge-inactive jets: real", n_r, "generated", n_f, "of", B, "each; closest to a margin", margin)
        assert n_r >= 4 and n_f >= 2 and n_r < B and margin > 1e-2
    ts._seg_D()
    c32 = lambda sd: {k: v.float() for k, v in sd.items()}
    _, _, cD, cG = T.train_iteration("mpgan", c32(sdD), c32(sdG), {}, {}, data.float(), labels.float(), nD.float(), nG.float(),
                                     0.0, train.LR["g"][1], return_grads=True, loss=loss, cfg=cfg)
    dl, gl, gD, gG = T.train_iteration("mpgan", sdD, sdG, {}, {}, data.double(), labels.double(), nD.double(),
                                       nG.double(), 0.0, train.LR["g"][1], return_grads=True, loss=loss, cfg=cfg)
    _assert_grads(D, gD, 1e-3, control=cD)   # (1e-3, or 3x what the fp32 oracle itself shows against fp64 here)
    ts._seg_G()
    _assert_grads(G, gG, 1e-3, control=cG)
    ts._seg_end()
    assert abs(float(ts.D_loss) - dl) < 1e-4 * max(abs(dl), 1e-3) and abs(float(ts.G_loss) - gl) < 1e-4 * max(abs(gl), 1e-3)


def test_train_step_top_jet_settings_vs_oracle():
    """BASELINE config 3's settings on one rank's shard shapes (``--jets t``: lr_disc 6e-5, lr_gen 2e-5, setup_training.py:852-866;
    top jets nearly fill the 30 slots -- ``data.synthetic_jets(dist="top")``), B = 32: one whole iteration with BOTH optimizers
    stepping at those rates -- losses, D's and G's first-iteration gradients against the oracle (G's behind D's real update), and the
    size of the steps themselves (RMSprop's first step is 10 lr per entry whatever the gradient)."""
    from oracle import train_ref as T
    from mpgan_amd import train
    from mpgan_amd.data import synthetic_jets
    B, N = 32, 30
    lr_d, lr_g = train.LR["t"]
    assert (lr_d, lr_g) == (6e-5, 2e-5)
    G, D = train.default_mpgan(N, disc_dropout=0.0)
    sdG = T.init_state_dict(T.mpgan_param_shapes(True), 41, torch.float64)
    sdD = T.init_state_dict(T.mpgan_param_shapes(False), 42, torch.float64)
    G.load_state_dict({k: v.float() for k, v in sdG.items()})
    D.load_state_dict({k: v.float() for k, v in sdD.items()})
    w0 = {"D": D.state_dict()["mp_layers.1.fe.net.2.weight"].clone(), "G": G.state_dict()["mp_layers.1.fe.net.2.weight"].clone()}
    data, labels = synthetic_jets(B, N, seed=31, dist="top")
    assert float((data[..., 3] > 0).float().mean()) > 0.9          # (top jets: nearly every slot holds a particle)
    gen = torch.Generator().manual_seed(17)
    nD, nG = torch.randn(B, N, 32, generator=gen) * 0.2, torch.randn(B, N, 32, generator=gen) * 0.2
    ts = train.TrainStep(G, D, B, N, use_graphs=False, lr_disc=lr_d, lr_gen=lr_g)
    ts.set_batch(data.cuda(), labels.cuda())
    ts.fixed_noise = (nD.cuda(), nG.cuda())
    ts._seg_D()
    gradD = {k: p.grad.detach().double().cpu().numpy().copy() for k, p in D.named_parameters()}
    ts._seg_G()
    gradG = {k: p.grad.detach().double().cpu().numpy().copy() for k, p in G.named_parameters()}
    ts._seg_end()
    torch.cuda.synchronize()
    c32 = lambda sd: {k: v.float() for k, v in sd.items()}
    c64 = lambda sd: {k: v.clone() for k, v in sd.items()}
    _, _, cD, cG = T.train_iteration("mpgan", c32(sdD), c32(sdG), {}, {}, data.float(), labels.float(), nD.float(), nG.float(),
                                     lr_d, lr_g, return_grads=True)
    dl, gl, gD, gG = T.train_iteration("mpgan", c64(sdD), c64(sdG), {}, {}, data.double(), labels.double(), nD.double(), nG.double(),
                                       lr_d, lr_g, return_grads=True)
    num = lambda d: {k: v.detach().double().numpy() for k, v in d.items()}
    assert abs(float(ts.D_loss) - dl) < 1e-4 * abs(dl) and abs(float(ts.G_loss) - gl) < 1e-4 * abs(gl)
    assert_grads(gradD, num(gD), 1e-3, control=num(cD), what=("top", B, "D"))
    assert_grads(gradG, num(gG), 1e-3, control=num(cG), what=("top", B, "G"))
    for net, mod, lr in (("D", D, lr_d), ("G", G, lr_g)):
        step = (mod.state_dict()["mp_layers.1.fe.net.2.weight"] - w0[net]).abs()
        # (lr g / (sqrt(0.01 g^2) + 1e-8): 10 lr from below, by the few per cent the epsilon takes where the gradients are ~1e-6)
        assert 0.9 * 10.0 * lr < float(step.max()) <= 10.0 * lr * (1 + 1e-3), (net, float(step.max()), lr)


@pytest.mark.parametrize("opt", ["rmsprop", "adam", "adadelta"])
def test_fused_optimizers_vs_torch(opt):
    """mpg_rmsprop / mpg_adam / mpg_adadelta against torch.optim on the same gradients, five steps, incl. gscale."""
    from mpgan_amd.train import FlatParams
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(40, 30), torch.nn.Linear(30, 7)).cuda()
    ref = torch.nn.Sequential(torch.nn.Linear(40, 30), torch.nn.Linear(30, 7)).cuda().double()
    ref.load_state_dict({k: v.double() for k, v in net.state_dict().items()})
    cls = {"rmsprop": torch.optim.RMSprop, "adam": torch.optim.Adam, "adadelta": torch.optim.Adadelta}[opt]
    kw = {"weight_decay": 5e-4, "betas": (0.5, 0.9)} if opt == "adam" else {}
    lr = {"rmsprop": 1e-3, "adam": 1e-3, "adadelta": 1.0}[opt]
    to = cls(ref.parameters(), lr=lr, **kw)
    fp = FlatParams(net, opt, betas=(0.5, 0.9))
    for it in range(5):
        grads = [torch.randn_like(p) for p in net.parameters()]
        for p, q, gr in zip(net.parameters(), ref.parameters(), grads):
            p.grad.copy_(2.0 * gr)          # "summed over 2 ranks"
            q.grad = gr.double()
        fp.step(lr, gscale=0.5, zero_grad=it % 2 == 1)
        assert (float(fp.grad.abs().max()) == 0.0) == (it % 2 == 1)   # cleared behind its last use, only when asked
        to.step()
    for p, q in zip(net.parameters(), ref.parameters()):
        assert rel_err(p.detach().cpu().numpy(), q.detach().cpu().numpy()) < 1e-5
    sd, tsd = fp.state_dict(), to.state_dict()
    for i, ent in tsd["state"].items():
        for k, v in ent.items():
            assert rel_err(sd["state"][i][k].float().cpu().numpy(), torch.as_tensor(v).float().cpu().numpy()) < 1e-4, (i, k)


def test_generation_path_no_grad_vs_reference_golden():
    """Inference (reference gen.py / gen_multi_batch): the generator under ``no_grad`` -- no sign words, nothing saved
    for a backward -- in chunks, against the reference's own output; then the un-normalising epilogue."""
    from mpgan_amd import gen as mgen
    from mpgan_amd.data import unnormalise_jets, FEATURE_MAXES
    g = load_golden("mpgan_nets_f32.npz")
    G, _ = _setup(6, 30, seedG=11, seedD=12)
    G.eval()
    noise, labels = torch.from_numpy(g["noise"]).cuda(), torch.from_numpy(g["labels"])
    n = noise.shape[0]
    margs = {"lfc": False, "latent_node_size": 32}
    with torch.no_grad():
        whole = mgen.gen(margs, G, n, 30, noise=noise, labels=labels)
    assert not whole.requires_grad and rel_err(whole.cpu().numpy(), g["gout"]) < 1e-4
    # chunked, ragged last chunk, CPU gather (noise passed per call would repeat: exercise labels slicing with
    # generated noise only for shape / determinism of the mask column)
    out = mgen.gen_multi_batch(margs, G, 4, n, 30, out_device="cpu", detach=True, labels=labels)
    assert out.shape == (n, 30, 4) and out.device.type == "cpu" and not out.requires_grad
    n_real = (labels[:, 0] * 30).int()
    assert torch.equal((out[..., 3] > 0).sum(1).int(), n_real)             # mask_c: exactly n particles per jet
    # chunk == whole when the noise is the same
    parts = torch.cat([mgen.gen(margs, G, min(4, n - s), 30, noise=noise[s:s + 4], labels=labels[s:s + 4]).detach()
                       for s in range(0, n, 4)])
    assert rel_err(parts.cpu().numpy(), g["gout"]) < 1e-4
    jets = unnormalise_jets(whole, "g")
    ref = g["gout"][..., :3].astype(np.float64).copy()
    ref[..., 2] += 0.5
    ref *= np.array(FEATURE_MAXES["g"][:3])
    ref[g["gout"][..., 3] < 0.5 - 1e-6] = 0     # mask column is +-0.5: "mask >= 0.5" == real particle
    ref[..., 2] = np.maximum(ref[..., 2], 0)
    assert jets.shape == (n, 30, 3) and rel_err(jets.cpu().numpy(), ref) < 1e-4
    full = mgen.generate_jets(G, 1000, 30, labels=torch.full((1000, 1), 20 / 30.0), batch_size=512)
    assert full.shape == (1000, 30, 3) and bool(torch.isfinite(full).all())
    assert int((full.abs().sum(-1) > 0).sum(1).max()) <= 20


@pytest.mark.parametrize("which", ["three scalars per edge: un-fused", "two scalars per edge: fused"])
def test_discriminator_with_conditioning_options_vs_reference_golden(which):
    """A whole MPDiscriminator with the conditioning options on, output and gradients against the reference's own: with
    clabels, mask_fne_np, mask_fnd_np and delta-r edge features (three scalars per edge: the un-fused route of every layer and
    of the head), and with delta-r + clabels (two: every layer on the fused edge kernels)."""
    import numpy as np
    import gen_golden
    from oracle import train_ref as T
    from mpgan_amd.mpgan import MPDiscriminator
    fused = which.endswith("fused") and not which.endswith("un-fused")
    D_OPT = gen_golden.D_OPT2 if fused else gen_golden.D_OPT
    g = load_golden("mpdisc_opt2_f64.npz" if fused else "mpdisc_opt_f64.npz")
    D = MPDiscriminator(**D_OPT).cuda().eval()
    assert all(l.fused for l in D.mp_layers) == fused and any(l.fused for l in D.mp_layers) == fused
    shapes = {k: tuple(v.shape) for k, v in D.state_dict().items()}
    D.load_state_dict(T.init_state_dict(shapes, seed=int(g["seed"]), dtype=torch.float32))
    x = torch.from_numpy(g["x"]).float().cuda().requires_grad_(True)
    y = D(x, torch.from_numpy(g["labels"]).float().cuda())
    (y * torch.from_numpy(g["g"]).float().cuda()).sum().backward()
    assert rel_err(y.detach().cpu().numpy(), g["y"]) < 1e-4
    if fused:   # the fused layers take the mask as data (nothing upstream of it is ever trained: the generator's mask column
        # comes out of a ranking): no gradient for the mask column, the particle features' against the reference's
        assert rel_err(x.grad[..., :3].cpu().numpy(), g["dx"][..., :3]) < 1e-3
        assert float(x.grad[..., 3].abs().max()) == 0.0
    else:
        assert rel_err(x.grad.cpu().numpy(), g["dx"]) < 1e-3   # (the mask column included: it feeds the masked sums and njp)
    for k, p in D.named_parameters():
        assert summary_err(k, p.grad, g["grad__" + k]) < 1e-3, k


def _run_steps(opt, n_steps, tmp, save_at=None, resume_from=None, precaptured=False):
    """TrainStep with hipGraphs on fixed noise (dropout off).  ``save_at``: write the reference's checkpoint files after
    that many steps.  ``resume_from``: start from FRESH modules + a fresh TrainStep and load that epoch's files before
    stepping (``precaptured``: the TrainStep has already captured its graphs -- and run a step on other weights -- when
    the checkpoint is loaded into it)."""
    from mpgan_amd import train, checkpoint as ck
    from oracle.train_ref import synthetic_batch
    B, N = 16, 30
    data, labels = synthetic_batch(B, N, seed=21)
    if resume_from is None:
        G, D = _setup(B, N)
    else:
        G, D = _setup(B, N, seedG=77, seedD=78)          # other weights: everything must come from the files
    ts = train.TrainStep(G, D, B, N, use_graphs=True, optimizer=opt, betas=(0.5, 0.9))
    ts.set_batch(data.cuda(), labels.cuda())
    gen = torch.Generator(device="cuda").manual_seed(8)
    ts.fixed_noise = (torch.randn(B, N, 32, device="cuda", generator=gen) * 0.2,
                      torch.randn(B, N, 32, device="cuda", generator=gen) * 0.2)
    if resume_from is not None:
        if precaptured:
            ts.capture(warmup=0)
            ts.step()
        ck.load_models(D, G, tmp, resume_from)
        ck.load_optimizers(ts.fD, ts.fG, tmp, resume_from)
    for it in range(n_steps):
        ts.step()
        if save_at is not None and it + 1 == save_at:
            torch.cuda.synchronize()
            ck.save_models(D, G, ts.fD, ts.fG, tmp, save_at)
    torch.cuda.synchronize()
    return ts.fD.flat.clone(), ts.fG.flat.clone(), ts.fD.sq.clone(), ts.fG.sq.clone(), ts.fD.steps, float(ts.D_loss), float(ts.G_loss)


@pytest.mark.parametrize("opt", ["rmsprop", "adam"])
def test_resume_from_checkpoint_equals_uninterrupted_run(opt, tmp_path):
    """setup_training.py:1134-1179, :1406-1416, :1525-1535 + train.py:526-537: four iterations in one go against two
    iterations, ``save_models``, fresh modules and a fresh TrainStep (hipGraphs on), ``load_models`` +
    ``load_optimizers``, two more -- bit-identical parameters, optimiser moments, step counters and losses.  Adam's step
    counter lives in device memory and the captured graphs hold buffer addresses: also with the checkpoint loaded into
    a TrainStep that has ALREADY captured its graphs."""
    tmp = str(tmp_path / "models")
    whole = _run_steps(opt, 4, tmp, save_at=2)
    import os
    assert sorted(os.listdir(tmp)) == ["D_2.pt", "D_optim_2.pt", "G_2.pt", "G_optim_2.pt"]
    sd = torch.load(os.path.join(tmp, "D_optim_2.pt"), weights_only=False)
    cls = {"rmsprop": torch.optim.RMSprop, "adam": torch.optim.Adam}[opt]
    probe = cls([torch.zeros(tuple(v.shape)) for v in torch.load(os.path.join(tmp, "D_2.pt")).values()], lr=1.0)
    probe.load_state_dict(sd)                            # the reference's own optimizer class reads the file
    for variant in (False, True):
        again = _run_steps(opt, 2, tmp, resume_from=2, precaptured=variant)
        for a, b in zip(whole[:4], again[:4]):
            assert torch.equal(a, b), (opt, variant)
        assert whole[4:] == again[4:], (opt, variant, whole[4:], again[4:])


def test_matmul_fn_is_twice_differentiable():
    """ops.MatMulFn (the product of the double-backward route): values, first and second derivatives of a scalar built
    from all three forms against torch's own matmul in fp64."""
    from mpgan_amd import ops
    torch.manual_seed(3)
    A = torch.randn(37, 20, device="cuda", requires_grad=True)
    Bm = torch.randn(11, 20, device="cuda", requires_grad=True)
    Cm = torch.randn(11, 5, device="cuda", requires_grad=True)

    def f(mm, a, b, c):
        y = mm(a, b, "nt")                 # [37, 11]
        z = mm(torch.tanh(y), c, "nn")     # [37, 5]
        w = mm(z, torch.sin(a), "tn")      # [5, 20]
        return (w ** 2).sum()

    ref_mm = lambda x, y, form: x @ y.t() if form == "nt" else (x @ y if form == "nn" else x.t() @ y)
    a64, b64, c64 = (t.detach().double().cpu().requires_grad_(True) for t in (A, Bm, Cm))
    v, r = f(ops.MatMulFn.apply, A, Bm, Cm), f(ref_mm, a64, b64, c64)
    assert abs(float(v) - float(r)) < 1e-4 * abs(float(r))
    g = torch.autograd.grad(v, (A, Bm, Cm), create_graph=True)
    g64 = torch.autograd.grad(r, (a64, b64, c64), create_graph=True)
    for x, y in zip(g, g64):
        assert rel_err(x.detach().cpu().numpy(), y.detach().numpy()) < 1e-4
    s, s64 = sum((x ** 2).sum() for x in g), sum((y ** 2).sum() for y in g64)
    h = torch.autograd.grad(s, (A, Bm, Cm))
    h64 = torch.autograd.grad(s64, (a64, b64, c64))
    for x, y in zip(h, h64):
        assert rel_err(x.cpu().numpy(), y.numpy()) < 1e-4


@pytest.mark.parametrize("loss", ["w", "ls"])
def test_gradient_penalty_step_vs_reference_golden(loss):
    """--gp (train.py:286-324, calc_D_loss :331-395): the D step's loss, penalty and gradients -- with the penalty's
    second-order terms, back-propagated through the double-backward route of the discriminator -- against what the
    reference's own functions produced (tests/gen_golden.py executes them from its source).  The fused route still
    declines a second derivative."""
    from oracle import train_ref as T
    from mpgan_amd import train, ops
    g = load_golden(f"gp_step_mpgan_{loss}.npz")
    B, N = g["data"].shape[:2]
    G, D = train.default_mpgan(N, disc_dropout=0.0, loss=loss)
    G.load_state_dict(T.init_state_dict(T.mpgan_param_shapes(True), 41, torch.float32))
    D.load_state_dict(T.init_state_dict(T.mpgan_param_shapes(False), 42, torch.float32))
    ts = train.TrainStep(G, D, B, N, use_graphs=False, loss=loss, gp_lambda=float(g["gp_lambda"]), lr_disc=0.0)
    ts.set_batch(torch.from_numpy(g["data"]).float().cuda(), torch.from_numpy(g["labels"]).float().cuda())
    nD = torch.from_numpy(g["noise_D"]).float().cuda()
    ts.fixed_noise = (nD, nD)
    ts.fixed_alpha = torch.from_numpy(g["alpha"]).float().cuda()
    ts._seg_D()
    torch.cuda.synchronize()
    assert abs(float(ts.GP) - float(g["gp"])) < 1e-3 * abs(float(g["gp"]))
    assert abs(float(ts.D_loss) - (float(g["Dr"]) + float(g["Df"]))) < 1e-4 * max(abs(float(g["Dr"]) + float(g["Df"])), 1e-3)
    assert abs(float(ts.D_loss) + float(ts.GP) - float(g["D_loss"])) < 1e-3 * abs(float(g["D_loss"]))
    for k, p in D.named_parameters():
        assert summary_err(k, p.grad, g["gradD__" + k]) < 1e-3, k
    # the fused kernels are first order: asking them for a second derivative fails loudly
    x = torch.from_numpy(g["data"]).float().cuda().requires_grad_(True)
    out = D(x)
    (gx,) = torch.autograd.grad(out.sum(), x, create_graph=True)
    with pytest.raises(RuntimeError):
        (gx ** 2).sum().backward()


@pytest.mark.parametrize("loss", ["ls", "w"])
def test_gradient_penalty_step_gapt_vs_reference_golden(loss):
    """--gp with the attention discriminator (train.py:301 calls D(interpolated) on whatever D is): loss, penalty and
    gradients against the reference's own gradient_penalty / calc_D_loss executed on its GAPT_D (tests/gen_golden.py).
    One jet of the golden batch attends to nothing (its two endpoints share no real particle): zero attention weights,
    as torch gives it.  Every MAB takes its double-backward form there; D(real) / D(generated) stay on the one-launch blocks."""
    from oracle import train_ref as T
    from mpgan_amd import train, ops
    g = load_golden(f"gp_step_gapt_{loss}.npz")
    B, N = g["data"].shape[:2]
    G, D = train.default_gapt(N, disc_dropout=0.0)
    G.load_state_dict(T.init_state_dict(T.gapt_param_shapes(True), 41, torch.float32))
    D.load_state_dict(T.init_state_dict(T.gapt_param_shapes(False), 42, torch.float32))
    ts = train.TrainStep(G, D, B, N, latent=64, use_graphs=False, loss=loss, gp_lambda=float(g["gp_lambda"]), lr_disc=0.0)
    ts.set_batch(torch.from_numpy(g["data"]).float().cuda(), torch.from_numpy(g["labels"]).float().cuda())
    nD = torch.from_numpy(g["noise_D"]).float().cuda()
    ts.fixed_noise = (nD, nD)
    ts.fixed_alpha = torch.from_numpy(g["alpha"]).float().cuda()
    ts._seg_D()
    torch.cuda.synchronize()
    assert abs(float(ts.GP) - float(g["gp"])) < 1e-3 * abs(float(g["gp"]))
    assert abs(float(ts.D_loss) - (float(g["Dr"]) + float(g["Df"]))) < 1e-4 * max(abs(float(g["Dr"]) + float(g["Df"])), 1e-3)
    assert abs(float(ts.D_loss) + float(ts.GP) - float(g["D_loss"])) < 1e-3 * abs(float(g["D_loss"]))
    for k, p in D.named_parameters():
        assert bool(torch.isfinite(p.grad).all()), k
        assert summary_err(k, p.grad, g["gradD__" + k]) < 1e-3, k
    # the one-launch block is first order: a second derivative through it fails loudly
    x = torch.from_numpy(g["data"]).float().cuda().requires_grad_(True)
    (gx,) = torch.autograd.grad(D(x).sum(), x, create_graph=True)
    with pytest.raises(RuntimeError):
        (gx ** 2).sum().backward()


@pytest.mark.parametrize("model", ["mpgan", "gapt"])
def test_gradient_penalty_under_graphs_equals_eager(model):
    """The --gp iteration (double-backward route inside train_D) captured into hipGraphs replays bit-identically to eager
    execution (dropout off, fixed noise and interpolation weights)."""
    from oracle.train_ref import synthetic_batch
    from mpgan_amd import train
    B, N = 8, 30
    data, labels = synthetic_batch(B, N, seed=13)
    res = []
    lat = 32 if model == "mpgan" else 64
    for use_graphs in (False, True):
        from oracle import train_ref as T
        if model == "mpgan":
            G, D = train.default_mpgan(N, disc_dropout=0.0, loss="w")
            shapes = T.mpgan_param_shapes
        else:
            G, D = train.default_gapt(N, disc_dropout=0.0)
            shapes = T.gapt_param_shapes
        G.load_state_dict(T.init_state_dict(shapes(True), 41, torch.float32))
        D.load_state_dict(T.init_state_dict(shapes(False), 42, torch.float32))
        ts = train.TrainStep(G, D, B, N, latent=lat, use_graphs=use_graphs, loss="w", gp_lambda=10.0)
        ts.set_batch(data.cuda(), labels.cuda())
        gen = torch.Generator(device="cuda").manual_seed(2)
        ts.fixed_noise = (torch.randn(B, N, lat, device="cuda", generator=gen) * 0.2,
                          torch.randn(B, N, lat, device="cuda", generator=gen) * 0.2)
        ts.fixed_alpha = torch.rand(B, 1, 1, device="cuda", generator=gen)
        for _ in range(2):
            ts.step()
        torch.cuda.synchronize()
        res.append((ts.fD.flat.clone(), ts.fG.flat.clone(), float(ts.D_loss), float(ts.GP), float(ts.G_loss)))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]) and res[0][2:] == res[1][2:]
    assert res[0][3] > 0


def test_saturated_generator_vs_oracle():
    """The published generators sit deep in tanh's saturation (|pre-activation| of many outputs well beyond 5), the one
    regime where the forward's power-of-two operand scales could run out of fp16 range.  A seeded synthetic stand-in --
    the deterministic initialisation scaled up until at least 20 % of the real particles' outputs have
    |pre-tanh| > 5 -- through the HIP path against the fp64 oracle.  (The published weights themselves stay with the
    reference: tests/test_oracle_golden.py checks the oracle on them.)"""
    import oracle
    from oracle import train_ref as T
    from mpgan_amd import train
    B, N = 32, 30
    data, labels = T.synthetic_batch(B, N, seed=17)
    noise = torch.from_numpy(np.random.RandomState(23).normal(0, 0.2, size=(B, N, 32)))
    real = (data[..., 3] > 0).numpy()
    for scale in (1.0, 1.5, 2.0, 2.5, 3.0, 4.0, 5.0, 6.0, 8.0):
        sd64 = T.init_state_dict(T.mpgan_param_shapes(True), 41, torch.float64, scale=scale)
        with torch.no_grad():
            ref = oracle.mpgen_forward(sd64, noise, labels.double(), num_particles=N)
        frac = float((np.abs(ref[..., :3].numpy()) > np.tanh(5.0))[real].mean())
        if frac >= 0.2:
            break
    assert frac >= 0.2, frac
    G, _ = train.default_mpgan(N)
    G.load_state_dict({k: v.float() for k, v in sd64.items()})
    G.eval()
    with torch.no_grad():
        out = G(noise.float().cuda(), labels.cuda())
    print(f"weights x{scale}: {frac:.0%} of the real outputs beyond |pre-tanh| = 5; max |out - ref| / max |ref| = "
          f"{rel_err(out.cpu().numpy(), ref.numpy()):.1e}")
    assert bool(torch.isfinite(out).all())
    assert rel_err(out.cpu().numpy(), ref.numpy()) < 1e-4


def test_range_guard_reports_overflowing_weight_images():
    """The packed weight images are fp16 with power-of-two operand scales: a weight beyond 65504 / scale turns into inf there
    and every product with it is lost.  mpg_pack_many notes that in a device word; TrainStep.check_range raises."""
    from mpgan_amd import ops, train
    dev = torch.device("cuda:0")
    ops.range_status(dev, clear=True)
    G, D = train.default_mpgan(30, device=dev)
    ts = train.TrainStep(G, D, 4, 30, use_graphs=False)
    from mpgan_amd.data import synthetic_jets
    data, labels = synthetic_jets(4, 30)
    ts.set_batch(data.to(dev), labels.to(dev))
    ts.step()
    ts.check_range()                      # a healthy step: nothing to report
    assert ops.range_status(dev) == 0
    with torch.no_grad():
        D.mp_layers[0].fe.net[1].weight[3, 5] = 2.0e4      # times the operand scale 16 x dropout scale 2: beyond fp16
    ts.step()
    assert ops.range_status(dev) & 1
    with pytest.raises(FloatingPointError):
        ts.check_range()
    with torch.no_grad():
        D.mp_layers[0].fe.net[1].weight[3, 5] = float("nan")
    ops.range_status(dev, clear=True)
    ts.step()
    assert ops.range_status(dev, clear=True) & 2


def _norm_run(use_graphs, steps, gen_ahead_env=None, **norms):
    """Parameters, power-iteration vectors and running statistics after ``steps`` iterations of a TrainStep whose networks
    carry spectral / batch norm (the un-fused route of every layer), from fixed weights, data and noise."""
    import os
    from mpgan_amd import train
    from oracle.train_ref import synthetic_batch
    B, N = 8, 30
    torch.manual_seed(11)
    G, D = train.default_mpgan(N, disc_dropout=0.0, **norms)
    data, labels = synthetic_batch(B, N, seed=5)
    if gen_ahead_env is not None:
        os.environ["MPG_GEN_AHEAD"] = gen_ahead_env
    try:
        ts = train.TrainStep(G, D, B, N, use_graphs=use_graphs, lr_disc=1e-3, lr_gen=1e-3)
    finally:
        os.environ.pop("MPG_GEN_AHEAD", None)
    ts.set_batch(data.cuda(), labels.cuda())
    gen = torch.Generator(device="cuda").manual_seed(6)
    ts.fixed_noise = (torch.randn(B, N, 32, device="cuda", generator=gen) * 0.2,
                      torch.randn(B, N, 32, device="cuda", generator=gen) * 0.2)
    for _ in range(steps):
        ts.step()
    torch.cuda.synchronize()
    state = {"flatD": ts.fD.flat.clone(), "flatG": ts.fG.flat.clone()}
    for name, net in (("G", G), ("D", D)):
        for k, v in net.state_dict().items():
            if k.endswith(("weight_u", "weight_v", "running_mean", "running_var", "num_batches_tracked")):
                state[f"{name}.{k}"] = v.clone()
    return state, ts


@pytest.mark.parametrize("norms", [dict(spectral_norm_disc=True, spectral_norm_gen=True),
                                   dict(batch_norm_gen=True, spectral_norm_disc=True)], ids=["sn-both", "bnG-snD"])
def test_forward_time_state_under_graphs_equals_eager(norms):
    """Spectral norm's power iteration and batch norm's running statistics are state a FORWARD writes.  Under hipGraph replay
    they must keep accumulating at the modules' own addresses exactly as in eager execution (the reference's
    spectral_normalization.py:29-39 carries u / v from step to step): parameters, u / v and the running statistics after
    three captured-and-replayed iterations are bit-identical to three eager ones, capturing (with its warm-up iterations)
    leaves them where they were, and the generator-ahead stream stays off for such a generator (its forked forward would
    write that state beside the D step's own generator call)."""
    eager, ts_e = _norm_run(False, 3, **norms)
    graphs, ts_g = _norm_run(True, 3, **norms)
    assert not ts_e.gen_ahead and not ts_g.gen_ahead
    assert any(k.endswith("weight_u") for k in eager)
    for k in eager:
        assert torch.equal(eager[k], graphs[k]), k
    one, _ = _norm_run(True, 1, **norms)
    moved = [k for k in eager if k.endswith(("weight_u", "running_mean")) and not torch.equal(one[k], graphs[k])]
    assert moved, "the forward-time state did not advance between replays"


@pytest.mark.parametrize("use_graphs,split", [(True, False), (True, True), (False, False)])
def test_generator_ahead_stream_changes_no_result(use_graphs, split):
    """TrainStep launches the G step's generator forward beside the D step on a second stream (it reads nothing the D step
    writes).  Same weights, data and noise with and without it (MPG_GEN_AHEAD=0): parameters after three iterations are
    bit-identical -- captured right after construction (the weight images the two generator calls share are built on the
    first iteration), as one graph, as three segments and eagerly.  (Dropout off: its masks are a function of the order in
    which the fused ops are issued, which is what changes.)"""
    import os
    with_it = _three_steps(64, 30, use_graphs, split=split)
    os.environ["MPG_GEN_AHEAD"] = "0"
    try:
        without = _three_steps(64, 30, use_graphs, split=split)
    finally:
        os.environ.pop("MPG_GEN_AHEAD", None)
    assert torch.equal(with_it[0], without[0]) and torch.equal(with_it[1], without[1]) and with_it[2:] == without[2:]


@pytest.mark.parametrize("use_graphs,split", [(True, False), (True, True), (False, False)])
@pytest.mark.parametrize("B", [64, 16])
def test_weight_gradient_side_stream_changes_no_result(use_graphs, split, B):
    """The launches that only produce weight gradients (mpg_edge_dw + reduction, the grouped node-network products) run on
    a second stream, forked per layer behind mpg_edge_bwd and joined before the optimizer step (and before the all-reduce in
    the three-segment form).  Same launches in the same order per parameter: parameters after three iterations are
    bit-identical to the run without it (MPG_WGRAD_SIDE=0) -- as one graph, as three segments and eagerly, with the
    generator-ahead stream on in both."""
    import os
    with_it = _three_steps(B, 30, use_graphs, split=split)
    os.environ["MPG_WGRAD_SIDE"] = "0"
    try:
        without = _three_steps(B, 30, use_graphs, split=split)
    finally:
        os.environ.pop("MPG_WGRAD_SIDE", None)
    assert torch.equal(with_it[0], without[0]) and torch.equal(with_it[1], without[1]) and with_it[2:] == without[2:]


@pytest.mark.parametrize("use_graphs,split,N,B", [(True, False, 30, 64), (True, True, 30, 64), (False, False, 30, 16), (True, False, 150, 4)])
def test_tail_arrangements_change_no_result(use_graphs, split, N, B):
    """Round 5's two changes around the weight-gradient tails -- the generator-ahead branch forked behind the D step's last
    data-gradient launch (``MPG_GEN_AHEAD_LATE``) and ``mpg_edge_dw``'s reduction inside the layer's grouped split-K reduction launch
    (``ops.OPTIONS['dw_reduce_grouped']``: ``mpg_splitk_reduce_group_dw``) -- are arrangements of the same launches and sums: parameters
    after three iterations are bit-identical with either of them off, as one graph, as three segments, eagerly, and at 150 particles
    (sender chunks)."""
    import os
    from mpgan_amd import ops
    ref = _three_steps(B, N, use_graphs, split=split)
    os.environ["MPG_GEN_AHEAD_LATE"] = "0"
    try:
        early = _three_steps(B, N, use_graphs, split=split)
    finally:
        os.environ.pop("MPG_GEN_AHEAD_LATE", None)
    saved = ops.OPTIONS["dw_reduce_grouped"]
    ops.OPTIONS["dw_reduce_grouped"] = False
    try:
        own = _three_steps(B, N, use_graphs, split=split)
    finally:
        ops.OPTIONS["dw_reduce_grouped"] = saved
    for r in (early, own):
        assert torch.equal(ref[0], r[0]) and torch.equal(ref[1], r[1]) and ref[2:] == r[2:]


@pytest.mark.parametrize("model", ["mpgan", "gapt"])
def test_features_and_mask_held_apart_change_no_result(model):
    """TrainStep hands the generator's particle features and mask to the discriminator APART (``generate_parts`` /
    ``features_parts``: no mask column glued on, split off again and padded back in the gradient).  Same weights, data and
    noise with the reference's [B, N, 4] tensors between the networks (MPG_PARTS=0): parameters after three iterations are
    bit-identical, under hipGraphs."""
    import os
    os.environ["MPG_BRIDGE"] = "0"   # (GAPT: the one-launch bridge between the networks has its own arithmetic and its own test)
    try:
        with_it = _three_steps(64, 30, True, model=model)
        os.environ["MPG_PARTS"] = "0"
        without = _three_steps(64, 30, True, model=model)
    finally:
        os.environ.pop("MPG_PARTS", None)
        os.environ.pop("MPG_BRIDGE", None)
    assert torch.equal(with_it[0], without[0]) and torch.equal(with_it[1], without[1]) and with_it[2:] == without[2:]


@pytest.mark.parametrize("cfg", ["mpgan", "mpgan_bn", "gapt", "gapt_ln", "gapt_ln_blocks"])
def test_train_G_leaves_the_discriminators_gradient_buffer_clean(cfg):
    """``TrainStep`` has no ``zero_grad`` launch at the top of train_D: D's flat gradient buffer is cleared by D's optimizer launch and
    must stay clear through train_G (where D's parameters are frozen: train.py:494-521 forms their gradients and throws them away).
    Checked for the default networks, a batch-norm discriminator and layer-norm attention blocks on both of their routes."""
    from mpgan_amd import train
    from mpgan_amd.gapt import GAPT_G, GAPT_D, MAB
    from oracle.train_ref import synthetic_batch
    B, N = 16, 30
    fused = True
    if cfg.startswith("mpgan"):
        G, D = train.default_mpgan(N, disc_dropout=0.0, batch_norm_disc=(cfg == "mpgan_bn"))
        latent, lrs = 32, train.LR["g"]
    elif cfg == "gapt":
        G, D = train.default_gapt(N, disc_dropout=0.0)
        latent, lrs = 64, train.LR_GAPT
    else:
        lin = {"leaky_relu_alpha": 0.2, "dropout_p": 0.0, "batch_norm": False, "spectral_norm": False}
        common = {"num_particles": N, "num_heads": 4, "embed_dim": 64, "sab_fc_layers": [], "use_mask": True, "use_isab": False,
                  "num_isab_nodes": 10, "final_fc_layers": [], "dropout_p": 0.0, "layer_norm": True, "linear_args": lin}
        G = GAPT_G(sab_layers=2, output_feat_size=3, **common).cuda()
        D = GAPT_D(sab_layers=2, input_feat_size=3, **common).cuda()
        latent, lrs = 64, train.LR_GAPT
        fused = cfg == "gapt_ln"
    MAB.fused = fused
    try:
        ts = train.TrainStep(G, D, B, N, latent=latent, lr_disc=lrs[0], lr_gen=lrs[1], use_graphs=False)
        data, labels = synthetic_batch(B, N, seed=2)
        ts.set_batch(data.cuda(), labels.cuda())
        for _ in range(2):
            ts._seg_D()
            assert float(ts.fD.grad.abs().max()) > 0
            ts._seg_G()
            assert float(ts.fD.grad.abs().max()) == 0.0, cfg
            assert float(ts.fG.grad.abs().max()) > 0
            ts._seg_end()
            assert float(ts.fG.grad.abs().max()) == 0.0
    finally:
        MAB.fused = True


# ---------------------------------------------------------------------------------------------------------------------
# The headline's own mode: D in training mode with dropout 1/2 in BOTH half-steps (train.py:419-421, :494-495).
def _site_masks(log, n_jets, N, model, dev):
    """Keep masks of one discriminator pass over ``n_jets`` jets, dumped site by site with ``mpg_dropout_mask`` from the
    (kind, tag base, thr) entries ``ops.next_tag`` logged for it (those that carry dropout), as float32 {0, 1} tensors in
    the oracle's ``keeps`` layout."""
    from mpgan_amd import ops
    ent = [e for e in log if e[2] > 0]
    thr = ent[0][2]
    dm = lambda rows, F, tag: ops.dropout_mask(rows, F, tag, thr, dev).cpu()
    if model == "mpgan":
        assert [e[0] for e in ent] == ["mplayer", "mplayer", "head"], log
        widths = {"e0": 96, "e1": 160, "e2": 192, "n0": 256, "n1": 256, "n2": 32}
        sites = {"e0": ops.TAG_E0, "e1": ops.TAG_E1, "e2": ops.TAG_E2, "n0": ops.TAG_N0, "n1": ops.TAG_N1, "n2": ops.TAG_N2}
        layers = []
        for _, tag, _ in ent[:2]:
            k = {}
            for s, wdt in widths.items():
                if s.startswith("e"):
                    k[s] = dm(n_jets * N * N, wdt, tag + sites[s]).reshape(n_jets, N, N, wdt)
                else:
                    k[s] = dm(n_jets * N, wdt, tag + sites[s]).reshape(n_jets, N, wdt)
            layers.append(k)
        return {"layers": layers, "fnd": dm(n_jets, 1, ent[2][1] + ops.TAG_GENERIC).reshape(n_jets, 1)}
    kinds = [e[0] for e in ent]
    assert kinds in (["bridge", "mab", "mab", "mab", "head"], ["linear", "mab", "mab", "mab", "head"]), log
    E = 64
    blk = lambda tag, L: {k: dm(n_jets * L, E, tag + s).reshape(n_jets, L, E) for s, k in enumerate(("a", "f", "o"))}
    return {"emb": dm(n_jets * N, E, ent[0][1] + ops.TAG_GENERIC).reshape(n_jets, N, E),
            "sab0": blk(ent[1][1], N), "sab1": blk(ent[2][1], N), "pma": blk(ent[3][1], 1),
            "fc": dm(n_jets, 1, ent[4][1] + ops.TAG_GENERIC).reshape(n_jets, 1)}


def _slice_keeps(k, lo, hi):
    if isinstance(k, dict):
        return {a: _slice_keeps(v, lo, hi) for a, v in k.items()}
    if isinstance(k, list):
        return [_slice_keeps(v, lo, hi) for v in k]
    return k[lo:hi]


def _oracle_keeps(k, model):
    """(keeps as ``oracle.train_ref._fwd_D`` takes them for ``model``)"""
    if model == "mpgan":
        return dict(enumerate(k["layers"]), fnd=k["fnd"])
    return k


@pytest.mark.parametrize("model,B,p_disc", [("mpgan", 8, 0.5), ("mpgan", 64, 0.5), ("gapt", 8, 0.5), ("gapt", 64, 0.5),
                                            ("mpgan", 256, 0.0)])
def test_train_iteration_with_dropout_vs_oracle(model, B, p_disc):
    """(``("mpgan", 256, 0.0)``: BASELINE config 2's own shapes -- the whole iteration at B = 256, N = 30 against the oracle, dropout
    off: at that size the keep masks of one iteration are 4 GB of floats; the dropout-on cases stop at B = 64.)
    One whole train_D + train_G at ``disc_dropout = 0.5`` -- the bench's configuration: one-bit dropout in both
    message-passing layers / every attention block of D, in its embedding and in its head, the fused epilogues, the
    real + generated pass over 2B jets, the generator -> discriminator bridge -- against the oracle's iteration fed with the
    very keep masks the launches drew (dumped per site; the site tags come from ``ops.next_tag``'s log).  Losses 1e-4,
    first-iteration gradients of both networks 1e-3: GAPT with the oracle's own fp32 evaluation as the kink-flip control,
    MPGAN against the fp64 oracle outright or the sign-conditioned one (see below) -- no allowance for flips at all."""
    from oracle import train_ref as T
    from oracle.train_ref import synthetic_batch
    from mpgan_amd import train, ops
    N = 30
    dev = torch.device("cuda", torch.cuda.current_device())
    if model == "mpgan":
        G, D = train.default_mpgan(N, disc_dropout=p_disc)
        shG, shD, latent, lrs = T.mpgan_param_shapes(True), T.mpgan_param_shapes(False), 32, train.LR["g"]
    else:
        G, D = train.default_gapt(N, disc_dropout=p_disc)
        shG, shD, latent, lrs = T.gapt_param_shapes(True), T.gapt_param_shapes(False), 64, train.LR_GAPT
    sdG = T.init_state_dict(shG, 41, torch.float64)
    sdD = T.init_state_dict(shD, 42, torch.float64)
    G.load_state_dict({k: v.float() for k, v in sdG.items()})
    D.load_state_dict({k: v.float() for k, v in sdD.items()})
    data, labels = synthetic_batch(B, N, seed=21)
    gen = torch.Generator().manual_seed(9)
    nD, nG = torch.randn(B, N, latent, generator=gen) * 0.2, torch.randn(B, N, latent, generator=gen) * 0.2
    # (lr_disc = 0: see test_train_step_n150_vs_oracle -- RMSprop's first step is -10 lr sign(g), and the G step is compared
    # on the SAME discriminator here and in the oracle)
    ts = train.TrainStep(G, D, B, N, latent=latent, use_graphs=False, lr_disc=0.0, lr_gen=lrs[1])
    ts.set_batch(data.cuda(), labels.cuda())
    ts.fixed_noise = (nD.cuda(), nG.cuda())
    ops.set_seed(0x5EED0000 + B)
    st = ops.dev_state(dev)
    import itertools
    st.tags = itertools.count(2502 if B == 8 else 7000 + B)   # (the site tags, hence the masks drawn, independent of what ran before:
                                                            #  at B = 8 a realisation in which the launches DO flip three kinks --
                                                            #  two in D's upper edge network, one in its node network -- that fp64 and
                                                            #  fp32 do not: every D tensor is then 2-5e-3 off the plain oracle and must
                                                            #  meet the bar against the sign-conditioned one)
    st.tag_log, st.sign_tap = [], ([] if model == "mpgan" else None)
    try:
        ts._seg_D()
        log_D, st.tag_log = st.tag_log, []
        gradD = {k: p.grad.detach().double().cpu().numpy().copy() for k, p in D.named_parameters()}
        kD = _site_masks(log_D, 2 * B, N, model, dev) if p_disc else None       # (the seed moves on in _seg_end: dump before)
        ts._seg_G()
        log_G = st.tag_log
        gradG = {k: p.grad.detach().double().cpu().numpy().copy() for k, p in G.named_parameters()}
        kG = _site_masks(log_G, B, N, model, dev) if p_disc else None
        taps = st.sign_tap
    finally:
        st.tag_log = st.sign_tap = None
    ts._seg_end()
    torch.cuda.synchronize()
    if p_disc:
        frac = float(kD["fnd" if model == "mpgan" else "fc"].mean())
        print("tag log D step", log_D, "\nG step", log_G, "; head keep fraction", frac)
        keeps = (_oracle_keeps(_slice_keeps(kD, 0, B), model), _oracle_keeps(_slice_keeps(kD, B, 2 * B), model),
                 _oracle_keeps(kG, model))
    else:
        keeps = None
    big = B >= 256   # (one fp64 iteration of the oracle at this size is a minute of the box's host cores: the fp32 control --
                     #  printed for orientation only on this route -- is skipped, and the sign-conditioned evaluation runs only
                     #  if some tensor is beyond the bar outright)
    c32 = lambda sd: {k: v.float() for k, v in sd.items()}
    cD = cG = None
    if not big:
        _, _, cD, cG = T.train_iteration(model, c32(sdD), c32(sdG), {}, {}, data.float(), labels.float(), nD.float(), nG.float(),
                                         0.0, lrs[1], p_disc=p_disc, keeps=keeps, return_grads=True)
    c64 = lambda sd: {k: v.clone() for k, v in sd.items()}   # (train_iteration steps the parameters it is given IN PLACE)
    dl, gl, gD, gG = T.train_iteration(model, c64(sdD), c64(sdG), {}, {}, data.double(), labels.double(), nD.double(), nG.double(),
                                       0.0, lrs[1], p_disc=p_disc, keeps=keeps, return_grads=True)
    num = lambda d: {k: v.detach().double().numpy() for k, v in d.items()}
    print("losses: HIP", float(ts.D_loss), float(ts.G_loss), "oracle", dl, gl)
    assert abs(float(ts.D_loss) - dl) < 1e-4 * abs(dl) and abs(float(ts.G_loss) - gl) < 1e-4 * abs(gl)
    if model != "mpgan":
        assert_grads(gradD, num(gD), 1e-3, control=num(cD), what=(model, B, "D"))
        assert_grads(gradG, num(gG), 1e-3, control=num(cG), what=(model, B, "G"))
        return
    # MPGAN: LeakyReLU kinks in every layer.  The fp32 control above is printed for orientation only; the bar is 1e-3 per
    # tensor against the fp64 oracle outright or -- strictly, no allowance for flips -- against the SIGN-CONDITIONED fp64
    # oracle: the same iteration with every LeakyReLU branch of every message-passing layer taken as the launches took it
    # (their own sign bits, tapped per fused call: ops.DeviceState.sign_tap, conftest.hip_signs_from).
    from conftest import hip_signs_from, record_parity

    def rel_all(got, ref):
        scale = max(float(np.abs(v).max()) for v in ref.values())
        return {k: float(np.abs(got[k] - ref[k]).max() / max(np.abs(ref[k]).max(), 1e-3 * scale)) for k in ref}
    outright = {"D": rel_all(gradD, num(gD)), "G": rel_all(gradG, num(gG))}
    qD = qG = None
    if not big or any(v > 1e-3 for d in outright.values() for v in d.values()):
        sg = [hip_signs_from(t["ac"], t["stE2"], t["sign3"], t["h1"], t["h2"], t["B"], t["N"]) for t in taps]
        nj = [t["B"] for t in taps]
        d2 = [s_ for s_, n in zip(sg, nj) if n == 2 * B]          # D's two layers over the 2B jets of the D step
        g1 = [s_ for s_, n in zip(sg, nj) if n == B]              # G step: G's two layers, then D's two (host order)
        assert len(d2) == 2 and len(g1) == 4, nj
        cut = lambda d, lo, hi: {k: v[lo:hi] for k, v in d.items()}
        signs = ([cut(d, 0, B) for d in d2], [cut(d, B, 2 * B) for d in d2], g1[:2], g1[2:])
        _, _, qD, qG = T.train_iteration(model, c64(sdD), c64(sdG), {}, {}, data.double(), labels.double(), nD.double(), nG.double(),
                                         0.0, lrs[1], p_disc=p_disc, keeps=keeps, return_grads=True, signs=signs)
    nan = float("nan")
    for net, got, ref, cond, ctl in (("D", gradD, num(gD), qD, cD), ("G", gradG, num(gG), qG, cG)):
        e_cond = rel_all(got, num(cond)) if cond is not None else {k: nan for k in ref}
        e_ctl = rel_all(num(ctl), ref) if ctl is not None else {k: nan for k in ref}
        report = {k: (outright[net][k], e_cond[k], e_ctl[k]) for k in ref}
        print(net, "per tensor (vs fp64, vs sign-conditioned fp64, fp32's own vs fp64):", report)
        bad = {k: v for k, v in report.items() if not (v[0] <= 1e-3 or v[1] <= 1e-3)}
        wk = max(report, key=lambda k: report[k][0] if cond is None else min(report[k][0], report[k][1]))
        record_parity("iteration", (model, B, p_disc, net), tensors=len(report), outright=sum(v[0] <= 1e-3 for v in report.values()),
                      conditioned=sum(v[0] > 1e-3 for v in report.values()) - len(bad), failed=len(bad), worst=wk,
                      err=report[wk][0], err_conditioned=report[wk][1], fp32_err=report[wk][2],
                      max_err=max(v[0] for v in report.values()), max_fp32_err=max(v[2] for v in report.values()))
        assert not bad, (model, B, net, bad)


def test_device_seed_follows_torch_seed_and_travels_with_the_checkpoint():
    """The noise / dropout streams are keyed by the device seed: ``TrainStep`` derives it from ``torch.initial_seed()`` and the
    rank (torch.manual_seed keeps the reference's meaning, setup_training.py:184), an explicit ``ops.set_seed`` is never
    overwritten, and the value rides in G's optimizer state dict so that a resumed run continues the stream."""
    from mpgan_amd import train, ops
    from oracle.train_ref import synthetic_batch
    B, N = 4, 30
    dev = torch.device("cuda", torch.cuda.current_device())
    st = ops.dev_state(dev)
    before = torch.initial_seed()
    try:
        st.seed_is_default, st.auto_seed_key = True, None
        torch.manual_seed(5)
        G, D = _setup(B, N, disc_dropout=0.5)
        ts = train.TrainStep(G, D, B, N, use_graphs=False)
        assert ops.get_seed(dev) == ops.derived_seed(5, 0) and st.seed_is_default
        # a second TrainStep under the same torch seed (a bench's secondary workload, another batch size) does not rewind the stream
        ops.bump_seed(dev)
        train.TrainStep(G, D, B, N, use_graphs=False)
        assert ops.get_seed(dev) == (ops.derived_seed(5, 0) + ops.SEED_STEP) & 0xFFFFFFFFFFFFFFFF
        assert len({ops.derived_seed(s, r) for s in (5, 6) for r in range(8)}) == 16
        torch.manual_seed(6)
        ts = train.TrainStep(G, D, B, N, use_graphs=False)
        assert ops.get_seed(dev) == ops.derived_seed(6, 0)
        ops.set_seed(123, dev)
        ts = train.TrainStep(G, D, B, N, use_graphs=False)
        assert ops.get_seed(dev) == 123                   # the caller's choice stands
        data, labels = synthetic_batch(B, N, seed=2)
        ts.set_batch(data.cuda(), labels.cuda())
        ts.step()
        torch.cuda.synchronize()
        now = ops.get_seed(dev)
        assert now == (123 + ops.SEED_STEP) & 0xFFFFFFFFFFFFFFFF   # one iteration on
        sdD, sdG = ts.optimizer_state_dicts()
        assert sdG["param_groups"][0][train.FlatParams.SEED_KEY] == now and train.FlatParams.SEED_KEY not in sdD["param_groups"][0]
        assert sdG["param_groups"][0][train.FlatParams.SEED_RANK_KEY] == 0
        torch.optim.RMSprop([torch.zeros(tuple(p.shape)) for p in G.parameters()], lr=1.0).load_state_dict(sdG)   # torch reads it
        ops.set_seed(999, dev)
        ts.load_optimizer_state_dicts(sdD, sdG)
        assert ops.get_seed(dev) == now
        # another rank reading the same file gets a stream of its own (tests/test_dist_cpu.py runs it on two ranks)
        ts._seed.rank = 3
        ts.load_optimizer_state_dicts(sdD, sdG)
        assert ops.get_seed(dev) == ops.rerank_seed(now, 0, 3) != now
    finally:
        st.seed_is_default, st.auto_seed_key = True, None
        torch.manual_seed(before)


def test_generator_ahead_branch_joins_where_each_arrangement_says(monkeypatch):
    """Where the generator-ahead branch joins the main stream, without a process group (``TrainStep.gen_join``): at the end of a D
    segment that stands alone -- called directly, or a hipGraph of its own -- and only where the G step takes the jets when both
    segments share an eager iteration or one graph.  The default MPGAN at B = 8, N = 30 without dropout: the smallest shape with
    the branch, its late fork and the weight-gradient stream all live.  Every arrangement, and the step without the branch, ends
    at the same bits after two iterations."""
    from mpgan_amd import train
    from oracle.train_ref import synthetic_batch
    B, N = 8, 30
    data, labels = synthetic_batch(B, N, seed=3)
    gen = torch.Generator(device="cuda").manual_seed(5)
    noise = tuple(torch.randn(B, N, 32, device="cuda", generator=gen) * 0.2 for _ in range(2))

    def run(how, n_graphs=None, env=()):
        with monkeypatch.context() as m:
            for name, value in env:
                m.setenv(name, value)
            G, D = _setup(B, N, disc_dropout=0.0)
            ts = train.TrainStep(G, D, B, N, lr_disc=train.LR["g"][0], lr_gen=train.LR["g"][1], use_graphs=n_graphs is not None)
        ts.set_batch(data.cuda(), labels.cuda())
        ts.fixed_noise = noise
        if n_graphs is not None:
            ts.capture(warmup=0)
            assert len(ts._graphs) == n_graphs
        for _ in range(2):
            if how == "segments":
                ts._seg_D(); ts._seg_G(); ts._seg_end()
            elif how == "eager":
                ts._eager()
            else:
                ts.step()
        torch.cuda.synchronize()
        return ts, (ts.fD.flat.clone(), ts.fG.flat.clone(), ts.D_loss.clone(), ts.G_loss.clone())

    results = []
    for how, n_graphs, env, joined in (("segments", None, (), "seg_D"), ("eager", None, (), "seg_G"), ("graphs", 1, (), "seg_G"),
                                       ("graphs", 3, (("MPG_SPLIT_GRAPHS", "1"),), "seg_D")):
        ts, res = run(how, n_graphs, env)
        assert ts.gen_ahead and ts.gen_ahead_late and ts.wgrad_side, how
        assert ts.gen_join == joined, (how, n_graphs, ts.gen_join)
        results.append(res)
    ts, res = run("eager", env=(("MPG_GEN_AHEAD", "0"),))
    assert ts.gen_ahead is False and ts.gen_join is None
    results.append(res)
    for res in results[1:]:
        assert all(torch.equal(a, b) for a, b in zip(results[0], res))
    assert all(bool(torch.isfinite(t).all()) for t in results[0])


def test_a_backward_that_raises_leaves_no_branch_and_no_weight_gradient_state_open(monkeypatch):
    """A Python exception out of the D step's backward: the late fork of the generator-ahead branch sits behind that backward and
    must not have run -- no side stream, no jets pending, nothing to join -- and the weight-gradient collection is taken down
    (``deferred_wgrad``, ``wgrad_stream``, ``wgrad_keep``).  The step then runs a whole iteration as if nothing had happened."""
    from mpgan_amd import train, ops
    from oracle.train_ref import synthetic_batch
    B, N = 8, 30
    G, D = _setup(B, N, disc_dropout=0.0)
    ts = train.TrainStep(G, D, B, N, use_graphs=False)
    assert ts.gen_ahead and ts.gen_ahead_late and ts.wgrad_side
    data, labels = synthetic_batch(B, N, seed=3)
    ts.set_batch(data.cuda(), labels.cuda())

    def refuse(*args, **kwargs):
        raise RuntimeError("backward refused")
    with monkeypatch.context() as m:
        m.setattr(torch.autograd, "backward", refuse)
        with pytest.raises(RuntimeError, match="backward refused"):
            ts._seg_D()
    assert ts._ahead.jets is None and not ts._ahead.open
    assert ts._ahead.stream is None and ts.gen_join is None        # (the first fork makes the stream: there was none)
    st = ops.dev_state(ts.dev)
    assert st.deferred_wgrad is None and st.wgrad_stream is None and len(st.wgrad_keep) == 0
    ts.mark_grads_dirty()
    ts._eager()
    torch.cuda.synchronize()
    assert ts.gen_join == "seg_G" and ts._ahead.jets is None and not ts._ahead.open
    assert np.isfinite(float(ts.D_loss)) and np.isfinite(float(ts.G_loss))


def test_every_option_at_once_capture_restores_graphs_equal_eager_resume_equals_the_run():
    """The four augmentations at p = 0.5 under ``adaptive_prob`` (interval 2), label noise 0.1, ``num_critic=2``, the epoch's loss
    sums and a ``DeviceJetLoader`` over 16 jets in ONE step, MPGAN defaults at N = 30, B = 4, D's dropout on:
    (i) ``capture`` of both kinds of batch leaves every tensor of ``_training_state``, the seed, ``ada``, ``batch_ndx`` and the
    loader's position where they were; (ii) six captured steps equal six eager ones bit for bit; (iii) the optimizer state dicts and
    the loader's state saved after step 3, loaded into a fresh step over other weights with a fresh loader, give the same six.
    (The dropout sites of an eager step are numbered anew on every step, a graph keeps those of its capture: the counter is put back
    before each eager step and before the captures that are compared with them.)"""
    import itertools
    from mpgan_amd import ops, train
    from mpgan_amd.data import DeviceJetLoader, synthetic_jets
    B, N, dev = 4, 30, torch.device("cuda", torch.cuda.current_device())
    st = ops.dev_state(dev)
    particles, labels = synthetic_jets(16, N, seed=4)

    def build(use_graphs, loader_seed=13, **seeds):
        G, D = _setup(B, N, disc_dropout=0.5, **seeds)
        aug = train.Augment(aug_r90=True, aug_f=True, aug_t=True, aug_s=True, aug_prob=0.5, adaptive_prob=True, ada_interval=2)
        loader = DeviceJetLoader((particles, labels), B, "cuda", seed=loader_seed)
        ts = train.TrainStep(G, D, B, N, use_graphs=use_graphs, augment=aug, label_noise=0.1, num_critic=2, track_epoch_losses=True,
                             loader=loader)
        ops.set_seed(0x5EED, dev)
        return ts

    def result(ts):
        torch.cuda.synchronize()
        return ([t.clone() for t in (ts.fD.flat, ts.fG.flat, ts.fD.sq, ts.fG.sq, ts.D_loss, ts.G_loss)], ts.ada, ops.get_seed(dev),
                ts.batch_ndx, ts.loader.position)

    def eager_step(ts):
        st.tags = itertools.count(1)
        ts.step()

    def same(a, b):
        return all(torch.equal(x, y) for x, y in zip(a[0], b[0])) and a[1:] == b[1:]

    try:
        eager = build(False)
        for _ in range(3):
            eager_step(eager)
        torch.cuda.synchronize()
        clone = lambda sd: {k: v.clone() for k, v in sd.items()}
        saved = (eager.optimizer_state_dicts(), eager.loader.state_dict(), clone(eager.G.state_dict()), clone(eager.D.state_dict()))
        assert eager.last_ran == ("D",) and saved[0][0]["param_groups"][0]["mpgan_amd_ada"]["steps"] == 1    # (mid-interval)
        for _ in range(3):
            eager_step(eager)
        want = result(eager)
        assert want[3] == 6 and want[4] == 6 * B
        # (i), (ii)
        ts = build(True)
        before = ([t.clone() for t in ts._training_state()], result(ts))
        ts.capture(kind="DG")
        ts.capture(kind="D")
        torch.cuda.synchronize()
        after = ts._training_state()
        assert len(after) == len(before[0]) and all(torch.equal(a, b) for a, b in zip(after, before[0]))
        assert same(result(ts), before[1]) and before[1][2] == 0x5EED and before[1][3:] == (0, 0)
        for kind in ("DG", "D"):       # (captured again without a warm-up, from the first dropout site on)
            st.tags = itertools.count(1)
            ts.capture(warmup=0, kind=kind)
        for _ in range(6):
            ts.step()
        assert same(result(ts), want)
        assert eager.epoch_losses(reset=False) == ts.epoch_losses(reset=False)
        # (iii)
        again = build(False, loader_seed=99, seedG=77, seedD=78)
        ops.set_seed(999, dev)
        again.G.load_state_dict(saved[2]); again.D.load_state_dict(saved[3])
        again.loader.load_state_dict(saved[1])
        again.load_optimizer_state_dicts(*saved[0])
        assert again.batch_ndx == 3 and again.loader.position == 3 * B
        for _ in range(3):
            eager_step(again)
        assert same(result(again), want)
    finally:
        st.seed_is_default, st.auto_seed_key = True, None
