#!/usr/bin/env python3
"""Count the device kernels one eager G+D iteration launches, by aten op (which PyTorch glue is left)."""
import sys, os, collections
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from torch.profiler import profile, ProfilerActivity
from mpgan_amd import ops, train
from mpgan_amd.data import synthetic_jets
dev = torch.device("cuda:0")
BATCH = 512 if os.environ.get("OPC_GAPT") else 256
# (OPC_AUG=1: the step with the four augmentations at a fixed probability; OPC_ADA=1: the same with adaptive_prob)
AUG = train.Augment(aug_r90=True, aug_f=True, aug_t=True, aug_s=True, aug_prob=0.5, adaptive_prob=bool(os.environ.get("OPC_ADA"))) \
    if os.environ.get("OPC_AUG") or os.environ.get("OPC_ADA") else None
# (OPC_SN=1: spectral norm in G and D, counted twice -- ops.OPTIONS["sn_fused"] on, then off: the grouped power-iteration launch and
# the fused edge kernels against a launch per wrapped layer and the un-fused route)
SN = bool(os.environ.get("OPC_SN"))
# (OPC_EMA=1: the averaged generator, folded by G's optimizer launch -- the default step's counts, launch for launch)
EMA = train.Ema(kimg=10) if os.environ.get("OPC_EMA") else None
# (OPC_CTL=1: a learning-rate schedule and a gradient clip on both networks -- the default step's library launches plus the two
# mpg_step_control launches, 43 + 2, and its ATen launches unchanged at 87)
CTL = dict(lr_schedule=train.LrSchedule.warmup_decay(100, 5000, 6000, 0.1), grad_clip=train.GradClip(1.0)) if os.environ.get("OPC_CTL") \
    else {}


def count(title):
    torch.manual_seed(0)
    if os.environ.get("OPC_GAPT"):
        G, D = train.default_gapt(30, device=dev)
    else:
        G, D = train.default_mpgan(30, device=dev, spectral_norm_gen=SN, spectral_norm_disc=SN)
    ts = train.TrainStep(G, D, BATCH, 30, latent=64 if os.environ.get("OPC_GAPT") else 32, use_graphs=False, augment=AUG, ema=EMA, **CTL)
    data, labels = synthetic_jets(BATCH, 30, seed=1, dist="gluon")
    ts.set_batch(data.to(dev), labels.to(dev))
    for _ in range(3): ts.step()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        ts.step()
        torch.cuda.synchronize()
    rows = [(e.key, e.count, e.device_time_total) for e in prof.key_averages() if e.device_time_total > 0]
    rows.sort(key=lambda r: -r[2])
    for k, c, t in rows[:60]:
        print(f"{k[:70]:70s} n={c:4d} dev_us={t:9.1f}")
    ours = lambda k: any(s in k for s in ("_kernel", "mpg_")) and "at::" not in k and "aten" not in k
    n_ours = sum(c for k, c, _ in rows if ours(k)); n_other = sum(c for k, c, _ in rows if not ours(k))
    t_ours = sum(t for k, _, t in rows if ours(k)); t_other = sum(t for k, _, t in rows if not ours(k))
    print(f"{title}library kernels: {n_ours} launches, {t_ours:.0f} us;  other (ATen) kernels: {n_other} launches, {t_other:.0f} us")


def count_gp(title, gp_chain, B=None):
    """OPC_GP=1: one eager penalty D step (``loss="w"``, ``gp_lambda=10``, the existing switches gp_rows / gp_attn on) with
    ``gp_chain`` off and on: launches by kind, and -- at B = 16 -- the peak allocation of the step."""
    torch.manual_seed(0)
    gapt = bool(os.environ.get("OPC_GAPT"))
    b = BATCH if B is None else B
    G, D = train.default_gapt(30, device=dev) if gapt else train.default_mpgan(30, device=dev, loss="w")
    ts = train.TrainStep(G, D, b, 30, latent=64 if gapt else 32, use_graphs=False, loss="w", gp_lambda=10.0, gp_rows=True, gp_attn=True,
                         gp_chain=gp_chain)
    data, labels = synthetic_jets(b, 30, seed=1, dist="gluon")
    ts.set_batch(data.to(dev), labels.to(dev))
    for _ in range(2): ts._seg_D()
    torch.cuda.synchronize()
    if B is not None:
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        ts._seg_D()
        torch.cuda.synchronize()
        print(f"{title}peak allocation of one penalty D step at B = {b}: {torch.cuda.max_memory_allocated() - base} bytes")
        return
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        ts._seg_D()
        torch.cuda.synchronize()
    rows = [(e.key, e.count, e.device_time_total) for e in prof.key_averages() if e.device_time_total > 0]
    ours = lambda k: any(s in k for s in ("_kernel", "mpg_")) and "at::" not in k and "aten" not in k
    n_ours = sum(c for k, c, _ in rows if ours(k)); n_other = sum(c for k, c, _ in rows if not ours(k))
    t_ours = sum(t for k, _, t in rows if ours(k)); t_other = sum(t for k, _, t in rows if not ours(k))
    print(f"{title}library kernels: {n_ours} launches, {t_ours:.0f} us;  other (ATen) kernels: {n_other} launches, {t_other:.0f} us")


def count_baseline(title, which, fused):
    """OPC_BASELINE=pointnet | rgan: one eager D step (``loss="ls"``) of the default MP generator against a baseline discriminator of
    ``mpgan_amd.ext_models`` at its default widths, with ``ops.OPTIONS["point_pool"]`` on and off: launches by kind."""
    import types
    from mpgan_amd import ext_models
    torch.manual_seed(0)
    args = types.SimpleNamespace(rgand_sfc=[64, 128, 256, 256, 512], rgand_fc=[128, 64], pointnetd_pointfc=[64, 128, 1024],
                                 pointnetd_fc=[512], num_hits=30, node_feat_size=3, leaky_relu_alpha=0.2, mask=True)
    G, _ = train.default_mpgan(30, device=dev)
    D = (ext_models.PointNetMixD if which == "pointnet" else ext_models.rGAND)(args).to(dev)
    if which == "rgan":    # (rGAND takes the three particle features: the mask column stays outside)
        inner = D.forward
        D.forward = lambda x, labels=None, epoch=None: inner(x[..., :3])
    ops.OPTIONS["point_pool"] = fused
    ts = train.TrainStep(G, D, BATCH, 30, use_graphs=False)
    data, labels = synthetic_jets(BATCH, 30, seed=1, dist="gluon")
    ts.set_batch(data.to(dev), labels.to(dev))
    for _ in range(2): ts._seg_D()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        ts._seg_D()
        torch.cuda.synchronize()
    # (device kernels and copies only: the profiler's rows of the operators and autograd nodes that issued them repeat their time)
    rows = [(e.key, e.count, e.device_time_total) for e in prof.key_averages()
            if e.device_time_total > 0 and e.key.startswith(("void ", "(anonymous namespace)::", "Memcpy", "Memset"))]
    ours = lambda k: "at::native" not in k and not k.startswith(("Memcpy", "Memset"))
    n_ours = sum(c for k, c, _ in rows if ours(k)); n_other = sum(c for k, c, _ in rows if not ours(k))
    t_ours = sum(t for k, _, t in rows if ours(k)); t_other = sum(t for k, _, t in rows if not ours(k))
    if os.environ.get("OPC_ROWS"):
        for k, c, t in sorted(rows, key=lambda r: -r[2]):
            print(f"{k[:90]:90s} n={c:4d} dev_us={t:9.1f}")
    print(f"{title}library kernels: {n_ours} launches, {t_ours:.0f} us;  ATen kernels and copies: {n_other} launches, {t_other:.0f} us")


def count_treegan(title, fused):
    """OPC_BASELINE=treegan: one eager forward + backward of ``ext_models.TreeGANG`` at its default configuration, B = 256, with
    ``ops.OPTIONS["tree_gcn"]`` on and off: launches by kind."""
    from mpgan_amd import ext_models
    torch.manual_seed(0)
    G = ext_models.TreeGANG([96, 64, 64, 64, 64, 3], [2, 2, 2, 2, 2], 10).to(dev)
    noise = torch.randn(BATCH, 1, 96, device=dev) * 0.2
    up = torch.randn(BATCH, 32, 3, device=dev)
    ops.OPTIONS["tree_gcn"] = fused
    go = lambda: (G([noise]) * up).sum().backward()
    for _ in range(2): go()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        go()
        torch.cuda.synchronize()
    rows = [(e.key, e.count, e.device_time_total) for e in prof.key_averages()
            if e.device_time_total > 0 and e.key.startswith(("void ", "(anonymous namespace)::", "Memcpy", "Memset", "Cijk_"))]
    ours = lambda k: k.startswith(("void ", "(anonymous namespace)::")) and "at::native" not in k
    n_ours = sum(c for k, c, _ in rows if ours(k)); n_other = sum(c for k, c, _ in rows if not ours(k))
    t_ours = sum(t for k, _, t in rows if ours(k)); t_other = sum(t for k, _, t in rows if not ours(k))
    if os.environ.get("OPC_ROWS"):
        for k, c, t in sorted(rows, key=lambda r: -r[2]):
            print(f"{k[:90]:90s} n={c:4d} dev_us={t:9.1f}")
    print(f"{title}library kernels: {n_ours} launches, {t_ours:.0f} us;  ATen kernels and copies: {n_other} launches, {t_other:.0f} us")


def count_graphcnn(title, fused):
    """OPC_BASELINE=graphcnn: one eager forward + backward of ``ext_models.GraphCNNGANG`` at the published configuration, B = 256,
    with ``ops.OPTIONS["nnconv"]`` on and off: launches by kind."""
    import types
    from mpgan_amd import ext_models
    torch.manual_seed(0)
    G = ext_models.GraphCNNGANG(types.SimpleNamespace(latent_dim=128, num_hits=30, graphcnng_layers=[32, 24], node_feat_size=3, num_knn=20,
                                                      leaky_relu_alpha=0.2, graphcnng_tanh=False, device=dev)).to(dev)
    noise = torch.randn(BATCH, 128, device=dev) * 0.2
    up = torch.randn(BATCH, 30, 3, device=dev)
    ops.OPTIONS["nnconv"] = fused
    go = lambda: (G(noise) * up).sum().backward()
    for _ in range(2): go()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        go()
        torch.cuda.synchronize()
    rows = [(e.key, e.count, e.device_time_total) for e in prof.key_averages()
            if e.device_time_total > 0 and e.key.startswith(("void ", "(anonymous namespace)::", "Memcpy", "Memset", "Cijk_"))]
    ours = lambda k: k.startswith(("void ", "(anonymous namespace)::")) and "at::native" not in k
    n_ours = sum(c for k, c, _ in rows if ours(k)); n_other = sum(c for k, c, _ in rows if not ours(k))
    t_ours = sum(t for k, _, t in rows if ours(k)); t_other = sum(t for k, _, t in rows if not ours(k))
    if os.environ.get("OPC_ROWS"):
        for k, c, t in sorted(rows, key=lambda r: -r[2]):
            print(f"{k[:90]:90s} n={c:4d} dev_us={t:9.1f}")
    print(f"{title}library kernels: {n_ours} launches, {t_ours:.0f} us;  ATen kernels and copies: {n_other} launches, {t_other:.0f} us")


if os.environ.get("OPC_BASELINE") == "treegan":
    for on in (True, False):
        count_treegan(f"TreeGANG forward + backward, tree_gcn={on}: ", on)
elif os.environ.get("OPC_BASELINE") == "graphcnn":
    for on in (True, False):
        count_graphcnn(f"GraphCNNGANG forward + backward, nnconv={on}: ", on)
elif os.environ.get("OPC_BASELINE"):
    for on in (True, False):
        count_baseline(f"D step, {os.environ['OPC_BASELINE']} discriminator, point_pool={on}: ", os.environ["OPC_BASELINE"], on)
elif os.environ.get("OPC_GP"):
    for on in (False, True):
        count_gp(f"penalty D step, gp_chain={on}: ", on)
        count_gp(f"penalty D step, gp_chain={on}: ", on, B=16)
elif SN:
    for on in (True, False):
        ops.OPTIONS["sn_fused"] = on
        count(f"spectral norm, sn_fused={on}: ")
else:
    count("")
