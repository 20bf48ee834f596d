"""GPU: the adaptive augmentation probability -- ``ops.ada_update`` (``mpg_ada_update``) against the numpy restatement of
tests/test_ada_cpu.py bit for bit, and ``TrainStep(augment=Augment(adaptive_prob=True, ...))``: captured against eager, the
probability after every step against the restatement fed with that step's own outputs, which launches read the old and which the
new probability, the num_critic / num_gen schedule, resume, and the step without the option unchanged.  The reference offers
nothing to compare against (it names ``--adaptive-prob`` and never fills ``augment_p``): the restatement is the specification."""
import numpy as np
import pytest
import torch

from test_ada_cpu import F32, N_REAL, _same, outputs, restate
from test_gpu_augment import P_ALL, _is_ident, _reset_tags
from test_gpu_labels import _seed_at
from test_gpu_schedule import RAN, _all_equal, _device_seed, _state, _step

pytestmark = pytest.mark.gpu

B = 8
# B * ada_interval / (1000 * ada_kimg) = 16 / 128 = 0.125 exactly: p moves visibly and reaches a clamp within a few intervals
ADA = dict(aug_t=True, aug_f=True, adaptive_prob=True, aug_prob=0.25, ada_target=0.5, ada_interval=2, ada_kimg=0.128)


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _words(state, p, r):
    return (torch.tensor(state, dtype=torch.int32, device="cuda"), torch.tensor([p], dtype=torch.float32, device="cuda"),
            torch.tensor([r], dtype=torch.float32, device="cuda"))


def _read(st, p, r):
    torch.cuda.synchronize()
    s = st.tolist()
    return (s[0], s[1]), p.cpu().numpy()[0], r.cpu().numpy()[0]


@pytest.mark.parametrize("n_real", N_REAL)
def test_one_launch_against_the_restatement(n_real):
    """Outputs drawn on the host (fixed seed, values equal to ``mid`` planted, one NaN), more of them than ``n_real`` so that a
    read past the real half would show.  A launch that leaves the interval open, then one that closes it from a state in its last
    step: state as integers, p and r as bit patterns."""
    from mpgan_amd import ops
    mid, target, step = F32(0.5), F32(0.6), F32(0.01)
    o = np.concatenate([outputs(n_real, 31 * n_real), np.full(n_real + 3, 0.9, dtype=np.float32)])
    out = torch.from_numpy(o).cuda()
    for interval, state in ((4, (0, 0)), (4, (n_real // 2, 3)), (1, (0, 0))):
        st, p, r = _words(state, 0.5, 0.0)
        ops.ada_update(out, n_real, mid, target, step, interval, st, p, r)
        got = _read(st, p, r)
        want = restate(o, n_real, mid, target, step, interval, state, F32(0.5), F32(0))
        assert _same(got, want), (interval, state, got, want)
    assert want[0] == (0, 0)


def test_twelve_launches_on_one_state():
    from mpgan_amd import ops
    n, mid, target, step = 257, F32(0.0), F32(0.6), F32(0.03)
    st, p, r = _words((0, 0), 0.05, 0.0)
    want = ((0, 0), F32(0.05), F32(0))
    seen = []
    for k in range(12):
        o = (outputs(n, 7 + k, mid=0.0) + F32(0.12 * (k // 4) - 0.1)).astype(np.float32)
        ops.ada_update(torch.from_numpy(o).cuda(), n, mid, target, step, 4, st, p, r)
        want = restate(o, n, mid, target, step, 4, *want)
        got = _read(st, p, r)
        assert _same(got, want), (k, got, want)
        seen.append(float(got[1]))
    assert want[0] == (0, 0) and len(set(seen)) >= 3 and seen[0] == seen[2] != seen[3]


def test_argument_checks():
    from mpgan_amd import ops
    out = torch.zeros(8, device="cuda")
    st, p, r = _words((0, 0), 0.5, 0.0)
    ok = dict(out=out, n_real=8, mid=0.5, target=0.6, step=0.01, interval=2, state=st, aug_p=p, r_out=r)
    for bad in (dict(n_real=9), dict(n_real=0), dict(interval=0), dict(target=1.5), dict(target=-0.5), dict(step=-0.01),
                dict(step=float("nan")), dict(state=st.float()), dict(state=torch.zeros(3, dtype=torch.int32, device="cuda")),
                dict(aug_p=torch.zeros(2, device="cuda")), dict(r_out=torch.zeros(1)), dict(aug_p=p.double()),
                dict(out=torch.zeros(8, 2, device="cuda")[:, 0])):
        with pytest.raises(ValueError):
            ops.ada_update(**dict(ok, **bad))
    torch.cuda.synchronize()
    assert st.tolist() == [0, 0] and float(p) == 0.5          # (nothing was launched)


# ---- the step -------------------------------------------------------------------------------------------------------------------
def _ada_step(augment=None, **kw):
    """MPGAN, N = 30, B = 8, dropout 0.5 in D, translation and flip, fresh generator noise every step."""
    from mpgan_amd import train
    kw.setdefault("fixed", False)
    return _step("mpgan", B, disc_dropout=0.5, augment=train.Augment(**(ADA if augment is None else augment)), **kw)


def _mid(ts):
    return F32(ts._ada.mid)


def _follow(ts, steps, want):
    """``steps`` steps; after each the step's words against the restatement applied to its own ``out`` (kept by the test hook)."""
    a = ts._ada
    ps = []
    for k in range(steps):
        ts.step()
        torch.cuda.synchronize()
        if "D" in ts.last_ran:
            o = ts.ada_last_out.detach().reshape(-1).cpu().numpy()
            assert o.shape == (2 * B,)
            want = restate(o, B, _mid(ts), F32(a.target), F32(a.step), a.interval, *want)
        got = ts.ada
        assert got == {"p": float(want[1]), "r": float(want[2]), "sign_sum": want[0][0], "steps": want[0][1]}, (k, got, want)
        ps.append(got["p"])
    return want, ps


def test_captured_equals_eager_over_seven_steps():
    """The dropout sites of an eager step are numbered anew on every step, a graph keeps those of its capture: the counter is put
    back before each eager step.  Parameters, optimizer state, seed, p, the open interval, r (``_training_state``) and the saved
    maps after every step."""
    res = []
    with _device_seed() as seed:
        for use_graphs in (False, True):
            seed()
            ts = _ada_step(use_graphs=use_graphs)
            assert ts._route() != "module" and any(t is ts.aug_p for t in ts._training_state())
            if use_graphs:
                _reset_tags()
                ts.capture(warmup=0)
            seen = []
            for _ in range(7):
                if not use_graphs:
                    _reset_tags()
                ts.step()
                seen.append(_state(ts) + [q.clone() for q in ts.aug_params[:2]] + [ts.ada_state.clone(), ts.ada_r.clone()])
            res.append((seen, ts.ada))
    for k, (a, c) in enumerate(zip(res[0][0], res[1][0])):
        assert _all_equal(a, c), (k, [i for i, (x, y) in enumerate(zip(a, c)) if not torch.equal(x, y)])
    assert res[0][1] == res[1][1] and res[0][1]["steps"] == 1          # (seven D steps: three intervals and a half)


def test_capture_leaves_p_and_the_open_interval_where_they_were():
    """``capture`` runs three real iterations to warm up and puts the training state back: the controller's words with it."""
    with _device_seed() as seed:
        seed()
        ts = _ada_step()
        ts.set_aug_prob(0.375)
        ts.ada_state.copy_(torch.tensor([3, 1], dtype=torch.int32))
        ts.ada_r.fill_(0.25)
        before = ts.ada
        ts.capture()
        assert ts.ada == before == {"p": 0.375, "r": 0.25, "sign_sum": 3, "steps": 1}
        ts.step()                  # the first replay closes the interval that was open
        after = ts.ada
        assert after["steps"] == 0 and after["sign_sum"] == 0 and after["p"] in (0.25, 0.375, 0.5)


@pytest.mark.parametrize("use_graphs", [False, True], ids=["eager", "captured"])
@pytest.mark.parametrize("loss", ["ls", "w"])
def test_p_after_every_step_is_the_restatement_on_that_steps_own_outputs(loss, use_graphs):
    """``ls`` scores sigmoid outputs against 1 / 0: mid = 0.5; ``w`` has no final activation: mid = 0."""
    with _device_seed() as seed:
        seed()
        ts = _ada_step(loss=loss, use_graphs=use_graphs)
        assert ts._ada.mid == (0.5 if loss == "ls" else 0.0)
        ts.ada_keep_out = True       # (before the capture: the graph's own ``out`` tensor is the one kept)
        _, ps = _follow(ts, 6, ((0, 0), F32(0.25), F32(0)))
    assert ps[0] == 0.25 and ps[1] == ps[2] and ps[3] == ps[4]          # (p moves behind D steps 2, 4, 6 only)


def _bias_head(ts, value):
    """D's last bias set so that every jet scores on one side of ``mid``, whatever the weights say (+-1e4: the sigmoid saturates)."""
    w, b = ts.D.fused_head()[:2]
    assert b is not None
    with torch.no_grad():
        b.fill_(value)


@pytest.mark.parametrize("p0,kimg,bias,p1", [(0.0, 0.064, 1e4, 0.125), (1.0, 0.008, -1e4, 0.0), (P_ALL, 0.008, -1e4, 0.0),
                                             (0.0, 0.016, 1e4, 0.5)],
                         ids=["0_to_0.125", "1_down_to_0", "below_1_down_to_0", "0_up_to_0.5"])
def test_train_g_augments_under_the_new_probability(p0, kimg, bias, p1):
    """ada_interval = 1: the first D step closes an interval, and the bias of D's head puts every real jet that the head's dropout
    keeps on one side (a dropped jet scores sigmoid(0) = mid exactly and counts on neither), so the direction is known: r is plus
    or minus the kept share, against a target of 0 on the way up and 0.6 on the way down.  The D step's own augmentation launch (site D_fake) runs in front of the update and must have
    drawn its maps under the OLD p; train_G's (site G_fake) follows the update in stream order and must have drawn under the NEW
    one.  Both sets of maps are recomputed by ``ops.augment_params`` under the seed the iteration started from.  The reasoning
    that tells the two apart without any recomputation: at p = 0 every jet's map is the identity; just below 1 (``P_ALL``) every
    jet takes the translation, which shows in its map.  From there down to 0 the G_fake maps are identities for all jets -- under
    the old p they would not be -- and D_fake's are not for any.  At p = 1 EXACTLY the reference's ``rand_mix`` takes nothing (its
    quirk, kept by ``mpg_augment``), so the case "from 1.0 down" shows identities at both sites and only the recomputation speaks;
    from 0 to 0.125 and to 0.5 D_fake's are identities and G_fake's are the maps of the new p."""
    from mpgan_amd import ops, train
    with _device_seed() as seed:
        seed()
        _reset_tags()          # (the head's dropout site: the same kept jets whatever ran before)
        ts = _ada_step(dict(ADA, aug_prob=p0, ada_interval=1, ada_kimg=kimg, ada_target=0.0 if bias > 0 else 0.6), use_graphs=False)
        _bias_head(ts, bias)
        ts.ada_keep_out = True
        before = ops.seed_tensor(ts.dev).clone()
        ts.step()
        got = ts.ada
        o = ts.ada_last_out[:B].cpu()
        kept = int((o != 0.5).sum())
        print("outputs of the real half", o.tolist(), "ada", got)
        assert kept >= 1 and bool((o[o != 0.5] == (1.0 if bias > 0 else 0.0)).all())
        assert got["r"] == (kept if bias > 0 else -kept) / B and got["p"] == p1 and got["steps"] == 0
        d_fake, g_fake = (ts.aug_params[train.AUG_SITES[k]].clone() for k in ("D_fake", "G_fake"))
        with _seed_at(before):
            a = ts.aug
            want = {(k, p): ops.augment_params(B, torch.full((1,), p, device="cuda"), a.flags, a.translate_ratio, a.scale_sd,
                                               train.AUG_SITES[k]) for k in ("D_fake", "G_fake") for p in (p0, p1)}
            torch.cuda.synchronize()
    assert torch.equal(d_fake, want["D_fake", p0]) and torch.equal(g_fake, want["G_fake", p1])
    ident = {"D_fake": _is_ident(d_fake.cpu()), "G_fake": _is_ident(g_fake.cpu())}
    for k, p in (("D_fake", p0), ("G_fake", p1)):
        if p in (0.0, 1.0):
            assert bool(ident[k].all()), k
        if p == P_ALL:
            assert not bool(ident[k].any()), k
    if P_ALL in (p0, p1) or 0.5 in (p0, p1):      # (the maps under the other probability are different maps: the comparison above can fail)
        assert not torch.equal(want["G_fake", p0], want["G_fake", p1]) and not torch.equal(want["D_fake", p0], want["D_fake", p1])


@pytest.mark.parametrize("num_critic,num_gen", [(3, 1), (1, 2)])
def test_the_state_counts_d_steps(num_critic, num_gen):
    """num_critic = 3: batches D / D+G / D / D / D+G / D / D -- every batch trains D, the D-only ones included: seven updates.
    num_gen = 2: batches D+G / D+G / G / D+G / G -- a G-only batch leaves the controller's words as they were: three updates."""
    with _device_seed() as seed:
        seed()
        ts = _ada_step(num_critic=num_critic, num_gen=num_gen, use_graphs=False)
        ts.ada_keep_out = True
        ran = RAN[(num_critic, num_gen)]
        want, n_d = ((0, 0), F32(0.25), F32(0)), 0
        for k, r in enumerate(ran):
            before = ts.ada
            want, _ = _follow(ts, 1, want)
            assert ts.last_ran == r
            n_d += "D" in r
            if "D" not in r:
                assert ts.ada == before
            assert ts.ada["steps"] == n_d % 2, (k, r)
    assert n_d == (7 if num_critic == 3 else 3)


def test_resume_at_step_three_equals_the_uninterrupted_run_at_step_seven(tmp_path):
    """Saved behind step 3 -- in the middle of the second interval --, loaded into fresh objects with other weights, four more
    steps: everything of the seven uninterrupted steps, bit for bit.  The controller's words travel in D's optimizer file."""
    from mpgan_amd import checkpoint as ck, train
    tmp = str(tmp_path / "models")
    with _device_seed() as seed:
        seed()
        _reset_tags()              # (both runs capture from the same count of dropout sites)
        ts = _ada_step()
        for b in range(7):
            ts.step()
            if b == 2:
                torch.cuda.synchronize()
                ck.save_models(ts.D, ts.G, ts.fD, ts.fG, tmp, 3)
                saved = ts.ada
        whole = _state(ts, device_counters=False) + [q.clone() for q in ts.aug_params[:2]]
        assert saved["steps"] == 1
        assert ts.optimizer_state_dicts()[0]["param_groups"][0][train.FlatParams.ADA_KEY] == ts.ada
        seed()
        _reset_tags()
        again = _ada_step(seeds=(77, 78))
        ck.load_models(again.D, again.G, tmp, 3)
        ck.load_optimizers(again.fD, again.fG, tmp, 3)
        assert again.ada == saved
        for b in range(3, 7):
            again.step()
        got = _state(again, device_counters=False) + [q.clone() for q in again.aug_params[:2]]
        assert again.ada == ts.ada
    assert _all_equal(whole, got), [i for i, (x, y) in enumerate(zip(whole, got)) if not torch.equal(x, y)]


def test_without_adaptive_prob_the_step_has_no_such_launch(monkeypatch):
    """``adaptive_prob=False`` (and ``True`` with every switch off): no buffers, and ``ops.ada_update`` is never called -- the
    iteration is the parent's, launch for launch.  The project's op counter (tools/opcount.py) is a script around the profiler
    and cannot be called from a test: the launch counts of the default and the fixed-probability step are its output, recorded
    with the change that added this file."""
    from mpgan_amd import ops, train

    def never(*a, **k):
        raise AssertionError("ops.ada_update launched without adaptive_prob")
    monkeypatch.setattr(ops, "ada_update", never)
    res = []
    with _device_seed() as seed:
        for aug in (dict(ADA, adaptive_prob=False), dict(aug_prob=0.25, adaptive_prob=True),
                    dict(aug_t=True, aug_f=True, aug_prob=0.25)):
            seed()
            _reset_tags()
            ts = _ada_step(aug, use_graphs=False, fixed=True)
            ts.step()
            assert ts._ada is None and ts.ada_state is None and ts.ada_r is None and ts.fD.carried == []
            assert train.FlatParams.ADA_KEY not in ts.optimizer_state_dicts()[0]["param_groups"][0]
            res.append(_state(ts))
    assert _all_equal(res[0], res[2]) and len(res[1]) == len(res[0])
