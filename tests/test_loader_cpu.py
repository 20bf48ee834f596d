"""CPU: the keyed shuffle of the device-resident data set -- a numpy restatement written from include/mpgan_amd.h against the
library's host entry point --, the rank slicing of the stream, and the host logic of ``TrainStep(loader=...)`` on toy networks
(``DeviceJetLoader.feed`` goes through ``indices`` and ``index_select`` for CPU tensors)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from test_dist_cpu import ToyG, ToyD, _torch_rmsprop, N, LAT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mpgan_amd.h")

SIZES = (1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 64, 65, 1000)
KEYS = (0, 0x0123456789ABCDEF, 0xFFFFFFFF00000001)
EPOCHS = (0, 1, 2 ** 32 + 1)
U32 = np.uint64(0xFFFFFFFF)


def _tag():
    return int(re.search(r"^#define\s+MPG_SHUFFLE_TAG\s+(0x[0-9A-Fa-f]+)\s*$", open(HEADER).read(), flags=re.M).group(1), 16)


def _word(key, tag, row, grp):
    """The header's hash, on uint64 arrays masked to 32 bits after every step (row: array; the rest scalars)."""
    lo, hi = np.uint64(key & 0xFFFFFFFF), np.uint64(key >> 32)
    x = ((row + lo) & U32) * np.uint64(0x9E3779B1) & U32
    x ^= ((np.uint64((grp + tag * 0x10001) & 0xFFFFFFFF) * np.uint64(0x85EBCA77) & U32) + hi) & U32
    x ^= x >> np.uint64(16); x = x * np.uint64(0x7feb352d) & U32
    x ^= x >> np.uint64(15); x = x * np.uint64(0x846ca68b) & U32
    x ^= x >> np.uint64(16)
    return x


def perm_numpy(key, epoch, n):
    """perm(key, epoch, i, n) for every i < n, restated from the header: balanced Feistel network, four rounds, cycle walking."""
    if n == 1:
        return np.zeros(1, dtype=np.int64)
    tag, k = _tag(), int(n - 1).bit_length()
    h = (k + 1) // 2
    assert 2 ** (2 * h) < 4 * n
    m, hh, ep = np.uint64(2 ** h - 1), np.uint64(h), epoch & 0xFFFFFFFF
    x = np.arange(n, dtype=np.uint64)
    todo = np.ones(n, dtype=bool)
    while todo.any():
        L, R = x[todo] >> hh, x[todo] & m
        for r in range(4):
            L, R = R, L ^ (_word(key, tag + r, R, ep) & m)
        x[todo] = (L << hh) | R
        todo = x >= np.uint64(n)
    return x.astype(np.int64)


def host_rows(key, pos0, count, n):
    from mpgan_amd import _lib
    out = np.full(count, -1, dtype=np.int32)
    assert _lib.lib().mpg_shuffle_index_host(key, pos0, count, n, out.ctypes.data_as(C.c_void_p)) == 0
    return out.astype(np.int64)


_epoch_rows = {}


def epoch_rows(key, epoch, n):
    """One epoch's rows from the host entry point (computed once, shared by the tests below)."""
    k = (key, epoch, n)
    if k not in _epoch_rows:
        _epoch_rows[k] = host_rows(key, epoch * n, n, n)
        _epoch_rows[k].setflags(write=False)
    return _epoch_rows[k]


def test_symbols_and_tag():
    from mpgan_amd import _lib, ops
    lib = _lib.lib()
    assert hasattr(lib, "mpg_shuffle_index_host") and hasattr(lib, "mpg_batch_feed")
    txt = open(HEADER).read()
    for name in ("mpg_shuffle_index_host", "mpg_batch_feed"):
        decl = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", txt, flags=re.M | re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name
    tag = _tag()
    assert tag == ops.SHUFFLE_TAG
    others = [ops.NOISE_TAG, ops.NOISE_TAG + 1] + [ops.AUG_TAG + s for s in range(3)]
    assert all(tag + r >= (1 << 27) + 8 and tag + r not in others for r in range(4))
    # the error returns the header states
    out = np.zeros(4, dtype=np.int32)
    assert lib.mpg_shuffle_index_host(1, 0, 4, 0, out.ctypes.data_as(C.c_void_p)) == -1
    assert lib.mpg_shuffle_index_host(1, 0, 4, 5, None) == -1
    assert lib.mpg_batch_feed(None, None, 5, 30, 1, None, None, 4, 4, None, None, None, None, None, None, None, None) == -1


@pytest.mark.parametrize("n", SIZES)
def test_host_shuffle_equals_the_numpy_restatement_and_is_a_permutation(n):
    for key in KEYS:
        for epoch in EPOCHS:
            got = epoch_rows(key, epoch, n)
            assert np.array_equal(got, perm_numpy(key, epoch, n)), (n, key, epoch)
            assert np.array_equal(np.sort(got), np.arange(n)), (n, key, epoch)
    # only the low 32 bits of the epoch enter
    assert np.array_equal(epoch_rows(KEYS[1], 2 ** 32 + 1, n), epoch_rows(KEYS[1], 1, n))


@pytest.mark.parametrize("n", [n for n in SIZES if n >= 31])
def test_epochs_and_keys_shuffle_differently(n):
    for key in KEYS:
        e0, e1 = epoch_rows(key, 0, n), epoch_rows(key, 1, n)
        assert not np.array_equal(e0, e1)
        assert not np.array_equal(e0, np.arange(n)) and not np.array_equal(e1, np.arange(n))
    assert not np.array_equal(epoch_rows(KEYS[0], 0, n), epoch_rows(KEYS[1], 0, n))
    assert not np.array_equal(epoch_rows(KEYS[1], 0, n), epoch_rows(KEYS[2], 0, n))


def test_stream_is_continuous_across_epochs():
    """Positions are taken modulo n into the epoch's permutation: a window that straddles the boundary is the tail of one
    epoch followed by the head of the next."""
    n, key = 37, KEYS[1]
    got = host_rows(key, 30, 20, n)
    assert np.array_equal(got, np.concatenate([epoch_rows(key, 0, n)[30:], epoch_rows(key, 1, n)[:13]]))


def _arrays(n, seed=2):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, N, 4, generator=g), torch.rand(n, 1, generator=g)


def test_ranks_take_disjoint_slices_of_one_stream():
    from mpgan_amd.data import DeviceJetLoader
    W, B, n, steps = 3, 4, 37, 10
    arrays = _arrays(n)
    ranks = [DeviceJetLoader(arrays, B, "cpu", seed=5, rank=r, world_size=W) for r in range(W)]
    one = DeviceJetLoader(arrays, W * B, "cpu", seed=5)
    assert [l.steps_per_epoch for l in ranks] == [4] * W and one.steps_per_epoch == 4
    assert len({l.key for l in ranks + [one]}) == 1               # the key does not depend on the rank
    for s in range(steps):
        inter = torch.cat([l.indices(s) for l in ranks])
        assert torch.equal(inter, one.indices(s)), s
    whole = torch.cat([one.indices(s) for s in range(steps)]).numpy()
    assert np.array_equal(whole, host_rows(one.key, 0, steps * W * B, n))
    for e in range(3):
        assert np.array_equal(np.sort(whole[e * n:(e + 1) * n]), np.arange(n))
    # default key: from torch's seed, and not the noise / dropout seed derived from it
    from mpgan_amd import ops
    torch.manual_seed(77)
    a = DeviceJetLoader(arrays, B, "cpu")
    torch.manual_seed(78)
    b = DeviceJetLoader(arrays, B, "cpu")
    assert a.key != b.key and a.key == DeviceJetLoader(arrays, B, "cpu", seed=77).key and a.key != ops.derived_seed(77, 0)


def _toy_step(loader, B=4, **kw):
    from mpgan_amd import train
    torch.manual_seed(3)
    G, D = ToyG(), ToyD()
    ts = train.TrainStep(G, D, B, N, latent=LAT, lr_disc=1e-2, lr_gen=2e-2, use_graphs=False, loader=loader, **kw)
    g = torch.Generator().manual_seed(7)
    ts.fixed_noise = (torch.randn(B, N, LAT, generator=g) * 0.2, torch.randn(B, N, LAT, generator=g) * 0.2)
    return ts


def _check_buffers(ts, x, l):
    B = ts.B
    assert torch.equal(ts.data, x) and torch.equal(ts.labels, l)
    assert torch.equal(ts._dcat[:B], x) and torch.equal(ts._x3[:B], x[..., :3])
    assert torch.equal(ts._mask2[:B], x[..., 3:] + 0.5) and torch.equal(ts._ign2[:B], 0.5 - x[..., 3])
    assert torch.equal(ts._labels2[:B], l) and torch.equal(ts._labels2[B:], l)


def test_cpu_step_takes_its_batches_from_the_loader_and_resumes(monkeypatch):
    from mpgan_amd import train
    from mpgan_amd.data import DeviceJetLoader
    monkeypatch.setattr(train.FlatParams, "step", _torch_rmsprop)
    n, B = 11, 4
    particles, labels = _arrays(n)
    loader = DeviceJetLoader((particles, labels), B, "cpu", seed=9)
    ts = _toy_step(loader)
    assert loader.position == 0 and loader.epoch == 0 and loader.steps_per_epoch == 3
    seen, saved = [], None
    for step in range(6):
        ts.step()
        idx = loader.indices(step)
        _check_buffers(ts, particles[idx], labels[idx])
        assert loader.position == (step + 1) * B and loader.epoch == (step + 1) * B // n
        seen.append(ts.data.clone())
        if step == 2:
            saved = loader.state_dict()
    assert saved == {"key": loader.key, "cursor": 12, "n": n, "batch_size": B, "rank": 0, "world_size": 1}
    assert np.array_equal(np.sort(torch.cat([loader.indices(s) for s in range(3)]).numpy()[:n]), np.arange(n))
    # a fresh loader (another default key) from the state saved after the third step serves steps 4-6 again
    fresh = DeviceJetLoader((particles, labels), B, "cpu", seed=1234)
    fresh.load_state_dict(saved)
    ts2 = _toy_step(fresh)
    for step in range(3, 6):
        ts2.step()
        assert torch.equal(ts2.data, seen[step]) and torch.equal(fresh.indices(step), loader.indices(step))
    assert fresh.position == loader.position == 24
    # ... and under another layout the ranks go on contiguously from the saved global position
    two = [DeviceJetLoader((particles, labels), 2, "cpu", rank=r, world_size=2) for r in range(2)]
    for l in two:
        l.load_state_dict(saved)
    assert [l.position for l in two] == [12, 14]
    assert torch.equal(torch.cat([l.indices(3) for l in two]), loader.indices(3))


def test_error_cases(monkeypatch):
    from mpgan_amd import train
    from mpgan_amd.data import DeviceJetLoader
    monkeypatch.setattr(train.FlatParams, "step", _torch_rmsprop)
    arrays = _arrays(11)
    with pytest.raises(ValueError, match="batches of 3"):
        _toy_step(DeviceJetLoader(arrays, 3, "cpu"))
    with pytest.raises(ValueError, match="particles"):
        _toy_step(DeviceJetLoader((torch.zeros(11, N + 1, 4), torch.zeros(11, 1)), 4, "cpu"))
    ts = _toy_step(DeviceJetLoader(arrays, 4, "cpu"))
    with pytest.raises(RuntimeError, match="DeviceJetLoader"):
        ts.set_batch(arrays[0][:4], arrays[1][:4])
    other = DeviceJetLoader(_arrays(12), 4, "cpu")
    with pytest.raises(ValueError, match="11 jets"):
        other.load_state_dict(ts.loader.state_dict())
    # attach_loader is the same door; without a loader set_batch works as ever
    plain = _toy_step(None)
    plain.set_batch(arrays[0][:4], arrays[1][:4])
    plain.attach_loader(DeviceJetLoader(arrays, 4, "cpu"))
    with pytest.raises(RuntimeError):
        plain.set_batch(arrays[0][:4], arrays[1][:4])
