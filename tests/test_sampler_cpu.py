"""CPU: the row stream of bulk generation (``gen.JetSampler``) as far as it lives on the host -- the label draw's host twin
(``mpg_label_pick_host``: the kernel's own function, include/mpgan_amd.h states it), the refusals of the three entry points, which
return before any HIP call, and the host-side rules (no CPU path, the noise functions' default seed)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mpgan_amd.h")
KEY = 0x0123456789ABCDEF


def _word(key, tag, row, grp):
    """The project's counter-based hash as the header spells it out, in Python integers."""
    m = 0xFFFFFFFF
    lo, hi = key & m, (key >> 32) & m
    x = ((row + lo) * 0x9E3779B1) & m
    x ^= (((grp + tag * 0x10001) * 0x85EBCA77) + hi) & m
    x ^= x >> 16; x = (x * 0x7feb352d) & m
    x ^= x >> 15; x = (x * 0x846ca68b) & m
    x ^= x >> 16
    return x


def test_pick_is_the_headers_statement():
    from mpgan_amd import ops
    tag = int(re.search(r"^#define\s+MPG_PICK_TAG\s+(0x[0-9A-Fa-f]+)\s*$", open(HEADER).read(), flags=re.M).group(1), 16)
    assert tag == ops.PICK_TAG
    # (clear of every other family: test_cabi_cpu.py::test_tag_table)
    for n, pos0 in ((7, 0), (1000, 123), (2**31 - 1, 2**32 - 3), (30, 5 * 2**32 + 1)):
        got = ops.label_pick_indices(KEY, pos0, 6, n).tolist()
        want = [(_word(KEY, tag, (pos0 + c) & 0xFFFFFFFF, (pos0 + c) >> 32) * n) >> 32 for c in range(6)]
        assert got == want, (n, pos0)


def test_pick_range_slices_keys_and_far_rows():
    from mpgan_amd import ops
    for n in (1, 2, 7, 31, 1000, 2**31 - 1):
        idx = ops.label_pick_indices(KEY, 0, 4096, n)
        assert idx.dtype == torch.int64 and int(idx.min()) >= 0 and int(idx.max()) < n, n
    assert not bool(ops.label_pick_indices(KEY, 17, 500, 1).any())                   # n = 1: all zeros
    assert torch.equal(ops.label_pick_indices(KEY, 0, 10, 30)[5:], ops.label_pick_indices(KEY, 5, 5, 30))
    assert not torch.equal(ops.label_pick_indices(KEY, 0, 64, 30), ops.label_pick_indices(KEY + 1, 0, 64, 30))
    # rows beyond 2^32: the high word of the row enters the hash, and a slice there is still a slice
    far = 3 * 2**32 + 11
    a = ops.label_pick_indices(KEY, far, 64, 30)
    assert int(a.min()) >= 0 and int(a.max()) < 30 and torch.equal(a[7:], ops.label_pick_indices(KEY, far + 7, 57, 30))
    assert not torch.equal(a, ops.label_pick_indices(KEY, 11, 64, 30))
    assert ops.label_pick_indices(KEY, 0, 0, 30).numel() == 0


def test_pick_is_uniform():
    """n = 7, 70 000 draws under a fixed key: every bin within 5 standard deviations of 10 000
    (sigma = sqrt(70000 * 1/7 * 6/7) = 92.6: +-463).  The draw is deterministic."""
    from mpgan_amd import ops
    counts = np.bincount(ops.label_pick_indices(KEY, 0, 70000, 7).numpy(), minlength=7)
    print("bin counts:", counts.tolist())
    assert counts.sum() == 70000 and np.abs(counts - 10000).max() <= 463, counts.tolist()


def test_entry_points_refuse_what_the_header_says_without_a_device():
    from mpgan_amd import _lib
    L = _lib.lib()
    out = np.zeros(4, dtype=np.int32)
    po = out.ctypes.data_as(C.c_void_p)
    assert L.mpg_label_pick_host(1, 0, 4, 0, po) == -1
    assert L.mpg_label_pick_host(1, 0, 4, 2**31, po) == -1
    assert L.mpg_label_pick_host(1, 0, -1, 5, po) == -1
    assert L.mpg_label_pick_host(1, 0, 4, 5, None) == -1
    assert L.mpg_label_pick_host(1, 0, 4, 2**31 - 1, po) == 0
    # the device launches return before any HIP call.  A host array's address stands in for "not NULL": nothing is launched
    buf = np.zeros(16, dtype=np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    pick = lambda **kw: L.mpg_label_pick(kw.get("table", p), kw.get("n", 3), 1, kw.get("cursor", p), kw.get("B", 2), kw.get("labels", p), None)
    for bad in (dict(n=0), dict(n=2**31), dict(B=0), dict(table=None), dict(cursor=None), dict(labels=None)):
        assert pick(**bad) == -1, bad
    f3 = (C.c_float * 3)(1.0, 1.0, 1.0)
    fin = lambda **kw: L.mpg_jets_finish(kw.get("feat", p), kw.get("ld", 3), None, kw.get("B", 2), kw.get("N", 2), kw.get("maxes", f3), f3, f3,
                                         kw.get("out", p), None, 0, kw.get("total", 2), 1, kw.get("cursor", p), kw.get("seed", p),
                                         kw.get("ticket", p), None)
    for bad in (dict(B=0), dict(N=0), dict(total=-1), dict(feat=None), dict(out=None), dict(cursor=None), dict(seed=None),
                dict(ticket=None), dict(ld=2), dict(maxes=None)):
        assert fin(**bad) == -1, bad
    assert not buf.any()


def test_chunk_seed_words():
    from mpgan_amd import ops
    assert ops.chunk_seed(5, 0) == 5 and ops.chunk_seed(5, 1) == 5 + 0x9E3779B97F4A7C15
    assert ops.chunk_seed(2**64 - 1, 2) == (2**64 - 1 + 2 * 0x9E3779B97F4A7C15) % 2**64     # mod 2^64
    assert ops.u64_as_i64(2**64 - 1) == -1 and ops.u64_as_i64(7) == 7
    assert torch.tensor([ops.u64_as_i64(ops.chunk_seed(2**63, 3))], dtype=torch.int64).item() & (2**64 - 1) == ops.chunk_seed(2**63, 3)


def test_sampler_on_a_cpu_module_raises():
    from mpgan_amd import gen, train
    G, _ = train.default_mpgan(30, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        gen.JetSampler(G, torch.linspace(0, 1, 31), 30)


def test_noise_functions_still_default_to_the_device_seed():
    from mpgan_amd import ops
    for fn in (ops.normal_noise, ops.normal_noise_masked):
        ps = inspect.signature(fn).parameters
        assert ps["seed_t"].default is None and ps["out"].default is None, fn.__name__
        assert list(ps)[:2] == ["shape", "std"] and ps["site"].default == 0 and ps["device"].default == "cuda"
    t = ops.seed_tensor("cpu")
    assert ops._seed_word(None, torch.device("cpu")) is t           # None: the device's own seed word, as before
    mine = torch.zeros(1, dtype=torch.int64)
    assert ops._seed_word(mine, torch.device("cpu")) is mine
    with pytest.raises(ValueError):
        ops._seed_word(torch.zeros(1, dtype=torch.int32), torch.device("cpu"))


def test_evaluate_generator_takes_a_sampler():
    from mpgan_amd import evaluation
    assert inspect.signature(evaluation.evaluate_generator).parameters["sampler"].default is None
