"""CPU: the host side of the sparse k-NN route of the fused MPLayer (``mpg_knn_edge_fwd`` / ``mpg_knn_edge_bwd``): struct layouts,
the option, the launch plan and the route selection.  No compute calls."""
import ctypes
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mpgan_amd.h")

GRID = [(1, 30, 1), (3, 30, 10), (2, 40, 7), (2, 150, 20), (16, 150, 20), (256, 30, 10), (2, 9, 8), (1, 192, 191), (5, 33, 32), (64, 64, 32)]


def test_struct_layouts_match_header():
    """sizeof of the two new structs as gcc sees the header == ctypes.sizeof of the Python mirrors; both entry points are bound."""
    from mpgan_amd import _lib
    structs = ["MpgKnnEdgeFwd", "MpgKnnEdgeBwd"]
    src = '#include <stdio.h>\n#include "mpgan_amd.h"\nint main(){' + "".join(
        f'printf("{s} %zu\\n", sizeof({s}));' for s in structs) + "return 0;}"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-I", os.path.dirname(HEADER), c, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    sizes = dict(line.split() for line in out.strip().splitlines())
    for s in structs:
        assert int(sizes[s]) == ctypes.sizeof(getattr(_lib, s)), s
    assert "mpg_knn_edge_fwd" in _lib.SIGNATURES and "mpg_knn_edge_bwd" in _lib.SIGNATURES
    lib = _lib.lib()
    assert hasattr(lib, "mpg_knn_edge_fwd") and hasattr(lib, "mpg_knn_edge_bwd")


def test_option_exists_and_is_off_by_default():
    """``OPTIONS["knn_sparse"]`` follows MPG_KNN_SPARSE and is off without it (a fresh interpreter: the test process may carry
    the variable)."""
    from mpgan_amd import ops
    assert "knn_sparse" in ops.OPTIONS and isinstance(ops.OPTIONS["knn_sparse"], bool)
    code = "from mpgan_amd import ops; print(int(ops.OPTIONS['knn_sparse']))"
    for val, want in ((None, "0"), ("0", "0"), ("1", "1")):
        env = {k: v for k, v in os.environ.items() if k != "MPG_KNN_SPARSE"}
        if val is not None:
            env["MPG_KNN_SPARSE"] = val
        env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
        out = subprocess.run([os.sys.executable, "-c", code], check=True, capture_output=True, text=True, env=env, cwd=ROOT).stdout
        assert out.strip() == want, (val, out)


@pytest.mark.parametrize("B,N,k", GRID)
@pytest.mark.parametrize("need_grad", [False, True])
def test_knn_plan_invariants(B, N, k, need_grad):
    from mpgan_amd import ops
    p = ops.knn_plan(B, N, k, need_grad)
    assert p.rows == N * k
    assert 1 <= p.RW <= N and p.workgroups == B * -(-N // p.RW)
    assert p.RW * k * ops.KNN_STAGE_BYTES <= ops.KNN_LDS_BYTES           # a workgroup's rows fit its LDS
    tiles = ops.knn_block_tiles(N, k, p.RW)
    assert p.tiles == len(tiles)
    # every edge row lies in exactly one tile
    seen = [0] * (N * k)
    for r0, n in tiles:
        assert 1 <= n <= 32
        for r in range(r0, r0 + n):
            seen[r] += 1
    assert seen == [1] * (N * k)
    # no receiver's rows are split across workgroups, and no tile reaches into another workgroup's rows
    for i in range(N):
        assert len({(i * k + r) // (p.RW * k) for r in range(k)}) == 1
    for r0, n in tiles:
        assert r0 // (p.RW * k) == (r0 + n - 1) // (p.RW * k)
    # parked bytes: E1 [rows, 96] and E2 [rows, 160] in fp32 and six pairs of 16-bit sign words per row; gradient rows in fp32
    assert ops.KNN_PARK_ROW_BYTES == 96 * 4 + 160 * 4 + 6 * 2 * 2 and ops.KNN_GRAD_ROW_BYTES == (96 + 160 + 192) * 4
    assert p.parked_bytes == (B * N * k * ops.KNN_PARK_ROW_BYTES if need_grad else 0)
    assert p.grad_bytes == (B * N * k * ops.KNN_GRAD_ROW_BYTES if need_grad else 0)


def test_knn_plan_fills_the_cus_where_it_can():
    from mpgan_amd import ops
    assert ops.knn_plan(16, 150, 20, True).workgroups >= ops.NUM_CUS
    assert ops.knn_plan(256, 30, 10, True).workgroups >= ops.NUM_CUS
    small = ops.knn_plan(2, 150, 20, True)       # 300 receivers: one each rather than 50 workgroups of six
    assert small.workgroups >= ops.NUM_CUS and small.RW == 1
    tiny = ops.knn_plan(1, 30, 1, False)         # 30 rows in all: not a workgroup per row
    assert tiny.RW * 1 >= 30 and tiny.workgroups == 1


def test_knn_plan_guard_raises_above_2gib():
    from mpgan_amd import ops
    rows = 150 * 20
    ok = 0x7fffffff // (rows * ops.KNN_GRAD_ROW_BYTES)
    ops.knn_plan(ok, 150, 20, True)
    with pytest.raises(RuntimeError, match="2 GiB"):
        ops.knn_plan(ok + 1, 150, 20, True)
    ops.knn_plan(ok + 1, 150, 20, False)         # (nothing is parked without a backward)
    for bad in ((2, 30, 0), (2, 30, 31), (2, 193, 10), (0, 30, 10)):
        with pytest.raises(ValueError):
            ops.knn_plan(*bad, True)


def test_route_selection():
    """The sparse launches are taken only with neighbour sets, the option on, no edge scalars and k < N; spectral norm, other widths
    and the double-backward route keep the routes they have."""
    from mpgan_amd import ops
    on, off = dict(ops.OPTIONS, knn_sparse=True), dict(ops.OPTIONS, knn_sparse=False)
    assert ops.knn_sparse_route(True, 0, 30, 10, options=on)
    assert not ops.knn_sparse_route(True, 0, 30, 10, options=off)
    assert not ops.knn_sparse_route(False, 0, 30, 10, options=on)               # fully connected
    assert not ops.knn_sparse_route(True, 1, 30, 10, options=on)                # edge scalars (nq > 0)
    assert not ops.knn_sparse_route(True, 2, 30, 10, options=on)
    assert not ops.knn_sparse_route(True, 0, 30, 30, options=on)                # k = N: every sender
    assert not ops.knn_sparse_route(True, 0, 30, 10, spectral_norm=True, options=on)
    assert not ops.knn_sparse_route(True, 0, 30, 10, fused=False, options=on)   # other widths: the un-fused layer
    assert not ops.knn_sparse_route(True, 0, 30, 10, double_backward=True, options=on)
    assert ops.knn_sparse_route(True, 0, 150, 20, options=on) and ops.knn_sparse_route(True, 0, 9, 8, options=on)
    # the settings of a call: a spectral-norm layer says so, everyone else may go sparse
    assert ops.MPLayerSettings(True, 0.2, 0.0, False).sparse_ok is True and "sparse_ok" in ops.MPLayerSettings._fields
    assert ops.KnnSaved._fields == ("E1", "E2", "sign3")


def test_layers_of_other_configurations_do_not_reach_the_sparse_route(monkeypatch):
    """What MPLayer.forward decides before it calls the fused function: other widths are not fused at all, a layer with edge scalars
    has n_es > 0, a spectral-norm layer is refused by ``knn_sparse_route``."""
    from mpgan_amd import ops
    from mpgan_amd.mpgan import MPLayer
    monkeypatch.setitem(ops.OPTIONS, "knn_sparse", True)
    plain = MPLayer(32, [96, 160, 192], [256, 256], 32, fully_connected=False, num_knn=10)
    assert plain.fused and ops.knn_sparse_route(True, plain.n_es, 30, plain.num_knn, spectral_norm=plain.spectral_norm)
    ef = MPLayer(32, [96, 160, 192], [256, 256], 32, fully_connected=False, num_knn=5, pos_diffs=True)
    assert ef.fused and ef.n_es > 0 and not ops.knn_sparse_route(True, ef.n_es, 30, ef.num_knn, spectral_norm=ef.spectral_norm)
    sn = MPLayer(32, [96, 160, 192], [256, 256], 32, fully_connected=False, num_knn=10, spectral_norm=True)
    assert not ops.knn_sparse_route(True, sn.n_es, 30, sn.num_knn, spectral_norm=sn.spectral_norm)
    other = MPLayer(16, [64, 48], [40], 8, fully_connected=False, num_knn=10)
    assert not other.fused
    assert not ops.knn_sparse_route(True, 0, 30, 10, fused=other.fused)
