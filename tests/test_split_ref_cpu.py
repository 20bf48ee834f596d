"""The numpy emulation of the three-term hi/lo product (tests/split_ref.py) pinned to the figures the documentation states for it
("Operand magnitudes of the un-fused route") -- the GPU test of ``ops.linear_fwd`` bounds the kernel by this emulation,
so the emulation itself must not drift."""
import numpy as np
import pytest

import split_ref as S


def test_rounding_helpers():
    x = np.array([1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 65504.0, 65520.0, 2.0 ** -24, 2.0 ** -26, -0.1], dtype=np.float32)
    h = S.round_f16(x)
    # ties go to even; 65520 is the first value that rounds to inf; 2^-24 is the smallest subnormal, 2^-26 rounds to zero
    assert h[0] == 1.0 and h[1] == 1.0 and h[2] == np.float32(1.0 + 2.0 ** -9) and h[3] == 65504.0 and np.isinf(h[4])
    assert h[5] == np.float32(2.0 ** -24) and h[6] == 0.0
    y = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 2.0 ** 100, 2.0 ** -100 * 1.5, -0.1], dtype=np.float32)
    b = S.round_bf16(y)
    assert b[0] == 1.0 and b[1] == 1.0 and b[2] == np.float32(1.0 + 2.0 ** -6) and b[3] == np.float32(2.0 ** 100)
    assert b[4] == np.float32(2.0 ** -100 * 1.5)
    assert (b.view(np.uint32) & 0xFFFF == 0).all()
    # hi + lo restores 16 bits (bf16) / 22 bits (fp16, at unit magnitude) of the value
    rs = np.random.RandomState(1)
    v = rs.normal(size=4096).astype(np.float32)
    for f16, bits in ((False, 16), (True, 22)):
        hi, lo = S.split(v, f16)
        assert np.abs((hi.astype(np.float64) + lo) - v).max() <= np.abs(v).max() * 2.0 ** -bits


@pytest.mark.parametrize("e", sorted(S.TABLE_F16))
def test_fp16_split_error_per_scale(e):
    """Within 10 % of the tabulated figure (the table has two digits)."""
    got = S.split_err(e, True)
    assert abs(got - S.TABLE_F16[e]) <= 0.1 * S.TABLE_F16[e], (e, got)


@pytest.mark.parametrize("e", S.E_BF16)
def test_bf16_split_error_is_flat(e):
    got = S.split_err(e, False)
    assert abs(got - S.TABLE_BF16) <= 0.1 * S.TABLE_BF16, (e, got)


def test_fp16_overflows_where_bf16_does_not():
    assert np.isnan(S.split_err(15.9, True))
    assert S.split_err(15.9, False) < 5e-6
    assert S.split_err(14, True) < 2e-7      # the largest scale the GPU test runs on the fp16 route: still inside the range


def test_bound_of_the_fp16_route():
    """4 x (split error + plain fp32 product error); the fp32 product itself sits below 1e-6 on these operands."""
    for e in S.E_F16:
        assert S.fp32_product_err(e) < 1e-6
        assert S.f16_bound(e) == 4.0 * (S.split_err(e, True) + S.fp32_product_err(e))
    assert S.f16_bound(-10) < 1e-4     # TIGHT holds down to 2^-10 with the margin included
