"""A numpy emulation of the three-term hi/lo product ``mpg_gemm`` forms on the matrix cores (csrc/common.h: split8, mfma3), and
the operands the magnitude tests share (tests/test_split_ref_cpu.py, tests/test_gpu_gemm.py).

Every float32 operand x is split into hi = round16(x) and lo = round16(x - hi), round16 = round-to-nearest-even to fp16
(11 significant bits, normal down to 2^-14, subnormal steps of 2^-24, inf beyond 65504) or to bf16 (8 bits, float32's own
exponent range).  A product is hi*hi' + hi*lo' + lo*hi'; the lo*lo' term is left out.  The emulation adds the terms up in fp64
and rounds the sum to fp32 once, so its error against the fp64 product of the float32 operands is the error of the split alone;
the matrix cores add in fp32, which ``fp32_product_err`` measures on the same operands."""
import numpy as np

M, N, K = 96, 80, 72
SEED = 0
# what the emulation gives at these shapes and this seed under ``rel_err`` (max|err| / max|ref|), A scaled by 2^e: the fp16
# pair keeps its 22 bits only while lo stays a normal fp16 number; below that the product fades out, above 65504 hi is inf
TABLE_F16 = {0: 9e-8, -6: 1.2e-6, -10: 1.7e-5, -13: 1.25e-4, -16: 1.0e-3, -20: 1.7e-2, -40: 1.0}
TABLE_BF16 = 4.5e-6     # at every scale: bf16 has float32's exponents
E_BF16 = [0, -6, -10, -13, -16, -20, 14, -40, 40]
E_F16 = [0, -6, -10, -13, -16, -20, 14]


def round_f16(x):
    """float32 -> fp16 (round to nearest even, subnormals kept, inf beyond the range) -> float32."""
    with np.errstate(over="ignore"):
        return np.asarray(x, dtype=np.float32).astype(np.float16).astype(np.float32)


def round_bf16(x):
    """float32 -> bf16 (round to nearest even on the upper 16 bits) -> float32."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def split(x, f16):
    r = round_f16 if f16 else round_bf16
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        hi = r(x)
        lo = r(x - hi)      # (the residual is exact in float32)
    return hi, lo


def split_product(A, B, f16):
    """(A B^T) as the kernels form it, A [M, K] and B [N, K] float32: three terms, accumulated in fp64, rounded to fp32."""
    ah, al = (t.astype(np.float64) for t in split(A, f16))
    bh, bl = (t.astype(np.float64) for t in split(B, f16))
    with np.errstate(invalid="ignore", over="ignore"):
        return (ah @ bh.T + ah @ bl.T + al @ bh.T).astype(np.float32)


def operands(e=0):
    """The shared case: A [M, K] ~ N(0, 1) times 2^e (exact in float32) and B [N, K] ~ N(0, 1), float32."""
    rs = np.random.RandomState(SEED)
    A = rs.normal(size=(M, K)).astype(np.float32)
    B = rs.normal(size=(N, K)).astype(np.float32)
    return A * np.float32(2.0 ** e), B


def reference(A, B):
    return A.astype(np.float64) @ B.astype(np.float64).T


def rel_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    den = np.abs(b).max()
    with np.errstate(invalid="ignore"):
        return float(np.abs(a - b).max() / (den if den > 0 else 1.0))


def split_err(e, f16):
    """Error of the emulated split product at scale 2^e against fp64."""
    A, B = operands(e)
    return rel_err(split_product(A, B, f16), reference(A, B))


def fp32_product_err(e):
    """Error of a plain float32 numpy product of the same operands against fp64: what fp32 accumulation costs."""
    A, B = operands(e)
    return rel_err(A @ B.T, reference(A, B))


def f16_bound(e):
    """What the fp16 route is held to at scale 2^e, from the reference side alone: the emulated split error plus the error of
    a plain fp32 product (the emulation accumulates in fp64, the matrix pipe in fp32), times 4 (the maximum over M N rounding
    walks varies from one summation order to another)."""
    return 4.0 * (split_err(e, True) + fp32_product_err(e))
