"""What the 8-bit input features MEAN, stated once on the host (no GPU, no library).

1. Widening.  ``widen_table(dtype)`` is the float32 value of each of the 256 codes: torch's CPU ``uint8 view -> .float()`` for the two
   OCP float formats (``torch.float8_e4m3fn``, ``torch.float8_e5m2``), a sign extension for ``torch.int8``.  ``widen(t)`` applies it
   to a tensor.  The kernels (segmm_gather_l1_b, segmm_l1norm_b) are "the float32 kernel on widen(t)", bit for bit.

2. The row quantiser, ``quantize_rows`` -- the rule segmm_quantize_rows gives the bytes of, in numpy float32 operations:
     a = max|x_j|;  a < 2^-100 or not finite: all-zero codes, scale 0
     e4m3: a = m 2^e (frexp), s = 2^(8-e);  e5m2: s = 2^(15-e);  codes = RNE(x s)   (s is a power of two: x s is exact, |x s| < 256 / 32768)
     int8: r = fp32(127) / a,  codes = rint(fp32(x r))                              (in +-127)
   RNE onto an fp8 grid is written out in integer operations (``fp8_codes``): at or above the format's smallest normal the float32
   mantissa is rounded to M bits in place, below it the code is the count of subnormal steps.  tests/test_feature8_cpu.py checks that
   this equals torch's own float32 -> float8 cast on the values the rule can produce."""
import numpy as np
import torch

F = np.float32
E4M3, E5M2, I8 = torch.float8_e4m3fn, torch.float8_e5m2, torch.int8
DTYPES = (E4M3, E5M2, I8)
NAMES = {E4M3: "e4m3", E5M2: "e5m2", I8: "int8"}
ELEM = {E4M3: 3, E5M2: 4, I8: 5}          # SEGMM_ELEM_E4M3 / _E5M2 / _I8
# (exponent bias, mantissa bits, exponent of the row target: |x s| < 2^TOP)
FP8 = {E4M3: (7, 3, 8), E5M2: (15, 2, 15)}
A_MIN = F(2.0 ** -100)


def widen_table(dtype):
    """float32 [256]: the value of every code"""
    codes = torch.arange(256, dtype=torch.uint8)
    if dtype == I8:
        return ((codes.to(torch.int32) ^ 128) - 128).to(torch.float32)
    return codes.view(dtype).float()


def codes_of(t):
    """the raw bytes of an 8-bit tensor (uint8, same shape)"""
    return t.contiguous().view(torch.uint8)


def widen(t):
    """float32 tensor of the exact values of an 8-bit tensor ``t`` (any device), by table lookup"""
    return widen_table(t.dtype).to(t.device)[codes_of(t).long()]


def from_codes(codes, dtype):
    """uint8 array / tensor -> tensor of ``dtype`` with those bytes"""
    c = torch.as_tensor(np.ascontiguousarray(codes) if isinstance(codes, np.ndarray) else codes).contiguous()
    assert c.dtype == torch.uint8
    return c.view(dtype)


def fp8_codes(v, dtype):
    """RNE of float32 ``v`` (finite, inside the format's range) onto the fp8 grid of ``dtype`` -> uint8 codes"""
    EB, M, _ = FP8[dtype]
    v = np.ascontiguousarray(v, dtype=F)
    b = v.view(np.uint32).astype(np.int64)
    sign = (b >> 24) & 0x80
    u = b & 0x7FFFFFFF
    normal = u >= ((127 + 1 - EB) << 23)
    un = u + ((u >> (23 - M)) & 1) + ((1 << (22 - M)) - 1)
    cn = (un >> (23 - M)) - ((127 - EB) << M)
    with np.errstate(all="ignore"):
        cs = np.rint(np.abs(v) * F(2.0 ** (EB - 1 + M))).astype(np.int64)          # the product is exact; rint rounds to even
    return (sign | np.where(normal, cn, cs)).astype(np.uint8)


def row_scale(x, dtype):
    """float32 [rows]: the factor each row is multiplied by (0: a dead row -- a < 2^-100 or not finite)"""
    x = np.ascontiguousarray(x, dtype=F)
    with np.errstate(all="ignore"):
        a = np.max(np.abs(x), axis=1)          # propagates NaN
        live = np.isfinite(a) & (a >= A_MIN)
        a1 = np.where(live, a, F(1)).astype(F)
        if dtype == I8:
            s = (F(127) / a1).astype(F)
        else:
            _, e = np.frexp(a1)
            s = np.ldexp(F(1), FP8[dtype][2] - e).astype(F)
    return np.where(live, s, F(0)).astype(F)


def scaled(x, dtype):
    """float32 [rows, D]: fp32(x s), what the codes are rounded from (dead rows: 0)"""
    x = np.ascontiguousarray(x, dtype=F)
    s = row_scale(x, dtype)
    with np.errstate(all="ignore"):
        v = (x * s[:, None]).astype(F)
    v[s == 0] = 0
    return v


def quantize_rows(x, dtype):
    """-> (codes uint8 [rows, D], scale float32 [rows])"""
    s = row_scale(x, dtype)
    v = scaled(x, dtype)
    if dtype == I8:
        q = (np.rint(v).astype(np.int64) & 0xFF).astype(np.uint8)
    else:
        q = fp8_codes(v, dtype)
    q[s == 0] = 0
    return q, s


# the error of one code in SCALED units, from the formats: half a step of the grid at |v| -- relative 2^-(M+1) above the smallest normal,
# half a subnormal step below it -- plus 2^-16 for the float32 product (int8: x r is rounded once, relative 2^-24 of at most 127.5)
def code_error_bound(v, dtype):
    av = np.abs(np.asarray(v, dtype=np.float64))
    if dtype == E4M3:
        return np.maximum(2.0 ** -4 * av, 2.0 ** -10) + 2.0 ** -16
    if dtype == E5M2:
        return np.maximum(2.0 ** -3 * av, 2.0 ** -17) + 2.0 ** -16
    return np.full_like(av, 0.5) + 2.0 ** -16
