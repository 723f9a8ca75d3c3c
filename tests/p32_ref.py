"""The P32 fp16 plane format and its site header, restated on the host in plain numpy (include/segmm_hip.h "Plane-operand GEMM" and
"PLANE OUTPUTS of producers"; the comments of csrc/common.h).  The yardstick of tests/test_p32_format_gpu.py and of
tests/test_planes_gpu.py's ``_ref_planes``; tests/test_p32_format_cpu.py shows it correct without a GPU.

A matrix X[R][C] (C % 32 == 0) under a power-of-two scale s is stored as ONE fp16 array with row stride ld2 (halves); per row and per
block of 32 columns [32 hi | 32 lo]: element (r, c) has hi at r * ld2 + (c / 32) * 64 + c % 32 and lo 32 halves further on, with

    hi = rn16(x s + 0)         lo = rn16(x s - hi)

each rounded ONCE, to nearest even, fp16 subnormals kept.  The "+ 0" is the device's rule for signed zeros: both device forms of the
split are a fused multiply-add with a +0 addend (v_fma_mix{lo,hi}_f16 x, s, 0), and (-0) + (+0) = +0, so x = -0.0 is stored as
hi = +0 (0x0000), lo = (-0) - (+0) = -0 (0x8000) -- the zero keeps its value, its sign moves to the lo term.  Measured on the MI355X
(gfx950): fp16 subnormal lo terms are KEPT by both forms, bit for bit as numpy rounds them (a third of the lo terms of the 24-octave
input below are subnormal); a NaN comes out as 0x7E00 in both terms.  x s (s a power of two) and x s - hi (at most 13 significant bits left
of the 24) are exact in fp32, so "rounded once from the exact value" (the fused multiply-add forms of the kernels) and "computed in
fp32, then rounded" (here) are the same number; ``split`` asserts both exactness claims instead of assuming them.

The site header of a plane tensor is SITE_HDR floats followed by AMAX_SLOTS partial maxima of |x|: hdr[0] the scale the planes were
written with, hdr[1] != 0 (as an integer) when an element left the fp16 range under that scale.
"""
import numpy as np

SITE_HDR = 8
AMAX_SLOTS = 256
SITE_FLOATS = SITE_HDR + AMAX_SLOTS
F16_MAX = np.float32(65504.0)
CANARY = 0x7BFF          # a finite fp16 pattern (65504) no split of the test inputs writes next to itself by accident


# |hi + lo - x s|: hi = rn16(p) leaves d = p - hi with |d| <= 2^-11 |p| (11-bit significand; p = x s).  lo = rn16(d) is off by at most
# 2^-11 |d| <= 2^-22 |p| while lo is a normal fp16 number, and by at most 2^-25 -- half the subnormal spacing 2^-24 -- once |d| < 2^-14.
# 2^-25 <= 2^-22 |p| from |p| = 2^-3 on; below 2^-3, |d| <= 2^-14 is always in (or at the edge of) the subnormal range.  (|p| < 2^-14:
# hi itself is subnormal, |d| <= 2^-25, and lo -- a multiple of 2^-24 -- is again within 2^-25.)
REL, ABS, KNEE = 2.0 ** -22, 2.0 ** -25, 2.0 ** -3


def exact_scale(amax):
    """The power of two s with amax * s in [2^14, 2^15), its exponent clamped to +-60; 1 for amax = 0, NaN or Inf."""
    a = np.float32(amax)
    if not (a > 0) or not np.isfinite(a):
        return np.float32(1.0)
    e = int(np.frexp(a)[1]) - 1          # a in [2^e, 2^(e+1))
    return np.float32(2.0 ** max(-60, min(60, 14 - e)))


def amax_of(x):
    """max |x| as the producers record it: their maxima are taken with fmaxf, which drops a NaN operand."""
    a = np.abs(np.asarray(x, dtype=np.float32)).reshape(-1)
    return np.float32(np.fmax.reduce(a, initial=np.float32(0.0))) if a.size else np.float32(0.0)


def split(x, s):
    """(hi, lo) as fp16 arrays of x's shape: hi = rn16(x s + 0), lo = rn16(x s - hi)."""
    x = np.asarray(x, dtype=np.float32)
    s = np.float32(s)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        p = x * s
        fin = np.isfinite(x)
        assert np.array_equal(p[fin].astype(np.float64), x[fin].astype(np.float64) * np.float64(s)), "x * s is not exact in fp32"
        hi = (p + np.float32(0.0)).astype(np.float16)          # (-0) + (+0) = +0: a zero product is stored as hi = +0
        d = p - hi.astype(np.float32)
        ok = np.isfinite(hi)
        assert np.array_equal(d[ok].astype(np.float64), p[ok].astype(np.float64) - hi[ok].astype(np.float64)), "x * s - hi is not exact in fp32"
        lo = d.astype(np.float16)
    return hi, lo


def _offsets(R, C, ld2):
    assert C % 32 == 0 and ld2 >= 2 * C
    r = np.arange(R, dtype=np.int64)[:, None]
    c = np.arange(C, dtype=np.int64)[None, :]
    return r * ld2 + (c // 32) * 64 + c % 32


def pack(x2d, s, ld2=None, fill=CANARY):
    """(image, written): the uint16 plane image [R * ld2] of x2d [R, C] under scale s -- halves no element maps to hold ``fill`` --
    and the bool mask of the halves that were written."""
    x2d = np.asarray(x2d, dtype=np.float32)
    R, C = x2d.shape
    ld2 = 2 * C if ld2 is None else int(ld2)
    hi, lo = split(x2d, s)
    off = _offsets(R, C, ld2)
    img = np.full(R * ld2, fill, dtype=np.uint16)
    written = np.zeros(R * ld2, dtype=bool)
    img[off] = hi.view(np.uint16)
    img[off + 32] = lo.view(np.uint16)
    written[off] = True
    written[off + 32] = True
    return img, written


def pack_transposed(x2d, s, ld2=None, fill=CANARY):
    """Planes of the transpose: plane row c holds x2d[:, c]; the blocks of 32 run over the rows of x2d (R % 32 == 0, ld2 >= 2 R)."""
    x2d = np.asarray(x2d, dtype=np.float32)
    return pack(np.ascontiguousarray(x2d.T), s, ld2, fill)


def unpack(img, R, C, ld2=None):
    """(hi, lo) fp16 arrays [R, C] read back from a plane image."""
    ld2 = 2 * C if ld2 is None else int(ld2)
    img = np.asarray(img).reshape(-1).view(np.uint16)
    off = _offsets(R, C, ld2)
    return img[off].view(np.float16), img[off + 32].view(np.float16)


def overflow_flag(x, s):
    """Raised iff not (max|x| * s < 65504), evaluated in fp32; a NaN anywhere in x raises it."""
    a = np.abs(np.asarray(x, dtype=np.float32)).reshape(-1)
    if a.size == 0:
        return False
    with np.errstate(over="ignore", invalid="ignore"):
        return not bool(np.float32(a.max()) * np.float32(s) < F16_MAX)          # (ndarray.max propagates a NaN)


def flag_boundaries(s):
    """(name, maximum, flag) at the edge of the fp16 range under the scale s: the last fp32 value below 65504, 65504 itself, a value
    between 65504 and the rounding tie 65520 (its hi term is still the finite 65504), and a NaN."""
    s = np.float32(s)
    return [("below", np.nextafter(F16_MAX, np.float32(0)) / s, False), ("at", F16_MAX / s, True),
            ("above_hi_finite", np.float32(65512.0) / s, True), ("nan", np.float32("nan"), True)]


def planes_ok(amax, s, flag):
    """The consumer's rule (common.h, comment of site_planes_ok): planes written with the scale s are usable iff a scale was written,
    the flag is down and the tensor's maximum sits inside the fp16 window -- below 65504, and not below 2^-2 (the lo terms would sink
    into the subnormals) unless the scale already stands at its upper clamp 2^60.  An all-zero tensor is always usable."""
    amax, s = np.float32(amax), np.float32(s)
    if not (s > 0) or flag:
        return False
    if not (amax > 0):
        return True
    with np.errstate(over="ignore"):
        m = amax * s
    return bool((m >= np.float32(0.25) or s >= np.float32(2.0 ** 60)) and m < F16_MAX)


def slot_fill(x, n=AMAX_SLOTS):
    """n complete partial maxima of |x|, the way a producer leaves them: chunk k of the flattened tensor in slot k."""
    a = np.abs(np.asarray(x, dtype=np.float32)).reshape(-1)
    return np.array([np.fmax.reduce(ch, initial=np.float32(0.0)) for ch in np.array_split(a, n)], dtype=np.float32)


def log_uniform(n, octaves, seed, top=1.0):
    """n fp32 values of random sign with magnitudes log-uniform over ``octaves`` octaves below ``top``; element 0 is the maximum
    itself, just below ``top``, so that the exact scale maps [top / 2^octaves, top) onto [2^(15 - octaves), 2^15)."""
    rng = np.random.RandomState(seed)
    mag = np.float64(top) * 2.0 ** (-octaves * rng.random_sample(n))
    x = (mag * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    x[0] = np.nextafter(np.float32(top), np.float32(0.0))
    return x


# the input of the reconstruction-error test, shared with the GPU tests: 2^20 values over 24 octaves.  Under the exact scale
# |x s| runs over [2^-9, 2^15): the twelve octaves [2^3, 2^15) of a well-scaled tensor, in which hardly any lo term is subnormal
# (|x s - hi| < 2^-14 has probability 2^(-3-e) in octave e), and twelve more in which most are -- every lo term below 2^-3.
LOG_N, LOG_OCTAVES, LOG_SEED = 1 << 20, 24, 1234
_LOG = {}


def log_input(octaves=LOG_OCTAVES):
    if octaves not in _LOG:
        x = log_uniform(LOG_N, octaves, LOG_SEED)
        x.setflags(write=False)
        _LOG[octaves] = x
    return _LOG[octaves]
