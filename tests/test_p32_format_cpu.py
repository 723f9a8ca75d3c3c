"""The host statement of the P32 plane format (tests/p32_ref.py) without a GPU: reconstruction error of the two-term split where
the lo terms are normal and where they are fp16 subnormals, the exact scale's window and clamps, the overflow flag at the edge of
the fp16 range, the consumers' window rule, pack / unpack, numpy against torch rounding -- and the argument checks of the three C
entry points the format's kernels sit behind."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import p32_ref as P      # noqa: E402


def _errors(x, s):
    hi, lo = P.split(x, s)
    p = x.astype(np.float64) * float(s)
    return p, np.abs(hi.astype(np.float64) + lo.astype(np.float64) - p), hi, lo


@pytest.mark.parametrize("octaves", [24, 44])
def test_split_reconstruction_error_in_the_normal_and_the_subnormal_range(octaves):
    """2^20 log-uniform values at the exact scale: 24 octaves (the GPU tests' input; about 30 % of the lo terms are subnormal) and
    44 octaves (|x s| down to 2^-29: hi terms subnormal and zero too)."""
    x = P.log_input(octaves)
    s = P.exact_scale(P.amax_of(x))
    assert 2.0 ** 14 <= float(P.amax_of(x)) * float(s) < 2.0 ** 15
    p, err, hi, lo = _errors(x, s)
    big = np.abs(p) >= P.KNEE
    lo_sub = (lo != 0) & (np.abs(lo.astype(np.float64)) < 2.0 ** -14)
    worst_rel, worst_abs = float((err[big] / np.abs(p[big])).max()), float(err[~big].max())
    print("octaves %d: worst relative error %.4f x 2^-22, worst absolute error %.4f x 2^-25, subnormal lo terms %.1f %%, subnormal or zero hi %d"
          % (octaves, worst_rel / P.REL, worst_abs / P.ABS, 100.0 * lo_sub.mean(), int((np.abs(hi.astype(np.float64)) < 2.0 ** -14).sum())))
    assert big.sum() > 1000 and (~big).sum() > 1000
    assert lo_sub.mean() > 0.2, "the input does not exercise the subnormal range"
    assert (err[big] <= P.REL * np.abs(p[big])).all()
    assert (err[~big] <= P.ABS).all()
    if octaves == 44:
        assert (np.abs(hi.astype(np.float64)) < 2.0 ** -14).sum() > 1000
    # a split that flushed its subnormal lo terms would miss the bound: the test has teeth
    flushed = np.where(lo_sub, np.float16(0), lo)
    err_f = np.abs(hi.astype(np.float64) + flushed.astype(np.float64) - p)
    assert (err_f[~big] > P.ABS).any() or (err_f[big] > P.REL * np.abs(p[big])).any()


def test_split_rounds_each_term_once_to_nearest_even():
    """Known answers: ties, the fused subtract, signed zero, the top of the range."""
    one = np.float32(1.0)
    # 2049 = 2048 + 1 sits between the fp16 neighbours 2048 and 2050: the tie goes to even (2048), lo = +1; 2051 -> 2052, lo = -1
    hi, lo = P.split(np.array([2049.0, 2051.0, -2049.0], dtype=np.float32), one)
    assert hi.tolist() == [2048.0, 2052.0, -2048.0] and lo.tolist() == [1.0, -1.0, -1.0]
    # lo needs the subtract: x = 1 + 2^-11 + 2^-20 -> hi = 1 (tie to even would give 1; above the tie: 1 + 2^-10), lo = the rest
    x = np.array([1.0 + 2.0 ** -11 + 2.0 ** -20], dtype=np.float32)
    hi, lo = P.split(x, one)
    assert float(hi[0]) == 1.0 + 2.0 ** -10 and float(lo[0]) == float(x[0]) - float(hi[0]) and float(lo[0]) < 0
    # lo in the subnormals: kept as a multiple of 2^-24, ties to even (x = 2^-4 + 3 * 2^-25 -> lo = 2 * 2^-24: 1.5 -> 2)
    hi, lo = P.split(np.array([2.0 ** -4 + 2.0 ** -24, 2.0 ** -4 + 3 * 2.0 ** -25, 2.0 ** -4 + 2.0 ** -25], dtype=np.float32), one)
    assert hi.tolist() == [2.0 ** -4] * 3 and lo.tolist() == [2.0 ** -24, 2.0 ** -23, 0.0]
    # signed zero, the device's rule (fma with a +0 addend): hi = (-0) + (+0) = +0, lo = (-0) - (+0) = -0; the value is unchanged
    hi, lo = P.split(np.array([-0.0, 0.0], dtype=np.float32), np.float32(4.0))
    assert hi.view(np.uint16).tolist() == [0, 0] and lo.view(np.uint16).tolist() == [0x8000, 0]
    # the top: 65504 and everything below the tie 65520 stay finite; 65520 rounds to infinity and drags lo along; NaN stays NaN
    hi, lo = P.split(np.array([65504.0, 65512.0, 65519.996, 65520.0, np.nan], dtype=np.float32), one)
    assert hi[:3].tolist() == [65504.0] * 3 and lo[:3].tolist() == [0.0, 8.0, 16.0]
    assert np.isinf(hi[3]) and hi[3] > 0 and np.isinf(lo[3]) and lo[3] < 0 and np.isnan(hi[4]) and np.isnan(lo[4])
    # the scale is applied before the first rounding
    hi, lo = P.split(np.array([2049.0 / 1024.0], dtype=np.float32), np.float32(1024.0))
    assert (float(hi[0]), float(lo[0])) == (2048.0, 1.0)


def test_split_refuses_a_product_that_is_not_exact():
    with pytest.raises(AssertionError, match="x \\* s"):
        P.split(np.array([1e-40], dtype=np.float32), np.float32(2.0 ** -20))          # underflows past the fp32 subnormals


def test_exact_scale_window_and_clamps():
    rng = np.random.RandomState(5)
    for a in np.concatenate([2.0 ** rng.uniform(-45, 74, 2000), 2.0 ** np.arange(-45.0, 75.0), np.nextafter(2.0 ** np.arange(-45.0, 75.0), 0)]).astype(np.float32):
        s = P.exact_scale(a)
        m, e = np.frexp(s)
        assert m == 0.5 and s.dtype == np.float32          # a power of two
        assert 2.0 ** 14 <= float(a) * float(s) < 2.0 ** 15, (a, s)
    assert P.exact_scale(2.0 ** 14) == 1 and P.exact_scale(np.nextafter(np.float32(2.0 ** 14), np.float32(0))) == 2
    # clamps: 2^60 from amax < 2^-45 down (fp32 subnormals included), 2^-60 from amax >= 2^75 up
    assert P.exact_scale(2.0 ** -46) == P.exact_scale(2.0 ** -60) == P.exact_scale(1e-45) == np.float32(2.0 ** 60)
    assert P.exact_scale(2.0 ** -45) == np.float32(2.0 ** 59)
    assert P.exact_scale(2.0 ** 74) == P.exact_scale(2.0 ** 75) == P.exact_scale(3e38) == np.float32(2.0 ** -60)
    assert P.exact_scale(2.0 ** 73) == np.float32(2.0 ** -59)
    for a in (0.0, -0.0, float("nan"), float("inf"), -1.0):
        assert P.exact_scale(a) == 1
    assert P.amax_of(np.array([1.0, float("nan"), -3.0], dtype=np.float32)) == 3 and P.amax_of(np.zeros(0)) == 0


@pytest.mark.parametrize("s", [1.0, 4.0, 2.0 ** -7, 2.0 ** 20])
def test_overflow_flag_at_the_edge_of_the_fp16_range(s):
    rng = np.random.RandomState(2)
    for name, m, want in P.flag_boundaries(s):
        x = (rng.standard_normal(257) * 100.0 / s).astype(np.float32)
        x[101] = -m if name == "above_hi_finite" else m
        assert P.overflow_flag(x, s) is want, name
        hi, lo = P.split(x, s)
        if name != "nan":
            assert np.isfinite(hi).all() and np.isfinite(lo).all()          # the flag is up before a term becomes infinite
            assert abs(float(hi[101])) == 65504.0
    x = np.array([65520.0, 1.0], dtype=np.float32)
    assert P.overflow_flag(x, 1.0) and P.overflow_flag(x, 0.5) is False and np.isinf(P.split(x, 1.0)[0][0])
    assert P.overflow_flag(np.zeros(4), 1.0) is False and P.overflow_flag(np.zeros(0), 1.0) is False
    assert P.overflow_flag(np.array([3e38], dtype=np.float32), 4.0)          # the product overflows fp32: not < 65504


def test_planes_ok_is_the_consumers_window():
    assert P.planes_ok(1.0, 2.0 ** 14, 0) and P.planes_ok(0.0, 2.0 ** 14, 0)
    assert not P.planes_ok(1.0, 0.0, 0) and not P.planes_ok(1.0, 2.0 ** 14, 1) and not P.planes_ok(0.0, 2.0 ** 14, 1)
    assert P.planes_ok(0.25, 1.0, 0) and not P.planes_ok(np.nextafter(np.float32(0.25), np.float32(0)), 1.0, 0)
    assert P.planes_ok(np.nextafter(P.F16_MAX, np.float32(0)), 1.0, 0) and not P.planes_ok(65504.0, 1.0, 0)
    assert P.planes_ok(1e-30, 2.0 ** 60, 0) and not P.planes_ok(1e-30, 2.0 ** 59, 0)          # at the upper clamp the fallback could do no better
    # the exact scale passes for every maximum below its lower clamp (2^75); a tensor that shrank by 2^17 since its scale was
    # derived does not, unless the scale stands at the upper clamp
    for a in (1e-30, 1e-6, 1.0, 777.0, 1e20):
        assert P.planes_ok(a, P.exact_scale(a), 0)
        assert P.planes_ok(a * 2.0 ** -17, P.exact_scale(a), 0) is (a == 1e-30)
    assert not P.planes_ok(1e30, P.exact_scale(1e30), 0)          # beyond the clamp: the planes overflow, the consumer refuses them


@pytest.mark.parametrize("R,C,ld2", [(1, 32, None), (3, 64, 192), (5, 96, None), (40, 32, 128)])
def test_pack_layout_and_round_trip(R, C, ld2):
    rng = np.random.RandomState(R + C)
    x = (rng.standard_normal((R, C)) * 3.0).astype(np.float32)
    s = P.exact_scale(P.amax_of(x))
    img, written = P.pack(x, s, ld2)
    L = 2 * C if ld2 is None else ld2
    hi, lo = P.split(x, s)
    assert img.dtype == np.uint16 and img.shape == (R * L,) and written.sum() == 2 * R * C
    for r, c in [(0, 0), (R - 1, C - 1), (R // 2, 31), (R // 2, C // 2)]:          # the header's formula, element by element
        assert img[r * L + (c // 32) * 64 + c % 32] == hi[r, c].view(np.uint16) and img[r * L + (c // 32) * 64 + c % 32 + 32] == lo[r, c].view(np.uint16)
    assert (img[~written] == P.CANARY).all()
    h2, l2 = P.unpack(img, R, C, ld2)
    assert np.array_equal(h2.view(np.uint16), hi.view(np.uint16)) and np.array_equal(l2.view(np.uint16), lo.view(np.uint16))
    back = (h2.astype(np.float64) + l2.astype(np.float64)) / float(s)
    assert np.abs(back - x).max() <= 2.0 ** -22 * np.abs(x).max()


@pytest.mark.parametrize("R,C,ld2", [(32, 5, None), (64, 40, 192)])
def test_pack_transposed_puts_column_c_in_plane_row_c(R, C, ld2):
    rng = np.random.RandomState(R + C)
    x = rng.standard_normal((R, C)).astype(np.float32)
    s = P.exact_scale(P.amax_of(x))
    img, written = P.pack_transposed(x, s, ld2)
    L = 2 * R if ld2 is None else ld2
    hi, lo = P.split(x, s)
    assert img.shape == (C * L,) and written.sum() == 2 * R * C and (img[~written] == P.CANARY).all()
    for r, c in [(0, 0), (R - 1, C - 1), (31, 2), (R // 2, C // 2)]:
        assert img[c * L + (r // 32) * 64 + r % 32] == hi[r, c].view(np.uint16) and img[c * L + (r // 32) * 64 + r % 32 + 32] == lo[r, c].view(np.uint16)
    hT, lT = P.unpack(img, C, R, ld2)
    assert np.array_equal(hT.view(np.uint16), hi.T.view(np.uint16)) and np.array_equal(lT.view(np.uint16), lo.T.view(np.uint16))


def test_numpy_and_torch_round_alike():
    """numpy's astype(float16) and torch's .half(): the same bits on the shared input, subnormal lo terms included."""
    x = P.log_input()
    s = P.exact_scale(P.amax_of(x))
    hi, lo = P.split(x, s)
    p = torch.from_numpy(x.copy()) * float(s)
    th = p.half()
    tl = (p - th.float()).half()
    assert np.array_equal(th.numpy().view(np.uint16), hi.view(np.uint16))
    assert np.array_equal(tl.numpy().view(np.uint16), lo.view(np.uint16))
    edge = np.array([65504.0, 65512.0, 65519.996, 65520.0, -0.0, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -14 - 2.0 ** -26], dtype=np.float32)
    with np.errstate(over="ignore"):
        assert np.array_equal(torch.from_numpy(edge).half().numpy().view(np.uint16), edge.astype(np.float16).view(np.uint16))


def test_entry_points_validate_arguments_without_a_gpu():
    """segmm_split_p32, segmm_split_p32_transpose and segmm_wsplit_p32 refuse malformed shapes before any GPU call, with a message
    naming the function."""
    from segmminterest_amd import hipabi
    L = hipabi.lib()
    buf = (ctypes.c_float * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15

    def split(rows=4, cols=64, ld=64, ld2=128, mode=0, x=p, planes=p, hdr=p):
        return L.segmm_split_p32(x, rows, cols, ld, planes, ld2, hdr, mode, None)
    for kw in (dict(cols=48), dict(cols=0), dict(ld2=160), dict(ld2=64), dict(ld=60), dict(ld=62, cols=64), dict(mode=2), dict(mode=-1),
               dict(x=None), dict(planes=None), dict(hdr=None), dict(x=p + 4), dict(planes=p + 2), dict(rows=-1)):
        assert split(**kw) != 0 and b"split_p32" in L.segmm_last_error() and b"transpose" not in L.segmm_last_error(), kw
    assert split(rows=0) == 0          # nothing to do: launches nothing

    def splitT(R=64, C=40, ld=40, ld2=128, x=p, planes=p, hdr=p):
        return L.segmm_split_p32_transpose(x, R, C, ld, planes, ld2, hdr, None)
    for kw in (dict(R=48), dict(R=0), dict(ld2=64), dict(ld2=160), dict(ld=32), dict(C=0), dict(x=None), dict(planes=None), dict(hdr=None), dict(planes=p + 2)):
        assert splitT(**kw) != 0 and b"split_p32_transpose" in L.segmm_last_error(), kw

    def wsplit(n_mats=1, n_tiles=1, flat=p, desc=p, hdr=p, wpl=p, wTpl=p):
        return L.segmm_wsplit_p32(flat, desc, n_mats, n_tiles, hdr, wpl, wTpl, None)
    for kw in (dict(n_mats=0), dict(n_mats=-3), dict(n_tiles=0), dict(flat=None), dict(desc=None), dict(hdr=None), dict(wpl=None), dict(flat=p + 4)):
        assert wsplit(**kw) != 0 and b"wsplit_p32" in L.segmm_last_error(), kw
