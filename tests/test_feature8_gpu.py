"""Input features stored in 8 bits -- OCP e4m3fn, OCP e5m2, int8: the resident feature table (segmm_gather_l1_b), host-fed batches
(segmm_l1norm_b) and the loader's row quantiser (segmm_quantize_rows).

Every code of the three formats is an exact fp32 value (tests/feature8_ref.py holds the tables, from torch's CPU conversion), and the
8-bit kernels are DEFINED as "the fp32 kernel applied to the exactly widened values".  So nothing here has a tolerance of its own:
every output of an 8-bit launch -- rows, masks, reciprocal scales, planes, site headers, partial maxima, and through them losses and
parameters of whole training steps -- is compared BIT FOR BIT with the fp32 launch on the CPU-widened tensor; the quantiser's codes and
scales are compared byte for byte with the numpy statement of its rule; the one bound used is rowops_ref.l1_bounds against float64,
unchanged.  Output buffers are pre-filled with a recorded pattern and every element outside the documented output region is compared
afterwards (the launch helpers are those of tests/test_feature_dtype_gpu.py)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import feature8_ref as Q
import rowops_ref as R
from test_feature_dtype_gpu import (G_ROWS, N_LINES, _assert_same_tree, _bits, _equal_runs, _gather_run, _host, _index_batches, _knob,
                                    _l1_run, _pattern, _same, _steps, _trainer)

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
FMTS = list(Q.DTYPES)
IDS = [Q.NAMES[d] for d in FMTS]
# one dword per row | a 12-byte row pitch | a 4-column tail behind V = 1 | V = 3 | V = 6 | the loop form
DS = [4, 12, 260, 768, 1536, 2052]


def _abi():
    from segmminterest_amd import hipabi
    hipabi.lib()
    # a binding without the 8-bit entry points would hand an 8-bit buffer to a wider kernel (more bytes read than the buffer holds): stop
    # before any launch
    for name in ("segmm_l1norm_b", "segmm_gather_l1_b", "segmm_quantize_rows"):
        assert name in hipabi.SIGNATURES, "no 8-bit feature kernels in this library"
    return hipabi


def _finite_codes(dtype):
    return np.nonzero(torch.isfinite(Q.widen_table(dtype)).numpy())[0].astype(np.uint8)


def _special_codes(dtype):
    """(minus zero -- int8: the most negative code --, largest finite, its negative, the subnormal codes -- int8: +-1 .. +-3)"""
    if dtype == Q.E4M3:
        return 0x80, 0x7E, 0xFE, [c | s for c in range(1, 8) for s in (0, 0x80)]
    if dtype == Q.E5M2:
        return 0x80, 0x7B, 0xFB, [c | s for c in range(1, 4) for s in (0, 0x80)]
    return 0x80, 0x7F, 0x81, [1, 0xFF, 2, 0xFE, 3, 0xFD]


def _rows8(rows, D, seed, dtype):
    """uint8 codes [rows, D] as a tensor of ``dtype``: random finite codes; row 0 walks through ALL finite codes of the format, repeated
    (from a row-dependent start, so that D = 4 tables see many of them); from 5 rows on, rows 1 .. 4 are: all zeros | -0.0 codes | the
    largest finite code with alternating sign | the subnormal codes.  No NaN or inf code; every row sum is finite in fp32."""
    fin = _finite_codes(dtype)
    g = np.random.default_rng(300 + seed)
    c = fin[g.integers(0, len(fin), (rows, D))]
    c[0] = fin[(np.arange(D) + 7 * seed) % len(fin)]
    if rows >= 5:
        neg0, top, ntop, sub = _special_codes(dtype)
        c[1] = 0
        c[2] = neg0
        c[3] = np.where(np.arange(D) % 2 == 0, top, ntop)
        c[4] = np.asarray(sub, np.uint8)[np.arange(D) % len(sub)]
    t = Q.from_codes(c, dtype)
    w = Q.widen(t)
    assert torch.isfinite(w).all() and torch.isfinite(w.abs().sum(1)).all()
    return t


# ------------------------------------------------------------------ 0. what a code means
@pytest.mark.parametrize("dtype", FMTS, ids=IDS)
def test_all_256_codes_widen_to_the_reference_values(dtype):
    """normalize = 0: the gathered row IS the widened row.  Every code, NaN and inf codes included, in every byte position of a dword."""
    H = _abi()
    codes = np.arange(256, dtype=np.uint8)
    table = Q.from_codes(np.stack([np.roll(codes, k) for k in range(4)]), dtype)          # [4, 256]: each code at columns = 0, 1, 2, 3 mod 4
    want = Q.widen(table)
    idx = torch.arange(4, device=DEV)
    out, mask = H.gather_l1(table.to(DEV), idx, normalize=False)
    got = _host(out)
    assert bool(mask.all()) and got.dtype == torch.float32
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan)
    assert torch.equal(_bits(got)[~nan], _bits(want)[~nan])          # signed zeros, subnormal codes, e5m2's infinities: the bits
    # the same through the loop form's load (D = 2304 > 2048: nine times the 256 codes)
    wide = Q.from_codes(np.tile(np.roll(codes, 1), (2, 9)), dtype)
    got = _host(H.gather_l1(wide.to(DEV), idx[:2], normalize=False)[0])
    want = Q.widen(wide)
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan) and torch.equal(_bits(got)[~nan], _bits(want)[~nan])


# ------------------------------------------------------------------ 1. gather
def _gather_idx(D):
    idx = np.random.default_rng(D).integers(0, N_LINES, G_ROWS).astype(np.int64)
    idx[[0, 1, 2, 3, 4, 5, 6, 7, 8]] = [-1, N_LINES, 10 ** 9, 0, N_LINES - 1, 1, 2, 3, 4]
    return idx


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("dtype", FMTS, ids=IDS)
@pytest.mark.parametrize("D", DS)
def test_gather_8bit_equals_fp32_gather_of_the_widened_table(D, dtype, normalize):
    H = _abi()
    t8 = _rows8(N_LINES, D, D, dtype)
    wide = Q.widen(t8)
    idx = _gather_idx(D)
    ok = (idx >= 0) & (idx < N_LINES)
    idx_d = torch.from_numpy(idx.reshape(3, 7)).to(DEV)
    t8d, wided = t8.to(DEV), wide.to(DEV)
    got, want = _gather_run(H, t8d, idx_d, normalize, D), _gather_run(H, wided, idx_d, normalize, D)
    assert got["out"].dtype == torch.float32
    assert _same(got["out"], want["out"]) and _same(got["mask"], want["mask"])
    assert np.array_equal(got["mask"].numpy(), ok.astype(np.uint8))
    assert not _bits(got["out"][torch.from_numpy(~ok)]).any()          # +0.0 in every padded element
    g = wide.numpy()[idx[ok]]
    o = got["out"].numpy()[ok]
    if not normalize:
        assert np.array_equal(o.view(np.uint32), g.view(np.uint32))          # the widened table rows, signed zeros included
    else:
        _, _, y64 = R.l1_ref(g)
        with np.errstate(all="ignore"):
            r = R.ratio(np.abs(o.astype(np.float64) - y64), R.l1_bounds(g)[2])
        print("gather_l1_b D=%d %s: worst error / l1 bound = %.3g" % (D, Q.NAMES[dtype], r))
        assert r <= 1.0
    a8, a32 = _gather_run(H, t8d, idx_d, normalize, D, amax=True), _gather_run(H, wided, idx_d, normalize, D, amax=True)
    assert _same(a8["amax"], a32["amax"]) and _same(a8["out"], want["out"]) and float(a32["amax"].max()) > 0
    if D % 32 == 0 and normalize:
        p8, p32 = _gather_run(H, t8d, idx_d, normalize, D, planes=True), _gather_run(H, wided, idx_d, normalize, D, planes=True)
        assert _same(p8["planes"], p32["planes"]) and _same(p8["hdr"], p32["hdr"]) and _same(p8["out"], want["out"])
        assert float(p32["hdr"][0]) == 2.0 ** 13 and bool(p32["planes"].any())


def _same_but_nan(a, b):
    """the NaN pattern of ``a`` is that of ``b``, and the bits agree everywhere else"""
    na, nb = torch.isnan(a), torch.isnan(b)
    return a.shape == b.shape and torch.equal(na, nb) and torch.equal(_bits(a)[~na], _bits(b)[~nb])


@pytest.mark.parametrize("dtype", [Q.E4M3, Q.E5M2], ids=["e4m3", "e5m2"])
@pytest.mark.parametrize("D", [12, 768, 2052])
def test_a_row_with_a_nan_code_behaves_as_in_the_fp32_kernels(D, dtype):
    H = _abi()
    t8 = _rows8(N_LINES, D, D + 1, dtype)
    c = Q.codes_of(t8).clone()
    c[6, D // 2 + 1] = 0x7F if dtype == Q.E4M3 else 0xFE          # a NaN code of either sign
    t8 = Q.from_codes(c, dtype)
    wide = Q.widen(t8)
    assert int(torch.isnan(wide).sum()) == 1
    idx = _gather_idx(D)
    idx[9] = 6
    idx_d = torch.from_numpy(idx.reshape(3, 7)).to(DEV)
    for normalize in (True, False):
        got, want = _gather_run(H, t8.to(DEV), idx_d, normalize, D, amax=True), _gather_run(H, wide.to(DEV), idx_d, normalize, D, amax=True)
        assert _same_but_nan(got["out"], want["out"]) and _same(got["mask"], want["mask"]) and _same_but_nan(got["amax"], want["amax"])
        assert bool(torch.isnan(want["out"][9]).all() if normalize else torch.isnan(want["out"][9]).sum() == 1)
    x8, xw = t8[:7].contiguous().to(DEV), wide[:7].contiguous().to(DEV)
    got, want = _l1_run(H, x8, 7, D, True, True), _l1_run(H, xw, 7, D, True, True)
    assert _same_but_nan(got["y"], want["y"]) and _same_but_nan(got["inv"], want["inv"])
    assert bool(torch.isnan(want["inv"][6])) and int(torch.isnan(want["inv"]).sum()) == 1


# ------------------------------------------------------------------ 2. L1 normalisation of an 8-bit x
@pytest.mark.parametrize("rows", [1, 5, 21])
@pytest.mark.parametrize("dtype", FMTS, ids=IDS)
@pytest.mark.parametrize("D", DS)
def test_l1norm_8bit_equals_fp32_l1norm_of_the_widened_rows(D, dtype, rows):
    H = _abi()
    x8h = _rows8(rows, D, D + rows, dtype)
    x8, wide = x8h.to(DEV), Q.widen(x8h).to(DEV)
    modes = [(True, True, False), (True, False, False), (False, True, False)]
    if D % 32 == 0:
        modes += [(False, False, True), (True, True, True)]          # planes only (y null), and planes next to y
    for with_y, with_inv, planes in modes:
        got = _l1_run(H, x8, rows, D, with_y, with_inv, planes)
        for reg in (1, 0):
            with _knob(H, "L1NORM_REG", reg):
                want = _l1_run(H, wide, rows, D, with_y, with_inv, planes)
            what = "D=%d rows=%d %s y=%d inv=%d planes=%d reg=%d" % (D, rows, Q.NAMES[dtype], with_y, with_inv, planes, reg)
            assert _same(got["y"], want["y"]) and _same(got["inv"], want["inv"]), what
            if planes:
                assert _same(got["planes"], want["planes"]) and _same(got["hdr"], want["hdr"]), what
                assert bool(want["planes"].any()) and float(want["hdr"][0]) == 2.0 ** 14, what
    if rows >= 5:          # the special rows did what they are there for: the zero row gives 0 / 1e-6, the alternating row +-1 / D
        y = _l1_run(H, x8, rows, D, True, True)
        yr = y["y"].reshape(rows, D)
        assert not yr[1].any() and float(y["inv"][1]) == float(np.float32(1.0) / np.float32(1e-6))
        if dtype != Q.I8:
            assert not yr[2].any() and bool((_bits(yr[2]) == -2 ** 31).all())          # -0.0 / 1e-6 = -0.0
        assert torch.equal(torch.sign(yr[3]), torch.where(torch.arange(D) % 2 == 0, 1.0, -1.0))


# ------------------------------------------------------------------ 3. the row quantiser
def _quant_rows(D, seed):
    """float32 [24, D]: Gaussian rows scaled by 2^-90 .. 2^90; then a zero row, a row under 2^-100, a row with an inf, a row whose
    FIRST element is NaN, two rows whose absmax is a power of two (2^0, 2^-37), two one ulp under a power of two, a row of +-one value
    with signed zeros, and a row on the floor 2^-100 itself."""
    g = np.random.default_rng(500 + seed)
    x = np.zeros((24, D), F)
    for k, e in enumerate(np.linspace(-90, 90, 14)):
        x[k] = (g.standard_normal(D) * 2.0 ** e).astype(F)
    x[14] = 0
    x[15] = (g.uniform(-1, 1, D) * 2.0 ** -101).astype(F)
    x[16] = g.standard_normal(D).astype(F)
    x[16, D - 1] = -np.inf
    x[17] = g.standard_normal(D).astype(F)
    x[17, 0] = np.nan
    for r, top in ((18, F(1.0)), (19, F(2.0 ** -37)), (20, np.nextafter(F(4.0), F(0))), (21, np.nextafter(F(2.0 ** 60), F(0)))):
        x[r] = (g.uniform(-1, 1, D) * top).astype(F)
        x[r, D // 2] = -top
    x[22] = np.where(np.arange(D) % 2 == 0, F(0.75), F(-0.75))
    x[22, 1::4] = -0.0
    x[22, 2::4] = 0.0
    x[22, 0] = 0.75
    x[23] = F(2.0 ** -100)
    return x


@pytest.mark.parametrize("dtype", FMTS, ids=IDS)
@pytest.mark.parametrize("D", DS)
def test_quantize_rows_gives_the_reference_bytes(D, dtype):
    H = _abi()
    x = _quant_rows(D, D)
    rows = x.shape[0]
    q_ref, s_ref = Q.quantize_rows(x, dtype)
    assert not q_ref[14:18].any() and not s_ref[14:18].any() and (s_ref[:14] > 0).all() and (s_ref[18:] > 0).all()
    n = rows * D
    q0 = torch.from_numpy(np.random.default_rng(9).integers(0, 256, n + 3 * D + 8).astype(np.uint8))
    s0 = _pattern(rows + 5, 4)
    qd, sd = q0.to(DEV), s0.to(DEV)
    xd = torch.from_numpy(x).to(DEV)
    out = H.quantize_rows(xd, dtype, out=qd[:n].view(dtype).view(rows, D), scale_out=sd[:rows])
    assert out.dtype == dtype and out.data_ptr() == qd.data_ptr()
    q, s = _host(qd), _host(sd)
    assert _same(q[n:], q0[n:]) and _same(s[rows:], s0[rows:])          # nothing outside the output region was written
    got_q, got_s = q[:n].reshape(rows, D).numpy(), s[:rows].numpy()
    bad = np.nonzero((got_q != q_ref).any(axis=1))[0]
    assert bad.size == 0, "rows %s differ: first %s vs %s" % (bad.tolist(), got_q[bad[0]][:8], q_ref[bad[0]][:8])
    assert np.array_equal(got_s.view(np.uint32), s_ref.view(np.uint32))
    # without scale_out, into a fresh tensor: the same codes
    q2 = H.quantize_rows(xd, dtype)
    assert q2.dtype == dtype and tuple(q2.shape) == (rows, D) and np.array_equal(_host(Q.codes_of(q2)).numpy(), q_ref)


# ------------------------------------------------------------------ 4. refusals
def test_refusals_launch_nothing():
    H = _abi()
    D, n = 8, 5
    idx = torch.zeros((3,), dtype=torch.int64, device=DEV)
    o0 = _pattern(3 * D + 16, 5)
    od = o0.to(DEV)
    base = torch.randint(-100, 100, (n, D), device=DEV)
    wide2 = torch.randint(-100, 100, (n, 2 * D), device=DEV).to(torch.int8)
    strided = wide2[:, ::2]
    assert not strided.is_contiguous()
    for bad, word in ((base.to(torch.uint8), "uint8"), (base.to(torch.int16), "int16"), (base.double(), "float64"), (strided, "int8")):
        with pytest.raises(RuntimeError, match=word):
            H.gather_l1(bad, idx, out=od)
        with pytest.raises(RuntimeError, match=word):
            H.l1norm(bad, od[:n * D].view(n, D))
    for dtype in FMTS:
        six = torch.zeros(n, 6).to(dtype).to(DEV)          # (converted on the host: the device only ever copies 8-bit tensors)
        with pytest.raises(RuntimeError, match="D=6"):
            H.gather_l1(six, idx, out=od)
        with pytest.raises(RuntimeError, match="D=6"):
            H.l1norm(six, od[:n * 6].view(n, 6))
        with pytest.raises(RuntimeError, match="D=6"):
            H.quantize_rows(torch.zeros(n, 6, device=DEV), dtype)
        # outputs stay float32, the quantiser's input is float32
        with pytest.raises(RuntimeError, match="float32"):
            H.l1norm(torch.zeros(n, D).to(dtype).to(DEV), torch.empty(n, D, dtype=torch.float16, device=DEV))
        with pytest.raises(RuntimeError, match="float32"):
            H.quantize_rows(base.half(), dtype)
    with pytest.raises(RuntimeError, match="uint8"):
        H.quantize_rows(base.float(), torch.uint8)
    # through the raw C entry points: an error return with a message, never a launch
    L = H.lib()
    t8 = base.to(torch.int8)
    q8 = torch.zeros(n * D + 8, dtype=torch.uint8, device=DEV)
    xf = base.float()
    st = H._stream()
    for elem in (0, 1, 2, 6):
        rc = L.segmm_gather_l1_b(t8.data_ptr(), elem, n, D, idx.data_ptr(), 3, 1, od.data_ptr(), None, None, None, 0, None, None, st)
        assert rc != 0 and b"elem" in L.segmm_last_error()
        rc = L.segmm_l1norm_b(t8.data_ptr(), elem, od.data_ptr(), None, 3, D, None, None, 0, None, None, st)
        assert rc != 0 and b"elem" in L.segmm_last_error()
        rc = L.segmm_quantize_rows(xf.data_ptr(), n, D, elem, q8.data_ptr(), None, st)
        assert rc != 0 and b"elem" in L.segmm_last_error()
    for elem in (3, 4, 5):
        # D = 6, and a base that is 2 bytes off a dword
        rc = L.segmm_gather_l1_b(t8.data_ptr(), elem, n, 6, idx.data_ptr(), 3, 1, od.data_ptr(), None, None, None, 0, None, None, st)
        assert rc != 0 and b"D=6" in L.segmm_last_error()
        rc = L.segmm_l1norm_b(t8.data_ptr(), elem, od.data_ptr(), None, 3, 6, None, None, 0, None, None, st)
        assert rc != 0 and b"D=6" in L.segmm_last_error()
        rc = L.segmm_gather_l1_b(t8.data_ptr() + 2, elem, n - 1, D, idx.data_ptr(), 3, 1, od.data_ptr(), None, None, None, 0, None, None, st)
        assert rc != 0 and b"alignment" in L.segmm_last_error()
        rc = L.segmm_l1norm_b(t8.data_ptr() + 2, elem, od.data_ptr(), None, 3, D, None, None, 0, None, None, st)
        assert rc != 0 and b"alignment" in L.segmm_last_error()
        rc = L.segmm_quantize_rows(xf.data_ptr(), n - 1, D, elem, q8.data_ptr() + 2, None, st)
        assert rc != 0 and b"alignment" in L.segmm_last_error()
    # the 16-bit entry points keep refusing the 8-bit codes
    rc = L.segmm_gather_l1_h(t8.data_ptr(), 3, n // 2, D, idx.data_ptr(), 3, 1, od.data_ptr(), None, None, None, 0, None, None, st)
    assert rc != 0 and b"elem" in L.segmm_last_error()
    assert _same(_host(od), o0) and not _host(q8).any()          # nothing was launched: the buffers still hold their patterns


# ------------------------------------------------------------------ 5. whole model, resident table
def _dataset8():
    from test_assemble_gpu import _dataset as ds
    table, feats = ds()
    return table, feats.float().numpy()


def _table8(feats, dtype):
    """the float32 features quantised by the reference rule: every trainer below sees these codes, or their widened values"""
    return Q.from_codes(Q.quantize_rows(feats, dtype)[0], dtype)


def _wide(t):
    return t.float() if t.dtype in (torch.float16, torch.bfloat16) else Q.widen(t)


CASES = {          # photo table, user table (None: the same), d_model, how, trainer keywords
    "eager_e4m3": (Q.E4M3, None, 32, "eager", {"dropout": False}),
    "eager_e5m2": (Q.E5M2, None, 32, "eager", {"dropout": False}),
    "d48_fp32_consumers_int8": (Q.I8, None, 48, "eager", {"dropout": False}),
    "dropout_device_state_e5m2": (Q.E5M2, None, 32, "eager", {"dropout": True, "device_state": True}),
    "prefetch_int8": (Q.I8, None, 32, "prefetch", {"dropout": False}),
    "recorded_e4m3": (Q.E4M3, None, 32, "recorded", {"dropout": False, "device_state": True}),
    "recorded_int8": (Q.I8, None, 32, "recorded", {"dropout": False, "device_state": True}),
    "photo_e4m3_user_int8": (Q.E4M3, Q.I8, 32, "eager", {"dropout": False}),
    "photo_int8_user_float16_recorded": (Q.I8, torch.float16, 32, "recorded", {"dropout": False, "device_state": True}),
}


@pytest.mark.parametrize("case", list(CASES))
def test_training_on_an_8bit_table_equals_training_on_the_widened_table(case):
    _abi()
    _, _, batches = _index_batches()
    _, feats = _dataset8()
    pd, ud, d, how, kw = CASES[case]
    photo = _table8(feats, pd)
    user = None if ud is None else (torch.from_numpy(feats).to(ud) if ud in (torch.float16, torch.bfloat16) else _table8(feats, ud))
    a = _steps(photo, batches, d=d, how=how, user_feats=user, **kw)
    b = _steps(_wide(photo), batches, d=d, how=how, user_feats=None if user is None else _wide(user), **kw)
    _equal_runs(a, b)
    assert not torch.equal(a[0][0], a[0][-1])          # the steps moved the model


def test_fit_recorded_and_eager_on_an_8bit_table_equal_the_widened_table():
    from test_assemble_gpu import B_E, LT_E, S_E
    from segmminterest_amd import feature_store as FS
    _abi()
    table, feats = _dataset8()
    dev = table.to(DEV)
    valid = list(FS.DeviceBatches(dev, 16, S_E, LT_E, shuffle=False)(0))
    t8 = _table8(feats, Q.E5M2)
    ends = {}
    for name, f in (("e5m2", t8), ("wide", Q.widen(t8))):
        for mode in ("eager", "recorded"):
            model, tr = _trainer(f, device_state=True)
            db = FS.DeviceBatches(dev, B_E, S_E, LT_E, seed=3, drop_last=True)
            hist = tr.fit(db, valid, epochs=2, valid_step=100, permutation=0, recorded=(mode == "recorded"))
            assert hist["global_step"] == 8
            if mode == "recorded":
                assert tr.__dict__.get("_recorded") is not None
            ends[name, mode] = model._store.flat.detach().clone()
    ref = ends["wide", "eager"]
    assert torch.isfinite(ref).all() and all(torch.equal(v, ref) for v in ends.values())


# ------------------------------------------------------------------ 6. whole model, host-fed 8-bit batches
def _feature_batches8(dtype, wide, n=4):
    """``dtype`` batches (``wide``: their widened float32 values instead)"""
    from test_assemble_gpu import B_E, D_E, LT_E, S_E
    from segmminterest_amd.synth import make_batch
    out = []
    for i in range(n):
        b = make_batch(B_E, S_E, LT_E, D_E, n_users=50, n_items=500, seed=40 + i)
        for k in ("user", "photo"):
            x = b[k].float().numpy()
            t = Q.from_codes(Q.quantize_rows(x.reshape(-1, x.shape[-1]), dtype)[0].reshape(x.shape), dtype)
            b[k] = Q.widen(t) if wide else t
        out.append({k: v.to(DEV) for k, v in b.items()})
    return out


@pytest.mark.parametrize("how,dtype,kw", [("eager", Q.I8, {}), ("eager", Q.E4M3, {}), ("recorded", Q.E5M2, {}), ("recorded", Q.I8, {}),
                                          ("prefetch", Q.E4M3, {}), ("eager", Q.E5M2, {"micro_batch": 3})],
                         ids=["eager_int8", "eager_e4m3", "recorded_e5m2", "recorded_int8", "prefetch_e4m3", "micro_batch_e5m2"])
def test_host_fed_8bit_batches_equal_the_widened_batches(how, dtype, kw):
    _abi()
    kw = dict({"dropout": False, "device_state": how == "recorded"}, **kw)
    b8, b32 = _feature_batches8(dtype, False), _feature_batches8(dtype, True)
    assert b8[0]["user"].dtype == dtype and b32[0]["photo"].dtype == torch.float32
    assert b8[0]["photo"].element_size() == 1 and torch.equal(Q.widen(b8[0]["photo"]), b32[0]["photo"])
    if "micro_batch" in kw:
        assert b8[0]["user"].shape[0] > kw["micro_batch"]
    _equal_runs(_steps(None, b8, how=how, **kw), _steps(None, b32, how=how, **kw))


def test_a_recorded_step_refuses_a_batch_of_another_feature_dtype():
    _abi()
    sets = {"int8": _feature_batches8(Q.I8, False, 2), "e4m3": _feature_batches8(Q.E4M3, False, 2), "f32": _feature_batches8(Q.I8, True, 2)}
    sets["f16"] = [dict(b, user=b["user"].half(), photo=b["photo"].half()) for b in sets["f32"]]
    for rec, others in (("int8", ("e4m3", "f32", "f16")), ("f32", ("int8",)), ("e4m3", ("int8",))):
        model, tr = _trainer(None, dropout=False, device_state=True)
        tr.record(sets[rec][0], warmup=1)
        tr.run_recorded(sets[rec][1])          # the recorded dtype replays onto another batch object
        flat = model._store.flat.detach().clone()
        for other in others:
            with pytest.raises(RuntimeError, match="run_recorded"):
                tr.run_recorded(sets[other][1])
        torch.cuda.synchronize()
        assert torch.equal(model._store.flat, flat)          # the refused calls enqueued nothing
    # record() itself: one feature dtype per batch, and uint8 is no feature dtype
    model, tr = _trainer(None, dropout=False, device_state=True)
    with pytest.raises(RuntimeError, match="one dtype"):
        tr.record(dict(sets["int8"][0], photo=sets["e4m3"][0]["photo"]), warmup=1)
    with pytest.raises(RuntimeError, match="uint8"):
        tr.record(dict(sets["int8"][0], user=sets["int8"][0]["user"].view(torch.uint8), photo=sets["int8"][0]["photo"].view(torch.uint8)), warmup=1)


# ------------------------------------------------------------------ 7. evaluation
@pytest.mark.parametrize("dtype", [Q.E4M3, Q.I8], ids=["e4m3", "int8"])
def test_validation_and_test_metrics_equal_on_the_8bit_and_the_widened_table(dtype):
    from test_assemble_gpu import LT_E, S_E
    from segmminterest_amd import feature_store as FS
    _abi()
    table, feats = _dataset8()
    valid = list(FS.DeviceBatches(table.to(DEV), 16, S_E, LT_E, shuffle=False)(0))
    evals = ["JaccardSim", "LeaveMSE", "LeaveCTR", "LeaveCTR_view", "TOP_K", "ProbAUC"]
    t8 = _table8(feats, dtype)
    res = []
    for f in (t8, Q.widen(t8)):
        _, tr = _trainer(f)
        res.append((tr.valid_model(valid, permutation=0), tr.test_model(valid, evals, top_k_permutation=0)["final"],
                    tr.test_model(valid, evals, top_k_permutation=0, device_metrics=True)["final"]))
    _assert_same_tree(res[0], res[1])
    assert len(res[0][0]) > 0 and all(np.isfinite(v) for v in res[0][0].values())


# ------------------------------------------------------------------ 8. from_memmap
def test_from_memmap_quantises_in_chunks(tmp_path):
    from segmminterest_amd.feature_store import ResidentFeatureTable
    _abi()
    a = (np.random.default_rng(5).standard_normal((37, 64)) * np.exp(np.linspace(-8, 8, 37))[:, None]).astype(F)
    a[20] = 0
    path = str(tmp_path / "features.bin")
    a.tofile(path)
    for dtype in FMTS:
        t = ResidentFeatureTable.from_memmap(path, 37, 64, dtype=dtype, device=DEV, chunk_rows=16)          # 16 + 16 + 5 lines
        assert t.tables["photo"].dtype == dtype and t.tables["user"] is t.tables["photo"] and t.normalize
        assert np.array_equal(_host(Q.codes_of(t.tables["photo"])).numpy(), Q.quantize_rows(a, dtype)[0])
        whole = ResidentFeatureTable.from_memmap(path, 37, 64, dtype=dtype, device=DEV)
        assert _same(_host(Q.codes_of(whole.tables["photo"])), _host(Q.codes_of(t.tables["photo"])))
        idx = torch.tensor([[0, 36, -1, 20]], device=DEV)
        out, mask = t.gather("photo", idx)
        assert out.dtype == torch.float32 and mask.tolist() == [[True, True, False, True]] and not _host(out)[0, 3].any()
        with pytest.raises(RuntimeError, match="normalize=False"):
            ResidentFeatureTable.from_memmap(path, 37, 64, dtype=dtype, device=DEV, normalize=False)
        # a table the user quantised themself -- codes that ARE the values -- runs with either setting
        own = ResidentFeatureTable(t.tables["photo"], normalize=False)
        raw, _ = own.gather("photo", idx)
        assert _same(_host(raw)[0, :2], Q.widen(_host(t.tables["photo"]))[[0, 36]])
    # float32 and 16-bit loads are what they were
    t16 = ResidentFeatureTable.from_memmap(path, 37, 64, dtype=torch.float16, device=DEV, chunk_rows=16)
    assert _same(_host(t16.tables["photo"]), torch.from_numpy(a).half())
    tb = ResidentFeatureTable.from_memmap(path, 37, 64, dtype=torch.bfloat16, device=DEV, chunk_rows=16)
    assert _same(_host(tb.tables["photo"]), torch.from_numpy(a).bfloat16())
    t32 = ResidentFeatureTable.from_memmap(path, 37, 64, device=DEV, chunk_rows=16)
    assert t32.tables["photo"].dtype == torch.float32 and _same(_host(t32.tables["photo"]), torch.from_numpy(a))
    a[33, 7] = np.inf          # the first line with a non-finite value is named
    a[35, 1] = np.nan
    a.tofile(path)
    for dtype in FMTS:
        with pytest.raises(ValueError, match=r"line 33\b"):
            ResidentFeatureTable.from_memmap(path, 37, 64, dtype=dtype, device=DEV, chunk_rows=16)
    with pytest.raises(RuntimeError, match="uint8"):
        ResidentFeatureTable(torch.zeros(4, 8, dtype=torch.uint8, device=DEV))
