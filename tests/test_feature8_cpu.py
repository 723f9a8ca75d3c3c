"""8-bit input features (OCP e4m3fn, OCP e5m2, int8) as the host sees them: what the 256 codes of each format mean
(tests/feature8_ref.py), the additive C ABI (segmm_gather_l1_b, segmm_l1norm_b, segmm_quantize_rows; SEGMM_ELEM_E4M3 / _E5M2 / _I8) as
the binding sees it, a recorded command's round trip, the refusals that happen before a device is touched, and the row quantiser's rule:
its error in scaled units is bounded by the formats alone.  No GPU."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import feature8_ref as Q
from helpers import ROOT

_spec = importlib.util.spec_from_file_location("gen_cmd_dispatch", os.path.join(ROOT, "tools", "gen_cmd_dispatch.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

F = np.float32
NEW = ("segmm_gather_l1_b", "segmm_l1norm_b")
TWIN = {"segmm_gather_l1_b": "segmm_gather_l1", "segmm_l1norm_b": "segmm_l1norm"}


def _header():
    return open(gen.HDR).read()


# ------------------------------------------------------------------ 1. the codes
@pytest.mark.parametrize("dtype,n_nan,n_inf", [(Q.E4M3, 2, 0), (Q.E5M2, 6, 2), (Q.I8, 0, 0)], ids=["e4m3", "e5m2", "int8"])
def test_every_code_is_an_exact_fp16_and_fp32_value(dtype, n_nan, n_inf):
    w = Q.widen_table(dtype)
    assert w.dtype == torch.float32 and w.shape == (256,)
    assert int(torch.isnan(w).sum()) == n_nan and int(torch.isinf(w).sum()) == n_inf
    fin = torch.isfinite(w)
    assert torch.equal(w[fin].half().float(), w[fin]) and torch.equal(w[fin].double().float(), w[fin])          # exact in fp16, hence in fp32
    assert len(set(w[fin].tolist())) == int(fin.sum()) - (0 if dtype == Q.I8 else 1)          # distinct values, +0 and -0 aside
    if dtype == Q.I8:
        assert w.tolist() == [float(c if c < 128 else c - 256) for c in range(256)]
    else:
        # the formula of the format, code by code: (-1)^s 2^(e-bias) (1 + m / 2^M), subnormals 2^(1-bias) m / 2^M
        EB, M, _ = Q.FP8[dtype]
        for c in range(256):
            s, e, m = c >> 7, (c >> M) & ((1 << (7 - M)) - 1), c & ((1 << M) - 1)
            val = (2.0 ** (1 - EB) * m / 2 ** M) if e == 0 else 2.0 ** (e - EB) * (1 + m / 2 ** M)
            if torch.isfinite(w[c]):
                assert float(w[c]) == (-val if s else val), c
                assert (np.signbit(float(w[c])) != 0) == bool(s), c
        top = float(w[fin].max())
        assert top == (448.0 if dtype == Q.E4M3 else 57344.0)
    t = Q.from_codes(np.arange(256, dtype=np.uint8), dtype)
    assert t.dtype == dtype and torch.equal(Q.widen(t).nan_to_num(7.0), w.nan_to_num(7.0)) and torch.equal(Q.codes_of(t), torch.arange(256, dtype=torch.uint8))


# ------------------------------------------------------------------ 2. the ABI
def test_the_new_entry_points_are_bound_with_the_headers_types():
    from segmminterest_amd import hipabi as H
    ct = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32}
    protos = dict(gen.prototypes(_header()))
    L = H.lib()
    for name in NEW + ("segmm_quantize_rows",):
        assert name in H.SIGNATURES and name in H.PARAMS and name in protos
        ps = protos[name]
        want = [ctypes.c_void_p if (ty.endswith("*") or ty == "segmm_stream_t") else ct[ty] for ty, _ in ps]
        assert list(getattr(L, name).argtypes) == want == H.SIGNATURES[name]
        assert H.PARAMS[name] == tuple(p for _, p in ps)
        assert name in H.op_ids()          # dispatchable: a recorded step can carry it
    for name in NEW:
        # (const uint8_t* input, int elem, ...) followed by the remaining arguments of the fp32 twin, types and names -- as the _h forms
        ps, twin, h = protos[name], protos[TWIN[name]], protos[name[:-1] + "h"]
        assert ps[0][0] == "const uint8_t*" and ps[1] == ("int", "elem") and ps[0][1] == twin[0][1]
        assert ps[2:] == twin[1:] == h[2:]
        assert TWIN[name] in H.op_ids()
    assert protos["segmm_quantize_rows"] == [("const float*", "x"), ("int64_t", "rows"), ("int", "D"), ("int", "elem"), ("uint8_t*", "q"),
                                             ("float*", "scale_out"), ("segmm_stream_t", "stream")]


def test_abi_version_constants_and_mirrors():
    from segmminterest_amd import _abi, hipabi as H
    k = gen.constants(_header())
    assert H.ABI_VERSION == _abi.ABI_VERSION == k["SEGMM_ABI_VERSION"] == 30 == H.lib().segmm_abi_version()
    assert (k["SEGMM_ELEM_F16"], k["SEGMM_ELEM_BF16"], k["SEGMM_ELEM_E4M3"], k["SEGMM_ELEM_E5M2"], k["SEGMM_ELEM_I8"]) == (1, 2, 3, 4, 5)
    assert (_abi.CONSTANTS["SEGMM_ELEM_E4M3"], _abi.CONSTANTS["SEGMM_ELEM_E5M2"], _abi.CONSTANTS["SEGMM_ELEM_I8"]) == (
        H.ELEM_E4M3, H.ELEM_E5M2, H.ELEM_I8) == (3, 4, 5)
    assert H._ELEM == {torch.float16: 1, torch.bfloat16: 2}          # the 16-bit map is what it was; the 8-bit codes have their own
    assert H._ELEM8 == {torch.float8_e4m3fn: 3, torch.float8_e5m2: 4, torch.int8: 5} == {d: Q.ELEM[d] for d in Q.DTYPES}
    gen.check(_header(), {p: open(p).read() for p in (gen.OUT, gen.OUT_ABI)})          # both generated files are current
    inc = open(gen.OUT).read()
    for name in NEW:
        assert '"%s",' % name in inc and "return %s((const uint8_t*)a[0].p, (int)a[1].i," % name in inc
    assert "return segmm_quantize_rows((const float*)a[0].p, (int64_t)a[1].i, (int)a[2].i, (int)a[3].i, (uint8_t*)a[4].p, (float*)a[5].p, st);" in inc


def test_a_recorded_8bit_command_round_trips():
    from segmminterest_amd import hipabi as H

    def args(name, **kw):
        assert set(kw) <= set(H.PARAMS[name])
        return tuple(kw.get(p, None if ct is H._p else 0) for p, ct in zip(H.PARAMS[name], H.SIGNATURES[name]))

    rec = H.Recorder(111, 222)
    rec.mark(H.PHASE_STEP_BEGIN)
    rec.call("segmm_gather_l1_b", args("segmm_gather_l1_b", table=4096, elem=H.ELEM_E5M2, n_lines=200000, D=768, idx=8192, rows=51200,
                                       normalize=1, out=12288, stream=111))
    rec.call("segmm_l1norm_b", args("segmm_l1norm_b", x=16384, elem=H.ELEM_I8, rows=20480, D=1024, stream=222))
    (ph, a), = rec.finish()
    assert ph.n_cmds == 2 and a[0].op == H.op_ids()["segmm_gather_l1_b"] and a[1].op == H.op_ids()["segmm_l1norm_b"]
    g = lambda p: H.cmd_arg(a[0], "segmm_gather_l1_b", p)
    assert (g("table"), g("elem"), g("n_lines"), g("D"), g("idx"), g("rows"), g("normalize"), g("out"), g("mask")) == (
        4096, 4, 200000, 768, 8192, 51200, 1, 12288, None) and a[0].stream == 0
    n = lambda p: H.cmd_arg(a[1], "segmm_l1norm_b", p)
    assert (n("x"), n("elem"), n("rows"), n("D"), n("y")) == (16384, 5, 20480, 1024, None) and a[1].stream == 1
    # the pointer slots a replay may re-base: table / idx / out of the gather, x of the normalisation -- never elem or D
    names = [[H.PARAMS[nm][k] for ci, k in rec.pslots[0] if ci == c] for c, nm in enumerate(NEW)]
    assert names == [["table", "idx", "out"], ["x"]]


# ------------------------------------------------------------------ 3. host-side refusals
def test_dtype_rules_refuse_on_the_host():
    from segmminterest_amd import hipabi as H
    from segmminterest_amd.feature_store import ResidentFeatureTable
    from segmminterest_amd.trainer import Trainer
    for bad in (torch.zeros(4, 8, dtype=torch.uint8), torch.zeros(4, 8, dtype=torch.int16), torch.zeros(4, 8, dtype=torch.float64),
                torch.zeros(4, 8, dtype=torch.bool)):
        word = str(bad.dtype).replace(".", r"\.")
        with pytest.raises(RuntimeError, match=word + ".*float32.*float16.*bfloat16.*float8_e4m3fn.*float8_e5m2.*int8"):
            H._feat(bad, "x")
        with pytest.raises(RuntimeError, match="float32.*float16.*bfloat16.*float8_e4m3fn.*float8_e5m2.*int8"):
            ResidentFeatureTable(bad)
    assert [H._feat(torch.zeros(2, 4).to(d), "x") for d in Q.DTYPES] == [3, 4, 5]
    assert [H._feat(torch.zeros(2, 4, dtype=d), "x") for d in (torch.float32, torch.float16, torch.bfloat16)] == [None, 1, 2]
    for d in Q.DTYPES:
        with pytest.raises(RuntimeError, match="contiguous"):
            H._feat(torch.zeros(4, 16).to(d)[:, ::2], "x")
        with pytest.raises(RuntimeError, match="HIP tensor"):
            ResidentFeatureTable(torch.zeros(4, 8).to(d))          # a host tensor is no resident table
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            H.quantize_rows(torch.zeros(4, 8), d)
        # the loader drops the row scale: refused by name without L1 normalisation, before the file is opened
        with pytest.raises(RuntimeError, match="normalize=False"):
            ResidentFeatureTable.from_memmap("/nonexistent/features.bin", 4, 8, dtype=d, device="cpu", normalize=False)
    with pytest.raises(RuntimeError, match="uint8"):
        ResidentFeatureTable.from_memmap("/nonexistent/features.bin", 4, 8, dtype=torch.uint8, device="cpu")
    # record()'s batch rules: an 8-bit tensor is a feature under "user" / "photo" only, and both carry one dtype
    z = lambda d: torch.zeros(2, 3, 8).to(d)
    ids = torch.zeros(2, 3, dtype=torch.int64)
    for d in Q.DTYPES:
        Trainer._refuse_unrecordable({"user": z(d), "photo": z(d), "photo_id": ids}, "record()", "step")
        with pytest.raises(RuntimeError, match="one dtype"):
            Trainer._refuse_unrecordable({"user": z(d), "photo": z(torch.float32)}, "record()", "step")
        with pytest.raises(RuntimeError, match="other"):
            Trainer._refuse_unrecordable({"other": z(d)}, "record()", "step")
    with pytest.raises(RuntimeError, match="one dtype"):
        Trainer._refuse_unrecordable({"user": z(torch.int8), "photo": z(torch.float8_e5m2)}, "record()", "step")
    with pytest.raises(RuntimeError, match="int64 ids"):
        Trainer._refuse_unrecordable({"user": z(torch.uint8), "photo": z(torch.uint8)}, "record()", "step")


# ------------------------------------------------------------------ 4. the quantiser's rule
def _rule_rows():
    """64 x 768 Gaussian rows with magnitudes e^-20 .. e^20, one zero row, and rows whose maximum sits on / one ulp under a power of two"""
    rng = np.random.default_rng(8)
    x = (rng.standard_normal((64, 768)) * np.exp(np.linspace(-20, 20, 64))[:, None]).astype(F)
    x[7] = 0
    x[11] = rng.uniform(-1, 1, 768).astype(F)
    x[11, 100] = F(-1.0)
    x[12] = x[11]
    x[12, 100] = np.nextafter(F(1.0), F(0))
    return x


@pytest.mark.parametrize("dtype", Q.DTYPES, ids=["e4m3", "e5m2", "int8"])
def test_the_reference_quantiser_stays_inside_the_formats_error(dtype):
    x = _rule_rows()
    q, s = Q.quantize_rows(x, dtype)
    assert q.dtype == np.uint8 and q.shape == x.shape and s.dtype == F and s.shape == (64,)
    w = Q.widen(Q.from_codes(q, dtype)).numpy()
    assert np.isfinite(w).all()          # no code of a finite row is NaN or inf
    assert s[7] == 0 and not q[7].any() and (s[np.arange(64) != 7] > 0).all()
    v = Q.scaled(x, dtype)
    err = np.abs(w.astype(np.float64) - v.astype(np.float64))
    bound = Q.code_error_bound(v, dtype)
    print("%s: worst error / bound = %.4f" % (Q.NAMES[dtype], float((err / bound).max())))
    assert (err <= bound).all()
    top = {Q.E4M3: 256.0, Q.E5M2: 32768.0, Q.I8: 127.0}[dtype]
    assert np.abs(w).max() <= top
    live = s > 0
    if dtype == Q.I8:
        assert (np.abs(w[live]).max(axis=1) == 127).all()          # the row maximum lands on the last code
    else:
        m = np.abs(v[live]).max(axis=1)
        assert (m >= top / 2).all() and (m < top).all()          # a s in [top / 2, top)
        assert (np.frexp(s[live])[0] == 0.5).all()          # a power of two: the product is exact
        assert (v[live].astype(np.float64) == x[live].astype(np.float64) * s[live, None].astype(np.float64)).all()
        # on a power of two and one ulp under it: frexp puts 1.0 at 0.5 * 2^1, the value below at (1 - 2^-24) * 2^0
        assert s[11] == top / 2 and s[12] == top and np.abs(w[11]).max() == top / 2 and np.abs(w[12]).max() == top
        # round to nearest EVEN is torch's own float32 -> float8 cast on everything the rule produces
        assert np.array_equal(q, torch.from_numpy(v).to(dtype).view(torch.uint8).numpy())


def test_dead_rows_and_signs():
    x = np.zeros((6, 8), F)
    x[0, 3] = np.inf
    x[1, 0] = np.nan          # a NaN in the first place, which a float max would drop
    x[1, 1:] = 1.0
    x[2] = F(2.0 ** -101)          # under the floor
    x[3] = F(2.0 ** -100)          # on it: alive
    x[4] = [1.0, -1.0, 0.5, -0.5, 0.0, -0.0, 1e-30, -1e-30]
    x[5] = [3e38, -3e38, 1e38, 1.0, 0.0, -0.0, 1e30, -1e30]
    for dtype in Q.DTYPES:
        q, s = Q.quantize_rows(x, dtype)
        assert not q[:3].any() and not s[:3].any() and s[3] > 0 and q[3].all()
        w = Q.widen(Q.from_codes(q, dtype)).numpy()
        assert np.isfinite(w).all() and np.isfinite(s).all()
        assert (np.sign(w[4]) == np.sign(np.where(np.abs(x[4]) < 1e-20, 0, x[4]))).all()
        if dtype != Q.I8:
            assert list(q[4, 4:]) == [0, 0x80, 0, 0x80] and list(q[5, 4:6]) == [0, 0x80]          # signed zeros keep their sign bit
        else:
            assert not q[4, 4:].any() and list(w[4, :4]) == [127, -127, 64, -64]          # 63.5 -> 64: ties to even
