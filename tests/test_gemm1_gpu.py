"""The one-product plane GEMMs (segmm_gemm_pq, products = 1: gemm_pl_nt4<1>, gemm_pl_nt8<2|3|4, 1>, gemm_pl_tn4<1>, gemm_pl_tn8<1>)
against the float64 statement of tests/gemm1_ref.py: every output element under the one-product bound derived there (error / bound
<= 1, nothing excluded), bit equality where gemm_ref says so (planes against p32_ref.pack of the fp32 C the kernel wrote, header
words, the repair verdicts), every launch twice with bitwise the same result.  tests/test_gemm1_ref_cpu.py shows without a GPU that
the bound accepts a faithful emulation, rejects the planted defects and rejects a launch that ran three products.

The launch protocol -- NaN / canary-filled wider buffers, operands as column slices, an fp32 copy full of NaN beside usable planes
and canary planes beside an operand that must take its fp32 copy -- is test_gemm_float64_gpu.py's own code, called through a
stand-in for the binding whose ``gemm_p`` adds ``products``.

Cases: gemm1_ref.NT_SHAPES x NT_FORMS under each of NT_ARMS (library knobs, restored afterwards), gemm1_ref.TN_SHAPES x TN_FORMS x
tn_splits under each of TN_ARMS.  A launch that the restated rule (gemm_ref.nt_kernel / tn_plan) sends to a round-2 kernel is held
to gemm_ref's THREE-product statement: products does not reach those kernels.

Run with ``pytest -m gpu -s`` to see the worst error / bound per (kernel, output); SEGMM_GEMM1_RATIO_LOG=path writes them to a file
(profiles/mixed_precision/ratios.txt)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm1_ref as G1      # noqa: E402
import gemm_ref as G      # noqa: E402
import p32_ref as P32      # noqa: E402
import test_gemm_float64_gpu as T      # noqa: E402  (its buffer and launch helpers; no test of it is imported by name)

pytestmark = pytest.mark.gpu
RATIOS = {}
_REF = {}
knobs = T.knobs          # the fixture that sets an arm's knobs and restores them


class _Products:
    """hipabi with ``gemm_p(..., products=n)`` for every launch made through it"""

    def __init__(self, H, n):
        self._H, self._n = H, n

    def __getattr__(self, name):
        return getattr(self._H, name)

    def gemm_p(self, *a, **kw):
        return self._H.gemm_p(*a, products=self._n, **kw)


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    lines = ["%-46s worst error / bound %.3g" % ("%s %s" % k, v) for k, v in sorted(RATIOS.items())]
    print("\n" + "\n".join(lines))
    path = os.environ.get("SEGMM_GEMM1_RATIO_LOG")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


def _note(kernel, ratios):
    for k, r in ratios.items():
        RATIOS[(kernel, k)] = max(RATIOS.get((kernel, k), 0.0), r)


def _bits(x):
    return None if x is None else np.ascontiguousarray(x).view(np.uint16 if x.dtype == np.float16 else np.uint32)


def _same(a, b):
    return set(a) == set(b) and all((a[k] is None and b[k] is None) or np.array_equal(_bits(a[k]), _bits(b[k])) for k in a)


# ------------------------------------------------------------------ NT
def _nt_got(H, form, shape, ref, what):
    """test_gemm_float64_gpu._nt_case's launches and region checks, returning what judge_nt takes"""
    M, N, K = shape
    if form["live"]:
        H.step_set(G.STEP_WORDS, 0)
    got = {}
    if form["repair"]:
        plain = dict(form, planes=False, repair=None, write_c=True)
        got["C32"] = T._region_f32(T._nt_launch(H, plain, shape, ref, False)["C"], M, N, what + " (fp32 launch)")
        st = T._nt_launch(H, form, shape, ref, True, write_c=False, c_scale=ref["c_scale"])
        got["hdr0"] = st["hdr"].cpu().numpy().copy()
        got["hi0"], got["lo0"] = T._region_planes(st["pl"], M, N, 2 * N + 64, what + " (first launch)", overflowed=form["repair"] == "overflow")
        T._nt_launch(H, form, shape, ref, True, write_c=False, repair=True, state=st)          # (the repair launch: the same products)
    else:
        st = T._nt_launch(H, form, shape, ref, form["planes"], write_c=form["write_c"], c_scale=ref["c_scale"])
    got["C"] = T._region_f32(st["C"], M, N, what + " C", written=form["write_c"])
    if form["act"] == G.EPI_GELU:
        got["aux"] = T._region_f32(st["aux"], M, N, what + " aux")
    if form["planes"]:
        got["hi"], got["lo"] = T._region_planes(st["pl"], M, N, 2 * N + 64, what + " planes")
    if "hdr" in st:
        got["hdr"] = st["hdr"].cpu().numpy().copy()
    if form["live"]:
        H.step_set(0, 0)
    return got


def _nt_ref(form, shape, products):
    key = (shape, form["name"], products)
    if key not in _REF:
        _REF[key] = G1.nt_reference(form, shape) if products == 1 else G.nt_reference(form, shape)
    return _REF[key]


@pytest.mark.parametrize("shape", G1.NT_SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("arm", [a for a, _ in G1.NT_ARMS])
def test_nt_one_product(arm, shape, knobs):
    H0 = T._abi()
    live = knobs(dict(G1.NT_ARMS)[arm])
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    H = _Products(H0, 1)
    ran = 0
    for form in G1.NT_FORMS + [G1.NT_ROUND2_FORM]:
        if not G.nt_form_runs(form, shape, "default" if form is G1.NT_ROUND2_FORM else arm):
            continue
        kernel = G.nt_kernel(G.nt_launch(form, shape), live, ncu)
        assert not kernel.startswith("!"), (arm, shape, form["name"], kernel)
        round2 = kernel == "gemm_pl_nt"
        assert round2 == (form is G1.NT_ROUND2_FORM) and (round2 or kernel == ("gemm_pl_nt4" if arm == "nt4" else "gemm_pl_" + arm)), (arm, kernel)
        # a launch the rule sends to the round-2 kernel runs three products whatever is passed: gemm_ref's statement
        ref = _nt_ref(form, shape, 3 if round2 else 1)
        what = "%s products=1 %s %s" % (kernel, shape, form["name"])
        got = _nt_got(H, form, shape, ref, what)
        ratios, exact = G.judge_nt(form, ref, got)
        _note(kernel + (" (three products)" if round2 else " x1"), ratios)
        print("%-64s %s" % (what, " ".join("%s %.3g" % kv for kv in sorted(ratios.items()))))
        assert all(exact.values()), (what, exact)
        assert all(r <= 1.0 for r in ratios.values()), (what, ratios)
        assert _same(got, _nt_got(H, form, shape, ref, what)), what + ": two runs differ"
        ran += 1
    assert ran == len(G1.NT_FORMS) + 1 - (7 if shape[1] % 32 else 0) or shape[1] % 32 == 0


@pytest.mark.parametrize("arm", [a for a, _ in G1.NT_ARMS])
def test_nt_three_products_is_gemm_p(arm, knobs):
    """products = 3 through the new entry point is bitwise segmm_gemm_p: one case per arm, the form with the most outputs"""
    H0 = T._abi()
    knobs(dict(G1.NT_ARMS)[arm])
    shape = (300, 448, 96)
    form = next(f for f in G1.NT_FORMS if f["name"] == "planes")
    ref = _nt_ref(form, shape, 3)

    class _ViaPq(_Products):          # (hipabi.gemm_p calls segmm_gemm_p itself at products = 3: go to the entry point directly)
        def gemm_p(self, *a, **kw):
            L = self._H.lib()
            real = L.segmm_gemm_p
            L.segmm_gemm_p = lambda *args: L.segmm_gemm_pq(*args[:-1], 3, args[-1])
            try:
                return self._H.gemm_p(*a, **kw)
            finally:
                L.segmm_gemm_p = real

    a = _nt_got(H0, form, shape, ref, "segmm_gemm_p")
    b = _nt_got(_ViaPq(H0, 3), form, shape, ref, "segmm_gemm_pq products=3")
    assert _same(a, b)
    assert all(r <= 1.0 for r in G.judge_nt(form, ref, b)[0].values())


# ------------------------------------------------------------------ TN
def _tn_got(H, form, shape, splits, what):
    """test_gemm_float64_gpu._tn_case's launch and region checks"""
    M, N, K = shape
    b = G.tn_base(shape)
    opA, opB = G.tn_operands(shape, form)
    img = np.full(K * 6 * M, P32.CANARY, np.uint16)
    if not opA["fallback"]:
        off = P32._offsets(K, M, 6 * M) + 2 * M
        img[off], img[off + 32] = opA["hi"].view(np.uint16), opA["lo"].view(np.uint16)
    a32 = T._dev(b["A3"]) if opA["fallback"] else T._nan_buf(K, 3 * M)
    pa = H.PT(T._dev(img.view(np.int16)).view(torch.float16), T._dev(opA["hdr"].copy()), K, M, ld2=6 * M, p_off=2 * M, f32=a32, ldf=3 * M, f_off=M)
    wideB = np.full((K, N + 32), np.float32(0.5), np.float32)
    wideB[:, :N] = b["B"]
    pb = T._operand_pt(H, opB, K, N, 2 * N + 64, 0, wideB, N + 32, 0, opB["fallback"])
    C = T._nan_buf(M + 3, N + 32)
    cs = T._nan_buf(1, M + 3)
    if form["acc"]:
        C[:M, :N] = T._dev(b["cold"])
        cs[0, :M] = T._dev(b["csold"])
    nsl = max(1, min(splits, (K + 31) // 32))
    ws = T._nan_buf(1, nsl * (M * N + M) + 64)
    H.gemm_p(H.LAYOUT_TN, M, N, K, pa, pb, C, N + 32, splits=splits, workspace=ws, accumulate=form["acc"], colsum_out=cs if form["colsum"] else None)
    torch.cuda.synchronize()
    got = dict(C=T._region_f32(C, M, N, what + " C"), colsum=None)
    colsum = T._region_f32(cs, 1, M, what + " colsum", written=form["colsum"] or form["acc"])
    if form["colsum"]:
        got["colsum"] = colsum[0]
    elif form["acc"]:
        assert np.array_equal(colsum[0], b["csold"]), what + ": column sums written without colsum_out"
    return got


@pytest.mark.parametrize("shape", G1.TN_SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("arm", [a for a, _ in G1.TN_ARMS])
def test_tn_one_product(arm, shape, knobs):
    H0 = T._abi()
    live = knobs(dict(G1.TN_ARMS)[arm])
    H = _Products(H0, 1)
    M, N, K = shape
    for form in G1.TN_FORMS:
        for splits in G1.tn_splits(K):
            kernel, slabs, _ = G.tn_plan(M, N, K, splits, N + 32, form["acc"], live)
            round2 = kernel == "gemm_pl_tn"          # (accumulate without split-K, 128 rows under tn8): three products, gemm_ref's statement
            assert round2 or kernel == "gemm_pl_" + arm, (arm, kernel)
            key = ("tn", shape, form["name"], splits, round2)
            if key not in _REF:
                _REF[key] = G.tn_reference(form, shape, splits) if round2 else G1.tn_reference(form, shape, splits)
            ref = _REF[key]
            what = "%s%s products=1 %s %s splits %d" % (kernel, "+splitk_reduce" if slabs > 1 else "", shape, form["name"], splits)
            got = _tn_got(H, form, shape, splits, what)
            ratios, _ = G.judge_tn(form, ref, got)
            _note(kernel + (" (three products)" if round2 else " x1"), ratios)
            print("%-72s %s" % (what, " ".join("%s %.3g" % kv for kv in sorted(ratios.items()))))
            assert all(r <= 1.0 for r in ratios.values()), (what, ratios)
            assert _same(got, _tn_got(H, form, shape, splits, what)), what + ": two runs differ"


@pytest.mark.parametrize("arm", [a for a, _ in G1.TN_ARMS])
def test_tn_three_products_is_gemm_p(arm, knobs):
    H0 = T._abi()
    live = knobs(dict(G1.TN_ARMS)[arm])
    shape, splits = (256, 256, 203), 3
    form = next(f for f in G1.TN_FORMS if f["name"] == "colsum")
    assert G.tn_plan(256, 256, 203, splits, 288, False, live)[0] == "gemm_pl_" + arm
    L = H0.lib()
    a = _tn_got(H0, form, shape, splits, "segmm_gemm_p")
    real = L.segmm_gemm_p
    L.segmm_gemm_p = lambda *args: L.segmm_gemm_pq(*args[:-1], 3, args[-1])
    try:
        b = _tn_got(H0, form, shape, splits, "segmm_gemm_pq products=3")
    finally:
        L.segmm_gemm_p = real
    assert _same(a, b)


# ------------------------------------------------------------------ refusals
@pytest.mark.parametrize("products", [0, 2, 4, -1])
def test_other_product_counts_are_refused_by_name(products):
    H0 = T._abi()
    form, shape = G1.NT_FORMS[0], (256, 256, 32)
    with pytest.raises(RuntimeError) as e:
        T._nt_launch(_Products(H0, products), form, shape, _nt_ref(form, shape, 1), False)
    assert "products %d" % products in str(e.value)
