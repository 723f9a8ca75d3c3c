"""tests/gemm1_ref.py, the host statement of the one-product plane GEMMs, shown sound without a GPU: a faithful fp32 emulation of
the one-product arithmetic passes its bound at every case test_gemm1_gpu.py runs, every planted defect is rejected, and the
one-product and three-product statements cannot be mistaken for each other -- gemm_ref's three-product emulation fails the
one-product bound (a launch that silently ran three products cannot pass test_gemm1_gpu.py) and the one-product emulation fails
gemm_ref's bound (the default path's float64 test cannot pass on one product)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm1_ref as G1      # noqa: E402
import gemm_ref as G      # noqa: E402

_ID = lambda s: "%dx%dx%d" % s


@pytest.mark.parametrize("shape", G1.NT_SHAPES, ids=_ID)
def test_nt_emulation_passes_the_bound(shape):
    ran = 0
    for form in G1.NT_FORMS:
        if (form["planes"] or form["repair"]) and shape[1] % 32:
            continue
        ref = G1.nt_reference(form, shape)
        ratios, exact = G1.judge_nt(form, ref, G1.emulate_nt(form, shape, ref))
        assert all(exact.values()), (shape, form["name"], exact)
        assert all(r <= 1.0 for r in ratios.values()), (shape, form["name"], ratios)
        ran += 1
    assert ran == len(G1.NT_FORMS)


@pytest.mark.parametrize("shape", G1.TN_SHAPES, ids=_ID)
def test_tn_emulation_passes_the_bound(shape):
    for form in G1.TN_FORMS:
        for splits in G1.tn_splits(shape[2]):
            ref = G1.tn_reference(form, shape, splits)
            ratios, _ = G1.judge_tn(form, ref, G1.emulate_tn(form, shape, splits))
            assert all(r <= 1.0 for r in ratios.values()), (shape, form["name"], splits, ratios)


def test_case_list_is_what_the_kernels_need():
    assert [s[2] for s in G1.NT_SHAPES[:5]] == [32, 64, 96, 128, 224] and (130, 96, 64) in G1.NT_SHAPES and (300, 448, 96) in G1.NT_SHAPES
    assert sorted({s[2] for s in G1.TN_SHAPES}) == [1, 8, 40, 200, 203] and {s[:2] for s in G1.TN_SHAPES} == {(256, 256), (128, 256)}
    names = {f["name"] for f in G1.NT_FORMS}
    assert {"repair_" + r for r in G.REPAIR_SHIFT} <= names and {"a_flag", "b_flag", "a_delay3", "b_delay3"} <= names
    # every arm reaches its kernel at every shape by the restated rule, and the round-2 form reaches the round-2 kernel under every arm
    for arm, kn in G1.NT_ARMS:
        for shape in G1.NT_SHAPES:
            for form in G1.NT_FORMS:
                k = G.nt_kernel(G.nt_launch(form, shape), kn)
                assert k == ("gemm_pl_nt4" if arm == "nt4" else "gemm_pl_" + arm), (arm, shape, form["name"], k)
            assert G.nt_kernel(G.nt_launch(G1.NT_ROUND2_FORM, shape), kn) == "gemm_pl_nt"
    for arm, kn in G1.TN_ARMS:
        for M, N, K in G1.TN_SHAPES:
            for form in G1.TN_FORMS:
                for splits in G1.tn_splits(K):
                    k = G.tn_plan(M, N, K, splits, N + 32, form["acc"], kn)[0]
                    # (what does not fit a kernel's whole tiles, or accumulates without split-K, goes to the round-2 kernel: three products)
                    assert k in ("gemm_pl_" + arm, "gemm_pl_tn"), (arm, (M, N, K), k)
    assert any(G.tn_plan(M, N, K, s, N + 32, f["acc"], kn)[0] == "gemm_pl_" + arm for arm, kn in G1.TN_ARMS for M, N, K in G1.TN_SHAPES
               for f in G1.TN_FORMS for s in G1.tn_splits(K))


NT_DEFECT_CASES = [((256, 256, 224), "plain"), ((300, 448, 96), "bias_gelu"), ((130, 96, 64), "planes"), ((256, 256, 64), "a_flag")]


@pytest.mark.parametrize("defect", [d for d in G1.DEFECTS if d != "colsum_kept_lo"])
def test_nt_planted_defects_are_rejected(defect):
    forms = {f["name"]: f for f in G1.NT_FORMS}
    for shape, name in NT_DEFECT_CASES:
        form = forms[name]
        ref = G1.nt_reference(form, shape)
        assert G1.rejected(*G1.judge_nt(form, ref, G1.emulate_nt(form, shape, ref, defect))), (defect, shape, name)


@pytest.mark.parametrize("defect", G1.DEFECTS)
def test_tn_planted_defects_are_rejected(defect):
    forms = {f["name"]: f for f in G1.TN_FORMS}
    for shape, name, splits in (((256, 256, 203), "colsum", 1), ((128, 256, 200), "colsum_acc", 3), ((256, 256, 40), "a_flag_colsum", 2)):
        form = forms[name]
        ref = G1.tn_reference(form, shape, splits)
        assert G1.rejected(*G1.judge_tn(form, ref, G1.emulate_tn(form, shape, splits, defect))), (defect, shape, name)


def test_the_two_statements_cannot_be_confused():
    """Three products held to the one-product bound and one product held to the three-product bound both fail at every shape the
    GPU test runs.  The cross terms hi lo + lo hi are ~2^-12.5 sqrt(2 K) of the products' RMS, the one-product bound K 2^-24 of their
    absolute SUM (K terms): worst element / bound ~ 2^12 / K^1.5 times a few sigma -- 177 at K = 32, 10 at K = 224 (printed below).  The
    margin shrinks with K (a worst-case chain bound grows as K^2, a random-sign error as sqrt K): near K = 768 it is of order one, so
    the statement discriminates at the test's shapes, which is where it is used, and is no claim about the step's widths."""
    plain = G1.NT_FORMS[0]
    for shape in G1.NT_SHAPES:
        ref1, ref3 = G1.nt_reference(plain, shape), G.nt_reference(plain, shape)
        three = G.emulate_nt(plain, shape, ref3)
        one = G1.emulate_nt(plain, shape, ref1)
        r31 = G1.judge_nt(plain, ref1, three)[0]["C"]
        r13 = G.judge_nt(plain, ref3, one)[0]["C"]
        print("%s: three products / one-product bound %.3g, one product / three-product bound %.3g" % (shape, r31, r13))
        assert r31 > 1.0 and r13 > 1.0, (shape, r31, r13)
        assert G.judge_nt(plain, ref3, three)[0]["C"] <= 1.0 and G1.judge_nt(plain, ref1, one)[0]["C"] <= 1.0
    assert max(s[2] for s in G1.NT_SHAPES) == 224          # (the figures above are for these widths)
    tn = G1.TN_FORMS[0]
    for shape in ((256, 256, 203), (128, 256, 40)):
        r = G1.judge_tn(tn, G1.tn_reference(tn, shape, 1), G.emulate_tn(tn, shape, 1))[0]["C"]
        assert r > 1.0, (shape, r)


def test_gemm_ref_is_left_as_it_was():
    terms, acc = G._terms, G._acc32
    with G1.one_product():
        assert G._terms is not terms and G._acc32 is not acc
    assert G._terms is terms and G._acc32 is acc
