"""tests/gemm_ref.py shown sound without a GPU: an fp32 emulation of the plane GEMMs' arithmetic sits inside every bound at every
case of test_gemm_float64_gpu.py's list, every planted defect is rejected at a case of that list, the restated dispatch rule agrees
with a table worked out by hand, the case list reaches every kernel and every compiled copy of the epilogue (asserted: the list
cannot silently lose an arm), the two tile maps are permutations, and make_drop quantises as common.h says.

Worst emulation ratio (error / bound) over the list (printed with ``-s``): NT C 0.90, aux 0.90, C|aux 0.99, planes 0.06, recorded
maximum 0.015; TN C 0.58, column sums 0.31.  What only passes the accumulator sits at 0.02 - 0.06 (the bound charges one rounding per
product term).  The figures near 1 are single roundings measured against their own u |result|: the row_scale form has a row whose
scale is 2e-4, so its result is the bias plus almost nothing and the bias add's rounding is the whole error and nearly the whole
bound (0.90); with a residual that dominates gelu(aux) the same holds for the residual add (C|aux 0.99); K = 1 has three products
and four charged roundings (TN 0.58)."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_ref as G      # noqa: E402

_REF = {}
WORST = {}


def _ref(form, shape):
    key = (shape, form["name"])
    if key not in _REF:
        _REF[key] = G.nt_reference(form, shape)
    return _REF[key]


def _runs_somewhere(form, shape):
    return any(G.nt_form_runs(form, shape, arm) for arm, _ in G.NT_ARMS)


@pytest.mark.parametrize("shape", G.NT_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_nt_emulation_inside_every_bound(shape):
    for form in G.NT_FORMS:
        if not _runs_somewhere(form, shape):
            continue
        ratios, exact = G.judge_nt(form, _ref(form, shape), G.emulate_nt(form, shape, _ref(form, shape)))
        for k, r in ratios.items():
            WORST["nt " + k] = max(WORST.get("nt " + k, 0.0), r)
        assert not G.rejected(ratios, exact), (form["name"], ratios, exact)
    print({k: round(v, 3) for k, v in WORST.items()})


@pytest.mark.parametrize("shape", G.TN_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_tn_emulation_inside_every_bound(shape):
    for form in G.TN_FORMS:
        for splits in G.tn_splits(shape[2]):
            ratios, exact = G.judge_tn(dict(form, colsum=True), G.tn_reference(form, shape, splits), G.emulate_tn(dict(form, colsum=True), shape, splits))
            for k, r in ratios.items():
                WORST["tn " + k] = max(WORST.get("tn " + k, 0.0), r)
            assert not G.rejected(ratios, exact), (form["name"], splits, ratios)
    print({k: round(v, 3) for k, v in WORST.items()})


@pytest.mark.parametrize("engine", G.ONFLY_ENGINES)
def test_on_the_fly_emulation_inside_every_bound(engine):
    for shape in G.ONFLY_NT_SHAPES:
        for form in G.ONFLY_FORMS:
            ref = G.nt_reference(form, shape, "planes" if engine == "f16x3" else engine)
            ratios, exact = G.judge_nt(form, ref, G.emulate_nt(form, shape, ref, engine="planes" if engine == "f16x3" else engine))
            assert not G.rejected(ratios, exact), (engine, form["name"], ratios, exact)
    for layout in ("nn", "tn"):
        for splits in (1, 2):
            want, bound = G.plain_reference(layout, engine, splits)
            assert G.ratio(G.emulate_plain(layout, engine, splits), want, bound) <= 1.0, (engine, layout, splits)
    assert G.plain_plan(2) == (2, 192) and G.plain_plan(1) == (1, 384)


_FORM = {f["name"]: f for f in G.NT_FORMS}
# where each planted defect is looked for first (any case of the list that rejects it will do)
_AT = {"bias_after_activation": "gelu_p0", "residual_row_not_wrapped": "bias_res100_drop", "dropout_index_with_ldc": "none_p0.5",
       "dropout_after_residual": "bias_res100_drop", "aux_holds_post_activation": "gelu_p0", "dgelu_reads_c": "dgelu_p0",
       "accumulate_ignored": "accumulate", "last_ktile_dropped": "plain", "hi_lo_dropped": "plain", "lo_hi_dropped": "plain",
       "tanh_gelu": "gelu_p0", "wrong_pdf_constant": "dgelu_p0", "block4x4_transposed": "plain", "row_scale_after_bias": "row_scale",
       "plane_scale_x2": "none_p0_planes", "planes_swapped": "none_p0_planes", "flag_not_raised": "repair_overflow"}


@pytest.mark.parametrize("defect", G.NT_DEFECTS)
def test_nt_planted_defect_rejected(defect):
    shapes = [(130, 96, 64), (300, 448, 96)]
    forms = ([_FORM[_AT[defect]]] if defect in _AT else []) + G.NT_FORMS
    for shape in shapes:
        for form in forms:
            if not _runs_somewhere(form, shape):
                continue
            ref = _ref(form, shape)
            if G.rejected(*G.judge_nt(form, ref, G.emulate_nt(form, shape, ref, defect))):
                assert not G.rejected(*G.judge_nt(form, ref, G.emulate_nt(form, shape, ref))), "the faithful emulation is rejected as well"
                return
    pytest.fail("no case of the list rejects the planted defect " + defect)


@pytest.mark.parametrize("defect", G.TN_DEFECTS)
def test_tn_planted_defect_rejected(defect):
    for shape in [(96, 64, 300), (256, 256, 203)]:
        for form in G.TN_FORMS:
            form = dict(form, colsum=True)
            for splits in G.tn_splits(shape[2]):
                ref = G.tn_reference(form, shape, splits)
                if G.rejected(*G.judge_tn(form, ref, G.emulate_tn(form, shape, splits, defect))):
                    assert not G.rejected(*G.judge_tn(form, ref, G.emulate_tn(form, shape, splits)))
                    return
    pytest.fail("no case of the list rejects the planted defect " + defect)


def test_defect_list_is_the_documented_one():
    assert len(set(G.NT_DEFECTS) | set(G.TN_DEFECTS)) == 20


def _L(M, N, K, **kw):
    L = dict(M=M, N=N, K=K, ldc=N, ldaux=N, ldr=N, ldc2=2 * N, res_period=M, act=0)
    L.update(kw)
    return L


def test_dispatch_rule_against_a_hand_written_table():
    """256 CUs.  The NJ model by hand: cost(nj) = rounds * (15 + 11.4 nj K / 768), a narrower tile wins below 0.93 of the best so far."""
    nt = [(_L(20480, 768, 768), {}, "gemm_pl_nt4"), (_L(20480, 3072, 768, act=G.EPI_GELU, aux=True), {}, "gemm_pl_nt4"),
          (_L(20480, 512, 2048), {}, "gemm_pl_nt8<3>"),          # 160 / 240 / 320 tiles: 136.6, 106.2, 2 x 75.8
          (_L(256, 256, 32), {}, "gemm_pl_nt8<4>"),             # 16.9, 16.4, 15.95: no step below 0.93
          (_L(256, 256, 768), {}, "gemm_pl_nt8<2>"),            # one round each: 60.6 -> 49.2 -> 37.8
          (_L(20480, 768, 512), {}, "gemm_pl_nt8<4>"),          # 240 tiles in one round; 320 and 480 need two
          (_L(20480, 768, 768, row_scale=True), {}, "gemm_pl_nt"),
          (_L(20480, 768, 768, residual=True, act=G.EPI_DGELU, aux=True), {}, "gemm_pl_nt"),
          (_L(20480, 768, 768, residual=True, act=G.EPI_GELU, aux=True), {}, "gemm_pl_nt4"),
          (_L(600000, 1024, 64), {}, "gemm_pl_nt"),             # M ldc 4 >= 2^31
          (_L(256, 256, 32), dict(PL_VAR=44), "gemm_pl_nt4"), (_L(20480, 768, 768), dict(PL_VAR=8), "gemm_pl_nt8<4>"),
          (_L(20480, 768, 768), dict(PL_VAR=8, PL_NJ=3), "gemm_pl_nt8<3>"), (_L(20480, 768, 768), dict(PL_VAR=1), "gemm_pl_nt")]
    for L, knobs, want in nt:
        assert G.nt_kernel(L, knobs, ncu=256) == want, (L, knobs)
    assert G.nt_kernel(_L(256, 256, 32, repair=True), dict(PL_VAR=1)).startswith("!")
    assert G.nt_kernel(_L(256, 256, 32, b_f32=True, row_scale=True)).startswith("!")
    tn = [((768, 768, 20480, 28, 768, False), {}, ("gemm_pl_tn4", 28, 736)),          # 640 k-tiles, 23 per slab
          ((3072, 768, 20480, 8, 768, False), {}, ("gemm_pl_tn8", 8, 2560)), ((128, 256, 200, 1, 256, False), {}, ("gemm_pl_tn4", 1, 224)),
          ((96, 64, 300, 3, 64, False), {}, ("gemm_pl_tn", 3, 128)), ((96, 64, 300, 11, 64, False), {}, ("gemm_pl_tn", 10, 32)),
          ((256, 256, 200, 1, 256, True), {}, ("gemm_pl_tn", 1, 224)), ((256, 256, 200, 2, 256, True), {}, ("gemm_pl_tn8", 2, 128)),
          ((256, 256, 203, 3, 256, False), dict(TN_VAR=4), ("gemm_pl_tn4", 3, 96)), ((128, 256, 40, 1, 256, False), dict(TN_VAR=88), ("gemm_pl_tn", 1, 64)),
          ((256, 256, 40, 1, 256, False), dict(TN_VAR=0), ("gemm_pl_tn", 1, 64))]
    for args, knobs, want in tn:
        assert G.tn_plan(*args, knobs=knobs) == want, (args, knobs)
    # the epilogue copy: whole tile, no activation, no dropout, no plane output -> a fast loop; anything else -> one of the twelve
    assert G.nt_epilogue_copies("gemm_pl_nt8<4>", _L(512, 256, 32), False, False) == {"fast<>"}
    assert G.nt_epilogue_copies("gemm_pl_nt8<4>", _L(512, 256, 32, residual=True), False, False) == {"fast<E>"}
    assert G.nt_epilogue_copies("gemm_pl_nt8<4>", _L(300, 256, 32), False, False) == {"fast<>", "row<0,0,0>"}
    assert G.nt_epilogue_copies("gemm_pl_nt4", _L(128, 256, 32, act=G.EPI_DRELU, aux=True), True, True) == {"row<1,1,1>"}
    assert G.nt_epilogue_copies("gemm_pl_nt8<2>", _L(256, 128, 32, act=G.EPI_GELU, aux=True), False, True) == {"row<2,0,1>"}


def test_case_list_reaches_every_kernel_and_epilogue_copy():
    reached = {}
    for arm, knobs in G.NT_ARMS:
        for shape in G.NT_SHAPES:
            for form in G.NT_FORMS:
                if not G.nt_form_runs(form, shape, arm):
                    continue
                L = G.nt_launch(form, shape)
                k = G.nt_kernel(L, knobs)
                assert not k.startswith("!"), (arm, shape, form["name"], k)
                reached.setdefault(k, set()).update(G.nt_epilogue_copies(k, L, form["p"] > 0, form["planes"]))
    twelve = {"row<%d,%d,%d>" % (a, d, p) for a in range(3) for d in range(2) for p in range(2)}
    for k in ("gemm_pl_nt8<2>", "gemm_pl_nt8<3>", "gemm_pl_nt8<4>", "gemm_pl_nt4"):
        assert twelve <= reached[k], (k, sorted(twelve - reached[k]))
        assert {"fast<E>", "fast<>"} <= reached[k], k
    assert any("+row_scale" in t for t in reached["gemm_pl_nt"]) and any("+res+dact" in t for t in reached["gemm_pl_nt"])
    tn, split = set(), False
    for arm, knobs in G.TN_ARMS:
        for shape in G.TN_SHAPES:
            for form in G.TN_FORMS:
                for s in G.tn_splits(shape[2]):
                    k, slabs, _ = G.tn_plan(shape[0], shape[1], shape[2], s, shape[1] + 32, form["acc"], knobs)
                    tn.add(k)
                    split |= slabs > 1
    assert tn == {"gemm_pl_tn4", "gemm_pl_tn8", "gemm_pl_tn"} and split          # with splitk_reduce: the eight GEMM kernels
    assert len(reached) == 5


def test_tile_maps_are_permutations():
    for nbm in range(1, 41):
        for nbn in range(1, 41):
            n = nbm * nbn
            lb = sorted(G.xcd_remap(b, n) for b in range(n))
            assert lb == list(range(n)), (nbm, nbn)
            tiles = {G.nt4_tile(i, nbm, nbn) for i in range(n)}
            assert tiles == {(m, c) for m in range(nbm) for c in range(nbn)}, (nbm, nbn)
    # gemm_pl_nt4's order: groups of four column tiles, row-major inside a group; 5 column tiles: the last group is one tile wide
    assert [G.nt4_tile(i, 2, 5) for i in range(10)] == [(0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (1, 1), (1, 2), (1, 3), (0, 4), (1, 4)]


def test_make_drop():
    assert G.make_drop(0.1, 1, 2)["thresh"] == 6554
    assert G.make_drop(0.99999, 1, 2)["thresh"] == 65535 and G.make_drop(np.nextafter(np.float32(1), np.float32(0)), 1, 2)["thresh"] == 65535
    assert G.make_drop(0.0, 1, 2)["thresh"] == 0 and G.make_drop(0.0, 1, 2)["scale"] == 1
    for p in (0.1, 0.25, 0.5, 0.999, 0.99999):
        d = G.make_drop(p, 1, 2)
        keep = (65536 - d["thresh"]) / 65536.0          # share of the 2^16 draws that are kept
        assert d["scale"] == np.float32(65536.0 / (65536 - d["thresh"]))
        # the expected multiplier keep * scale: exactly 1 with the quantised p (Fraction arithmetic), 1 within the scale's fp32 rounding as stored
        assert Fraction(65536 - d["thresh"], 65536) * Fraction(65536, 65536 - d["thresh"]) == 1
        assert abs(keep * float(d["scale"]) - 1.0) <= 2.0 ** -24
    assert G.make_drop(0.25, 1, 2)["thresh"] == 16384
    assert G.make_drop(0.5, 1, 2)["scale"] * np.float32(0.5) == 1.0
    d = G.make_drop(0.5, G.LIVE_SEED | 0x1_00000003, 7, step_seed=0xFFFFFFFF_00000005)
    assert (d["seed_lo"], d["seed_hi"], d["live"]) == (3 ^ 5, 1 ^ 0x7FFFFFFF, 1)
    # the stream: a census of one site's multipliers meets p, and the four elements of a quad come from (a lo, a hi, b lo, b hi)
    d = G.make_drop(0.25, 0xABCDEF_12345678, 9)
    m = G.drop_mult(d, np.arange(1 << 16))
    assert abs(float((m == 0).mean()) - 0.25) < 0.01 and set(np.unique(m)) == {np.float32(0), d["scale"]}
    a, b = G.drop_rand_quad(d, np.arange(4))
    bits = np.stack([a & 0xFFFF, a >> 16, b & 0xFFFF, b >> 16], 1).reshape(-1)
    assert np.array_equal(m[:16] != 0, bits >= d["thresh"])
