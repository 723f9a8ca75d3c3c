"""tests/attn_ref.py shown sound without a GPU: a faithful fp32 emulation of the attention forward and backward sits inside every
bound at every shape test_attn_float64_gpu.py uses, every planted defect is rejected by a bound, and the restated dispatch rule
agrees with a table of (call -> kernel instance) written out by hand from capi.hip."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_ref as R      # noqa: E402

_CACHE = {}


def _case(shape, p):
    """(inputs, multipliers, statement, forward bounds, backward bounds) of one (shape, p): computed once, never modified"""
    key = (shape, p)
    if key not in _CACHE:
        inp = R.make_inputs(shape)
        mult = R.numpy_mult(shape, p, seed=5)
        st = R.statement(R.operands(inp), inp["mq"], inp["mka"], inp["mkb"], shape[1], mult, inp["dO"])
        bf = R.bounds_fwd(st)
        _CACHE[key] = (inp, mult, st, bf, R.bounds_bwd(st, bf))
    return _CACHE[key]


CASES = [(s, p) for s in R.SHAPES for p in R.drop_ps(s)]


def test_the_masks_hold_every_case_the_gpu_test_needs():
    for shape in R.SHAPES:
        B0, H, dh, Lq, La, Lb = shape
        mq, mka, mkb = R.make_masks(shape, 7)
        assert not mq[0, 0] and (Lq == 1 or mq[0, 1])                       # a masked query in a row that has valid ones
        assert not mka[B0].any() and not mka[B0 + 1].any() and not mkb[B0 + 1].any()
        assert mq[B0 + 2].all() and mka[B0 + 2].all() and mkb[B0 + 2].all()
    for shape, p in CASES:
        if p > 0:
            inp, mult, st = _case(shape, p)[:3]
            dropped = st["mu"] == 0
            assert (dropped & ~st["valid"]).any()                               # a masked key that is dropped: logit 0, not the fill
            assert (dropped & ~inp["mq"][:, None, :, None]).any()               # ... and one in a masked query's row


def test_reference_against_itself_is_at_ratio_zero():
    for shape, p in CASES[:6]:
        inp, mult, st, bf, bb = _case(shape, p)
        again = R.statement(R.operands(inp), inp["mq"], inp["mka"], inp["mkb"], shape[1], mult, inp["dO"])
        assert max(R.ratios(again, st, bf, bb).values()) == 0.0


def test_fp32_emulation_sits_inside_every_bound():
    worst = {}
    for shape, p in CASES:
        inp, mult, st, bf, bb = _case(shape, p)
        r = R.ratios(R.emulate(inp, mult), st, bf, bb)
        assert set(r) == set(R.OUTPUTS_FWD + R.OUTPUTS_BWD)
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
            assert v <= 1.0, (shape, p, k, v)
    print("\n" + "\n".join("fp32 emulation %-4s worst error / bound %.3g" % kv for kv in sorted(worst.items())))
    # the bounds are not slack by orders of magnitude either: a chain bound over <= 200 terms against random rounding
    assert max(worst.values()) > 0.05


# defect -> the outputs at least one of which must leave its bound, at the (shape, p) named
DEFECT_SEEN_BY = {
    "pad_key_filled": (("inv", "O"), (2, 2, 32, 20, 20, 1), 0.0),               # the uniform rows of masked queries: 21 keys, not 48
    "mult_b_unpadded": (("O", "dVb"), (2, 2, 32, 20, 20, 12), 0.1),             # La = 20, La_p = 32
    "drop_after_scale_fills_undropped": (("m", "O"), (2, 3, 48, 40, 40, 100), 0.1),
    "dropped_masked_key_kept": (("O", "inv"), (2, 3, 48, 40, 40, 100), 0.5),
    "key_mask_shifted": (("O", "m"), (2, 3, 48, 40, 40, 100), 0.0),
    "mq_ignored": (("O", "dQa"), (2, 2, 48, 100, 40, 100), 0.0),
    "qb_for_qa": (("O", "dKa"), (1, 2, 64, 49, 17, 30), 0.0),
    "D_without_dropped": (("D",), (2, 3, 48, 40, 40, 100), 0.5),
    "dlogit_without_mult": (("dQa", "dKb"), (2, 3, 48, 40, 40, 100), 0.1),
    "dqa_takes_block_b": (("dQa",), (1, 2, 32, 48, 64, 16), 0.0),
    "head_offset": (("O",), (1, 2, 16, 112, 96, 96), 0.0),
    "inv_holds_sum": (("inv",), (2, 2, 16, 8, 40, 8), 0.0),
    "lse_swapped": (("m", "inv"), (2, 2, 8, 7, 40, 7), 0.0),
    "dq_skips_last_tile": (("dQb",), (1, 1, 48, 33, 176, 16), 0.0),
    "p_rel_2^-11": (("O", "dVa"), (2, 3, 48, 40, 40, 100), 0.0),
}


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_planted_defect_is_rejected(defect):
    outs, shape, p = DEFECT_SEEN_BY[defect]
    inp, mult, st, bf, bb = _case(shape, p)
    r = R.ratios(R.emulate(inp, mult, defect), st, bf, bb)
    assert max(r[k] for k in outs) > 1.0, (defect, {k: r[k] for k in outs})
    if defect == "p_rel_2^-11":          # a lost lo plane must not hide under the wider bounds of the fp16 forms either
        for rep in ("f16x3", "planes"):
            bf2 = R.bounds_fwd(st, rep)
            r2 = R.ratios(R.emulate(inp, mult, defect), st, bf2, R.bounds_bwd(st, bf2, rep))
            assert r2["O"] > 1.0 and r2["dVa"] > 1.0 and r2["dQa"] > 1.0, (rep, r2)


def test_the_fp16_forms_get_wider_bounds_only_by_the_counted_terms():
    inp, mult, st, bf, bb = _case((2, 3, 48, 40, 40, 100), 0.1)
    for rep in ("f16x3", "planes"):
        bf2 = R.bounds_fwd(st, rep)
        bb2 = R.bounds_bwd(st, bf2, rep)
        for k in R.OUTPUTS_FWD:
            assert (bf2[k] >= bf[k]).all() and bf2[k].max() <= 2 * bf[k].max(), (rep, k)
        for k in R.OUTPUTS_BWD:
            assert (bb2[k] >= bb[k]).all() and bb2[k].max() <= 2 * bb[k].max(), (rep, k)


# ------------------------------------------------------------------ dispatch: the table, by hand from capi.hip
# (dh, Lq, La, Lb), pin, knobs -> forward instance
FWD_TABLE = [
    ((16, 1, 1, 20), False, {}, "fwd<16,4>"),
    ((32, 20, 20, 1), False, {}, "fwd<32,4>"),
    ((32, 20, 20, 12), False, {}, "fwd<32,4>"),
    ((32, 20, 20, 12), True, {}, "fwd_pl<32,4>"),
    ((32, 20, 20, 12), True, {"ATT_FWD_PL": 0}, "fwd<32,4>"),
    ((32, 20, 20, 1), True, {}, "fwd<32,4>"),                                   # Lb % 4 != 0: the planes-in forward declines
    ((48, 40, 40, 100), False, {}, "fwd<48,10>"),                               # three query tiles: direct by default
    ((48, 40, 40, 100), False, {"ATT_FWD_LDS": 0}, "fwd<48,10>"),
    ((48, 40, 40, 100), False, {"ATT_FWD_LDS": 2}, "fwd_lds<48,10>ksp1"),
    ((48, 40, 40, 100), False, {"ATT_FWD_LDS": 2, "ATT_FWD_KSPLIT": 2}, "fwd_lds<48,10>ksp2"),
    ((48, 40, 40, 100), False, {"ATT_FWD_LDS": 2, "ATT_FWD_KSPLIT": 3}, "fwd_lds<48,10>ksp3"),
    ((48, 40, 40, 100), True, {}, "fwd_pl<48,9,40,hot>"),
    ((48, 100, 40, 100), False, {}, "fwd_lds<48,10>ksp1"),                      # seven query tiles: staged by default
    ((48, 100, 40, 100), False, {"ATT_FWD_LDS": 2, "ATT_FWD_KSPLIT": 2}, "fwd_lds<48,10>ksp1"),          # 14 waves > 12: one group
    ((48, 100, 40, 100), False, {"ATT_FWD_LDS": 0}, "fwd<48,10>"),
    ((48, 100, 40, 100), True, {}, "fwd_pl<48,9,40,hot>"),
    ((64, 49, 17, 30), False, {}, "fwd_lds<64,4>ksp1"),                         # four query tiles, Tp = 64
    ((64, 49, 17, 30), False, {"ATT_FWD_LDS": 0}, "fwd<64,4>"),
    ((64, 49, 17, 30), False, {"ATT_FWD_LDS": 2, "ATT_FWD_KSPLIT": 3}, "fwd_lds<64,4>ksp3"),
    ((64, 49, 17, 30), True, {}, "fwd_lds<64,4>ksp1"),
    ((16, 112, 96, 96), False, {}, "fwd_lds<16,12>ksp1"),
    ((16, 112, 96, 96), False, {"ATT_FWD_LDS": 0}, "fwd<16,12>"),
    ((16, 112, 96, 96), True, {}, "fwd_pl<16,12>"),
    ((16, 113, 96, 96), True, {}, "fwd_lds<16,12>ksp1"),                        # Lq = 112 | 113: eight query tiles, no planes-in form
    ((48, 33, 176, 16), False, {}, "fwd<48,12>"),
    ((48, 33, 176, 16), False, {"ATT_FWD_LDS": 2}, "fwd<48,12>"),               # 82 112 bytes of K / V: over the staged form's 80 KB
    ((48, 33, 176, 16), True, {}, "fwd_pl<48,12>"),
    ((32, 48, 64, 16), False, {}, "fwd<32,10>"),
    ((32, 48, 64, 16), False, {"ATT_FWD_LDS": 2, "ATT_FWD_KSPLIT": 3}, "fwd_lds<32,10>ksp3"),
    ((32, 48, 64, 16), True, {}, "fwd_pl<32,9>"),
    ((16, 8, 40, 8), False, {}, "fwd<16,4>"),
    ((16, 8, 40, 8), True, {}, "fwd_pl<16,4>"),
    ((8, 7, 40, 7), False, {"ATT_FWD_LDS": 2}, "fwd<8,4>"),                     # no staged form below head dim 16
    ((4, 33, 5, 3), False, {"ATT_FWD_LDS": 2}, "fwd<4,4>"),
    ((16, 40, 0, 100), False, {}, "fwd<16,10>"),
    ((16, 40, 0, 100), True, {}, "fwd_pl<16,9>"),
    ((16, 40, 40, 0), False, {}, "fwd<16,4>"),
    ((16, 40, 40, 0), True, {}, "fwd_pl<16,4>"),
    # Tp = 64 | 80, 160 | 176, 192 | 208
    ((16, 40, 64, 0), False, {}, "fwd<16,4>"), ((16, 40, 64, 16), False, {}, "fwd<16,10>"),
    ((16, 40, 160, 0), False, {}, "fwd<16,10>"), ((16, 40, 160, 16), False, {}, "fwd<16,12>"),
    ((16, 40, 176, 16), False, {}, "fwd<16,12>"), ((16, 40, 192, 16), False, {}, "fwd_stream<16>"),
    ((16, 40, 40, 8), False, {"ATT_STREAM": 1}, "fwd_stream<16>"),
    # planes-in forward: T = 64 | 68, 144 | 148
    ((16, 40, 32, 32), True, {}, "fwd_pl<16,4>"), ((16, 40, 32, 36), True, {}, "fwd_pl<16,9>"),
    ((16, 40, 44, 100), True, {}, "fwd_pl<16,9>"), ((16, 40, 48, 100), True, {}, "fwd_pl<16,12>"),
    ((48, 40, 40, 88), True, {}, "fwd_pl<48,9>"), ((48, 40, 40, 92), True, {}, "fwd_pl<48,9,40,hot>"),          # hot: 128 < T <= 144
]

# (dh, Lq, La, Lb), phase, mode, pin, knobs -> launches
BWD_TABLE = [
    ((16, 1, 1, 20), 4, 1, False, {}, ("fused<16,4,merged,16>",)),
    ((16, 1, 1, 20), 4, 0, False, {}, ("fused<16,4,merged,16>",)),
    ((16, 1, 1, 20), 4, 2, False, {}, ("fused16<16,4,one>a/w1", "fused16<16,4,one>b/w2")),
    ((16, 1, 1, 20), 4, 0, False, {"ATT_MERGE": 0}, ("fused<16,4,16>a/w1", "fused<16,4,16>b/w2")),
    ((16, 1, 1, 20), 0, 1, False, {}, ("dq<16,4>", "dkv<16,1>")),
    ((32, 20, 20, 1), 4, 1, False, {}, ("fused<32,4,merged,32>",)),
    ((32, 20, 20, 1), 4, 1, False, {"ATT_MERGE": 0}, ("fused<32,4,32>a/w2", "fused<32,4,32>b/w1")),
    ((32, 20, 20, 12), 4, 1, False, {}, ("fused<32,4,merged,32>",)),
    ((32, 20, 20, 12), 4, 1, True, {}, ("pl<32,4,one>a/w2", "pl<32,4,one>b/w1")),
    ((32, 20, 20, 12), 5, 1, False, {}, ("fused<32,4,32>a/w2",)),               # one key block: never the merged form
    ((48, 40, 40, 100), 4, 1, False, {}, ("fused16<48,4,one>a/w3", "fused16<48,4,one>b/w4")),          # 7 tiles in passes over 4 waves
    ((48, 40, 40, 100), 4, 1, False, {"ATT_WAVES": 1}, ("fused16<48,4,one>a/w1", "fused16<48,4,one>b/w1")),
    ((48, 40, 40, 100), 4, 0, False, {}, ("fused<48,4,one>a/w3", "fused<48,8,one>b/w7")),
    ((48, 40, 40, 100), 4, 2, False, {}, ("fused16<48,4,one>a/w3", "fused16<48,4,one>b/w4")),
    ((48, 40, 40, 100), 4, 1, False, {"ATT_FUSED_LAUNCH": 1}, ("fused16<48,4,one>ab/w4",)),
    ((48, 40, 40, 100), 4, 0, False, {"ATT_FUSED_LAUNCH": 1}, ("fused<48,8,one>ab/w7",)),
    ((48, 40, 40, 100), 5, 1, False, {}, ("fused16<48,4,one>a/w3",)),
    ((48, 40, 40, 100), 6, 1, False, {}, ("fused16<48,4,one>b/w4",)),
    ((48, 40, 40, 100), 4, 1, True, {}, ("pl<48,4,one>a/w3", "pl<48,4,one>b/w3")),
    ((48, 40, 40, 100), 4, 1, True, {"ATT_WAVES_PL": 1}, ("pl<48,4,one>a/w1", "pl<48,4,one>b/w1")),
    ((48, 40, 40, 100), 0, 1, False, {}, ("dq<48,10>", "dkv<48,3>")),
    ((48, 40, 40, 100), 1, 1, False, {}, ("D<48>",)),
    ((48, 40, 40, 100), 2, 1, False, {}, ("dq<48,10>",)),
    ((48, 40, 40, 100), 3, 1, False, {}, ("dkv<48,3>",)),
    ((48, 100, 40, 100), 4, 1, False, {}, ("fused<48,4,chunks>a/w3", "fused<48,8,chunks>b/w7")),          # several chunks: fp32 by default
    ((48, 100, 40, 100), 4, 2, False, {}, ("fused16<48,4,chunks>a/w3", "fused16<48,8,chunks>b/w7")),
    ((48, 100, 40, 100), 4, 1, True, {}, ("pl<48,4,chunks>a/w3", "pl<48,8,chunks>b/w7")),
    ((48, 100, 40, 100), 0, 1, False, {}, ("dq<48,10>", "dkv<48,0>")),
    ((64, 49, 17, 30), 4, 1, False, {}, ("fused<64,4,chunks>a/w2", "fused<64,4,chunks>b/w2")),
    ((64, 49, 17, 30), 4, 2, False, {}, ("fused<64,4,chunks>a/w2", "fused<64,4,chunks>b/w2")),          # no fp16x3 form at head dim 64
    ((64, 49, 17, 30), 4, 1, True, {}, ("fused<64,4,chunks>a/w2", "fused<64,4,chunks>b/w2")),
    ((64, 48, 17, 30), 4, 1, False, {}, ("fused<64,4,one>a/w2", "fused<64,4,one>b/w2")),                # Lq = 48 | 49
    ((16, 112, 96, 96), 4, 1, False, {}, ("fused<16,8,chunks>a/w6", "fused<16,8,chunks>b/w6")),
    ((16, 112, 96, 96), 4, 1, True, {}, ("pl<16,8,chunks>a/w6", "pl<16,8,chunks>b/w6")),
    ((16, 112, 96, 96), 0, 1, False, {}, ("dq<16,12>", "dkv<16,0>")),
    ((48, 33, 176, 16), 4, 1, False, {}, ("fused16<48,4,one>a/w4", "fused16<48,4,one>b/w1")),
    ((48, 33, 176, 16), 4, 0, False, {}, ("fused<48,12,one>a/w11", "fused<48,4,one>b/w1")),
    ((48, 33, 176, 16), 4, 1, True, {}, ("pl<48,4,one>a/w3", "pl<48,4,one>b/w1")),
    ((48, 33, 176, 16), 4, 1, True, {"ATT_WAVES_PL": 4}, ("pl<48,4,one>a/w4", "pl<48,4,one>b/w1")),
    ((32, 48, 64, 16), 4, 1, False, {}, ("fused16<32,4,one>a/w4", "fused16<32,4,one>b/w1")),
    ((32, 48, 64, 16), 4, 0, False, {}, ("fused<32,4,one>a/w4", "fused<32,4,one>b/w1")),
    ((32, 48, 64, 16), 0, 1, False, {}, ("dq<32,10>", "dkv<32,3>")),
    ((16, 8, 40, 8), 4, 1, False, {}, ("fused<16,4,merged,16>",)),              # nta + ntb = 4 | 5
    ((16, 8, 56, 8), 4, 1, False, {}, ("fused<16,4,16>a/w4", "fused<16,4,16>b/w1")),
    ((16, 8, 40, 8), 4, 1, True, {}, ("pl<16,4,one>a/w3", "pl<16,4,one>b/w1")),
    ((8, 7, 40, 7), 4, 1, False, {}, ("fused<8,4,merged,16>",)),
    ((8, 7, 40, 7), 4, 2, False, {}, ("fused<8,4,merged,16>",)),
    ((4, 33, 5, 3), 4, 1, False, {}, ("fused<4,4,one>a/w1", "fused<4,4,one>b/w1")),
    ((4, 33, 5, 3), 0, 1, False, {}, ("dq<4,4>", "dkv<4,3>")),
    ((16, 40, 0, 100), 4, 1, False, {}, ("fused16<16,4,one>b/w4",)),
    ((16, 40, 0, 100), 4, 0, False, {}, ("fused<16,8,one>b/w7",)),
    ((16, 40, 40, 0), 4, 1, False, {}, ("fused16<16,4,one>a/w3",)),
    ((16, 40, 40, 0), 4, 1, True, {}, ("pl<16,4,one>a/w3",)),
    # Lq = 16 | 17, 32 | 33 (mode 0: the fp32 instances; mode 1: the fp16x3 form from 33 queries on)
    ((16, 16, 40, 100), 4, 0, False, {}, ("fused<16,4,16>a/w3", "fused<16,8,16>b/w7")),
    ((16, 17, 40, 100), 4, 0, False, {}, ("fused<16,4,32>a/w3", "fused<16,8,32>b/w7")),
    ((16, 32, 40, 100), 4, 1, False, {}, ("fused<16,4,32>a/w3", "fused<16,8,32>b/w7")),
    ((16, 33, 40, 100), 4, 1, False, {}, ("fused16<16,4,one>a/w3", "fused16<16,4,one>b/w4")),
    ((16, 32, 20, 12), 4, 1, False, {}, ("fused<16,4,merged,32>",)),
    ((16, 33, 20, 12), 4, 1, False, {}, ("fused16<16,4,one>a/w2", "fused16<16,4,one>b/w1")),
]


@pytest.mark.parametrize("row", FWD_TABLE, ids=lambda r: "%s-pin%d-%s" % ("x".join(map(str, r[0])), r[1], ",".join("%s=%s" % kv for kv in r[2].items())))
def test_forward_dispatch_rule_agrees_with_the_table(row):
    (dh, Lq, La, Lb), pin, knobs, want = row
    assert R.fwd_instance(dh, Lq, La, Lb, pin=pin, knobs=knobs) == want


@pytest.mark.parametrize("row", BWD_TABLE, ids=lambda r: "%s-ph%d-m%d-pin%d-%s" % ("x".join(map(str, r[0])), r[1], r[2], r[3], ",".join("%s=%s" % kv for kv in r[4].items())))
def test_backward_dispatch_rule_agrees_with_the_table(row):
    (dh, Lq, La, Lb), phase, mode, pin, knobs, want = row
    assert R.bwd_instance(dh, Lq, La, Lb, phase, mode=mode, pin=pin, knobs=knobs) == want


def test_the_table_covers_every_gpu_shape():
    fw = {r[0] for r in FWD_TABLE}
    bw = {r[0] for r in BWD_TABLE}
    for shape in R.SHAPES:
        assert shape[2:] in fw and shape[2:] in bw, shape
    assert R.rep_of(("pl<48,4,one>a/w3", "pl<48,4,one>b/w3")) == "planes"
    assert R.rep_of(("fused16<48,4,one>a/w3",)) == "f16x3" and R.rep_of(("fused<8,4,merged,16>",)) == "f32"
    assert R.fwd_ksplit("fwd_lds<48,10>ksp3") == 3 and R.fwd_ksplit("fwd<48,10>") == 1
    assert np.float64(R.scale_of(48)) == np.float64(np.float32(1.0) / np.sqrt(np.float32(48.0)))
