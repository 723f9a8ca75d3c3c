"""tests/attn_ref.py shown sound without a GPU: a faithful fp32 emulation of the attention forward and backward sits inside every
bound at every shape test_attn_float64_gpu.py uses, every planted defect is rejected by a bound, and the restated dispatch rule
agrees with a table of (call -> kernel instance) written out by hand from capi.hip.  The second half does the same for the wide
heads and the streamed kernels (test_attn_wide_stream_float64_gpu.py): the online order's emulation under the streamed constants,
its planted defects, the launch rule with workgroup shapes and pass counts, and the dropout preconditions on the kernels' own stream."""
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


# ================================================================== wide heads (96, 128) and the streamed kernels
_CACHE_X = {}
NEW_SHAPES = R.STREAM_SMALL + R.STREAM_LONG + R.STREAM_FUSED + R.STREAM_FUSED_RUN + R.WIDE_SHAPES
NEW_CASES = [(s, p) for s in NEW_SHAPES for p in R.drop_ps_x(s)]


def _case_x(shape, p):
    """as _case, under the host restatement of the kernels' dropout stream (the seed and site of the GPU module) and with the
    streamed forward's constants: the widest forward a shape of the list is run behind"""
    key = (shape, p)
    if key not in _CACHE_X:
        inp = R.make_inputs(shape)
        mult = R.host_mult(shape, p)
        st = R.statement(R.operands(inp), inp["mq"], inp["mka"], inp["mkb"], shape[1], mult, inp["dO"])
        bf = R.bounds_fwd(st, stream=R.n_tiles(shape))
        _CACHE_X[key] = (inp, mult, st, bf, R.bounds_bwd(st, bf))
    return _CACHE_X[key]


def test_the_dropout_preconditions_hold_on_the_kernels_own_stream():
    """every p > 0 case of the GPU module: a dropped masked key, and a dropped key in a masked query's row, under the recorded seed"""
    for shape, p in NEW_CASES:
        mq, mka, mkb = R.make_masks(shape, 7)
        B0 = shape[0]
        assert not mka[B0].any() and not mka[B0 + 1].any() and not mkb[B0 + 1].any() and mq[B0 + 2].all()
        if p > 0:
            inp, mult, st = _case_x(shape, p)[:3]
            thresh = int(float(np.float32(p)) * 65536.0 + 0.5)
            assert set(np.unique(mult)) == {np.float32(0.0), np.float32(65536.0 / (65536.0 - thresh))}
            assert abs(float((mult == 0).mean()) - p) < 0.05, (shape, p)
            dropped = st["mu"] == 0
            assert (dropped & ~st["valid"]).any(), (shape, p)
            assert (dropped & ~inp["mq"][:, None, :, None]).any(), (shape, p)


def test_online_order_emulation_sits_inside_every_bound():
    """The streamed order (tile by tile, m / a / l / o) at every new shape under the streamed form's constants, with dQ in passes over
    8 waves and the wide kernel's D order at the wide head dims, attn_row_D's and one chain over the keys at the others."""
    worst = {}
    for shape, p in NEW_CASES:
        inp, mult, st, bf, bb = _case_x(shape, p)
        wide = R.wide(shape[2])
        r = R.ratios(R.emulate_online(inp, mult, passes=R.ATT_WIDE_MAXW if wide else 0, d_order="wide" if wide else "row"), st, bf, bb)
        assert set(r) == set(R.OUTPUTS_FWD + R.OUTPUTS_BWD)
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
            assert v <= 1.0, (shape, p, k, v)
    print("\n" + "\n".join("online-order emulation %-4s worst error / bound %.3g" % kv for kv in sorted(worst.items())))
    assert max(worst.values()) > 0.05


def test_the_streamed_constants_only_add_the_counted_terms():
    """bounds_fwd(stream=nt) against the held form at a 14-tile shape: every bound at least the held one less the row-sum chain it
    replaces, and below three times it; stream = 0 is the held form, bit for bit"""
    inp, mult, st, bf, bb = _case_x((1, 2, 16, 17, 200, 9), 0.1)
    held = R.bounds_fwd(st)
    again = R.bounds_fwd(st, "f32", False, 0)
    for k in ("O", "m", "inv", "N"):
        assert (again[k] == held[k]).all()
        assert (bf[k] <= 3 * held[k]).all() and (bf[k] >= 0.1 * held[k]).all(), k
    assert (bf["m"] == held["m"]).all()
    T, nt = 209, 14
    assert np.allclose(bf["N"] - held["N"], ((2 * nt + 7) - (T + 3) + 2 * (nt - 1)) * R.U, rtol=0, atol=1e-12)


def test_held_order_and_defect_at_the_wide_head_dims():
    """the direct kernels at 96 and 128 are held to the HELD forward's constants: the index-order emulation sits inside them, the
    relative 2^-11 on P does not"""
    for shape in ((1, 2, 96, 40, 40, 100), (1, 2, 128, 49, 17, 30)):
        inp, mult, st = _case_x(shape, 0.1)[:3]
        bf = R.bounds_fwd(st)
        bb = R.bounds_bwd(st, bf)
        assert max(R.ratios(R.emulate(inp, mult), st, bf, bb).values()) <= 1.0
        r = R.ratios(R.emulate(inp, mult, "p_rel_2^-11"), st, bf, bb)
        assert r["O"] > 1.0 and r["dVa"] > 1.0, r


# defect -> (outputs ALL of which must leave their bounds, shape, p)
STREAM_DEFECT_SEEN_BY = {
    "rescale_l_not_o": (("O", "D"), (1, 2, 16, 17, 200, 9), 0.0),
    "max_follows_lower_tile": (("m", "inv", "O"), (1, 2, 16, 17, 200, 9), 0.0),
    "odd_last_tile_dropped": (("O", "dVa"), (1, 2, 48, 40, 200, 0), 0.0),                  # 13 tiles
    "block_b_tile_not_rebased": (("O", "dQb"), (1, 2, 16, 17, 200, 9), 0.0),
    "pad_key_a_in_rowsum": (("inv", "O"), (2, 2, 32, 20, 20, 12), 0.0),                    # La = 20: 12 pad keys in block a
    "drop_index_T": (("O", "inv"), (1, 2, 16, 17, 200, 9), 0.1),                           # T = 209, Tp = 224
    "carry_lost": (("dQa",), (1, 1, 96, 33, 176, 16), 0.0),                                # 11 tiles: passes of 8 + 3
    "carry_twice": (("dQa",), (1, 1, 128, 52, 132, 16), 0.0),                              # 9 tiles: 8 + 1, two chunks
    "pass2_owns_tile_w": (("dQa",), (1, 1, 96, 33, 176, 16), 0.0),
    "head_offset_128_at_96": (("O",), (1, 2, 96, 40, 40, 100), 0.0),
    "D_first_partials": (("D",), (1, 2, 96, 40, 40, 100), 0.0),
    "p_rel_2^-11": (("O", "dVa"), (1, 1, 128, 33, 256, 256), 0.0),                         # at the widest bounds of the list: 32 tiles
}


@pytest.mark.parametrize("defect", R.STREAM_DEFECTS)
def test_planted_streamed_or_wide_defect_is_rejected(defect):
    outs, shape, p = STREAM_DEFECT_SEEN_BY[defect]
    inp, mult, st, bf, bb = _case_x(shape, p)
    wide = R.wide(shape[2])
    kw = dict(passes=R.ATT_WIDE_MAXW if wide else 0, d_order="wide" if wide else "row")
    sound = R.ratios(R.emulate_online(inp, mult, **kw), st, bf, bb)
    r = R.ratios(R.emulate_online(inp, mult, defect, **kw), st, bf, bb)
    assert max(sound.values()) <= 1.0
    assert all(r[k] > 1.0 for k in outs), (defect, {k: r[k] for k in outs})


# (H, dh, Lq, La, Lb), knobs -> forward launch; by hand from attn_launch_fwd / attn_shape
FWD_TABLE_X = [
    ((2, 96, 40, 40, 100), {}, "fwd<96,10>/wq3/hpb1"),
    ((2, 128, 100, 40, 100), {}, "fwd<128,10>/wq4/hpb1"),                          # 7 query tiles: 4 + 3 and a surplus wave
    ((2, 128, 100, 40, 100), {"ATT_FWD_LDS": 2}, "fwd<128,10>/wq4/hpb1"),          # no staged form at a wide head
    ((2, 96, 80, 40, 100), {}, "fwd<96,10>/wq5/hpb1"),                             # the direct forward is bounded for five waves at every dh
    ((2, 96, 80, 40, 100), {"ATT_STREAM": 1}, "fwd_stream<96>/wq4/hpb1"),          # ... the streamed one for four at a wide head
    ((2, 48, 80, 40, 100), {"ATT_STREAM": 1}, "fwd_stream<48>/wq5/hpb1"),
    ((1, 128, 33, 256, 256), {}, "fwd_stream<128>/wq3/hpb1"),
    ((2, 32, 20, 20, 12), {"ATT_HPB_FWD": 2}, "fwd<32,4>/wq2/hpb2"),
    ((4, 4, 33, 5, 3), {"ATT_HPB_FWD": 2}, "fwd<4,4>/wq3/hpb1"),                   # 2 x 3 waves > 5: the knob cannot take effect
    ((4, 4, 33, 5, 3), {"ATT_HPB_FWD": 2 | 2 << 8}, "fwd<4,4>/wq2/hpb2"),
    ((2, 16, 17, 200, 9), {"ATT_HPB_FWD": 2}, "fwd_stream<16>/wq2/hpb2"),
]
# (H, dh, Lq, La, Lb), phase, pin, knobs -> backward launches; by hand from attn_launch_bwd
BWD_TABLE_X = [
    ((2, 96, 1, 1, 20), 4, False, {}, ("wide<96,4,merged,16>/w3/p1",)),
    ((2, 128, 20, 20, 12), 4, False, {}, ("wide<128,4,merged,32>/w3/p1",)),
    ((2, 128, 20, 20, 12), 4, False, {"ATT_MERGE": 0}, ("wide<128,4,32>a/w2/p1", "wide<128,4,32>b/w1/p1")),
    ((2, 96, 40, 40, 100), 4, False, {}, ("wide<96,4,one>a/w3/p1", "wide<96,8,one>b/w7/p1")),
    ((2, 96, 40, 40, 100), 4, False, {"ATT_FUSED_LAUNCH": 1}, ("wide<96,8,one>ab/w7/p1",)),
    ((2, 96, 40, 40, 100), 6, False, {}, ("wide<96,8,one>b/w7/p1",)),
    ((2, 128, 100, 40, 100), 4, False, {}, ("wide<128,4,chunks>a/w3/p1", "wide<128,8,chunks>b/w7/p1")),
    ((1, 96, 33, 176, 16), 4, False, {}, ("wide<96,8,one>a/w8/p2", "wide<96,4,one>b/w1/p1")),           # 11 tiles: 8 + 3
    ((1, 128, 52, 132, 16), 4, False, {}, ("wide<128,8,chunks>a/w8/p2", "wide<128,4,chunks>b/w1/p1")),  # 9 tiles: 8 + 1, two chunks
    ((1, 128, 40, 176, 16), 4, False, {}, ("wide<128,8,one>ab/w8/p2",)) + (True,),                        # the repair launch: both blocks
    ((1, 128, 33, 208, 16), 4, False, {}, ("!more than 192 padded keys in the fused backward",)),
    ((2, 96, 40, 40, 100), 4, True, {}, ("!wide heads take the fp32 views",)),
    ((1, 64, 33, 256, 256), 4, False, {}, ("!more than 192 padded keys in the fused backward",)),
    ((1, 96, 33, 0, 208), 6, False, {}, ("!more than 192 padded keys in the fused backward",)),
    ((2, 48, 33, 176, 32), 4, False, {}, ("!more than 192 padded keys in the fused backward",)),    # 11 + 2 tiles: each block fits, the sum does not
    ((2, 128, 33, 176, 32), 5, False, {}, ("!more than 192 padded keys in the fused backward",)),
    ((2, 48, 33, 176, 16), 4, False, {"ATT_STREAM": 1}, ("fused16<48,4,one>a/w4", "fused16<48,4,one>b/w1")),   # the knob does not reach phase 4
    ((2, 96, 33, 176, 16), 4, False, {"ATT_STREAM": 1}, ("wide<96,8,one>a/w8/p2", "wide<96,4,one>b/w1/p1")),
    ((2, 96, 40, 40, 100), 0, False, {}, ("dq<96,10>/wq3/hpb1", "dkv<96,3>/wq2/hpb1")),
    ((2, 96, 100, 40, 100), 0, False, {}, ("dq<96,10>/wq4/hpb1", "dkv<96,0>/wq2/hpb1")),                # 7 query tiles, four waves
    ((2, 48, 100, 40, 100), 2, False, {}, ("dq<48,10>/wq4/hpb1",)),
    ((2, 128, 40, 40, 100), 1, False, {"ATT_STREAM": 1}, ("D_stream<128>",)),
    ((1, 128, 17, 200, 9), 0, False, {}, ("dq_stream<128>/wq2/hpb1", "dkv<128,0>/wq2/hpb1")),
    ((2, 32, 20, 20, 12), 2, False, {"ATT_HPB_DQ": 2}, ("dq<32,4>/wq2/hpb2",)),
    ((2, 16, 17, 200, 9), 2, False, {"ATT_HPB_DQ": 2}, ("dq_stream<16>/wq2/hpb2",)),
    ((2, 96, 20, 20, 12), 3, False, {"ATT_HPB_DKV": 2}, ("dkv<96,0>/wq3/hpb1",)),                       # 2 x 3 waves > 4
    ((2, 96, 20, 20, 12), 3, False, {"ATT_HPB_DKV": 2 | 2 << 8}, ("dkv<96,0>/wq2/hpb2",)),
    ((2, 16, 17, 200, 9), 3, False, {"ATT_HPB_DKV": 2}, ("dkv<16,0>/wq4/hpb2",)),                       # 14 key tiles
    ((4, 4, 33, 5, 3), 3, False, {"ATT_HPB_DKV": 2 | 1 << 8}, ("dkv<4,3>/wq1/hpb2",)),
]


@pytest.mark.parametrize("row", FWD_TABLE_X, ids=lambda r: "%s-%s" % ("x".join(map(str, r[0])), ",".join("%s=%s" % kv for kv in r[1].items())))
def test_forward_launch_rule_agrees_with_the_table(row):
    (H, dh, Lq, La, Lb), knobs, want = row
    assert R.fwd_launch(H, dh, Lq, La, Lb, knobs=knobs) == want


@pytest.mark.parametrize("row", BWD_TABLE_X, ids=lambda r: "%s-ph%d-pin%d-%s" % ("x".join(map(str, r[0])), r[1], r[2], ",".join("%s=%s" % kv for kv in r[3].items())))
def test_backward_launch_rule_agrees_with_the_table(row):
    (H, dh, Lq, La, Lb), phase, pin, knobs, want = row[:5]
    assert R.bwd_launch(H, dh, Lq, La, Lb, phase, pin=pin, knobs=knobs, repair=len(row) > 5) == want


def test_the_launch_rule_is_the_instance_rule_for_narrow_heads():
    """fwd_launch / bwd_launch only ADD the workgroup shape to what fwd_instance / bwd_instance name at head dims <= 64"""
    for row in FWD_TABLE:
        (dh, Lq, La, Lb), pin, knobs, want = row
        assert R.fwd_launch(2, dh, Lq, La, Lb, pin=pin, knobs=knobs).split("/")[0] == want
    for row in BWD_TABLE:
        (dh, Lq, La, Lb), phase, mode, pin, knobs, want = row
        got = R.bwd_launch(2, dh, Lq, La, Lb, phase, mode=mode, pin=pin, knobs=knobs)
        assert tuple(n.split("/wq")[0] for n in got) == want
    assert R.attn_shape(7, 2, 12, 0) == (4, 1) and R.attn_shape(10, 2, 12, 0) == (5, 1) and R.attn_shape(9, 2, 12, 0) == (3, 1)
    assert R.attn_shape(9, 4, 12, 4) == (3, 4) and R.attn_shape(9, 4, 12, 4 | 2 << 8) == (2, 4) and R.attn_shape(3, 3, 5, 2) == (3, 1)
    assert R.launch_field("wide<96,8,one>a/w8/p2", "p") == 2 and R.launch_field("dq<32,4>/wq2/hpb2", "hpb") == 2
    assert R.launch_field("dq<32,4>/wq2/hpb2", "w") is None
