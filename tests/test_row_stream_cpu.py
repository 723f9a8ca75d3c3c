"""Without a GPU: the fp32 restatements of tests/test_row_stream_gpu.py (the summation orders the column-sum kernels and the split-K
combine must reproduce bit for bit) agree with float64 sums within the chain bounds of tests/rowops_ref.py -- c u sum|terms|, far
inside "a few ulp x M" -- and catch a planted change of order; the committed compiler report (profiles/row_stream/
resource_usage.txt) shows no scratch and no spill for any instance of the changed kernels, and the LayerNorm forward's grid table in
capi.hip is 256 CUs x the occupancy that report lists."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import rowops_ref as R
import test_row_stream_gpu as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.mark.parametrize("N", [4, 260])
@pytest.mark.parametrize("M", [1, 15, 17, 100, 4097])
def test_colsum_restatement_against_float64(M, N):
    X = R.grad_rows(M, N, seed=M + N)
    w = R.signed_rows(1, M, seed=M)[0]
    out0 = np.random.default_rng(M).standard_normal(N).astype(F)
    for use_w in (None, w):
        for acc in (None, out0):
            want, bound = R.colsum_ref(X, use_w, acc)
            got = G.f32_colsum(X, use_w, acc)
            assert got.dtype == F and R.ratio(np.abs(got.astype(np.float64) - want), bound) <= 1.0
    # the order matters at these sizes: the plain row chain gives other bits (what the GPU test would see of a reordered kernel)
    if M >= 100:
        plain = G._chain(X)
        assert not np.array_equal(plain.view(np.int32), G.f32_colsum(X).view(np.int32))


@pytest.mark.parametrize("P,period", [(7, 1), (1000, 1), (41, 40), (1000, 40), (100, 100), (1700, 100)])
def test_colsum_pos_restatement_against_float64(P, period):
    part = R.grad_rows(P, 260, seed=P + period)
    want, bound = R.colsum_pos_ref(part, period)
    got = G.f32_colsum_pos(part, period)
    assert got.dtype == F and R.ratio(np.abs(got.astype(np.float64) - want), bound) <= 1.0


@pytest.mark.parametrize("splits", [2, 5, 7, 22])
def test_splitk_restatement_against_float64(splits):
    """a chain over the slabs (and + C): c = splits + 1 on sum|terms|"""
    g = np.random.default_rng(splits)
    slabs, c0, cs = R.grad_rows(splits, 1028, seed=splits).reshape(splits, 4, 257), g.standard_normal((4, 257)).astype(F), R.grad_rows(splits, 64, seed=9)
    for acc in (None, c0):
        want = slabs.astype(np.float64).sum(0) + (0 if acc is None else acc.astype(np.float64))
        mag = np.abs(slabs.astype(np.float64)).sum(0) + (0 if acc is None else np.abs(acc.astype(np.float64)))
        got = G.f32_splitk(slabs, acc)
        assert got.dtype == F and R.ratio(np.abs(got.astype(np.float64) - want), (splits + 1) * R.U * mag) <= 1.0
    got = G.f32_splitk_cs(cs, c0[0, :64])
    want = cs.astype(np.float64).sum(0) + c0[0, :64]
    mag = np.abs(cs.astype(np.float64)).sum(0) + np.abs(c0[0, :64].astype(np.float64))
    assert R.ratio(np.abs(got.astype(np.float64) - want), (splits + 1) * R.U * mag) <= 1.0


def test_split_count_rule():
    """segmm_gemm_p's effective split count at the GPU test's shapes: whole k tiles, no empty split"""
    assert [G.tn_splits(96, s) for s in (2, 5, 7, 28)] == [2, 3, 3, 3]
    assert [G.tn_splits(2048, s) for s in (2, 5, 7, 28)] == [2, 5, 7, 22]


# ------------------------------------------------------------------ the committed resource report
def _resource_table():
    rows = {}
    with open(os.path.join(ROOT, "profiles", "row_stream", "resource_usage.txt")) as f:
        for line in f:
            if line.startswith("#") or line.startswith("kernel") or not line.strip():
                continue
            m = re.match(r"(.+?)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s*$", line)
            assert m, line
            rows[m.group(1).strip()] = dict(zip(("sgprs", "vgprs", "agprs", "scratch", "occupancy", "lds", "spills"), map(int, m.groups()[1:])))
    return rows


def test_no_instance_uses_scratch():
    t = _resource_table()
    want = ["colsum_partial_kernel", "colsum_final_kernel", "colsum_partial3_kernel", "colsum_final3_kernel", "colsum_pos_kernel", "splitk_reduce"]
    want += ["layernorm_fwd_walk_kernel<%d, %s>" % (v, b) for v in (1, 2, 3, 4) for b in ("false", "true")]
    for name in want:
        assert name in t, "%s is missing from profiles/row_stream/resource_usage.txt" % name
    for name, r in t.items():
        assert r["scratch"] == 0 and r["spills"] == 0, "%s: scratch %d B/lane, %d spilled VGPRs" % (name, r["scratch"], r["spills"])
    assert not any(n.startswith("layernorm_fwd_walk_kernel<8") for n in t)          # V = 8 keeps the one-wave-per-row form


def test_layernorm_fwd_grid_table_matches_the_report():
    """one round = 256 CUs x the waves per SIMD of the instance (a four-wave workgroup puts one wave on each SIMD of its CU); the
    table as capi.hip states it, as the GPU test restates it, and as the report implies it"""
    t = _resource_table()
    src = open(os.path.join(ROOT, "segmminterest_amd", "csrc", "capi.hip")).read()
    body = src[src.index("static int ln_fwd_cap("):]
    body = body[:body.index("\n}\n")]
    m_dot = re.search(r"if \(dot\) return d <= 256 \? (\d+) : d <= 512 \? (\d+) : (\d+);", body)
    m_pl = re.search(r"return d <= 256 \? (\d+) : d <= 512 \? (\d+) : d <= 768 \? (\d+) : (\d+);", body)
    assert m_dot and m_pl, "ln_fwd_cap no longer has the form this test reads"
    dot = list(map(int, m_dot.groups())) + [int(m_dot.group(3))]          # d <= 768 and d <= 1024 share the last entry
    plain = list(map(int, m_pl.groups()))
    for k, (v, d) in enumerate(((1, 256), (2, 512), (3, 768), (4, 1024))):
        assert plain[k] == 256 * t["layernorm_fwd_walk_kernel<%d, false>" % v]["occupancy"] == G.ln_fwd_cap(d, False)
        assert dot[k] == 256 * t["layernorm_fwd_walk_kernel<%d, true>" % v]["occupancy"] == G.ln_fwd_cap(d, True)
    assert G.ln_fwd_cap(2048, False) == 0 and "d > 1024) return 0" in body
