"""The yardstick of tests/test_rowops_gpu.py shown sound without a GPU (tests/rowops_ref.py): its float64 statements agree with
independent ones in torch, every bound accepts a faithful fp32 emulation of the kernels' documented summation order on every
input generator, every planted defect is rejected by at least one generator and case, and the generators are what they say."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import rowops_ref as R

F = np.float32
L1_DS = (4, 48, 260, 768, 1536, 2052, 4096)
COLSUM_MS = (1, 15, 16, 17, 300, 4097)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


# ------------------------------------------------------------------ the float64 statements against torch
@pytest.mark.parametrize("rows,d", [(7, 32), (11, 260)])
def test_layernorm_statement_is_torch_autograd(rows, d):
    """ln_fwd_ref / ln_bwd_ref with both dropout multipliers against float64 autograd of torch.nn.functional.layer_norm"""
    g = np.random.default_rng(d)
    x, dy = R.ln_rows(rows, d, 1), R.grad_rows(rows, d, 2)
    gamma, beta = (1 + 0.1 * g.standard_normal(d)).astype(F), (0.1 * g.standard_normal(d)).astype(F)
    my = np.where(g.random((rows, d)) < 0.1, 0.0, 1 / 0.9).astype(F)
    mb = np.where(g.random((rows, d)) < 0.1, 0.0, 1 / 0.9).astype(F)
    xr, gr, br = _t(x).requires_grad_(True), _t(gamma).requires_grad_(True), _t(beta).requires_grad_(True)
    y = torch.nn.functional.layer_norm(xr, (d,), gr, br, R.EPS_LN) * _t(my)
    y.backward(_t(dy))
    yr, _ = R.ln_fwd_ref(x, gamma, beta, my)
    r = R.ln_bwd_ref(dy, x, gamma, my, mb)
    scale = lambda t: 1e-12 * max(1.0, float(t.abs().max()))
    assert (torch.from_numpy(yr) - y.detach()).abs().max() <= scale(y.detach())
    assert (torch.from_numpy(r["dx"]) - xr.grad).abs().max() <= scale(xr.grad)
    assert (torch.from_numpy(r["dx_drop"]) - xr.grad * _t(mb)).abs().max() <= scale(xr.grad)
    assert (torch.from_numpy(r["dgamma"]) - gr.grad).abs().max() <= scale(gr.grad)
    assert (torch.from_numpy(r["dbeta"]) - br.grad).abs().max() <= scale(br.grad)
    assert np.abs(r["dsum"] - (xr.grad * _t(mb)).sum(0).numpy()).max() <= scale(xr.grad) * rows


def test_l1_and_sum_statements_are_torch():
    x = R.l1_rows(9, 260, 3)
    xt = _t(x)
    s, inv, y = R.l1_ref(x)
    want = xt / (xt.norm(p=1, dim=-1, keepdim=True) + 1e-6)
    assert np.abs(y - want.numpy()).max() <= 1e-15 and np.abs(inv * (s + 1e-6) - 1).max() <= 1e-15
    X, w, o = R.grad_rows(37, 12, 4), R.signed_rows(1, 37, 5)[0], R.signed_rows(1, 12, 6)[0]
    val, _ = R.colsum_ref(X, w, o)
    assert np.abs(val - ((_t(X) * _t(w)[:, None]).sum(0) + _t(o)).numpy()).max() <= 1e-12
    B, S, d = 5, 3, 8
    dpre = R.grad_rows(B * S, d + 4, 7)
    val, _ = R.pe_grad_ref(dpre, B, S, d)
    assert np.abs(val - _t(dpre)[:, :d].view(B, S, d).sum(0).numpy()).max() <= 1e-12
    part = R.grad_rows(41, 8, 8)
    val, _ = R.colsum_pos_ref(part, 7)
    for s_ in range(7):
        assert np.abs(val[s_] - _t(part)[s_::7].sum(0).numpy()).max() <= 1e-12
    val, _ = R.rowdot_ref(X, o, 0.375, w)
    assert np.abs(val - (_t(X) @ _t(o) + 0.375 + _t(w)).numpy()).max() <= 1e-12


@pytest.mark.parametrize("S", [1, 4])
def test_embedding_statements_are_torch(S):
    B, n_rows, dh = 37, 50, 8
    ids = R.id_list(B, n_rows, 9)
    ok = (ids >= 0) & (ids < n_rows)
    g = R.grad_rows(B * S, dh, 10)
    t0 = R.signed_rows(n_rows, dh, 11)
    val, _ = R.embed_bwd_ref(g, S, ids, t0)
    want = _t(t0)
    want.index_add_(0, torch.from_numpy(ids[ok]), _t(g).view(B, S, dh).sum(1)[torch.from_numpy(ok)])
    assert np.abs(val - want.numpy()).max() <= 1e-12
    z = R.zero_rows_ref(t0, ids)
    want = torch.from_numpy(t0.copy())
    want[torch.from_numpy(ids[ok])] = 0
    assert np.array_equal(z, want.numpy())
    table, fw, fb, pe = R.signed_rows(n_rows, dh, 12), R.signed_rows(1, dh, 13)[0], R.signed_rows(1, dh, 14)[0], R.signed_rows(S, 2 * dh, 15)
    val, bound, ok2 = R.embed_vid_ref(ids, table, fw, fb, pe, None, B, S)
    assert np.array_equal(ok, ok2) and np.isnan(val[~ok][:, :, :dh]).all() and np.isfinite(val[:, :, dh:]).all()
    emb = torch.nn.functional.embedding(torch.from_numpy(ids[ok]), _t(table))
    pos = torch.arange(S).double()
    want = torch.cat([emb[:, None, :].expand(-1, S, dh), (pos[:, None] * _t(fw) + _t(fb))[None].expand(int(ok.sum()), S, dh)], -1) + _t(pe)
    assert np.abs(val[ok] - want.numpy()).max() <= 1e-12
    assert (bound[:, :, :dh] == 0).all() and (bound[:, :, dh:] > 0).all()


# ------------------------------------------------------------------ bounds against the emulation and the planted defects
def _l1_cases():
    for D in L1_DS:
        for name, row in R.special_rows(D, 100 + D).items():
            yield "D=%d %s" % (D, name), row[None, :]


def _l1_ratios(x, got):
    s, inv, y = R.l1_ref(x)
    bs, bi, by = R.l1_bounds(x)
    return max(R.ratio(np.abs(got[0] - s), bs), R.ratio(np.abs(got[1] - inv), bi), R.ratio(np.abs(got[2] - y), by))


def _rowdot_cases():
    for d in (4, 260, 1024):
        x = R.l1_rows(6, d, 200 + d)
        w = R.signed_rows(1, d, 201 + d)[0]
        out0 = R.signed_rows(1, 6, 202 + d)[0]
        for bias in (None, 0.375):
            for o in (None, out0):
                yield "d=%d bias=%s accumulate=%d" % (d, bias, o is not None), x, w, bias, o


def _colsum_cases():
    for M in COLSUM_MS:
        N = 8
        X = R.l1_rows(M, N, 300 + M)
        w = R.signed_rows(1, M, 301 + M)[0]
        out0 = R.signed_rows(1, N, 302 + M)[0]
        for ww in (None, w):
            for o in (None, out0):
                yield "M=%d w=%d accumulate=%d" % (M, ww is not None, o is not None), X, ww, o


def test_bounds_accept_the_emulation_on_every_generator():
    worst = {"l1": 0.0, "rowdot": 0.0, "colsum": 0.0}
    for name, x in _l1_cases():
        got = R.emul_l1(x)
        r = _l1_ratios(x, got)
        assert r <= 1.0, ("l1", name, r)
        assert R.true_division_ok(x, got[0], got[2]), name
        worst["l1"] = max(worst["l1"], r)
    for name, x, w, bias, o in _rowdot_cases():
        val, bound = R.rowdot_ref(x, w, bias, o)
        r = R.ratio(np.abs(R.emul_rowdot(x, w, bias, o) - val), bound)
        assert r <= 1.0, ("rowdot", name, r)
        worst["rowdot"] = max(worst["rowdot"], r)
    for name, X, w, o in _colsum_cases():
        val, bound = R.colsum_ref(X, w, o)
        r = R.ratio(np.abs(R.emul_colsum(X, w, o) - val), bound)
        assert r <= 1.0, ("colsum", name, r)
        worst["colsum"] = max(worst["colsum"], r)
    print("unmodified emulation, worst error / bound:", {k: float("%.3g" % v) for k, v in worst.items()})
    assert all(v > 0 for v in worst.values())          # the emulations do round: the bounds were exercised, not met by exact sums


def test_every_planted_defect_is_rejected():
    """Each defect, applied to the emulation, leaves at least one generator and case outside its bound (or, for the product with
    the rounded reciprocal, off the bit pattern of the true division); the case that caught it is printed."""
    caught = {}
    for defect in R.DEFECTS_L1:
        where = caught.setdefault("l1: " + defect, [])
        for name, x in _l1_cases():
            got = R.emul_l1(x, defect)
            r = _l1_ratios(x, got)
            if r > 1.0:
                where.append((name, "error/bound %.3g" % r))
            elif not R.true_division_ok(x, R.emul_l1(x)[0], got[2]):
                where.append((name, "not the true division"))
    for defect in R.DEFECTS_ROWDOT:
        where = caught.setdefault("rowdot: " + defect, [])
        for name, x, w, bias, o in _rowdot_cases():
            val, bound = R.rowdot_ref(x, w, bias, o)
            r = R.ratio(np.abs(R.emul_rowdot(x, w, bias, o, defect) - val), bound)
            if r > 1.0:
                where.append((name, "error/bound %.3g" % r))
    for defect in R.DEFECTS_COLSUM:
        where = caught.setdefault("colsum: " + defect, [])
        for name, X, w, o in _colsum_cases():
            val, bound = R.colsum_ref(X, w, o)
            r = R.ratio(np.abs(R.emul_colsum(X, w, o, defect) - val), bound)
            if r > 1.0:
                where.append((name, "error/bound %.3g" % r))
    for defect, where in caught.items():
        print(defect, "rejected at", where[:4], "(%d cases)" % len(where))
        assert where, "defect %s passes everywhere: the inputs are too tame" % defect
    assert len(caught) == len(R.DEFECTS_L1) + len(R.DEFECTS_ROWDOT) + len(R.DEFECTS_COLSUM)


# ------------------------------------------------------------------ the generators are what they say
@pytest.mark.parametrize("D", L1_DS[1:])
def test_generators_meet_their_conditions(D):
    sp = R.special_rows(D, 7)
    for name in ("signed", "tiny", "span", "huge"):
        neg = float((sp[name] < 0).mean())
        assert 0.4 <= neg <= 0.6, (name, neg)
    assert not sp["zero"].any()
    tiny = float(np.abs(sp["tiny"].astype(np.float64)).sum())
    assert 0.5e-7 < tiny < 1e-6 and (sp["tiny"] != 0).all()
    mag = np.abs(sp["span"].astype(np.float64))
    assert mag.max() / mag.min() >= 2.0 ** 39
    mag = np.abs(sp["huge"].astype(np.float64))
    assert mag.max() >= 1e7 * np.sort(mag)[-2] and int(mag.argmax()) >= D - 4
    x = R.l1_rows(1027, D, 8)
    assert 0.4 <= float((x < 0).mean()) <= 0.6
    assert 0.4 <= float((R.signed_rows(5, D, 9) < 0).mean()) <= 0.6


def test_id_generator_meets_its_conditions():
    for n_rows in (5, 64, 1000):
        ids = R.id_list(37, n_rows, n_rows)
        assert ids.dtype == np.int64 and len(ids) == 37
        assert R.longest_run(ids) >= 9 and R.max_multiplicity(ids, n_rows) >= 12
        assert 0 in ids and n_rows - 1 in ids and -1 in ids and n_rows in ids and 10 ** 9 in ids


def test_launch_geometry_restated():
    """the chunk rule at its edges (segmm_colsum_chunks) and the LayerNorm-backward grid (segmm_layernorm_bwd_parts)"""
    assert [R.colsum_chunks(M) for M in (1, 15, 16, 17, 4096, 4097, 10 ** 6)] == [1, 1, 1, 2, 256, 256, 256]
    assert [R.colsum_rows_per_chunk(M) for M in (1, 15, 16, 17, 4096, 4097)] == [1, 15, 16, 9, 16, 17]
    assert R.ln_bwd_parts(1027, 768) == 257 and R.ln_bwd_parts(1027, 768, 64) == 64 and R.ln_bwd_parts(3, 2048) == 1
    assert R.ln_bwd_parts(20480, 768) == 768 and R.ln_bwd_parts(20480, 2048) == 256
    assert R.c_l1(768) == 18 and R.c_l1(4) == 10 and R.c_l1(2052) == 42
    assert R.c_colsum(4097) == 5 + 64 + 8 and R.c_vecsum(1025) == 2 + 22
