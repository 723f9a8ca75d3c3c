"""The row kernels of csrc/rowops.h that the older tests only touch at one shape -- L1 normalisation (loop and register forms),
the feature gather of csrc/evalops.h, the dropout streams and partial sums of the LayerNorm backward, the column sums, the
Linear(d, 1) head helpers and the id-embedding kernels -- against the float64 statements of tests/rowops_ref.py, within the
bounds derived there (c u sum|terms|, c counted on the documented reduction shape; see that module's docstring: no tolerance
here is a bare constant).  Every output buffer is pre-filled with a recorded random pattern and every element outside the
documented output region -- rows past ``rows``, columns between d and ld, a pad after the end -- is compared bit for bit afterwards.
Run with ``pytest -m gpu -s`` to see the worst error / bound per kernel (SEGMM_ROWOPS_RATIO_LOG=path writes them to a file);
tests/test_rowops_cpu.py shows without a GPU that the bounds accept a faithful fp32 emulation and reject planted defects."""
import contextlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import rowops_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
RATIOS = {}


def _abi():
    from segmminterest_amd import hipabi
    hipabi.lib()
    return hipabi


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    lines = ["%-22s worst error / bound %.3g" % (k, v) for k, v in sorted(RATIOS.items())]
    print("\n" + "\n".join(lines))
    path = os.environ.get("SEGMM_ROWOPS_RATIO_LOG")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


@contextlib.contextmanager
def _knob(H, name, value):
    prev = H.config_set(name, value)
    try:
        yield
    finally:
        H.config_set(name, prev)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 2: np.uint16, 1: np.uint8, 8: np.uint64}[a.dtype.itemsize])


def _same(a, b):
    return a.shape == b.shape and bool((_bits(a) == _bits(b)).all())


def _pattern(shape, seed):
    """the recorded random fill of an output buffer (and the previous contents under ``accumulate``)"""
    return np.random.default_rng(1000 + seed).standard_normal(shape).astype(F)


def _within(kernel, got, want, bound, what=""):
    with np.errstate(all="ignore"):
        err = np.abs(np.asarray(got, np.float64) - want)
    r = R.ratio(err, bound)
    RATIOS[kernel] = max(RATIOS.get(kernel, 0.0), r)
    assert r <= 1.0, "%s %s: error / bound = %.4g" % (kernel, what, r)


# ------------------------------------------------------------------ L1 normalisation
L1_DS = [4, 48, 256, 260, 512, 768, 1024, 1028, 1536, 2048, 2052, 4096]          # V = 1, 1, 1, 2, 2, 3, 4, 6, 6, 8 | loop, loop


def _l1_run(H, xd, rows, D, with_y, with_inv, po=None):
    """-> (y [rows, D] or None, inv [rows] or None); guards checked"""
    n = rows * D
    y0, i0 = _pattern(n + 2 * D + 16, 1), _pattern(rows + 5, 2)
    yd, idv = _dev(y0), _dev(i0)
    H.l1norm(xd, yd if with_y else None, idv if with_inv else None, po=po)
    y, inv = _host(yd), _host(idv)
    assert _same(y[n:], y0[n:]) and _same(inv[rows:], i0[rows:])
    if not with_y:
        assert _same(y, y0)
    if not with_inv:
        assert _same(inv, i0)
    return (y[:n].reshape(rows, D) if with_y else None), (inv[:rows] if with_inv else None)


@pytest.mark.parametrize("rows", [1, 5, 1027])
@pytest.mark.parametrize("D", L1_DS)
def test_l1norm(D, rows):
    """Signed rows, a zero row, a row whose 1e-6 matters, a row spanning 2^40 and a row with one huge entry, in every register
    form (V = 1, 2, 3, 4, 6, 8, full and partial last groups) and the loop form (D > 2048, or knob L1NORM_REG = 0).  y and
    inv_scale within the float64 bound AND bit for bit the fp32 emulation of the documented order (per-lane stride-256 float4
    walk, xor butterfly, ONE true division); the three output modes, the two forms and the run with a plane output agree bit for bit."""
    H = _abi()
    x = R.l1_rows(rows, D, seed=D + rows)
    xd = _dev(x)
    s64, inv64, y64 = R.l1_ref(x)
    _, b_inv, b_y = R.l1_bounds(x)
    out = {}
    for reg in (1, 0):
        with _knob(H, "L1NORM_REG", reg):
            y, inv = _l1_run(H, xd, rows, D, True, True)
            _within("l1norm y", y, y64, b_y, "D=%d rows=%d reg=%d" % (D, rows, reg))
            _within("l1norm inv_scale", inv, inv64, b_inv, "D=%d rows=%d reg=%d" % (D, rows, reg))
            _, inv_only = _l1_run(H, xd, rows, D, False, True)
            y_only, _ = _l1_run(H, xd, rows, D, True, False)
            assert _same(inv_only, inv) and _same(y_only, y)
            out[reg] = (y, inv)
    assert _same(out[0][0], out[1][0]) and _same(out[0][1], out[1][1])          # "element for element the arithmetic of l1norm_kernel"
    es, einv, ey = R.emul_l1(x)
    assert _same(out[1][1], einv) and _same(out[1][0], ey)
    assert R.true_division_ok(x, es, out[1][0])
    if D % 32 == 0:
        scale = 2.0 ** 13          # |y| <= 1: the planes' high halves stay below 2^13
        for reg in (1, 0):
            with _knob(H, "L1NORM_REG", reg):
                hdr = H.new_site(DEV)[0]
                sc = torch.tensor([scale], dtype=torch.float32, device=DEV)
                pl = torch.zeros((rows, 2 * D), dtype=torch.float16, device=DEV)
                y, inv = _l1_run(H, xd, rows, D, True, True, po=H.PO(pl, 2 * D, hdr, sc.data_ptr()))
                assert _same(y, out[1][0]) and _same(inv, out[1][1])
                hdr2 = H.new_site(DEV)[0]
                hdr2[0] = scale
                pl2 = torch.empty((rows, 2 * D), dtype=torch.float16, device=DEV)
                H.split_p32(_dev(y), rows, D, D, pl2, 2 * D, hdr2, mode=1)
                assert _same(_host(pl).view(np.uint16), _host(pl2).view(np.uint16)) and float(hdr[0]) == scale


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("D", [4, 260, 768, 1536])
def test_gather_l1(D, normalize):
    """Signed table rows (the special rows among them); indices -1, n_lines, 10^9 (padding: exact zeros, mask 0), row 0 and the
    last row.  Not normalised: the table rows bit for bit; normalised: within the L1 bound and bit for bit segmm_l1norm of the
    gathered rows (the same per-lane order and division)."""
    H = _abi()
    n_lines, rows = 23, 21
    table = R.l1_rows(n_lines, D, seed=D)
    idx = np.random.default_rng(D).integers(0, n_lines, rows).astype(np.int64)
    idx[[0, 1, 2, 3, 4, 5, 6, 7, 8]] = [-1, n_lines, 10 ** 9, 0, n_lines - 1, 1, 2, 3, 4]
    ok = (idx >= 0) & (idx < n_lines)
    n = rows * D
    o0, m0 = _pattern(n + 2 * D + 16, 3), np.full(rows + 8, 7, np.uint8)
    od, md, td = _dev(o0), _dev(m0), _dev(table)
    H.gather_l1(td, _dev(idx.reshape(3, 7)), normalize=normalize, out=od, mask=md)
    o, m = _host(od), _host(md)
    assert _same(o[n:], o0[n:]) and _same(m[rows:], m0[rows:])
    assert np.array_equal(m[:rows], ok.astype(np.uint8))
    o = o[:n].reshape(rows, D)
    assert not _bits(o[~ok]).any()          # +0.0 in every padded element
    g = table[idx[ok]]
    if not normalize:
        assert _same(o[ok], g)
        return
    _, _, y64 = R.l1_ref(g)
    _within("gather_l1", o[ok], y64, R.l1_bounds(g)[2], "D=%d" % D)
    y = torch.empty(g.shape, dtype=torch.float32, device=DEV)
    H.l1norm(_dev(g), y)
    assert _same(o[ok], _host(y))


# ------------------------------------------------------------------ LayerNorm backward and forward with dropout
LN_DS = [32, 260, 768, 1024, 1280, 2048]          # V = 1, 2, 3, 4, 8, 8
P_DROP, SEED, SITE_Y, SITE_B = 0.1, 3, 9, 4


def _mult(H, n, site):
    m = torch.empty(n, device=DEV)
    H.dropout_mult(m, n, P_DROP, SEED, site)
    return _host(m)


def _ln_inputs(H, rows, d, seed):
    g = np.random.default_rng(seed)
    x, dy = R.ln_rows(rows, d, seed), R.grad_rows(rows, d, seed + 1)
    gamma, beta = (1 + 0.1 * g.standard_normal(d)).astype(F), (0.1 * g.standard_normal(d)).astype(F)
    xd, gd, bd = _dev(x), _dev(gamma), _dev(beta)
    y, mean, rstd = torch.empty(rows, d, device=DEV), torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
    H.layernorm_fwd(xd, gd, bd, y, mean, rstd)
    return x, dy, gamma, beta, xd, _dev(dy), gd, bd, mean, rstd


def _ln_bwd_run(H, rows, d, parts, dyd, xd, mean, rstd, gd, pos=None):
    """one backward launch with both dropout streams, dx_drop and part_dsum; -> host dx, dx_drop, the three partial matrices
    [parts, d] (and part_pos [4 parts, d] on the per-position grid, ``pos`` = period); guards checked"""
    n = rows * d
    bufs0 = [_pattern(n + d + 16, 4), _pattern(n + d + 16, 5)] + [_pattern((parts + 1) * d, 6 + k) for k in range(3)]
    bufs = [_dev(b) for b in bufs0]
    kw = dict(drop_y_p=P_DROP, drop_y_site=SITE_Y, drop_b_p=P_DROP, drop_b_site=SITE_B, seed=SEED, part_dsum=bufs[4])
    if pos is None:
        H.layernorm_bwd(dyd, xd, mean, rstd, gd, bufs[0], bufs[1], bufs[2], bufs[3], **kw)
    else:
        pp0 = _pattern((4 * parts + 1) * d, 9)
        ppd = _dev(pp0)
        H.layernorm_bwd_pos(dyd, xd, mean, rstd, gd, bufs[0], bufs[1], bufs[2], bufs[3], ppd, pos, **kw)
    got = [_host(b) for b in bufs]
    for k in (0, 1):
        assert _same(got[k][n:], bufs0[k][n:])
    for k in (2, 3, 4):
        assert _same(got[k][parts * d:], bufs0[k][parts * d:])
    res = [got[0][:n].reshape(rows, d), got[1][:n].reshape(rows, d)] + [got[k][:parts * d].reshape(parts, d) for k in (2, 3, 4)]
    if pos is not None:
        pp = _host(ppd)
        assert _same(pp[4 * parts * d:], pp0[4 * parts * d:])
        res.append((ppd, pp[:4 * parts * d].reshape(4 * parts, d)))
    return res


def _ln_bwd_check(ref, mb, rows, parts, dx, dxd, pg, pb, ps, what):
    _within("layernorm_bwd dx", dx, ref["dx"], ref["b_dx"], what)
    _within("layernorm_bwd dx_drop", dxd, ref["dx_drop"], ref["b_dx_drop"], what)
    keep = mb != 0
    assert not _bits(dxd[~keep]).any() and _same(dxd[keep], (dx * mb)[keep])          # dx_drop = dx x mask: one fp32 product
    b_g, b_b, b_s = R.ln_part_bounds(ref, rows, parts)
    _within("layernorm_bwd dgamma", pg.astype(np.float64).sum(0), ref["dgamma"], b_g, what)
    _within("layernorm_bwd dbeta", pb.astype(np.float64).sum(0), ref["dbeta"], b_b, what)
    _within("layernorm_bwd dsum", ps.astype(np.float64).sum(0), ref["dsum"], b_s, what)


@pytest.mark.parametrize("rows", [3, 1027])
@pytest.mark.parametrize("d", LN_DS)
def test_layernorm_bwd_dropout_streams_and_partials(d, rows):
    """Both dropout streams (masks from segmm_dropout_mult, applied by the float64 reference), dx_drop and the three partial
    matrices, on the default grid and with LN_BWD_PARTS = 64 (1027 rows: 64 workgroups, every wave walks 4 or 5 rows with
    running accumulators); dx is bit-identical between the two grids."""
    H = _abi()
    x, dy, gamma, beta, xd, dyd, gd, bd, mean, rstd = _ln_inputs(H, rows, d, seed=d + rows)
    my, mb = _mult(H, rows * d, SITE_Y).reshape(rows, d), _mult(H, rows * d, SITE_B).reshape(rows, d)
    assert set(np.unique(my)) <= {F(0), my.max()} and 0.05 < float((mb == 0).mean()) < 0.2 and not np.array_equal(my, mb)
    ref = R.ln_bwd_ref(dy, x, gamma, my, mb)
    dxs = []
    for knob in (0, 64):
        with _knob(H, "LN_BWD_PARTS", knob):
            parts = H.layernorm_bwd_parts(rows, d)
            assert parts == R.ln_bwd_parts(rows, d, knob)
            if knob and rows > 1000:
                assert parts == 64 and R.cdiv(rows, 4 * parts) >= 4          # multi-row waves
            dx, dxd, pg, pb, ps = _ln_bwd_run(H, rows, d, parts, dyd, xd, mean, rstd, gd)
        _ln_bwd_check(ref, mb, rows, parts, dx, dxd, pg, pb, ps, "d=%d rows=%d LN_BWD_PARTS=%d" % (d, rows, knob))
        dxs.append(dx)
    assert _same(dxs[0], dxs[1])


@pytest.mark.parametrize("B,L", [(9, 7), (64, 1), (26, 40)])
@pytest.mark.parametrize("d", [260, 768])
def test_layernorm_bwd_pos_with_dropout(d, B, L):
    """The per-position grid with both dropout streams: everything the plain entry leaves (dx bit for bit), and the positional
    sums sum_b dx[b, s, :] through part_pos + segmm_colsum_pos."""
    H = _abi()
    rows = B * L
    x, dy, gamma, beta, xd, dyd, gd, bd, mean, rstd = _ln_inputs(H, rows, d, seed=d + rows)
    my, mb = _mult(H, rows * d, SITE_Y).reshape(rows, d), _mult(H, rows * d, SITE_B).reshape(rows, d)
    ref = R.ln_bwd_ref(dy, x, gamma, my, mb)
    parts0 = H.layernorm_bwd_parts(rows, d)
    dx0 = _ln_bwd_run(H, rows, d, parts0, dyd, xd, mean, rstd, gd)[0]
    parts = H.layernorm_bwd_pos_parts(rows, L, d)
    assert parts > 0 and (4 * parts) % L == 0
    dx, dxd, pg, pb, ps, (ppd, pp) = _ln_bwd_run(H, rows, d, parts, dyd, xd, mean, rstd, gd, pos=L)
    what = "d=%d B=%d L=%d" % (d, B, L)
    _ln_bwd_check(ref, mb, rows, parts, dx, dxd, pg, pb, ps, what)
    assert _same(dx, dx0)
    o0 = _pattern((L + 1) * d, 10)
    od = _dev(o0)
    H.colsum_pos(ppd[:4 * parts * d].view(4 * parts, d), L, od)
    o = _host(od)
    assert _same(o[L * d:], o0[L * d:])
    want, bound = R.pos_sum_ref(ref, B, L, rows, parts)
    _within("layernorm_bwd_pos sums", o[:L * d].reshape(L, d), want, bound, what)


@pytest.mark.parametrize("d", LN_DS)
def test_layernorm_fwd_dropout(d):
    """y = LN64(x) x mask within the forward bound; the elements the mask drops are exact zeros."""
    H = _abi()
    rows = 5
    g = np.random.default_rng(d)
    x = R.ln_rows(rows, d, d)
    gamma, beta = (1 + 0.1 * g.standard_normal(d)).astype(F), (0.1 * g.standard_normal(d)).astype(F)
    n = rows * d
    y0 = _pattern(n + d + 16, 11)
    yd, mean, rstd = _dev(y0), torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
    H.layernorm_fwd(_dev(x), _dev(gamma), _dev(beta), yd, mean, rstd, drop_p=P_DROP, seed=SEED, site=SITE_Y)
    m = _mult(H, n, SITE_Y).reshape(rows, d)
    y = _host(yd)
    assert _same(y[n:], y0[n:])
    y = y[:n].reshape(rows, d)
    want, bound = R.ln_fwd_ref(x, gamma, beta, m)
    _within("layernorm_fwd dropout", y, want, bound, "d=%d" % d)
    assert (m == 0).any() and not _bits(y[m == 0]).any()


# ------------------------------------------------------------------ column sums
COLSUM_MS = [1, 15, 16, 17, 4096, 4097]          # the chunk rule's edges: 1 chunk of M rows up to 16, 2 x 9, 256 x 16, 256 x 17
COLSUM_NS = [4, 252, 256, 260, 1028]


@pytest.mark.parametrize("N", COLSUM_NS)
@pytest.mark.parametrize("M", COLSUM_MS)
def test_colsum(M, N):
    """Contiguous [M, N] and the column slice [:, N + 4 : 2 N + 4] of an [M, 2 N + 8] matrix (engine._embed_bwd's form), with and
    without the row weight and ``accumulate``, into out_off > 0 of a longer vector."""
    H = _abi()
    chunks = H.colsum_chunks(M)
    assert chunks == R.colsum_chunks(M)
    w = R.signed_rows(1, M, seed=M)[0]
    wd = _dev(w)
    for ld, x_off, out_off in ((N, 0, 0), (2 * N + 8, N + 4, 8)):
        Xb = R.grad_rows(M, ld, seed=M + N + ld)
        Xd = _dev(Xb)
        X = Xb[:, x_off:x_off + N]
        for use_w in (False, True):
            for acc in (False, True):
                o0, ws0 = _pattern(out_off + N + 8, 12 + acc), _pattern(chunks * N + 16, 14)
                od, wsd = _dev(o0), _dev(ws0)
                H.colsum(Xd, ld, M, N, od, wsd, w=wd if use_w else None, accumulate=acc, x_off=x_off, out_off=out_off)
                o, ws = _host(od), _host(wsd)
                keep = np.ones(o.shape, bool)
                keep[out_off:out_off + N] = False
                assert _same(o[keep], o0[keep]) and _same(ws[chunks * N:], ws0[chunks * N:])
                want, bound = R.colsum_ref(X, w if use_w else None, o0[out_off:out_off + N] if acc else None)
                _within("colsum", o[out_off:out_off + N], want, bound, "M=%d N=%d ld=%d w=%d acc=%d" % (M, N, ld, use_w, acc))


@pytest.mark.parametrize("nmat", [1, 2, 3])
@pytest.mark.parametrize("N", COLSUM_NS)
@pytest.mark.parametrize("M", COLSUM_MS)
def test_colsum3(M, N, nmat):
    H = _abi()
    chunks = H.colsum_chunks(M)
    Xs = [R.grad_rows(M, N, seed=M + N + k) for k in range(nmat)]
    o0 = [_pattern(N + 8, 15 + k) for k in range(nmat)]
    ws0 = _pattern(3 * chunks * N + 16, 18)
    ods, wsd = [_dev(o) for o in o0], _dev(ws0)
    H.colsum3([_dev(X) for X in Xs], N, M, N, ods, wsd)
    assert _same(_host(wsd)[3 * chunks * N:], ws0[3 * chunks * N:])
    for k in range(nmat):
        o = _host(ods[k])
        assert _same(o[N:], o0[k][N:])
        want, bound = R.colsum_ref(Xs[k])
        _within("colsum3", o[:N], want, bound, "M=%d N=%d matrix %d of %d" % (M, N, k, nmat))


@pytest.mark.parametrize("N", [4, 260])
@pytest.mark.parametrize("P,period", [(P, s) for P in (7, 40, 41, 640, 1000) for s in (1, 7, 40) if s <= P])
def test_colsum_pos(P, period, N):
    """out[s, :] = sum of the partial rows p = s (mod period), directly on a random partial matrix: from one row per position
    (P = period) to 1000 (16 row lanes walking 63 rows each), positions with unequal row counts (41 rows, period 7 or 40)."""
    H = _abi()
    part = R.grad_rows(P, N, seed=P + period + N)
    o0 = _pattern((period + 1) * N + 16, 19)
    od = _dev(o0)
    H.colsum_pos(_dev(part), period, od)
    o = _host(od)
    assert _same(o[period * N:], o0[period * N:])
    want, bound = R.colsum_pos_ref(part, period)
    _within("colsum_pos", o[:period * N].reshape(period, N), want, bound, "P=%d period=%d N=%d" % (P, period, N))


# ------------------------------------------------------------------ head helpers
@pytest.mark.parametrize("rows", [1, 5, 1027])
@pytest.mark.parametrize("d", [4, 32, 260, 1024])
def test_rowdot_and_rowscale_bcast_strided(d, rows):
    """x[:, 4 : 4 + d] of an [rows, d + 12] matrix, w at offset 4 of a longer vector, dx at column offset 8; bias present and
    None; accumulate 0 and 1.  rowscale_bcast without accumulate is ONE fp32 product: bit for bit."""
    H = _abi()
    ld, x_off, w_off, dx_off = d + 12, 4, 4, 8
    xb, wb = _pattern((rows, ld), 20), _pattern(d + 8, 21)
    xb[:, x_off:x_off + d] = R.l1_rows(rows, d, seed=d + rows)
    x, w = xb[:, x_off:x_off + d], wb[w_off:w_off + d]
    bias = np.array([0.375], F)
    xd, wd, biasd = _dev(xb), _dev(wb), _dev(bias)
    for use_b in (False, True):
        for acc in (False, True):
            o0 = _pattern(rows + 5, 22 + acc)
            od = _dev(o0)
            H.rowdot(xd, ld, wd, biasd if use_b else None, od, rows, d, accumulate=acc, x_off=x_off, w_off=w_off)
            o = _host(od)
            assert _same(o[rows:], o0[rows:])
            want, bound = R.rowdot_ref(x, w, 0.375 if use_b else None, o0[:rows] if acc else None)
            _within("rowdot", o[:rows], want, bound, "d=%d rows=%d bias=%d acc=%d" % (d, rows, use_b, acc))
    g = R.signed_rows(1, rows, seed=rows)[0]
    gd = _dev(g)
    for acc in (False, True):
        d0 = _pattern((rows + 1, ld), 24 + acc)
        dd = _dev(d0)
        H.rowscale_bcast(gd, wd, dd, ld, rows, d, accumulate=acc, w_off=w_off, dx_off=dx_off)
        got = _host(dd)
        keep = np.ones(d0.shape, bool)
        keep[:rows, dx_off:dx_off + d] = False
        assert _same(got[keep], d0[keep])
        reg = got[:rows, dx_off:dx_off + d]
        if acc:
            want, bound = R.rowscale_ref(g, w, d0[:rows, dx_off:dx_off + d])
            _within("rowscale_bcast", reg, want, bound, "d=%d rows=%d accumulate" % (d, rows))
        else:
            assert _same(reg, g[:, None] * w[None, :])


@pytest.mark.parametrize("acc", [False, True])
@pytest.mark.parametrize("n", [1, 63, 64, 1023, 1024, 1025, 100003])
def test_vecsum(n, acc):
    H = _abi()
    v = R.grad_rows(1, n, seed=n)[0]
    vd = _dev(v)
    o0 = _pattern(4, 26)
    runs = []
    for _ in range(2):
        od = _dev(o0)
        H.vecsum(vd, n, od, accumulate=acc)
        o = _host(od)
        assert _same(o[1:], o0[1:])
        runs.append(o[:1])
    assert _same(runs[0], runs[1])          # one workgroup, a fixed order: deterministic
    want, bound = R.vecsum_ref(v, o0[0] if acc else None)
    _within("vecsum", runs[0][0], want, bound, "n=%d acc=%d" % (n, acc))


# ------------------------------------------------------------------ id embedding
EMB_DS = [8, 64, 520, 1024]          # d / 2 = 4 (one float4: the other lanes idle), 32, 260 (a second, partial pass of the 64 lanes), 512 (two full passes)
EMB_B = 37


@pytest.mark.parametrize("with_pos", [False, True])
@pytest.mark.parametrize("with_pe", [False, True])
@pytest.mark.parametrize("S", [1, 20])
@pytest.mark.parametrize("d", EMB_DS)
def test_embed_id_forward(d, S, with_pe, with_pos):
    """embed_id_vid: the table half is ONE fp32 add (table[id] + pe: bit for bit), the frame half fw pos + fb + pe within 2 u of
    its terms; rows whose id lies outside the table are NaN in the table half only.  embed_id_usr: table[id] + pe[0] bit for bit."""
    H = _abi()
    B, dh, n_items, n_users = EMB_B, d // 2, 50, 24
    g = np.random.default_rng(d + S)
    ids = R.id_list(B, n_items, seed=d)
    table, fw, fb = R.signed_rows(n_items, dh, d + 1), R.signed_rows(1, dh, d + 2)[0], R.signed_rows(1, dh, d + 3)[0]
    pe = R.signed_rows(S, d, d + 4) if with_pe else None
    fpos = g.permutation(B * S).astype(F) if with_pos else None
    n = B * S * d
    o0 = _pattern(n + d + 16, 27)
    od = _dev(o0)
    H.embed_id_vid(_dev(ids), _dev(table), dh, _dev(fw), _dev(fb), None if pe is None else _dev(pe), od, B, S,
                   frame_pos=None if fpos is None else _dev(fpos))
    o = _host(od)
    assert _same(o[n:], o0[n:])
    o = o[:n].reshape(B, S, d)
    want, bound, ok = R.embed_vid_ref(ids, table, fw, fb, pe, fpos, B, S)
    assert (~ok).sum() == 3 and np.isnan(o[~ok][:, :, :dh]).all() and np.isfinite(o[ok]).all()
    exact = table[ids[ok]][:, None, :] + (pe[None, :, :dh] if with_pe else np.zeros((1, S, dh), F))
    assert _same(o[ok][:, :, :dh], exact.astype(F))
    _within("embed_id_vid frame half", o[:, :, dh:], want[:, :, dh:], bound[:, :, dh:], "d=%d S=%d pe=%d pos=%d" % (d, S, with_pe, with_pos))
    if S == 1 and not with_pos:
        uids = R.id_list(B, n_users, seed=d + 5)
        utable = R.signed_rows(n_users, d, d + 6)
        u0 = _pattern((B + 1) * d + 16, 28)
        ud = _dev(u0)
        H.embed_id_usr(_dev(uids), _dev(utable), d, None if pe is None else _dev(pe), ud, B)
        u = _host(ud)
        assert _same(u[B * d:], u0[B * d:])
        u = u[:B * d].reshape(B, d)
        uok = (uids >= 0) & (uids < n_users)
        assert np.isnan(u[~uok]).all()
        assert _same(u[uok], (utable[uids[uok]] + (pe[0][None] if with_pe else np.zeros((1, d), F))).astype(F))


def _embed_bwd_case(H, name, dpre, tok, ld, col0, width, order, ids, n_rows, zero_table):
    t0 = np.zeros((n_rows + 1, width), F) if zero_table else _pattern((n_rows + 1, width), 29)
    t0[n_rows] = _pattern(width, 30)          # the guard row after the table
    td = _dev(t0)
    H.embed_id_bwd(_dev(dpre), tok, ld, col0, width, _dev(order), _dev(ids), td[:n_rows], len(ids))
    t = _host(td)
    want, bound = R.embed_bwd_ref(dpre.reshape(-1, ld)[:, col0:col0 + width], tok, ids, t0[:n_rows])
    _within("embed_id_bwd", t[:n_rows], want, bound, name)
    hit = np.zeros(n_rows + 1, bool)
    hit[ids[(ids >= 0) & (ids < n_rows)]] = True
    assert hit.sum() < n_rows and _same(t[~hit], t0[~hit])          # untouched rows and the guard row


@pytest.mark.parametrize("S", [1, 20])
@pytest.mark.parametrize("d", EMB_DS)
def test_embed_id_bwd_both_engine_forms(d, S):
    """Dense table gradient against float64 index_add_ (tests/test_rowops_cpu.py ties the statement to torch's): the form over
    the token gradient (tokens_per_row = S, ld = d, the stable argsort of the ids; both halves of a row through col0) and the
    form over pre-summed rows (tokens_per_row = 1, ld = width, identity order), into a zero and into a non-zero table; a run of
    12 equal ids, the first and the last table row, ids outside the table skipped."""
    H = _abi()
    B, width, n_rows = EMB_B, d // 2, 50
    ids = R.id_list(B, n_rows, seed=d + S)
    dpre = R.grad_rows(B * S, d, seed=d + S + 1)
    order = torch.argsort(torch.from_numpy(ids), stable=True).to(torch.int32).numpy()
    for col0 in (0, width):
        for zero_table in (True, False):
            _embed_bwd_case(H, "tokens d=%d S=%d col0=%d zero=%d" % (d, S, col0, zero_table), dpre, S, d, col0, width, order, ids,
                            n_rows, zero_table)
    # pre-summed rows, identity order: equal ids are then only found when adjacent -- the list is sorted first, as the engine's is
    srt = np.sort(ids, kind="stable")
    pre = R.grad_rows(B, width, seed=d + S + 2)
    for zero_table in (True, False):
        _embed_bwd_case(H, "pre-summed d=%d zero=%d" % (d, zero_table), pre, 1, width, 0, width, np.arange(B, dtype=np.int32), srt,
                        n_rows, zero_table)
        # ... and the unsorted list with its argsort, as the data-parallel exchange hands the gathered rows over
        _embed_bwd_case(H, "pre-summed, argsort d=%d zero=%d" % (d, zero_table), pre, 1, width, 0, width, order, ids, n_rows, zero_table)


@pytest.mark.parametrize("width", [4, 256, 260, 512])
def test_zero_rows(width):
    """Listed rows become exact zeros (duplicates, the first and the last row); ids outside the table are skipped; every other row
    and the guard after the table keep their bits; an empty list is a no-op."""
    H = _abi()
    n_rows = 50
    ids = R.id_list(EMB_B, n_rows, seed=width)
    t0 = _pattern((n_rows + 1, width), 31)
    td = _dev(t0)
    H.zero_rows(td[:n_rows], _dev(ids))
    t = _host(td)
    want = np.concatenate([R.zero_rows_ref(t0[:n_rows], ids), t0[n_rows:]])
    assert _same(t, want) and not _bits(t[0]).any() and not _bits(t[n_rows - 1]).any() and _same(t[n_rows], t0[n_rows])
    td = _dev(t0)
    H.zero_rows(td[:n_rows], torch.empty(0, dtype=torch.int64, device=DEV))
    assert _same(_host(td), t0)


@pytest.mark.parametrize("acc", [False, True])
@pytest.mark.parametrize("d", [4, 260])
@pytest.mark.parametrize("S", [1, 33])
@pytest.mark.parametrize("B", [1, 7])
def test_pe_grad(B, S, d, acc):
    """dpe[s, :] (+)= sum_b dpre[b S + s, :d] with ld = d + 8: a chain over the batch, (B + 1) u sum|terms|."""
    H = _abi()
    ld = d + 8
    dpre = R.grad_rows(B * S, ld, seed=B + S + d)
    o0 = _pattern((S + 1) * d + 16, 32 + acc)
    od = _dev(o0)
    H.pe_grad(_dev(dpre), ld, B, S, d, od, accumulate=acc)
    o = _host(od)
    assert _same(o[S * d:], o0[S * d:])
    want, bound = R.pe_grad_ref(dpre, B, S, d, o0[:S * d].reshape(S, d) if acc else None)
    _within("pe_grad", o[:S * d].reshape(S, d), want, bound, "B=%d S=%d d=%d acc=%d" % (B, S, d, acc))
