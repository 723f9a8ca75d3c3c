"""The streaming forms of the LayerNorm forward and the column sums change how loads are ISSUED and how often the maxima are committed,
never a bit of a result; the split-K combine's summation order is pinned beside them.

* LayerNorm forward: the row-walking form (layernorm_fwd_walk_kernel, knob LN_FWD_PARTS = 0 or a grid) against the one-wave-per-row
  form (LN_FWD_PARTS = 1) in one process, every output compared as integers -- y, the planes, the whole site header (scale, flag,
  maxima slots), the plain maxima slots, mean, rstd, dot_out -- and both against the float64 statement of tests/rowops_ref.py within
  the forward bound the existing row-kernel tests use.
* Column sums and the split-K combine: the summation ORDER restated below in numpy float32, one rounded add at a time (no pairwise
  np.sum): chunk, the four row lanes' stride, the four-way combine, then the final; the 16 row lanes of colsum_pos; slab order.  The
  kernels must give these bits.  (The restatements were held against the library of the commit BEFORE the loads were batched, so
  they state the order the project had, not the one this file arrived with.)  tests/test_row_stream_cpu.py holds the
  restatements against float64 without a GPU."""
import contextlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import rowops_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32


# ------------------------------------------------------------------ the summation orders, in fp32
def _chain(rows):
    """((0 + a) + b) + ... over the rows of a [k, N] fp32 matrix, one rounding per add"""
    acc = np.zeros(rows.shape[1:], F)
    for v in rows:
        acc = acc + v
    return acc


def f32_colsum_partials(X, w=None):
    """colsum_partial_kernel / colsum_partial3_kernel: [chunks, N].  Row lane ty of a chunk adds the rows r0 + ty, r0 + ty + 4, ... in
    order (each times w[r] first, the product rounded), then r0 + r1 + r2 + r3 left to right."""
    X = np.asarray(X, F)
    M, N = X.shape
    chunks = max(1, min(256, R.cdiv(M, 16)))
    rpc = max(1, R.cdiv(M, chunks))
    part = np.zeros((chunks, N), F)
    for ch in range(chunks):
        r0 = ch * rpc
        r1 = min(M, r0 + rpc)
        red = []
        for ty in range(4):
            idx = np.arange(r0 + ty, r1, 4)
            rows = X[idx] if w is None else (X[idx] * np.asarray(w, F)[idx, None]).astype(F)
            red.append(_chain(rows))
        part[ch] = ((red[0] + red[1]) + red[2]) + red[3]
    return part


def f32_colsum_final(part, out0=None):
    """colsum_final_kernel / colsum_final3_kernel: lane ty adds the partial rows ty, ty + 4, ...; (r0 + r1) + (r2 + r3); then + out"""
    part = np.asarray(part, F)
    red = [_chain(part[ty::4]) for ty in range(4)]
    s = (red[0] + red[1]) + (red[2] + red[3])
    if out0 is not None:
        s = s + np.asarray(out0, F)
    return s.astype(F)


def f32_colsum(X, w=None, out0=None):
    return f32_colsum_final(f32_colsum_partials(X, w), out0)


def f32_colsum_pos(part, period):
    """colsum_pos_kernel: row lane ty of 16 adds the rows s + period ty, + 16 period, ...; lane 0 then adds the 16 partials in lane order"""
    part = np.asarray(part, F)
    P, N = part.shape
    out = np.zeros((period, N), F)
    for s in range(period):
        red = [_chain(part[s + period * ty::16 * period]) for ty in range(16)]
        t = red[0]
        for k in range(1, 16):
            t = t + red[k]
        out[s] = t
    return out


def f32_splitk(slabs, c0=None):
    """splitk_reduce: slab 0, then + slab 1, + slab 2, ... in slab order; then + C under accumulate"""
    slabs = np.asarray(slabs, F)
    s = slabs[0].copy()
    for z in range(1, slabs.shape[0]):
        s = s + slabs[z]
    if c0 is not None:
        s = s + np.asarray(c0, F)
    return s.astype(F)


def f32_splitk_cs(cs_ws, out0=None):
    """the folded column sums: 0 + slab 0 + slab 1 + ...; cs_out + s under accumulate"""
    s = _chain(np.asarray(cs_ws, F))
    if out0 is not None:
        s = np.asarray(out0, F) + s
    return s.astype(F)


def tn_splits(K, splits):
    """the split count segmm_gemm_p runs with: whole 32-row k tiles per split, no empty split"""
    ktiles = R.cdiv(K, 32)
    splits = min(splits, ktiles)
    if splits <= 1:
        return 1
    tps = R.cdiv(ktiles, splits)
    return R.cdiv(ktiles, tps)


# LayerNorm forward, row-walking form: workgroups of one round (capi.hip ln_fwd_cap; 0: the form is not taken)
def ln_fwd_cap(d, dot):
    if d > 1024:
        return 0
    if dot:
        return 2048 if d <= 256 else 1280 if d <= 512 else 1024
    return 2048 if d <= 256 else 1536 if d <= 512 else 1280 if d <= 768 else 1024


# ------------------------------------------------------------------ plumbing
def _abi():
    from segmminterest_amd import hipabi
    hipabi.lib()
    return hipabi


def _torch():
    import torch
    return torch


@contextlib.contextmanager
def _knob(H, name, value):
    prev = H.config_set(name, value)
    try:
        yield
    finally:
        H.config_set(name, prev)


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).to(DEV)


def _host(t):
    _torch().cuda.synchronize()
    return t.detach().cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 2: np.int16}[a.dtype.itemsize])


def _same(a, b):
    return a.shape == b.shape and bool((_bits(a) == _bits(b)).all())


def _pattern(shape, seed):
    return np.random.default_rng(2000 + seed).standard_normal(shape).astype(F)


# ------------------------------------------------------------------ LayerNorm forward: the two forms
LN_DS = [32, 260, 768, 1024]          # V = 1, 2, 3, 4 (2048, V = 8, keeps the one-wave-per-row form: nothing to compare)
P_DROP, SEED, SITE = 0.1, 5, 11
PLANE_SCALE = 2.0 ** 8                # |y| <= (1.4 sqrt(d) + 0.4) / 0.9 < 52 at d <= 1024: inside the fp16 window


def _ln_launch(H, case, pat, xd, gd, bd, wd, dbd, rows, d):
    """one launch of case = (with_y, with_planes, drop_p, dot) into pattern-filled buffers -> dict of host arrays (guards included)"""
    torch = _torch()
    with_y, with_pl, drop_p, dot = case
    bufs = {k: _dev(v) for k, v in pat.items()}
    po = amax = None
    if with_pl:
        bufs["hdr"] = H.new_site(DEV)[0]
        bufs["planes"] = torch.zeros((rows + 1, 2 * d), dtype=torch.float16, device=DEV)
        sc = torch.tensor([PLANE_SCALE], dtype=torch.float32, device=DEV)
        po = H.PO(bufs["planes"], 2 * d, bufs["hdr"], sc.data_ptr())
    else:
        bufs["amax"] = torch.zeros(H.SITE_FLOATS, dtype=torch.float32, device=DEV)
        amax = bufs["amax"]
    y = bufs["y"] if with_y else None
    kw = dict(drop_p=drop_p, seed=SEED, site=SITE, amax=amax, po=po)
    if dot:
        H.layernorm_fwd_dot(xd, gd, bd, y, bufs["mean"], bufs["rstd"], wd, dbd, bufs["dot"], **kw)
    else:
        H.layernorm_fwd(xd, gd, bd, y, bufs["mean"], bufs["rstd"], **kw)
    return {k: _host(v) for k, v in bufs.items()}


@pytest.mark.parametrize("rows_kind", ["1", "3", "5", "1027", "resident+1"])
@pytest.mark.parametrize("d", LN_DS)
def test_layernorm_fwd_forms_same_bits(d, rows_kind):
    """Walking form on its default grid and on 64 workgroups (every wave walks several rows at 1027 rows and up) against the
    one-wave-per-row form: every output as int32, guards included; y and mean of both against float64 (y: the forward bound of
    rowops_ref; mean: a chain of 4 ceil(d / 256) + 6 adds and the division on mean|x|).  rows = one more than the waves of a full
    round: exactly one wave walks a second row."""
    H = _abi()
    torch = _torch()
    rows = 4 * ln_fwd_cap(d, False) + 1 if rows_kind == "resident+1" else int(rows_kind)
    n = rows * d
    g = np.random.default_rng(d + rows)
    x = R.ln_rows(rows, d, d + rows)
    gamma, beta = (1 + 0.1 * g.standard_normal(d)).astype(F), (0.1 * g.standard_normal(d)).astype(F)
    w, db = (0.05 * g.standard_normal(d)).astype(F), np.array([0.375], F)
    xd, gd, bd, wd, dbd = _dev(x), _dev(gamma), _dev(beta), _dev(w), _dev(db)
    mult = torch.empty(n, device=DEV)
    H.dropout_mult(mult, n, P_DROP, SEED, SITE)
    mult = _host(mult).reshape(rows, d)
    refs = {0.0: R.ln_fwd_ref(x, gamma, beta), P_DROP: R.ln_fwd_ref(x, gamma, beta, mult)}
    mean64 = R.ln_stats(x)[0]
    b_mean = (4 * R.cdiv(d, 256) + 7) * R.U * np.abs(x.astype(np.float64)).mean(1)
    pat = {"y": _pattern(n + d + 16, 1), "mean": _pattern(rows + 5, 2), "rstd": _pattern(rows + 5, 3), "dot": _pattern(rows + 5, 4)}
    planes_ok = d % 32 == 0
    cases = [(wy, wp, p, dot) for wy, wp in ((True, False), (True, True), (False, True)) for p in (0.0, P_DROP) for dot in (False, True)
             if planes_ok or not wp]
    # 64 workgroups: a wave stride of 256 rows, every row of a wave in ONE maxima slot (a running maximum, one commit per wave);
    # 100 workgroups: a stride of 400 rows, the slots differ from row to row (one commit per row, as in the old form)
    grids = (1, 0, 64, 100) if rows > 256 else (1, 0)
    for case in cases:
        with_y, with_pl, drop_p, dot = case
        outs = {}
        for knob in grids:
            with _knob(H, "LN_FWD_PARTS", knob):
                outs[knob] = _ln_launch(H, case, pat, xd, gd, bd, wd, dbd, rows, d)
        for knob in grids[1:]:
            for k, v in outs[1].items():
                assert _same(v, outs[knob][k]), "d=%d rows=%d case=%s LN_FWD_PARTS=%d: %s differs from the one-wave-per-row form" % (d, rows, case, knob, k)
        for knob in grids:
            o = outs[knob]
            what = "d=%d rows=%d case=%s LN_FWD_PARTS=%d" % (d, rows, case, knob)
            if with_y:
                want, bound = refs[drop_p]
                r = R.ratio(np.abs(o["y"][:n].reshape(rows, d).astype(np.float64) - want), bound)
                assert r <= 1.0, "%s: y error / bound %.3g" % (what, r)
                assert _same(o["y"][n:], pat["y"][n:]), what
            else:
                assert _same(o["y"], pat["y"]), what
            assert R.ratio(np.abs(o["mean"][:rows].astype(np.float64) - mean64), b_mean) <= 1.0, what
            assert _same(o["mean"][rows:], pat["mean"][rows:]) and _same(o["rstd"][rows:], pat["rstd"][rows:]), what
            assert _same(o["dot"][rows:] if dot else o["dot"], pat["dot"][rows:] if dot else pat["dot"]), what
            if with_pl:
                assert not o["planes"][rows:].view(np.int16).any(), what          # the guard row after the planes


# ------------------------------------------------------------------ column sums: the kernels give the restated bits
CS_MS = [1, 15, 17, 100, 4097]
CS_NS = [4, 260, 768]


@pytest.mark.parametrize("N", CS_NS)
@pytest.mark.parametrize("M", CS_MS)
def test_colsum_restated_bits(M, N):
    """plain, weighted, a column slice of a wider matrix (x_off), accumulate -- the workspace holds the restated partials as well"""
    H = _abi()
    chunks = H.colsum_chunks(M)
    w = R.signed_rows(1, M, seed=M)[0]
    wd = _dev(w)
    for ld, x_off in ((N, 0), (2 * N + 8, N + 4)):
        Xb = R.grad_rows(M, ld, seed=M + N + ld)
        Xd = _dev(Xb)
        X = Xb[:, x_off:x_off + N]
        for use_w in (False, True):
            part = f32_colsum_partials(X, w if use_w else None)
            assert part.shape[0] == chunks
            for acc in (False, True):
                o0, ws0 = _pattern(N + 8, 12 + acc), _pattern(chunks * N + 16, 14)
                od, wsd = _dev(o0), _dev(ws0)
                H.colsum(Xd, ld, M, N, od, wsd, w=wd if use_w else None, accumulate=acc, x_off=x_off)
                o, ws = _host(od), _host(wsd)
                what = "M=%d N=%d ld=%d w=%d acc=%d" % (M, N, ld, use_w, acc)
                assert _same(ws[:chunks * N].reshape(chunks, N), part) and _same(ws[chunks * N:], ws0[chunks * N:]), what
                assert _same(o[:N], f32_colsum_final(part, o0[:N] if acc else None)) and _same(o[N:], o0[N:]), what


@pytest.mark.parametrize("nmat", [1, 2, 3])
@pytest.mark.parametrize("N", CS_NS)
@pytest.mark.parametrize("M", CS_MS)
def test_colsum3_restated_bits(M, N, nmat):
    H = _abi()
    chunks = H.colsum_chunks(M)
    Xs = [R.grad_rows(M, N, seed=M + N + k) for k in range(nmat)]
    o0 = [_pattern(N + 8, 15 + k) for k in range(nmat)]
    ws0 = _pattern(3 * chunks * N + 16, 18)
    ods, wsd = [_dev(o) for o in o0], _dev(ws0)
    H.colsum3([_dev(X) for X in Xs], N, M, N, ods, wsd)
    ws = _host(wsd)
    assert _same(ws[3 * chunks * N:], ws0[3 * chunks * N:])
    for k in range(nmat):
        part = f32_colsum_partials(Xs[k])
        assert _same(ws[k * chunks * N:(k + 1) * chunks * N].reshape(chunks, N), part), "M=%d N=%d matrix %d of %d: partials" % (M, N, k, nmat)
        o = _host(ods[k])
        assert _same(o[:N], f32_colsum_final(part)) and _same(o[N:], o0[k][N:]), "M=%d N=%d matrix %d of %d" % (M, N, k, nmat)


@pytest.mark.parametrize("N", [4, 260])
@pytest.mark.parametrize("P,period", [(7, 1), (1000, 1), (41, 40), (1000, 40), (100, 100), (1700, 100)])
def test_colsum_pos_restated_bits(P, period, N):
    """P is no multiple of 16 period: row lanes with unequal (and zero) row counts; 1000 rows at period 1: 62 or 63 rows per lane
    (seven full rounds of eight loads and a remainder)"""
    H = _abi()
    assert P % (16 * period) != 0
    part = R.grad_rows(P, N, seed=P + period + N)
    o0 = _pattern((period + 1) * N + 16, 19)
    od = _dev(o0)
    H.colsum_pos(_dev(part), period, od)
    o = _host(od)
    assert _same(o[period * N:], o0[period * N:])
    assert _same(o[:period * N].reshape(period, N), f32_colsum_pos(part, period)), "P=%d period=%d N=%d" % (P, period, N)


# ------------------------------------------------------------------ split-K combine through the plane TN GEMM
@pytest.mark.parametrize("splits", [2, 5, 7, 28])
@pytest.mark.parametrize("M,N,K", [(128, 256, 96), (256, 256, 2048)])
def test_splitk_reduce_restated_bits(M, N, K, splits):
    """C and the folded column sums are the slabs the GEMM left in the workspace, added in slab order (then + C / + cs_out under
    accumulate).  28 splits of 64 k tiles run as 22 (five rounds of four loads and a remainder of one); 2 .. 7: one round or the
    remainder alone.  splitk_reduce itself kept its form (batching eight loads showed no gain, profiles/README.md): this pins the order
    for whoever tries again."""
    H = _abi()
    torch = _torch()
    eff = tn_splits(K, splits)
    g = np.random.default_rng(M + K + splits)
    dY, X = _dev((0.01 * g.standard_normal((K, M))).astype(F)), _dev(g.standard_normal((K, N)).astype(F))
    pdy, px = H.to_planes(dY, K, M), H.to_planes(X, K, N)
    for with_cs in (False, True):
        for acc in (False, True):
            c0, cs0 = _pattern((M, N), 20 + acc), _pattern(M + 8, 22 + acc)
            C, cs = _dev(c0), _dev(cs0)
            ws = torch.zeros(splits * (M * N + M) + 16, device=DEV)
            H.gemm_p(H.LAYOUT_TN, M, N, K, pdy, px, C, N, splits=splits, workspace=ws, colsum_out=cs if with_cs else None, accumulate=acc)
            wsh = _host(ws)
            what = "M=%d N=%d K=%d splits=%d (%d) colsum_out=%d accumulate=%d" % (M, N, K, splits, eff, with_cs, acc)
            slabs = wsh[:eff * M * N].reshape(eff, M, N)
            assert _same(_host(C), f32_splitk(slabs, c0 if acc else None)), what
            csh = _host(cs)
            if with_cs:
                cs_ws = wsh[eff * M * N:eff * (M * N + M)].reshape(eff, M)
                assert _same(csh[:M], f32_splitk_cs(cs_ws, cs0[:M] if acc else None)) and _same(csh[M:], cs0[M:]), what
            else:
                assert _same(csh, cs0), what
    ref = _host(dY).astype(np.float64).T @ _host(X).astype(np.float64)
    C = _dev(np.zeros((M, N), F))
    H.gemm_p(H.LAYOUT_TN, M, N, K, pdy, px, C, N, splits=splits, workspace=torch.zeros(splits * (M * N + M), device=DEV))
    assert float(np.abs(_host(C) - ref).max() / np.abs(ref).max()) < 3e-6          # (the slabs are a weight gradient at all)
