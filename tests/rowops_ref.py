"""The row, column-sum and id-embedding kernels of csrc/rowops.h and the feature gather of csrc/evalops.h, restated on the host:
a float64 statement of every operation (written from the definitions in the kernels' header comments, not from their loops), an
error bound per output, fixed-seed input generators, fp32 emulations of three reductions in their documented summation order,
and a list of planted defects.  Shared by test_rowops_cpu.py (the yardstick shown sound without a GPU) and test_rowops_gpu.py.

Error bounds.  u = 2^-24 is the unit roundoff of fp32.  A sum of n terms evaluated in fp32 along ANY tree whose longest chain of
roundings from a term to the result is c satisfies |computed - exact| <= c u sum|terms| to first order in u (each rounding
multiplies what passes through it by (1 + delta), |delta| <= u; a term passes through at most c of them).  Every bound below is
c u sum|terms| with c counted on the documented reduction shape:

* one wave per row, lane l walks the float4 groups at columns 4 l, 4 l + 256, ...: ceil(D / 256) groups, each group costs three
  adds inside the group and one into the running sum: 4 ceil(D / 256) roundings; then the six-step xor butterfly of wave_sum:
      L1 sum:               c = 4 ceil(D / 256) + 6
      1 / (sum + 1e-6):     c + 3   (1e-6 as an fp32 constant, the add, the division)
      x / (sum + 1e-6):     c + 3   (the same denominator, one true division)
      rowdot:               c + 3   (the rounding of each product, the bias add, the accumulate add) on sum|x w| + |bias| + |out|
* column sums, segmm_colsum_chunks(M) chunks of rows_per_chunk = ceil(M / chunks) rows: four row lanes per column walk
  ceil(rows_per_chunk / 4) rows each, then the second launch walks ceil(chunks / 4) partials per lane; the constant covers the
  row-weight product (1), the two four-lane combines (3 + 2), the accumulate add (1) and one spare:
      colsum / colsum3:     c = ceil(rows_per_chunk / 4) + ceil(chunks / 4) + 8
      colsum_pos:           c = ceil(ceil(P / period) / 16) + 16   (16 row lanes per position, then 15 adds in lane order, 1 spare)
* vecsum, one workgroup of 1024 threads: ceil(n / 1024) adds per thread, the butterfly, 16 wave partials in order (15 adds and
  the accumulate add):      c = ceil(n / 1024) + 6 + 16
* pe_grad: a chain over the batch:                 c = B + 1 (accumulate)
* embed_id_bwd: a chain over the run of equal ids x the tokens per row, then the add into the table:   c = run S + 1
* rowscale_bcast with accumulate: the product and the add:   c = 2 on |g w| + |dx|; without accumulate ONE fp32 product: exact.
* embed_id_vid's frame half: fw pos + fb + pe in fp32: one fused multiply-add (the compiler's default contraction of
  ``fw * pos + fb``), then the add of pe: u |fw pos + fb| + u |fw pos + fb + pe| <= 2 u (|fw pos| + |fb| + |pe|); the table
  half is one add: bit-exact in fp32.

LayerNorm (the conditioning argument of tests/test_head_gpu.py): the row mean is a sum of d <= 2048 values in chains of at most
4 x 8 + 6 = 38 roundings, error <= 38 u |mean| < 2^-18.7 |mean|; (x - mean) rstd carries that times rstd.  Forward: 2^-16 per unit
of (1 + |mean| rstd) (max|gamma| + max|beta| scale); backward dx: three such products and two row means, 2^-14 per unit of
rstd max|gamma dy| (1 + |mean| rstd).  dx_drop = dx m (ONE fp32 product with the dropout multiplier m in {0, 1 / (1 - p)}):
the dx bound times m plus u |dx_drop|.  The partial sums (summed over the partial rows in float64 by the test): a wave adds the
ceil(rows / (4 parts)) rows it walks, the workgroup adds its four waves: c = ceil(rows / (4 parts)) + 3 + 2 (the products that
form a term) on sum|terms|, plus the error the terms themselves carry: sum|dy| 2^-16 (1 + |mean| rstd) for d gamma (xhat is a
forward quantity), the dx_drop bounds summed over the rows for the column sums of dx_drop, nothing for d beta."""
import numpy as np

U = 2.0 ** -24
F = np.float32
EPS_LN = 1e-12
L1_EPS = 1e-6


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------ launch geometry restated (capi.hip)
def colsum_chunks(M):
    """segmm_colsum_chunks: at least 16 rows per chunk, at most 256 chunks."""
    return max(1, min(256, cdiv(M, 16)))


def colsum_rows_per_chunk(M):
    return max(1, cdiv(M, colsum_chunks(M)))


def ln_bwd_cap(d, knob=0):
    if knob >= 64:
        return knob
    return 1024 if d <= 512 else 768 if d <= 768 else 512 if d <= 1024 else 256


def ln_bwd_parts(rows, d, knob=0):
    """segmm_layernorm_bwd_parts"""
    return max(1, min(cdiv(rows, 4), ln_bwd_cap(d, knob)))


# ------------------------------------------------------------------ chain lengths
def c_l1(D):
    return 4 * cdiv(D, 256) + 6


def c_rowdot(d):
    return c_l1(d) + 3


def c_colsum(M):
    return cdiv(colsum_rows_per_chunk(M), 4) + cdiv(colsum_chunks(M), 4) + 8


def c_colsum_pos(P, period):
    return cdiv(cdiv(P, period), 16) + 16


def c_vecsum(n):
    return cdiv(n, 1024) + 6 + 16


def c_ln_parts(rows, parts):
    return cdiv(rows, 4 * parts) + 3 + 2


# ------------------------------------------------------------------ generators (fixed seeds)
def _signs(g, rows, D):
    """+-1 [rows, D], D // 2 of each row negative, at random places (so that a short row is balanced too)"""
    base = np.where(np.arange(D) < D // 2, -1.0, 1.0)
    return np.stack([g.permutation(base) for _ in range(rows)])


def signed_rows(rows, D, seed):
    """|N(0, 1)| with balanced random signs: half the entries of every row negative."""
    g = np.random.default_rng(seed)
    return (np.abs(g.standard_normal((rows, D))) * _signs(g, rows, D)).astype(F)


def zero_row(D):
    return np.zeros(D, F)


def tiny_row(D, seed):
    """signed, sum|x| about 1e-7: the 1e-6 of the denominator is ten times the sum"""
    r = signed_rows(1, D, seed)[0].astype(np.float64)
    return (r * (1e-7 / np.abs(r).sum())).astype(F)


def span_row(D, seed):
    """signed, magnitudes 2^e with e uniform in [-20, 20]: about 2^40 between the smallest and the largest"""
    g = np.random.default_rng(seed)
    e = g.uniform(-20.0, 20.0, D)
    e[0], e[-1] = -20.0, 20.0
    return (_signs(g, 1, D)[0] * 2.0 ** e).astype(F)


def huge_row(D, seed):
    """N(0, 1) with ONE entry of -3e8 (in the last float4 group: a tail lane of the walk when D % 256 != 0)"""
    r = signed_rows(1, D, seed)[0]
    r[D - 2] = F(-3e8)
    return r


SPECIAL = ("signed", "zero", "tiny", "span", "huge")


def special_rows(D, seed):
    """{generator name: one row [D]}"""
    return {"signed": signed_rows(1, D, seed)[0], "zero": zero_row(D), "tiny": tiny_row(D, seed + 1), "span": span_row(D, seed + 2),
            "huge": huge_row(D, seed + 3)}


def l1_rows(rows, D, seed):
    """[rows, D]: signed rows; from 5 rows on, rows 1..4 are the zero, tiny, span and huge rows."""
    x = signed_rows(rows, D, seed)
    if rows >= 5:
        sp = special_rows(D, seed)
        for k, name in enumerate(SPECIAL[1:]):
            x[1 + k] = sp[name]
    return x


def ln_rows(rows, d, seed):
    """N(0.3, 2) rows; every 5th row sits at a common offset of +-300 with spread 0.5 (|mean| >> spread)."""
    g = np.random.default_rng(seed)
    x = g.standard_normal((rows, d)) * 2 + 0.3
    for r in range(4, rows, 5):
        x[r] = (300.0 if r % 2 == 0 else -300.0) + 0.5 * g.standard_normal(d)
    return x.astype(F)


def grad_rows(rows, d, seed):
    """N(0, 1) x log-normal: a gradient with a wide spread of magnitudes"""
    g = np.random.default_rng(seed)
    return (g.standard_normal((rows, d)) * np.exp(g.standard_normal((rows, d)))).astype(F)


def id_list(B, n_rows, seed):
    """int64 [B], B >= 24: ten equal ids in a row, the same id twice more further on, the first and the last table row, three
    ids outside the table (-1, n_rows, 10^9), the rest random."""
    assert B >= 24 and n_rows >= 4
    g = np.random.default_rng(seed)
    ids = g.integers(0, n_rows, B).astype(np.int64)
    rep = int(n_rows // 2)
    ids[3:13] = rep
    ids[B - 1] = rep
    ids[B - 4] = rep
    ids[0], ids[1] = 0, n_rows - 1
    ids[14], ids[15], ids[16] = -1, n_rows, 10 ** 9
    return ids


def longest_run(ids):
    best = run = 1
    for a, b in zip(ids[:-1], ids[1:]):
        run = run + 1 if a == b else 1
        best = max(best, run)
    return best


def max_multiplicity(ids, n_rows):
    ok = ids[(ids >= 0) & (ids < n_rows)]
    return int(np.bincount(ok).max()) if ok.size else 0


# ------------------------------------------------------------------ float64 statements and bounds
def l1_ref(x):
    """-> (sum|x| [rows], 1 / (sum|x| + 1e-6) [rows], x / (sum|x| + 1e-6) [rows, D]) in float64"""
    x = np.asarray(x, np.float64)
    s = np.abs(x).sum(-1)
    return s, 1.0 / (s + L1_EPS), x / (s + L1_EPS)[..., None]


def l1_bounds(x):
    """-> (bound of the sum, of the reciprocal scale, of the normalised elements)"""
    s, inv, y = l1_ref(x)
    c = c_l1(np.shape(x)[-1])
    return c * U * s, (c + 3) * U * inv, (c + 3) * U * np.abs(y)


def rowdot_ref(x, w, bias=None, out0=None):
    """out[m] = x[m, :] . w (+ bias) (+ out0[m]); -> (value, bound)"""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    val, mag = x @ w, np.abs(x) @ np.abs(w)
    if bias is not None:
        val, mag = val + float(bias), mag + abs(float(bias))
    if out0 is not None:
        val, mag = val + np.asarray(out0, np.float64), mag + np.abs(np.asarray(out0, np.float64))
    return val, c_rowdot(x.shape[1]) * U * mag


def rowscale_ref(g, w, dx0=None):
    """dx[m, :] = g[m] w (+ dx0[m, :]); -> (value, bound); without dx0 the fp32 product is exact: compare bits with fp32 g * w"""
    p = np.asarray(g, np.float64)[:, None] * np.asarray(w, np.float64)[None, :]
    if dx0 is None:
        return p, U * np.abs(p)
    d0 = np.asarray(dx0, np.float64)
    return p + d0, 2 * U * (np.abs(p) + np.abs(d0))


def vecsum_ref(v, out0=None):
    v = np.asarray(v, np.float64)
    val, mag = v.sum(), np.abs(v).sum()
    if out0 is not None:
        val, mag = val + float(out0), mag + abs(float(out0))
    return val, c_vecsum(v.size) * U * mag


def colsum_ref(X, w=None, out0=None):
    """out[n] = sum_m w[m] X[m, n] (+ out0[n]); -> (value, bound)"""
    X = np.asarray(X, np.float64)
    if w is not None:
        X = X * np.asarray(w, np.float64)[:, None]
    val, mag = X.sum(0), np.abs(X).sum(0)
    if out0 is not None:
        val, mag = val + np.asarray(out0, np.float64), mag + np.abs(np.asarray(out0, np.float64))
    return val, c_colsum(X.shape[0]) * U * mag


def colsum_pos_ref(part, period):
    """out[s, :] = sum of the rows p = s (mod period) of part [P, N]; -> (value [period, N], bound)"""
    part = np.asarray(part, np.float64)
    P, N = part.shape
    val, mag = np.zeros((period, N)), np.zeros((period, N))
    for p in range(P):
        val[p % period] += part[p]
        mag[p % period] += np.abs(part[p])
    return val, c_colsum_pos(P, period) * U * mag


def pe_grad_ref(dpre, B, S, d, dpe0=None):
    """dpe[s, :] = sum_b dpre[b S + s, :d] (+ dpe0); dpre [B S, ld]; -> (value, bound)"""
    t = np.asarray(dpre, np.float64)[:, :d].reshape(B, S, d)
    val, mag = t.sum(0), np.abs(t).sum(0)
    if dpe0 is not None:
        val, mag = val + np.asarray(dpe0, np.float64), mag + np.abs(np.asarray(dpe0, np.float64))
    return val, (B + 1) * U * mag


def embed_vid_ref(item_id, table, fw, fb, pe, frame_pos, B, S):
    """vid[b, s, :] = cat(table[item_id[b]], fw pos[b, s] + fb) + pe[s], pos[b, s] = s unless given.
    -> (value [B, S, d] float64 with NaN in the table half of rows whose id is outside the table, bound [B, S, d]: 0 on the table
    half (one fp32 add: the test compares bits with the fp32 sum), 2 u (|fw pos| + |fb| + |pe|) on the frame half, ok [B] bool)"""
    table, fw, fb = np.asarray(table, np.float64), np.asarray(fw, np.float64), np.asarray(fb, np.float64)
    n_rows, dh = table.shape
    pos = np.broadcast_to(np.arange(S, dtype=np.float64), (B, S)) if frame_pos is None else np.asarray(frame_pos, np.float64).reshape(B, S)
    pe_ = np.zeros((S, 2 * dh)) if pe is None else np.asarray(pe, np.float64)
    ok = (item_id >= 0) & (item_id < n_rows)
    val, bound = np.empty((B, S, 2 * dh)), np.zeros((B, S, 2 * dh))
    for b in range(B):
        val[b, :, :dh] = (table[item_id[b]] if ok[b] else np.nan) + pe_[:, :dh]
        val[b, :, dh:] = pos[b][:, None] * fw + fb + pe_[:, dh:]
        bound[b, :, dh:] = 2 * U * (np.abs(pos[b][:, None] * fw) + np.abs(fb) + np.abs(pe_[:, dh:]))
    return val, bound, ok


def embed_bwd_ref(rows_grad, tokens_per_row, ids, dtable0):
    """dtable[ids[b], :] += sum over the tokens of batch row b of rows_grad [B tokens_per_row, width]; ids outside the table are
    skipped.  -> (value, bound) with c = (largest multiplicity of an id) x tokens_per_row + 1"""
    g = np.asarray(rows_grad, np.float64)
    B = len(ids)
    width = g.shape[1]
    g = g.reshape(B, tokens_per_row, width)
    val, mag = np.array(dtable0, np.float64), np.abs(np.array(dtable0, np.float64))
    n_rows = val.shape[0]
    for b in range(B):
        if 0 <= ids[b] < n_rows:
            val[ids[b]] += g[b].sum(0)
            mag[ids[b]] += np.abs(g[b]).sum(0)
    return val, (max_multiplicity(np.asarray(ids), n_rows) * tokens_per_row + 1) * U * mag


def zero_rows_ref(table0, ids):
    out = np.array(table0)
    for i in ids:
        if 0 <= i < out.shape[0]:
            out[i] = 0
    return out


def ln_stats(x, eps=EPS_LN):
    x = np.asarray(x, np.float64)
    mean = x.mean(1)
    rstd = 1.0 / np.sqrt(((x - mean[:, None]) ** 2).mean(1) + eps)
    return mean, rstd


def ln_fwd_ref(x, gamma, beta, mult=None, eps=EPS_LN):
    """y = ((x - mean) rstd gamma + beta) m; -> (value, bound [rows, 1])"""
    x, gamma, beta = np.asarray(x, np.float64), np.asarray(gamma, np.float64), np.asarray(beta, np.float64)
    mean, rstd = ln_stats(x, eps)
    y = (x - mean[:, None]) * rstd[:, None] * gamma + beta
    cond = 1 + np.abs(mean) * rstd
    bound = 2.0 ** -16 * (cond * np.abs(gamma).max() + np.abs(beta).max())
    if mult is not None:
        m = np.asarray(mult, np.float64).reshape(x.shape)
        y = y * m
        bound = bound * m.max() * (1 + U)          # one more fp32 product
    return y, np.broadcast_to(np.reshape(bound, (-1, 1)), (x.shape[0], 1))


def ln_bwd_ref(dy, x, gamma, mult_y=None, mult_b=None, eps=EPS_LN):
    """dy_eff = dy m_y; xhat = (x - mean) rstd; g = gamma dy_eff; dx = rstd (g - mean_c(g) - xhat mean_c(g xhat));
    dx_drop = dx m_b; d gamma = sum_rows dy_eff xhat; d beta = sum_rows dy_eff; dsum = sum_rows dx_drop.
    -> dict of the float64 values, the element bounds b_dx / b_dx_drop, and what ln_part_bounds needs for the three sums: sum|terms|
    (mag_*) and the error the terms themselves carry (in_*); see the module docstring"""
    dy, x, gamma = np.asarray(dy, np.float64), np.asarray(x, np.float64), np.asarray(gamma, np.float64)
    rows, d = x.shape
    my = np.ones_like(x) if mult_y is None else np.asarray(mult_y, np.float64).reshape(rows, d)
    mb = np.ones_like(x) if mult_b is None else np.asarray(mult_b, np.float64).reshape(rows, d)
    mean, rstd = ln_stats(x, eps)
    xhat = (x - mean[:, None]) * rstd[:, None]
    dye = dy * my
    g = gamma * dye
    dx = rstd[:, None] * (g - g.mean(1)[:, None] - xhat * (g * xhat).mean(1)[:, None])
    dxd = dx * mb
    cond = 1 + np.abs(mean) * rstd
    b_dx = (2.0 ** -14 * rstd * np.abs(g).max(1) * cond)[:, None] * np.ones((1, d))
    b_dxd = b_dx * mb + U * np.abs(dxd)
    return dict(dx=dx, dx_drop=dxd, dgamma=(dye * xhat).sum(0), dbeta=dye.sum(0), dsum=dxd.sum(0), b_dx=b_dx, b_dx_drop=b_dxd,
                mag_dgamma=np.abs(dye * xhat).sum(0), mag_dbeta=np.abs(dye).sum(0), mag_dsum=np.abs(dxd).sum(0),
                in_dgamma=(np.abs(dye) * (2.0 ** -16 * cond)[:, None]).sum(0), in_dsum=b_dxd.sum(0), mean=mean, rstd=rstd)


def ln_part_bounds(r, rows, parts):
    """bounds of the float64 sums of the partial rows part_dgamma / part_dbeta / part_dsum given ln_bwd_ref's dict"""
    c = c_ln_parts(rows, parts) * U
    return c * r["mag_dgamma"] + r["in_dgamma"], c * r["mag_dbeta"], c * r["mag_dsum"] + r["in_dsum"]


def pos_sum_ref(r, B, L, rows, parts):
    """sum_b dx[b, s, :] through part_pos (one partial row per WAVE: 4 parts rows) + colsum_pos with period L
    -> (value [L, d], bound): the wave chain ceil(rows / (4 parts)), colsum_pos's chain, and the dx bounds summed"""
    d = r["dx"].shape[1]
    c = (cdiv(rows, 4 * parts) + c_colsum_pos(4 * parts, L)) * U
    return (r["dx"].reshape(B, L, d).sum(0), c * np.abs(r["dx"]).reshape(B, L, d).sum(0) + r["b_dx"].reshape(B, L, d).sum(0))


# ------------------------------------------------------------------ fp32 emulations in the documented order, planted defects
DEFECTS_L1 = ("sum_without_abs", "missing_1e-6", "reciprocal_multiply", "dropped_tail_columns")
DEFECTS_ROWDOT = ("accumulate_ignored", "dropped_tail_columns")
DEFECTS_COLSUM = ("accumulate_ignored", "row_weight_ignored", "chunk_tail_rows_dropped")


def _butterfly(s):
    """wave_sum: v += v[lane ^ o] for o = 32, 16, 8, 4, 2, 1 (every lane ends with the same value)"""
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lane ^ o]
    return s[:, 0]


def _lane_groups(x, D, drop_tail):
    """[rows, groups, 64 lanes, 4]: lane l's float4 groups at columns 4 l + 256 i; columns past D read as +0 (x + 0 = x)"""
    rows = x.shape[0]
    V = cdiv(D, 256)
    xp = np.zeros((rows, V * 256), F)
    xp[:, :D] = x
    if drop_tail and D % 256:
        xp[:, (D // 256) * 256:] = 0
    return xp.reshape(rows, V, 64, 4)


def emul_l1(x, defect=None):
    """l1norm_kernel / l1norm_reg_kernel<V> / gather_l1_kernel in fp32 -> (sum, inv_scale, y), all float32"""
    x = np.asarray(x, F)
    rows, D = x.shape
    a = _lane_groups(x if defect == "sum_without_abs" else np.abs(x), D, defect == "dropped_tail_columns")
    s = np.zeros((rows, 64), F)
    for i in range(a.shape[1]):
        s = s + (((a[:, i, :, 0] + a[:, i, :, 1]) + a[:, i, :, 2]) + a[:, i, :, 3])
    s = _butterfly(s)
    with np.errstate(all="ignore"):
        den = s if defect == "missing_1e-6" else s + F(L1_EPS)
        inv = F(1.0) / den
        y = x * inv[:, None] if defect == "reciprocal_multiply" else x / den[:, None]
    return s, inv.astype(F), y.astype(F)


def emul_rowdot(x, w, bias=None, out0=None, defect=None):
    """rowdot_kernel in fp32, products rounded one by one (the kernel may fuse them: fewer roundings)"""
    x, w = np.asarray(x, F), np.asarray(w, F)
    rows, d = x.shape
    drop = defect == "dropped_tail_columns"
    a, b = _lane_groups(x, d, drop), _lane_groups(w[None, :], d, drop)
    s = np.zeros((rows, 64), F)
    for i in range(a.shape[1]):
        p = a[:, i] * b[:, i]
        s = s + (((p[..., 0] + p[..., 1]) + p[..., 2]) + p[..., 3])
    s = _butterfly(s)
    if bias is not None:
        s = s + F(bias)
    if out0 is not None and defect != "accumulate_ignored":
        s = np.asarray(out0, F) + s
    return s.astype(F)


def emul_colsum(X, w=None, out0=None, defect=None):
    """colsum_partial_kernel + colsum_final_kernel in fp32"""
    X = np.asarray(X, F)
    M, N = X.shape
    chunks, rpc = colsum_chunks(M), colsum_rows_per_chunk(M)
    if defect == "row_weight_ignored":
        w = None
    partial = np.zeros((chunks, N), F)
    for ch in range(chunks):
        r0 = ch * rpc
        r1 = min(M, r0 + rpc)
        if defect == "chunk_tail_rows_dropped":
            r1 = r0 + max(0, r1 - r0) // 4 * 4
        red = np.zeros((4, N), F)
        for ty in range(4):
            for r in range(r0 + ty, r1, 4):
                red[ty] = red[ty] + (X[r] * F(w[r]) if w is not None else X[r])
        partial[ch] = ((red[0] + red[1]) + red[2]) + red[3]
    red = np.zeros((4, N), F)
    for ty in range(4):
        for p in range(ty, chunks, 4):
            red[ty] = red[ty] + partial[p]
    s = (red[0] + red[1]) + (red[2] + red[3])
    if out0 is not None and defect != "accumulate_ignored":
        s = s + np.asarray(out0, F)
    return s.astype(F)


def ratio(err, bound):
    """worst err / bound over the elements: 0 where both are 0, inf where the error is not finite or the bound is 0 and the error is not"""
    err, bound = np.broadcast_arrays(np.asarray(err, np.float64), np.asarray(bound, np.float64))
    with np.errstate(all="ignore"):
        q = np.where(err == 0, 0.0, np.where(np.isfinite(err) & (bound > 0), err / bound, np.inf))
    return float(q.max()) if q.size else 0.0


def true_division_ok(x, s, y):
    """y is bit for bit x / (s + 1e-6f) in fp32 (ONE correctly rounded division per element): what separates the kernels' true
    division from a product with the rounded reciprocal, which stays inside any bound of a few u"""
    with np.errstate(all="ignore"):
        want = (np.asarray(x, F) / (np.asarray(s, F) + F(L1_EPS))[:, None]).astype(F)
    return bool((want.view(np.uint32) == np.asarray(y, F).view(np.uint32)).all())
