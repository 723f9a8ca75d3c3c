"""K7, the interest head (csrc/rowops.h): segmm_layernorm_fwd_dot / segmm_layernorm_bwd_outer for the Linear(d, 1) head on the
backbone's last LayerNorm, segmm_rowdot_pair / segmm_rowscale_mat for the bilinear fusion head, and the small kernels around the
loss (segmm_bias_grad, segmm_focal_relabel) against float64 and against the unfused kernels they replace (bit for bit).
Run with ``pytest -m gpu``.

Tolerances, u = 2^-24: LayerNorm's mean is a sum of d <= 2048 values in chains of <= 4 V + 6 = 38 fp32 adds, so its error is
<= 38 u |mean| < 2^-18.7 |mean|; (x - mean) rstd carries that error times rstd, which is what rows with |mean| >> spread
exercise.  The bounds below allow 2^-16 (forward) / 2^-14 (backward: three such products and two row means) per unit of
(1 + |mean| rstd) -- 2^-14 covers 4 x that worst case."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-12


def _abi():
    from segmminterest_amd import hipabi
    hipabi.lib()
    return hipabi


def _x(rows, d, seed):
    """N(0.3, 2) rows; every 5th row sits at a common offset of +-300 with spread 0.5 (|mean| >> spread)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, d, generator=g) * 2 + 0.3
    off = torch.arange(rows) % 5 == 4
    x[off] = torch.where(torch.arange(rows)[off, None] % 2 == 0, 300.0, -300.0) + 0.5 * torch.randn(int(off.sum()), d, generator=g)
    return x


def _ln_params(d, seed):
    g = torch.Generator().manual_seed(seed)
    return 1 + 0.1 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)


def _po(H, rows, cols, scale):
    hdr = H.new_site(DEV)[0]
    sc = torch.tensor([scale], dtype=torch.float32, device=DEV)
    pl = torch.zeros((rows, 2 * cols), dtype=torch.float16, device=DEV)
    return pl, hdr, H.PO(pl, 2 * cols, hdr, sc.data_ptr()), sc


DS = [32, 64, 256, 260, 768, 1024, 2048]          # every V of layernorm_fwd_kernel<V> / layernorm_bwd_kernel<V>


@pytest.mark.parametrize("with_b", [False, True])
@pytest.mark.parametrize("rows", [1, 3, 4097])
@pytest.mark.parametrize("d", DS)
def test_layernorm_fwd_dot(d, rows, with_b):
    H = _abi()
    x = _x(rows, d, seed=d + rows)
    gamma, beta = _ln_params(d, seed=d)
    g = torch.Generator().manual_seed(rows)
    w = torch.randn(d, generator=g) / math.sqrt(d)
    b = torch.tensor([0.375])
    xd, gd, bd, wd = x.to(DEV), gamma.to(DEV), beta.to(DEV), w.to(DEV)
    y, mean, rstd, dot = (torch.full(s, float("nan"), device=DEV) for s in ((rows, d), (rows,), (rows,), (rows,)))
    H.layernorm_fwd_dot(xd, gd, bd, y, mean, rstd, wd, b.to(DEV) if with_b else None, dot)
    # y, mean, rstd bitwise those of the plain forward
    y0, m0, r0 = torch.empty_like(y), torch.empty_like(mean), torch.empty_like(rstd)
    H.layernorm_fwd(xd, gd, bd, y0, m0, r0)
    assert torch.equal(y, y0) and torch.equal(mean, m0) and torch.equal(rstd, r0)
    # against float64
    xt = x.double()
    mt = xt.mean(1)
    rt = 1 / torch.sqrt(((xt - mt[:, None]) ** 2).mean(1) + EPS)
    yt = (xt - mt[:, None]) * rt[:, None] * gamma.double() + beta.double()
    cond = 1 + mt.abs() * rt                                          # (1 + |mean| rstd): the conditioning of x - mean
    tol_y = 2.0 ** -16 * (cond * gamma.abs().max() + beta.abs().max())
    assert ((y.cpu().double() - yt).abs().max(1).values <= tol_y).all()
    assert ((mean.cpu().double() - mt).abs() <= 2.0 ** -16 * xt.abs().mean(1)).all()
    assert ((rstd.cpu().double() - rt).abs() <= 2.0 ** -16 * rt * cond).all()
    dt = yt @ w.double() + (0.375 if with_b else 0.0)
    tol_dot = tol_y * w.abs().sum() + 2.0 ** -16 * (yt.abs() @ w.abs().double() + 0.375)
    assert ((dot.cpu().double() - dt).abs() <= tol_dot).all()
    if d % 32 == 0:
        # with the engine's plane output: the same planes and site header as the plain forward's
        pl, hdr, po, sc = _po(H, rows, d, 2.0 ** 10)
        H.layernorm_fwd_dot(xd, gd, bd, y, mean, rstd, wd, b.to(DEV) if with_b else None, dot, po=po)
        pl0, hdr0, po0, sc0 = _po(H, rows, d, 2.0 ** 10)
        H.layernorm_fwd(xd, gd, bd, y0, m0, r0, po=po0)
        torch.cuda.synchronize()
        assert torch.equal(pl, pl0) and torch.equal(hdr, hdr0) and torch.equal(y, y0)


@pytest.mark.parametrize("rows", [1, 3, 4097])
@pytest.mark.parametrize("d", DS)
def test_layernorm_bwd_outer(d, rows):
    H = _abi()
    x = _x(rows, d, seed=3 * d + rows)
    gamma, beta = _ln_params(d, seed=d + 1)
    g = torch.Generator().manual_seed(d * rows)
    dl = torch.randn(rows, generator=g) * torch.exp(torch.randn(rows, generator=g))
    w = torch.randn(d, generator=g) / math.sqrt(d)
    xd, gd, bd = x.to(DEV), gamma.to(DEV), beta.to(DEV)
    y, mean, rstd = torch.empty(rows, d, device=DEV), torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
    H.layernorm_fwd(xd, gd, bd, y, mean, rstd)
    parts = H.layernorm_bwd_parts(rows, d)
    dx, pg, pb = (torch.full(s, float("nan"), device=DEV) for s in ((rows, d), (parts, d), (parts, d)))
    H.layernorm_bwd_outer(dl.to(DEV), w.to(DEV), xd, mean, rstd, gd, dx, None, pg, pb)
    # bitwise the plain backward on the materialised dl[:, None] * w (one fp32 rounding either way)
    dy = dl.to(DEV)[:, None] * w.to(DEV)
    dx0, pg0, pb0 = torch.empty_like(dx), torch.empty_like(pg), torch.empty_like(pb)
    H.layernorm_bwd(dy, xd, mean, rstd, gd, dx0, None, pg0, pb0)
    assert torch.equal(dx, dx0) and torch.equal(pg, pg0) and torch.equal(pb, pb0)
    # against the float64 LayerNorm backward with dy = dl (x) w; partial rows summed in float64 here
    xr = x.double().requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    dyt = dl.double()[:, None] * w.double()
    torch.nn.functional.layer_norm(xr, (d,), gr, br, EPS).backward(dyt)
    mt = x.double().mean(1)
    rt = 1 / torch.sqrt(((x.double() - mt[:, None]) ** 2).mean(1) + EPS)
    cond = 1 + mt.abs() * rt
    gdy = (gamma.double() * dyt).abs().max(1).values
    assert ((dx.cpu().double() - xr.grad).abs().max(1).values <= 2.0 ** -14 * rt * gdy * cond).all()
    dg, db = pg.cpu().double().sum(0), pb.cpu().double().sum(0)
    xhat_abs = ((x.double() - mt[:, None]) * rt[:, None]).abs()
    assert ((dg - gr.grad).abs() <= 2.0 ** -14 * (dyt.abs() * (xhat_abs + cond[:, None])).sum(0)).all()
    assert ((db - br.grad).abs() <= 2.0 ** -16 * dyt.abs().sum(0)).all()


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("rows", [5, 1027])
@pytest.mark.parametrize("d", [4, 32, 260, 1024])
def test_rowdot_pair_strided(d, rows, accumulate):
    """out[m] (+)= a[m, a_off : a_off + d] . b[m, b_off : b_off + d] with row strides lda / ldb wider than d (the fusion head's
    T and v2 views, decoder_leave_focal.py _head_fwd); out entries past ``rows`` untouched."""
    H = _abi()
    g = torch.Generator().manual_seed(d + rows)
    lda, ldb, a_off, b_off = d + 12, 2 * d + 4, 8, d
    A = torch.randn(rows, lda, generator=g)
    Bm = torch.randn(rows, ldb, generator=g)
    out0 = torch.randn(rows + 5, generator=g)
    out = out0.to(DEV)
    H.rowdot_pair(A.to(DEV), lda, Bm.to(DEV), ldb, out, rows, d, accumulate=bool(accumulate), a_off=a_off, b_off=b_off)
    a, b = A[:, a_off:a_off + d].double(), Bm[:, b_off:b_off + d].double()
    want = (a * b).sum(1) + (out0[:rows].double() if accumulate else 0)
    tol = 2.0 ** -16 * ((a * b).abs().sum(1) + (out0[:rows].double().abs() if accumulate else 0))
    got = out.cpu()
    assert ((got[:rows].double() - want).abs() <= tol).all()
    assert torch.equal(got[rows:], out0[rows:])


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("rows", [5, 1027])
@pytest.mark.parametrize("d", [4, 32, 260, 1024])
def test_rowscale_mat_strided(d, rows, accumulate):
    """out[m, :d] (+)= g[m] X[m, :d] on column-offset views with strides ldx / ldo wider than d (dv2 += dl * T, dT = dl * v2
    in the fusion head's backward); every element of the output buffer outside the written columns is left as it was."""
    H = _abi()
    gen = torch.Generator().manual_seed(7 * d + rows)
    ldx, ldo, x_off, o_off = d + 8, 2 * d + 12, 4, d + 4
    X = torch.randn(rows, ldx, generator=gen)
    gs = torch.randn(rows, generator=gen)
    O0 = torch.randn(rows + 2, ldo, generator=gen)
    Od = O0.to(DEV)
    Xd = X.to(DEV)
    H.rowscale_mat(gs.to(DEV), Xd[:, x_off:], ldx, Od[:, o_off:], ldo, rows, d, accumulate=bool(accumulate))
    got = Od.cpu()
    prod = gs[:, None].double() * X[:, x_off:x_off + d].double()
    if accumulate:
        want = prod + O0[:rows, o_off:o_off + d].double()
        assert ((got[:rows, o_off:o_off + d].double() - want).abs() <= 2.0 ** -23 * (prod.abs() + O0[:rows, o_off:o_off + d].double().abs())).all()
    else:
        assert torch.equal(got[:rows, o_off:o_off + d], gs[:, None] * X[:, x_off:x_off + d])       # one fp32 product
    keep = torch.ones_like(O0, dtype=torch.bool)
    keep[:rows, o_off:o_off + d] = False
    assert torch.equal(got[keep], O0[keep])


@pytest.mark.parametrize("B,S", [(1, 40), (7, 1), (300, 33), (2048, 64)])
def test_bias_grad(B, S):
    """d bias_bias[s] = sum_b dl[b, s] against float64 (a B-long fp32 chain: <= B u sum |dl|), d bias_weight[s] = (s + 1) of it
    bit for bit."""
    H = _abi()
    g = torch.Generator().manual_seed(B * S)
    dl = torch.randn(B, S, generator=g) * torch.exp(torch.randn(B, S, generator=g))
    gbw, gbb = torch.full((S,), float("nan"), device=DEV), torch.full((S,), float("nan"), device=DEV)
    H.bias_grad(dl.to(DEV), B, S, gbw, gbb)
    gbw, gbb = gbw.cpu(), gbb.cpu()
    want = dl.double().sum(0)
    assert ((gbb.double() - want).abs() <= B * 2.0 ** -24 * dl.double().abs().sum(0)).all()
    assert torch.equal(gbw, (torch.arange(S, dtype=torch.float32) + 1) * gbb)


def test_focal_relabel_mapping():
    """gt > 0 -> 1, gt == -1 -> 0, everything else unchanged, at an n that is not a multiple of the 1024 x 256 grid stride."""
    H = _abi()
    n = 2 * 1024 * 256 + 37
    g = torch.Generator().manual_seed(1)
    vals = torch.tensor([1, 0, -1, -2, 2, 7, -3])
    gt = vals[torch.randint(0, len(vals), (n,), generator=g)]
    gt[-1] = -1
    gt[-2] = 1
    gd = gt.to(DEV)
    H.focal_relabel(gd)
    want = torch.where(gt > 0, 1, torch.where(gt == -1, 0, gt))
    got = gd.cpu()
    assert torch.equal(got, want)
    assert set(torch.unique(got[(gt >= -2) & (gt <= 1)]).tolist()) <= {1, 0, -2}
