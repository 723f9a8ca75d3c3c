"""segmm_valid_rows (csrc/evalops.h valid_rows_kernel): the tail of a validation batch in one launch -- interests =
sigmoid(logits) * exposure, the candidate shuffles drawn in the kernel, the leave rank -- against the host definitions."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
DEV = torch.device("cuda:0")
SHAPES = [(5, 1), (7, 20), (48, 40), (9, 65), (6, 256)]


@functools.lru_cache(maxsize=None)
def _inputs(B, S):
    """(logits [B, S + 3] fp32, exposure [S] fp32, gt [B, S] int64) on the host, made once per shape and never written.  Rows 0 .. 3
    are fixed: fully watched (invalid), leave at 0, a fully padded tail, an exact tie of the target with another candidate."""
    g = torch.Generator().manual_seed(1000 * B + S)
    logits = torch.randn(B, S + 3, generator=g) * 3.0
    exposure = torch.rand(S, generator=g) * 0.5 + 0.5
    gt = torch.full((B, S), -2, dtype=torch.int64)
    for b in range(B):
        dur = int(torch.randint(1, S + 1, (1,), generator=g))
        vl = int(torch.randint(0, dur + 1, (1,), generator=g))
        if b == 0:
            dur, vl = S, S                      # fully watched: no leave segment
        elif b == 1:
            dur, vl = S, 0                      # leave at position 0
        elif b == 2:
            dur = max(S // 2, 1)                # the tail from dur on is padding
            vl = min(vl, dur - 1)
        elif b == 3 and S >= 3:
            dur, vl = S, 1
        gt[b, :vl] = 1
        if vl < dur:
            gt[b, vl] = 0
            gt[b, vl + 1:dur] = -1
    if S >= 3:                                  # row 3: target (position 1) and position 2 have identical logit AND exposure
        exposure[2] = exposure[1]
        logits[3, 2] = logits[3, 1]
    return logits, exposure, gt


def _host_ranks(interests, perm, gt, masked, seq_valid):
    """valid_model's host arithmetic (my_evaluation._topk) on given interests and candidate permutations; 0 for invalid rows."""
    from segmminterest_amd.my_evaluation import _rank_of_target
    B, S = gt.shape
    vl = (gt == 1).sum(1)
    mask = gt != -2
    valid = (vl != mask.sum(1)) if masked else (vl < seq_valid)
    x = interests[valid]
    if masked:
        x = np.where(mask[valid], x, np.float32(1.1))
    pred = np.take_along_axis(x, perm[valid], 1)
    target = np.argmax(perm[valid] == vl[valid][:, None], axis=1)
    out = np.zeros(B, dtype=np.int64)
    if valid.any():
        out[valid] = _rank_of_target(pred, target)
    return out


def _e_ref(logits, exposure):
    """Max relative error of torch's float32 sigmoid(logit) * exposure on the CPU against float64, on these inputs."""
    ref = torch.sigmoid(logits.double()) * exposure.double()
    got = (torch.sigmoid(logits) * exposure).double()
    return float(((got - ref).abs() / ref).max()), ref


@pytest.mark.parametrize("sv_default", [True, False])
@pytest.mark.parametrize("permute", [0, 1])
@pytest.mark.parametrize("masked", [0, 1])
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("B,S", SHAPES)
def test_ranks_and_interests_match_the_host_definitions(B, S, pad, masked, permute, sv_default):
    """Ranks: integer for integer _rank_of_target (my_evaluation.py) on the kernel's OWN interests and permutation.  Interests against
    float64 sigmoid(logit) * exposure: the kernel gets 4 * e_ref, e_ref = the max relative error of torch's float32 CPU expression on
    the same inputs (room for a device expf a couple of ulp off the host's, one divide and one multiply).  Measured on an MI355X, (B, S):
    e_ref / kernel = (5, 1) 1.07e-07 / 6.9e-08, (7, 20) 1.12e-07 / 1.12e-07, (48, 40) 1.31e-07 / 1.31e-07, (9, 65) 1.48e-07 / 1.48e-07,
    (6, 256) 1.45e-07 / 1.30e-07: the kernel is as close to float64 as the host expression, the bounds are 4.3e-07 .. 5.9e-07."""
    from segmminterest_amd import hipabi as H
    logits_h, exposure_h, gt_h = _inputs(B, S)
    ld = S + pad
    logits = logits_h[:, :ld].contiguous().to(DEV)[:, :S]
    exposure, gt = exposure_h.to(DEV), gt_h.to(DEV)
    seq_valid = S if sv_default else S - 1
    interests = torch.full((B, S), -1.0, device=DEV)
    perm_out = torch.full((B, S), -1, dtype=torch.int32, device=DEV)
    ranks = H.valid_rows(logits, exposure, gt, masked=masked, seq_valid=None if sv_default else seq_valid, permute=permute, seed=11,
                         site=5, row0=100, interests=interests, perm_out=perm_out)
    assert logits.stride(0) == ld
    x, perm, r = interests.cpu().numpy(), perm_out.cpu().numpy().astype(np.int64), ranks.cpu().numpy().astype(np.int64)
    assert (np.sort(perm, 1) == np.arange(S)[None, :]).all()
    if not permute:
        assert (perm == np.arange(S)[None, :]).all()
    want = _host_ranks(x, perm, gt_h.numpy(), masked, seq_valid)
    assert (r == want).all(), (r, want)
    assert r[0] == 0 and (S == 1 or (r > 0).any())          # the fully watched row; the other rows are not all invalid
    e_ref, ref = _e_ref(logits_h[:, :S], exposure_h)
    err = float(((torch.from_numpy(x).double() - ref).abs() / ref).max())
    print("valid_rows B=%d S=%d: e_ref %.3e  kernel %.3e  bound %.3e" % (B, S, e_ref, err, 4 * e_ref))
    assert err <= 4 * e_ref, (err, e_ref)
    # without the optional outputs: the same ranks
    r2 = H.valid_rows(logits, exposure, gt, masked=masked, seq_valid=seq_valid, permute=permute, seed=11, site=5, row0=100)
    assert torch.equal(r2, ranks)


def test_a_row_draws_the_same_permutation_in_any_batch_split():
    """The draw is keyed by (seed, site, row0 + b): one launch of 48 rows == two launches of 24 with row0 = 0 and 24; another seed
    (or site) gives another draw; every row is a permutation of 0 .. S-1."""
    from segmminterest_amd import hipabi as H
    B, S = 48, 40
    logits_h, exposure_h, gt_h = _inputs(B, S)
    logits, exposure, gt = logits_h[:, :S].contiguous().to(DEV), exposure_h.to(DEV), gt_h.to(DEV)

    def run(lo, hi, seed, site=3, base=0):
        p = torch.empty((hi - lo, S), dtype=torch.int32, device=DEV)
        r = H.valid_rows(logits[lo:hi], exposure, gt[lo:hi], permute=1, seed=seed, site=site, row0=base + lo, perm_out=p)
        return r, p

    r, p = run(0, B, 77)
    assert torch.equal(p.sort(1).values, torch.arange(S, device=DEV, dtype=torch.int32).expand(B, S))
    ra, pa = run(0, 24, 77)
    rb, pb = run(24, B, 77)
    assert torch.equal(torch.cat([pa, pb]), p) and torch.equal(torch.cat([ra, rb]), r)
    assert not torch.equal(run(0, B, 78)[1], p) and not torch.equal(run(0, B, 77, site=4)[1], p)
    assert not torch.equal(run(0, B, 77, base=48)[1], p)
    assert len({tuple(row.tolist()) for row in p}) == B


def test_drawn_permutations_are_uniform():
    """Over 4096 rows at S = 8 the position of element 0 is uniform, within the allowance of
    test_eval_gpu.test_device_draws_have_the_reference_distributions (every count within 40 % of the mean)."""
    from segmminterest_amd import hipabi as H
    rows, S = 4096, 8
    g = torch.Generator().manual_seed(5)
    logits = torch.randn(rows, S, generator=g).to(DEV)
    exposure = torch.ones(S, device=DEV)
    gt = torch.zeros((rows, S), dtype=torch.int64, device=DEV)
    perm = torch.empty((rows, S), dtype=torch.int32, device=DEV)
    H.valid_rows(logits, exposure, gt, permute=1, seed=777, site=5, perm_out=perm)
    pos0 = (perm == 0).int().argmax(1)
    cnt = torch.bincount(pos0, minlength=S).float()
    assert float((cnt / cnt.mean() - 1).abs().max()) < 0.4


def test_refusals_name_what_is_wrong():
    from segmminterest_amd import hipabi as H
    B, S = 4, 300
    logits = torch.zeros((B, S), device=DEV)
    gt = torch.zeros((B, S), dtype=torch.int64, device=DEV)
    exposure = torch.ones(S, device=DEV)
    with pytest.raises(RuntimeError, match=r"permute.*S = 300 > 256"):
        H.valid_rows(logits, exposure, gt, permute=1)
    assert H.valid_rows(logits, exposure, gt, permute=0).shape == (B,)          # any S without permute
    with pytest.raises(RuntimeError, match=r"exposure is null"):
        H.valid_rows(logits, None, gt)
    with pytest.raises(RuntimeError, match=r"seq_valid"):
        H.valid_rows(logits, exposure, gt, seq_valid=S + 1)
    assert H.valid_rows(logits[:0], exposure, gt[:0], permute=1 if S <= 256 else 0).numel() == 0          # B == 0 launches nothing
    torch.cuda.synchronize()
