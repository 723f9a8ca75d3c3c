"""The comparison rule of the loss-kernel tests (helpers.loss_check / loss_compare) on the CPU: it accepts the float32 oracle, the
reference's own arithmetic, and rejects defects planted into that oracle -- each one a mistake a loss kernel could make
(csrc/loss.h).  No GPU needed."""
import os
import sys
import types

import numpy as np
import pytest
import torch

from helpers import LOSS_WEIGHTS, ROOT, all_label_rows, loss_cfg, loss_compare, make_logits, oracle_loss

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import segmm_oracle  # noqa: E402
from segmminterest_amd.synth import make_labels  # noqa: E402

ALL7 = ["focal", "interestBPR", "surviveCE", "interestCE", "interestKL", "huber", "hazard"]


def _fp32(res):
    return dict(slots=res["slots"], total=res["total"], dlogits=res["dlogits"])


def _rejects(got, t, r, cfg):
    with pytest.raises(AssertionError):
        loss_compare(got, t, r, cfg)


def test_all_label_rows_cover_make_labels():
    assert all_label_rows(40).shape == (860, 40) and all_label_rows(64).shape == (2144, 64)
    for S in (2, 7, 40):
        rows = {tuple(r) for r in all_label_rows(S).tolist()}
        assert len(rows) == all_label_rows(S).shape[0]
        lab, _, _ = make_labels(500, S, torch.Generator().manual_seed(S))
        assert all(tuple(r) in rows for r in lab.tolist())


@pytest.mark.parametrize("regime", ["init", "trained", "saturated", "ties"])
@pytest.mark.parametrize("losses,mask_loss", [(ALL7, 0), (ALL7[1:] + ALL7[:1], 1), (["interestBPR"], 0), (["hazard", "huber"], 1)])
def test_rule_accepts_float32_reference(regime, losses, mask_loss):
    """(The "extreme" regime is not here: the float32 reference itself is not finite there, which the rule rejects.)"""
    S = 20
    gt = all_label_rows(S)
    z = make_logits(regime, gt.shape[0], S, seed=3)
    cfg = loss_cfg(losses, S, mask_loss=mask_loss, exposure="stat")
    t, r = oracle_loss(z, gt, cfg), oracle_loss(z, gt, cfg, dtype=torch.float32)
    n_edge = loss_compare(_fp32(r), t, r, cfg)
    assert n_edge <= gt.shape[0] // 100


@pytest.mark.parametrize("regime", ["init", "trained"])
def test_rejects_local_normaliser(regime):
    """A data-parallel shard normalised by its own rows (B, mask count, valid-row count) instead of the global batch's."""
    S, G = 40, 4
    gt_all, _, _ = make_labels(256, S, torch.Generator().manual_seed(11))
    z_all = make_logits(regime, 256, S, seed=12)
    v_all = (gt_all == 1).sum(1).float()
    gs = dict(v_all=v_all, v2_all=(gt_all >= 0).sum(1).float(),
              norms=torch.tensor([float((v_all < S).sum()), 256.0, float((gt_all != -2).sum())]))
    cfg = loss_cfg(ALL7[1:], S)
    sl = slice(0, 256 // G)
    t = oracle_loss(z_all[sl], gt_all[sl], cfg, gs=gs)
    r = oracle_loss(z_all[sl], gt_all[sl], cfg, gs=gs, dtype=torch.float32)
    loss_compare(_fp32(r), t, r, cfg)
    _rejects(_fp32(oracle_loss(z_all[sl], gt_all[sl], cfg, dtype=torch.float32)), t, r, cfg)


def test_rejects_hazard_without_epsilon(monkeypatch):
    """log(hazard + 1e-6) without the 1e-6: saturated positive logits put the hazard at the leave to 0."""
    S = 40
    gt = all_label_rows(S)
    z = make_logits("saturated", gt.shape[0], S, seed=5)
    cfg = loss_cfg(["hazard"], S)
    t, r = oracle_loss(z, gt, cfg), oracle_loss(z, gt, cfg, dtype=torch.float32)

    def no_eps(hazard, view_len, S, B_global=None):
        ll = hazard.new_zeros(())
        for i in range(view_len.shape[0]):
            k = int(view_len[i])
            if k < S:
                ll = ll + torch.log(hazard[i, k]) - torch.log(hazard[i, k:].sum())
        return -ll / (view_len.shape[0] if B_global is None else B_global)

    monkeypatch.setattr(segmm_oracle, "partial_likelihood", no_eps)
    _rejects(_fp32(oracle_loss(z, gt, cfg, dtype=torch.float32)), t, r, cfg)


@pytest.mark.parametrize("regime", ["init", "trained", "saturated", "ties"])
def test_rejects_flipped_bpr_positive_gradient(regime):
    S = 40
    gt = all_label_rows(S)
    z = make_logits(regime, gt.shape[0], S, seed=6)
    cfg = loss_cfg(["interestBPR"], S)
    t, r = oracle_loss(z, gt, cfg), oracle_loss(z, gt, cfg, dtype=torch.float32)
    bad = _fp32(r)
    bad["dlogits"] = r["dlogits"].copy()
    v = (gt == 1).sum(1).numpy()
    rows = np.nonzero(v < S)[0]
    bad["dlogits"][rows, v[rows]] *= -1
    _rejects(bad, t, r, cfg)


@pytest.mark.parametrize("other", ["interestCE", "interestKL"])
def test_rejects_unrewritten_labels_after_focal(other):
    """interestCE / interestKL after focal see the labels focal rewrote in place; the defect reads the original labels."""
    S = 40
    gt = all_label_rows(S)
    z = make_logits("trained", gt.shape[0], S, seed=7)
    cfg = loss_cfg(["focal", other], S)
    t, r = oracle_loss(z, gt, cfg), oracle_loss(z, gt, cfg, dtype=torch.float32)
    _rejects(_fp32(oracle_loss(z, gt, loss_cfg([other, "focal"], S), dtype=torch.float32)), t, r, cfg)


@pytest.mark.parametrize("losses", [["surviveCE"], ["hazard"], ["huber"]])
def test_rejects_exclusive_survival_scan(monkeypatch, losses):
    """h_t = log p_0 + ... + log p_(t-1) instead of ... + log p_t."""
    S = 40
    gt = all_label_rows(S)
    z = make_logits("trained", gt.shape[0], S, seed=8)
    cfg = loss_cfg(losses, S)
    t, r = oracle_loss(z, gt, cfg), oracle_loss(z, gt, cfg, dtype=torch.float32)
    proxy = types.SimpleNamespace(**{k: getattr(torch, k) for k in dir(torch) if not k.startswith("__")})
    proxy.cumsum = lambda x, dim: torch.cumsum(x, dim=dim) - x
    monkeypatch.setattr(segmm_oracle, "torch", proxy)
    _rejects(_fp32(oracle_loss(z, gt, cfg, dtype=torch.float32)), t, r, cfg)


def test_rejects_huber_weight_from_its_own_key():
    """compute_loss weights huber by loss_weight['mse'] (decoder_leave_focal.py:561-566), not by loss_weight['huber']."""
    S = 40
    gt = all_label_rows(S)
    z = make_logits("trained", gt.shape[0], S, seed=9)
    cfg = loss_cfg(["interestBPR", "huber"], S)
    t, r = oracle_loss(z, gt, cfg), oracle_loss(z, gt, cfg, dtype=torch.float32)
    w = dict(LOSS_WEIGHTS, mse=LOSS_WEIGHTS["huber"])
    _rejects(_fp32(oracle_loss(z, gt, loss_cfg(["interestBPR", "huber"], S, weights=w), dtype=torch.float32)), t, r, cfg)
