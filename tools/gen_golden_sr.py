#!/usr/bin/env python
"""Golden vectors of the REAL reference with spatial-reduction attention, sr_ratio > 1 (TEST INFRASTRUCTURE ONLY).

Runs only where the reference checkout exists (``oracle/ref_import.py`` finds it).  Same recipe and file format as
``oracle/gen_golden.py`` -- its ``perturb``, ``make_inputs``, ``_gen_case_body`` and ``MaskRecorder`` are imported, not copied, and
``coarsen_dead`` / ``slim`` come from ``tools/gen_golden_ffn.py`` -- with one difference: the model builder below passes a per-layer
``sr_ratio_lvls`` (the case's ``"sr"`` list, which therefore also lands in the fixture's ``cfg`` JSON).  The fixtures go to
``tests/golden/sr/``: a directory of their own, because every ``.npz`` directly under ``tests/golden/`` is picked up by the
existing fixture-parametrised tests, whose model builder hard-codes ``sr_ratio_lvls = [1] * N``.

Every file stays under 1 MiB (``slim``, ``coarsen_dead``).

    python tools/gen_golden_sr.py            # regenerate every fixture of this family
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, ROOT)

import ref_import  # noqa: E402
import gen_golden as G  # noqa: E402
from gen_golden_ffn import coarsen_dead, slim  # noqa: E402

_BASE = dict(d=32, h=4, N=3, S=40, Lt=10, D_in=48, B=8, loss="interestBPR")
# layer N-1 is dead in every case: its sr conv (sr_id_d32_N3: r = 8) is only ever loaded.  S = 41: token 40 is in no window of
# r = 2, and r = 4 has S % 4 = 1.  CrossAtt: layer 1 projects no video keys, its sr gets no gradient.  SelfAtt r = 8: Ls = 5.
CASES = {
    "sr_img_d32_N3": dict(_BASE, user="image", photo="image", loss="interestBPR,surviveCE", adam=True, sr=[2, 4, 1]),
    # (surviveCE: the reference's interestBPR counts a row as valid when view_len < 40, a constant; the oracle and the engine read
    #  that as view_len < S, which differs at S = 41 for the forced row with view_len = 40 -- nothing of this feature)
    "sr_img_S41_N3": dict(_BASE, user="image", photo="image", S=41, loss="surviveCE", sr=[2, 4, 1]),
    "sr_id_d32_N3": dict(_BASE, user="id", photo="id", Lt=1, D_in=0, n_users=50, n_items=200, sr=[4, 2, 8]),
    "sr_crossatt_N3": dict(_BASE, user="image", photo="image", ablation="CrossAtt", sr=[2, 2, 1]),
    "sr_selfatt_N3": dict(_BASE, user="image", photo="image", ablation="SelfAtt", sr=[8, 2, 1]),
    "sr_both_N2": dict(_BASE, user="both", photo="both", N=2, fusion_heads=2, n_users=50, n_items=200, sr=[2, 1]),
}
TRAIN_CASES = {
    "train_sr_img_d32_N3": dict(_BASE, user="image", photo="image", loss="interestBPR,surviveCE", adam=True, sr=[2, 4, 1]),
}


def build_reference_model(c, enc, dec):
    """The reference's model for case ``c`` with ``sr_ratio_lvls = c["sr"]`` (one ratio per layer)."""
    S, N, d, h = c["S"], c["N"], c["d"], c["h"]
    sr = list(c["sr"])
    assert len(sr) == N
    cfg = argparse.Namespace(debug=0, num_layers_enc=N, ablation_type=c.get("ablation", "ours"), d_model=d, nhead=h,
                             input_type={"user": c["user"], "photo": c["photo"]}, learnable_bias=c.get("learnable_bias", 0),
                             exposure_prob=[1.0] * S, fusion_heads=c.get("fusion_heads", 2),
                             loss_type_list=[x.strip() for x in c["loss"].split(",")], loss_weight=dict(G.ALL_LOSS_W),
                             mask_loss=c.get("mask_loss", 0), use_pe=c.get("use_pe", 1))

    def backbone(user_id_max, video_id_max, max_usr_len):
        return enc.SegFormerX(d_model_in=d, d_model_lvls=[d] * N, num_head_lvls=[h] * N, ff_dim_lvls=[d] * N,
                              input_vid_dim=max(c["D_in"], 1), input_usr_dim=max(c["D_in"], 1), max_vid_len=S,
                              max_usr_len=max_usr_len, sr_ratio_lvls=sr, use_patch_merge=[False] * N, output_layers=[-1],
                              model_cfg=cfg, user_id_max=user_id_max, video_id_max=video_id_max, use_pe=c.get("use_pe", 1))

    nu, ni = c.get("n_users", 0), c.get("n_items", 0)
    u, p = c["user"], c["photo"]
    if u == "both" or p == "both":
        um1, ul1, um2, ul2 = {"both": (-1, c["Lt"], nu, 1), "id": (nu, 1, nu, 1), "image": (-1, c["Lt"], -1, c["Lt"])}[u]
        vm1, vm2 = {"both": (-1, ni), "id": (ni, ni), "image": (-1, -1)}[p]
        model = dec.MultiScaleTemporalDetrLeaveFocal(backbone(um1, vm1, ul1), backbone(um2, vm2, ul2), None, torch.nn.Identity(), cfg)
    else:
        um1, ul1 = (nu, 1) if u == "id" else (-1, c["Lt"])
        model = dec.MultiScaleTemporalDetrLeaveFocal(backbone(um1, ni if p == "id" else -1, ul1), None, None, torch.nn.Identity(), cfg)
    return model, cfg


def gen_case(name, c, enc, dec, outdir, train=False):
    torch.manual_seed(sum(ord(ch) for ch in name))
    model, cfg = build_reference_model(c, enc, dec)
    G.perturb(model, seed=11 + len(name))
    with torch.no_grad():          # (perturb widens the 2-D weights only: the conv weights get the same factor)
        for n_, p in model.named_parameters():
            if n_.endswith("cross_attn.sr.weight"):
                p.mul_(6.0)
    model.eval()
    coarsen_dead(model, c)
    rec = None
    if train:
        import torch.nn.functional as F
        model.train()
        rec = G.MaskRecorder(seed=77 + len(name))
        F_dropout, F.dropout = F.dropout, rec
    else:
        model.eval()
    try:
        G._gen_case_body(name, c, cfg, model, outdir, rec)
    finally:
        if train:
            F.dropout = F_dropout
    slim(os.path.join(outdir, name + ".npz"))


def main():
    ap_ = argparse.ArgumentParser()
    ap_.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "sr"))
    a = ap_.parse_args()
    os.makedirs(a.out, exist_ok=True)
    torch.set_num_threads(1)
    enc, dec, _ = ref_import.load()
    for name, c in CASES.items():
        gen_case(name, c, enc, dec, a.out)
    for name, c in TRAIN_CASES.items():
        gen_case(name, c, enc, dec, a.out, train=True)


if __name__ == "__main__":
    main()
