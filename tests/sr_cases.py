"""Shared by test_sr_cpu.py / test_sr_gpu.py: the reference fixtures with spatial-reduction attention (tests/golden/sr,
tools/gen_golden_sr.py) and a model builder that passes ``sr_ratio_lvls`` with the opt-in key ``model_cfg.sr_attn = 1``
(helpers.build_model hard-codes ``[1] * N``)."""
import argparse

import torch

from helpers import load_case

SR_EVAL_CASES = ("sr_img_d32_N3", "sr_img_S41_N3", "sr_id_d32_N3", "sr_crossatt_N3", "sr_selfatt_N3", "sr_both_N2")
SR_TRAIN_CASES = ("train_sr_img_d32_N3",)


def load_sr_case(name):
    """helpers.load_case on tests/golden/sr/<name>.npz, completed to the layout of the other fixtures: the ``adam1`` / ``adam3``
    entries of the parameters without a gradient (the generator leaves them out: AdamW skips them, they equal ``sd``)."""
    cfg, grp, nograd, extra = load_case("sr/" + name)
    for a in ("adam1", "adam3"):
        if grp[a]:
            for k in nograd:
                grp[a].setdefault(k, grp["sd"][k].clone())
    assert len(cfg["sr"]) == cfg["N"]
    return cfg, grp, nograd, extra


def sr_args(cfg, sr_attn=1):
    a = argparse.Namespace(debug=0, num_layers_enc=cfg["N"], ablation_type=cfg.get("ablation_type", "ours"), d_model=cfg["d"],
                           nhead=cfg["h"], input_type={"user": cfg["user"], "photo": cfg["photo"]},
                           learnable_bias=cfg.get("learnable_bias", 0), exposure_prob=cfg["exposure_prob"],
                           fusion_heads=cfg.get("fusion_heads", 2), loss_type_list=cfg["loss_type_list"],
                           loss_weight=cfg["loss_weight"], mask_loss=cfg.get("mask_loss", 0), use_pe=cfg.get("use_pe", 1))
    if sr_attn is not None:
        a.sr_attn = sr_attn
    return a


def build_sr_model(cfg):
    """helpers.build_model with ``sr_ratio_lvls = cfg["sr"]`` and the opt-in key."""
    import segmminterest_amd as M
    S, N, d, h = cfg["S"], cfg["N"], cfg["d"], cfg["h"]
    args = sr_args(cfg)

    def backbone(user_id_max, video_id_max, max_usr_len):
        return M.SegFormerX(d_model_in=d, d_model_lvls=[d] * N, num_head_lvls=[h] * N, ff_dim_lvls=[d] * N,
                            input_vid_dim=max(cfg["D_in"], 1), input_usr_dim=max(cfg["D_in"], 1), max_vid_len=S,
                            max_usr_len=max_usr_len, sr_ratio_lvls=list(cfg["sr"]), use_patch_merge=[False] * N, output_layers=[-1],
                            model_cfg=args, user_id_max=user_id_max, video_id_max=video_id_max, use_pe=cfg.get("use_pe", 1))

    nu, ni = cfg.get("n_users", 0), cfg.get("n_items", 0)
    u, p = cfg["user"], cfg["photo"]
    if u == "both" or p == "both":
        um1, ul1, um2, ul2 = {"both": (-1, cfg["Lt"], nu, 1), "id": (nu, 1, nu, 1), "image": (-1, cfg["Lt"], -1, cfg["Lt"])}[u]
        vm1, vm2 = {"both": (-1, ni), "id": (ni, ni), "image": (-1, -1)}[p]
        model = M.MultiScaleTemporalDetrLeaveFocal(backbone(um1, vm1, ul1), backbone(um2, vm2, ul2), None, torch.nn.Identity(), args)
    else:
        um1, ul1 = (nu, 1) if u == "id" else (-1, cfg["Lt"])
        model = M.MultiScaleTemporalDetrLeaveFocal(backbone(um1, ni if p == "id" else -1, ul1), None, None, torch.nn.Identity(), args)
    model._test_fwd_seed = None
    return model
