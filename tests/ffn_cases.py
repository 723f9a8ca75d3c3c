"""Shared by test_ffn_width_cpu.py / test_ffn_width_gpu.py: the reference fixtures with feed-forward widths that differ from
d_model (tests/golden/ffn, tools/gen_golden_ffn.py) and a model builder that passes ``ff_dim_lvls`` (helpers.build_model
hard-codes ``[d] * N``)."""
import argparse
import os

import numpy as np
import torch

from helpers import GOLDEN, load_case

FF_EVAL_CASES = ("ff_img_d32_N3", "ff_both_d32_N2", "ff_crossatt_N3", "ff_narrow_d64_N3")
FF_TRAIN_CASES = ("train_ff_img_d32_N3",)


def load_ff_case(name):
    """helpers.load_case on tests/golden/ffn/<name>.npz, completed to the layout of the other fixtures: the ``grad`` group from
    <name>.grad.npz where the generator split it off, and the ``adam1`` / ``adam3`` entries of the parameters without a gradient
    (the generator leaves them out: AdamW skips them, they equal ``sd``)."""
    cfg, grp, nograd, extra = load_case("ffn/" + name)
    gpath = os.path.join(GOLDEN, "ffn", name + ".grad.npz")
    if os.path.exists(gpath):
        assert not grp["grad"]
        z = np.load(gpath)
        grp["grad"] = {k.split("/", 1)[1]: torch.from_numpy(z[k]) for k in z.files}
    for a in ("adam1", "adam3"):
        if grp[a]:
            for k in nograd:
                grp[a].setdefault(k, grp["sd"][k].clone())
    assert len(cfg["ff"]) == cfg["N"]
    return cfg, grp, nograd, extra


def ff_args(cfg):
    return argparse.Namespace(debug=0, num_layers_enc=cfg["N"], ablation_type=cfg.get("ablation_type", "ours"), d_model=cfg["d"],
                              nhead=cfg["h"], input_type={"user": cfg["user"], "photo": cfg["photo"]},
                              learnable_bias=cfg.get("learnable_bias", 0), exposure_prob=cfg["exposure_prob"],
                              fusion_heads=cfg.get("fusion_heads", 2), loss_type_list=cfg["loss_type_list"],
                              loss_weight=cfg["loss_weight"], mask_loss=cfg.get("mask_loss", 0), use_pe=cfg.get("use_pe", 1))


def build_ff_model(cfg):
    """helpers.build_model with ``ff_dim_lvls = cfg["ff"]``."""
    import segmminterest_amd as M
    S, N, d, h = cfg["S"], cfg["N"], cfg["d"], cfg["h"]
    args = ff_args(cfg)

    def backbone(user_id_max, video_id_max, max_usr_len):
        return M.SegFormerX(d_model_in=d, d_model_lvls=[d] * N, num_head_lvls=[h] * N, ff_dim_lvls=list(cfg["ff"]),
                            input_vid_dim=max(cfg["D_in"], 1), input_usr_dim=max(cfg["D_in"], 1), max_vid_len=S,
                            max_usr_len=max_usr_len, sr_ratio_lvls=[1] * N, use_patch_merge=[False] * N, output_layers=[-1],
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
