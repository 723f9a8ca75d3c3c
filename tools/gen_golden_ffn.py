#!/usr/bin/env python
"""Golden vectors of the REAL reference with feed-forward widths that differ from d_model (TEST INFRASTRUCTURE ONLY).

Runs only where the reference checkout exists (``oracle/ref_import.py`` finds it).  Same recipe and file format as
``oracle/gen_golden.py`` -- its ``perturb``, ``make_inputs``, ``_gen_case_body`` and ``MaskRecorder`` are imported, not copied --
with one difference: the model builder below passes a per-layer ``ff_dim_lvls`` (the case's ``"ff"`` list, which therefore also
lands in the fixture's ``cfg`` JSON).  The fixtures go to ``tests/golden/ffn/``: a directory of their own, because every ``.npz``
directly under ``tests/golden/`` is picked up by the existing fixture-parametrised tests, whose model builder hard-codes
``ff_dim_lvls = [d] * N``.  ``helpers.load_case("ffn/<name>")`` reads them.

Every file stays under 1 MiB (``slim``, ``coarsen_dead``): dead parameters are coarse values, the optimizer-step copies of dead
parameters are left out, and a fixture that is still too large keeps its ``grad/`` group in ``<name>.grad.npz`` next to it.

    python tools/gen_golden_ffn.py            # regenerate every fixture of this family
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)

import ref_import  # noqa: E402
import gen_golden as G  # noqa: E402

# layer N-1 is dead in every case: its width is only ever loaded, never computed with.  ff_narrow_d64_N3: 32 < d, then 160 > d.
CASES = {
    "ff_img_d32_N3": dict(user="image", photo="image", d=32, h=4, N=3, S=40, Lt=10, D_in=48, B=8,
                          loss="interestBPR,surviveCE", adam=True, ff=[64, 96, 32]),
    "ff_both_d32_N2": dict(user="both", photo="both", d=32, h=4, N=2, S=40, Lt=10, D_in=48, B=8,
                           loss="interestBPR", fusion_heads=2, n_users=50, n_items=200, adam=True, ff=[128, 32]),
    "ff_crossatt_N3": dict(user="image", photo="image", d=32, h=4, N=3, S=40, Lt=10, D_in=48, B=8,
                           loss="interestBPR", ablation="CrossAtt", ff=[96, 64, 32]),
    "ff_narrow_d64_N3": dict(user="image", photo="image", d=64, h=4, N=3, S=40, Lt=7, D_in=40, B=5,
                             loss="interestBPR", ff=[32, 160, 64]),
}
TRAIN_CASES = {
    "train_ff_img_d32_N3": dict(user="image", photo="image", d=32, h=4, N=3, S=40, Lt=10, D_in=48, B=8,
                                loss="interestBPR,surviveCE", adam=True, ff=[64, 96, 32]),
}


def build_reference_model(c, enc, dec):
    """The reference's model for case ``c`` with ``ff_dim_lvls = c["ff"]`` (one width per layer)."""
    S, N, d, h = c["S"], c["N"], c["d"], c["h"]
    ff = list(c["ff"])
    assert len(ff) == N
    cfg = argparse.Namespace(debug=0, num_layers_enc=N, ablation_type=c.get("ablation", "ours"), d_model=d, nhead=h,
                             input_type={"user": c["user"], "photo": c["photo"]}, learnable_bias=c.get("learnable_bias", 0),
                             exposure_prob=[1.0] * S, fusion_heads=c.get("fusion_heads", 2),
                             loss_type_list=[x.strip() for x in c["loss"].split(",")], loss_weight=dict(G.ALL_LOSS_W),
                             mask_loss=c.get("mask_loss", 0), use_pe=c.get("use_pe", 1))

    def backbone(user_id_max, video_id_max, max_usr_len):
        return enc.SegFormerX(d_model_in=d, d_model_lvls=[d] * N, num_head_lvls=[h] * N, ff_dim_lvls=ff,
                              input_vid_dim=max(c["D_in"], 1), input_usr_dim=max(c["D_in"], 1), max_vid_len=S,
                              max_usr_len=max_usr_len, sr_ratio_lvls=[1] * N, use_patch_merge=[False] * N, output_layers=[-1],
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


def coarsen_dead(model, c):
    """Before the reference runs: parameters that can never receive a gradient are rounded to bfloat16-representable fp32 values
    (their low 16 bits are zero, so they deflate to half the size).  They are what the reference then runs with and what the
    fixture records; no output depends on them.  The set comes from a throw-away backward on the case's own inputs."""
    inp = G.make_inputs(c, seed=1)
    model.zero_grad()
    G.run_model(model, inp, "train")["loss"].backward()
    with torch.no_grad():
        for _, p in model.named_parameters():
            if p.grad is None:
                p.copy_(p.to(torch.bfloat16).to(torch.float32))
    model.zero_grad(set_to_none=True)


def slim(path):
    """Keeps a fixture under the size limit of a committed file: the ``adam1/`` / ``adam3/`` copies of parameters without a
    gradient are dropped (AdamW skips them: they equal ``sd/`` bit for bit, which the tests check from ``sd/`` and ``nograd``)."""
    import json
    import numpy as np
    z = np.load(path)
    dead = set(json.loads(str(z["nograd"])))
    blob = {k: z[k] for k in z.files if not (k.split("/", 1)[0] in ("adam1", "adam3") and k.split("/", 1)[1] in dead)}
    for k in z.files:
        if k not in blob:
            assert np.array_equal(z[k], z["sd/" + k.split("/", 1)[1]]), k
    np.savez_compressed(path, **blob)
    if os.path.getsize(path) > (1 << 20):          # (d = 64: parameters and gradients do not fit one file) -> <name>.grad.npz
        gpath = path[:-4] + ".grad.npz"
        np.savez_compressed(gpath, **{k: v for k, v in blob.items() if k.startswith("grad/")})
        np.savez_compressed(path, **{k: v for k, v in blob.items() if not k.startswith("grad/")})
        print("%-28s -> %.0f KB" % (os.path.basename(gpath), os.path.getsize(gpath) / 1024))
        assert os.path.getsize(gpath) <= (1 << 20), gpath
    print("%-28s -> %.0f KB" % (os.path.basename(path), os.path.getsize(path) / 1024))
    assert os.path.getsize(path) <= (1 << 20), path


def main():
    ap_ = argparse.ArgumentParser()
    ap_.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "ffn"))
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
