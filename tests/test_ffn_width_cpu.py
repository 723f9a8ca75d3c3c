"""Encoder layers whose feed-forward width differs from d_model, without a GPU: the CPU oracle against fixtures captured from
the real reference built with ``ff_dim_lvls != [d] * N`` (tests/golden/ffn, tools/gen_golden_ffn.py), with the criteria of
test_oracle_golden.py, and the facade's construction, state-dict and liveness surface."""
import os
import sys

import pytest
import torch

from ffn_cases import FF_EVAL_CASES, FF_TRAIN_CASES, build_ff_model, load_ff_case
from helpers import ROOT
from test_oracle_golden import MaskReplay, _live_call_order, adam_close

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import segmm_oracle as O  # noqa: E402


def _mlp_shapes(sd):
    """name -> shape of every encoder-layer MLP weight (both sides, every backbone) in a state dict."""
    return {k: tuple(v.shape) for k, v in sd.items() if (".ff_vid.layers." in k or ".ff_usr.layers." in k) and k.endswith("weight")}


# ------------------------------------------------------------------------------------------------ the oracle against the reference
@pytest.mark.parametrize("name", FF_EVAL_CASES)
def test_fixture_has_the_widths_it_names(name):
    cfg, g, _, _ = load_ff_case(name)
    d = cfg["d"]
    shapes = _mlp_shapes(g["sd"])
    assert shapes
    for k, shp in shapes.items():
        i = int(k.split("encoder.layers.")[1].split(".")[0])
        assert shp == ((cfg["ff"][i], d) if ".layers.0.weight" in k else (d, cfg["ff"][i])), (k, shp)
    assert any(f != d for f in cfg["ff"])


@pytest.mark.parametrize("name", FF_EVAL_CASES)
def test_oracle_forward_loss_grads(name):
    cfg, g, nograd, _ = load_ff_case(name)
    out, grads = O.forward_backward(g["sd"], cfg, g["in"])
    assert torch.allclose(out["logits"], g["out"]["logits"], atol=2e-6, rtol=1e-5)
    for k, ref in g["out"].items():
        if ref.dim() == 0:
            assert torch.allclose(out[k].detach().float(), ref, rtol=2e-5, atol=1e-6), (k, float(out[k]), float(ref))
    assert torch.equal(out["gt"], g["out"]["gt"])
    live = {k for k, v in grads.items() if v is not None and k in g["grad"]}
    assert live == set(g["grad"].keys())
    for k in nograd:
        assert grads[k] is None or float(grads[k].abs().max()) == 0.0, k
    for k, ref in g["grad"].items():
        scale = max(float(ref.abs().max()), 1e-6)
        err = float((grads[k] - ref).abs().max())
        assert err <= 2e-5 * scale + 2e-7, (k, err, scale)


@pytest.mark.parametrize("name", FF_EVAL_CASES)
def test_oracle_dead_layers_do_not_change_outputs(name):
    cfg, g, _, _ = load_ff_case(name)
    a = O.model_forward(g["sd"], cfg, {k: v.clone() for k, v in g["in"].items()}, "inference", skip_dead=True)
    b = O.model_forward(g["sd"], cfg, {k: v.clone() for k, v in g["in"].items()}, "inference", skip_dead=False)
    assert torch.equal(a["logits"], b["logits"])
    assert torch.allclose(a["logits"], g["inf"]["logits"], atol=2e-6, rtol=1e-5)


@pytest.mark.parametrize("name", [n for n in FF_EVAL_CASES if load_ff_case(n)[1]["adam3"]])
def test_oracle_adamw_steps(name):
    cfg, g, nograd, extra = load_ff_case(name)
    _, own = O.forward_backward(g["sd"], cfg, g["in"])
    p1, _ = O.train_steps(g["sd"], cfg, g["in"], 1)
    for k, ref in g["adam1"].items():
        assert adam_close(p1[k], ref, [g["grad"].get(k), own.get(k)], 2e-6, 1e-5, 1), k
    p3, losses = O.train_steps(g["sd"], cfg, g["in"], 3)
    for k, ref in g["adam3"].items():
        assert adam_close(p3[k], ref, [g["grad"].get(k), own.get(k)], 2e-5, 1e-4, 3), k
    for k in nograd:
        assert torch.equal(p3[k], g["sd"][k]), k


@pytest.mark.parametrize("name", FF_TRAIN_CASES)
def test_oracle_train_mode_dropout_placement(name):
    """Mask replay by call position, whole graph.  MaskReplay asserts every mask's shape against the tensor the oracle drops: the
    MLP's inner dropout therefore acts on a [B, L, ff] tensor at the reference's call position (checked below that such masks
    exist, with the layer's own ff, video and user side)."""
    cfg, g, nograd, extra = load_ff_case(name)
    masks, nfwd = extra["masks"], extra["mask_calls_fwd"]
    feed = MaskReplay(masks)
    out, grads = O.forward_backward(g["sd"], cfg, g["in"], skip_dead=False, drop=feed)
    assert feed.i == nfwd, "the oracle called dropout %d times, the reference %d times" % (feed.i, nfwd)
    assert torch.allclose(out["logits"], g["out"]["logits"], atol=2e-6, rtol=1e-5)
    for k, ref in g["out"].items():
        if ref.dim() == 0:
            assert torch.allclose(out[k].detach().float(), ref, rtol=2e-5, atol=1e-6), (k, float(out[k]), float(ref))
    live = {k for k, v in grads.items() if v is not None and k in g["grad"]}
    assert live == set(g["grad"].keys())
    for k in nograd:
        assert grads[k] is None or float(grads[k].abs().max()) == 0.0, k
    for k, ref in g["grad"].items():
        scale = max(float(ref.abs().max()), 1e-6)
        assert float((grads[k] - ref).abs().max()) <= 2e-5 * scale + 2e-7, k
    assert all(abs(p - 0.1) < 1e-12 for p, _ in masks)
    ev = O.model_forward(g["sd"], cfg, {k: v.clone() for k, v in g["in"].items()}, "inference")["logits"]
    assert float((ev - out["logits"].detach()).abs().max()) > 1e-3
    # call positions of one forward (test_oracle_golden._live_call_order): 2 embedding calls, then 8 per layer, of which
    # call 4 is the video MLP's inner dropout and call 6 the user MLP's
    B, S, Lt = cfg["B"], cfg["S"], cfg["Lt"]
    for i, f in enumerate(cfg["ff"]):
        assert tuple(masks[2 + 8 * i + 4][1].shape) == (B, S, f), i
        assert tuple(masks[2 + 8 * i + 6][1].shape) == (B, Lt, f), i


@pytest.mark.parametrize("name", FF_TRAIN_CASES)
def test_oracle_train_mode_live_graph(name):
    cfg, g, nograd, extra = load_ff_case(name)
    order, ncalls = _live_call_order(cfg)
    assert ncalls == extra["mask_calls_fwd"]
    feed = MaskReplay(extra["masks"], order)
    out, grads = O.forward_backward(g["sd"], cfg, g["in"], skip_dead=True, drop=feed)
    assert feed.i == len(order)
    assert torch.allclose(out["logits"], g["out"]["logits"], atol=2e-6, rtol=1e-5)
    assert abs(float(out["loss"]) - float(g["out"]["loss"])) < 2e-5 * max(1.0, abs(float(g["out"]["loss"])))
    for k, ref in g["grad"].items():
        scale = max(float(ref.abs().max()), 1e-6)
        assert float((grads[k] - ref).abs().max()) <= 2e-5 * scale + 2e-7, k


@pytest.mark.parametrize("name", FF_TRAIN_CASES)
def test_oracle_train_mode_adamw_steps(name):
    cfg, g, nograd, extra = load_ff_case(name)
    masks, nfwd = extra["masks"], extra["mask_calls_fwd"]
    assert len(masks) == 4 * nfwd
    params = {k: v.clone() for k, v in g["sd"].items()}
    m = {k: torch.zeros_like(p) for k, p in params.items()}
    v = {k: torch.zeros_like(p) for k, p in params.items()}
    step_grads = []
    for step in range(1, 4):
        feed = MaskReplay(masks, start=step * nfwd)
        _, grads = O.forward_backward(params, cfg, g["in"], skip_dead=False, drop=feed)
        step_grads.append(grads)
        with torch.no_grad():
            O.adamw_step(params, grads, m, v, step)
        if step in (1, 3):
            for k, ref in g["adam%d" % step].items():
                grads_k = [g["grad"].get(k)] + [gs.get(k) for gs in step_grads]
                assert adam_close(params[k], ref, grads_k, 2e-6 if step == 1 else 2e-5, 1e-4, step), (k, step)


# ------------------------------------------------------------------------------------------------ the facade
@pytest.mark.parametrize("name", FF_EVAL_CASES + FF_TRAIN_CASES)
def test_facade_loads_the_reference_state_dict_and_agrees_on_liveness(name):
    from segmminterest_amd import engine as E
    cfg, g, nograd, _ = load_ff_case(name)
    model = build_ff_model(cfg)
    sd = model.state_dict()
    assert set(sd.keys()) == set(g["sd"].keys())
    for k, v in g["sd"].items():
        assert tuple(sd[k].shape) == tuple(v.shape), k
    model.load_state_dict(g["sd"], strict=True)
    for k, v in model.state_dict().items():
        assert torch.equal(v, g["sd"][k]), k
    live = set()
    for pre, bb in (("backbone1.", model.backbone1), ("backbone2.", getattr(model, "backbone2", None))):
        if bb is None:
            continue
        for _, groups in E.backbone_layout(pre, bb):
            for grp in groups:
                live.update(grp)
    want = {k for k in g["grad"] if k.startswith("backbone")}
    assert live == want
    assert live.isdisjoint(nograd)


def _bb(ff, d=32, h=4, **kw):
    import segmminterest_amd as M
    N = len(ff)
    a = dict(d_model_in=d, d_model_lvls=[d] * N, num_head_lvls=[h] * N, ff_dim_lvls=ff, input_vid_dim=48, input_usr_dim=48,
             max_vid_len=40, max_usr_len=10, sr_ratio_lvls=[1] * N, use_patch_merge=[False] * N, output_layers=[-1])
    a.update(kw)
    return M.SegFormerX(**a)


def test_construction_with_per_layer_widths():
    bb = _bb([64, 96, 48])          # (the last, dead layer's width differs from d too: it is only ever loaded)
    for i, f in enumerate([64, 96, 48]):
        for side in ("ff_vid", "ff_usr"):
            mlp = getattr(bb.encoder.layers[i], side)
            assert tuple(mlp.layers[0].weight.shape) == (f, 32) and tuple(mlp.layers[1].weight.shape) == (32, f)
            assert tuple(mlp.layers[0].bias.shape) == (f,) and tuple(mlp.layers[1].bias.shape) == (32,)
    # a state dict with these shapes round-trips; one built with other widths does not load
    other = _bb([64, 96, 48])
    other.load_state_dict(bb.state_dict(), strict=True)
    with pytest.raises(RuntimeError, match="size mismatch"):
        _bb([64, 96, 32]).load_state_dict(bb.state_dict(), strict=True)
    # a multiple of 4 that is no multiple of 32 is built (its GEMMs take the fp32-operand kernels)
    assert tuple(_bb((36, 32)).encoder.layers[0].ff_usr.layers[0].weight.shape) == (36, 32)


@pytest.mark.parametrize("ff,layer", [([64, 30, 32], 1), ([30, 32], 0), ([32, 0], 1), ([32, -32], 1), ([32, 32, 34], 2)])
def test_bad_width_names_the_layer(ff, layer):
    with pytest.raises(ValueError, match=r"ff_dim_lvls\[%d\].*layer %d" % (layer, layer)):
        _bb(ff)


def test_wrong_number_of_widths():
    import segmminterest_amd as M
    with pytest.raises(ValueError, match="ff_dim_lvls has 2 entries for 3 layers"):
        M.SegFormerX(d_model_in=32, d_model_lvls=[32] * 3, num_head_lvls=[4] * 3, ff_dim_lvls=[64, 64], input_vid_dim=48,
                     input_usr_dim=48, max_vid_len=40, max_usr_len=10, sr_ratio_lvls=[1] * 3, use_patch_merge=[False] * 3,
                     output_layers=[-1])


def test_each_remaining_refusal_names_only_what_it_refuses():
    cases = [(dict(d_model_lvls=[32, 64]), "d_model_lvls"), (dict(sr_ratio_lvls=[2, 1]), "sr_ratio"),
             (dict(use_patch_merge=[True, False]), "patch merging"), (dict(num_head_lvls=[4, 8]), "head count"),
             (dict(output_layers=[0, 1]), "output_layers")]
    words = [w for _, w in cases] + ["ff_dim"]
    for kw, word in cases:
        with pytest.raises(NotImplementedError) as e:
            _bb([64, 32], **kw)
        msg = str(e.value)
        assert word in msg
        assert not any(w in msg for w in words if w != word), msg


def test_mlp_ablations_ignore_the_widths():
    import argparse
    for abl in ("SelfMLP", "CrossMLP", "w/oAtt"):
        N = 5
        bb = _bb([30, 7, 0, 64, 32], model_cfg=argparse.Namespace(ablation_type=abl, num_layers_enc=N))          # never looked at
        assert not hasattr(bb, "encoder") and hasattr(bb, "encoder_mlp")


def test_init_model_ff_dim_is_opt_in():
    from segmminterest_amd.trainer import default_args, init_model
    a = default_args(num_layers_enc=3, d_model=32, nhead=4, input_type={"user": "image", "photo": "image"}, ff_dim=512)

    def widths(model):
        return [tuple(l.ff_vid.layers[0].weight.shape) for l in model.backbone1.encoder.layers]
    kw = dict(n_users=5, n_items=5, input_dim=48, max_vid_len=40, max_usr_len=10)
    assert widths(init_model(a, **kw)) == [(32, 32)] * 3          # args.ff_dim is NOT read (main...SegMM.py:91)
    assert widths(init_model(a, ff_dim=None, **kw)) == [(32, 32)] * 3
    assert widths(init_model(a, ff_dim=64, **kw)) == [(64, 32)] * 3
    assert widths(init_model(a, ff_dim=[64, 96, 32], **kw)) == [(64, 32), (96, 32), (32, 32)]
    with pytest.raises(ValueError, match="num_layers_enc"):
        init_model(a, ff_dim=[64, 96], **kw)
    with pytest.raises(ValueError, match=r"ff_dim_lvls\[0\]"):
        init_model(a, ff_dim=30, **kw)
    both = default_args(num_layers_enc=2, d_model=32, nhead=4)
    m = init_model(both, ff_dim=[128, 32], n_users=5, n_items=5, input_dim=48)
    assert widths(m) == [(128, 32), (32, 32)] and tuple(m.backbone2.encoder.layers[0].ff_usr.layers[1].weight.shape) == (32, 128)


def test_checkpointer_round_trips_a_reference_checkpoint(tmp_path):
    """A reference checkpoint with ff != d (the fixture's state dict) through CheckPointer.save_checkpoint / load_checkpoint."""
    from segmminterest_amd.trainer import CheckPointer
    cfg, g, _, _ = load_ff_case("ff_narrow_d64_N3")
    model = build_ff_model(cfg)
    model.load_state_dict(g["sd"], strict=True)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
    ck = CheckPointer("loss", str(tmp_path))
    ck.save_checkpoint(model, opt, 1, {"loss": 1.0})
    again = build_ff_model(cfg)
    ck.load_checkpoint(again, None)
    for k, v in again.state_dict().items():
        assert torch.equal(v, g["sd"][k]), k
