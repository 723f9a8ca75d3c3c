"""Spatial-reduction attention (sr_ratio > 1) without a GPU: ``sr_ref`` -- the oracle with reduced layers -- against fixtures
captured from the real reference built with ``sr_ratio_lvls != [1] * N`` (tests/golden/sr, tools/gen_golden_sr.py), with the criteria
of test_oracle_golden.py; the numpy statements of the two kernels against torch's own conv / pool; and the facade's opt-in,
construction, refusals and liveness surface."""
import argparse
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sr_ref as R
from helpers import ROOT
from sr_cases import SR_EVAL_CASES, SR_TRAIN_CASES, build_sr_model, load_sr_case, sr_args
from test_oracle_golden import MaskReplay, _live_call_order, adam_close

OK_SHAPES = [(40, 2), (41, 2), (40, 4), (41, 4), (40, 8), (41, 8), (8, 8), (2, 2), (9, 3), (15, 5), (12, 6), (14, 7)]


# ------------------------------------------------------------------------------------------------ the numpy statements
@pytest.mark.parametrize("S,r", OK_SHAPES)
def test_pack_then_gemm_is_the_conv_and_the_pool_is_max_pool(S, r):
    """A . W2^T + b with W2 = weight.view(d, r d) is torch's Conv1d(d, d, r, stride = r, padding = (r - 1) // 2) -- the K order
    c r + t is the weight as stored; the pooled mask is MaxPool1d(r, r) of the mask."""
    g = torch.Generator().manual_seed(S * 16 + r)
    B, d = 3, 8
    x = torch.randn(B, S, d, generator=g, dtype=torch.float64)
    w = torch.randn(d, d, r, generator=g, dtype=torch.float64)
    b = torch.randn(d, generator=g, dtype=torch.float64)
    want = F.conv1d(x.transpose(1, 2), w, b, stride=r, padding=(r - 1) // 2).transpose(1, 2)
    Ls = R.sr_len(S, r)
    assert want.shape[1] == Ls
    A = R.pack_np(x.numpy(), r)
    got = (A @ w.reshape(d, d * r).numpy().T + b.numpy()).reshape(B, Ls, d)
    assert np.abs(got - want.numpy()).max() < 1e-12
    assert np.array_equal(R.pack(x, r).reshape(B * Ls, r * d).numpy(), A)
    m = torch.rand(B, S, generator=g) < 0.3
    m[0] = False
    m[1] = True
    pool = F.max_pool1d(m[:, None, :].float(), kernel_size=r, stride=r)[:, 0] > 0
    assert np.array_equal(R.mask_pool_np(m.numpy(), r), pool.numpy())


@pytest.mark.parametrize("S,r", OK_SHAPES)
def test_unpack_is_the_adjoint_of_pack(S, r):
    """<pack(x), dA> == <x, unpack(dA)> for integer-valued operands (exact), every row outside a window gets the residual alone."""
    rng = np.random.RandomState(S + r)
    B, d = 2, 4
    Ls = R.sr_len(S, r)
    x = rng.randint(-8, 9, size=(B, S, d)).astype(np.float64)
    dA = rng.randint(-8, 9, size=(B * Ls, r * d)).astype(np.float64)
    G0 = R.unpack_np(dA, None, B, S, d, r)
    assert float((R.pack_np(x, r) * dA).sum()) == float((x * G0).sum())
    res = rng.randint(-8, 9, size=(B, S, d)).astype(np.float64)
    assert np.array_equal(R.unpack_np(dA, res, B, S, d, r), res + G0)
    p = (r - 1) // 2
    for i in range(S):
        if (i + p) // r >= Ls:
            assert not G0[:, i].any()


@pytest.mark.parametrize("S,r", [(42, 4), (40, 3), (43, 4), (44, 8), (1, 2), (7, 8)])
def test_length_mismatch_is_refused_by_name(S, r):
    """Where the conv length and the mask-pool length differ (the reference raises IndexError) -- or no window exists -- the host
    check, the engine's pre-pass check and both C entry points refuse, naming S and the ratio; nothing is launched."""
    from segmminterest_amd import engine as E
    from segmminterest_amd import hipabi as H
    with pytest.raises(ValueError):
        R.sr_len(S, r)
    with pytest.raises(RuntimeError, match=r"S=%d .*sr_ratio=%d" % (S, r)):
        H.sr_len(S, r)
    run = E.BackboneRun.__new__(E.BackboneRun)
    run.abl, run.N, run.mode, run.bb = "ours", 3, "joint", argparse.Namespace(sr_ratio_lvls=[1, r, 1])
    with pytest.raises(RuntimeError, match=r"S=%d .*sr_ratio=%d" % (S, r)):
        run._require_attn_keys(S, 10)
    L = H.lib()
    for rc in (L.segmm_sr_pack(None, 32, None, None, None, None, 2, S, 32, r, None), L.segmm_sr_unpack(None, None, None, 2, S, 32, r, None)):
        assert rc != 0
        msg = H._lib_real().segmm_last_error().decode()
        assert "S=%d" % S in msg and "r=%d" % r in msg, msg


def test_entry_points_refuse_other_ratios_and_widths_by_name():
    from segmminterest_amd import hipabi as H
    L = H.lib()
    for r in (1, 9, 0):
        assert L.segmm_sr_pack(None, 32, None, None, None, None, 2, 40, 32, r, None) != 0
        assert "r=%d" % r in H._lib_real().segmm_last_error().decode()
        with pytest.raises(NotImplementedError, match="sr_ratio = %d" % r):
            H.sr_len(40, r)
    for d in (30, 2, 0):
        assert L.segmm_sr_unpack(None, None, None, 2, 40, d, 2, None) != 0
        assert "d=%d" % d in H._lib_real().segmm_last_error().decode()


def test_generated_abi_tables_are_current():
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_cmd_dispatch.py"), "--check"])
    from segmminterest_amd import hipabi as H
    assert {"segmm_sr_pack", "segmm_sr_unpack"} <= set(H.op_ids())          # commands of a recorded step


# ------------------------------------------------------------------------------------------------ sr_ref against the reference
@pytest.mark.parametrize("name", SR_EVAL_CASES + SR_TRAIN_CASES)
def test_fixture_has_the_convs_it_names(name):
    cfg, g, _, _ = load_sr_case(name)
    d = cfg["d"]
    assert any(r > 1 for r in cfg["sr"])
    for b in ("backbone1", "backbone2"):
        if b + ".vid_ln.weight" not in g["sd"]:
            continue
        for i, r in enumerate(cfg["sr"]):
            k = "%s.encoder.layers.%d.cross_attn.sr.weight" % (b, i)
            assert (k in g["sd"]) is (r > 1), k
            if r > 1:
                assert tuple(g["sd"][k].shape) == (d, d, r) and tuple(g["sd"][k[:-6] + "bias"].shape) == (d,)


@pytest.mark.parametrize("name", SR_EVAL_CASES)
def test_sr_ref_forward_loss_grads(name):
    cfg, g, nograd, _ = load_sr_case(name)
    out, grads = R.forward_backward(g["sd"], cfg, g["in"])
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
    # the reduction is not a no-op: the same weights with every ratio read as 1 give other logits
    plain = R.O.model_forward(g["sd"], cfg, {k: v.clone() for k, v in g["in"].items()}, "inference")["logits"]
    assert float((plain - g["inf"]["logits"]).abs().max()) > 1e-3


@pytest.mark.parametrize("name", SR_EVAL_CASES)
def test_sr_ref_dead_layers_do_not_change_outputs(name):
    cfg, g, _, _ = load_sr_case(name)
    a = R.model_forward(g["sd"], cfg, {k: v.clone() for k, v in g["in"].items()}, "inference", skip_dead=True)
    b = R.model_forward(g["sd"], cfg, {k: v.clone() for k, v in g["in"].items()}, "inference", skip_dead=False)
    assert torch.equal(a["logits"], b["logits"])
    assert torch.allclose(a["logits"], g["inf"]["logits"], atol=2e-6, rtol=1e-5)


@pytest.mark.parametrize("name", [n for n in SR_EVAL_CASES if load_sr_case(n)[1]["adam3"]])
def test_sr_ref_adamw_steps(name):
    cfg, g, nograd, extra = load_sr_case(name)
    _, own = R.forward_backward(g["sd"], cfg, g["in"])
    p1, _ = R.train_steps(g["sd"], cfg, g["in"], 1)
    for k, ref in g["adam1"].items():
        assert adam_close(p1[k], ref, [g["grad"].get(k), own.get(k)], 2e-6, 1e-5, 1), k
    p3, losses = R.train_steps(g["sd"], cfg, g["in"], 3)
    for k, ref in g["adam3"].items():
        assert adam_close(p3[k], ref, [g["grad"].get(k), own.get(k)], 2e-5, 1e-4, 3), k
    for k in nograd:
        assert torch.equal(p3[k], g["sd"][k]), k


@pytest.mark.parametrize("name", SR_TRAIN_CASES)
def test_sr_ref_train_mode_dropout_placement(name):
    """The reference's masks replayed in call order, whole graph (MaskReplay asserts every mask's shape against the tensor dropped):
    the logits masks of a reduced layer are [B, h, Lq, Ls + Lt]."""
    cfg, g, nograd, extra = load_sr_case(name)
    masks, nfwd = extra["masks"], extra["mask_calls_fwd"]
    feed = MaskReplay(masks)
    out, grads = R.forward_backward(g["sd"], cfg, g["in"], skip_dead=False, drop=feed)
    assert feed.i == nfwd, "sr_ref called dropout %d times, the reference %d times" % (feed.i, nfwd)
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
    B, S, Lt, h = cfg["B"], cfg["S"], cfg["Lt"], cfg["h"]
    for i, r in enumerate(cfg["sr"]):          # call positions of one forward: 2 embedding calls, then 8 per layer; 0 / 1 are the logits
        assert tuple(masks[2 + 8 * i][1].shape) == (B, h, S, S // r + Lt), i
        assert tuple(masks[2 + 8 * i + 1][1].shape) == (B, h, Lt, S // r + Lt), i


@pytest.mark.parametrize("name", SR_TRAIN_CASES)
def test_sr_ref_train_mode_live_graph(name):
    cfg, g, nograd, extra = load_sr_case(name)
    order, ncalls = _live_call_order(cfg)
    assert ncalls == extra["mask_calls_fwd"]
    feed = MaskReplay(extra["masks"], order)
    out, grads = R.forward_backward(g["sd"], cfg, g["in"], skip_dead=True, drop=feed)
    assert feed.i == len(order)
    assert torch.allclose(out["logits"], g["out"]["logits"], atol=2e-6, rtol=1e-5)
    assert abs(float(out["loss"]) - float(g["out"]["loss"])) < 2e-5 * max(1.0, abs(float(g["out"]["loss"])))
    for k, ref in g["grad"].items():
        scale = max(float(ref.abs().max()), 1e-6)
        assert float((grads[k] - ref).abs().max()) <= 2e-5 * scale + 2e-7, k


@pytest.mark.parametrize("name", SR_TRAIN_CASES)
def test_sr_ref_train_mode_adamw_steps(name):
    cfg, g, nograd, extra = load_sr_case(name)
    masks, nfwd = extra["masks"], extra["mask_calls_fwd"]
    assert len(masks) == 4 * nfwd
    params = {k: v.clone() for k, v in g["sd"].items()}
    m = {k: torch.zeros_like(p) for k, p in params.items()}
    v = {k: torch.zeros_like(p) for k, p in params.items()}
    step_grads = []
    for step in range(1, 4):
        feed = MaskReplay(masks, start=step * nfwd)
        _, grads = R.forward_backward(params, cfg, g["in"], skip_dead=False, drop=feed)
        step_grads.append(grads)
        with torch.no_grad():
            R.O.adamw_step(params, grads, m, v, step)
        if step in (1, 3):
            for k, ref in g["adam%d" % step].items():
                grads_k = [g["grad"].get(k)] + [gs.get(k) for gs in step_grads]
                assert adam_close(params[k], ref, grads_k, 2e-6 if step == 1 else 2e-5, 1e-4, step), (k, step)


# ------------------------------------------------------------------------------------------------ the facade
@pytest.mark.parametrize("name", SR_EVAL_CASES + SR_TRAIN_CASES)
def test_facade_loads_the_reference_state_dict_and_agrees_on_liveness(name):
    from segmminterest_amd import engine as E
    cfg, g, nograd, _ = load_sr_case(name)
    model = build_sr_model(cfg)
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
        for i, layer in enumerate(bb.encoder.layers):
            assert hasattr(layer.cross_attn, "sr") is (cfg["sr"][i] > 1), i
        for _, groups in E.backbone_layout(pre, bb):
            for grp in groups:
                live.update(grp)
    want = {k for k in g["grad"] if k.startswith("backbone")}
    assert live == want
    assert live.isdisjoint(nograd)
    # the exact-liveness rule of the conv: live iff the layer is live and projects video keys; the last layer's is only ever loaded
    N, mode = cfg["N"], E.attn_mode(model.backbone1)
    for i, r in enumerate(cfg["sr"]):
        k = "backbone1.encoder.layers.%d.cross_attn.sr.weight" % i
        if r > 1:
            assert (k in live) is (i <= (N - 3 if mode == "cross" else N - 2)), (k, mode)
    if name == "sr_crossatt_N3":
        assert "backbone1.encoder.layers.1.cross_attn.sr.weight" in nograd


def test_reduced_layer_splits_the_video_group():
    """Queries read Xv, keys and values read Xsr: two fused groups where a default layer has one; ``sr`` rides as singles."""
    from segmminterest_amd import engine as E
    cfg, _, _, _ = load_sr_case("sr_img_d32_N3")
    model = build_sr_model(cfg)
    buckets = dict(E.backbone_layout("backbone1.", model.backbone1))
    ca = "backbone1.encoder.layers.%d.cross_attn."
    g0 = [grp for grp in buckets["backbone1.layer0"]]
    assert [ca % 0 + n + ".weight" for n in ("v2v_proj.0", "t2v_proj.0")] in g0
    assert [ca % 0 + n + ".weight" for n in ("v2v_proj.1", "v2v_proj.2", "v2t_proj.1", "v2t_proj.2")] in g0
    assert [ca % 0 + "sr.weight"] in g0 and [ca % 0 + "sr.bias"] in g0
    g1 = [grp for grp in buckets["backbone1.layer1"]]
    assert [ca % 1 + n + ".weight" for n in ("v2v_proj.1", "v2v_proj.2")] in g1 and [ca % 1 + "sr.bias"] in g1
    # [1] * N with the key: the layout of the default model, group for group
    import segmminterest_amd as M
    kw = dict(d_model_in=32, d_model_lvls=[32] * 3, num_head_lvls=[4] * 3, ff_dim_lvls=[32] * 3, input_vid_dim=48, input_usr_dim=48,
              max_vid_len=40, max_usr_len=10, sr_ratio_lvls=[1] * 3, use_patch_merge=[False] * 3, output_layers=[-1])
    assert E.backbone_layout("", M.SegFormerX(model_cfg=argparse.Namespace(sr_attn=1), **kw)) == E.backbone_layout("", M.SegFormerX(**kw))


def _bb(sr, model_cfg=None, d=32, h=4):
    import segmminterest_amd as M
    N = len(sr)
    return M.SegFormerX(d_model_in=d, d_model_lvls=[d] * N, num_head_lvls=[h] * N, ff_dim_lvls=[d] * N, input_vid_dim=48,
                        input_usr_dim=48, max_vid_len=40, max_usr_len=10, sr_ratio_lvls=sr, use_patch_merge=[False] * N,
                        output_layers=[-1], model_cfg=model_cfg)


FORBIDDEN = ("d_model_lvls", "patch merging", "head count", "output_layers", "ff_dim")


def test_without_the_key_the_refusal_stands_and_names_the_key():
    from segmminterest_amd.encoder import SegFormerXAttention
    for make in (lambda: _bb([2, 1]), lambda: _bb([2, 1], argparse.Namespace(sr_attn=0)), lambda: _bb([2, 1], argparse.Namespace()),
                 lambda: SegFormerXAttention(32, 4, sr_ratio=2)):
        with pytest.raises(NotImplementedError) as e:
            make()
        msg = str(e.value)
        assert "sr_ratio" in msg and "sr_attn" in msg
        assert not any(w in msg for w in FORBIDDEN), msg
    assert not any(w in "sr_attn" for w in FORBIDDEN)


def test_construction_with_the_key():
    bb = _bb([2, 8, 1], argparse.Namespace(sr_attn=1))
    for i, r in enumerate([2, 8, 1]):
        ca = bb.encoder.layers[i].cross_attn
        assert hasattr(ca, "sr") is (r > 1)
        if r > 1:
            assert isinstance(ca.sr, torch.nn.Conv1d) and tuple(ca.sr.weight.shape) == (32, 32, r) and tuple(ca.sr.bias.shape) == (32,)
            assert ca.sr.stride == (r,) and ca.sr.padding == ((r - 1) // 2,) and ca.sr.kernel_size == (r,)
    other = _bb([2, 8, 1], argparse.Namespace(sr_attn=1))
    other.load_state_dict(bb.state_dict(), strict=True)
    with pytest.raises(RuntimeError, match="Unexpected key|Missing key|size mismatch"):
        _bb([2, 4, 1], argparse.Namespace(sr_attn=1)).load_state_dict(bb.state_dict(), strict=True)
    assert bb.sr_ratio_lvls == [2, 8, 1] and _bb([1, 1]).sr_ratio_lvls == [1, 1]


@pytest.mark.parametrize("r", [9, 16, 0, -2])
def test_other_ratios_are_refused_by_name(r):
    with pytest.raises(NotImplementedError) as e:
        _bb([r, 1], argparse.Namespace(sr_attn=1))
    msg = str(e.value)
    assert "sr_ratio = %d" % r in msg and not any(w in msg for w in FORBIDDEN), msg


def test_init_model_sr_ratio_is_opt_in():
    from segmminterest_amd.trainer import default_args, init_model
    kw = dict(n_users=5, n_items=5, input_dim=48, max_vid_len=40, max_usr_len=10)
    io = {"user": "image", "photo": "image"}

    def ratios(model):
        return [int(l.cross_attn.sr.weight.shape[2]) if hasattr(l.cross_attn, "sr") else 1 for l in model.backbone1.encoder.layers]
    a = default_args(num_layers_enc=3, d_model=32, nhead=4, input_type=io, sr_attn=1)
    assert ratios(init_model(a, **kw)) == [1, 1, 1] and ratios(init_model(a, sr_ratio=None, **kw)) == [1, 1, 1]
    assert ratios(init_model(a, sr_ratio=2, **kw)) == [2, 2, 2]
    assert ratios(init_model(a, sr_ratio=[4, 2, 1], **kw)) == [4, 2, 1]
    with pytest.raises(ValueError, match="sr_ratio lists 2 ratios for num_layers_enc = 3"):
        init_model(a, sr_ratio=[2, 1], **kw)
    with pytest.raises(NotImplementedError, match="sr_attn"):
        init_model(default_args(num_layers_enc=3, d_model=32, nhead=4, input_type=io), sr_ratio=2, **kw)
    for abl in ("SelfMLP", "CrossMLP", "w/oAtt"):          # no encoder: the ratios are never looked at, with or without the key
        m = init_model(default_args(num_layers_enc=5, d_model=32, nhead=4, input_type=io, ablation_type=abl), sr_ratio=[9, 9, 9], **kw)
        assert not hasattr(m.backbone1, "encoder")


def test_reduced_keys_move_the_192_limit():
    """pad16(S // r) + pad16(Lt) <= 192 per layer: S = 160, Lt = 100 passes with [4, 4, 1] and is refused, with today's message, at
    [1, 1, 1] and where only the video-only layer is reduced."""
    from segmminterest_amd import engine as E

    def run(sr):
        r_ = E.BackboneRun.__new__(E.BackboneRun)
        r_.abl, r_.N, r_.mode, r_.bb = "ours", 3, "joint", argparse.Namespace(sr_ratio_lvls=sr)
        return r_
    run([4, 4, 1])._require_attn_keys(160, 100)
    for sr in ([1, 1, 1], [1, 4, 1], [4, 1, 1]):
        with pytest.raises(RuntimeError, match=r"> 192 not built .*pad16\(S\) \+ pad16\(Lt\) <= 192"):
            run(sr)._require_attn_keys(160, 100)
    assert run([4, 2, 1])._attn_calls.__func__ is E.BackboneRun._attn_calls
    r_ = run([4, 2, 1])
    r_.S, r_.Lt = 96, 10
    assert r_._attn_calls() == [(96, 24, 10), (10, 24, 10), (96, 48, 10)]
