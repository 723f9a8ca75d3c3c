"""Streamed attention (csrc/attention_stream.h) on the MI355X: more than 192 padded keys, up to 256 tokens per key block and 256
queries.  Kernel level: forward and the phase-0 backward against the fp64 restatement of test_ops_gpu (its input recipe, the absolute
bounds of test_long_rows_gpu.test_attention_fwd_bwd_long_blocks: |O - ref| < 2e-5, every gradient < 5e-5), dropout through the
kernel's own mask, empty key blocks, fully masked rows, bitwise reproducibility, the knob ATT_STREAM against the held kernels
at shapes both take, the plane output.  Model level (``model_cfg.attn_stream = 1``): whole models against the CPU oracle, AdamW
steps, recorded steps, validation, and the default that stays the default.  Run with ``pytest -m gpu``.

The kernel-level bounds here (2e-5, 5e-5) are COARSE end-to-end checks: fixed absolute tolerances, several hundred fp32 ulps of a
typical output.  The streamed kernels are pinned to the float64 statement at every built head dim, per element and under the
online softmax's own derived bounds, by tests/test_attn_wide_stream_float64_gpu.py (tests/attn_ref.py); what this module adds to
that is reproducibility, the knob against the held kernels, and the model-level and recorded-step cases."""
import os
import sys

import numpy as np
import pytest
import torch

from helpers import LOSS_SLOTS, ROOT, build_model, call_model, loss_check, oracle_loss
from test_long_rows_gpu import _long_model_case, _oracle_model
from test_model_gpu import _check_live_grads
from test_ops_gpu import _attn_ref
from test_planes_gpu import _po, _ref_planes

pytestmark = pytest.mark.gpu
DEV = "cuda"

sys.path.insert(0, os.path.join(ROOT, "oracle"))
from segmminterest_amd.synth import l1_normalize, make_batch  # noqa: E402

FWD_BOUND, GRAD_BOUND = 2e-5, 5e-5
GRADS = ("dQa", "dQb", "dKa", "dVa", "dKb", "dVb")


def _abi():
    from segmminterest_amd import hipabi
    hipabi.lib()
    return hipabi


def _inputs(B, H_, dh, Lq, La, Lb, masks=True):
    """The recipe of test_ops_gpu.test_attention_fwd_bwd; an empty key block keeps zero-row tensors for the reference."""
    d = H_ * dh
    g = torch.Generator().manual_seed(B * 1000 + Lq)
    mk = lambda L: (torch.randn(B, L, d, generator=g) * 0.7).to(DEV)
    t = dict(zip(("Qa", "Qb", "Ka", "Va", "Kb", "Vb"), (mk(Lq), mk(Lq), mk(La), mk(La), mk(Lb), mk(Lb))))
    t["mq"] = (torch.rand(B, Lq, generator=g) < 0.8).to(DEV)
    t["mka"] = (torch.rand(B, La, generator=g) < 0.8).to(DEV)
    t["mkb"] = (torch.rand(B, Lb, generator=g) < 0.7).to(DEV)
    t["mq"][0, 0] = False
    t["mq"][-1, -1] = True
    t["dO"] = torch.randn(B * Lq, d, generator=g).to(DEV)
    return t


def _run(H, shape, t, p=0.0, phases=(0,), po=None, amax_o=None, backward=True):
    """attn_fwd and attn_bwd on the tensors of ``t``; returns O, lse and the six gradients (NaN-filled before the launch)."""
    B, H_, dh, Lq, La, Lb = shape
    d = H_ * dh
    z = lambda x, L: (x, 0) if L else None
    O = torch.full((B * Lq, d), float("nan"), device=DEV)
    lse = torch.full((2, B, H_, Lq), float("nan"), device=DEV)
    views = (z(t["Qa"], 1), z(t["Qb"], 1), d, z(t["Ka"], La), z(t["Va"], La), d, z(t["Kb"], Lb), z(t["Vb"], Lb), d,
             t["mq"], t["mka"] if La else None, t["mkb"] if Lb else None)
    H.attn_fwd(B, H_, dh, Lq, La, Lb, *views, O, d, lse, drop_p=p, seed=11, site=3, po=po, amax_o=amax_o)
    if not backward:
        return O, lse, None
    Dv = torch.full((B, H_, Lq), float("nan"), device=DEV)
    outs = [torch.full_like(t[k], float("nan")) for k in ("Qa", "Qb", "Ka", "Va", "Kb", "Vb")]
    lens = (1, 1, La, La, Lb, Lb)
    for ph in phases:
        H.attn_bwd(B, H_, dh, Lq, La, Lb, *views, lse, O, d, t["dO"], d, Dv, z(outs[0], La), z(outs[1], Lb), d, z(outs[2], La),
                   z(outs[3], La), d, z(outs[4], Lb), z(outs[5], Lb), d, drop_p=p, seed=11, site=3, phase=ph)
    return O, lse, [o if n else None for o, n in zip(outs, (La, Lb) + lens[2:])]


def _mult(H, shape, p):
    """The kernel's own dropout multipliers, sliced to the real keys as in test_ops_gpu.test_attention_dropout_consistency."""
    B, H_, dh, Lq, La, Lb = shape
    La_p, Lb_p = (La + 15) // 16 * 16, (Lb + 15) // 16 * 16
    Tp = La_p + Lb_p
    mult = torch.empty(B * H_ * Lq * Tp, device=DEV)
    H.dropout_mult(mult, mult.numel(), p, 11, 3)
    mult = mult.view(B, H_, Lq, Tp)
    return torch.cat([mult[..., :La], mult[..., La_p:La_p + Lb]], -1).double()


def _check_fp64(H, shape, t, O, outs, p=0.0):
    B, H_, dh, Lq, La, Lb = shape
    d = H_ * dh
    leaves = [t[k].double().requires_grad_(True) for k in ("Qa", "Qb", "Ka", "Va", "Kb", "Vb")]
    ref = _attn_ref(*leaves, t["mq"], t["mka"], t["mkb"], H_, mult=_mult(H, shape, p) if p > 0 else None)
    err = (O.view(B, Lq, d).double() - ref).abs().max().item()
    print("streamed attention %s p=%.1f fwd err %.3e" % (shape, p, err))
    assert err < FWD_BOUND, err
    if outs is None:
        return
    ref.backward(t["dO"].view(B, Lq, d).double())
    for name, got, leaf in zip(GRADS, outs, leaves):
        if got is None:          # the empty key block: its gradients are not written (dQ of its projection is zero)
            continue
        err = (got.double() - leaf.grad).abs().max().item()
        print("streamed attention %s p=%.1f %s err %.3e" % (shape, p, name, err))
        assert err < GRAD_BOUND, (name, err)


# ------------------------------------------------------------------ kernels against fp64
STREAM_SHAPES = [(2, 2, 16, 208, 208, 1), (2, 2, 16, 1, 208, 1), (1, 2, 32, 97, 97, 90), (2, 4, 8, 200, 200, 7), (1, 2, 64, 193, 193, 3),
                 (2, 2, 48, 100, 256, 100), (2, 2, 48, 256, 256, 100), (1, 2, 4, 250, 250, 250)]


@pytest.mark.parametrize("shape", STREAM_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_streamed_fwd_bwd_vs_fp64(shape):
    """13 + 1 tiles (the first shape over the limit) ... 16 + 16 tiles (the maximum); partial tiles in both blocks, one query,
    Lq no multiple of 16, every head dim."""
    H = _abi()
    t = _inputs(*shape)
    O, lse, outs = _run(H, shape, t)
    assert torch.isfinite(lse).all()
    _check_fp64(H, shape, t, O, outs)


@pytest.mark.parametrize("shape", [(2, 2, 16, 40, 208, 10), (1, 2, 48, 100, 256, 100)], ids=lambda s: "-".join(map(str, s)))
def test_streamed_dropout_vs_fp64(shape):
    """p = 0.1: the forward and the backward kernels regenerate one mask, the one segmm_dropout_mult reports."""
    H = _abi()
    t = _inputs(*shape)
    O, lse, outs = _run(H, shape, t, p=0.1)
    _check_fp64(H, shape, t, O, outs, p=0.1)


@pytest.mark.parametrize("shape", [(2, 2, 16, 208, 208, 0), (2, 2, 16, 40, 0, 208)], ids=lambda s: "-".join(map(str, s)))
def test_streamed_one_empty_key_block(shape):
    H = _abi()
    t = _inputs(*shape)
    O, lse, outs = _run(H, shape, t)
    _check_fp64(H, shape, t, O, outs)


def test_streamed_fully_masked_rows():
    """A batch row whose keys are all masked and a batch row whose queries are all masked: the uniform average of the reference
    (finite -10000 fills), finite statistics."""
    H = _abi()
    shape = (2, 2, 16, 48, 208, 16)
    t = _inputs(*shape)
    t["mka"][0] = False
    t["mkb"][0] = False
    t["mq"][1] = False
    O, lse, outs = _run(H, shape, t)
    assert torch.isfinite(O).all() and torch.isfinite(lse).all() and all(torch.isfinite(o).all() for o in outs)
    _check_fp64(H, shape, t, O, outs)


def test_streamed_reproducible_and_phases():
    """The workload's largest call: two runs bitwise equal, phases 1 + 2 + 3 bitwise equal to phase 0, the fused phase refused."""
    H = _abi()
    shape = (2, 2, 48, 256, 256, 100)
    t = _inputs(*shape)
    a = _run(H, shape, t, p=0.1)
    b = _run(H, shape, t, p=0.1)
    c = _run(H, shape, t, p=0.1, phases=(1, 2, 3))
    for what, x in (("second run", b), ("phases 1 + 2 + 3", c)):
        assert torch.equal(a[0], x[0]) and torch.equal(a[1], x[1]), what
        for name, u, v in zip(GRADS, a[2], x[2]):
            assert torch.equal(u, v), (what, name, float((u - v).abs().max()))
    with pytest.raises(RuntimeError, match=r"padded keys > 192 take the streamed backward"):
        _run(H, shape, t, phases=(4,))


# ------------------------------------------------------------------ the knob, at shapes the held kernels take too
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("shape", [(2, 4, 16, 40, 40, 100), (2, 2, 48, 100, 40, 100), (3, 4, 8, 7, 40, 7), (2, 2, 32, 176, 176, 16)],
                         ids=lambda s: "-".join(map(str, s)))
def test_knob_att_stream_against_held_kernels(shape, p):
    """ATT_STREAM = 1: within the fp64 bounds, and against the held forward under the rule between the project's two forward
    forms (test_ops_gpu.test_attention_fwd_lds_staged_form_equals_direct_form)."""
    H = _abi()
    t = _inputs(*shape)
    held = _run(H, shape, t, p=p)
    prev = H.config_set("ATT_STREAM", 1)
    try:
        O, lse, outs = _run(H, shape, t, p=p)
    finally:
        H.config_set("ATT_STREAM", prev)
    assert prev == 0 and H.knob("ATT_STREAM") == 0
    _check_fp64(H, shape, t, O, outs, p=p)
    omax = float(held[0].abs().max())
    assert float((held[0] - O).abs().max()) <= 2e-6 * omax
    assert float((held[1][0] - lse[0]).abs().max()) <= 1e-6 * float(held[1][0].abs().max())          # row maxima
    assert float(((held[1][1] - lse[1]) / held[1][1]).abs().max()) <= 2e-6                             # 1 / row sums


def test_streamed_forward_writes_planes_and_maxima():
    """po= / amax_o= at a streamed shape: the planes are the split pass of the fp32 output (itself held to tests/p32_ref.py by
    test_planes_gpu._ref_planes), bit for bit as for the held kernel; the recorded maximum is max |O|."""
    H = _abi()
    shape = (2, 2, 48, 100, 256, 100)
    B, H_, dh, Lq, La, Lb = shape
    d = H_ * dh
    t = _inputs(*shape)
    pl, hdr, sc, po = _po(H, B * Lq, d, 2.0 ** 12)
    O, lse, _ = _run(H, shape, t, p=0.1, po=po, backward=False)
    ref_pl, _ = _ref_planes(H, O, B * Lq, d, 2.0 ** 12)
    assert torch.equal(pl, ref_pl) and float(hdr[0]) == 2.0 ** 12
    assert float(hdr[H.SITE_HDR:].max()) == float(O.abs().max())
    am = torch.zeros(H.AMAX_SLOTS, device=DEV)
    O2, _, _ = _run(H, shape, t, p=0.1, amax_o=am, backward=False)
    assert torch.equal(O, O2) and float(am.max()) == float(O.abs().max())


# ------------------------------------------------------------------ whole models, model_cfg.attn_stream = 1
def _opt_in(model):
    """What ``model_cfg.attn_stream = 1`` leaves on every backbone (helpers.build_model builds its own model_cfg)."""
    from segmminterest_amd.encoder import SegFormerX
    n = 0
    for m in model.modules():
        if isinstance(m, SegFormerX):
            m.attn_stream = 1
            n += 1
    assert n
    return model


@pytest.mark.parametrize("kind,S,Lt,d,h,N", [("image", 208, 100, 64, 4, 3), ("image", 256, 100, 64, 4, 2), ("id", 256, 1, 64, 4, 2)])
def test_streamed_model_vs_oracle(kind, S, Lt, d, h, N):
    """test_long_rows_gpu.test_long_video_model_vs_oracle beyond 192 keys: logits within 1e-4 of the float64 and the float32
    oracle, losses by loss_check, live gradients by _check_live_grads."""
    cfg, model, inp = _long_model_case(kind, S, Lt, d, h, N)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    ref, rgrads = _oracle_model(sd, cfg, inp, torch.float32)
    t64, _ = _oracle_model(sd, cfg, inp, torch.float64)
    model = _opt_in(model).cuda().eval()
    out = call_model(model, inp, "train", DEV)
    err = (out["logits"].cpu().double() - t64["logits"].detach()).abs().max().item()
    print("streamed model %s logits err vs float64 %.3e" % ((kind, S, Lt, d, h, N), err))
    assert err < 1e-4
    assert (out["logits"].cpu() - ref["logits"].detach()).abs().max().item() < 1e-4
    sc = oracle_loss(t64["logits"].detach(), inp["gt"], dict(cfg, learnable_bias=0))
    for i, name in enumerate(LOSS_SLOTS):
        if name in cfg["loss_type_list"] or name in ("mse", "mse2"):
            loss_check(float(out[name]), float(t64[name].detach()), float(ref[name].detach()), sc["slot_scales"][i], "model:" + name,
                       "%s S=%d" % (kind, S))
    loss_check(float(out["loss"].detach()), float(t64["loss"].detach()), float(ref["loss"].detach()), sc["total_scale"], "model:total",
               "%s S=%d" % (kind, S))
    out["loss"].backward()
    _check_live_grads(model, rgrads)


def _steps_case(S, Lt, opt_in):
    """The model and batch of test_model_gpu.test_long_token_axes_train_steps_keep_the_fp32_projection_buffers."""
    B, D, N, h = 6, 64, 3, 4
    cfg = dict(N=N, h=h, S=S, d=D, D_in=D, Lt=Lt, user="image", photo="image", loss_type_list=["interestBPR"],
               loss_weight={"interestBPR": 1.0, "mse": 1.0}, exposure_prob=[1.0] * S)
    torch.manual_seed(5)
    model = build_model(cfg)
    for m in model.modules():          # train mode (delayed scales, planes from the producers) without the dropout draws
        for a in ("dropout_p", "inner_dropout"):
            if isinstance(getattr(m, a, None), float):
                setattr(m, a, 0.0)
    if opt_in:
        _opt_in(model)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    b = make_batch(B, S, Lt, D, seed=9)
    inp = dict(usr_image=l1_normalize(b["user"]), usr_id=b["user_identity_id"], usr_mask=b["user_mask"],
               vid_image=l1_normalize(b["photo"]), vid_id=b["photo_identity_id"], vid_mask=b["photo_mask"], gt=b["label"])
    batch = dict(user=inp["usr_image"].to(DEV), photo=inp["vid_image"].to(DEV), user_mask=inp["usr_mask"].to(DEV),
                 photo_mask=inp["vid_mask"].to(DEV), label=inp["gt"].to(DEV), user_identity_id=inp["usr_id"].to(DEV),
                 photo_identity_id=inp["vid_id"].to(DEV))
    return cfg, model, sd, inp, batch


def _trainer(model):
    from segmminterest_amd.trainer import Trainer
    tr = Trainer(model.cuda())
    tr.normalize = lambda key, x, *a, **k: x             # already L1-normalised
    return tr


def test_streamed_train_steps_vs_oracle(monkeypatch):
    """Four training-mode AdamW steps at (S, Lt) = (100, 100) -- 224 padded keys, refused without the opt-in -- against the CPU
    oracle's own train loop, under the 2e-4 relative rule of the test that shows the refusal."""
    import segmm_oracle as O
    from segmminterest_amd import engine as E
    monkeypatch.setattr(E, "MLP_INNER_DROPOUT", 0.0)
    cfg, model, sd, inp, batch = _steps_case(100, 100, True)
    ref_losses = O.train_steps(sd, cfg, inp, 4, skip_dead=True)[1]
    tr = _trainer(model)
    got = [float(tr.train_step(batch)["loss"]) for _ in range(4)]
    assert model.training
    for s, (a, r) in enumerate(zip(got, ref_losses)):
        assert abs(a - r) <= 2e-4 * max(1.0, abs(r)), (s, got, ref_losses)


def test_default_still_refuses_and_opt_in_changes_nothing_below_the_limit(monkeypatch):
    """Without attn_stream the (100, 100) model raises the 192 message; with it, a model whose calls all fit the held kernels
    (S = 40, Lt = 100) takes bitwise the steps of one without it."""
    from segmminterest_amd import engine as E
    monkeypatch.setattr(E, "MLP_INNER_DROPOUT", 0.0)
    cfg, model, sd, inp, batch = _steps_case(100, 100, False)
    with pytest.raises(RuntimeError, match=r"> 192 not built .*pad16\(S\) \+ pad16\(Lt\) <= 192"):
        _trainer(model).train_step(batch)
    res = []
    for opt_in in (False, True):
        cfg, model, sd, inp, batch = _steps_case(40, 100, opt_in)
        tr = _trainer(model)
        losses = [float(tr.train_step(batch)["loss"]) for _ in range(3)]
        res.append((losses, model._store.flat.detach().clone()))
    assert all(np.isfinite(res[0][0])) and res[0][0] == res[1][0] and torch.equal(res[0][1], res[1][1])


def _trainer_setup(S=208, Lt=10, D=64, N=2, h=4, B=24):
    from segmminterest_amd.trainer import default_args
    margs = default_args(num_layers_enc=N, d_model=D, nhead=h, input_type={"user": "image", "photo": "image"}, exposure_prob=[0.9] * S,
                         attn_stream=1)
    batches = [{k: v.to(DEV) for k, v in make_batch(B, S, Lt, D, n_users=50, n_items=500, seed=300 + i).items()} for i in range(3)]
    return margs, batches


def test_recorded_steps_equal_eager_steps_s208():
    """test_long_rows_gpu.test_recorded_steps_equal_eager_steps_s96 at S = 208, Lt = 10 (224 padded keys), built through
    default_args(attn_stream=1): record / run_recorded leave the parameters and losses of the eager steps, bitwise."""
    from segmminterest_amd.trainer import Trainer, init_model
    S, Lt, D = 208, 10, 64
    margs, batches = _trainer_setup(S, Lt, D)

    def run(recorded):
        torch.manual_seed(7)
        model = init_model(margs, n_users=50, n_items=500, input_dim=D, max_vid_len=S, max_usr_len=Lt).to(DEV)
        tr = Trainer(model, lr=1e-3, weight_decay=1e-4, device_state=True)
        if recorded:
            tr.record(batches[0], warmup=3)
        else:
            for _ in range(4):
                tr.train_step(batches[0])
        losses = []
        for t in range(6):
            out = tr.run_recorded(batches[t % 3]) if recorded else tr.train_step(batches[t % 3])
            losses.append(float(out["loss"].detach()))
        torch.cuda.synchronize()
        return model._store.flat.detach().clone(), losses

    pe, le = run(False)
    pr, lr_ = run(True)
    assert torch.isfinite(pe).all() and all(np.isfinite(le)) and le == lr_ and len(set(le)) > 1
    assert torch.equal(pe, pr)


def test_valid_model_matches_host_metrics_s208():
    """Trainer.valid_model (device ranks) == the reference's host loop at S = 208, as test_long_rows_gpu's S = 96 case."""
    from segmminterest_amd import my_evaluation as E
    from segmminterest_amd.trainer import Trainer, init_model
    S, Lt, D = 208, 10, 64
    margs, batches = _trainer_setup(S, Lt, D, B=48)
    torch.manual_seed(3)
    model = init_model(margs, n_users=50, n_items=500, input_dim=D, max_vid_len=S, max_usr_len=Lt).to(DEV)
    tr = Trainer(model)
    np.random.seed(7)
    got = tr.valid_model(batches, permutation=1)
    np.random.seed(7)
    acc = {}
    for b in batches:
        out = tr.eval_step(b, mode="train")
        interests = torch.sigmoid(out["logits"]) * torch.tensor(model.exposure_prob, device=DEV)
        gt = out["gt"]
        ev = E.TOP_K_leave(interests.cpu().numpy(), (gt == 1).sum(1, keepdim=True).cpu().numpy(), (gt != -2).cpu().numpy(), permutation=1)
        for k, v in ev.items():
            acc.setdefault(k, []).append(float(v))
        acc.setdefault("valid_loss", []).append(float(out["loss"]))
    assert np.isfinite(acc["valid_loss"]).all()
    for k, v in acc.items():
        assert got[k] == sum(v) / len(v), k
