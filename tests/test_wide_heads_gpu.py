"""Wide attention heads (dh = 96, 128) on the MI355X: the direct and streamed forward, the D kernels, the dQ / dK-dV pair and the
wide fused backward (csrc/attention_wide.h) against the float64 restatement of test_ops_gpu, under its bounds (2e-5 forward, 5e-5
gradients: the scaled logits have the same spread at any width); plane outputs by the rule of test_planes_gpu; whole models, the
trainer and recorded steps against the CPU oracle as test_long_rows_gpu does.  H = 2 throughout the kernel cases, so that the
second head starts at a non-zero column.  Run with ``pytest -m gpu``.

The kernel-level bounds here are COARSE end-to-end checks: fixed absolute tolerances on one seed per shape, several hundred fp32
ulps of a typical output; they do not look at lse, Dvec, amax_o or the words around an output.  The kernels are pinned to the
float64 statement, per element and under derived bounds, by tests/test_attn_wide_stream_float64_gpu.py (tests/attn_ref.py); what
this module adds to that is the model-level and recorded-step cases."""
import os
import sys

import numpy as np
import pytest
import torch

from helpers import LOSS_SLOTS, ROOT, build_model, call_model, loss_check, oracle_loss
from test_long_rows_gpu import _long_model_case, _oracle_model
from test_model_gpu import _check_live_grads
from test_ops_gpu import _attn_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"

sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import p32_ref as P32      # noqa: E402
from segmminterest_amd.synth import l1_normalize, make_batch      # noqa: E402

WIDE = (96, 128)
H_ = 2


def _abi():
    from segmminterest_amd import hipabi
    hipabi.lib()
    return hipabi


_CASES = {}


def _case(B, dh, Lq, La, Lb, p=0.0):
    """Inputs (the distribution and masks of test_ops_gpu.test_attention_fwd_bwd: one masked query, padded rows) and the float64
    output and gradients, computed once per shape and left unchanged."""
    key = (B, dh, Lq, La, Lb, p)
    if key in _CASES:
        return _CASES[key]
    H = _abi()
    d = H_ * dh
    g = torch.Generator().manual_seed(B * 1000 + Lq + dh)
    mk = lambda L: (torch.randn(B, L, d, generator=g) * 0.7).to(DEV)
    t = [mk(Lq), mk(Lq), mk(max(La, 1)), mk(max(La, 1)), mk(max(Lb, 1)), mk(max(Lb, 1))]
    mq = (torch.rand(B, Lq, generator=g) < 0.8).to(DEV)
    mka = (torch.rand(B, max(La, 1), generator=g) < 0.8).to(DEV)
    mkb = (torch.rand(B, max(Lb, 1), generator=g) < 0.7).to(DEV)
    mq[0, 0] = False
    mq[-1, -1] = True
    dO = torch.randn(B * Lq, d, generator=g).to(DEV)
    mult = None
    if p > 0:
        La_p, Lb_p = (La + 15) // 16 * 16, (Lb + 15) // 16 * 16
        Tp = La_p + Lb_p
        m = torch.empty(B * H_ * Lq * Tp, device=DEV)
        H.dropout_mult(m, m.numel(), p, 11, 3)
        m = m.view(B, H_, Lq, Tp)
        mult = torch.cat([m[..., :La], m[..., La_p:La_p + Lb]], -1).double()
    leaves = [x.double().requires_grad_(True) for x in t]
    sl = lambda x, L: x[:, :L]
    ref = _attn_ref(leaves[0], leaves[1], sl(leaves[2], La), sl(leaves[3], La), sl(leaves[4], Lb), sl(leaves[5], Lb),
                    mq, mka[:, :La], mkb[:, :Lb], H_, mult=mult)
    ref.backward(dO.view(B, Lq, d).double())
    grads = [leaf.grad for leaf in leaves]
    _CASES[key] = (t, (mq, mka, mkb), dO, ref.detach(), grads)
    return _CASES[key]


def _run(H, B, dh, Lq, La, Lb, phases, p=0.0, po=None, planes=None):
    """forward + backward (the phases in order) on the shared inputs; an empty key block is handed as None / length 0."""
    d = H_ * dh
    t, (mq, mka, mkb), dO, _, _ = _case(B, dh, Lq, La, Lb, p)
    z = lambda x, on=True: (x, 0) if on else None
    args = (B, H_, dh, Lq, La, Lb, z(t[0], La > 0), z(t[1], Lb > 0), d, z(t[2], La > 0), z(t[3], La > 0), d if La else 0,
            z(t[4], Lb > 0), z(t[5], Lb > 0), d if Lb else 0, mq, mka if La else None, mkb if Lb else None)
    O = torch.full((B * Lq, d), float("nan"), device=DEV)
    lse = torch.full((2, B, H_, Lq), float("nan"), device=DEV)
    kw = dict(drop_p=p, seed=11, site=3)
    H.attn_fwd(*args, O, d, lse, po=po, **kw)
    Dv = torch.empty(B, H_, Lq, device=DEV)
    outs = [torch.full_like(x, float("nan")) for x in t]
    for ph in phases:
        H.attn_bwd(*args, lse, O, d, dO, d, Dv, z(outs[0], La > 0), z(outs[1], Lb > 0), d, z(outs[2], La > 0), z(outs[3], La > 0),
                   d if La else 0, z(outs[4], Lb > 0), z(outs[5], Lb > 0), d if Lb else 0, phase=ph, planes=planes, **kw)
    torch.cuda.synchronize()
    return O, lse, outs


def _check(B, dh, Lq, La, Lb, O, outs, p=0.0):
    d = H_ * dh
    _, _, _, ref, grads = _case(B, dh, Lq, La, Lb, p)
    err = (O.view(B, Lq, d).double() - ref).abs().max().item()
    print("dh=%d (%d,%d,%d,%d) p=%g O err %.3e" % (dh, B, Lq, La, Lb, p, err))
    assert err < 2e-5, err
    live = (La > 0, Lb > 0, La > 0, La > 0, Lb > 0, Lb > 0)
    lens = (Lq, Lq, La, La, Lb, Lb)
    for name, got, want, on, L in zip(("dQa", "dQb", "dKa", "dVa", "dKb", "dVb"), outs, grads, live, lens):
        if on:
            e = (got[:, :L].double() - want[:, :L]).abs().max().item()
            print("    %s err %.3e" % (name, e))
            assert e < 5e-5, (name, e)


# (B, Lq, La, Lb): 3 query tiles, 3 + 7 key tiles | short heads and the merged form | several query chunks | one empty key block |
# 12 key tiles (11 in one block: two passes of the wide fused kernel)
SHAPES = [(2, 40, 40, 100), (2, 7, 40, 7), (2, 1, 40, 1), (1, 100, 40, 100), (2, 40, 0, 100), (2, 40, 40, 0), (1, 176, 176, 16)]


@pytest.mark.parametrize("phase", [0, 4])
@pytest.mark.parametrize("B,Lq,La,Lb", SHAPES)
@pytest.mark.parametrize("dh", WIDE)
def test_wide_attention_vs_float64(dh, B, Lq, La, Lb, phase):
    H = _abi()
    O, _, outs = _run(H, B, dh, Lq, La, Lb, (phase,))
    _check(B, dh, Lq, La, Lb, O, outs)


@pytest.mark.parametrize("B,Lq,La,Lb", [(2, 40, 40, 100), (1, 176, 176, 16)])
@pytest.mark.parametrize("dh", WIDE)
def test_wide_phases_5_and_6_are_bitwise_phase_4(dh, B, Lq, La, Lb):
    H = _abi()
    _, _, whole = _run(H, B, dh, Lq, La, Lb, (4,))
    _, _, parts = _run(H, B, dh, Lq, La, Lb, (5, 6))
    for a, b in zip(whole, parts):
        assert torch.equal(a, b)


@pytest.mark.parametrize("phase", [0, 4])
@pytest.mark.parametrize("dh", WIDE)
def test_wide_attention_dropout(dh, phase):
    """p = 0.1 against the restatement with the library's own mask (dropout_mult), both backward forms."""
    H = _abi()
    B, Lq, La, Lb = 2, 40, 40, 10
    O, _, outs = _run(H, B, dh, Lq, La, Lb, (phase,), p=0.1)
    _check(B, dh, Lq, La, Lb, O, outs, p=0.1)


@pytest.mark.parametrize("dh", WIDE)
def test_wide_streamed_kernels_under_the_knob(dh):
    H = _abi()
    B, Lq, La, Lb = 2, 40, 40, 100
    prev = H.config_set("ATT_STREAM", 1)
    try:
        O, _, outs = _run(H, B, dh, Lq, La, Lb, (0,))
    finally:
        H.config_set("ATT_STREAM", prev)
    _check(B, dh, Lq, La, Lb, O, outs)


@pytest.mark.parametrize("B,Lq,La,Lb", [(1, 17, 200, 9), (1, 200, 200, 100)])
@pytest.mark.parametrize("dh", WIDE)
def test_wide_streamed_kernels_above_192_keys(dh, B, Lq, La, Lb):
    H = _abi()
    O, _, outs = _run(H, B, dh, Lq, La, Lb, (0,))
    _check(B, dh, Lq, La, Lb, O, outs)


def test_wide_attention_is_reproducible():
    H = _abi()
    a = _run(H, 2, 128, 40, 40, 100, (4,))
    b = _run(H, 2, 128, 40, 40, 100, (4,))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for x, y in zip(a[2], b[2]):
        assert torch.equal(x, y)


# ------------------------------------------------------------------ plane outputs (test_planes_gpu's rule)
def _ref_planes(H, x, rows, cols, scale):
    """planes of x made by the stand-alone split pass with a given scale, itself held to the host statement of the format"""
    hdr = H.new_site(x.device)[0]
    hdr[0] = scale
    pl = torch.empty((rows, 2 * cols), dtype=torch.float16, device=x.device)
    H.split_p32(x, rows, cols, cols, pl, 2 * cols, hdr, mode=1)
    want, _ = P32.pack(x.detach().cpu().numpy().reshape(rows, cols), scale)
    got = pl.cpu().view(torch.int16).numpy().view(want.dtype).reshape(-1)
    assert (got == want).all()
    return pl


def _po(H, rows, cols, scale):
    hdr = H.new_site(DEV)[0]
    sc = torch.tensor([scale], dtype=torch.float32, device=DEV)
    pl = torch.zeros((rows, 2 * cols), dtype=torch.float16, device=DEV)
    return pl, hdr, sc, H.PO(pl, 2 * cols, hdr, sc.data_ptr())


@pytest.mark.parametrize("Hh,dh,B", [(2, 96, 3), (1, 128, 3), (2, 128, 3)])
def test_wide_attention_producers_write_the_split_pass_planes(Hh, dh, B):
    H = _abi()
    S, Lt = 40, 23
    d = Hh * dh
    rnd = lambda *shape, seed: torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(DEV)
    Yv, Yu = rnd(B * S, 4 * d, seed=30), rnd(B * Lt, 2 * d, seed=31)
    vm = (torch.rand(B, S, generator=torch.Generator().manual_seed(1)) > 0.2).to(torch.uint8).to(DEV)
    um = (torch.rand(B, Lt, generator=torch.Generator().manual_seed(2)) > 0.2).to(torch.uint8).to(DEV)
    O, lse = torch.empty(B * S, d, device=DEV), torch.empty(2, B, Hh, S, device=DEV)
    args = (B, Hh, dh, S, S, Lt, (Yv, 0), (Yv, d), 4 * d, (Yv, 2 * d), (Yv, 3 * d), 4 * d, (Yu, 0), (Yu, d), 2 * d, vm, vm, um)
    pl, hdr, sc, po = _po(H, B * S, d, 2.0 ** 12)
    H.attn_fwd(*args, O, d, lse, drop_p=0.1, seed=3, site=2, po=po)
    assert torch.equal(pl, _ref_planes(H, O, B * S, d, 2.0 ** 12)) and float(hdr[0]) == 2.0 ** 12
    assert float(hdr[H.SITE_HDR:].max()) == float(O.abs().max())
    dO = rnd(B * S, d, seed=32)
    dYv, dYu = torch.zeros_like(Yv), torch.zeros_like(Yu)
    Dv = torch.empty(B * Hh * S, device=DEV)
    plv, hv, scv, _ = _po(H, B * S, 4 * d, 2.0 ** 9)
    plu, hu, scu, _ = _po(H, B * Lt, 2 * d, 2.0 ** 8)
    pln = H.AttnPlanes()
    base_v, base_u = plv.data_ptr(), plu.data_ptr()
    pln.dqa, pln.dqb, pln.lddq2 = base_v, base_v + 4 * d, 8 * d
    pln.dka, pln.dva, pln.lddka2 = base_v + 8 * d, base_v + 12 * d, 8 * d
    pln.dkb, pln.dvb, pln.lddkb2 = base_u, base_u + 4 * d, 4 * d
    pln.hdr_q = pln.hdr_ka = hv.data_ptr()
    pln.hdr_kb = hu.data_ptr()
    pln.sin_q = pln.sin_ka = scv.data_ptr()
    pln.sin_kb = scu.data_ptr()
    H.attn_bwd(*args, lse, O, d, dO, d, Dv, (dYv, 0), (dYv, d), 4 * d, (dYv, 2 * d), (dYv, 3 * d), 4 * d, (dYu, 0), (dYu, d), 2 * d,
               drop_p=0.1, seed=3, site=2, phase=4, planes=pln)
    assert torch.equal(plv, _ref_planes(H, dYv, B * S, 4 * d, 2.0 ** 9)) and torch.equal(plu, _ref_planes(H, dYu, B * Lt, 2 * d, 2.0 ** 8))
    assert float(hv[0]) == 2.0 ** 9 and float(hu[0]) == 2.0 ** 8 and float(hv[1]) == 0.0 and float(hu[1]) == 0.0
    assert float(hv[H.SITE_HDR:].max()) == float(dYv.abs().max()) and float(hu[H.SITE_HDR:].max()) == float(dYu.abs().max())


# ------------------------------------------------------------------ whole models against the CPU oracle
def _opt_in(model):
    from segmminterest_amd.encoder import SegFormerX
    for m in model.modules():
        if isinstance(m, SegFormerX):
            m.attn_stream = 1
    return model


@pytest.mark.parametrize("kind,S,Lt,d,h,N,stream", [("image", 20, 10, 192, 2, 3, 0), ("id", 20, 1, 256, 2, 2, 0), ("image", 208, 10, 192, 2, 2, 1)])
def test_wide_model_vs_oracle(kind, S, Lt, d, h, N, stream):
    """test_long_rows_gpu.test_long_video_model_vs_oracle at dh = 96 and 128: logits within 1e-4 of the float64 and the float32
    oracle, every loss by loss_check, every live gradient by _check_live_grads, the same dead parameters."""
    cfg, model, inp = _long_model_case(kind, S, Lt, d, h, N)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    ref, rgrads = _oracle_model(sd, cfg, inp, torch.float32)
    t64, _ = _oracle_model(sd, cfg, inp, torch.float64)
    if stream:
        _opt_in(model)
    model = model.cuda().eval()
    out = call_model(model, inp, "train", DEV)
    err = (out["logits"].cpu().double() - t64["logits"].detach()).abs().max().item()
    print("wide model %s logits err vs float64 %.3e" % ((kind, S, Lt, d, h, N), err))
    assert err < 1e-4
    assert (out["logits"].cpu() - ref["logits"].detach()).abs().max().item() < 1e-4
    sc = oracle_loss(t64["logits"].detach(), inp["gt"], dict(cfg, learnable_bias=0))
    for i, name in enumerate(LOSS_SLOTS):
        if name in cfg["loss_type_list"] or name in ("mse", "mse2"):
            loss_check(float(out[name]), float(t64[name].detach()), float(ref[name].detach()), sc["slot_scales"][i], "model:" + name,
                       "%s d=%d" % (kind, d))
    loss_check(float(out["loss"].detach()), float(t64["loss"].detach()), float(ref["loss"].detach()), sc["total_scale"], "model:total",
               "%s d=%d" % (kind, d))
    out["loss"].backward()
    _check_live_grads(model, rgrads)


def test_wide_trainer_steps_vs_oracle_and_recorded(monkeypatch):
    """Image mode, d = 192, h = 2: three eager train_steps against segmm_oracle.train_steps under the 2e-4 relative rule of
    test_model_gpu; three recorded steps leave bitwise the losses and parameters of three eager ones."""
    import segmm_oracle as O
    from segmminterest_amd import engine as E
    from segmminterest_amd.trainer import Trainer
    monkeypatch.setattr(E, "MLP_INNER_DROPOUT", 0.0)
    B, S, Lt, D, N, h = 6, 20, 10, 192, 2, 2
    cfg = dict(N=N, h=h, S=S, d=D, D_in=D, Lt=Lt, user="image", photo="image", loss_type_list=["interestBPR"],
               loss_weight={"interestBPR": 1.0, "mse": 1.0}, exposure_prob=[1.0] * S)
    b = make_batch(B, S, Lt, D, seed=9)
    inp = dict(usr_image=l1_normalize(b["user"]), usr_id=b["user_identity_id"], usr_mask=b["user_mask"],
               vid_image=l1_normalize(b["photo"]), vid_id=b["photo_identity_id"], vid_mask=b["photo_mask"], gt=b["label"])
    batch = dict(user=inp["usr_image"].to(DEV), photo=inp["vid_image"].to(DEV), user_mask=inp["usr_mask"].to(DEV),
                 photo_mask=inp["vid_mask"].to(DEV), label=inp["gt"].to(DEV), user_identity_id=inp["usr_id"].to(DEV),
                 photo_identity_id=inp["vid_id"].to(DEV))

    def fresh(**kw):
        torch.manual_seed(5)
        model = build_model(cfg)
        for m in model.modules():          # train mode (delayed scales, planes from the producers) without the dropout draws
            for a in ("dropout_p", "inner_dropout"):
                if isinstance(getattr(m, a, None), float):
                    setattr(m, a, 0.0)
        sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
        tr = Trainer(model.cuda(), **kw)
        tr.normalize = lambda key, x, *a, **k: x             # already L1-normalised
        return model, sd, tr

    model, sd, tr = fresh()
    ref_losses = O.train_steps(sd, cfg, inp, 3, skip_dead=True)[1]
    got = [float(tr.train_step(batch)["loss"].detach()) for _ in range(3)]
    assert model.training
    for s, (a, r) in enumerate(zip(got, ref_losses)):
        assert abs(a - r) <= 2e-4 * max(1.0, abs(r)), (s, got, ref_losses)

    def run(recorded):
        model, _, tr = fresh(device_state=True)
        if recorded:
            tr.record(batch, warmup=3)
        else:
            for _ in range(4):
                tr.train_step(batch)
        losses = [float((tr.run_recorded(batch) if recorded else tr.train_step(batch))["loss"].detach()) for _ in range(3)]
        torch.cuda.synchronize()
        return model._store.flat.detach().clone(), losses

    pe, le = run(False)
    pr, lr_ = run(True)
    assert torch.isfinite(pe).all() and all(np.isfinite(le)) and le == lr_
    assert torch.equal(pe, pr)
