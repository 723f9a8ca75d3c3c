"""Spatial-reduction attention (sr_ratio > 1) on the MI355X: the two window kernels against their numpy statements bit for bit, the
reference fixtures of tests/golden/sr with the criteria of test_ffn_width_gpu.py, one synthetic model against ``sr_ref`` in float64
(eval mode, and train mode on delayed scales with the device's exported dropout masks), the moved 192-key limit, and recorded steps
against eager ones.  Run with ``pytest -m gpu``."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sr_ref as R      # noqa: E402
from helpers import call_model, note_grad_err      # noqa: E402
from sr_cases import SR_EVAL_CASES, build_sr_model, load_sr_case, sr_args      # noqa: E402
from test_ffn_width_gpu import _MaskFeed, _check_live_grads      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _abi():
    from segmminterest_amd import hipabi
    hipabi.lib()
    return hipabi


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ 1. the kernels, bit for bit
# (40, 2) / (41, 2): p = 0, S = 41 leaves token 40 in no window; (40, 4) / (41, 4): p = 1, (40, 8) / (8, 8): p = 3 -- the left zero pad,
# Ls = 1 at (8, 8) and (2, 2); d = 4: one lane per window, 48: no plane width at r = 2 .. (96 is), 32: the fixtures'.  The last four: the
# remaining template instances.
GRID = [(S, r, d) for (S, r) in [(40, 2), (41, 2), (40, 4), (41, 4), (40, 8), (8, 8), (2, 2)] for d in (4, 32, 48)] + \
       [(9, 3, 32), (15, 5, 32), (12, 6, 32), (14, 7, 32)]


@pytest.mark.parametrize("S,r,d", GRID)
def test_pack_unpack_and_mask_pool_bit_for_bit(S, r, d):
    H = _abi()
    B, ldx = 3, d + 8
    Ls = H.sr_len(S, r)
    assert Ls == R.sr_len(S, r)
    g = torch.Generator().manual_seed(S * 100 + r * 10 + d)
    xb = torch.randn(B * S, ldx, generator=g)
    xb[5 % (B * S), 1] = -37.5          # the maximum, negative, in a covered or uncovered row alike
    m = torch.rand(B, S, generator=g) < 0.35          # partial windows
    m[0] = False          # empty windows
    m[1] = True           # full windows
    x_dev, m_dev = xb.to(DEV), m.to(DEV)
    A = torch.full((B * Ls, r * d), 7.0, device=DEV)
    msr = torch.full((B, Ls), 9, dtype=torch.uint8, device=DEV)
    hdr = H.new_site(DEV)[0]
    H.sr_pack(x_dev, ldx, m_dev.view(torch.uint8), A, msr, hdr[H.SITE_HDR:], B, S, d, r)
    x_np = xb[:, :d].reshape(B, S, d).numpy()
    want = R.pack_np(x_np, r)
    assert np.array_equal(_bits(A).numpy(), want.view(np.int32))
    assert np.array_equal(msr.cpu().numpy(), R.mask_pool_np(m.numpy(), r).astype(np.uint8))
    assert float(hdr[H.SITE_HDR:].max()) == float(np.abs(want).max()) and float(hdr[0]) == 0.0 and float(hdr[1]) == 0.0
    # without a mask and without maxima: the same windows
    A2 = torch.full_like(A, 7.0)
    H.sr_pack(x_dev, ldx, None, A2, None, None, B, S, d, r)
    assert torch.equal(_bits(A2), _bits(A))
    # unpack: res given and null
    dA = torch.randn(B * Ls, r * d, generator=g)
    res = torch.randn(B * S, d, generator=g)
    for rs in (res, None):
        G = torch.full((B * S, d), 7.0, device=DEV)
        H.sr_unpack(dA.to(DEV), None if rs is None else rs.to(DEV), G, B, S, d, r)
        wantG = R.unpack_np(dA.numpy(), None if rs is None else rs.reshape(B, S, d).numpy(), B, S, d, r)
        assert np.array_equal(_bits(G).numpy().reshape(-1), wantG.view(np.int32).reshape(-1)), "res given" if rs is not None else "res null"


def test_pack_more_than_one_block_and_the_plane_split_of_its_output():
    """B Ls d / 4 = 16 x 20 x 24 = 7680 lanes = 30 blocks; the engine makes the planes of the packed windows with the split pass under
    the header the pack filled: they are the host P32 split of the kernel's output."""
    import p32_ref as P32
    H = _abi()
    B, S, d, r = 16, 40, 96, 2
    Ls = S // r
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B * S, d, generator=g)
    A = torch.empty((B * Ls, r * d), device=DEV)
    hdr = H.new_site(DEV)[0]
    H.sr_pack(x.to(DEV), d, None, A, None, hdr[H.SITE_HDR:], B, S, d, r)
    want = R.pack_np(x.reshape(B, S, d).numpy(), r)
    assert np.array_equal(_bits(A).numpy(), want.view(np.int32))
    assert float(hdr[H.SITE_HDR:].max()) == float(np.abs(want).max())
    pl = torch.empty((B * Ls, 2 * r * d), dtype=torch.float16, device=DEV)
    H.split_p32(A, B * Ls, r * d, r * d, pl, 2 * r * d, hdr, mode=0)
    scale = float(hdr[0])
    assert scale > 0 and float(hdr[1]) == 0.0
    ref_pl, _ = P32.pack(want, scale)
    got = pl.cpu().view(torch.int16).numpy().view(ref_pl.dtype).reshape(-1)
    assert (got == ref_pl).all()


# ------------------------------------------------------------------------------------------------ 2. the reference fixtures
def _loaded(name):
    cfg, g, nograd, extra = load_sr_case(name)
    model = build_sr_model(cfg)
    model.load_state_dict(g["sd"])
    return cfg, g, nograd, extra, model.cuda().eval()


@pytest.mark.parametrize("name", SR_EVAL_CASES)
def test_forward_loss_backward_vs_reference_golden(name):
    cfg, g, nograd, _, model = _loaded(name)
    out = call_model(model, g["in"], "train", DEV)
    err = (out["logits"].cpu() - g["out"]["logits"]).abs().max().item()
    print("%s: logits err %.3e" % (name, err))
    assert err < 1e-4, ("logits", err)
    for k, ref in g["out"].items():
        if ref.dim() == 0:
            got = float(out[k])
            assert abs(got - float(ref)) <= 1e-4 * max(1.0, abs(float(ref))), (k, got, float(ref))
    assert torch.equal(out["gt"].cpu(), g["out"]["gt"])
    out["loss"].backward()
    params = dict(model.named_parameters())
    for k in nograd:
        assert params[k].grad is None, k
    worst = 0.0
    for k, ref in g["grad"].items():
        got = params[k].grad
        assert got is not None, k
        scale = max(float(ref.abs().max()), 1e-6)
        e = float((got.cpu() - ref).abs().max())
        note_grad_err(k, e, scale)
        worst = max(worst, e / (5e-5 * scale + 2e-6))
        assert e <= 5e-5 * scale + 2e-6, (k, e, scale)
    print("%s: worst gradient error / bound %.3f" % (name, worst))
    # bucket layout: every live tensor inside exactly one bucket of the flat gradient buffer, none overlapping; the conv rides there
    st = model._store
    spans = sorted((st.index[k][0], st.index[k][0] + st.index[k][1], k) for k in st.live_names)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    assert spans[-1][1] <= st.n_live == st.gflat.numel()
    for o, e_, k in spans:
        assert sum(1 for _, s0, e0 in st.buckets if s0 <= o and e_ <= e0) == 1, k
        assert tuple(st.g(k).shape) == tuple(g["sd"][k].shape), k
    live_sr = [k for k in st.live_names if k.endswith("cross_attn.sr.weight")]
    assert live_sr and all(k in g["grad"] for k in live_sr)
    if st.engine_p:          # the conv weight as the [d, r d] GEMM matrix, with its transpose
        mats = {n: (R_, C_, tr) for n, _, R_, C_, tr in st._wmats}
        for k in live_sr:
            d_, _, r_ = g["sd"][k].shape
            assert mats[k] == (d_, d_ * r_, True) and k in st.wpt and k in st.wTpt


@pytest.mark.parametrize("name", SR_EVAL_CASES)
def test_inference_logits(name):
    cfg, g, _, _, model = _loaded(name)
    with torch.no_grad():
        out = call_model(model, g["in"], "inference", DEV)
    assert (out["logits"].cpu() - g["inf"]["logits"]).abs().max().item() < 1e-4


@pytest.mark.parametrize("name", [n for n in SR_EVAL_CASES if load_sr_case(n)[1]["adam3"]])
def test_adamw_steps_torch_optimizer_dropin(name):
    """test_ffn_width_gpu.test_adamw_steps_torch_optimizer_dropin on the reduced fixtures."""
    cfg, g, nograd, extra, model = _loaded(name)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=1e-4)
    counts = {"all": 0, "loose": 0}

    def check(k, got, ref, base, steps):
        if k not in g["grad"]:
            assert torch.equal(got, ref), k
            return
        gabs = g["grad"][k].abs()
        solid = gabs > max(1e-5, 2e-3 * float(gabs.max()))
        err = (got - ref).abs()
        lim_solid = base + 1e-4 * ref.abs()
        lim = torch.where(solid, torch.full_like(err, base), torch.full_like(err, 2.2e-3 * steps)) + 1e-4 * ref.abs()
        counts["all"] += err.numel()
        counts["loose"] += int(((~solid) & (err > lim_solid)).sum())
        bad = err > lim
        if bool(bad.any()):
            i = int((err - lim).argmax())
            raise AssertionError("step %d %s: elem %d err %.3e lim %.3e |g_ref| %.3e gmax %.3e" % (
                steps, k, i, float(err.view(-1)[i]), float(lim.view(-1)[i]), float(gabs.view(-1)[i]), float(gabs.max())))
    for step in range(1, 4):
        opt.zero_grad()
        out = call_model(model, g["in"], "train", DEV)
        out["loss"].backward()
        opt.step()
        if step in (1, 3):
            ref = g["adam%d" % step]
            counts["all"] = counts["loose"] = 0
            for k, p in model.named_parameters():
                check(k, p.detach().cpu(), ref[k], 3e-5 * step, step)
            print("%s step %d: loose %d of %d" % (name, step, counts["loose"], counts["all"]))
            assert counts["loose"] <= 0.01 * counts["all"], (step, counts)
    for k, p in model.named_parameters():
        if k in nograd:
            assert torch.equal(p.detach().cpu(), g["sd"][k]), k


# ------------------------------------------------------------------------------------------------ 3. a synthetic model against sr_ref
def _synth(d, h, N, sr, S, Lt, Din, B, seed=0, scale_layers=2.0, scale_in=100.0, sr_attn=1):
    """test_ffn_width_gpu._synth with ``sr_ratio_lvls = sr`` and the key: a single-backbone image-mode model, one batch, the cfg."""
    import segmminterest_amd as M
    from segmminterest_amd.synth import l1_normalize, make_batch
    torch.manual_seed(seed)
    cfg = dict(N=N, h=h, d=d, S=S, Lt=Lt, user="image", photo="image", loss_type_list=["interestBPR"],
               loss_weight={"interestBPR": 1.0, "mse": 1.0}, exposure_prob=[1.0] * S, sr=list(sr))
    args = sr_args(cfg, sr_attn)
    bb = M.SegFormerX(d_model_in=d, d_model_lvls=[d] * N, num_head_lvls=[h] * N, ff_dim_lvls=[d] * N, input_vid_dim=Din, input_usr_dim=Din,
                      max_vid_len=S, max_usr_len=Lt, sr_ratio_lvls=list(sr), use_patch_merge=[False] * N, output_layers=[-1], model_cfg=args)
    model = M.MultiScaleTemporalDetrLeaveFocal(bb, None, None, torch.nn.Identity(), args)
    with torch.no_grad():
        for n_, p in model.named_parameters():
            if (p.dim() == 2 or n_.endswith("cross_attn.sr.weight")) and ".encoder.layers." in n_ and "ln_" not in n_:
                p.mul_(scale_layers)
            if n_.endswith("vid_proj.weight") or n_.endswith("usr_proj.weight"):
                p.mul_(scale_in)
            if n_.endswith("cross_attn.sr.bias"):
                p.normal_(0.0, 0.02)          # (make the conv's bias count)
    b = make_batch(B, S, Lt, Din, seed=11)
    inp = dict(usr_image=l1_normalize(b["user"]), usr_id=b["user_identity_id"], usr_mask=b["user_mask"],
               vid_image=l1_normalize(b["photo"]), vid_id=b["photo_identity_id"], vid_mask=b["photo_mask"], gt=b["label"])
    return model, inp, cfg


SYN = dict(d=64, h=4, N=3, sr=[4, 2, 1], S=96, Lt=10, Din=64, B=4)          # 96 -> 24 and 48 keys; pad16 + 16 user keys fit


def test_synthetic_reduced_model_vs_sr_ref_float64():
    """Eval mode against ``sr_ref`` in float64, with the eval-mode bounds of test_ffn_width_gpu.test_synthetic_widths_vs_oracle."""
    model, inp, cfg = _synth(**SYN)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    ref, rgrads = R.forward_backward(sd, cfg, inp, dtype=torch.float64)
    model = model.cuda().eval()
    out = call_model(model, inp, "train", DEV)
    e = (out["logits"].cpu().double() - ref["logits"].detach()).abs().max().item()
    print("synthetic eval: logits err %.3e" % e)
    assert e < 1e-4
    assert abs(float(out["loss"].detach()) - float(ref["loss"].detach())) < 1e-5 * max(1.0, abs(float(ref["loss"])))
    out["loss"].backward()
    _check_live_grads(model, {k: (None if v is None else v.float()) for k, v in rgrads.items()})
    assert model.backbone1.encoder.layers[0].cross_attn.sr.weight.grad is not None
    assert model.backbone1.encoder.layers[2].cross_attn.ff_vid.weight.grad is None


def test_synthetic_train_mode_delayed_scales_with_exported_masks():
    """test_ffn_width_gpu.test_train_mode_delayed_scales_with_exported_masks at the synthetic reduced shape: one calibration step,
    then the measured train-mode step on delayed plane scales against ``sr_ref`` fed the device's masks.  The logits masks of a
    reduced layer cover [B, h, Lq, pad16(Ls) + pad16(Lt)]."""
    from segmminterest_amd import engine as E
    model, inp, cfg = _synth(seed=1, **SYN)
    S, Lt = SYN["S"], SYN["Lt"]
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model = model.cuda().train()
    st = model._store
    if st.engine_p:
        assert st.scaling == "delayed"
    torch.manual_seed(100)
    call_model(model, inp, "train", DEV)["loss"].backward()
    for p in model.parameters():
        p.grad = None
    torch.manual_seed(7)
    seed = int(torch.randint(0, 2 ** 62, (1,)).item())          # what engine.next_seed() will draw
    torch.manual_seed(7)
    out = call_model(model, inp, "train", DEV)
    out["loss"].backward()
    if st.engine_p:
        assert len(st.calibrated) > 10 and "backbone1.L0.Xsr" in st.calibrated and "backbone1.dXsr1" in st.calibrated
    assert st.overflow_count() == 0, "a delayed scale left its window (the fallback would have run)"
    p = float(model.backbone1.dropout_p)
    pi = E.MLP_INNER_DROPOUT
    s = lambda layer, kind: E._site(0, layer, kind)
    L0, L1 = S // 4, S // 2
    # dropout call order of the live graph (sr_ref.cross_attention / encoder_layer): embedding video, user; layer 0 (full): video
    # logits, user logits, ff_usr, ff_vid, video MLP inner / outer, user MLP inner / outer; layer 1 (video side): logits, ff_vid, MLP
    plan = [(s(0, E.K_EMB_V), p, "tokens"), (s(0, E.K_EMB_U), p, "tokens"),
            (s(0, E.K_ATT_V), p, (L0, Lt)), (s(0, E.K_ATT_U), p, (L0, Lt)), (s(0, E.K_AO_U), p, "tokens"), (s(0, E.K_AO_V), p, "tokens"),
            (s(0, E.K_MI_V), pi, "tokens"), (s(0, E.K_MO_V), p, "tokens"), (s(0, E.K_MI_U), pi, "tokens"), (s(0, E.K_MO_U), p, "tokens"),
            (s(1, E.K_ATT_V), p, (L1, Lt)), (s(1, E.K_AO_V), p, "tokens"), (s(1, E.K_MI_V), pi, "tokens"), (s(1, E.K_MO_V), p, "tokens")]
    feed = _MaskFeed(seed, plan)
    ref, rgrads = R.forward_backward(sd, cfg, inp, drop=feed)
    assert feed.i == len(plan)
    ref_eval = R.model_forward(sd, cfg, inp, "inference")["logits"]
    assert (ref["logits"].detach() - ref_eval.detach()).abs().max().item() > 1e-2
    e = (out["logits"].cpu() - ref["logits"].detach()).abs().max().item()
    print("synthetic train: logits err %.3e" % e)
    assert e < 1e-4
    assert abs(float(out["loss"].detach()) - float(ref["loss"].detach())) < 1e-5 * max(1.0, abs(float(ref["loss"])))
    _check_live_grads(model, rgrads)


# ------------------------------------------------------------------------------------------------ 4. the moved 192-key limit
def test_S160_Lt100_runs_reduced_and_is_still_refused_unreduced():
    """S = 160, Lt = 100: 160 + 112 padded keys are refused as ever at [1, 1, 1]; with [4, 4, 1] every call has 48 + 112 and runs on
    the held kernels, without ``attn_stream`` -- checked against ``sr_ref`` with the fixtures' bounds."""
    kw = dict(d=32, h=4, N=3, S=160, Lt=100, Din=32, B=2)
    model, inp, cfg = _synth(sr=[4, 4, 1], **kw)
    assert not getattr(model.backbone1, "attn_stream", 0)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    ref, rgrads = R.forward_backward(sd, cfg, inp)
    model = model.cuda().eval()
    out = call_model(model, inp, "train", DEV)
    assert (out["logits"].cpu() - ref["logits"].detach()).abs().max().item() < 1e-4
    out["loss"].backward()
    _check_live_grads(model, rgrads)
    plain, inp1, _ = _synth(sr=[1, 1, 1], **kw)
    plain = plain.cuda().eval()
    with pytest.raises(RuntimeError, match=r"S=160 video segments and Lt=100 user tokens make 272 padded keys > 192 not built"):
        call_model(plain, inp1, "train", DEV)


# ------------------------------------------------------------------------------------------------ 5. the trainer
def _steps(recorded, sr, sr_attn, mixed_precision=None, n_warm=3):
    from segmminterest_amd.synth import make_batch
    from segmminterest_amd.trainer import FusedAdamW, Trainer, default_args, init_model
    B, S, D, N, h, Lt = 32, 40, 32, 3, 4, 10
    over = {} if sr_attn is None else dict(sr_attn=sr_attn)
    margs = default_args(num_layers_enc=N, d_model=D, nhead=h, input_type={"user": "image", "photo": "image"}, exposure_prob=[1.0] * S, **over)
    batches = [{k: v.to(DEV) for k, v in make_batch(B, S, Lt, D, seed=200 + i).items()} for i in range(3)]
    torch.manual_seed(5)
    model = init_model(margs, n_users=50, n_items=500, input_dim=D, max_vid_len=S, max_usr_len=Lt, sr_ratio=sr).to(DEV)
    tr = Trainer(model, lr=1e-3, weight_decay=1e-4, device_state=True, **({} if mixed_precision is None else dict(mixed_precision=mixed_precision)))
    assert isinstance(tr.opt, FusedAdamW)
    if recorded:
        tr.record(batches[0], warmup=n_warm - 1)
    else:
        for _ in range(n_warm):
            tr.train_step(batches[0])
    losses = []
    for t in range(3):
        out = tr.run_recorded(batches[t % 3]) if recorded else tr.train_step(batches[t % 3])
        losses.append(out["loss"].detach().clone())
    torch.cuda.synchronize()
    names = [n for n in model._store.live_names]
    return model._store.flat.detach().clone(), tr.opt.m.clone(), torch.stack(losses), names


@pytest.mark.parametrize("mp", [None, True], ids=["default", "mixed_precision"])
def test_recorded_steps_equal_eager_steps(mp):
    """d = 32, S = 40, N = 3, sr = [2, 4, 1]: record() then three run_recorded() steps on rotating batches leave bitwise the
    parameters, the FusedAdamW moments and the losses of the same steps taken by train_step -- the pack, the conv GEMM, the unpack
    and the pooled masks are C commands of the replay."""
    p_e, m_e, l_e, names = _steps(False, [2, 4, 1], 1, mp)
    p_r, m_r, l_r, _ = _steps(True, [2, 4, 1], 1, mp)
    assert any(n.endswith("layers.1.cross_attn.sr.weight") for n in names)
    assert bool(torch.isfinite(l_e).all()) and bool(torch.isfinite(p_e).all())
    assert torch.equal(l_e, l_r)
    assert torch.equal(p_e, p_r) and torch.equal(m_e, m_r)


def test_key_with_unit_ratios_takes_the_default_steps():
    """``model_cfg.sr_attn = 1`` with ``[1] * N`` changes nothing: the steps of the model built without the key, bit for bit."""
    p_k, m_k, l_k, n_k = _steps(False, None, 1)
    p_d, m_d, l_d, n_d = _steps(False, None, None)
    assert n_k == n_d
    assert torch.equal(l_k, l_d) and torch.equal(p_k, p_d) and torch.equal(m_k, m_d)
    p_1, m_1, l_1, _ = _steps(False, [1, 1, 1], 1)
    assert torch.equal(l_1, l_d) and torch.equal(p_1, p_d) and torch.equal(m_1, m_d)


def test_eval_mode_is_bitwise_reproducible():
    model, inp, cfg = _synth(32, 4, 3, [2, 4, 1], 40, 10, 48, 8)
    model = model.cuda().eval()
    a = call_model(model, inp, "train", DEV)
    a["loss"].backward()
    ga = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    assert "backbone1.encoder.layers.1.cross_attn.sr.weight" in ga
    model.zero_grad()
    b = call_model(model, inp, "train", DEV)
    b["loss"].backward()
    assert torch.equal(a["logits"], b["logits"]) and torch.equal(a["loss"], b["loss"])
    for k, p in model.named_parameters():
        if p.grad is not None:
            assert torch.equal(p.grad, ga[k]), k
