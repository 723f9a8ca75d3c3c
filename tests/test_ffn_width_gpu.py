"""Encoder layers whose feed-forward width differs from d_model, on the MI355X: the reference fixtures of tests/golden/ffn with
the criteria of test_model_gpu.py, full width against the CPU oracle (eval mode, and train mode on delayed scales with the device's
exported dropout masks), recorded steps against eager ones, and the plane GEMMs / the weight split at rectangular FFN shapes
against float64.  Run with ``pytest -m gpu``."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ffn_cases import FF_EVAL_CASES, build_ff_model, ff_args, load_ff_case      # noqa: E402
from helpers import ROOT, call_model, note_grad_err      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"

sys.path.insert(0, os.path.join(ROOT, "oracle"))


def _abi():
    from segmminterest_amd import hipabi
    hipabi.lib()
    return hipabi


def _loaded(name):
    cfg, g, nograd, extra = load_ff_case(name)
    model = build_ff_model(cfg)
    model.load_state_dict(g["sd"])
    return cfg, g, nograd, extra, model.cuda().eval()


# ------------------------------------------------------------------------------------------------ 1. the reference fixtures
@pytest.mark.parametrize("name", FF_EVAL_CASES)
def test_forward_loss_backward_vs_reference_golden(name):
    cfg, g, nograd, _, model = _loaded(name)
    out = call_model(model, g["in"], "train", DEV)
    err = (out["logits"].cpu() - g["out"]["logits"]).abs().max().item()
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
    for k, ref in g["grad"].items():
        got = params[k].grad
        assert got is not None, k
        scale = max(float(ref.abs().max()), 1e-6)
        e = float((got.cpu() - ref).abs().max())
        note_grad_err(k, e, scale)
        assert e <= 5e-5 * scale + 2e-6, (k, e, scale)
    # the data-parallel bucket layout comes from the parameters' sizes: every live tensor lies inside exactly one bucket of the flat
    # gradient buffer, no two overlap, and the feed-forward matrices have the fixture's shapes there
    st = model._store
    spans = sorted((st.index[k][0], st.index[k][0] + st.index[k][1], k) for k in st.live_names)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    assert spans[-1][1] <= st.n_live == st.gflat.numel()
    for o, e_, k in spans:
        assert sum(1 for _, s0, e0 in st.buckets if s0 <= o and e_ <= e0) == 1, k
        assert tuple(st.g(k).shape) == tuple(g["sd"][k].shape), k


@pytest.mark.parametrize("name", FF_EVAL_CASES)
def test_inference_logits(name):
    cfg, g, _, _, model = _loaded(name)
    with torch.no_grad():
        out = call_model(model, g["in"], "inference", DEV)
    assert (out["logits"].cpu() - g["inf"]["logits"]).abs().max().item() < 1e-4


@pytest.mark.parametrize("name", [n for n in FF_EVAL_CASES if load_ff_case(n)[1]["adam3"]])
def test_adamw_steps_torch_optimizer_dropin(name):
    """test_model_gpu.test_adamw_steps_torch_optimizer_dropin on the ff != d fixtures."""
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
            assert counts["loose"] <= 0.01 * counts["all"], (step, counts)
    for k, p in model.named_parameters():
        if k in nograd:
            assert torch.equal(p.detach().cpu(), g["sd"][k]), k


# ------------------------------------------------------------------------------------------------ synthetic models against the oracle
def _synth(d, h, N, ff, S, Lt, Din, B, seed=0, scale_layers=2.0, scale_in=100.0):
    """A single-backbone image-mode model with ``ff_dim_lvls = ff`` (weights scaled as test_model_gpu._cfg2_model scales them:
    attention and LayerNorm non-trivial), one batch, and the oracle's cfg."""
    import segmminterest_amd as M
    from segmminterest_amd.synth import l1_normalize, make_batch
    torch.manual_seed(seed)
    cfg = dict(N=N, h=h, d=d, S=S, Lt=Lt, user="image", photo="image", loss_type_list=["interestBPR"],
               loss_weight={"interestBPR": 1.0, "mse": 1.0}, exposure_prob=[1.0] * S)
    args = ff_args(cfg)
    bb = M.SegFormerX(d_model_in=d, d_model_lvls=[d] * N, num_head_lvls=[h] * N, ff_dim_lvls=ff, input_vid_dim=Din, input_usr_dim=Din,
                      max_vid_len=S, max_usr_len=Lt, sr_ratio_lvls=[1] * N, use_patch_merge=[False] * N, output_layers=[-1], model_cfg=args)
    model = M.MultiScaleTemporalDetrLeaveFocal(bb, None, None, torch.nn.Identity(), args)
    with torch.no_grad():
        for n_, p in model.named_parameters():
            if p.dim() == 2 and ".encoder.layers." in n_ and "ln_" not in n_:
                p.mul_(scale_layers)
            if n_.endswith("vid_proj.weight") or n_.endswith("usr_proj.weight"):
                p.mul_(scale_in)
            if n_.endswith(".bias") and ".encoder.layers." in n_ and ".ff_" in n_:
                p.normal_(0.0, 0.02)          # (the reference zero-initialises biases: make the [ff] ones count)
    b = make_batch(B, S, Lt, Din, seed=11)
    inp = dict(usr_image=l1_normalize(b["user"]), usr_id=b["user_identity_id"], usr_mask=b["user_mask"],
               vid_image=l1_normalize(b["photo"]), vid_id=b["photo_identity_id"], vid_mask=b["photo_mask"], gt=b["label"])
    return model, inp, cfg


def _check_live_grads(model, rgrads):
    """test_model_gpu._check_live_grads: every live gradient within 5e-5 of its tensor's maximum plus 1e-6 of the model's largest."""
    gmax = max(float(r.abs().max()) for r in rgrads.values() if r is not None)
    bad = {}
    for k, p in model.named_parameters():
        if rgrads[k] is None:
            assert p.grad is None, k
            continue
        scale = float(rgrads[k].abs().max())
        e = float((p.grad.cpu() - rgrads[k]).abs().max())
        if scale > 1e-6 * gmax:
            note_grad_err(k, e, scale)
        if e > 5e-5 * scale + 1e-6 * gmax:
            bad[k] = (e, scale, gmax)
    assert not bad, bad


# (1056 = 33 x 32: no multiple of 64 / 128 / 256 -- ragged column tiles and k tails, the weight gradients on the round-2 TN kernel;
#  3072: both sides of the full layer 0 on gemm_pl_nt4 / gemm_pl_tn8.  [40, 36, 32] at d = 32: multiples of 4 that are no multiples of
#  32 -- the four GEMMs with ff as a dimension take the fp32-operand kernels, everything else of the model stays on the planes)
@pytest.mark.parametrize("d,h,ff,Lt,B", [(768, 16, [3072, 1056, 768], 100, 32), (32, 4, [40, 36, 32], 10, 8)], ids=["full_width", "not_mult_32"])
def test_synthetic_widths_vs_oracle(d, h, ff, Lt, B):
    import segmm_oracle as O
    S, N = 40, 3
    model, inp, cfg = _synth(d, h, N, ff, S, Lt, d, B)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    ref, rgrads = O.forward_backward(sd, cfg, inp)
    model = model.cuda().eval()
    out = call_model(model, inp, "train", DEV)
    assert (out["logits"].cpu() - ref["logits"].detach()).abs().max().item() < 1e-4
    assert abs(float(out["loss"].detach()) - float(ref["loss"].detach())) < 1e-5 * max(1.0, abs(float(ref["loss"])))
    out["loss"].backward()
    _check_live_grads(model, rgrads)
    st = model._store
    if st.engine_p:
        f0 = "backbone1.encoder.layers.0.ff_vid.layers.0.weight"
        assert ((f0 in st.wpt) and (f0 in st.wTpt)) is (ff[0] % 32 == 0)


class _MaskFeed:
    """test_model_gpu._MaskFeed (the oracle's ``drop`` hook fed the device's own masks, exported per site); records the element
    count of every token-shaped mask it exported."""

    def __init__(self, seed, plan):
        self.seed, self.plan, self.i, self.numel = seed, plan, 0, {}

    def __call__(self, t):
        from segmminterest_amd import hipabi as H
        site, p, kind = self.plan[self.i]
        self.i += 1
        if kind == "tokens":
            m = torch.empty(t.numel(), device=DEV)
            H.dropout_mult(m, m.numel(), p, self.seed, site)
            self.numel[site] = m.numel()
            return t * m.view(t.shape).cpu()
        B, h, Lq, T = t.shape
        La, Lb = kind
        assert La + Lb == T
        La_p, Lb_p = (La + 15) // 16 * 16, (Lb + 15) // 16 * 16
        m = torch.empty(B * h * Lq * (La_p + Lb_p), device=DEV)
        H.dropout_mult(m, m.numel(), p, self.seed, site)
        m = m.view(B, h, Lq, La_p + Lb_p)
        return t * torch.cat([m[..., :La], m[..., La_p:La_p + Lb]], -1).cpu()


def test_train_mode_delayed_scales_with_exported_masks():
    """test_model_gpu.test_full_size_train_mode_gradients_with_exported_masks at ff = 1536 (d = 768, h = 16, N = 2, S = 40, Lt = 100,
    B = 64): one calibration step, then the measured train-mode step on delayed plane scales against the oracle fed the device's
    masks.  The inner-dropout mask (K_MI_V) is exported over B * S * ff elements: its index is the flat index of the [M, ff] tensor."""
    import segmm_oracle as O
    from segmminterest_amd import engine as E
    B, S, Lt, ffw = 64, 40, 100, 1536
    model, inp, cfg = _synth(768, 16, 2, [ffw, 768], S, Lt, 768, B, seed=1)
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
        assert len(st.calibrated) > 10
    assert st.overflow_count() == 0, "a delayed scale left its window (the fallback would have run)"
    p = float(model.backbone1.dropout_p)
    s = lambda kind: E._site(0, 0, kind)
    plan = [(s(E.K_EMB_V), p, "tokens"), (s(E.K_EMB_U), p, "tokens"), (s(E.K_ATT_V), p, (S, Lt)), (s(E.K_AO_V), p, "tokens"),
            (s(E.K_MI_V), E.MLP_INNER_DROPOUT, "tokens"), (s(E.K_MO_V), p, "tokens")]
    feed = _MaskFeed(seed, plan)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    ref, rgrads = O.forward_backward(sd, cfg, inp, drop=feed)
    assert feed.i == len(plan)
    assert feed.numel[s(E.K_MI_V)] == B * S * ffw and feed.numel[s(E.K_MO_V)] == B * S * 768
    ref_eval = O.model_forward(sd, cfg, inp, "inference")["logits"]
    assert (ref["logits"].detach() - ref_eval.detach()).abs().max().item() > 1e-2
    assert (out["logits"].cpu() - ref["logits"].detach()).abs().max().item() < 1e-4
    assert abs(float(out["loss"].detach()) - float(ref["loss"].detach())) < 1e-5 * max(1.0, abs(float(ref["loss"])))
    _check_live_grads(model, rgrads)


# ------------------------------------------------------------------------------------------------ 4. the recorded step
@pytest.mark.parametrize("mode", ["image", "id"])
def test_recorded_steps_equal_eager_steps(mode):
    """d = 64, h = 4, N = 3, ff = [160, 32, 64]: record() then three run_recorded() steps on rotating batches leave bitwise the
    parameters, the FusedAdamW moments and the losses of the same steps taken by train_step (layer 0 is full: both sides, the user
    side on the side stream, at ff = 160; layer 1 runs its video side at ff = 32 < d)."""
    from segmminterest_amd.synth import make_batch
    from segmminterest_amd.trainer import FusedAdamW, Trainer, default_args, init_model
    B, S, D, N, h, ff = 32, 40, 64, 3, 4, [160, 32, 64]
    if mode == "image":
        Lt, Din, kw = 10, D, {}
        margs = default_args(num_layers_enc=N, d_model=D, nhead=h, input_type={"user": "image", "photo": "image"}, exposure_prob=[1.0] * S)
    else:
        Lt, Din, kw = 1, 4, dict(n_users=50, n_items=500)
        margs = default_args(num_layers_enc=N, d_model=D, nhead=h, input_type={"user": "id", "photo": "id"}, exposure_prob=[1.0] * S)
    batches = [{k: v.to(DEV) for k, v in make_batch(B, S, Lt, Din, seed=200 + i, **kw).items()} for i in range(3)]

    def run(recorded):
        torch.manual_seed(5)
        model = init_model(margs, n_users=50, n_items=500, input_dim=Din, max_vid_len=S, max_usr_len=Lt, ff_dim=ff).to(DEV)
        tr = Trainer(model, lr=1e-3, weight_decay=1e-4, device_state=True)
        assert isinstance(tr.opt, FusedAdamW)
        if recorded:
            tr.record(batches[0], warmup=2)
        else:
            for _ in range(3):
                tr.train_step(batches[0])
        losses = []
        for t in range(3):
            out = tr.run_recorded(batches[t % 3]) if recorded else tr.train_step(batches[t % 3])
            losses.append(out["loss"].detach().clone())
        torch.cuda.synchronize()
        shapes = [tuple(l.ff_vid.layers[0].weight.shape) for l in model.backbone1.encoder.layers]
        assert shapes == [(f, D) for f in ff]
        return model._store.flat.detach().clone(), tr.opt.m.clone(), torch.stack(losses)

    p_e, m_e, l_e = run(False)
    p_r, m_r, l_r = run(True)
    assert bool(torch.isfinite(l_e).all()) and bool(torch.isfinite(p_e).all())
    assert torch.equal(l_e, l_r)
    assert torch.equal(p_e, p_r) and torch.equal(m_e, m_r)


# ------------------------------------------------------------------------------------------------ 5. reproducibility
def test_eval_mode_is_bitwise_reproducible():
    model, inp, cfg = _synth(32, 4, 2, [96, 32], 40, 10, 48, 8)
    model = model.cuda().eval()
    a = call_model(model, inp, "train", DEV)
    a["loss"].backward()
    ga = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    assert "backbone1.encoder.layers.0.ff_vid.layers.0.weight" in ga
    model.zero_grad()
    b = call_model(model, inp, "train", DEV)
    b["loss"].backward()
    assert torch.equal(a["logits"], b["logits"]) and torch.equal(a["loss"], b["loss"])
    for k, p in model.named_parameters():
        if p.grad is not None:
            assert torch.equal(p.grad, ga[k]), k


# ------------------------------------------------------------------------------------------------ 6. kernels at rectangular FFN shapes
# (M, N, K) of the NT launches = (tokens, out, in); the weight gradient of the same Linear is the TN launch (N, K, tokens)
FFN_SHAPES = [(80, 96, 32), (80, 32, 96), (640, 1056, 768), (640, 768, 1056), (640, 1536, 768), (640, 768, 1536)]
E_SITE = 4096 + 32 + 7          # a dropout site id as the engine forms them (backbone 1, layer 1, K_MI_V)


@pytest.fixture(params=["default", "round6", "round3"])
def gemm_generation(request):
    """test_planes_gpu.gemm_generation: the library's own kernel choice, the round-6 kernels wherever they fit, the round-3 kernels."""
    if request.param == "default":
        yield request.param
        return
    H = _abi()
    pl, tn = (44, 4) if request.param == "round6" else (8, 88)
    prev = H.config_set("PL_VAR", pl), H.config_set("TN_VAR", tn)
    try:
        yield request.param
    finally:
        H.config_set("PL_VAR", prev[0])
        H.config_set("TN_VAR", prev[1])


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def _mean_rel(x, ref):
    return float((x.double() - ref).abs().mean() / ref.abs().mean())


def _gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / np.sqrt(2.0)))


def _dgelu64(x):
    return 0.5 * (1.0 + torch.erf(x / np.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / np.sqrt(2.0 * np.pi)


def _ref_planes(H, x, rows, cols, scale):
    """test_planes_gpu._ref_planes: the stand-alone split pass with a given scale, itself held to the host split of p32_ref."""
    import p32_ref as P32
    hdr = H.new_site(x.device)[0]
    hdr[0] = scale
    pl = torch.empty((rows, 2 * cols), dtype=torch.float16, device=x.device)
    H.split_p32(x, rows, cols, cols, pl, 2 * cols, hdr, mode=1)
    want, _ = P32.pack(x.detach().cpu().numpy().reshape(rows, cols), scale)
    got = pl.cpu().view(torch.int16).numpy().view(want.dtype).reshape(-1)
    assert (got == want).all(), "split_p32 departs from the host split in %d halves" % int((got != want).sum())
    return pl


@pytest.mark.parametrize("M,N,K", FFN_SHAPES)
def test_gemm_p_nt_gelu_aux_dropout_planes_at_ffn_shapes(gemm_generation, M, N, K):
    """The first FFN GEMM's launch: H = drop(gelu(X . W0^T + b0)), pre-activation to aux (ldaux = N), planes of H written by the
    epilogue with a given scale.  Rules of test_planes_gpu for this kernel and epilogue: against the on-the-fly fp16x3 kernel
    2e-6 of the maximum (C and aux), planes bit for bit those of the split pass of C (itself the host P32 split).  Against float64
    (drop mask exported with segmm_dropout_mult over the FLAT index of the [M, N] output) there is no counterpart in
    test_planes_gpu for this epilogue: the plane kernel's mean relative error may be 1.5 x that of the exact-fp32 engine on the same
    inputs + 1e-7 (the allowance test_gemm_p_nt_matches_fp64_and_on_the_fly gives the plain product).  Measured on an MI355X, mean
    relative errors plane / exact-fp32: C 1.0e-7 .. 4.2e-7 / 1.1e-7 .. 6.7e-7, aux 8.5e-8 .. 3.9e-7 / 9.1e-8 .. 6.2e-7 over the
    six shapes (the three kernel generations give the same figures; both grow with K)."""
    H = _abi()
    A, W, bias = _rand(M, K, seed=1), _rand(N, K, seed=2, scale=0.05), _rand(N, seed=3, scale=0.1)
    A[::7] *= 3.0
    kw = dict(bias=bias, activation=H.ACT_GELU, drop_p=0.1, seed=61, site=E_SITE, ldaux=N)
    Cp, Cl, Cf = (torch.full((M, N), 7.0, device=DEV) for _ in range(3))
    auxp, auxl, auxf = (torch.zeros(M, N, device=DEV) for _ in range(3))
    scale = 2.0 ** 6
    hdr = H.new_site(DEV)[0]
    sc = torch.tensor([scale], dtype=torch.float32, device=DEV)
    pl = torch.zeros((M, 2 * N), dtype=torch.float16, device=DEV)
    H.gemm_p(H.LAYOUT_NT, M, N, K, H.to_planes(A, M, K), H.to_planes(W, N, K, keep_f32=False), Cp, N, aux=auxp,
             c_pt=H.PT(pl, hdr, M, N, f32=Cp), c_scale_ptr=sc.data_ptr(), **kw)
    H.gemm(H.LAYOUT_NT, M, N, K, A, K, W, K, Cl, N, engine=H.ENGINE_F16X3, aux=auxl, **kw)
    H.gemm(H.LAYOUT_NT, M, N, K, A, K, W, K, Cf, N, engine=H.ENGINE_F32, aux=auxf, **kw)
    assert float((Cp - Cl).abs().max()) <= 2e-6 * float(Cl.abs().max())
    assert float((auxp - auxl).abs().max()) <= 2e-6 * float(auxl.abs().max())
    assert torch.equal(pl, _ref_planes(H, Cp, M, N, scale))
    assert float(hdr[0]) == scale and float(hdr[1]) == 0.0 and float(hdr[H.SITE_HDR:].max()) == float(Cp.abs().max())
    mult = torch.empty(M * N, device=DEV)
    H.dropout_mult(mult, M * N, 0.1, 61, E_SITE)
    G = A.double() @ W.double().t() + bias.double()
    ref = _gelu64(G) * mult.view(M, N).double()
    assert 0.05 < float((mult == 0).float().mean()) < 0.15
    e = dict(C=(_mean_rel(Cp, ref), _mean_rel(Cf, ref)), aux=(_mean_rel(auxp, G), _mean_rel(auxf, G)))
    print("ffn nt gelu %s (%d, %d, %d): mean rel err plane / exact-fp32  C %.2e / %.2e  aux %.2e / %.2e" % (
        gemm_generation, M, N, K, e["C"][0], e["C"][1], e["aux"][0], e["aux"][1]))
    for k, (ep, ef) in e.items():
        assert ep <= 1.5 * ef + 1e-7, (k, ep, ef)


@pytest.mark.parametrize("M,N,K", FFN_SHAPES)
def test_gemm_p_nt_dgelu_reads_aux_at_ffn_shapes(gemm_generation, M, N, K):
    """The DGELU input-gradient launch: dG = drop(dM . W1) * gelu'(aux), aux [M, N] read at ldaux = N (N = ff when K = d), planes of
    dG written by the epilogue.  Rules as in the GELU test; measured mean relative errors plane / exact-fp32 against float64:
    1.0e-7 .. 3.9e-7 / 1.0e-7 .. 6.2e-7 over the six shapes, the same on every kernel generation."""
    H = _abi()
    A, W = _rand(M, K, seed=4, scale=0.01), _rand(N, K, seed=5, scale=0.05)
    aux = _rand(M, N, seed=6)
    kw = dict(activation=H.ACT_DGELU, drop_p=0.1, seed=62, site=E_SITE, ldaux=N)
    Cp, Cl, Cf = (torch.full((M, N), 7.0, device=DEV) for _ in range(3))
    scale = 2.0 ** 12
    hdr = H.new_site(DEV)[0]
    sc = torch.tensor([scale], dtype=torch.float32, device=DEV)
    pl = torch.zeros((M, 2 * N), dtype=torch.float16, device=DEV)
    H.gemm_p(H.LAYOUT_NT, M, N, K, H.to_planes(A, M, K), H.to_planes(W, N, K, keep_f32=False), Cp, N, aux=aux.clone(),
             c_pt=H.PT(pl, hdr, M, N, f32=Cp), c_scale_ptr=sc.data_ptr(), **kw)
    H.gemm(H.LAYOUT_NT, M, N, K, A, K, W, K, Cl, N, engine=H.ENGINE_F16X3, aux=aux.clone(), **kw)
    H.gemm(H.LAYOUT_NT, M, N, K, A, K, W, K, Cf, N, engine=H.ENGINE_F32, aux=aux.clone(), **kw)
    assert float((Cp - Cl).abs().max()) <= 2e-6 * float(Cl.abs().max())
    assert torch.equal(pl, _ref_planes(H, Cp, M, N, scale))
    assert float(hdr[1]) == 0.0 and float(hdr[H.SITE_HDR:].max()) == float(Cp.abs().max())
    mult = torch.empty(M * N, device=DEV)
    H.dropout_mult(mult, M * N, 0.1, 62, E_SITE)
    ref = (A.double() @ W.double().t()) * mult.view(M, N).double() * _dgelu64(aux.double())
    ep, ef = _mean_rel(Cp, ref), _mean_rel(Cf, ref)
    print("ffn nt dgelu %s (%d, %d, %d): mean rel err plane / exact-fp32 %.2e / %.2e" % (gemm_generation, M, N, K, ep, ef))
    assert ep <= 1.5 * ef + 1e-7, (ep, ef)


@pytest.mark.parametrize("splits", [1, 4])
@pytest.mark.parametrize("T,N,K", FFN_SHAPES)
def test_gemm_p_tn_colsum_at_ffn_shapes(gemm_generation, T, N, K, splits):
    """The weight gradient of the Linear whose forward is the NT shape (T, N, K): gW [N, K] = dY[T, N]^T . X[T, K] with the bias
    gradient (column sums of dY, width N) from the same launch, one slab and split-K.  Rules of
    test_planes_gpu.test_gemm_p_tn_folded_column_sums: 3e-6 of the maximum against float64, column sums 3e-6 of the largest
    column's sum of magnitudes."""
    H = _abi()
    dY, X = _rand(T, N, seed=40, scale=0.01), _rand(T, K, seed=41)
    C, cs = torch.full((N, K), 7.0, device=DEV), torch.full((N,), 7.0, device=DEV)
    ws = torch.empty(splits * (N * K + N), device=DEV)
    pdy, px = H.to_planes(dY, T, N), H.to_planes(X, T, K)
    H.gemm_p(H.LAYOUT_TN, N, K, T, pdy, px, C, K, splits=splits, workspace=ws, colsum_out=cs)
    ref = dY.double().sum(0)
    tol = 3e-6 * float(dY.double().abs().sum(0).max())
    assert float((cs.double() - ref).abs().max()) <= tol
    refC = dY.double().t() @ X.double()
    assert float((C.double() - refC).abs().max() / refC.abs().max()) < 3e-6
    H.gemm_p(H.LAYOUT_TN, N, K, T, pdy, px, C, K, splits=splits, workspace=ws, colsum_out=cs, accumulate=True)
    assert float((cs.double() - 2 * ref).abs().max()) <= 2 * tol
    assert float((C.double() - 2 * refC).abs().max() / refC.abs().max()) < 6e-6


@pytest.mark.parametrize("d,ff", [(32, [96, 32]), (64, [32, 160, 64]), (768, [1056, 768])])
def test_store_weight_planes_of_rectangular_mlp_matrices(d, ff):
    """segmm_wsplit_p32 through the parameter store: the planes of every [ff, d] and [d, ff] matrix and of their transposes
    ([d, ff] and [ff, d] images, what the input-gradient GEMMs read) are the host P32 split of the weights, bit for bit
    (test_p32_format_gpu._check_store)."""
    from test_p32_format_gpu import _check_store
    H = _abi()
    if H.GEMM_ENGINE != H.ENGINE_F16X3P:
        pytest.skip("plane engine only")
    model, _, _ = _synth(d, 4 if d < 768 else 16, len(ff), ff, 40, 10, d, 2)
    model = model.cuda()
    st = model._store
    st.ensure()
    torch.cuda.synchronize()
    _check_store(st, st.flat.detach().cpu().numpy().copy(), "ff = %s" % ff)
    mats = {n: (R, C, tr) for n, _, R, C, tr in st._wmats}
    for i, f in enumerate(ff[:-1]):
        assert mats["backbone1.encoder.layers.%d.ff_vid.layers.0.weight" % i] == (f, d, True)
        assert mats["backbone1.encoder.layers.%d.ff_vid.layers.1.weight" % i] == (d, f, True)
