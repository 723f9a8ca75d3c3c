"""Videos of more than 64 segments on the MI355X: the loss kernel (csrc/loss.h: loss_fwd_bwd_kernel<R>, R = ceil(S / 64) segments per
lane, here R = 2, 3, 4) under the float64 rule of helpers.loss_check -- the rule, tau and the checks of test_loss_gpu.run_case
unchanged --, the device permutation draws up to S = 256, the attention kernels at key blocks of up to 176 + 16 tokens, whole models, the trainer and the
evaluation kernels at S in (64, 176].  The yardstick at these sizes is the CPU oracle (oracle/segmm_oracle.py) in float64, which
the golden fixtures pin to the reference at S = 20 and 40.  Run with ``pytest -m gpu``.

SEGMM_LOSS_RATIO_LOG=<file>: the worst |k - t| / allowance per quantity family of this module's loss cases is written there."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from helpers import (LOGIT_REGIMES, LOSS_SLOTS, ROOT, WORST_RATIO, all_label_rows, build_model, call_model, loss_cfg, loss_check,
                     loss_compare, make_logits, oracle_loss)
from test_loss_gpu import ORDERS, REAL_LISTS, _bias, _spec, _stats_host, k8, run_case
from test_model_gpu import _check_live_grads
from test_ops_gpu import _attn_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"

sys.path.insert(0, os.path.join(ROOT, "oracle"))
from segmminterest_amd.synth import l1_normalize, make_batch, make_labels  # noqa: E402

ALL_LOSSES = ["focal", "interestBPR", "surviveCE", "interestCE", "interestKL", "huber", "hazard"]
# durations at which a lane-ownership, carry or leave-index mistake shows: around every multiple of the wave, and the maximum
BOUNDARY_DURS = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193)


@pytest.fixture(scope="module", autouse=True)
def ratio_log():
    before = dict(WORST_RATIO)
    WORST_RATIO.clear()
    yield
    path = os.environ.get("SEGMM_LOSS_RATIO_LOG")
    if path:
        with open(path, "w") as f:
            json.dump(dict(sorted(WORST_RATIO.items())), f, indent=1)
    for k, v in before.items():
        WORST_RATIO[k] = max(WORST_RATIO.get(k, 0.0), v)


def _abi():
    from segmminterest_amd import hipabi
    hipabi.lib()
    return hipabi


def boundary_rows(S):
    """all_label_rows' rows of the durations BOUNDARY_DURS + (S - 1, S) that fit S, every leave index v in [0, dur] (v = dur: fully
    watched): 457 rows at S = 128, 1 679 at S = 256."""
    rows = []
    for dur in sorted({d for d in BOUNDARY_DURS + (S - 1, S) if 1 <= d <= S}):
        for v in range(dur + 1):
            r = [-2] * S
            for j in range(dur):
                r[j] = 1 if (j < v or v == dur) else (0 if j == v else -1)
            rows.append(r)
    return torch.tensor(rows, dtype=torch.int64)


def test_boundary_rows_counts():
    assert boundary_rows(128).shape == (457, 128) and boundary_rows(256).shape == (1679, 256)
    full = {tuple(r) for r in all_label_rows(70).tolist()}
    assert {tuple(r) for r in boundary_rows(70).tolist()} <= full


# ------------------------------------------------------------------ the loss kernel, S = 65: every label row
_CASES65 = [(reg, order) for reg in LOGIT_REGIMES for order in ORDERS]


@pytest.mark.parametrize("regime,order", _CASES65)
def test_all_label_rows_s65(regime, order):
    """All 2 210 (dur, v) rows of S = 65 -- one segment in the second slot of lane 0 -- in one batch, all 7 losses; mask_loss,
    learnable_bias and the exposure profile cycle over the cases as in test_loss_gpu.test_all_label_rows."""
    S = 65
    i = _CASES65.index((regime, order))
    mask_loss, bias, expo = i % 2, (i // 2) % 2 and regime != "ties", ("ones", "stat")[(i // 4) % 2]
    gt = all_label_rows(S)
    assert gt.shape[0] == 2210
    z = make_logits(regime, gt.shape[0], S, seed=100 + i)
    cfg = loss_cfg(ORDERS[order], S, mask_loss=mask_loss, learnable_bias=int(bias), exposure=expo)
    run_case(z, gt, cfg, _bias(S, i) if bias else None, what="S=%d %s %s" % (S, regime, order))


# ------------------------------------------------------------------ one past a wave, exact multiples, one past them, the maximum
_SIZES = (100, 128, 129, 192, 193, 255, 256)
_CASES_B = [(S, reg) for S in _SIZES for reg in LOGIT_REGIMES]


@pytest.mark.parametrize("S,regime", _CASES_B)
def test_boundary_rows_long_sizes(S, regime):
    """The rows of boundary_rows(S) (R = 2, 3 and 4 segments per lane; full and partial last slots), all 7 losses, every regime;
    the order of the list, mask_loss, learnable_bias and the exposure profile cycle over the cases."""
    i = _CASES_B.index((S, regime))
    order = list(ORDERS)[i % 3]
    mask_loss, bias, expo = (i // 3) % 2, i % 2 and regime != "ties", ("ones", "stat")[(i // 2) % 2]
    gt = boundary_rows(S)
    z = make_logits(regime, gt.shape[0], S, seed=300 + i)
    cfg = loss_cfg(ORDERS[order], S, mask_loss=mask_loss, learnable_bias=int(bias), exposure=expo)
    run_case(z, gt, cfg, _bias(S, i) if bias else None, what="S=%d %s %s" % (S, regime, order))


@pytest.mark.parametrize("mask_loss", [0, 1])
@pytest.mark.parametrize("regime", LOGIT_REGIMES)
@pytest.mark.parametrize("loss", ALL_LOSSES)
def test_each_loss_alone_s130(loss, regime, mask_loss):
    """One loss alone at S = 130 (three slots, the last with two segments), as test_loss_gpu.test_each_loss_alone at S = 33: its
    gradient sets every row's scale.  Rows: boundary_rows(130) (718 rows; all 8 645 rows cost the float64 oracle ~10 s a case)."""
    S = 130
    gt = boundary_rows(S)
    z = make_logits(regime, gt.shape[0], S, seed=7 + LOSS_SLOTS.index(loss))
    run_case(z, gt, loss_cfg([loss], S, mask_loss=mask_loss, exposure="stat"), what="%s %s" % (loss, regime))


@pytest.mark.parametrize("B", [1, 65, 257])
@pytest.mark.parametrize("li", range(len(REAL_LISTS)))
def test_reference_lists_make_labels_s160(li, B):
    """make_labels batches with the reference configurations' loss lists at S = 160; huber / mse loop over Bg (1, 2 and 5 trips)."""
    S = 160
    gt, _, _ = make_labels(B, S, torch.Generator().manual_seed(B + 17 * li), allow_full_len=False)
    z = make_logits("trained", B, S, seed=B + li)
    lst = REAL_LISTS[li]
    cfg = loss_cfg(lst, S, mask_loss=int("interestCE" in lst and li % 2), learnable_bias=li % 2, exposure="stat" if li % 3 else "ones")
    run_case(z, gt, cfg, _bias(S, li) if li % 2 else None, what="list %d B=%d" % (li, B))


def test_data_parallel_shards_add_up_s100():
    """512 rows of S = 100 in G = 8 shards, as test_loss_gpu.test_data_parallel_shards_add_up: global statistics through
    label_stats / label_stats_unpack, the shard losses add up to the full batch's float64 loss, the shard dlogits are its rows."""
    H = _abi()
    S, G, Bfull = 100, 8, 512
    B = Bfull // G
    gt, _, _ = make_labels(Bfull, S, torch.Generator().manual_seed(5))
    z = make_logits("trained", Bfull, S, seed=5)
    cfg = loss_cfg(ALL_LOSSES, S, mask_loss=1, exposure="stat")
    sp = _spec(cfg)
    gathered = torch.full((G, 2 * B + 3), float("nan"), device=DEV)
    for g in range(G):
        rec = gathered[g]
        H.label_stats(gt[g * B:(g + 1) * B].to(DEV).contiguous(), B, S, int(sp.has_focal), rec[:B], rec[B:2 * B], rec[2 * B:])
    v_all, v2_all, norms = torch.empty(G * B, device=DEV), torch.empty(G * B, device=DEV), torch.empty(3, device=DEV)
    H.label_stats_unpack(gathered, G, B, v_all, v2_all, norms)
    v, v2, nh = _stats_host(gt, True)
    assert torch.equal(v_all.cpu(), v) and torch.equal(v2_all.cpu(), v2) and torch.equal(norms.cpu(), nh)
    slots, total, dls = np.zeros(9), 0.0, []
    for g in range(G):
        sh = slice(g * B, (g + 1) * B)
        o = k8(z[sh], gt[sh], cfg, stats=(v_all, v2_all, norms))
        assert torch.equal(o["logits_out"], z[sh].float())
        slots += o["slots"]
        total += o["total"]
        dls.append(o["dlogits"])
    t, r = oracle_loss(z, gt, cfg), oracle_loss(z, gt, cfg, dtype=torch.float32)
    n_edge = loss_compare(dict(slots=slots, total=total, dlogits=np.concatenate(dls)), t, r, cfg, "G=8 shards S=100")
    assert n_edge <= max(1, int(0.02 * Bfull))


def test_loss_refuses_more_than_256_segments():
    H = _abi()
    B, S = 4, 257
    z, gt = torch.zeros(B, S, device=DEV), torch.ones(B, S, dtype=torch.int64, device=DEV)
    f = lambda *s: torch.zeros(*s, device=DEV)
    with pytest.raises(RuntimeError, match="256"):
        H.loss_fwd_bwd(B, S, z, gt, None, None, f(S), [0.0] * 9, [1] * 9, 0, 0, 0, f(3), f(B), f(B), B, f(B, S), f(B, S), f(B, 12))


# ------------------------------------------------------------------ draws
@pytest.mark.parametrize("S", [65, 128, 256])
def test_device_permutations_up_to_256(S):
    """segmm_rand_perm_rows beyond one segment per lane: every row a permutation of 0 .. S-1, every value equally likely in the
    first position (256 expected each; the bound of test_eval_gpu's S = 40 case), another seed another draw."""
    H = _abi()
    rows = 256 * S
    perm = torch.full((rows, S), float("nan"), device=DEV)
    H.rand_perm_rows(perm, rows, S, 777, 5)
    assert torch.equal(perm.sort(1).values, torch.arange(S, device=DEV, dtype=torch.float32).expand(rows, S))
    first = torch.bincount(perm[:, 0].long(), minlength=S).float()
    assert float((first / first.mean() - 1).abs().max()) < 0.4
    assert len({tuple(r.tolist()) for r in perm[:64]}) == 64
    perm2 = torch.full((rows, S), float("nan"), device=DEV)
    H.rand_perm_rows(perm2, rows, S, 778, 5)
    assert not torch.equal(perm, perm2)
    assert torch.equal(perm2.sort(1).values, perm.sort(1).values)


def test_device_permutations_refuse_257():
    H = _abi()
    with pytest.raises(RuntimeError, match="256"):
        H.rand_perm_rows(torch.empty(4, 257, device=DEV), 4, 257, 1, 1)


def test_device_permutations_keep_their_stream_up_to_64():
    """S <= 64 (rand_perm_rows_kernel<1>, one index per lane) keeps its stream: rank of index i's key r.x of counter row * 64 + i
    (recorded noPos steps depend on the stream).  Restated on the host for one row through the same kernel's own output at
    another S: the first 40 keys of a row are the same at S = 40 and S = 64, so the relative order of 0 .. 39 agrees."""
    H = _abi()
    a, b = torch.empty(8, 40, device=DEV), torch.empty(8, 64, device=DEV)
    H.rand_perm_rows(a, 8, 40, 99, 3)
    H.rand_perm_rows(b, 8, 64, 99, 3)
    for r in range(8):
        assert [int(x) for x in b[r].tolist() if x < 40] == [int(x) for x in a[r].tolist()]


# ------------------------------------------------------------------ attention at the new shapes
@pytest.mark.parametrize("B,H_,dh,Lq,La,Lb", [(2, 4, 16, 96, 96, 10), (2, 4, 16, 10, 10, 96), (2, 4, 16, 160, 160, 1), (2, 4, 16, 1, 1, 160),
                                              (2, 4, 32, 80, 80, 100), (2, 4, 32, 100, 100, 80), (2, 2, 48, 176, 176, 16)])
def test_attention_fwd_bwd_long_blocks(B, H_, dh, Lq, La, Lb):
    """The fp64 restatement, input distribution and absolute bounds of test_ops_gpu.test_attention_fwd_bwd at the video-side and
    user-side calls of the long-video models below and at the 192-key maximum."""
    H = _abi()
    d = H_ * dh
    g = torch.Generator().manual_seed(B * 1000 + Lq)
    mk = lambda L: (torch.randn(B, L, d, generator=g) * 0.7).to(DEV)
    Qa, Qb, Ka, Va, Kb, Vb = mk(Lq), mk(Lq), mk(La), mk(La), mk(Lb), mk(Lb)
    mq = (torch.rand(B, Lq, generator=g) < 0.8).to(DEV)
    mka = (torch.rand(B, La, generator=g) < 0.8).to(DEV)
    mkb = (torch.rand(B, Lb, generator=g) < 0.7).to(DEV)
    mq[0, 0] = False
    mq[-1, -1] = True
    O = torch.empty(B * Lq, d, device=DEV)
    lse = torch.empty(2, B, H_, Lq, device=DEV)
    z = lambda t: (t, 0)
    H.attn_fwd(B, H_, dh, Lq, La, Lb, z(Qa), z(Qb), d, z(Ka), z(Va), d, z(Kb), z(Vb), d, mq, mka, mkb, O, d, lse)
    leaves = [t.double().requires_grad_(True) for t in (Qa, Qb, Ka, Va, Kb, Vb)]
    ref = _attn_ref(*leaves, mq, mka, mkb, H_)
    err = (O.view(B, Lq, d).double() - ref).abs().max().item()
    print("attention %s fwd err %.3e" % ((B, H_, dh, Lq, La, Lb), err))
    assert err < 2e-5
    dO = (torch.randn(B * Lq, d, generator=g)).to(DEV)
    ref.backward(dO.view(B, Lq, d).double())
    Dv = torch.empty(B, H_, Lq, device=DEV)
    outs = [torch.full_like(t, float("nan")) for t in (Qa, Qb, Ka, Va, Kb, Vb)]
    H.attn_bwd(B, H_, dh, Lq, La, Lb, z(Qa), z(Qb), d, z(Ka), z(Va), d, z(Kb), z(Vb), d, mq, mka, mkb, lse, O, d, dO, d, Dv,
               z(outs[0]), z(outs[1]), d, z(outs[2]), z(outs[3]), d, z(outs[4]), z(outs[5]), d)
    for name, got, leaf in zip(("dQa", "dQb", "dKa", "dVa", "dKb", "dVb"), outs, leaves):
        err = (got.double() - leaf.grad).abs().max().item()
        print("attention %s %s err %.3e" % ((B, H_, dh, Lq, La, Lb), name, err))
        assert err < 5e-5, (name, err)


# ------------------------------------------------------------------ whole model against the CPU oracle
def _edge_rows(S):
    """Label rows with durations {1, 64, 65, 128, 129, S} (those that fit S) leaving at 0, at dur - 1, or fully watched."""
    rows = []
    for dur in sorted({d for d in (1, 64, 65, 128, 129, S) if d <= S}):
        for v in sorted({0, dur - 1, dur}):
            rows.append([(1 if (j < v or v == dur) else (0 if j == v else -1)) if j < dur else -2 for j in range(S)])
    return torch.tensor(rows, dtype=torch.int64)


def _long_model_case(kind, S, Lt, d, h, N, ablation="ours"):
    cfg = dict(N=N, h=h, S=S, d=d, D_in=d if kind == "image" else 4, Lt=Lt, user=kind, photo=kind, n_users=50, n_items=500,
               loss_type_list=list(ALL_LOSSES), loss_weight=dict(loss_cfg([], S)["loss_weight"]), exposure_prob=[1.0] * S, mask_loss=0,
               ablation_type=ablation)
    torch.manual_seed(5)
    model = build_model(cfg)
    with torch.no_grad():          # attention and LayerNorms away from their initial near-identity
        for n_, p in model.named_parameters():
            if p.dim() == 2 and ".encoder.layers." in n_ and "ln_" not in n_:
                p.mul_(2.0)
            if n_.endswith("vid_proj.weight") or n_.endswith("usr_proj.weight"):
                p.mul_(100.0 if kind == "image" else 6.0)
    edge = _edge_rows(S)
    B = 8 + edge.shape[0]
    b = make_batch(B, S, Lt, cfg["D_in"], n_users=50, n_items=500, seed=9, allow_full_len=False)
    lab = b["label"]
    lab[8:] = edge
    b["photo_mask"] = lab != -2
    b["photo"] = torch.rand(B, S, cfg["D_in"], generator=torch.Generator().manual_seed(6)) * b["photo_mask"][:, :, None]
    inp = dict(usr_image=l1_normalize(b["user"]), usr_id=b["user_identity_id"], usr_mask=b["user_mask"],
               vid_image=l1_normalize(b["photo"]), vid_id=b["photo_identity_id"], vid_mask=b["photo_mask"], gt=lab)
    return cfg, model, inp


def _oracle_model(sd, cfg, inp, dtype):
    import segmm_oracle as O
    ref, grads = O.forward_backward(sd, cfg, {k: v.clone() for k, v in inp.items()}, dtype=dtype)
    return ref, grads


@pytest.mark.parametrize("kind,S,Lt,d,h,N", [("image", 80, 100, 128, 4, 3), ("image", 96, 10, 96, 2, 2), ("id", 160, 1, 64, 4, 2)])
def test_long_video_model_vs_oracle(kind, S, Lt, d, h, N):
    """segmm_oracle.model_forward, mode "train", eval mode, all seven losses with focal first: every logit within 1e-4, every loss
    value by loss_check's rule (float64 oracle, float32 oracle, the slot scales of the float64 logits), every live gradient by
    test_model_gpu._check_live_grads, the same dead parameters.  (80, 100): 192 keys, full layers on both sides."""
    cfg, model, inp = _long_model_case(kind, S, Lt, d, h, N)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    ref, rgrads = _oracle_model(sd, cfg, inp, torch.float32)
    t64, _ = _oracle_model(sd, cfg, inp, torch.float64)
    model = model.cuda().eval()
    out = call_model(model, inp, "train", DEV)
    err = (out["logits"].cpu().double() - t64["logits"].detach()).abs().max().item()
    print("model %s logits err vs float64 %.3e" % ((kind, S, Lt, d, h, N), err))
    assert err < 1e-4
    assert (out["logits"].cpu() - ref["logits"].detach()).abs().max().item() < 1e-4
    # scales of the slots: sums of |term| at the float64 model's own logits
    sc = oracle_loss(t64["logits"].detach(), inp["gt"], dict(cfg, learnable_bias=0))
    for i, name in enumerate(LOSS_SLOTS):
        if name in cfg["loss_type_list"] or name in ("mse", "mse2"):
            assert abs(sc["slots"][i] - float(t64[name].detach())) <= 1e-9 * max(1.0, abs(sc["slots"][i]))
            loss_check(float(out[name]), float(t64[name].detach()), float(ref[name].detach()), sc["slot_scales"][i], "model:" + name,
                       "%s S=%d" % (kind, S))
    loss_check(float(out["loss"].detach()), float(t64["loss"].detach()), float(ref["loss"].detach()), sc["total_scale"], "model:total",
               "%s S=%d" % (kind, S))
    out["loss"].backward()
    _check_live_grads(model, rgrads)


def test_nopos_long_video_draws_on_the_device(monkeypatch):
    """id / id, S = 160, noPos: with the step's state on the device the frame positions of a training step are drawn by
    segmm_rand_perm_rows (S <= 256), not by torch.randperm -- every row of the draw is a permutation of 0 .. S-1, two trainers
    from one seed take the same steps bitwise."""
    from segmminterest_amd import hipabi as H
    from segmminterest_amd.trainer import Trainer, default_args, init_model
    B, S, D, N, h = 16, 160, 64, 2, 4
    margs = default_args(num_layers_enc=N, d_model=D, nhead=h, input_type={"user": "id", "photo": "id"}, exposure_prob=[1.0] * S,
                         ablation_type="noPos")
    batch = {k: v.to(DEV) for k, v in make_batch(B, S, 1, D, n_users=50, n_items=500, seed=700, features=False).items()}
    fallbacks = []
    real = H.torch_fallback
    monkeypatch.setattr(H, "torch_fallback", lambda what: (fallbacks.append(what), real(what))[1])

    def run():
        torch.manual_seed(11)
        model = init_model(margs, n_users=50, n_items=500, input_dim=D, max_vid_len=S, max_usr_len=1).to(DEV)
        tr = Trainer(model, lr=1e-3, weight_decay=1e-4, device_state=True)
        losses = [float(tr.train_step(batch)["loss"].detach()) for _ in range(3)]
        fpos = model._store.buf("nopos_fpos0", (B, S)).clone()
        return losses, model._store.flat.detach().clone(), fpos

    la, pa, fa = run()
    lb, pb, fb = run()
    assert not [w for w in fallbacks if "randperm" in w], fallbacks
    assert all(np.isfinite(la)) and la == lb and torch.equal(pa, pb) and torch.equal(fa, fb)
    assert torch.equal(fa.sort(1).values, torch.arange(S, device=DEV, dtype=torch.float32).expand(B, S))
    assert len({tuple(r.tolist()) for r in fa}) == B


# ------------------------------------------------------------------ trainer
def _trainer_setup(S=96, Lt=10, D=64, N=2, h=4, B=24):
    from segmminterest_amd.trainer import default_args
    margs = default_args(num_layers_enc=N, d_model=D, nhead=h, input_type={"user": "image", "photo": "image"}, exposure_prob=[0.9] * S)
    batches = [{k: v.to(DEV) for k, v in make_batch(B, S, Lt, D, n_users=50, n_items=500, seed=300 + i).items()} for i in range(3)]
    return margs, batches


def test_trainer_steps_reproducible_s96():
    """Three Trainer.train_steps (dropout off) at S = 96, Lt = 10: finite losses, bitwise the same on a second run from the seed."""
    from segmminterest_amd.trainer import Trainer, init_model
    S, Lt, D = 96, 10, 64
    margs, batches = _trainer_setup(S, Lt, D)

    def run():
        torch.manual_seed(7)
        model = init_model(margs, n_users=50, n_items=500, input_dim=D, max_vid_len=S, max_usr_len=Lt).to(DEV)
        tr = Trainer(model, lr=1e-3, weight_decay=1e-4, dropout=False)
        losses = [float(tr.train_step(batches[i])["loss"].detach()) for i in range(3)]
        return losses, model._store.flat.detach().clone()

    la, pa = run()
    lb, pb = run()
    assert all(np.isfinite(la)) and la == lb and len(set(la)) > 1
    assert torch.isfinite(pa).all() and torch.equal(pa, pb)


def test_recorded_steps_equal_eager_steps_s96():
    """record / run_recorded at S = 96 (the loss and every launch of the step through the recorded C phases) leave the
    parameters and losses of the same steps enqueued from Python, bitwise."""
    from segmminterest_amd.trainer import Trainer, init_model
    S, Lt, D = 96, 10, 64
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


def test_valid_model_matches_host_metrics_s96():
    """Trainer.valid_model (device ranks) == the reference's host loop, as test_eval_gpu.test_valid_model_matches_host_metrics."""
    from segmminterest_amd import my_evaluation as E
    from segmminterest_amd.trainer import Trainer, init_model
    S, Lt, D = 96, 10, 64
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


def test_too_many_attention_keys_refused_before_any_launch(monkeypatch):
    """S = 200, Lt = 1: 208 + 16 padded keys.  The forward raises a RuntimeError that names the limit of 192 before any C call of the
    pass (today's C check fired at the first attention launch, after the embedding and projection launches)."""
    from segmminterest_amd import hipabi as H
    from segmminterest_amd.trainer import Trainer, default_args, init_model
    S, D = 200, 64
    margs = default_args(num_layers_enc=2, d_model=D, nhead=4, input_type={"user": "id", "photo": "id"}, exposure_prob=[1.0] * S)
    torch.manual_seed(1)
    model = init_model(margs, n_users=50, n_items=500, input_dim=D, max_vid_len=S, max_usr_len=1).to(DEV)
    tr = Trainer(model, dropout=False)
    batch = {k: v.to(DEV) for k, v in make_batch(8, S, 1, D, n_users=50, n_items=500, seed=1, features=False).items()}
    model._store.ensure()
    torch.cuda.synchronize()
    calls = []
    for name in ("layernorm_fwd", "embed_id_vid", "embed_id_usr", "attn_fwd", "gemm"):
        if hasattr(H, name):
            monkeypatch.setattr(H, name, lambda *a, _n=name, **k: calls.append(_n))
    with pytest.raises(RuntimeError, match=r"192"):
        tr.train_step(batch)
    assert calls == []


# ------------------------------------------------------------------ evaluation kernels above 64 segments
@pytest.mark.parametrize("S", [65, 160])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("permutation", [0, 1])
def test_rank_leave_long_rows(S, masked, permutation):
    """TOP_K_leave_device: integer ranks equal numpy's (as test_eval_gpu.test_rank_leave_bit_exact_vs_oracle, at S = 65 and 160)."""
    _abi()
    from oracle import segmm_oracle as O
    from segmminterest_amd import my_evaluation as E
    B = 70
    gt = make_labels(B, S, torch.Generator().manual_seed(B + S))[0]
    g = torch.Generator().manual_seed(B * 7 + S)
    x = (torch.rand(B, S, generator=g) * 8).round() / 8 * 0.9 + 0.05          # many exact ties
    vl = (gt == 1).sum(1, keepdim=True).numpy()
    mb = (gt != -2).numpy()
    np.random.seed(123)
    want = O.top_k_leave(x.numpy(), vl, mb, permutation=permutation, S=S, masked=masked)
    np.random.seed(123)
    got = E.TOP_K_leave_device(x.to(DEV), gt.to(DEV), permutation=permutation, masked=masked)
    assert set(got) == set(want)
    for k in want:
        assert float(got[k]) == float(want[k]), (k, got[k], want[k])


def test_probauc_s160():
    H = _abi()
    from oracle import segmm_oracle as O
    from segmminterest_amd import my_evaluation as E
    B, S = 60, 160
    gt = make_labels(B, S, torch.Generator().manual_seed(9))[0]
    g = torch.Generator().manual_seed(4)
    interests = torch.rand(B, S, generator=g) * 0.1 + 0.9          # survival stays above fp32's underflow over 160 segments
    interests[:, ::7] = 0.95                                       # ties
    surv, label = H.survival(interests.to(DEV), gt.to(DEV))
    lab = label.cpu().numpy().reshape(-1)
    s = surv.cpu().numpy().reshape(-1).astype(np.float64)
    m = lab >= 0
    want = O.auc_rank_sum(lab[m] == 1, s[m])
    assert abs(E.ProbAUC_batch_device(interests.to(DEV), gt.to(DEV)) - want) < 1e-12
