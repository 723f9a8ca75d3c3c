"""Shared test helpers: golden-fixture loading."""
import json
import math
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

# metric known answers; config-1 labels of the reference's sample file; data-format fixtures (oracle/gen_golden_io.py)
NOT_MODEL_CASES = ("metrics_kat.npz", "cfg1_labels.npz", "io_dataloader.npz", "io_cliprec.npz")
# train_*: TRAIN-mode fixtures (the reference's dropout masks recorded in call order); they pin the oracle's dropout placement
TRAIN_CASES = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".npz") and f.startswith("train_"))
MODEL_CASES = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".npz") and f not in NOT_MODEL_CASES
                     and not f.startswith("train_"))


def load_case(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    cfg = json.loads(str(z["cfg"]))
    cfg["loss_type_list"] = [x.strip() for x in cfg["loss"].split(",")]
    grp = {"sd": {}, "in": {}, "out": {}, "grad": {}, "adam1": {}, "adam3": {}, "inf": {}}
    for k in z.files:
        if "/" in k and not k.startswith("mask"):
            g, n = k.split("/", 1)
            grp[g][n] = torch.from_numpy(z[k])
    nograd = json.loads(str(z["nograd"]))
    extra = {"adam_loss3": float(z["adam_loss3"])} if "adam_loss3" in z.files else {}
    if "mask_p" in z.files:          # train-mode fixture: dropout keep-masks of the reference in call order
        ps = z["mask_p"]
        masks = []
        for k in range(len(ps)):
            shape = tuple(int(x) for x in z["mask_shape/%d" % k])
            n = int(np.prod(shape))
            keep = np.unpackbits(z["mask/%d" % k])[:n].reshape(shape).astype(bool)
            masks.append((float(ps[k]), torch.from_numpy(keep)))
        extra["masks"] = masks
        extra["mask_calls_fwd"] = int(z["mask_calls_fwd"])
    return cfg, grp, nograd, extra


def build_model(cfg, device=None):
    """Builds the segmminterest_amd facade exactly like the reference's init_model builds its model
    (main_for_seq_leave_earlystop_SegMM.py:60-130), from a golden-fixture cfg dict."""
    import argparse
    import segmminterest_amd as M
    S, N, d, h = cfg["S"], cfg["N"], cfg["d"], cfg["h"]
    args = argparse.Namespace(debug=0, num_layers_enc=N, ablation_type=cfg.get("ablation_type", "ours"), d_model=d, nhead=h,
                              input_type={"user": cfg["user"], "photo": cfg["photo"]},
                              learnable_bias=cfg.get("learnable_bias", 0), exposure_prob=cfg["exposure_prob"],
                              fusion_heads=cfg.get("fusion_heads", 2), loss_type_list=cfg["loss_type_list"],
                              loss_weight=cfg["loss_weight"], mask_loss=cfg.get("mask_loss", 0), use_pe=cfg.get("use_pe", 1))

    def backbone(user_id_max, video_id_max, max_usr_len):
        return M.SegFormerX(d_model_in=d, d_model_lvls=[d] * N, num_head_lvls=[h] * N, ff_dim_lvls=[d] * N,
                            input_vid_dim=max(cfg["D_in"], 1), input_usr_dim=max(cfg["D_in"], 1), max_vid_len=S,
                            max_usr_len=max_usr_len, sr_ratio_lvls=[1] * N, use_patch_merge=[False] * N,
                            output_layers=[-1], model_cfg=args, user_id_max=user_id_max, video_id_max=video_id_max,
                            use_pe=cfg.get("use_pe", 1))

    nu, ni = cfg.get("n_users", 0), cfg.get("n_items", 0)
    u, p = cfg["user"], cfg["photo"]
    if u == "both" or p == "both":
        um1, ul1, um2, ul2 = {"both": (-1, cfg["Lt"], nu, 1), "id": (nu, 1, nu, 1), "image": (-1, cfg["Lt"], -1, cfg["Lt"])}[u]
        vm1, vm2 = {"both": (-1, ni), "id": (ni, ni), "image": (-1, -1)}[p]
        model = M.MultiScaleTemporalDetrLeaveFocal(backbone(um1, vm1, ul1), backbone(um2, vm2, ul2), None, torch.nn.Identity(), args)
    else:
        um1, ul1 = (nu, 1) if u == "id" else (-1, cfg["Lt"])
        vm1 = ni if p == "id" else -1
        model = M.MultiScaleTemporalDetrLeaveFocal(backbone(um1, vm1, ul1), None, None, torch.nn.Identity(), args)
    if device is not None:
        model = model.to(device)
    model._test_fwd_seed = cfg.get("fwd_seed")      # 'noPos' fixtures: torch is reseeded before every forward
    return model


def call_model(model, inp, mode="train", device=None, fwd_seed=None):
    """``fwd_seed``: the 'noPos' fixtures reseed torch before every forward (the model draws torch.randperm)."""
    kw = {k: (v.to(device) if device is not None else v) for k, v in inp.items()}
    fwd_seed = getattr(model, "_test_fwd_seed", None) if fwd_seed is None else fwd_seed
    if fwd_seed is not None:
        torch.manual_seed(fwd_seed)
    return model(usr_image=kw["usr_image"], usr_id=kw["usr_id"], usr_mask=kw["usr_mask"], vid_image=kw["vid_image"],
                 vid_id=kw["vid_id"], vid_mask=kw["vid_mask"], gt=kw["gt"].clone(), mode=mode)


# ------------------------------------------------------------------ observed gradient errors (DESIGN.md §5 quotes them)
GRAD_ERRS = {}          # test id -> (worst error / tensor maximum, tensor name, tensor maximum)


def note_grad_err(name, err, scale):
    """Whole-model tests call this for every live gradient they compare; with SEGMM_GRAD_ERR_LOG=<file> the session writes the
    worst relative error per test (conftest.pytest_sessionfinish) and which tensor it was."""
    label = os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0]
    if scale <= 1e-5:          # gradients that are zero in exact arithmetic (sums of d loss / d logits under the shift-invariant BPR
        return                 # loss): cancellation noise in the reference too, judged by the tests' absolute floor, not listed
    rel = err / max(scale, 1e-30)
    if label not in GRAD_ERRS or rel > GRAD_ERRS[label][0]:
        GRAD_ERRS[label] = (rel, name, scale)


# ------------------------------------------------------------------ leave/skip losses against float64 (test_loss_cpu.py, test_loss_gpu.py)
# The loss slots of segm_loss_fwd_bwd's `parts` / `losses` (csrc/loss.h L_BPR .. L_MSE2); mse / mse2 are logged, never weighted.
LOSS_SLOTS = ("interestBPR", "focal", "surviveCE", "interestCE", "interestKL", "huber", "hazard", "mse", "mse2")
# oracle/gen_golden.py's ALL_LOSS_W plus a 'huber' entry: compute_loss weights huber by 'mse' (decoder_leave_focal.py:561-566), so
# the 'huber' value is never used by a correct implementation; it differs from every other weight so that using it shows.
LOSS_WEIGHTS = {"focal": 1.0, "mse": 0.7, "hazard": 0.9, "surviveCE": 1.1, "interestBPR": 1.0, "interestCE": 0.8,
                "interestKL": 1.2, "huber": 0.45}
# Every value the loss kernels produce is a sum of fp32 terms, each term a few fp32 operations (exp / log / divide: a few units
# of rounding u = 2^-24 each).  The longest summation chain behind one value: a wave reduction (6 levels), the huber / mse loop
# over the global batch (Bg / 64 <= 32 adds per lane at Bg = 2048), then loss_finish's column sum (B / 64 chained adds, 2 + 16
# more, B <= 2144 here: <= 52 adds) -- under 100 additions in all, so the forward error of any slot is at most ~100 u of the sum
# of |term| = 2^-17.4 of it.  tau = 2^-16 leaves a factor of ~2.7 over that worst-case bound and is 500x below the smallest
# planted defect test_loss_cpu.py rejects.  dlogits: the same chains (a suffix scan over 64 lanes, the huber derivative over Bg)
# against the row's largest gradient.
LOSS_TAU = 2.0 ** -16
F32_MIN_SUBNORMAL = 2.0 ** -149          # below the fp32 grid: a true value this small can only come out as 0 or +-2^-149
BPR_EDGE_REL = 1e-3          # BPR rows whose float64 A lies this close (relative) to a clamp edge: the clamp is discontinuous there
WORST_RATIO = {}             # quantity family -> worst |k - t| / allowance seen (test_loss_gpu.py writes it out on request)


def loss_cfg(losses, S, mask_loss=0, learnable_bias=0, exposure="ones", weights=None):
    """A compute_loss cfg: ``exposure`` "ones" or "stat" (oracle/gen_golden.py: 0.5 + 0.5 U[0, 1), seed 7)."""
    if exposure == "stat":
        g = torch.Generator().manual_seed(7)
        expo = (0.5 + 0.5 * torch.rand(S, generator=g)).tolist()
    else:
        expo = [1.0] * S
    return dict(loss_type_list=list(losses), loss_weight=dict(weights or LOSS_WEIGHTS), exposure_prob=expo,
                mask_loss=int(mask_loss), learnable_bias=int(learnable_bias))


def _labels_seen_by(cfg, gt, name):
    """The labels loss ``name`` sees: 'focal' earlier in the list rewrites them in place (decoder_leave_focal.py:534-535)."""
    lst = cfg["loss_type_list"]
    if "focal" in lst and lst.index("focal") < lst.index(name):
        g = gt.clone()
        g[g > 0] = 1
        g[g == -1] = 0
        return g
    return gt


def _slot_scales(z, gt, cfg, out, gs):
    """Sum of |term| behind each slot (float64, no gradient).  Every term of focal, surviveCE, interestBPR, interestCE, huber,
    mse and mse2 is >= 0, so there the scale is |value|; interestKL and hazard are differences of two sums."""
    sc = {n: abs(float(out[n].detach())) for n in LOSS_SLOTS if n in out}
    B, S = gt.shape
    Bg = float(B if gs is None else gs["norms"][1])
    mask = (gt != -2).to(z.dtype)
    if "interestKL" in out:
        g = _labels_seen_by(cfg, gt, "interestKL")
        ng = (g != 0).to(z.dtype).softmax(1)
        logni = z.log_softmax(1)
        terms = (ng * ng.log()).abs() + (ng * logni).abs()
        if cfg.get("mask_loss", 0):          # (a row of padding only adds nothing, as in the kernel)
            terms = (terms * mask).sum(1) / mask.sum(1).clamp(min=1)
        sc["interestKL"] = float(terms.sum()) / Bg
    if "hazard" in out:
        hz = torch.where(gt != -2, 1 - torch.exp(torch.cumsum(torch.log(torch.sigmoid(z)), 1)), torch.zeros_like(z))
        v = (gt == 1).sum(1)
        acc = 0.0
        for i in range(B):
            t = int(v[i])
            if t < S:
                acc += abs(math.log(float(hz[i, t]) + 1e-6)) + abs(math.log(float(hz[i, t:].sum()) + 1e-6))
        sc["hazard"] = acc / Bg
    return sc


class _AccurateSigmoid(torch.autograd.Function):
    """sigmoid whose derivative is sigmoid(x) sigmoid(-x): torch's p (1 - p) rounds 1 - p to 0 for x > 37 even in float64, where
    the true derivative -- and the fp32 kernel's, which takes 1 - p as sigmoid(-x) -- is still e^-x."""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return torch.sigmoid(x)

    @staticmethod
    def backward(ctx, g):
        x, = ctx.saved_tensors
        return g * torch.sigmoid(x) * torch.sigmoid(-x)


class _float64_truth:
    """Runs segmm_oracle with _AccurateSigmoid and hands out the survival scan h (its torch.cumsum) through ``hs``."""

    def __init__(self, hs):
        self.hs = hs

    def __enter__(self):
        import types
        import segmm_oracle
        hs = self.hs
        self.saved = segmm_oracle.torch

        def cumsum(x, dim):
            h = torch.cumsum(x, dim=dim)
            hs.append(h)
            return h
        proxy = types.SimpleNamespace(**{k: getattr(torch, k) for k in dir(torch) if not k.startswith("__")})
        proxy.sigmoid = _AccurateSigmoid.apply
        proxy.cumsum = cumsum
        segmm_oracle.torch = proxy

    def __exit__(self, *exc):
        import segmm_oracle
        segmm_oracle.torch = self.saved


def _interest_terms(z, gt, cfg, gs):
    """Per row, the size of the terms of interestCE / interestKL's gradient coef (ni_j csum - c_j) / Bg (c = ng, or ng / dur on
    the unmasked segments; csum = sum c): a difference that is 0 exactly when ni matches ng (equal logits on a row without a
    leave) and cancels in fp32 in any evaluation order."""
    B, S = gt.shape
    Bg = float(B if gs is None else gs["norms"][1])
    out = np.zeros(B)
    ni = z.softmax(1)
    mask = (gt != -2).to(z.dtype)
    for name in ("interestCE", "interestKL"):
        if name not in cfg["loss_type_list"]:
            continue
        ng = (_labels_seen_by(cfg, gt, name) != 0).to(z.dtype).softmax(1)
        c = mask * ng / mask.sum(1, keepdim=True).clamp(min=1) if cfg.get("mask_loss", 0) else ng
        term = abs(cfg["loss_weight"][name]) / Bg * (ni * c.sum(1, keepdim=True) + c).max(1).values
        out = np.maximum(out, term.numpy())
    return out


def oracle_loss(logits_raw, gt, cfg, sd=None, gs=None, dtype=torch.float64, fn=None):
    """Runs ``fn`` (default: segmm_oracle.compute_loss) in ``dtype`` with autograd.  Returns slots [9] (nan where a loss is not
    computed), total, dlogits = d total / d logits_raw [B, S], logits (with the learnable bias), the float64 slot / total scales
    and the BPR rows' A = sum_j sigmoid(neg_j - pos) w_j (nan for rows without a positive)."""
    if fn is None:
        import segmm_oracle
        fn = segmm_oracle.compute_loss
    z = logits_raw.detach().to(dtype).clone().requires_grad_(True)
    sd_ = None if sd is None else {k: v.detach().to(dtype) for k, v in sd.items()}
    gs_ = None if gs is None else {k: (v.to(dtype) if torch.is_tensor(v) else v) for k, v in gs.items()}
    hs = []
    if dtype == torch.float64:
        with _float64_truth(hs):
            out = fn(z, gt.clone(), cfg, sd_, gs_)
    else:
        out = fn(z, gt.clone(), cfg, sd_, gs_)
    total = out["loss"]
    dh = None
    if torch.is_tensor(total) and total.requires_grad:
        dl, dh = torch.autograd.grad(total, [z, hs[0] if hs else z], allow_unused=True)
    else:
        dl = torch.zeros_like(z)
    slots = np.array([float(out[n].detach()) if n in out else np.nan for n in LOSS_SLOTS])
    total = float(total.detach()) if torch.is_tensor(total) else float(total)
    res = dict(slots=slots, total=total, dlogits=dl.detach().double().numpy(), logits=out["logits"].detach())
    if dtype == torch.float64:
        zl = out["logits"].detach()
        sc = _slot_scales(zl, gt, cfg, out, gs)
        res["slot_scales"] = np.array([sc.get(n, 0.0) for n in LOSS_SLOTS])
        res["total_scale"] = sum(abs(cfg["loss_weight"]["mse" if n == "huber" else n]) * sc[n] for n in cfg["loss_type_list"])
        B, S = gt.shape
        v = (gt == 1).sum(1)
        A = np.full(B, np.nan)
        for i in range(B):
            t = int(v[i])
            if t < S and S > 1:
                neg = torch.cat([zl[i, :t], zl[i, t + 1:]])
                w = (neg - neg.max()).softmax(0)
                A[i] = float(((neg - zl[i, t]).sigmoid() * w).sum())
        res["A"] = A
        # interestBPR's gradient is coef dA w_j (sg_j (1 - sg_j) + sg_j - A), dA = -1 / (A n_valid): a difference of terms of size
        # w_j sg_j and w_j A that cancels as A -> 1 in any evaluation order (the reference's softmax backward forms the same
        # difference).  Its term size, not the cancelled result, is what the row's fp32 rounding scales with.
        res["bpr_term"] = np.zeros(B)
        res["grad_term"] = _interest_terms(zl, gt, cfg, gs)
        # survival losses reach logit k through g_j = d total / d h_j, j >= k: dlogit_k = (1 - p_k) sum_(j >= k) g_j.  h_j is a
        # scan of log p <= 0: each of its <= 7 roundings (6 scan levels, the log) is relative to a partial sum of |log p|, so h_j
        # carries an absolute error <= 7 u |h_j| and exp(h_j) -- hence g_j -- a relative one of the same size.  Where the g_j
        # of consecutive segments cancel (hazard's 1 / ht against 1 / R when hazard ~ 1: the survival difference surv_v -
        # surv_(v+1) = surv_v (1 - p_(v+1))), that is what the result's error scales with, in fp32 whatever the summation order.
        # Scale of element k: (1 - p_k) sum_(j >= k) |g_j| (1 + |h_j|); tau = 2^-16 = 256 u covers 7 u |h_j| plus the few
        # roundings of exp, the product and the suffix sum 30-fold.
        res["surv_term"] = np.zeros((B, S))
        if dh is not None and hs:
            h = hs[0].detach()
            gabs = (dh.abs() * (1 + h.abs())).flip(1).cumsum(1).flip(1)
            res["surv_term"] = (torch.sigmoid(-zl) * gabs).numpy()
        if "interestBPR" in cfg["loss_type_list"] and S > 1:
            n_valid = float((v < S).sum()) if gs is None else float(gs["norms"][0])
            coef = abs(cfg["loss_weight"]["interestBPR"])
            for i in range(B):
                t = int(v[i])
                if t < S and A[i] > 0:
                    neg = torch.cat([zl[i, :t], zl[i, t + 1:]])
                    w = (neg - neg.max()).softmax(0)
                    sg = (neg - zl[i, t]).sigmoid()
                    res["bpr_term"][i] = coef * float((w * (sg + A[i])).max()) / (A[i] * max(n_valid, 1.0))
    return res


def bpr_edge_rows(A, rel=BPR_EDGE_REL):
    """Rows whose float64 A lies within ``rel`` of a clamp edge of interestBPR (A in 1e-8 or 1 - A in 1e-8, relative)."""
    A = np.asarray(A, dtype=np.float64)
    lo = np.abs(A - 1e-8) <= rel * 1e-8
    hi = np.abs((1.0 - A) - 1e-8) <= rel * 1e-8
    return np.nan_to_num(lo | hi, nan=False).astype(bool)


def loss_check(k, t, r, scale, family, what=""):
    """Rule of the loss tests: |k - t| <= 4 |r - t| + tau * scale + 2^-149 elementwise (k kernel, t float64 oracle, r float32
    oracle; the |r - t| term only where r is finite; 2^-149: the fp32 grid's floor), and k finite wherever t is.  Returns the
    worst |k - t| / allowance and records it."""
    k = np.asarray(k, dtype=np.float64)
    t = np.asarray(t, dtype=np.float64)
    r = np.asarray(r, dtype=np.float64)
    scale = np.broadcast_to(np.asarray(scale, dtype=np.float64), t.shape)
    tf = np.isfinite(t)
    nonfinite = tf & ~np.isfinite(k)
    assert not nonfinite.any(), "%s %s: non-finite output where float64 is finite at %s (k=%s t=%s)" % (
        family, what, np.argwhere(nonfinite)[:4].tolist(), k[nonfinite][:4], t[nonfinite][:4])
    rt = np.where(np.isfinite(r) & tf, np.abs(r - t), 0.0)
    allow = 4.0 * rt + LOSS_TAU * scale + F32_MIN_SUBNORMAL
    err = np.where(tf, np.abs(k - t), 0.0)
    ratio = np.where(allow > 0, err / np.where(allow > 0, allow, 1.0), np.where(err > 0, np.inf, 0.0))
    worst = float(ratio.max()) if ratio.size else 0.0
    WORST_RATIO[family] = max(WORST_RATIO.get(family, 0.0), worst)
    if worst > 1.0:
        i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        raise AssertionError("%s %s: |k - t| = %.3e > allowance %.3e (ratio %.2f) at %s: k=%r t=%r r=%r scale=%.3e" % (
            family, what, err[i], allow[i], worst, tuple(int(x) for x in i), float(k[i]), float(t[i]), float(r[i]), float(scale[i])))
    return worst


def loss_compare(got, t, r, cfg, what="", skip_rows=None):
    """loss_check on every slot that is computed (the selected losses, mse, mse2), the total and dlogits.  Scales: the sum of
    |terms| of a slot (oracle_loss), sum of |weight| x that for the total, and for a dlogits row its largest |t| (or interestBPR's
    term size on that row, when larger).
    ``got``: dict(slots[9], total, dlogits[B, S]) of the implementation under test; t / r: oracle_loss in float64 / float32.
    BPR rows near a clamp edge are left out of the gradient comparison (returned: their count).  ``skip_rows``: more rows to leave
    out of the gradient comparison."""
    lst = cfg["loss_type_list"]
    live = [i for i, n in enumerate(LOSS_SLOTS) if n in lst or n in ("mse", "mse2")]
    for i in live:
        loss_check(got["slots"][i], t["slots"][i], r["slots"][i], t["slot_scales"][i], "loss:" + LOSS_SLOTS[i], what)
    loss_check(got["total"], t["total"], r["total"], t["total_scale"], "total", what)
    keep = np.ones(t["dlogits"].shape[0], dtype=bool)
    n_edge = 0
    if "interestBPR" in lst:
        edge = bpr_edge_rows(t["A"])
        n_edge = int(edge.sum())
        keep &= ~edge
    if skip_rows is not None:
        keep &= ~np.asarray(skip_rows, dtype=bool)
    # The scale of a gradient element is the largest of: the row's largest |t| (the issue's rule), the size of the cancelling
    # terms of interestBPR / interestCE / interestKL on the row, and the survival-term size of the element (oracle_loss).  The
    # last two depart from "max |t| over the row"; elements where one of them decides are reported as families of their own.
    B, S = t["dlogits"].shape
    tmax = np.broadcast_to(np.abs(t["dlogits"]).max(1, initial=0.0)[:, None], (B, S))
    term = np.broadcast_to(np.maximum(t["bpr_term"], t["grad_term"])[:, None], (B, S))
    surv = t["surv_term"]
    scale = np.maximum(np.maximum(tmax, term), surv)
    fam = np.where(scale == tmax, 0, np.where(scale == term, 1, 2))
    kd = np.asarray(got["dlogits"], dtype=np.float64)
    sel = keep[:, None] & np.ones((B, S), dtype=bool)
    for f, name in enumerate(("dlogits", "dlogits:interest_term", "dlogits:survival_term")):
        e = sel & (fam == f)
        if e.any():
            loss_check(kd[e], t["dlogits"][e], r["dlogits"][e], scale[e], name, what)
    return n_edge


def all_label_rows(S):
    """Every in-domain label row of synth.make_labels' semantics at S: durations 1 .. S, leave index v in [0, dur) (1 before it,
    0 at it, -1 after, -2 padding) and v = dur for a fully watched row (all 1): sum over dur of (dur + 1) rows (860 at S = 40)."""
    rows = []
    for dur in range(1, S + 1):
        for v in range(dur + 1):
            r = [-2] * S
            for j in range(dur):
                r[j] = 1 if (j < v or v == dur) else (0 if j == v else -1)
            rows.append(r)
    return torch.tensor(rows, dtype=torch.int64)


LOGIT_REGIMES = ("init", "trained", "saturated", "extreme", "ties")


def make_logits(regime, B, S, seed):
    """init N(0, 0.1); trained N(0, 4); saturated +-U(15, 40); extreme: +-U(88, 120) on half the entries, N(0, 4) elsewhere (fp32
    sigmoid underflows to 0 below about -88, softmax tails vanish); ties: one N(0, 4) value per row."""
    g = torch.Generator().manual_seed(seed)
    sign = torch.where(torch.rand(B, S, generator=g) < 0.5, -1.0, 1.0)
    if regime == "init":
        return 0.1 * torch.randn(B, S, generator=g)
    if regime == "trained":
        return 4.0 * torch.randn(B, S, generator=g)
    if regime == "saturated":
        return sign * (15 + 25 * torch.rand(B, S, generator=g))
    if regime == "extreme":
        big = sign * (88 + 32 * torch.rand(B, S, generator=g))
        return torch.where(torch.rand(B, S, generator=g) < 0.5, big, 4.0 * torch.randn(B, S, generator=g))
    if regime == "ties":
        return (4.0 * torch.randn(B, 1, generator=g)).expand(B, S).contiguous()
    raise ValueError(regime)
