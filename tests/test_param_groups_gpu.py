"""Parameter groups of FusedAdamW on the MI355X: segmm_adamw_groups bit for bit against per-segment segmm_adamw launches, frozen
segments untouched, the grouped norm against float64, and the trainer with groups -- against torch.optim.AdamW with the same
groups, with an id table, recorded / scheduled / resumed, data parallel and micro-batched."""
import copy
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import adamw_ref as A
from helpers import ROOT, build_model, load_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32


def _H():
    from segmminterest_amd import hipabi as H
    H.lib()
    return H


def _f32mul(a, b):
    return float(F(a) * F(b))


# ------------------------------------------------------------------------------------------------ segment tables of the kernel tests
def _segments(n, last_frozen=True):
    """Nine segments over n floats: (ends, lr_scale, weight_decay, frozen).  Two are 4 floats long, one frozen at the front, one in
    the middle, one at the end (``last_frozen=False``: the end segment -- the one that owns the n % 4 tail -- steps instead);
    scales {1, 0, 0.1, 3}, decays {0, 1e-2, 0.1}; every interior end a multiple of 4, most of them inside a wave's 256 floats."""
    q = lambda f: int(n * f) // 4 * 4
    ends = [q(0.07), q(0.25), q(0.25) + 4, q(0.45), q(0.6), q(0.6) + 4, q(0.75), q(0.9), n]
    scale = [1.0, 1.0, 0.0, 0.1, 3.0, 3.0, 3.0, 0.1, 1.0]
    wd = [0.1, 1e-2, 0.0, 0.1, 0.0, 1e-2, 0.0, 1e-2, 0.1]
    frozen = [1, 0, 0, 0, 1, 0, 0, 0, 1 if last_frozen else 0]
    assert len(ends) == 9 and ends == sorted(set(ends)) and all(e % 4 == 0 for e in ends[:-1])
    return ends, scale, wd, frozen


def _table(seg):
    ends, scale, wd, frozen = seg
    return (torch.tensor(ends, dtype=torch.int64, device=DEV), torch.tensor(scale, dtype=torch.float32, device=DEV),
            torch.tensor(wd, dtype=torch.float32, device=DEV), torch.tensor(frozen, dtype=torch.uint8, device=DEV))


def _bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _start_state(r, n, seed):
    """p, m, v to start from: the regime's, or (m0 = v0 = None) small non-zero moments so that frozen segments hold something."""
    rng = np.random.default_rng(seed)
    p = torch.from_numpy(np.array(r["p0"]))
    m = torch.from_numpy(np.array(r["m0"]) if r["m0"] is not None else (1e-3 * rng.standard_normal(n)).astype(F))
    v = torch.from_numpy(np.array(r["v0"]) if r["v0"] is not None else (1e-6 * rng.random(n)).astype(F))
    return [t.to(DEV) for t in (p, m, v)]


@pytest.fixture
def step_state():
    """A zeroed device step state of the test's own, bound for the test; the library's default state is bound again afterwards."""
    H = _H()
    state = torch.zeros((H.step_state_bytes() + 3) // 4, dtype=torch.int32, device=DEV)
    H.step_bind(state)
    try:
        yield state
    finally:
        torch.cuda.synchronize()
        H.step_bind(None)


# ------------------------------------------------------------------------------------------------ 1. the kernel, bitwise
@pytest.mark.parametrize("live", [False, True], ids=["by_value", "live_lr"])
@pytest.mark.parametrize("n", [4099, 70001])
def test_adamw_groups_equals_per_segment_launches_bitwise(n, live, step_state):
    """Three consecutive steps of segmm_adamw_groups (one launch, and three sub-range launches whose cuts lie inside segments)
    against one segmm_adamw / segmm_adamw_scaled launch per non-frozen segment with lr = fp32(lr * scale) by value and the
    segment's decay: p, m, v equal as int32.  By-value rate with step >= 1, and the live path (SEGMM_LIVE_LR, step = -1) under a
    cosine schedule, where the comparison launches take fp32(device_lr * scale) by value and step = -1."""
    H = _H()
    for regime, last_frozen, with_coef in (("unit", True, False), ("decay", True, True), ("decades", False, True), ("decay", False, False)):
        r = A.regime(regime, n=n, T=3, seed=3)
        hp = r["hp"]
        seg = _segments(n, last_frozen)
        ends, scale, wd, frozen = seg
        tab = _table(seg)
        coef = torch.tensor([0.3712345], dtype=torch.float32, device=DEV) if with_coef else None
        cuts = [0, (ends[1] + ends[3]) // 2 // 4 * 4, (ends[6] + ends[7]) // 2 // 4 * 4, n]          # inside segments 3 and 7
        assert all(c % 4 == 0 and c not in ends for c in cuts[1:-1])
        one, ref, cut = (_start_state(r, n, 17) for _ in range(3))
        if live:
            H.step_set(12345, r["t0"], hp["b1"], hp["b2"])
            H.step_schedule("cosine", hp["lr"], warmup_steps=1, start_factor=0.5, decay_steps=4, eta_min=0.1 * hp["lr"])
        rates = []
        for k, g in enumerate(r["grads"]):
            g = torch.from_numpy(np.array(g)).to(DEV)
            if live:
                H.step_advance(hp["b1"], hp["b2"])
                lr, lr_arg, step = H.step_get_lr()[0], H.LIVE_LR, -1
            else:
                lr = lr_arg = hp["lr"]
                step = r["t0"] + k + 1
            rates.append(lr)
            H.adamw_groups(*one[:1], g, *one[1:], 0, n, tab, lr_arg, hp["b1"], hp["b2"], hp["eps"], step, coef=coef)
            for a, b in zip(cuts, cuts[1:]):
                H.adamw_groups(*cut[:1], g, *cut[1:], a, b - a, tab, lr_arg, hp["b1"], hp["b2"], hp["eps"], step, coef=coef)
            for s0, s1, sc, w, fz in zip([0] + ends[:-1], ends, scale, wd, frozen):
                if not fz:
                    H.adamw(ref[0], g, ref[1], ref[2], s1 - s0, _f32mul(lr, sc), hp["b1"], hp["b2"], hp["eps"], w, step, p_off=s0, coef=coef)
            torch.cuda.synchronize()
            for name, x, y, z in zip("pmv", one, ref, cut):
                assert _bits_equal(x, y), (regime, n, k, name, "one launch")
                assert _bits_equal(z, y), (regime, n, k, name, "three sub-range launches")
        if live:
            assert len(set(rates)) == 3 and all(x > 0 for x in rates), rates          # the schedule moved under the launches
        start = _start_state(r, n, 17)
        assert not _bits_equal(one[0], start[0]) and not _bits_equal(one[2], start[2])          # the steps did something


def test_one_segment_of_scale_one_is_segmm_adamw_bitwise():
    """One segment, scale 1: segmm_adamw_groups is segmm_adamw, and with a coefficient segmm_adamw_scaled."""
    H = _H()
    n = 70001
    r = A.regime("decay", n=n, T=3, seed=3)
    hp = r["hp"]
    tab = _table(([n], [1.0], [hp["wd"]], [0]))
    for coef in (None, torch.tensor([0.3712345], dtype=torch.float32, device=DEV)):
        a, b = _start_state(r, n, 5), _start_state(r, n, 5)
        for k, g in enumerate(r["grads"]):
            g = torch.from_numpy(np.array(g)).to(DEV)
            H.adamw_groups(a[0], g, a[1], a[2], 0, n, tab, hp["lr"], hp["b1"], hp["b2"], hp["eps"], k + 1, coef=coef)
            H.adamw(b[0], g, b[1], b[2], n, hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"], k + 1, coef=coef)
        assert all(_bits_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("n", [4099, 70001])
def test_no_frozen_flags_equal_all_zero_flags_bitwise(n):
    """seg_frozen == NULL (no segment is frozen: the kernel loads its elements without waiting for the table) against the same table
    with all-zero flags and against the per-segment launches, whole range and three sub-ranges, three steps, with a coefficient."""
    H = _H()
    r = A.regime("decay", n=n, T=3, seed=3)
    hp = r["hp"]
    ends, scale, wd, _ = _segments(n)
    tab = _table((ends, scale, wd, [0] * 9))
    bare = tab[:3] + (None,)
    coef = torch.tensor([0.3712345], dtype=torch.float32, device=DEV)
    cuts = [0, (ends[1] + ends[3]) // 2 // 4 * 4, (ends[6] + ends[7]) // 2 // 4 * 4, n]
    flagged, none, cut, ref = (_start_state(r, n, 17) for _ in range(4))
    for k, g in enumerate(r["grads"]):
        g = torch.from_numpy(np.array(g)).to(DEV)
        H.adamw_groups(flagged[0], g, flagged[1], flagged[2], 0, n, tab, hp["lr"], hp["b1"], hp["b2"], hp["eps"], k + 1, coef=coef)
        H.adamw_groups(none[0], g, none[1], none[2], 0, n, bare, hp["lr"], hp["b1"], hp["b2"], hp["eps"], k + 1, coef=coef)
        for a, b in zip(cuts, cuts[1:]):
            H.adamw_groups(cut[0], g, cut[1], cut[2], a, b - a, bare, hp["lr"], hp["b1"], hp["b2"], hp["eps"], k + 1, coef=coef)
        for s0, s1, sc, w in zip([0] + ends[:-1], ends, scale, wd):
            H.adamw(ref[0], g, ref[1], ref[2], s1 - s0, _f32mul(hp["lr"], sc), hp["b1"], hp["b2"], hp["eps"], w, k + 1, p_off=s0, coef=coef)
        for x, y, z, w_ in zip(flagged, none, cut, ref):
            assert _bits_equal(x, w_) and _bits_equal(y, w_) and _bits_equal(z, w_), (n, k)


# ------------------------------------------------------------------------------------------------ 2. frozen means untouched
@pytest.mark.parametrize("n", [4099, 70001])
def test_frozen_segments_are_untouched_and_stay_out_of_the_norm(n):
    """NaN and inf gradients planted in the frozen segments: p, m, v there are byte-identical before and after the step, the
    other segments move, and the norm and coefficient of segmm_grad_norm_groups are finite -- those of the non-frozen elements."""
    H = _H()
    seg = _segments(n)
    ends, _, _, frozen = seg
    tab = _table(seg)
    gen = torch.Generator().manual_seed(2)
    p0, g, m0 = (torch.randn(n, generator=gen) for _ in range(3))
    v0 = torch.rand(n, generator=gen) * 1e-3
    mask = torch.zeros(n, dtype=torch.bool)
    for s0, s1, fz in zip([0] + ends[:-1], ends, frozen):
        if fz:
            mask[s0:s1] = True
            g[s0:s1:3] = math.nan
            g[s0 + 1:s1:3] = math.inf
            g[s0 + 2:s1:3] = -math.inf
    assert mask[0] and mask[-1] and mask.sum() > 0.2 * n
    scratch = torch.zeros(H.GRAD_NORM_SCRATCH, dtype=torch.float64, device=DEV)
    out2 = torch.zeros(2, dtype=torch.float32, device=DEV)
    gd = g.to(DEV)
    H.grad_norm_groups(gd, n, tab, 1.0, scratch, out2)
    norm, coef = (float(x) for x in out2.cpu())
    ref = float(torch.linalg.vector_norm(g[~mask].double()))
    assert math.isfinite(norm) and math.isfinite(coef) and abs(norm - ref) <= 2.0 ** -22 * ref and 0.0 < coef < 1.0
    p, m, v = (t.to(DEV) for t in (p0, m0, v0))
    H.adamw_groups(p, gd, m, v, 0, n, tab, 1e-3, 0.9, 0.999, 1e-8, 1, coef=out2[1:2])
    md = mask.to(DEV)
    for x, x0 in ((p, p0), (m, m0), (v, v0)):
        x0 = x0.to(DEV)
        assert _bits_equal(x[md], x0[md])
        assert bool(torch.isfinite(x).all())
    # every other element moved (but the 4 floats at scale 0 and decay 0, whose p stays)
    assert bool((m[~md] != m0.to(DEV)[~md]).all()) and int((p[~md] == p0.to(DEV)[~md]).sum()) <= 4


# ------------------------------------------------------------------------------------------------ 3. the norm
@pytest.mark.parametrize("kind", ["randn", "tiny", "huge"])
def test_grad_norm_groups_vs_float64(kind):
    """segmm_grad_norm_groups: the 2-norm of the non-frozen elements to 2^-22 relative of the float64 norm (the bound and the data
    of test_clip_gpu.py::test_grad_norm_kernel_vs_float64), equal bits on a second run, the coefficient bit-equal to torch's clamp
    expression on the returned norm; without a frozen segment it is segmm_grad_norm bit for bit."""
    H = _H()
    scratch = torch.zeros(H.GRAD_NORM_SCRATCH, dtype=torch.float64, device=DEV)
    out2 = torch.zeros(2, dtype=torch.float32, device=DEV)
    gen = torch.Generator().manual_seed(7)
    for n in (3, 4099, 70001, 1_000_003):
        x = torch.randn(n, generator=gen)
        x = {"randn": x, "tiny": x * 1e-20, "huge": x * 1e19}[kind]
        xd = x.to(DEV)
        if n == 3:
            segs = [([n], [1.0], [0.0], [0])]
        else:
            segs = [_segments(n), _segments(n, last_frozen=False), ([n], [1.0], [0.0], [0])]
        for seg in segs:
            ends, _, _, frozen = seg
            keep = torch.ones(n, dtype=torch.bool)
            for s0, s1, fz in zip([0] + ends[:-1], ends, frozen):
                if fz:
                    keep[s0:s1] = False
            ref = float(torch.linalg.vector_norm(x[keep].double()))
            tab = _table(seg)
            for m in (0.5 * ref, 1.0, math.inf):
                H.grad_norm_groups(xd, n, tab, m, scratch, out2)
                first = out2.cpu().clone()
                scratch.fill_(float("nan"))
                H.grad_norm_groups(xd, n, tab, m, scratch, out2)
                assert _bits_equal(first, out2.cpu()), (n, m)
                t, c = float(first[0]), first[1]
                assert abs(t - ref) <= 2.0 ** -22 * ref, (n, t, ref)
                want = torch.tensor(1.0) if m == math.inf else torch.clamp(m / (torch.tensor(t, dtype=torch.float32) + 1e-6), max=1.0)
                assert _bits_equal(c.reshape(1), want.reshape(1)), (n, m, float(c), float(want))
                if not any(frozen):
                    H.grad_norm(xd, n, m, scratch, out2)
                    assert abs(float(out2[0]) - t) <= 2.0 ** -22 * ref


# ------------------------------------------------------------------------------------------------ the trainer
def _cfg(name, S=8, Lt=4):
    cfg, g, _, _ = load_case(name)
    return dict(cfg, S=S, Lt=min(Lt, cfg["Lt"]), exposure_prob=list(cfg["exposure_prob"])[:S])


def _batches(cfg, n=3, B=4, dev=DEV):
    from segmminterest_amd.synth import make_batch
    out = [make_batch(B, cfg["S"], cfg["Lt"], cfg["D_in"], n_users=cfg.get("n_users", 5) or 5, n_items=cfg.get("n_items", 5) or 5, seed=500 + i)
           for i in range(n)]
    return out if dev is None else [{k: v.to(dev) for k, v in b.items()} for b in out]


def _trainer(cfg, groups=None, **kw):
    """``groups``: a callable model -> param_groups (the recipes need the model's names)."""
    from segmminterest_amd.trainer import Trainer
    torch.manual_seed(5)
    model = build_model(cfg).to(DEV)
    kw.setdefault("dropout", False)
    if groups is not None:
        kw["param_groups"] = groups(model)
    return Trainer(model, **kw)


def _snap(tr):
    torch.cuda.synchronize()
    return tuple(x.detach().clone() for x in (tr.model._store.flat, tr.opt.m, tr.opt.v))


def _equal(a, b):
    return all(_bits_equal(x, y) for x, y in zip(a, b))


def _groups(model, head_scale=0.1):
    """The recipe of the trainer tests: no_decay_groups plus the head's weight matrices (everything outside the backbones whose
    name ends in .weight: stage_mlp1 / the fusion module's projections) at ``lr_scale``."""
    from segmminterest_amd.trainer import no_decay_groups
    head = [n for n, _ in model.named_parameters() if not n.startswith("backbone") and n.endswith(".weight")]
    assert head
    return no_decay_groups(model) + [{"params": head, "lr_scale": head_scale}]


# ------------------------------------------------------------------------------------------------ 4. one segment of scale 1 == today
def test_empty_group_list_equals_no_groups_bitwise():
    cfg = _cfg("img_d32_N2")
    batches = _batches(cfg)
    snaps = []
    for pg in (None, []):
        tr = _trainer(cfg, param_groups=pg)
        for t in range(3):
            tr.train_step(batches[t])
        snaps.append(_snap(tr))
        if pg is not None:
            assert tr.opt._segs_host == [(tr.model._store.n_live, 1.0, float(F(1e-4)), False)]
    assert _equal(*snaps)


# ------------------------------------------------------------------------------------------------ 5. against torch.optim.AdamW
@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("case", ["img_d32_N2", "both_fh2"])
def test_trainer_matches_torch_adamw_with_the_same_groups(case, clip):
    """5 train_steps with no_decay_groups + the head at lr_scale 0.1 (both_fh2: also backbone2.* frozen) against torch.optim.AdamW on
    the CPU in fp32, built with the same groups and fed the gradients the GPU step left in .grad; with ``max_grad_norm`` torch clips
    them first with clip_grad_norm_ over the non-frozen parameters.  Per element |p - p_ref| <= steps * (2^-20 |p_ref| + 1e-5 lr_group),
    the rule of test_fused_adamw_clip_matches_torch_clip_and_adamw with the group's own rate.  Frozen parameters keep their initial
    bits and have no entry in state_dict()["state"]."""
    lr, wd, steps = 1e-3, 1e-2, 5
    cfg = _cfg(case)
    batches = _batches(cfg)
    freeze = case == "both_fh2"

    def groups(model):
        pg = _groups(model)
        if freeze:
            pg[0]["params"] = [n for n in pg[0]["params"] if not n.startswith("backbone2.")]
            pg.append({"params": lambda n, p: n.startswith("backbone2."), "frozen": True})
        return pg

    max_norm = None
    if clip:          # 1 % of the first step's norm (the norm falls tenfold over these 5 steps: the clip stays active)
        probe = _trainer(cfg, groups, lr=lr, weight_decay=wd, max_grad_norm=math.inf)
        probe.train_step(batches[1])
        max_norm = 0.01 * float(probe.opt.grad_norm)
        assert max_norm > 0
    tr = _trainer(cfg, groups, lr=lr, weight_decay=wd, max_grad_norm=max_norm)
    model, opt = tr.model, tr.opt
    init = {k: p.detach().cpu().clone() for k, p in model.named_parameters()}
    frozen = [k for k in init if opt.group_of(k)[2]]
    assert bool(frozen) == freeze
    ref = {k: torch.nn.Parameter(v.clone()) for k, v in init.items() if k not in frozen}
    tgroups = [dict(params=[ref[k] for k in G["names"]], lr=_f32mul(lr, G["lr_scale"]) if G["lr_scale"] != 1.0 else lr,
                    weight_decay=G["weight_decay"]) for G in opt.groups if not G["frozen"]]
    topt = torch.optim.AdamW(tgroups, lr=lr, betas=opt.betas, eps=opt.eps, foreach=False)
    rate = {k: tg["lr"] for tg, G in zip(tgroups, [G for G in opt.groups if not G["frozen"]]) for k in G["names"]}
    assert len({(tg["lr"], tg["weight_decay"]) for tg in tgroups}) == 3
    for step in range(1, steps + 1):
        tr.train_step(batches[step % 3])
        torch.cuda.synchronize()
        live = [k for k, p in model.named_parameters() if p.grad is not None]
        for k, p in model.named_parameters():
            if k in ref:
                ref[k].grad = p.grad.detach().cpu().clone() if p.grad is not None else None
        if clip:
            tn = float(torch.nn.utils.clip_grad_norm_([ref[k] for k in live if k in ref], max_norm))
            got = float(opt.grad_norm)
            print("step %d: norm %.6g (torch %.6g), max_norm %.6g" % (step, got, tn, max_norm))
            assert abs(got - tn) <= 2.0 ** -20 * tn, (step, got, tn)
            assert step > 1 or tn > max_norm          # the clip is active
        topt.step()
        for k, p in model.named_parameters():
            got = p.detach().cpu()
            if k in frozen or k not in live:
                assert _bits_equal(got, init[k]), (step, k)
                continue
            want = ref[k].detach()
            err = (got.double() - want.double()).abs()
            lim = step * (2.0 ** -20 * want.double().abs() + 1e-5 * rate[k])
            assert bool((err <= lim).all()), (step, k, float((err - lim).max()))
    moved = [k for k in ref if k in live and not torch.equal(ref[k].detach(), init[k])]
    assert len(moved) > 10
    names = [k for k, _ in model.named_parameters()]
    sd = opt.state_dict()
    assert not any(names[i] in frozen for i in sd["state"]) and len(sd["state"]) == len([k for k in live if k not in frozen])
    if freeze:
        assert any(model.get_parameter(k).grad is not None for k in frozen)          # the backward still delivers their gradients


# ------------------------------------------------------------------------------------------------ 6. an id table in a group
TABLE = "backbone1.vid_proj.weight"


def _id_run(two_pass, frozen, q=None):
    """3 steps of the id-mode model with the item table in a group of its own; -> (flat, m, v) as numpy (and into ``q``)."""
    os.environ["SEGMM_TABLE_TWO_PASS"] = "1" if two_pass else "0"
    sys.path.insert(0, ROOT)
    cfg = _cfg("id_d32_N2")
    batches = _batches(cfg)
    group = {"params": [TABLE], "frozen": True} if frozen else {"params": [TABLE], "lr_scale": 0.1, "weight_decay": 0.0}
    tr = _trainer(cfg, lr=1e-3, weight_decay=1e-2, param_groups=[group])
    assert tr.table_two_pass == two_pass
    t0 = tr.model.get_parameter(TABLE).detach().cpu().clone()
    for t in range(3):
        tr.train_step(batches[t])
    torch.cuda.synchronize()
    flags = tr.opt.__dict__.get("_table_flags", {})
    if two_pass and not frozen:
        assert flags and all(int(f.abs().sum()) == 0 for f in flags.values())
    if frozen:          # no pass ever ran on the table: nothing was marked, nothing moved, no state
        assert all(int(f.abs().sum()) == 0 for f in flags.values()) and not tr.opt.__dict__.get("_early")
        assert _bits_equal(tr.model.get_parameter(TABLE).detach().cpu(), t0)
        o, k = tr.model._store.index[TABLE]
        assert not bool(tr.opt.m[o:o + k].any()) and not bool(tr.opt.v[o:o + k].any())
        assert bool(tr.model._store.gflat[o:o + k].any())          # (its gradient was delivered)
    else:
        assert not _bits_equal(tr.model.get_parameter(TABLE).detach().cpu(), t0)
    res = tuple(x.cpu().numpy() for x in _snap(tr))
    if q is not None:
        q.put(res)
    return res


def _child(target, *args, timeout=240):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=target, args=args + (q,))
    p.start()
    res = q.get(timeout=timeout)
    p.join(60)
    assert p.exitcode == 0
    return res


def test_id_table_group_two_pass_equals_dense_bitwise():
    """The item table at lr_scale 0.1, weight decay 0: the two-pass update (segmm_adamw_table_lrs, both phases) equals the one-launch
    dense update (SEGMM_TABLE_TWO_PASS=0, read when the process starts its trainer: a child process) bit for bit."""
    two = _id_run(True, False)
    os.environ.pop("SEGMM_TABLE_TWO_PASS", None)
    dense = _child(_id_run, False, False)
    for a, b in zip(two, dense):
        assert (a.view(np.int32) == b.view(np.int32)).all()


def test_frozen_id_table_is_untouched():
    try:
        _id_run(True, True)
    finally:
        os.environ.pop("SEGMM_TABLE_TWO_PASS", None)


# ------------------------------------------------------------------------------------------------ 7. recorded, scheduled, resumed
SCHED = dict(kind="cosine", warmup_steps=2, decay_steps=8, eta_min=1e-4)


def test_recorded_scheduled_resumed_with_groups():
    """Trainer(device_state=True, lr_schedule="cosine", param_groups=...): record() + run_recorded() equals the eager steps bitwise
    over 4 steps; after set_base_lr the groups' rates follow without re-recording; state_dict -> fresh trainer -> load_state_dict
    -> 2 more steps equals the uninterrupted run bitwise; another grouping is refused by name."""
    cfg = _cfg("img_d32_N2")
    batches = _batches(cfg)

    def make(groups=_groups):
        return _trainer(cfg, groups, lr=1e-3, weight_decay=1e-2, device_state=True, lr_schedule=SCHED)

    def run(tr, first, last, recorded_from=None, halve_at=None):
        for t in range(first, last + 1):
            b = batches[(t - 1) % 3]
            if halve_at == t:
                tr.opt.set_base_lr(5e-4)
            if recorded_from is None or t < recorded_from:
                tr.train_step(b)
            elif t == recorded_from:
                tr.record(b, warmup=0, prev_batch=batches[(t - 2) % 3])
            else:
                tr.run_recorded(b)

    eager, rec = make(), make()
    run(eager, 1, 6, halve_at=6)
    run(rec, 1, 6, recorded_from=2, halve_at=6)          # steps 3..6 replayed, the last one under the halved base rate
    assert _equal(_snap(eager), _snap(rec))
    stay = make()
    run(stay, 1, 6)
    assert not _equal(_snap(stay), _snap(eager))          # the halved rate was used
    sd = rec.opt.state_dict()
    base, nxt = 5e-4, rec.opt.current_lr()
    assert [g["lr"] for g in sd["param_groups"]] == [nxt, nxt, _f32mul(nxt, 0.1)]
    assert [g["initial_lr"] for g in sd["param_groups"]] == [base, base, _f32mul(base, 0.1)]
    # a changed group table is a changed hyperparameter: the recording is refused
    rec.opt.groups[2]["lr_scale"] = 0.5
    with pytest.raises(RuntimeError, match="record\\(\\) again"):
        rec.run_recorded(batches[0])
    # resume
    whole = make()
    run(whole, 1, 6)
    first = make()
    run(first, 1, 4)
    torch.cuda.synchronize()
    sd_model = {k: v.detach().cpu().clone() for k, v in first.model.state_dict().items()}
    sd_opt = copy.deepcopy(first.opt.state_dict())
    second = make(lambda m: [{"params": no_decay_names(m), "weight_decay": 0.5}, {"params": ["stage_mlp*.weight"], "lr_scale": 7.0}])
    second.model.load_state_dict(sd_model)
    second.opt.load_state_dict(sd_opt)
    assert second.opt.group_table() == first.opt.group_table() and second.opt.step_count == 4
    run(second, 5, 6)
    assert _equal(_snap(whole), _snap(second))
    other = make(lambda m: [{"params": ["stage_mlp*.weight"], "lr_scale": 0.1}])
    with pytest.raises(ValueError, match=r"load_state_dict: .*parameter backbone1\.\S+"):
        other.opt.load_state_dict(sd_opt)
    # torch.optim.AdamW with the same index groups takes the dict
    plist = list(first.model.parameters())
    topt = torch.optim.AdamW([{"params": [plist[i] for i in g["params"]]} for g in sd_opt["param_groups"]], lr=0.5)
    topt.load_state_dict(copy.deepcopy(sd_opt))
    assert [g["lr"] for g in topt.param_groups] == [g["lr"] for g in sd_opt["param_groups"]]


def no_decay_names(model):
    from segmminterest_amd.trainer import no_decay_groups
    return no_decay_groups(model)[0]["params"]


# ------------------------------------------------------------------------------------------------ 8. data parallel, micro-batches
def _run_dp(rank, world, port, q):
    """world = 1: the grouped step on 8 rows in one process; world = 2: gloo ranks sharing the GPU, 4 rows each."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from segmminterest_amd.trainer import DPComm, Trainer, shard_rows
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        cfg = _cfg("img_d32_N2")
        torch.manual_seed(5)
        model = build_model(cfg).cuda()
        tr = Trainer(model, lr=1e-3, weight_decay=1e-2, comm=DPComm(), overlap=True, dropout=False, param_groups=_groups(model))
        assert tr.comm.active == (world > 1)
        s, e = shard_rows(8, world, rank)
        shards = [{k: v[s:e].contiguous().cuda() for k, v in b.items()} for b in _batches(cfg, n=2, B=8, dev=None)]
        for t in range(2):
            tr.train_step(shards[t])
        torch.cuda.synchronize()
        q.put((rank, model._store.flat.detach().cpu().numpy(), {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}))
    finally:
        if world > 1:
            dist.destroy_process_group()


def _spawn(world, port):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_run_dp, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(world):
        r = q.get(timeout=240)
        res[r[0]] = r[1:]
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    return res


def test_two_ranks_grouped_step():
    """Two gloo ranks sharing the GPU, the per-bucket grouped step (sub-range launches that cut segments): parameters bitwise equal
    across ranks, and against the single-process run on the whole batch within test_micro_batch_gpu.py's tolerance."""
    base = 29700 + os.getpid() % 200
    single, two = _spawn(1, base), _spawn(2, base + 1)
    assert (two[0][0].view(np.int32) == two[1][0].view(np.int32)).all()
    for k in single[0][1]:
        assert torch.allclose(torch.from_numpy(single[0][1][k]), torch.from_numpy(two[0][1][k]), rtol=1e-4, atol=4.5e-3), k
    # the groups were in force: against the same two steps without groups the parameters differ
    cfg = _cfg("img_d32_N2")
    tr = _trainer(cfg, lr=1e-3, weight_decay=1e-2)
    for b in _batches(cfg, n=2, B=8):
        tr.train_step(b)
    torch.cuda.synchronize()
    assert not np.array_equal(tr.model._store.flat.detach().cpu().numpy(), single[0][0])


def test_micro_batched_grouped_step_recorded_equals_eager():
    """micro_batch=2 on B = 4 with groups: the recorded step equals the eager one bitwise."""
    cfg = _cfg("img_d32_N2")
    batches = _batches(cfg)
    snaps = []
    for recorded in (False, True):
        torch.manual_seed(5)
        model = build_model(cfg).to(DEV)
        from segmminterest_amd.trainer import Trainer
        tr = Trainer(model, lr=1e-3, weight_decay=1e-2, dropout=False, device_state=True, micro_batch=2, max_grad_norm=1e-4,
                     param_groups=_groups(model))
        if recorded:
            tr.record(batches[0], warmup=1)
        else:
            for _ in range(2):
                tr.train_step(batches[0])
        for t in range(3):
            (tr.run_recorded if recorded else tr.train_step)(batches[t])
        snaps.append(_snap(tr))
    assert _equal(*snaps)
