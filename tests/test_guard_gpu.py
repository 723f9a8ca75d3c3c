"""The non-finite guard on the MI355X: the guarded kernels through the C ABI, and Trainer(skip_nonfinite=True) eager, recorded,
micro-batched, with parameter groups and on two data-parallel ranks.  Every comparison is one of bits (int32 views): an applied
step under the guard is the unguarded step, a skipped step is the identity.

The reference of an applied step is tests/guard_ref.py (adamw_ref.emul32 with the bias corrections of the applied index)."""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import guard_ref as G
from helpers import ROOT, build_model, load_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
B1, B2, EPS, WD, LR = 0.9, 0.999, 1e-8, 1e-2, 1e-3
HP = (B1, B2, EPS)


def _H():
    from segmminterest_amd import hipabi as H
    H.lib()
    return H


def _i32(t):
    return t.detach().contiguous().view(torch.int32)


def _same(a, b):
    return bool((_i32(a) == _i32(b)).all())


@pytest.fixture
def state():
    """A step state of the test's own at step 1 of a guarded run, bound for the test; the library's default state is bound again
    afterwards."""
    H = _H()
    st = torch.zeros((H.step_state_bytes() + 3) // 4, dtype=torch.int32, device=DEV)
    H.step_bind(st)
    H.step_set(1234, 0, B1, B2)
    H.step_advance_guarded(B1, B2)
    try:
        yield st
    finally:
        torch.cuda.synchronize()
        H.step_bind(None)


def _rand(n, seed, scale=1.0, positive=False):
    g = torch.Generator().manual_seed(seed)
    t = torch.rand(n, generator=g) + 0.25 if positive else torch.randn(n, generator=g)
    return (scale * t).to(DEV)


def _pmv(n, seed):
    return [_rand(n, seed, 0.05), _rand(n, seed + 1, 0.1), _rand(n, seed + 2, 0.01, positive=True)]


class _Norm:
    """segmm_grad_norm + segmm_step_guard on a gradient: the verdict as the step makes it."""

    def __init__(self):
        self.H = _H()
        self.out2 = torch.zeros(2, device=DEV)
        self.scratch = torch.zeros(self.H.GRAD_NORM_SCRATCH, dtype=torch.float64, device=DEV)

    def __call__(self, g, n, max_norm=math.inf, segs=None):
        if segs is None:
            self.H.grad_norm(g, n, max_norm, self.scratch, self.out2)
        else:
            self.H.grad_norm_groups(g, n, segs, max_norm, self.scratch, self.out2)
        self.H.step_guard(self.out2)
        return self.H.step_get_skipped()


# ------------------------------------------------------------------------------------------------ 1. the kernels through the C ABI
@pytest.mark.parametrize("n", [1027, 70_003])
@pytest.mark.parametrize("clip", [False, True], ids=["plain", "coef"])
def test_flat_adamw_guarded(n, clip, state):
    """Finite norm: the bits of segmm_adamw / segmm_adamw_scaled on the same inputs.  One NaN, then one +inf, written into g: p, m, v
    keep every bit, skip = 1, skipped counts.  n = 1027: one workgroup and an n % 4 tail; 70 003: several workgroups."""
    H, norm = _H(), _Norm()
    a, g = _pmv(n, n), _rand(n, n + 7)
    b = [t.clone() for t in a]
    assert norm(g, n, 0.5 if clip else math.inf) == (0, 0)
    coef = norm.out2[1:2] if clip else None
    assert not clip or 0.0 < float(coef) < 1.0
    H.adamw(a[0], g, a[1], a[2], n, LR, *HP, WD, -1, coef=coef, guard=True)
    H.adamw(b[0], g, b[1], b[2], n, LR, *HP, WD, -1, coef=coef)
    assert all(_same(x, y) for x, y in zip(a, b)) and not _same(a[0], _pmv(n, n)[0])
    for k, poison in enumerate((math.nan, math.inf)):
        H.step_advance_guarded(B1, B2)
        assert H.step_get_skipped() == (0, k)          # the head of the step clears the verdict, the count stays
        g[n // 2 + k] = poison
        assert norm(g, n, 0.5 if clip else math.inf) == (1, k + 1)
        H.adamw(a[0], g, a[1], a[2], n, LR, *HP, WD, -1, coef=coef, guard=True)
        torch.cuda.synchronize()
        assert all(_same(x, y) for x, y in zip(a, b)), "a skipped step moved p, m or v"
        g[n // 2 + k] = 0.0
    # the next clean step is applied again
    H.step_advance_guarded(B1, B2)
    assert norm(g, n, 0.5 if clip else math.inf) == (0, 2)
    H.adamw(a[0], g, a[1], a[2], n, LR, *HP, WD, -1, coef=coef, guard=True)
    assert not _same(a[0], b[0])


def test_unguarded_entry_points_do_not_read_the_two_words(state):
    """segmm_adamw with the live state whose two words say "skip": it steps, with the bits it gives over zeroed words."""
    H = _H()
    n = 1027
    a, g = _pmv(n, 5), _rand(n, 6)
    b = [t.clone() for t in a]
    H.adamw(b[0], g, b[1], b[2], n, LR, *HP, WD, -1)
    state[H.STEP_SKIP_WORD] = 1
    state[H.STEP_SKIP_WORD + 1] = -1
    H.adamw(a[0], g, a[1], a[2], n, LR, *HP, WD, -1)
    assert all(_same(x, y) for x, y in zip(a, b)) and not _same(a[0], _pmv(n, 5)[0])


def test_groups_adamw_guarded(state):
    """Three segments over [0, 1027), the middle one frozen, the first end (260) inside a wave's 256 floats of the range."""
    H, norm = _H(), _Norm()
    n = 1027
    segs = (torch.tensor([260, 600, n], dtype=torch.int64, device=DEV), torch.tensor([1.0, 1.0, 0.5], device=DEV),
            torch.tensor([WD, 0.0, 0.0], device=DEV), torch.tensor([0, 1, 0], dtype=torch.uint8, device=DEV))
    a, g = _pmv(n, 21), _rand(n, 22)
    b = [t.clone() for t in a]
    g[300] = math.nan          # frozen: out of the norm, and the element is never loaded
    assert norm(g, n, 0.5, segs) == (0, 0)
    coef = norm.out2[1:2]
    H.adamw_groups(*a[:1], g, *a[1:], 0, n, segs, LR, *HP, -1, coef=coef, guard=True)
    H.adamw_groups(*b[:1], g, *b[1:], 0, n, segs, LR, *HP, -1, coef=coef)
    assert all(_same(x, y) for x, y in zip(a, b))
    assert _same(a[0][260:600], _pmv(n, 21)[0][260:600]) and not _same(a[0][:260], _pmv(n, 21)[0][:260])
    for k, (at, poison) in enumerate(((100, math.nan), (900, math.inf))):
        H.step_advance_guarded(B1, B2)
        g[at] = poison
        assert norm(g, n, 0.5, segs) == (1, k + 1)
        H.adamw_groups(*a[:1], g, *a[1:], 0, n, segs, LR, *HP, -1, coef=coef, guard=True)
        H.adamw_groups(*a[:1], g, *a[1:], 0, n, segs[:3] + (None,), LR, *HP, -1, guard=True)          # (the form without frozen flags)
        torch.cuda.synchronize()
        assert all(_same(x, y) for x, y in zip(a, b)), "a skipped step moved p, m or v"
        g[at] = 0.0


def test_id_table_rows_guarded(state):
    """37 rows x 8, a duplicate id and one out of range: both phases of segmm_adamw_table_lrs_guarded against the unguarded ones;
    a skipped step marks nothing, steps nothing and leaves no mark standing."""
    H, norm = _H(), _Norm()
    rows, width = 37, 8
    n = rows * width
    ids = torch.tensor([3, 5, 5, 36, 37, 0], dtype=torch.int64, device=DEV)
    a, g = _pmv(n, 31), _rand(n, 32)
    b = [t.clone() for t in a]
    fa, fb = (torch.zeros(rows, dtype=torch.int32, device=DEV) for _ in range(2))
    assert norm(g, n, 0.5) == (0, 0)
    coef = norm.out2[1:2]
    for t, f, kw in ((a, fa, dict(guard=True)), (b, fb, {})):
        H.adamw_table_lrs(t[0], None, t[1], t[2], 0, rows, width, ids, f, LR, 0.5, *HP, WD, -1, 0, **kw)
        H.adamw_table_lrs(t[0], g, t[1], t[2], 0, rows, width, ids, f, LR, 0.5, *HP, WD, -1, 1, coef=coef, **kw)
    assert all(_same(x, y) for x, y in zip(a, b)) and int(fa.abs().sum()) == 0 and int(fb.abs().sum()) == 0
    assert not _same(a[0], _pmv(n, 31)[0])
    for k, poison in enumerate((math.nan, math.inf)):
        H.step_advance_guarded(B1, B2)
        g[5 * width + 1] = poison
        assert norm(g, n, 0.5) == (1, k + 1)
        H.adamw_table_lrs(a[0], None, a[1], a[2], 0, rows, width, ids, fa, LR, 0.5, *HP, WD, -1, 0, guard=True)
        torch.cuda.synchronize()
        assert int(fa.abs().sum()) == 0, "a skipped phase 0 marked rows"
        H.adamw_table_lrs(a[0], g, a[1], a[2], 0, rows, width, ids, fa, LR, 0.5, *HP, WD, -1, 1, coef=coef, guard=True)
        torch.cuda.synchronize()
        assert all(_same(x, y) for x, y in zip(a, b)) and int(fa.abs().sum()) == 0
        g[5 * width + 1] = 0.0


@pytest.mark.parametrize("warmup", [False, True])
def test_ema_update_guarded(warmup, state):
    H, norm = _H(), _Norm()
    n = 1027
    sa, p, g = _rand(n, 41), _rand(n, 42), _rand(n, 43)
    sb = sa.clone()
    assert norm(g, n) == (0, 0)
    H.ema_update(sa, p, n, 0.1, warmup, -1, guard=True)
    H.ema_update(sb, p, n, 0.1, warmup, -1)
    assert _same(sa, sb) and not _same(sa, _rand(n, 41))
    for k, poison in enumerate((math.nan, math.inf)):
        H.step_advance_guarded(B1, B2)
        g[k] = poison
        assert norm(g, n) == (1, k + 1)
        H.ema_update(sa, p, n, 0.1, warmup, -1, guard=True)
        torch.cuda.synchronize()
        assert _same(sa, sb), "a skipped step moved the shadow"
        g[k] = 0.0


def test_step_advance_guarded_takes_the_applied_index():
    H = _H()
    a, b = (torch.zeros((H.step_state_bytes() + 3) // 4, dtype=torch.int32, device=DEV) for _ in range(2))
    try:
        # skipped = 0: word for word segmm_step_advance (seed words, count, corrections, scheduled rate)
        for st, adv in ((a, H.step_advance), (b, H.step_advance_guarded)):
            H.step_bind(st)
            H.step_set(777, 0, B1, B2)
            H.step_schedule("cosine", 2e-3, warmup_steps=2, start_factor=0.5, decay_steps=9, eta_min=1e-4)
            for _ in range(5):
                adv(B1, B2)
        torch.cuda.synchronize()
        assert bool((a == b).all())
        # skipped = 2 at count 6: step 7 takes the corrections of step 5 -- segmm_step_set's -- the rate and the count of step 7
        H.step_bind(a)
        H.step_set(777, 5, B1, B2)
        _, _, bc5 = H.step_get()
        H.step_set(777, 7, B1, B2)
        lr7 = H.step_get_lr()[0]
        H.step_bind(b)
        H.step_set(777, 6, B1, B2)
        H.step_set_skipped(2)
        H.step_advance_guarded(B1, B2)
        _, step, bc = H.step_get()
        assert step == 7 and bc == bc5 and H.step_get_lr()[0] == lr7 and H.step_get_skipped() == (0, 2)
        assert bc == tuple(float(x) for x in G.corrections(7, 2, B1, B2))
    finally:
        torch.cuda.synchronize()
        H.step_bind(None)


# ------------------------------------------------------------------------------------------------ the tiny trainer
KINDS = {"img": "img_d32_N2", "id": "both_fh2"}
TABLE = "backbone2.vid_proj.weight"
_BATCHES = {}


def _cfg(kind):
    cfg, _, _, _ = load_case(KINDS[kind])
    return dict(cfg, d=64, h=2, N=1, S=8, Lt=4, n_items=36, exposure_prob=list(cfg["exposure_prob"])[:8])


def _poisoned(batch, poison, row=1):
    out = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()}
    assert bool(out["photo_mask"][row, 0])
    out["photo"][row, 0, 5] = poison
    return out


def _batches(kind, B=4, n=6, host=False):
    """Batches 1 .. n on the device (built once, read-only)."""
    from segmminterest_amd.synth import make_batch
    key = (kind, B, host)
    if key not in _BATCHES:
        cfg = _cfg(kind)
        bs = [make_batch(B, cfg["S"], cfg["Lt"], cfg["D_in"], n_users=cfg.get("n_users", 50), n_items=cfg["n_items"], seed=700 + i) for i in range(n)]
        _BATCHES[key] = bs if host else [{k: v.to(DEV) for k, v in b.items()} for b in bs]
    return _BATCHES[key]


def _trainer(kind, **kw):
    from segmminterest_amd.trainer import Trainer
    torch.manual_seed(5)
    model = build_model(_cfg(kind)).to(DEV)
    kw.setdefault("weight_decay", WD)
    kw.setdefault("device_state", True)
    tr = Trainer(model, lr=LR, **kw)
    if kind == "id":
        assert tuple(dict(model.named_parameters())[TABLE].shape)[0] == 37
    return tr


def _snap(tr):
    torch.cuda.synchronize()
    st = tr.model._store
    out = [st.flat[:st.n_live], tr.opt.m, tr.opt.v] + ([tr.ema.shadow] if tr.ema is not None else [])
    return tuple(x.detach().clone() for x in out)


def _equal(a, b):
    return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))


GUARDED = dict(skip_nonfinite=True, ema=0.9)


def _five(kind, poison):
    bs = _batches(kind)[:5]
    return bs[:2] + [_poisoned(bs[2], poison)] + bs[3:]


@pytest.mark.parametrize("kind,poison", [("img", math.nan), ("img", math.inf), ("id", math.nan)], ids=["img-nan", "img-inf", "id-nan"])
def test_trainer_skips_the_poisoned_step_and_goes_on(kind, poison):
    """Five steps, dropout on, EMA; the third batch has one poisoned element in batch["photo"].  Step 3 leaves every live parameter
    (the id table with them), m, v and the shadow as step 2 left them; steps 4 and 5 train on; the counts; and step 4 IS the reference
    step from the state after step 2 on step 4's gradient at applied index 3."""
    tr = _trainer(kind, **GUARDED)
    st = tr.model._store
    snaps, outs = [], []
    for b in _five(kind, poison):
        out = tr.train_step(b)
        outs.append((int(out["skipped"]), float(out["loss"])))
        snaps.append(_snap(tr))
        if len(snaps) == 4:
            g4 = st.gflat[:st.n_live].detach().clone()
    print("skipped / loss per step:", outs)
    assert [s for s, _ in outs] == [0, 0, 1, 0, 0]
    assert _equal(snaps[2], snaps[1]), "the skipped step changed a parameter, a moment or the shadow"
    assert not _equal(snaps[1][:1], snaps[0][:1])
    assert all(math.isfinite(l) for _, l in outs[3:])
    assert not _same(snaps[3][0], snaps[2][0]) and not _same(snaps[4][0], snaps[3][0]) and not _same(snaps[4][3], snaps[2][3])
    assert all(bool(torch.isfinite(x).all()) for x in snaps[4])
    assert tr.opt.step_count == 5 and tr.opt.skipped_steps == 1 and tr.opt.applied_steps == 4
    sd = tr.opt.state_dict()
    assert {float(s["step"]) for s in sd["state"].values()} == {4.0} and sd["param_groups"][0]["segmm_skipped_steps"] == 1
    assert float(tr.opt.grad_norm) > 0.0          # (the guard alone reports the norm, as max_grad_norm=inf does)
    # step 4 against the reference: corrections of applied index 3, whatever the attempted count says
    p2, m2, v2 = (x.cpu().numpy() for x in snaps[1][:3])
    want = G.step(p2, m2, v2, g4.cpu().numpy(), 2, LR, B1, B2, EPS, WD)
    assert want[3] == 0
    for name, got, ref in zip("pmv", snaps[3][:3], want[:3]):
        diff = got.cpu().numpy().view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64)
        print("step 4, %s: %d of %d elements differ from guard_ref, at most %d ulp" % (name, int((diff != 0).sum()), diff.size, int(np.abs(diff).max())))
    for got, ref in zip(snaps[3][:3], want[:3]):
        assert (got.cpu().numpy().view(np.int32) == ref.view(np.int32)).all()


@pytest.mark.parametrize("kind", ["img", "id"])
def test_clean_batches_cost_no_bits(kind):
    """Four clean steps: the guarded trainer, the max_grad_norm=inf trainer and the plain trainer hold the same bits (the plain
    id-mode trainer steps its table in two passes, the guarded one densely at the tail)."""
    runs = []
    for kw in (dict(skip_nonfinite=True), dict(max_grad_norm=math.inf), {}):
        tr = _trainer(kind, ema=0.9, **kw)
        for b in _batches(kind)[:4]:
            out = tr.train_step(b)
        assert ("skipped" in out) == bool(kw.get("skip_nonfinite", False))
        runs.append(_snap(tr))
        if kw.get("skip_nonfinite"):
            assert tr.opt.skipped_steps == 0 and int(out["skipped"]) == 0
    assert _equal(runs[0], runs[1]), "guarded != max_grad_norm=inf"
    assert _equal(runs[0], runs[2]), "guarded != plain"


@pytest.mark.parametrize("kind", ["img", "id"])
def test_recorded_equals_eager(kind):
    """The same five batches: step 1 eager, step 2 recorded, steps 3 (the poisoned one), 4 and 5 replayed -- the bits and the counts
    of the eager guarded run; a changed option refuses the recording."""
    bs = _five(kind, math.nan)
    eager = _trainer(kind, **GUARDED)
    for b in bs:
        eager.train_step(b)
    rec = _trainer(kind, **GUARDED)
    rec.train_step(bs[0])
    rec.record(bs[1], warmup=0, prev_batch=bs[0])
    flags = []
    for b in bs[2:]:
        out = rec.run_recorded(b)
        flags.append(int(out["skipped"]))
    assert flags == [1, 0, 0]
    assert _equal(_snap(eager), _snap(rec))
    assert (rec.opt.step_count, rec.opt.skipped_steps) == (eager.opt.step_count, eager.opt.skipped_steps) == (5, 1)
    assert bool((eager._step_state == rec._step_state).all())          # seed words, counts, corrections: word for word
    rec.opt.skip_nonfinite = False
    with pytest.raises(RuntimeError, match="hyperparameters changed"):
        rec.run_recorded(bs[0])


def test_micro_batches_take_one_verdict_on_the_summed_gradient():
    """micro_batch = 2 at B = 4, the NaN in a row of the second pass: one skipped optimizer step, then training goes on."""
    bs = _batches("img")
    tr = _trainer("img", micro_batch=2, **GUARDED)
    tr.train_step(bs[0])
    before = _snap(tr)
    out = tr.train_step(_poisoned(bs[1], math.nan, row=3))
    assert int(out["skipped"]) == 1 and _equal(_snap(tr), before)
    out = tr.train_step(bs[2])
    assert int(out["skipped"]) == 0 and not _same(_snap(tr)[0], before[0]) and math.isfinite(float(out["loss"]))
    assert (tr.opt.step_count, tr.opt.skipped_steps) == (3, 1)


def test_a_poisoned_frozen_gradient_does_not_skip():
    """param_groups with a frozen group: NaN in the frozen parameters' gradient alone stays out of the norm -- the step is applied;
    the same NaN in a trained parameter's gradient skips it."""
    H = _H()
    probe = _trainer("img")          # (which parameters are live is the store's to say: the first and the last of the live range)
    probe.train_step(_batches("img")[0])
    live = sorted(probe.model._store.live_names, key=lambda n: probe.model._store.index[n][0])
    trained, frozen = live[0], live[-1]
    tr = _trainer("img", param_groups=[{"params": [frozen], "frozen": True}], **GUARDED)
    st = tr.model._store
    tr.train_step(_batches("img")[0])
    o, k = st.index[frozen]
    o2, _ = st.index[trained]
    assert trained != frozen and o + k <= st.n_live and k > 3
    for at, skipped in ((o + 3, 0), (o2 + 3, 1)):
        before = _snap(tr)
        st.gflat[at] = math.nan
        H.step_bind(tr._step_state)
        H.step_advance_guarded(B1, B2)          # (the head of a trainer's step)
        tr.opt.step()
        assert int(tr.opt.skipped) == skipped and tr.opt.skipped_steps == skipped
        after = _snap(tr)
        assert _same(after[0][o:o + k], before[0][o:o + k])          # frozen: never stepped
        assert _equal(after, before) == bool(skipped)
        st.gflat[at] = 0.0


# ------------------------------------------------------------------------------------------------ 6. two data-parallel ranks
def _run_dp(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from segmminterest_amd.trainer import DPComm, Trainer, shard_rows
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.manual_seed(5)
        model = build_model(_cfg("img")).cuda()
        tr = Trainer(model, lr=LR, weight_decay=WD, comm=DPComm(), overlap=True, device_state=True, **GUARDED)
        s, e = shard_rows(8, world, rank)
        flags, snaps = [], []
        for i, full in enumerate(_batches("img", B=8, n=3, host=True)):
            shard = {k: v[s:e].contiguous().cuda() for k, v in full.items()}
            if i == 1 and rank == 1:          # the poisoned row sits on rank 1 only
                shard = _poisoned(shard, math.nan)
            out = tr.train_step(shard)
            flags.append(int(out["skipped"]))
            snaps.append([x.cpu().numpy() for x in _snap(tr)])
        q.put((rank, flags, tr.opt.step_count, tr.opt.skipped_steps, snaps))
    finally:
        dist.destroy_process_group()


def test_two_ranks_skip_together():
    """Two gloo ranks on one GPU; every rank takes the norm of the same all-reduced gradient: both skip step 2, the replicas stay
    bitwise equal, the counts agree."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29700 + os.getpid() % 200
    procs = [ctx.Process(target=_run_dp, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict((r[0], r[1:]) for r in (q.get(timeout=240), q.get(timeout=240)))
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    (f0, n0, k0, s0), (f1, n1, k1, s1) = res[0], res[1]
    assert f0 == f1 == [0, 1, 0] and (n0, k0) == (n1, k1) == (3, 1)
    for a, b in zip(s0, s1):
        assert all((x.view(np.int32) == y.view(np.int32)).all() for x, y in zip(a, b)), "the replicas differ"
    assert all((x.view(np.int32) == y.view(np.int32)).all() for x, y in zip(s0[1], s0[0])), "the skipped step moved rank 0"
    assert not (s0[2][0].view(np.int32) == s0[1][0].view(np.int32)).all()
