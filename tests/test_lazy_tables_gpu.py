"""Lazy exact AdamW of the id tables on the device.  Every comparison is BITWISE (int32 views) and the yardstick is always the dense
update the project already has -- phase 0 + phase 1 of segmm_adamw_table (/ _lrs / _scaled) on a copy, or the default Trainer --
never the code under test.  tests/test_lazy_tables_cpu.py shows that a bitwise comparison of this kind rejects every defect of
order the protocol can have (range ends, stale ring slots, the wrong step's rate or bias corrections, duplicates).

1. the kernels: segmm_adamw_hist_push, segmm_adamw_table_catchup (listed rows, flush), segmm_adamw_table_stamp around today's
   phase 1, 12 steps with a ring of 4, at width / 4 below, at and above one wave's 64 lanes and past the flush's capped grid;
2. idempotence: a second catch-up changes nothing, a row whose stamp is current is neither replayed nor written;
3. Trainer(lazy_tables=dict(flush_every=8)) against the default trainer: eager, recorded, clipped + scheduled + grouped,
   micro-batched, around a validation pass, across a checkpoint, and the refusals."""
import copy
import types

import numpy as np
import pytest
import torch

from helpers import build_model, load_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
OFF, GUARD = 96, 32          # where a table sits inside its buffers, and the untouched floats checked behind it
B1, B2, EPS = 0.9, 0.999, 1e-8
STEPS, CAP = 12, 4


def _H():
    from segmminterest_amd import hipabi as H
    H.lib()
    return H


def _i32(t):
    return t.detach().contiguous().view(torch.int32)


def _same(a, b):
    return bool((_i32(a) == _i32(b)).all())


@pytest.fixture
def own_step_state():
    """A step state of the test's own, bound for the test; the library's default state is bound again afterwards."""
    H = _H()
    state = torch.zeros((H.step_state_bytes() + 3) // 4, dtype=torch.int32, device=DEV)
    H.step_bind(state)
    try:
        yield state
    finally:
        torch.cuda.synchronize()
        H.step_bind(None)


def _buffers(rows, width, seed):
    """p, m, v: a non-trivial table state at float OFF of buffers filled with other numbers."""
    g = torch.Generator().manual_seed(seed)
    n, size = rows * width, OFF + rows * width + GUARD
    out = []
    for k in range(3):
        h = 1000.0 + 100.0 * torch.randn(size, generator=g)
        t = torch.randn(n, generator=g)
        h[OFF:OFF + n] = (0.05 * t, 0.1 * t, 0.01 * (0.25 + 0.75 * torch.rand(n, generator=g)))[k]
        out.append(h)
    return out


def _id_lists(rows, n_ids, seed):
    """One id list per step: duplicates, ids outside the table; step 5 lists nothing; row 3 is never listed."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for k in range(STEPS):
        ids = torch.randint(0, rows, (n_ids,), generator=g)
        ids[ids == 3] = 4
        ids = torch.cat([ids[:n_ids // 2], ids[:n_ids // 4], torch.tensor([-1, rows, rows + 7, -2 ** 40]), ids[n_ids // 2:]])
        out.append((ids if k != 5 else ids[:0]).to(torch.int64).to(DEV))
    return out


KERNEL_CASES = [(257, 8, "plain"), (300, 384, "plain"), (70_000, 64, "plain"), (300, 384, "scaled_nodecay"), (300, 384, "clip"),
                (257, 8, "state"), (300, 384, "state"), (300, 256, "plain")]


@pytest.mark.parametrize("rows,width,variant", KERNEL_CASES, ids=["%dx%d-%s" % c for c in KERNEL_CASES])
def test_lazy_launches_equal_the_dense_launches_bitwise(rows, width, variant, own_step_state):
    """12 steps at a rate that changes every step, ring of 4 (it wraps three times; the flush comes whenever 4 steps are pending).
    Lazy: catch-up of the listed rows to T - 1, the ring's entry of T, phase 1, the stamp; a final flush.  Dense, on a copy: phase 0
    + phase 1.  p, m, v equal in every bit, every stamp 12, the lazy flags and the floats around the table untouched.
    Variants: ``scaled_nodecay`` lr_scale 0.5 and decay 0 (segmm_adamw_table_lrs); ``clip`` a clip coefficient on phase 1;
    ``state`` count, bias corrections and a cosine-scheduled rate from the device step state (step = -1, SEGMM_LIVE_LR, relative
    targets).  Widths 8, 256 and 384: width / 4 below, at and above one wave's 64 lanes."""
    H = _H()
    n = rows * width
    scale, wd = (0.5, 0.0) if variant == "scaled_nodecay" else (1.0, 1e-2)
    coef = torch.tensor([0.37], device=DEV) if variant == "clip" else None
    live = variant == "state"
    id_lists = _id_lists(rows, 40 if rows < 1000 else 500, rows + width)
    host = _buffers(rows, width, rows * 7 + width)
    lazy, dense = [h.clone().to(DEV) for h in host], [h.clone().to(DEV) for h in host]
    gen = torch.Generator().manual_seed(11)
    stamps = torch.zeros(rows, dtype=torch.int32, device=DEV)
    hist = torch.zeros((CAP, 4), device=DEV)
    flags_l = torch.zeros(rows, dtype=torch.int32, device=DEV)
    flags_d = torch.zeros(rows, dtype=torch.int32, device=DEV)
    flushed = 0
    for k, ids in enumerate(id_lists):
        T = k + 1
        g = torch.zeros(OFF + n + GUARD)
        g[OFF:OFF + n] = torch.randn(n, generator=gen)
        g = g.to(DEV)
        lr = H.LIVE_LR if live else 1e-3 * (1.0 + 0.3 * k)
        step = -1 if live else T
        if T - 1 - flushed >= CAP:          # the flush rule: the ring holds the last CAP steps
            H.adamw_table_catchup(*lazy, OFF, rows, width, None, stamps, hist, T - 1, scale, B1, B2, EPS, wd)
            flushed = T - 1
        if live:
            if k == 0:
                H.step_set(1234, 0, B1, B2)
                H.step_schedule("cosine", 2e-3, warmup_steps=2, start_factor=0.5, decay_steps=9, eta_min=1e-4)
            H.step_advance(B1, B2)
        H.adamw_table_lrs(dense[0], None, dense[1], dense[2], OFF, rows, width, ids, flags_d, lr, scale, B1, B2, EPS, wd, step, 0)
        H.adamw_table_lrs(dense[0], g, dense[1], dense[2], OFF, rows, width, ids, flags_d, lr, scale, B1, B2, EPS, wd, step, 1, coef=coef)
        H.adamw_table_catchup(*lazy, OFF, rows, width, ids, stamps, hist, -1 if live else T - 1, scale, B1, B2, EPS, wd, relative=live,
                              flags=flags_l)
        H.adamw_hist_push(hist, lr, B1, B2, step)
        H.adamw_table_lrs(lazy[0], g, lazy[1], lazy[2], OFF, rows, width, ids, flags_l, lr, scale, B1, B2, EPS, wd, step, 1, coef=coef)
        H.adamw_table_stamp(ids, rows, stamps, 0 if live else T, relative=live)
    assert int(stamps[3]) == flushed < STEPS          # the row never listed is behind until the flush
    H.adamw_table_catchup(*lazy, OFF, rows, width, None, stamps, hist, STEPS, scale, B1, B2, EPS, wd)
    torch.cuda.synchronize()
    assert int(flags_l.abs().sum()) == 0 and int(flags_d.abs().sum()) == 0
    assert bool((stamps == STEPS).all())
    for name, a, b, h in zip("pmv", lazy, dense, host):
        assert _same(a[OFF:OFF + n], b[OFF:OFF + n]), "%s differs from the dense update" % name
        assert not _same(a[OFF:OFF + n], h[OFF:OFF + n].to(DEV))
        assert _same(a[:OFF], h[:OFF].to(DEV)) and _same(a[OFF + n:], h[OFF + n:].to(DEV)), "%s: floats around the table moved" % name


@pytest.mark.parametrize("width", [8, 256, 384])
def test_catchup_is_idempotent_and_leaves_current_rows_alone(width):
    """A second catch-up to the same target changes no bit.  Rows whose stamp already says ``target`` are neither replayed nor written:
    they hold NaN sentinels in m (and arbitrary p, v) that a replay would spread into p and a rewrite would have to reproduce, and
    the floats behind each row's width -- the next row's first, the guard behind the table -- keep their bits too."""
    H = _H()
    rows, target = 64, 3
    n = rows * width
    bufs = [h.to(DEV) for h in _buffers(rows, width, 5)]
    hist = torch.tensor([[0.0, 1.0, 1.0, 0.0], [1e-3, 0.1, 0.0316, 0.0], [2e-3, 0.19, 0.0447, 0.0], [3e-3, 0.271, 0.0547, 0.0]], device=DEV)
    stamps = torch.zeros(rows, dtype=torch.int32, device=DEV)
    current = torch.arange(0, rows, 3, device=DEV)
    stamps[current] = target
    m_rows = bufs[1][OFF:OFF + n].view(rows, width)
    m_rows[current] = float("nan")
    before = [b.clone() for b in bufs]
    ids = torch.cat([torch.arange(rows), torch.arange(rows)]).to(torch.int64).to(DEV)          # every row, twice
    H.adamw_table_catchup(*bufs, OFF, rows, width, ids, stamps, hist, target, 1.0, B1, B2, EPS, 1e-2)
    torch.cuda.synchronize()
    once = [b.clone() for b in bufs]
    H.adamw_table_catchup(*bufs, OFF, rows, width, ids, stamps, hist, target, 1.0, B1, B2, EPS, 1e-2)
    H.adamw_table_catchup(*bufs, OFF, rows, width, None, stamps, hist, target, 1.0, B1, B2, EPS, 1e-2)
    torch.cuda.synchronize()
    assert bool((stamps == target).all())
    behind = torch.ones(rows, dtype=torch.bool, device=DEV)
    behind[current] = False
    for name, a, o, b in zip("pmv", bufs, once, before):
        assert _same(a, o), "%s: the second catch-up changed bits" % name
        ra, rb = a[OFF:OFF + n].view(rows, width), b[OFF:OFF + n].view(rows, width)
        assert _same(ra[current], rb[current]), "%s: a current row was touched" % name
        assert not bool((_i32(ra[behind]) == _i32(rb[behind])).all(dim=1).any()), "%s: a row behind the target did not move" % name
        assert _same(a[:OFF], b[:OFF]) and _same(a[OFF + n:], b[OFF + n:])
        assert not bool(torch.isnan(ra[behind]).any())


# ------------------------------------------------------------------------------------------------ 3. the trainer
TABLE = "backbone1.vid_proj.weight"
N_STEPS, LAZY = 24, dict(flush_every=8)
SCHED = dict(kind="cosine", warmup_steps=3, decay_steps=20, eta_min=1e-4)


def _cfg():
    cfg, _, _, _ = load_case("id_d32_N2")
    S = 20
    return dict(cfg, S=S, n_items=500, exposure_prob=list(cfg["exposure_prob"])[:S])


_BATCHES = {}


def _batches(n=N_STEPS + 8, B=16):
    from segmminterest_amd.synth import make_batch
    if not _BATCHES:
        cfg = _cfg()
        _BATCHES["b"] = [{k: v.to(DEV) for k, v in make_batch(B, cfg["S"], cfg["Lt"], cfg["D_in"], n_users=cfg["n_users"], n_items=cfg["n_items"],
                                                            seed=900 + i).items()} for i in range(n)]
    return _BATCHES["b"]


def _trainer(groups=None, **kw):
    from segmminterest_amd.trainer import Trainer
    torch.manual_seed(5)
    model = build_model(_cfg()).to(DEV)
    kw.setdefault("dropout", False)
    kw.setdefault("weight_decay", 1e-2)
    if groups is not None:
        kw["param_groups"] = groups
    return Trainer(model, **kw)


def _snap(tr):
    torch.cuda.synchronize()
    return tuple(x.detach().clone() for x in (tr.model._store.flat, tr.opt.m, tr.opt.v))


def _equal(a, b):
    return all(_same(x, y) for x, y in zip(a, b))


def _sd_equal(a, b):
    assert set(a) == set(b) == {"state", "param_groups"} and a["param_groups"] == b["param_groups"] and set(a["state"]) == set(b["state"])
    return all(_same(a["state"][i][k].to(DEV), b["state"][i][k].to(DEV)) for i in a["state"] for k in ("exp_avg", "exp_avg_sq")) and \
        all(float(a["state"][i]["step"]) == float(b["state"][i]["step"]) for i in a["state"])


def _run(tr, first, last, recorded_from=None):
    bs = _batches()
    for t in range(first, last + 1):
        if recorded_from is None or t < recorded_from:
            tr.train_step(bs[t - 1])
        elif t == recorded_from:
            tr.record(bs[t - 1], warmup=0, prev_batch=bs[t - 2])
        else:
            tr.run_recorded(bs[t - 1])


def test_trainer_eager_equals_dense_around_validation_and_checkpoint():
    """24 eager steps, a validation pass after step 10 (it flushes; the dense trainer's metrics exactly), ``state_dict()`` without an
    explicit flush, then 3 more steps and ``flush_tables()``."""
    dense, lazy = _trainer(), _trainer(lazy_tables=LAZY)
    _run(dense, 1, 10)
    _run(lazy, 1, 10)
    assert lazy.opt.tables_pending == 2 and not _equal(_snap(dense), _snap(lazy))          # (flushed ahead of step 9: rows are behind)
    vb = _batches()[N_STEPS:N_STEPS + 2]
    assert dense.valid_model(vb, permutation=0) == lazy.valid_model(vb, permutation=0)
    assert lazy.opt.tables_pending == 0 and _equal(_snap(dense), _snap(lazy))
    _run(dense, 11, N_STEPS)
    _run(lazy, 11, N_STEPS)
    assert lazy.opt.tables_pending > 0
    assert _sd_equal(dense.opt.state_dict(), lazy.opt.state_dict())
    assert lazy.opt.tables_pending == 0 and _equal(_snap(dense), _snap(lazy))
    _run(dense, N_STEPS + 1, N_STEPS + 3)
    _run(lazy, N_STEPS + 1, N_STEPS + 3)
    assert lazy.opt.tables_pending == 3
    lazy.opt.flush_tables()
    assert lazy.opt.tables_pending == 0 and _equal(_snap(dense), _snap(lazy))
    assert bool((lazy.opt._lazy[TABLE]["stamps"] == N_STEPS + 3).all())


def test_trainer_recorded_equals_eager_dense():
    """Steps 1-2 eager, step 3 recorded, 4-24 replayed (the host's periodic flush between replays; never inside the recording), a
    recorded validation pass after step 10: against the eager DENSE trainer in the same mode."""
    dense, lazy = _trainer(device_state=True), _trainer(device_state=True, lazy_tables=LAZY)
    vb = _batches()[N_STEPS:N_STEPS + 2]
    _run(dense, 1, 10)
    _run(lazy, 1, 10, recorded_from=3)
    assert lazy.opt.tables_pending == 8          # (record() flushed ahead of step 3; the flush of eight pending steps is due)
    assert dense.valid_model(vb, permutation=0, recorded=True, seed=3) == lazy.valid_model(vb, permutation=0, recorded=True, seed=3)
    assert lazy.opt.tables_pending == 0
    _run(dense, 11, N_STEPS)
    for t in range(11, N_STEPS + 1):
        lazy.run_recorded(_batches()[t - 1])
    assert lazy.opt.tables_pending > 0
    lazy.opt.flush_tables()
    assert _equal(_snap(dense), _snap(lazy))


@pytest.mark.parametrize("recorded", [False, True], ids=["eager", "recorded"])
def test_trainer_clipped_scheduled_grouped(recorded):
    """max_grad_norm, a cosine schedule with warm-up and the table in a group of its own at lr_scale 0.5 / decay 0.05; set_base_lr
    ahead of step 15 (the ring holds the rate each step used)."""
    kw = dict(device_state=True, max_grad_norm=0.05, lr_schedule=SCHED, groups=[{"params": [TABLE], "lr_scale": 0.5, "weight_decay": 0.05}])
    dense, lazy = _trainer(**kw), _trainer(lazy_tables=LAZY, **kw)
    _run(dense, 1, 14)
    _run(lazy, 1, 14, recorded_from=3 if recorded else None)
    dense.opt.set_base_lr(5e-4)
    lazy.opt.set_base_lr(5e-4)
    _run(dense, 15, N_STEPS)
    if recorded:
        for t in range(15, N_STEPS + 1):
            lazy.run_recorded(_batches()[t - 1])
    else:
        _run(lazy, 15, N_STEPS)
    assert _sd_equal(dense.opt.state_dict(), lazy.opt.state_dict()) and _equal(_snap(dense), _snap(lazy))


def test_trainer_micro_batched():
    dense, lazy = _trainer(micro_batch=8), _trainer(micro_batch=8, lazy_tables=LAZY)
    _run(dense, 1, N_STEPS)
    _run(lazy, 1, N_STEPS)
    assert lazy.opt.tables_pending == 8
    lazy.opt.flush_tables()
    assert _equal(_snap(dense), _snap(lazy))


def test_frozen_table_launches_nothing():
    lazy = _trainer(lazy_tables=LAZY, groups=[{"params": [TABLE], "frozen": True}])
    t0 = lazy.model.get_parameter(TABLE).detach().clone()
    _run(lazy, 1, 3)
    torch.cuda.synchronize()
    assert not lazy.opt._lazy and lazy.opt.tables_pending == 0 and _same(lazy.model.get_parameter(TABLE), t0)


def test_image_mode_step_is_unchanged_launch_for_launch():
    """A model without an id table: ``lazy_tables`` registers nothing, the recorded step holds the same commands and the same bits."""
    from segmminterest_amd.synth import make_batch
    from segmminterest_amd.trainer import Trainer
    cfg, _, _, _ = load_case("img_d32_N2")
    cfg = dict(cfg, S=8, Lt=min(4, cfg["Lt"]), exposure_prob=list(cfg["exposure_prob"])[:8])
    bs = [{k: v.to(DEV) for k, v in make_batch(4, 8, cfg["Lt"], cfg["D_in"], n_users=5, n_items=5, seed=700 + i).items()} for i in range(4)]
    runs = []
    for lazy in (None, True):
        torch.manual_seed(5)
        tr = Trainer(build_model(cfg).to(DEV), dropout=False, device_state=True, lazy_tables=lazy)
        tr.train_step(bs[0])
        tr.train_step(bs[1])
        tr.record(bs[2], warmup=0, prev_batch=bs[1])
        tr.run_recorded(bs[3])
        assert not tr.opt._lazy and tr.opt.tables_pending == 0
        ops = [(ph.kind, ph.backbone, ph.layer, [(arr[i].op, arr[i].stream) for i in range(ph.n_cmds)])
               for ph, arr in tr._recorded["phases"] if arr is not None]
        runs.append((ops, _snap(tr)))
    assert sum(len(p[3]) for p in runs[0][0]) > 20
    assert runs[0][0] == runs[1][0], "the recorded phases, entry points or stream slots differ"
    assert _equal(runs[0][1], runs[1][1])


def test_unusual_id_lists_are_caught_up_before_the_forward():
    """An int32 id list at step 5 and a strided int64 one at step 7 in the middle of a lazy run: the forward converts such a list and
    reads the batch's rows, so the lazy step must have brought those rows up to date first -- bitwise the dense trainer."""
    def odd(t, b):
        ids = b["photo_identity_id"]
        if t == 5:
            return dict(b, photo_identity_id=ids.to(torch.int32))
        if t == 7:
            wide = torch.stack([ids, ids + 1], dim=1)
            assert not wide[:, 0].is_contiguous()
            return dict(b, photo_identity_id=wide[:, 0])
        return b
    dense, lazy = _trainer(), _trainer(lazy_tables=LAZY)
    for t in range(1, 11):
        b = odd(t, _batches()[t - 1])
        dense.train_step(b)
        lazy.train_step(b)
        if t in (5, 7):
            assert lazy.opt.tables_pending == t          # (no flush stood in for the catch-up)
    lazy.opt.flush_tables()
    assert _equal(_snap(dense), _snap(lazy))


def test_a_forward_of_the_callers_own_needs_a_flush_first():
    """``eval_step`` flushes by itself; a manual forward + ``opt.step()`` with rows pending is refused by name."""
    lazy = _trainer(lazy_tables=LAZY)
    _run(lazy, 1, 3)
    assert lazy.opt.tables_pending == 3
    with pytest.raises(RuntimeError, match="flush_tables\\(\\) BEFORE a forward"):
        lazy.opt.step()
    lazy.eval_step(_batches()[N_STEPS], mode="train")
    assert lazy.opt.tables_pending == 0


def test_resume_from_a_lazy_checkpoint():
    """16 steps, checkpoint (model weights read AFTER the optimizer's state_dict, which flushed), a fresh lazy trainer loads both and
    takes 8 more steps: bitwise the uninterrupted dense run; after the load every stamp is the loaded step count."""
    dense, first = _trainer(), _trainer(lazy_tables=LAZY)
    _run(dense, 1, N_STEPS)
    _run(first, 1, 16)
    sd_opt = copy.deepcopy(first.opt.state_dict())
    torch.cuda.synchronize()
    sd_model = {k: v.detach().cpu().clone() for k, v in first.model.state_dict().items()}
    second = _trainer(lazy_tables=LAZY)
    _run(second, 1, 2)          # (its tables are registered and rows are pending when the checkpoint arrives)
    second.opt.flush_tables()
    second.model.load_state_dict(sd_model)
    second.opt.load_state_dict(sd_opt)
    torch.cuda.synchronize()
    assert second.opt.step_count == 16 and second.opt.tables_pending == 0 and bool((second.opt._lazy[TABLE]["stamps"] == 16).all())
    _run(second, 17, N_STEPS)
    second.opt.flush_tables()
    assert _equal(_snap(dense), _snap(second))


def test_refusals_name_what_they_refuse():
    from segmminterest_amd.trainer import Trainer
    model = build_model(_cfg()).to(DEV)
    with pytest.raises(ValueError, match="DPComm"):
        Trainer(model, lazy_tables=True, comm=types.SimpleNamespace(active=True))
    with pytest.raises(ValueError, match="ema"):
        Trainer(model, lazy_tables=True, ema=0.99)
    with pytest.raises(ValueError, match="flush_every"):
        Trainer(model, lazy_tables=dict(flush_every=0))
    with pytest.raises(ValueError, match="unknown key 'every'"):
        Trainer(model, lazy_tables=dict(every=8))
    tr = Trainer(model, lazy_tables=LAZY, dropout=False)
    h = model.get_parameter(TABLE).register_hook(lambda g: g)
    try:
        with pytest.raises(RuntimeError, match="parameter hooks"):
            tr.train_step(_batches()[0])
    finally:
        h.remove()
