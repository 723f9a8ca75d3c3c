"""Lazy id tables beside the weight average on the device (lazy_tables=dict(ema=True)).  Every comparison is BITWISE (int32 views)
and the yardstick is always code the project already has and pins by tests of its own -- phase 0 + phase 1 of
segmm_adamw_table_lrs followed by segmm_ema_update over the table, on a copy, or the dense trainer ``Trainer(ema=...)`` -- never the
code under test.  tests/test_lazy_ema_ref_cpu.py shows that a bitwise comparison of this kind rejects every defect of order the
replayed lerps can have.

1. the kernels: segmm_adamw_hist_push_ema, segmm_adamw_table_catchup_ema (listed rows, flush), segmm_adamw_table_lazy_rows_ema:
   12 steps with a ring of 4, at width / 4 below, at and above one wave's 64 lanes and past the flush's capped grid;
2. idempotence: a second launch changes nothing, a row whose stamp is current keeps a sentinel shadow;
3. Trainer(ema=..., lazy_tables=dict(flush_every=8, ema=True)) against the dense EMA trainer: eager, recorded, clipped + scheduled
   + grouped, micro-batched, an EMA validation pass with rows pending, a checkpoint round trip, a frozen table."""
import numpy as np
import pytest
import torch

import ema_ref as R
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
    """Equal in every bit; NaN lanes as ema_ref.bits_equal_nan_aware compares them (NaN on both sides)."""
    a, b = a.detach().contiguous(), b.detach().contiguous()
    if a.shape != b.shape:
        return False
    na, nb = torch.isnan(a), torch.isnan(b)
    return bool((na == nb).all() and (_i32(a)[~na] == _i32(b)[~na]).all())


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
    """p, m, v, shadow: a non-trivial table state at float OFF of buffers filled with other numbers."""
    g = torch.Generator().manual_seed(seed)
    n, size = rows * width, OFF + rows * width + GUARD
    out = []
    for k in range(4):
        h = 1000.0 + 100.0 * torch.randn(size, generator=g)
        t = torch.randn(n, generator=g)
        h[OFF:OFF + n] = (0.05 * t, 0.1 * t, 0.01 * (0.25 + 0.75 * torch.rand(n, generator=g)), 0.04 * t)[k]
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


KERNEL_CASES = [(257, 8, "plain"), (300, 256, "plain"), (300, 384, "plain"), (70_000, 64, "plain"), (300, 384, "nowarm"),
                (300, 256, "decay_change"), (300, 384, "scaled_nodecay"), (300, 384, "clip"), (257, 8, "state"), (300, 384, "state")]


@pytest.mark.parametrize("rows,width,variant", KERNEL_CASES, ids=["%dx%d-%s" % c for c in KERNEL_CASES])
def test_lazy_ema_launches_equal_the_dense_launches_bitwise(rows, width, variant, own_step_state):
    """12 steps at a rate that changes every step, ring of 4 (it wraps three times; the flush comes whenever 4 steps are pending).
    Lazy: catchup_ema of the FIRST HALF of the step's list to T - 1 (a rank's own rows), hist_push_ema, lazy_rows_ema on the whole
    list (the rows of the second half replay their gap there); a final flush.  Dense, on a copy: phase 0 + phase 1, then
    segmm_ema_update over the table.  p, m, v and the shadow equal in every bit, every stamp 12, the floats around the four tables
    untouched, the ring's fourth floats the bits of ema_ref.w_at.
    Variants: ``plain`` warm-up on (another weight every step); ``nowarm`` warm-up off; ``decay_change`` warm-up off and the EMA
    weight changed at step 7 with no flush (the ring holds the weight each step used); ``scaled_nodecay`` lr_scale 0.5 and decay
    0; ``clip`` a clip coefficient; ``state`` count, bias corrections, a cosine-scheduled rate and the warm-up's step from the device
    step state (step = -1, SEGMM_LIVE_LR, relative targets)."""
    H = _H()
    n = rows * width
    scale, wd = (0.5, 0.0) if variant == "scaled_nodecay" else (1.0, 1e-2)
    coef = torch.tensor([0.37], device=DEV) if variant == "clip" else None
    live = variant == "state"
    warmup = variant not in ("nowarm", "decay_change")
    decays = [0.9 if variant != "decay_change" or k < 6 else 0.75 for k in range(STEPS)]
    id_lists = _id_lists(rows, 40 if rows < 1000 else 500, rows + width)
    host = _buffers(rows, width, rows * 7 + width)
    lazy, dense = [h.clone().to(DEV) for h in host], [h.clone().to(DEV) for h in host]
    gen = torch.Generator().manual_seed(11)
    stamps = torch.zeros(rows, dtype=torch.int32, device=DEV)
    hist = torch.zeros((CAP, 4), device=DEV)
    flags_d = torch.zeros(rows, dtype=torch.int32, device=DEV)
    flushed = 0
    for k, ids in enumerate(id_lists):
        T = k + 1
        g = torch.zeros(OFF + n + GUARD)
        g[OFF:OFF + n] = torch.randn(n, generator=gen)
        g = g.to(DEV)
        lr = H.LIVE_LR if live else 1e-3 * (1.0 + 0.3 * k)
        step = -1 if live else T
        w = float(R.weight(decays[k]))
        if T - 1 - flushed >= CAP:          # the flush rule: the ring holds the last CAP steps
            H.adamw_table_catchup_ema(*lazy, OFF, OFF, rows, width, None, stamps, hist, T - 1, scale, B1, B2, EPS, wd)
            flushed = T - 1
        if live:
            if k == 0:
                H.step_set(1234, 0, B1, B2)
                H.step_schedule("cosine", 2e-3, warmup_steps=2, start_factor=0.5, decay_steps=9, eta_min=1e-4)
            H.step_advance(B1, B2)
        H.adamw_table_lrs(dense[0], None, dense[1], dense[2], OFF, rows, width, ids, flags_d, lr, scale, B1, B2, EPS, wd, step, 0)
        H.adamw_table_lrs(dense[0], g, dense[1], dense[2], OFF, rows, width, ids, flags_d, lr, scale, B1, B2, EPS, wd, step, 1, coef=coef)
        H.ema_update(dense[3], dense[0], n, w, warmup, step, shadow_off=OFF, p_off=OFF)
        own = ids[:ids.numel() // 2]
        H.adamw_table_catchup_ema(*lazy, OFF, OFF, rows, width, own, stamps, hist, -1 if live else T - 1, scale, B1, B2, EPS, wd, relative=live)
        H.adamw_hist_push_ema(hist, lr, B1, B2, step, w, warmup)
        H.adamw_table_lazy_rows_ema(lazy[0], g, lazy[1], lazy[2], lazy[3], OFF, OFF, rows, width, ids, stamps, hist, lr, scale, B1, B2, EPS, wd,
                                    step, coef=coef)
    assert int(stamps[3]) == flushed < STEPS          # the row never listed is behind until the flush
    assert not _same(lazy[3][OFF:OFF + n], dense[3][OFF:OFF + n])
    H.adamw_table_catchup_ema(*lazy, OFF, OFF, rows, width, None, stamps, hist, STEPS, scale, B1, B2, EPS, wd)
    torch.cuda.synchronize()
    assert int(flags_d.abs().sum()) == 0
    assert bool((stamps == STEPS).all())
    for name, a, b, h in zip(("p", "m", "v", "shadow"), lazy, dense, host):
        assert _same(a[OFF:OFF + n], b[OFF:OFF + n]), "%s differs from the dense update" % name
        assert not _same(a[OFF:OFF + n], h[OFF:OFF + n].to(DEV))
        assert _same(a[:OFF], h[:OFF].to(DEV)) and _same(a[OFF + n:], h[OFF + n:].to(DEV)), "%s: floats around the table moved" % name
    want = np.zeros(CAP, dtype=F)
    for t in range(STEPS - CAP + 1, STEPS + 1):
        want[t % CAP] = R.w_at(decays[t - 1], t, warmup)
    assert np.array_equal(hist[:, 3].cpu().numpy().view(np.int32), want.view(np.int32)), "the ring's fourth floats are not w_t"
    if variant == "plain":
        assert len(set(want.tolist())) == CAP          # warm-up: another weight every step


@pytest.mark.parametrize("width", [8, 256, 384])
@pytest.mark.parametrize("tail", [False, True], ids=["catchup_ema", "lazy_rows_ema"])
def test_second_launch_changes_nothing_and_current_rows_are_left_alone(width, tail):
    """A second launch on the same list changes no bit.  Rows whose stamp already says the target are neither replayed nor written:
    they hold NaN sentinels in the shadow and in m (and arbitrary p, v) that a replay would spread and a rewrite would have to
    reproduce; the floats behind each row's width keep their bits too."""
    H = _H()
    rows, target = 64, 3
    n = rows * width
    bufs = [h.to(DEV) for h in _buffers(rows, width, 5)]
    g = torch.zeros(OFF + n + GUARD)
    g[OFF:OFF + n] = torch.randn(n, generator=torch.Generator().manual_seed(3))
    g = g.to(DEV)
    hist = torch.tensor([[0.0, 1.0, 1.0, 0.0], [1e-3, 0.1, 0.0316, 0.8], [2e-3, 0.19, 0.0447, 0.7], [3e-3, 0.271, 0.0547, 0.6]], device=DEV)
    stamps = torch.zeros(rows, dtype=torch.int32, device=DEV)
    current = torch.arange(0, rows, 3, device=DEV)
    stamps[current] = target
    for k in (1, 3):
        bufs[k][OFF:OFF + n].view(rows, width)[current] = float("nan")
    before = [b.clone() for b in bufs]
    ids = torch.cat([torch.arange(rows), torch.arange(rows)]).to(torch.int64).to(DEV)          # every row, twice

    def launch(lst):
        if tail:
            H.adamw_table_lazy_rows_ema(bufs[0], g, bufs[1], bufs[2], bufs[3], OFF, OFF, rows, width, lst, stamps, hist, 3e-3, 1.0, B1, B2, EPS,
                                        1e-2, target)
        else:
            H.adamw_table_catchup_ema(*bufs, OFF, OFF, rows, width, lst, stamps, hist, target, 1.0, B1, B2, EPS, 1e-2)
    launch(ids)
    torch.cuda.synchronize()
    once = [b.clone() for b in bufs]
    launch(ids)
    H.adamw_table_catchup_ema(*bufs, OFF, OFF, rows, width, None, stamps, hist, target, 1.0, B1, B2, EPS, 1e-2)
    torch.cuda.synchronize()
    assert bool((stamps == target).all())
    behind = torch.ones(rows, dtype=torch.bool, device=DEV)
    behind[current] = False
    for name, a, o, b in zip(("p", "m", "v", "shadow"), bufs, once, before):
        assert _same(a, o), "%s: the second launch changed bits" % name
        ra, rb = a[OFF:OFF + n].view(rows, width), b[OFF:OFF + n].view(rows, width)
        assert bool((_i32(ra[current]) == _i32(rb[current])).all()), "%s: a current row was touched" % name
        assert not bool((_i32(ra[behind]) == _i32(rb[behind])).all(dim=1).any()), "%s: a row behind the target did not move" % name
        assert bool((_i32(a[:OFF]) == _i32(b[:OFF])).all()) and bool((_i32(a[OFF + n:]) == _i32(b[OFF + n:])).all())
        assert not bool(torch.isnan(ra[behind]).any())
    assert bool(torch.isnan(bufs[3][OFF:OFF + n].view(rows, width)[current]).all())          # the sentinel shadow is still there


# ------------------------------------------------------------------------------------------------ 3. the trainer
TABLE = "backbone1.vid_proj.weight"
N_STEPS = 20
EMA = dict(decay=0.99, warmup=True)
LAZY = dict(flush_every=8, ema=True)
SCHED = dict(kind="cosine", warmup_steps=3, decay_steps=20, eta_min=1e-4)


def _cfg():
    cfg, _, _, _ = load_case("id_d32_N2")
    S = 20
    return dict(cfg, S=S, n_items=500, exposure_prob=list(cfg["exposure_prob"])[:S])


_BATCHES = {}


def _batches(n=N_STEPS + 3, B=16):
    from segmminterest_amd.synth import make_batch
    if not _BATCHES:
        cfg = _cfg()
        _BATCHES["b"] = [{k: v.to(DEV) for k, v in make_batch(B, cfg["S"], cfg["Lt"], cfg["D_in"], n_users=cfg["n_users"], n_items=cfg["n_items"],
                                                            seed=1900 + i).items()} for i in range(n)]
    return _BATCHES["b"]


def _short():
    """The short last batch of an epoch: 5 rows of a batch of their own."""
    return {k: (v[:5].contiguous() if torch.is_tensor(v) else v) for k, v in _batches()[N_STEPS].items()}


def _trainer(groups=None, **kw):
    from segmminterest_amd.trainer import Trainer
    torch.manual_seed(5)
    model = build_model(_cfg()).to(DEV)
    kw.setdefault("dropout", False)
    kw.setdefault("weight_decay", 1e-2)
    kw.setdefault("ema", dict(EMA))
    if groups is not None:
        kw["param_groups"] = groups
    return Trainer(model, **kw)


def _pair(**kw):
    return _trainer(**kw), _trainer(lazy_tables=dict(LAZY), **kw)


def _snap(tr):
    torch.cuda.synchronize()
    return tuple(x.detach().clone() for x in (tr.model._store.flat, tr.opt.m, tr.opt.v, tr.ema.shadow))


def _equal(a, b):
    return all(_same(x, y) for x, y in zip(a, b))


def _ema_sd_equal(a, b):
    sa, sb = a.ema.state_dict(), b.ema.state_dict()
    return list(sa) == list(sb) and all(_same(sa[k], sb[k]) for k in sa)


def _run(tr, first, last, recorded_from=None):
    bs = _batches()
    for t in range(first, last + 1):
        if recorded_from is None or t < recorded_from:
            tr.train_step(bs[t - 1])
        elif t == recorded_from:
            tr.record(bs[t - 1], warmup=0, prev_batch=bs[t - 2])
        else:
            tr.run_recorded(bs[t - 1])


def _table_rows(tr, x):
    o, n = tr.model._store.index[TABLE]
    return x[o:o + n]


def test_trainer_eager_equals_the_dense_ema_trainer():
    """20 eager steps and the short last batch.  With rows pending the raw shadow is behind (that is the saving); after
    ``flush_tables()`` parameters, moments, the shadow and ``ema.state_dict()`` are the dense EMA trainer's in every bit."""
    dense, lazy = _pair()
    assert lazy.opt.lazy_ema is True and dense.opt.lazy_ema is False
    _run(dense, 1, N_STEPS)
    _run(lazy, 1, N_STEPS)
    for tr in (dense, lazy):
        tr.train_step(_short())
    assert lazy.opt.tables_pending == 5 and lazy.opt.step_count == N_STEPS + 1          # (flushed ahead of steps 9 and 17)
    sd, sl = _snap(dense), _snap(lazy)
    assert not _same(_table_rows(lazy, sl[3]), _table_rows(dense, sd[3])) and not _same(_table_rows(lazy, sl[0]), _table_rows(dense, sd[0]))
    lazy.opt.flush_tables()
    assert lazy.opt.tables_pending == 0 and _equal(_snap(dense), _snap(lazy))
    assert bool((lazy.opt._lazy[TABLE]["stamps"] == N_STEPS + 1).all())
    assert _ema_sd_equal(dense, lazy)
    _run(dense, 1, 2)
    _run(lazy, 1, 2)
    assert lazy.opt.tables_pending == 2 and _ema_sd_equal(dense, lazy) and lazy.opt.tables_pending == 0          # state_dict() flushes


def test_trainer_recorded_equals_the_eager_dense_ema_trainer():
    """Steps 1-2 eager, step 3 recorded, 4-20 replayed (the host's periodic flush between replays, never inside the recording), then
    the short last batch eagerly: against the eager DENSE EMA trainer in the same mode.  The recording holds the new launches as
    commands and no flush; after ``ema.decay`` changed a replay is refused."""
    dense, lazy = _pair(device_state=True)
    _run(dense, 1, N_STEPS)
    _run(lazy, 1, N_STEPS, recorded_from=3)
    H = _H()
    ops = {v: k for k, v in H.op_ids().items()}
    names = [ops.get(arr[i].op) for ph, arr in lazy._recorded["phases"] if arr is not None for i in range(ph.n_cmds)]          # (None: a fork / join)
    assert names.count("segmm_adamw_table_catchup_ema") == 1 and names.count("segmm_adamw_hist_push_ema") == 1
    st = lazy.model._store
    o, n = st.index[TABLE]
    assert names.count("segmm_adamw_table_lazy_rows_ema") == 1 and names.count("segmm_ema_update") == (o > 0) + (o + n < st.n_live) >= 1
    assert not any(n in names for n in ("segmm_adamw_table_catchup", "segmm_adamw_hist_push", "segmm_adamw_table_stamp", "segmm_adamw_table_lrs",
                                        "segmm_adamw_table"))
    assert names.index("segmm_adamw_hist_push_ema") < names.index("segmm_adamw_table_lazy_rows_ema") < names.index("segmm_ema_update")
    for tr in (dense, lazy):
        tr.train_step(_short())
    assert lazy.opt.tables_pending > 0
    lazy.opt.flush_tables()
    assert _equal(_snap(dense), _snap(lazy)) and _ema_sd_equal(dense, lazy)
    lazy.ema.decay = 0.95
    with pytest.raises(RuntimeError, match="hyperparameters changed"):
        lazy.run_recorded(_batches()[0])


@pytest.mark.parametrize("recorded", [False, True], ids=["eager", "recorded"])
def test_trainer_clipped_scheduled_grouped(recorded):
    """max_grad_norm, a cosine schedule with warm-up and the table in a group of its own at lr_scale 0.5 / decay 0.05; eagerly also
    ``ema.decay`` assigned ahead of step 12 with rows pending and no flush (the ring holds the weight each step used)."""
    kw = dict(device_state=True, max_grad_norm=0.05, lr_schedule=SCHED, groups=[{"params": [TABLE], "lr_scale": 0.5, "weight_decay": 0.05}])
    dense, lazy = _pair(**kw)
    _run(dense, 1, 11)
    _run(lazy, 1, 11, recorded_from=3 if recorded else None)
    if not recorded:
        pending = lazy.opt.tables_pending
        dense.ema.decay = lazy.ema.decay = 0.5
        _run(dense, 12, N_STEPS)
        _run(lazy, 12, 12)
        assert pending > 0 and lazy.opt.tables_pending == pending + 1          # (no flush stood in)
        _run(lazy, 13, N_STEPS)
    else:
        _run(dense, 12, N_STEPS)
        for t in range(12, N_STEPS + 1):
            lazy.run_recorded(_batches()[t - 1])
    lazy.opt.flush_tables()
    assert _equal(_snap(dense), _snap(lazy)) and _ema_sd_equal(dense, lazy)


def test_trainer_micro_batched():
    dense, lazy = _pair(micro_batch=8)
    _run(dense, 1, N_STEPS)
    _run(lazy, 1, N_STEPS)
    assert lazy.opt.tables_pending == 4
    lazy.opt.flush_tables()
    assert _equal(_snap(dense), _snap(lazy)) and _ema_sd_equal(dense, lazy)


def test_ema_validation_with_rows_pending():
    """``valid_model(ema=True)`` with rows pending flushes first: the dense run's metrics exactly, and training goes on bit-identically."""
    dense, lazy = _pair()
    _run(dense, 1, 13)
    _run(lazy, 1, 13)
    assert lazy.opt.tables_pending == 5
    vb = _batches()[N_STEPS + 1:N_STEPS + 3]
    got, want = lazy.valid_model(vb, permutation=0, ema=True), dense.valid_model(vb, permutation=0, ema=True)
    assert got == want and got != dense.valid_model(vb, permutation=0)
    assert lazy.opt.tables_pending == 0 and _equal(_snap(dense), _snap(lazy))
    _run(dense, 14, N_STEPS)
    _run(lazy, 14, N_STEPS)
    assert lazy.opt.tables_pending > 0
    lazy.opt.flush_tables()
    assert _equal(_snap(dense), _snap(lazy))


def test_checkpoint_round_trip_equals_the_dense_one(tmp_path):
    """``CheckPointer.save_checkpoint`` with rows pending: the file is the dense trainer's entry for entry, ``"model_ema"`` included; a
    fresh lazy trainer that loads it continues as the uninterrupted dense run."""
    from segmminterest_amd.trainer import CheckPointer
    dense, lazy = _pair()
    _run(dense, 1, 12)
    _run(lazy, 1, 12)
    assert lazy.opt.tables_pending == 4
    files = []
    for tag, tr in (("dense", dense), ("lazy", lazy)):
        ck = CheckPointer("main_metric", str(tmp_path / tag), mode="max")
        ck.save_checkpoint(tr.model, tr.opt, 1, {"main_metric": 0.5}, ema=tr.ema)
        files.append(torch.load(ck.ckpt_latest, map_location="cpu", weights_only=False))
    d, l = files
    assert set(d) == set(l) and "model_ema" in l
    for key in ("model", "model_ema"):
        assert list(d[key]) == list(l[key]) and all(_same(d[key][k], l[key][k]) for k in d[key]), key
    assert any(not _same(l["model"][k], l["model_ema"][k]) for k in l["model"])
    assert d["optimizer"]["param_groups"] == l["optimizer"]["param_groups"] and set(d["optimizer"]["state"]) == set(l["optimizer"]["state"])
    assert all(_same(d["optimizer"]["state"][i][k], l["optimizer"]["state"][i][k]) for i in d["optimizer"]["state"] for k in ("exp_avg", "exp_avg_sq"))
    second = _trainer(lazy_tables=dict(LAZY))
    _run(second, 1, 2)          # (its tables are registered and rows are pending when the checkpoint arrives)
    second.opt.flush_tables()
    ck.load_checkpoint(second.model, second.opt, ema=second.ema)
    torch.cuda.synchronize()
    assert second.opt.step_count == 12 and second.opt.tables_pending == 0
    _run(dense, 13, N_STEPS)
    _run(second, 13, N_STEPS)
    second.opt.flush_tables()
    assert _equal(_snap(dense), _snap(second))


def test_frozen_table_launches_nothing_and_keeps_shadow_equal_to_p():
    lazy = _trainer(lazy_tables=dict(LAZY), groups=[{"params": [TABLE], "frozen": True}])
    t0 = lazy.model.get_parameter(TABLE).detach().clone()
    _run(lazy, 1, 3)
    torch.cuda.synchronize()
    assert not lazy.opt._lazy and lazy.opt.tables_pending == 0 and _same(lazy.model.get_parameter(TABLE), t0)
    assert _same(_table_rows(lazy, lazy.ema.shadow), t0.reshape(-1))


def test_the_key_without_an_ema_is_todays_lazy_trainer():
    with_key, without = _trainer(ema=None, lazy_tables=dict(LAZY)), _trainer(ema=None, lazy_tables=dict(flush_every=8))
    _run(with_key, 1, 6)
    _run(without, 1, 6)
    torch.cuda.synchronize()
    assert with_key.ema is None and with_key.opt.tables_pending == without.opt.tables_pending == 6
    for a, b in zip((with_key.model._store.flat, with_key.opt.m, with_key.opt.v), (without.model._store.flat, without.opt.m, without.opt.v)):
        assert _same(a, b)
