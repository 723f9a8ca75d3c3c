"""Lazy exact AdamW of the id tables, without a GPU:
* the protocol's host statement (tests/lazy_table_ref.py) equals the dense update in every bit of p, m and v, and rejects every
  planted defect -- which is what makes the bitwise GPU comparisons of tests/test_lazy_tables_gpu.py a test of the protocol's order;
* the new entry points are exported, dispatchable and refuse bad arguments before any launch;
* the host logic of FusedAdamW(lazy_tables=...) -- refusals, the periodic flush, the hyperparameter snapshot, the flush points --
  against a fake ``hipabi`` that notes the launches."""
import numpy as np
import pytest
import torch

import adamw_ref as A
import lazy_table_ref as L

F = np.float32
ROWS, WIDTH, STEPS, FLUSH_EVERY, NEVER = 37, 8, 40, 8, 5
HP = dict(b1=0.9, b2=0.999, eps=1e-8, wd=1e-2)


def _bits(x):
    return np.ascontiguousarray(x, dtype=F).view(np.uint32)


def _case():
    rng = np.random.default_rng(7)
    p0 = (0.1 * rng.standard_normal((ROWS, WIDTH))).astype(F)
    m0 = (0.1 * rng.standard_normal((ROWS, WIDTH))).astype(F)
    v0 = (0.01 * rng.uniform(0.25, 1.0, size=(ROWS, WIDTH))).astype(F)
    rates = [F(1e-3 * (1.0 + 0.5 * np.cos(0.7 * k)) + 1e-5 * k) for k in range(STEPS)]          # another rate every step
    id_lists, grads = [], []
    for k in range(STEPS):
        ids = rng.integers(0, ROWS, size=6)
        ids[ids == NEVER] = NEVER + 1          # one row is never listed: it takes all 40 steps from the ring, flush by flush
        ids = np.concatenate([ids, ids[:2], [-1, ROWS, ROWS + 9, -2 ** 40]])          # duplicates; ids outside the table
        id_lists.append(ids)
        grads.append(L.dense_grad(rng.standard_normal((ROWS, WIDTH)).astype(F), ids, ROWS))
    return p0, m0, v0, rates, id_lists, grads


def _lazy(defect=None):
    p0, m0, v0, rates, id_lists, grads = _case()
    t = L.LazyTable(p0, m0, v0, FLUSH_EVERY, HP, defect=defect)
    for ids, g, lr in zip(id_lists, grads, rates):
        t.step(ids, g, lr)
    t.flush()
    return t


def test_protocol_equals_the_dense_update_bit_for_bit():
    p0, m0, v0, rates, id_lists, grads = _case()
    assert len(set(float(r) for r in rates)) == STEPS and not any(NEVER in ids for ids in id_lists)
    dense = L.dense_run(p0, m0, v0, grads, rates, HP)
    t = L.LazyTable(p0, m0, v0, FLUSH_EVERY, HP)
    for k, (ids, g, lr) in enumerate(zip(id_lists, grads, rates)):
        t.step(ids, g, lr)
        assert t.pending <= FLUSH_EVERY
        rows = sorted(set(int(r) for r in ids if 0 <= r < ROWS))          # the batch's rows are current after their step
        for got, want in zip((t.p, t.m, t.v), dense[k]):
            assert np.array_equal(_bits(got[rows]), _bits(want[rows])), k
    assert t.stamps[NEVER] < STEPS
    t.flush()
    assert t.n_flushes >= 5 and (t.stamps == STEPS).all()          # the ring of 8 wrapped five times over 40 steps
    for name, got, want in zip("pmv", (t.p, t.m, t.v), dense[-1]):
        assert np.array_equal(_bits(got), _bits(want)), name


@pytest.mark.parametrize("defect", L.DEFECTS)
def test_planted_defects_are_rejected(defect):
    p0, m0, v0, rates, id_lists, grads = _case()
    want = L.dense_run(p0, m0, v0, grads, rates, HP)[-1]
    t = _lazy(defect)
    assert not all(np.array_equal(_bits(g), _bits(w)) for g, w in zip((t.p, t.m, t.v), want)), defect


# ------------------------------------------------------------------------------------------------ the C ABI
def _H():
    from segmminterest_amd import hipabi as H
    H.lib()
    return H


NEW = ("segmm_adamw_hist_push", "segmm_adamw_table_catchup", "segmm_adamw_table_stamp")


def test_entry_points_exported_and_dispatchable():
    H = _H()
    ops = H.op_ids()
    for name in NEW:
        assert name in H.SIGNATURES and name in ops, name
        assert len(H.SIGNATURES[name]) - 1 <= H.CMD_MAX_ARGS


def test_entry_points_reject_bad_arguments():
    """Refused on the host, before any launch (no device is touched): null / misaligned pointers, a width that is no multiple of
    4, cap < 1, a target out of its range, a live rate without the device step state."""
    L_ = _H()._lib_real()
    buf = 1 << 20          # (an aligned, never dereferenced address: every call below is refused first)
    assert L_.segmm_adamw_hist_push(None, 4, 1e-3, 0.9, 0.999, 1, None) != 0
    assert L_.segmm_adamw_hist_push(buf, 0, 1e-3, 0.9, 0.999, 1, None) != 0
    assert L_.segmm_adamw_hist_push(buf, 4, 1e-3, 0.9, 0.999, 0, None) != 0
    assert L_.segmm_adamw_hist_push(buf, 4, -1.0, 0.9, 0.999, 3, None) != 0
    ok = (buf, buf, buf, 10, 8, buf, 4, buf, None, buf, 4, 3, 0, 1.0, 0.9, 0.999, 1e-8, 0.0, None)

    def catchup(**kw):
        names = [p for p in _H().PARAMS["segmm_adamw_table_catchup"]]
        args = list(ok)
        for k, v in kw.items():
            args[names.index(k)] = v
        return L_.segmm_adamw_table_catchup(*args)
    for bad in (dict(p=None), dict(stamps=None), dict(hist=None), dict(m=buf + 4), dict(width=6), dict(cap=0), dict(target=-1),
                dict(relative=1, target=2), dict(relative=1, target=-2), dict(lr_scale=-1.0), dict(ids=None, flags=buf)):
        assert catchup(**bad) != 0, bad
        assert b"adamw_table_catchup" in L_.segmm_last_error()
    assert L_.segmm_adamw_table_stamp(buf, 4, 10, None, 3, 0, None) != 0
    assert L_.segmm_adamw_table_stamp(buf, 4, 10, buf, -1, 0, None) != 0
    assert L_.segmm_adamw_table_stamp(buf, 4, 10, buf, 1, 1, None) != 0


# ------------------------------------------------------------------------------------------------ FusedAdamW's host logic
TABLE = "backbone1.vid_proj.weight"


class FakeH:
    """Notes the launches FusedAdamW makes; nothing runs."""
    LIVE_LR, RECORDER = -1.0, None

    def __init__(self):
        self.calls = []

    def torch_fallback(self, what):
        pass

    def __getattr__(self, name):
        def call(*a, **kw):
            self.calls.append((name, a, kw))
        return call

    def names(self):
        out = [c[0] for c in self.calls]
        self.calls = []
        return out


class FakeStore:
    def __init__(self):
        self.table = torch.nn.Parameter(torch.zeros(20, 8))
        self.other = torch.nn.Parameter(torch.zeros(32))
        self.flat, self.gflat = torch.zeros(192), torch.zeros(192)
        self.n_live, self.fused_version, self.direct_grads = 192, 0, True
        self.index = {TABLE: (0, 160), "w": (160, 32)}
        self.live_names = [TABLE, "w"]
        self._params = {TABLE: self.table, "w": self.other}

    def ensure(self):
        pass


class FakeModel:
    def __init__(self):
        self._store = FakeStore()

    def named_parameters(self):
        return [(TABLE, self._store.table), ("w", self._store.other)]

    def parameters(self):
        return [p for _, p in self.named_parameters()]


@pytest.fixture
def fake(monkeypatch):
    from segmminterest_amd import optim
    h = FakeH()
    monkeypatch.setattr(optim, "H", h)
    return optim, h


def _lazy_step(opt, ids=None):
    opt.lazy_step_head()
    opt.table_lazy(TABLE, torch.tensor([1, 2, 2] if ids is None else ids, dtype=torch.int64))
    opt.step()


@pytest.mark.parametrize("bad,word", [(dict(flush_every=0), "flush_every"), (dict(flush_every=True), "flush_every"), (dict(flush_every=2.0), "flush_every"),
                                      (dict(flush=8), "unknown key 'flush'"), (False, "lazy_tables"), (8, "lazy_tables")])
def test_lazy_tables_argument_is_validated(bad, word):
    from segmminterest_amd.optim import FusedAdamW
    with pytest.raises(ValueError, match=word):
        FusedAdamW(FakeModel(), lazy_tables=bad)


def test_lazy_tables_default_and_capacity():
    from segmminterest_amd import optim
    assert optim.FusedAdamW(FakeModel()).lazy_flush_every is None
    assert optim.FusedAdamW(FakeModel(), lazy_tables=True).lazy_flush_every == optim.LAZY_FLUSH_EVERY >= 1
    assert optim.FusedAdamW(FakeModel(), lazy_tables=dict(flush_every=3)).lazy_flush_every == 3


def test_default_mode_makes_todays_launches(fake):
    optim, h = fake
    opt = optim.FusedAdamW(FakeModel())
    opt.table_early(TABLE, torch.tensor([1, 2], dtype=torch.int64))
    opt.step()
    opt.flush_tables()
    opt.state_dict()
    assert h.names() == ["adamw_table", "adamw_table", "adamw"] and opt.tables_pending == 0


def test_ema_and_missing_argument_are_refused(fake):
    optim, h = fake
    with pytest.raises(RuntimeError, match="lazy_tables"):
        optim.FusedAdamW(FakeModel()).table_lazy(TABLE, torch.zeros(2, dtype=torch.int64))
    opt = optim.FusedAdamW(FakeModel(), lazy_tables=True, ema=0.99)
    with pytest.raises(RuntimeError, match="ema"):
        opt.table_lazy(TABLE, torch.zeros(2, dtype=torch.int64))


def test_step_protocol_and_periodic_flush(fake):
    optim, h = fake
    opt = optim.FusedAdamW(FakeModel(), lazy_tables=dict(flush_every=3))
    for k in range(3):
        _lazy_step(opt)
        # catch-up at the head; at the tail the ring's entry, phase 1 (never phase 0), the stamp, then the rest of the live range
        calls = h.calls
        assert h.names() == ["adamw_table_catchup", "adamw_hist_push", "adamw_table", "adamw_table_stamp", "adamw"], k
        assert calls[0][1][6] is not None and calls[0][1][9] == k and calls[2][1][15] == 1          # ids; target T - 1; phase
        assert opt.tables_pending == k + 1
    assert opt._lazy_hist.shape == (3, 4)
    _lazy_step(opt)          # three steps are pending: the ring holds no more -- the flush (ids None, target 3) comes first
    calls = h.calls
    assert h.names()[:2] == ["adamw_table_catchup", "adamw_table_catchup"]
    assert calls[0][1][6] is None and calls[0][1][9] == 3 and opt.tables_pending == 1
    opt.flush_tables()
    assert h.names() == ["adamw_table_catchup"] and opt.tables_pending == 0
    opt.flush_tables()
    assert h.names() == []          # nothing pending: nothing launched


def test_changed_hyperparameter_flushes_with_the_old_value(fake):
    optim, h = fake
    opt = optim.FusedAdamW(FakeModel(), weight_decay=0.25, lazy_tables=dict(flush_every=50))
    _lazy_step(opt)
    h.names()
    opt.lr = 5e-4          # the rate is in the ring: no flush
    _lazy_step(opt)
    assert h.names()[0] == "adamw_table_catchup" and opt.tables_pending == 2
    for change in (lambda: setattr(opt, "wd", 0.5), lambda: setattr(opt, "eps", 1e-6), lambda: setattr(opt, "betas", (0.8, 0.99))):
        old = (opt.betas[0], opt.betas[1], opt.eps, opt.wd)
        change()
        _lazy_step(opt)
        flush, head = h.calls[0], h.calls[1]
        assert h.names()[:2] == ["adamw_table_catchup", "adamw_table_catchup"]
        assert flush[1][6] is None and tuple(flush[1][11:15]) == old          # the flush replays the pending steps as they were taken
        assert tuple(head[1][11:15]) == (opt.betas[0], opt.betas[1], opt.eps, opt.wd) and opt.tables_pending == 1


def test_flush_points(fake):
    optim, h = fake
    opt = optim.FusedAdamW(FakeModel(), lazy_tables=dict(flush_every=50))
    _lazy_step(opt)
    _lazy_step(opt)
    h.names()
    sd = opt.state_dict()          # flushes first; no new keys
    assert h.names() == ["adamw_table_catchup"] and opt.tables_pending == 0
    assert set(sd) == {"state", "param_groups"} and set(sd["param_groups"][0]) == set(optim.FusedAdamW(FakeModel()).state_dict()["param_groups"][0])
    _lazy_step(opt)
    h.names()
    opt.load_state_dict(sd)          # what was pending is discarded: every stamp is SET to the loaded count
    calls = h.calls
    assert h.names() == ["adamw_table_stamp"] and calls[0][1][0] is None and calls[0][1][3] == opt.step_count == 2 and opt.tables_pending == 0
    _lazy_step(opt)
    st = opt.model._store
    st.flat = torch.zeros(192)          # the flat buffer is rebuilt: the moments are new, nothing is pending, the stamps are made again
    assert opt.tables_pending == 1
    opt._state()
    assert opt.tables_pending == 0 and not opt._lazy
    _lazy_step(opt)
    assert int(opt._lazy[TABLE]["stamps"].min()) == opt.step_count - 1          # (the fake ran no stamp launch)
    # a step whose forward did not go through table_lazy: with steps pending that forward read stale rows -- refused, nothing launched;
    # after a flush BEFORE the forward the table is stepped densely with the live range and every stamp is set to the step
    h.names()
    with pytest.raises(RuntimeError, match="flush_tables\\(\\) BEFORE a forward"):
        opt.step()
    assert h.names() == [] and opt.tables_pending == 1
    opt.flush_tables()
    count = opt.step_count
    opt.step()
    calls = h.calls
    assert h.names() == ["adamw_table_catchup", "adamw", "adamw_table_stamp"] and opt.tables_pending == 0 and opt.step_count == count + 1
    assert calls[2][1][0] is None and calls[2][1][3] == opt.step_count


def test_the_ring_rule_is_enforced_in_table_lazy(fake):
    """``table_lazy`` with ``flush_every`` steps pending would replay from an overwritten slot: refused, whoever forgot the head call."""
    optim, h = fake
    opt = optim.FusedAdamW(FakeModel(), lazy_tables=dict(flush_every=2))
    _lazy_step(opt)
    _lazy_step(opt)
    with pytest.raises(RuntimeError, match="2 steps are pending and the ring holds 2"):
        opt.table_lazy(TABLE, torch.tensor([1], dtype=torch.int64))
    opt.lazy_step_head()
    opt.table_lazy(TABLE, torch.tensor([1], dtype=torch.int64))


def test_a_flush_inside_a_recording_is_refused(fake):
    optim, h = fake
    opt = optim.FusedAdamW(FakeModel(), lazy_tables=dict(flush_every=50))
    _lazy_step(opt)
    h.RECORDER = object()
    with pytest.raises(RuntimeError, match="recorded step"):
        opt.flush_tables()
