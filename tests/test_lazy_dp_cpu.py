"""Lazy exact AdamW of the id tables under data parallelism, without a GPU:
* the host logic of FusedAdamW(lazy_tables=dict(data_parallel=True)) and of the trainer's three data-parallel tails against a fake
  ``hipabi`` that notes the launches: the head catches up the own ids and nothing else, the tail is one ring push and one
  segmm_adamw_table_lazy_rows on the gathered list, the dense ranges tile the live range minus the table;
* the new entry point is exported, dispatchable and refuses bad arguments before any launch;
* a numpy restatement of the fused row update (tests/lazy_table_ref.py's element step) equals the dense update bit for bit and
  rejects a wrong ring slot, a skipped step and a duplicate stepped twice -- which is what makes the bitwise comparisons of
  tests/test_lazy_dp_gpu.py a test of the kernel's order."""
import types

import numpy as np
import pytest
import torch

import lazy_table_ref as L

F = np.float32
TABLE = "backbone1.vid_proj.weight"
N_LIVE, T_OFF, T_ROWS, T_WIDTH = 224, 32, 20, 8          # a | the table | w
T_END = T_OFF + T_ROWS * T_WIDTH
LAZY_DP = dict(flush_every=3, data_parallel=True)


class FakeH:
    """Notes the launches FusedAdamW and the trainer make; nothing runs."""
    LIVE_LR, RECORDER, GRAD_NORM_SCRATCH = -1.0, None, 1024

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
        self.a = torch.nn.Parameter(torch.zeros(T_OFF))
        self.table = torch.nn.Parameter(torch.zeros(T_ROWS, T_WIDTH))
        self.other = torch.nn.Parameter(torch.zeros(N_LIVE - T_END))
        self.flat, self.gflat = torch.zeros(N_LIVE), torch.zeros(N_LIVE)
        self.n_live, self.fused_version, self.direct_grads = N_LIVE, 0, True
        self.index = {"a": (0, T_OFF), TABLE: (T_OFF, T_END - T_OFF), "w": (T_END, N_LIVE - T_END)}
        self.live_names = ["a", TABLE, "w"]
        self._params = {"a": self.a, TABLE: self.table, "w": self.other}
        self._tab_rows = {}

    def ensure(self):
        pass


class FakeModel:
    def __init__(self):
        self._store = FakeStore()

    def named_parameters(self):
        return [(n, self._store._params[n]) for n in self._store.live_names]

    def parameters(self):
        return [p for _, p in self.named_parameters()]


@pytest.fixture
def fake(monkeypatch):
    from segmminterest_amd import optim, trainer
    h = FakeH()
    monkeypatch.setattr(optim, "H", h)
    monkeypatch.setattr(trainer, "H", h)
    return optim, h


OWN = torch.tensor([1, 2, 2], dtype=torch.int64)
ALL = torch.tensor([1, 2, 2, 7, 9, 1], dtype=torch.int64)


def _adamw_ranges(calls):
    """[start, end) of the dense ``adamw`` launches among ``calls`` (hipabi.adamw(p, g, m, v, n, ..., p_off=start))."""
    return [(c[2]["p_off"], c[2]["p_off"] + c[1][4]) for c in calls if c[0] == "adamw"]


def _dp_step(opt, own=OWN, ids_all=ALL):
    opt.lazy_step_head()
    opt.table_lazy(TABLE, own, mark=False)
    opt.begin_step()
    opt.step_ranges(0, N_LIVE)
    opt.table_lazy_rows(TABLE, ids_all)
    opt.end_step()


# ------------------------------------------------------------------------------------------------ the key
@pytest.mark.parametrize("bad", [1, 0, "yes", None])
def test_data_parallel_key_is_validated(bad):
    from segmminterest_amd.optim import FusedAdamW
    with pytest.raises(ValueError, match="data_parallel must be a bool"):
        FusedAdamW(FakeModel(), lazy_tables=dict(data_parallel=bad))


def test_data_parallel_key_default_and_combination():
    from segmminterest_amd import optim
    assert optim.parse_lazy_tables(dict(data_parallel=True)) == optim.LAZY_FLUSH_EVERY          # (the return value is flush_every, as ever)
    assert optim.parse_lazy_tables(LAZY_DP) == 3
    assert optim.FusedAdamW(FakeModel()).lazy_data_parallel is False
    assert optim.FusedAdamW(FakeModel(), lazy_tables=True).lazy_data_parallel is False
    assert optim.FusedAdamW(FakeModel(), lazy_tables=dict(flush_every=3)).lazy_data_parallel is False
    opt = optim.FusedAdamW(FakeModel(), lazy_tables=LAZY_DP)
    assert opt.lazy_data_parallel is True and opt.lazy_flush_every == 3


# ------------------------------------------------------------------------------------------------ the C ABI
def _H():
    from segmminterest_amd import hipabi as H
    H.lib()
    return H


def test_entry_point_exported_and_dispatchable():
    H = _H()
    name = "segmm_adamw_table_lazy_rows"
    assert name in H.SIGNATURES and name in H.op_ids()
    assert len(H.SIGNATURES[name]) - 1 <= H.CMD_MAX_ARGS
    assert callable(H.adamw_table_lazy_rows)


def test_entry_point_rejects_bad_arguments():
    """Refused on the host, before any launch (no device is touched)."""
    H = _H()
    L_ = H._lib_real()
    buf = 1 << 20          # (an aligned, never dereferenced address: every call below is refused first)
    names = list(H.PARAMS["segmm_adamw_table_lazy_rows"])
    ok = dict(p=buf, g=buf, m=buf, v=buf, n_rows=10, width=8, ids=buf, n_ids=4, stamps=buf, hist=buf, cap=4, lr=1e-3, lr_scale=1.0,
              beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, step=3, coef=None, stream=None)
    assert names == list(ok)
    for bad in (dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(stamps=None), dict(hist=None), dict(ids=None), dict(g=buf + 4),
                dict(hist=buf + 8), dict(width=6), dict(width=0), dict(cap=0), dict(step=0), dict(step=-2), dict(lr=-1.0), dict(lr_scale=-0.5),
                dict(lr_scale=float("inf")), dict(lr_scale=float("nan"))):
        assert L_.segmm_adamw_table_lazy_rows(*[dict(ok, **bad)[k] for k in names]) != 0, bad
        assert b"adamw_table_lazy_rows" in L_.segmm_last_error()
    assert L_.segmm_adamw_table_lazy_rows(*[dict(ok, n_ids=0)[k] for k in names]) == 0          # nothing listed: nothing launched


# ------------------------------------------------------------------------------------------------ FusedAdamW's host logic
def test_one_data_parallel_lazy_step_launch_for_launch(fake):
    optim, h = fake
    opt = optim.FusedAdamW(FakeModel(), lazy_tables=LAZY_DP)
    opt.lazy_step_head()
    opt.table_lazy(TABLE, OWN, mark=False)
    calls = h.calls
    assert h.names() == ["adamw_table_catchup"]
    # the own ids, target T - 1 = 0, NO flags; nothing queued for step(), the table's range noted for the dense launches
    assert calls[0][1][6] is OWN and calls[0][1][9] == 0 and calls[0][2].get("flags") is None
    assert not opt.__dict__.get("_early") and opt._lazy_tail == {TABLE: (T_OFF, T_END - T_OFF)}
    opt.begin_step()
    opt.step_ranges(0, N_LIVE)
    opt.table_lazy_rows(TABLE, ALL)
    opt.end_step()
    calls = h.calls
    assert h.names() == ["adamw", "adamw", "adamw_hist_push", "adamw_table_lazy_rows"]
    assert _adamw_ranges(calls) == [(0, T_OFF), (T_END, N_LIVE)]
    rows_call = calls[3]
    assert rows_call[1][4:8] == (T_OFF, T_ROWS, T_WIDTH, ALL) and rows_call[1][-1] == 1 and rows_call[2] == dict(coef=None)          # step T = 1
    assert opt.tables_pending == 1 and not opt._lazy_tail and opt._lazy_snap == opt._lazy_hyper_now()


def test_ring_entry_is_pushed_once_per_step(fake):
    optim, h = fake
    opt = optim.FusedAdamW(FakeModel(), lazy_tables=LAZY_DP)
    opt.table_lazy(TABLE, OWN, mark=False)
    opt.begin_step()
    opt.table_lazy_rows(TABLE, ALL)
    opt.table_lazy_rows(TABLE, ALL)          # (a second table of the same step would come here)
    opt.end_step()
    assert h.names().count("adamw_hist_push") == 1
    _dp_step(opt)
    assert h.names().count("adamw_hist_push") == 1


def test_periodic_flush_after_flush_every_steps(fake):
    optim, h = fake
    opt = optim.FusedAdamW(FakeModel(), lazy_tables=LAZY_DP)
    for k in range(3):
        _dp_step(opt)
        assert h.names() == ["adamw_table_catchup", "adamw", "adamw", "adamw_hist_push", "adamw_table_lazy_rows"], k
        assert opt.tables_pending == k + 1
    _dp_step(opt)          # three steps pending, the ring holds three: the flush (ids None, target 3) comes first, on every rank alike
    calls = h.calls
    assert h.names()[:2] == ["adamw_table_catchup", "adamw_table_catchup"]
    assert calls[0][1][6] is None and calls[0][1][9] == 3 and calls[1][1][6] is OWN and opt.tables_pending == 1


def test_step_takes_the_gathered_list_and_refuses_to_skip_a_table(fake):
    optim, h = fake
    opt = optim.FusedAdamW(FakeModel(), lazy_tables=LAZY_DP)
    opt.table_lazy(TABLE, OWN, mark=False)
    h.names()
    with pytest.raises(RuntimeError, match="gathered id list"):
        opt.step()
    assert h.names() == [] and opt.step_count == 0
    opt.step(lazy_rows={TABLE: ALL})
    calls = h.calls
    assert h.names() == ["adamw", "adamw", "adamw_hist_push", "adamw_table_lazy_rows"] and _adamw_ranges(calls) == [(0, T_OFF), (T_END, N_LIVE)]
    with pytest.raises(RuntimeError, match="without table_lazy"):          # no head this step: the dense launches covered the range
        opt.begin_step()
        opt.table_lazy_rows(TABLE, ALL)


def test_frozen_table_launches_nothing(fake):
    optim, h = fake
    opt = optim.FusedAdamW(FakeModel(), lazy_tables=LAZY_DP, param_groups=[{"params": [TABLE], "frozen": True}])
    opt.lazy_step_head()
    opt.table_lazy(TABLE, OWN, mark=False)
    assert h.names() == [] and not opt._lazy and not opt._lazy_tail
    opt.begin_step()
    opt.step_ranges(0, N_LIVE)
    opt.table_lazy_rows(TABLE, ALL)
    opt.end_step()
    calls = h.calls
    assert h.names() == ["adamw_groups"] and calls[0][1][4:6] == (0, N_LIVE) and opt.tables_pending == 0


# ------------------------------------------------------------------------------------------------ the trainer's three tails
def _tail_trainer(optim, **kw):
    from segmminterest_amd.trainer import Trainer
    model = FakeModel()
    tr = object.__new__(Trainer)
    tr.model, tr.overlap, tr.per_bucket_adamw, tr.sparse_tables = model, True, True, False
    tr.comm = types.SimpleNamespace(active=True, finish=lambda: None, reduce_bucket=lambda *a: None, take_pending=lambda: [])
    tr.opt = optim.FusedAdamW(model, lazy_tables=LAZY_DP, **kw)
    tr._bucket_works = []
    model._store._tab_rows["backbone1.vid"] = (0, ALL)
    return tr


@pytest.mark.parametrize("tail", ["per_bucket", "per_bucket_interleaved", "clipped", "no_overlap", "no_per_bucket"])
def test_dense_ranges_tile_the_live_range_minus_the_table(fake, tail):
    """Per-bucket AdamW (a bucket boundary INSIDE the table too), the clipped single range and the opt.step() tails: the dense
    launches cover [0, n_live) minus the table exactly once, and the table takes one ring push and one lazy_rows launch on the
    gathered list the backward left in the store."""
    optim, h = fake
    tr = _tail_trainer(optim, **(dict(max_grad_norm=1.0) if tail == "clipped" else {}))
    cut = T_OFF + 40          # (no parameter boundary: the helper must cope)
    if tail == "per_bucket_interleaved":
        tr._bucket_works = [(cut, N_LIVE, []), (0, 16, []), (16, cut, [])]
    else:
        tr._bucket_works = [(cut, N_LIVE, []), (0, cut, [])]
    tr.overlap = tail != "no_overlap"
    tr.per_bucket_adamw = tail != "no_per_bucket"
    tr.opt.table_lazy(TABLE, OWN, mark=False)
    h.names()
    tr._finish_step({})
    calls = [c for c in h.calls if c[0] not in ("host_action", "mark")]
    names = [c[0] for c in calls]
    assert sorted(_adamw_ranges(calls)) in ([(0, T_OFF), (T_END, N_LIVE)], [(0, 16), (16, T_OFF), (T_END, N_LIVE)])
    assert names.count("adamw_hist_push") == 1 and names.count("adamw_table_lazy_rows") == 1
    assert names.index("adamw_hist_push") < names.index("adamw_table_lazy_rows")
    rows_call = calls[names.index("adamw_table_lazy_rows")]
    assert rows_call[1][7] is ALL
    if tail == "clipped":          # the norm first, the coefficient on every launch
        assert names[0] == "grad_norm" and rows_call[2]["coef"] is not None
        assert names.index("adamw_table_lazy_rows") > names.index("grad_norm")
    assert set(names) <= {"grad_norm", "adamw", "adamw_hist_push", "adamw_table_lazy_rows"}
    assert tr.opt.step_count == 1 and tr.opt.tables_pending == 1 and not tr.opt._lazy_tail


def test_a_missing_row_list_is_refused_by_name(fake):
    optim, h = fake
    tr = _tail_trainer(optim)
    tr.model._store._tab_rows.clear()
    tr._bucket_works = [(0, N_LIVE, [])]
    tr.opt.table_lazy(TABLE, OWN, mark=False)
    with pytest.raises(RuntimeError, match="no gathered row list for " + TABLE):
        tr._finish_step({})


# ------------------------------------------------------------------------------------------------ the fused row update, restated
ROWS, WIDTH, STEPS, CAP, NEVER = 37, 8, 24, 4, 5
HP = dict(b1=0.9, b2=0.999, eps=1e-8, wd=1e-2)
FUSED_DEFECTS = ("wrong_slot", "skip_step", "dup_twice")


def _bits(x):
    return np.ascontiguousarray(x, dtype=F).view(np.uint32)


def _case():
    rng = np.random.default_rng(17)
    p0 = (0.1 * rng.standard_normal((ROWS, WIDTH))).astype(F)
    m0 = (0.1 * rng.standard_normal((ROWS, WIDTH))).astype(F)
    v0 = (0.01 * rng.uniform(0.25, 1.0, size=(ROWS, WIDTH))).astype(F)
    rates = [F(1e-3 * (1.0 + 0.5 * np.cos(0.7 * k)) + 1e-5 * k) for k in range(STEPS)]          # another rate every step
    id_lists, grads = [], []
    for k in range(STEPS):
        ids = rng.integers(0, ROWS, size=6)
        ids[ids == NEVER] = NEVER + 1
        ids = np.concatenate([ids, ids[:2], [-1, ROWS, ROWS + 9, -2 ** 40]])          # duplicates; ids outside the table
        id_lists.append(ids)
        grads.append(L.dense_grad(rng.standard_normal((ROWS, WIDTH)).astype(F), ids, ROWS))
    return p0, m0, v0, rates, id_lists, grads


def _fused_rows(t, ids, g, lr, defect=None):
    """segmm_adamw_table_lazy_rows at step T = t.t + 1 on the state of a lazy_table_ref.LazyTable: the claim by the stamp, the
    replay of old + 1 .. T - 1 from the ring with g = 0, step T with the row of g, one stamp."""
    T = t.t + 1
    t.ring[T % t.cap] = t.newest = (F(lr), T)
    taken = set()
    for r in (int(r) for r in ids):
        if not 0 <= r < t.rows:
            continue
        old = int(t.stamps[r])
        if old >= T and not (defect == "dup_twice" and r in taken):
            continue
        taken.add(r)
        z = np.zeros_like(t.p[r])
        first = old + 1 + (1 if defect == "skip_step" and old + 1 < T else 0)
        for s in range(first, T):
            rate, count = t.ring[(s + (1 if defect == "wrong_slot" else 0)) % t.cap]
            t.p[r], t.m[r], t.v[r] = L.elem_step(t.p[r], t.m[r], t.v[r], z, max(count, 1), rate, t.hp, t.lr_scale)
        t.p[r], t.m[r], t.v[r] = L.elem_step(t.p[r], t.m[r], t.v[r], g[r], T, lr, t.hp, t.lr_scale)
        t.stamps[r] = T
    t.t = T


def _dp_run(defect=None):
    p0, m0, v0, rates, id_lists, grads = _case()
    t = L.LazyTable(p0, m0, v0, CAP, HP)
    reached = []
    for ids, g, lr in zip(id_lists, grads, rates):
        if t.pending >= CAP:
            t.flush()
        own = ids[:len(ids) // 3]
        t.catchup(own, t.t)          # the rank's own ids, ahead of the forward
        reached.append([t.t - int(t.stamps[r]) for r in set(int(r) for r in ids) if 0 <= r < ROWS])
        _fused_rows(t, ids, g, lr, defect)
    t.flush()
    return t, reached


def test_fused_row_update_equals_the_dense_update_bit_for_bit():
    p0, m0, v0, rates, id_lists, grads = _case()
    want = L.dense_run(p0, m0, v0, grads, rates, HP)[-1]
    t, reached = _dp_run()
    assert max(max(gaps) for gaps in reached if gaps) == CAP - 1 and (t.stamps == STEPS).all()          # the replay ran, up to the ring's reach
    for name, got, w in zip("pmv", (t.p, t.m, t.v), want):
        assert np.array_equal(_bits(got), _bits(w)), name


@pytest.mark.parametrize("defect", FUSED_DEFECTS)
def test_planted_defects_of_the_fused_update_are_rejected(defect):
    p0, m0, v0, rates, id_lists, grads = _case()
    want = L.dense_run(p0, m0, v0, grads, rates, HP)[-1]
    t, _ = _dp_run(defect)
    assert not all(np.array_equal(_bits(g), _bits(w)) for g, w in zip((t.p, t.m, t.v), want)), defect
