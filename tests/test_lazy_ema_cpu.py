"""Lazy id tables beside the weight average (lazy_tables=dict(ema=True)), without a GPU:
* the three new entry points are exported under ABI version 30, dispatchable and refuse bad arguments before any launch;
* the key is validated, and without it both old refusals of lazy tables + EMA still raise, naming ``ema`` and the key;
* the host protocol of FusedAdamW / WeightEMA against a fake ``hipabi`` that notes the launches: the launch sequence of one step,
  the periodic flush, the flush ahead of ``applied()`` / ``state_dict()`` / ``load_state_dict()``, the key without an EMA."""
import pytest
import torch

TABLE = "backbone1.vid_proj.weight"
T_OFF, T_ROWS, T_W = 32, 20, 8          # the table sits in the middle of the live range
N_LIVE = 224


# ------------------------------------------------------------------------------------------------ the C ABI
def _H():
    from segmminterest_amd import hipabi as H
    H.lib()
    return H


NEW = ("segmm_adamw_hist_push_ema", "segmm_adamw_table_catchup_ema", "segmm_adamw_table_lazy_rows_ema")


def test_entry_points_exported_and_dispatchable_under_version_30():
    H = _H()
    from segmminterest_amd import _abi
    assert _abi.ABI_VERSION == 30 and H._lib_real().segmm_abi_version() == 30
    ops = H.op_ids()
    for name in NEW:
        assert name in H.SIGNATURES and name in ops, name
        assert len(H.SIGNATURES[name]) - 1 <= H.CMD_MAX_ARGS
    for old in ("segmm_adamw_hist_push", "segmm_adamw_table_catchup", "segmm_adamw_table_lazy_rows", "segmm_ema_update"):
        assert old in ops, old
    names = list(H.PARAMS["segmm_adamw_table_catchup_ema"])
    assert names[:4] == ["p", "m", "v", "shadow"] and "flags" not in names
    assert list(H.PARAMS["segmm_adamw_hist_push_ema"])[-3:-1] == ["ema_weight", "ema_warmup"]


def test_entry_points_reject_bad_arguments():
    """Refused on the host, before any launch: the checks of the three siblings, a missing / misaligned / overlapping shadow, an
    EMA weight outside (0, 1]."""
    H = _H()
    L_ = H._lib_real()
    buf, far = 1 << 20, 1 << 24          # (aligned, never dereferenced addresses: every call below is refused first)
    for bad in ((None, 4, 1e-3, 0.9, 0.999, 1, 0.01, 1, None), (buf, 0, 1e-3, 0.9, 0.999, 1, 0.01, 1, None),
                (buf, 4, 1e-3, 0.9, 0.999, 0, 0.01, 1, None), (buf, 4, -1.0, 0.9, 0.999, 3, 0.01, 1, None),
                (buf, 4, 1e-3, 0.9, 0.999, 1, 0.0, 1, None), (buf, 4, 1e-3, 0.9, 0.999, 1, 1.5, 0, None)):
        assert L_.segmm_adamw_hist_push_ema(*bad) != 0, bad
        assert b"adamw_hist_push_ema" in L_.segmm_last_error()

    def call(fn, ok, **kw):
        names = list(H.PARAMS[fn])
        args = list(ok)
        for k, v in kw.items():
            args[names.index(k)] = v
        return getattr(L_, fn)(*args)
    ok_c = (buf, buf, buf, far, 10, 8, buf, 4, buf, buf, 4, 3, 0, 1.0, 0.9, 0.999, 1e-8, 0.0, None)
    for bad in (dict(p=None), dict(stamps=None), dict(hist=None), dict(m=buf + 4), dict(width=6), dict(cap=0), dict(target=-1),
                dict(relative=1, target=2), dict(lr_scale=-1.0), dict(shadow=None), dict(shadow=far + 4), dict(shadow=buf),
                dict(shadow=buf + 16), dict(shadow=buf - 16)):
        assert call("segmm_adamw_table_catchup_ema", ok_c, **bad) != 0, bad
        assert b"adamw_table_catchup_ema" in L_.segmm_last_error()
    ok_r = (buf, buf, buf, buf, far, 10, 8, buf, 4, buf, buf, 4, 1e-3, 1.0, 0.9, 0.999, 1e-8, 0.0, 3, None, None)
    for bad in (dict(p=None), dict(g=None), dict(ids=None), dict(hist=None), dict(v=buf + 4), dict(width=6), dict(cap=0), dict(step=0),
                dict(lr=-1.0), dict(lr_scale=-1.0), dict(shadow=None), dict(shadow=far + 8), dict(shadow=buf), dict(shadow=buf + 10 * 8 * 4 - 16)):
        assert call("segmm_adamw_table_lazy_rows_ema", ok_r, **bad) != 0, bad
        assert b"adamw_table_lazy_rows_ema" in L_.segmm_last_error()


# ------------------------------------------------------------------------------------------------ the host protocol
class FakeH:
    """Notes the launches FusedAdamW and WeightEMA make; nothing runs."""
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
        self.head = torch.nn.Parameter(torch.zeros(T_OFF))
        self.table = torch.nn.Parameter(torch.zeros(T_ROWS, T_W))
        self.other = torch.nn.Parameter(torch.zeros(32))
        self.flat, self.gflat = torch.zeros(N_LIVE), torch.zeros(N_LIVE)
        self.n_live, self.fused_version, self.direct_grads = N_LIVE, 0, True
        self.index = {"a": (0, T_OFF), TABLE: (T_OFF, T_ROWS * T_W), "w": (T_OFF + T_ROWS * T_W, 32)}
        self.live_names = ["a", TABLE, "w"]
        self._params = {"a": self.head, TABLE: self.table, "w": self.other}

    def ensure(self):
        pass


class FakeModel:
    def __init__(self):
        self._store = FakeStore()

    def named_parameters(self):
        return [(n, self._store._params[n]) for n in self._store.live_names]

    def parameters(self):
        return [p for _, p in self.named_parameters()]

    def state_dict(self):
        return dict(self.named_parameters())


@pytest.fixture
def fake(monkeypatch):
    from segmminterest_amd import optim
    h = FakeH()
    monkeypatch.setattr(optim, "H", h)
    return optim, h


IDS = torch.tensor([1, 2, 2], dtype=torch.int64)


def _ema_step(opt, ids=IDS):
    opt.lazy_step_head()
    opt.table_lazy(TABLE, ids, mark=False)
    opt.step(lazy_rows={TABLE: ids})


@pytest.mark.parametrize("bad", [1, 0, "yes", None, 1.0])
def test_the_key_is_validated(bad):
    from segmminterest_amd import optim
    assert "ema" in optim.LAZY_KEYS
    with pytest.raises(ValueError, match="lazy_tables: ema must be a bool"):
        optim.FusedAdamW(FakeModel(), lazy_tables=dict(ema=bad))
    with pytest.raises(ValueError, match="lazy_tables: ema must be a bool"):
        optim.parse_lazy_ema(dict(ema=bad))


def test_the_key_resolves_and_combines():
    from segmminterest_amd import optim
    assert optim.parse_lazy_ema(None) is False and optim.parse_lazy_ema(True) is False and optim.parse_lazy_ema(dict(flush_every=3)) is False
    opt = optim.FusedAdamW(FakeModel(), ema=0.99, lazy_tables=dict(ema=True, flush_every=3, data_parallel=True))
    assert opt.lazy_ema is True and opt.lazy_flush_every == 3 and opt.lazy_data_parallel is True
    assert optim.FusedAdamW(FakeModel(), ema=0.99, lazy_tables=True).lazy_ema is False
    assert optim.FusedAdamW(FakeModel(), lazy_tables=dict(ema=True)).lazy_flush_every == optim.LAZY_FLUSH_EVERY


def test_without_the_key_both_refusals_still_raise_and_name_the_key(fake):
    optim, h = fake
    for spec in (True, dict(flush_every=4), dict(ema=False)):
        opt = optim.FusedAdamW(FakeModel(), lazy_tables=spec, ema=0.99)
        with pytest.raises(RuntimeError, match=r"lazy_tables with ema.*lazy_tables=dict\(ema=True\)"):
            opt.table_lazy(TABLE, IDS)
    assert "adamw_table_catchup" not in h.names()
    from segmminterest_amd.trainer import Trainer
    import types
    bb = types.SimpleNamespace(id_vid=True)
    model = types.SimpleNamespace(backbone1=bb)
    with pytest.raises(ValueError, match=r"with ema.*lazy_tables=dict\(ema=True\)"):
        Trainer(model, lazy_tables=True, ema=0.99)
    with pytest.raises(ValueError, match="lazy_tables: ema must be a bool"):
        Trainer(model, lazy_tables=dict(ema=1), ema=0.99)


def test_launch_sequence_of_one_step(fake):
    """In order: the catch-up with the shadow at the head; the dense AdamW ranges around the table; the ring's entry with w_T; the
    fused rows launch with the shadow; the EMA's update over the live range minus the table."""
    optim, h = fake
    opt = optim.FusedAdamW(FakeModel(), ema=dict(decay=0.99, warmup=True), lazy_tables=dict(ema=True, flush_every=3))
    n_tab = T_ROWS * T_W
    for k in range(3):
        _ema_step(opt)
        calls = h.calls
        assert h.names() == ["adamw_table_catchup_ema", "adamw", "adamw", "adamw_hist_push_ema", "adamw_table_lazy_rows_ema",
                             "ema_update", "ema_update"], k
        head, a0, a1, push, rows, e0, e1 = calls
        # head: (p, m, v, shadow, off, shadow_off, n_rows, width, ids, stamps, hist, target, ...): target T - 1, no flags anywhere
        assert head[1][3] is opt.ema.shadow and head[1][4:8] == (T_OFF, T_OFF, T_ROWS, T_W) and head[1][8] is IDS and head[1][11] == k
        assert "flags" not in head[2]
        # the dense ranges: [0, T_OFF) and [T_OFF + n_tab, N_LIVE)
        assert (a0[1][4], a0[2]["p_off"]) == (T_OFF, 0) and (a1[1][4], a1[2]["p_off"]) == (N_LIVE - T_OFF - n_tab, T_OFF + n_tab)
        # the ring's entry: step T, the EMA's weight and warm-up flag
        assert push[1][4:] == (k + 1, opt.ema.weight, True)
        assert rows[1][4] is opt.ema.shadow and rows[1][5:9] == (T_OFF, T_OFF, T_ROWS, T_W) and rows[1][9] is IDS and rows[1][-1] == k + 1
        # the EMA around the table, with the step's weight
        for e, (o, n) in zip((e0, e1), ((0, T_OFF), (T_OFF + n_tab, N_LIVE - T_OFF - n_tab))):
            assert e[1][2:] == (n, opt.ema.weight, True, k + 1) and e[2] == dict(shadow_off=o, p_off=o)
        assert opt.tables_pending == k + 1 and opt._lazy_tail == {}
    assert opt._lazy_hist.shape == (3, 4)
    _ema_step(opt)          # three steps are pending: the ring holds no more -- the flush (ids None, target 3) comes first
    calls = h.calls
    assert h.names()[:2] == ["adamw_table_catchup_ema", "adamw_table_catchup_ema"]
    assert calls[0][1][8] is None and calls[0][1][11] == 3 and calls[0][1][3] is opt.ema.shadow and calls[1][1][8] is IDS
    assert opt.tables_pending == 1


def test_marked_head_is_refused_in_this_mode(fake):
    optim, h = fake
    opt = optim.FusedAdamW(FakeModel(), ema=0.99, lazy_tables=dict(ema=True))
    with pytest.raises(RuntimeError, match="mark=False"):
        opt.table_lazy(TABLE, IDS)
    assert h.names() == []


def test_whole_shadow_reads_flush_first(fake):
    optim, h = fake
    model = FakeModel()
    opt = optim.FusedAdamW(model, ema=0.99, lazy_tables=dict(ema=True, flush_every=8))
    _ema_step(opt)
    _ema_step(opt)
    h.names()
    assert opt.tables_pending == 2
    with opt.ema.applied():
        assert h.names() == ["adamw_table_catchup_ema", "vec_swap"] and opt.tables_pending == 0
    assert h.names() == ["vec_swap"]
    _ema_step(opt)
    h.names()
    sd = opt.ema.state_dict()
    assert h.names() == ["adamw_table_catchup_ema"] and opt.tables_pending == 0
    _ema_step(opt)
    h.names()
    opt.ema.load_state_dict(sd)
    assert h.names() == ["adamw_table_catchup_ema"] and opt.tables_pending == 0
    _ema_step(opt)
    h.names()
    opt.flush_tables()
    opt.flush_tables()
    assert h.names() == ["adamw_table_catchup_ema"]
    _ema_step(opt)
    h.names()
    opt.state_dict()
    assert h.names() == ["adamw_table_catchup_ema"]


def test_flush_inside_a_recording_is_refused(fake):
    optim, h = fake
    opt = optim.FusedAdamW(FakeModel(), ema=0.99, lazy_tables=dict(ema=True))
    _ema_step(opt)
    h.RECORDER = object()
    try:
        with pytest.raises(RuntimeError, match="recorded step"):
            opt.ema.state_dict()
    finally:
        h.RECORDER = None


def test_a_dense_step_of_the_lazy_table_averages_it_densely(fake):
    """``step()`` for a lazy table that did not come through ``table_lazy`` (nothing pending): one AdamW launch and ONE EMA launch over
    the whole live range, then every stamp is set."""
    optim, h = fake
    opt = optim.FusedAdamW(FakeModel(), ema=0.99, lazy_tables=dict(ema=True))
    _ema_step(opt)
    opt.flush_tables()
    h.names()
    opt.step()
    calls = h.calls
    assert h.names() == ["adamw", "adamw_table_stamp", "ema_update"]
    assert calls[2][1][2] == N_LIVE and calls[2][2] == {}
    _ema_step(opt)
    h.names()
    with pytest.raises(RuntimeError, match="flush_tables\\(\\) BEFORE a forward"):
        opt.step()


def test_the_key_without_an_ema_makes_todays_launches(fake):
    optim, h = fake
    seqs = []
    for spec in (dict(flush_every=3), dict(flush_every=3, ema=True)):
        opt = optim.FusedAdamW(FakeModel(), lazy_tables=spec)
        assert opt.ema is None
        seq = []
        for _ in range(4):
            opt.lazy_step_head()
            opt.table_lazy(TABLE, IDS)
            opt.step()
            seq.append(h.names())
        opt.lazy_step_head()
        opt.table_lazy(TABLE, IDS, mark=False)
        opt.step(lazy_rows={TABLE: IDS})
        seq.append(h.names())
        opt.flush_tables()
        seq.append(h.names())
        seqs.append(seq)
    assert seqs[0] == seqs[1]
    assert seqs[0][0] == ["adamw_table_catchup", "adamw", "adamw_hist_push", "adamw_table", "adamw_table_stamp", "adamw"]
    assert seqs[0][4] == ["adamw_table_catchup", "adamw", "adamw", "adamw_hist_push", "adamw_table_lazy_rows"]
    assert not any("_ema" in n or n == "ema_update" for s in seqs[0] for n in s)


def test_an_ema_without_lazy_tables_makes_one_update_launch(fake):
    optim, h = fake
    opt = optim.FusedAdamW(FakeModel(), ema=0.99)
    opt.step()
    calls = h.calls
    assert h.names() == ["adamw", "ema_update"] and calls[1][1][2] == N_LIVE and calls[1][2] == {}


def test_a_frozen_table_launches_nothing(fake):
    optim, h = fake
    opt = optim.FusedAdamW(FakeModel(), ema=0.99, lazy_tables=dict(ema=True), param_groups=[{"params": [TABLE], "frozen": True}])
    opt.lazy_step_head()
    opt.table_lazy(TABLE, IDS, mark=False)
    opt.step()
    names = h.names()
    assert not any(n.startswith("adamw_table") or n.startswith("adamw_hist") for n in names) and names.count("ema_update") == 1
    assert not opt._lazy and opt.tables_pending == 0
