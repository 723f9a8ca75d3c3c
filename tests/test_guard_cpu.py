"""The non-finite guard (FusedAdamW / Trainer(skip_nonfinite=True)) without a GPU: the reference of a guarded step
(tests/guard_ref.py), the parsing and the refusals, the two counts through ``state_dict`` / ``load_state_dict`` -- into
torch.optim.AdamW too -- and the regenerated ABI tables."""
import math
import os

import numpy as np
import pytest
import torch

import adamw_ref as A
import guard_ref as G
from helpers import ROOT, build_model, load_case

F = np.float32
NEW = ("segmm_step_advance_guarded", "segmm_step_guard", "segmm_step_set_skipped", "segmm_step_get_skipped", "segmm_adamw_guarded",
       "segmm_adamw_groups_guarded", "segmm_adamw_table_lrs_guarded", "segmm_ema_update_guarded")


@pytest.fixture(scope="module")
def model():
    cfg, _, _, _ = load_case("img_d32_N2")
    return build_model(cfg)


# ------------------------------------------------------------------------------------------------ 1. the reference
def _grads(n, T, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(n).astype(F) for _ in range(T)]


@pytest.mark.parametrize("poison", [math.nan, math.inf, -math.inf])
def test_reference_skips_as_torch_does(poison):
    """Five gradients, the third with one poisoned element: the guarded run equals the unguarded run over the four clean gradients
    (torch: state["step"] moves on applied steps only), bit for bit; the skipped step returns the arrays themselves."""
    n, hp = 1027, dict(A.HP)
    grads = _grads(n, 5, 3)
    bad = grads[2].copy()
    bad[517] = poison
    p0 = (0.01 * np.random.default_rng(1).standard_normal(n)).astype(F)
    z = np.zeros(n, dtype=F)
    p, m, v, t, skipped = G.run(p0, z, z, grads[:2] + [bad] + grads[3:], **hp)
    assert (t, skipped) == (5, 1)
    (want,) = A.emul32(p0, grads[:2] + grads[3:], **hp).values()
    for a, b in zip((p, m, v), want):
        assert a.view(np.int32).tolist() == b.view(np.int32).tolist()
    out = G.step(p0, z, z, bad, 0, **hp)
    assert out[0] is p0 and out[1] is z and out[2] is z and out[3] == 1
    assert G.verdict(grads[0]) == 0 and G.verdict(bad) == 1
    # a huge finite gradient is no overflow of the norm: the squares are taken in float64
    big = np.full(n, 3e38, dtype=F)
    assert G.verdict(big) == 0
    # a poisoned element of a frozen range stays out of the verdict, and frozen elements keep their bits
    fz = np.zeros(n, dtype=bool)
    fz[512:520] = True
    assert G.verdict(bad, fz) == 0
    q, qm, qv, s = G.step(p0, z, z, bad, 0, frozen=fz, **hp)
    assert s == 0 and (q[fz] == p0[fz]).all() and not (qm[fz] != 0).any() and (q[~fz] != p0[~fz]).any()


def test_corrections_are_those_of_the_applied_index():
    assert G.corrections(7, 2, 0.9, 0.999) == (A.host_bc(0.9, 5)[0], A.host_bc(0.999, 5)[1])
    assert G.corrections(7, 0, 0.9, 0.999) == (A.host_bc(0.9, 7)[0], A.host_bc(0.999, 7)[1])


# ------------------------------------------------------------------------------------------------ 2. parsing and refusals
@pytest.mark.parametrize("bad", [1, 0, "yes", None, 1.0])
def test_a_value_that_is_no_bool_is_refused(model, bad):
    from segmminterest_amd.trainer import FusedAdamW, Trainer
    with pytest.raises(ValueError, match="skip_nonfinite must be a bool"):
        FusedAdamW(model, skip_nonfinite=bad)
    with pytest.raises(ValueError, match="skip_nonfinite must be a bool"):
        Trainer(model, device_state=True, skip_nonfinite=bad)


def test_refusals_name_their_cause(model):
    from segmminterest_amd.trainer import FusedAdamW, Trainer
    assert FusedAdamW(model).skip_nonfinite is False and FusedAdamW(model, skip_nonfinite=True).skip_nonfinite is True
    with pytest.raises(ValueError, match="skip_nonfinite=True needs device_state=True"):
        Trainer(model, skip_nonfinite=True)
    with pytest.raises(ValueError, match="skip_nonfinite=True needs device_state=True"):
        Trainer(model, device_state=False, skip_nonfinite=True, max_grad_norm=1.0)
    for lazy in (True, dict(flush_every=4)):
        with pytest.raises(ValueError, match="skip_nonfinite=True with lazy_tables"):
            Trainer(model, device_state=True, skip_nonfinite=True, lazy_tables=lazy)
        with pytest.raises(ValueError, match="skip_nonfinite=True with lazy_tables"):
            FusedAdamW(model, skip_nonfinite=True, lazy_tables=lazy)
    # an optimizer built on its own has no device step state: refused at the first call that needs it
    opt = FusedAdamW(model, skip_nonfinite=True)
    for call in (lambda: opt.skipped_steps, lambda: opt.applied_steps, lambda: opt.skipped, lambda: opt._guard_state("step")):
        with pytest.raises(RuntimeError, match="skip_nonfinite needs the device step state"):
            call()
    # off: nothing to read, no launch keyword, the norm only with max_grad_norm
    off = FusedAdamW(model)
    assert off.skipped_steps == 0 and off.skipped is None and off._guard_kw() == {} and off.grad_norm is None
    assert opt._guard_kw() == {"guard": True}


# ------------------------------------------------------------------------------------------------ 3. the two counts in a checkpoint
class _Store:
    """What FusedAdamW.state_dict reads of a ParamStore, on the CPU: model order, every parameter at the next multiple of 32 floats."""

    def __init__(self, model):
        self.index, off = {}, 0
        for n, p in model.named_parameters():
            off = (off + 31) & ~31
            self.index[n] = (off, p.numel())
            off += p.numel()
        self.n_live = (off + 7) & ~7
        self._params = dict(model.named_parameters())
        self.live_names = list(self.index)
        self.flat = torch.zeros(self.n_live)

    def ensure(self):
        pass


class _FakeH:
    """The device step state's two counts, on the host.  One instance stands for hipabi in a test (``optim.H`` is one name for every
    optimizer), so the counts are kept per bound state: ``of(opt)`` is an optimizer's own view."""

    def __init__(self, states=None, calls=None):
        self.states = {} if states is None else states
        self.calls = [] if calls is None else calls
        self.cur = None

    def of(self, opt):
        h = _FakeH(self.states, self.calls)
        h.cur = opt._step_state
        return h

    def step_bind(self, state):
        self.cur = state

    @property
    def skipped(self):
        return self.states.setdefault(self.cur, [0, 0])[0]

    @skipped.setter
    def skipped(self, k):
        self.states.setdefault(self.cur, [0, 0])[0] = k

    @property
    def step(self):
        return self.states.setdefault(self.cur, [0, 0])[1]

    @step.setter
    def step(self, k):
        self.states.setdefault(self.cur, [0, 0])[1] = k

    def step_get_skipped(self):
        return 0, self.skipped

    def step_set_skipped(self, k):
        self.skipped = int(k)
        self.calls.append(("step_set_skipped", int(k)))

    def step_get(self):
        return 99, self.step, (1.0, 1.0)

    def step_set(self, seed, step, b1, b2):
        self.step = int(step)
        self.calls.append(("step_set", int(step)))


def _opt(model, st, h, monkeypatch, guard=True, groups=None):
    """-> (optimizer, its view of the fake's counts)"""
    from segmminterest_amd import optim
    monkeypatch.setattr(optim, "H", h)
    opt = optim.FusedAdamW(model, lr=1e-3, weight_decay=1e-2, skip_nonfinite=guard, param_groups=groups)

    class M:          # state_dict / load_state_dict read model._store, named_parameters and parameters only
        _store = st
        named_parameters = model.named_parameters
        parameters = model.parameters
    opt.model = M
    opt.m, opt.v, opt._flat_id = torch.rand(st.n_live), torch.rand(st.n_live), st.flat.data_ptr()
    opt.device_state, opt._step_state = True, object()
    if opt.groups is not None:
        opt._build_segments(st)
    return opt, h.of(opt)


def test_state_dict_round_trip_of_both_counts(model, monkeypatch):
    from segmminterest_amd.trainer import no_decay_groups
    st = _Store(model)
    for groups in (None, no_decay_groups(model)):
        h = _FakeH()
        src, hs = _opt(model, st, h, monkeypatch, groups=groups)
        src.step_count, hs.skipped = 7, 2
        assert src.skipped_steps == 2 and src.applied_steps == 5
        sd = src.state_dict()
        assert all(float(s["step"]) == 5.0 for s in sd["state"].values()) and sd["state"]
        assert [g["segmm_skipped_steps"] for g in sd["param_groups"]] == [2] * (1 if groups is None else 2)
        dst, hd = _opt(model, st, h, monkeypatch, groups=groups)
        del h.calls[:]
        dst.load_state_dict(sd)
        assert dst.step_count == 7 and hd.skipped == 2 and hd.step == 7 and dst.applied_steps == 5
        assert h.calls == [("step_set", 7), ("step_set_skipped", 2)]          # the attempted count, then the skipped one
        # the resumed optimizer writes the checkpoint it was given
        again = dst.state_dict()
        assert all(torch.equal(again["state"][i][k], sd["state"][i][k]) for i in sd["state"] for k in ("exp_avg", "exp_avg_sq"))
        assert again["param_groups"] == sd["param_groups"] and all(float(again["state"][i]["step"]) == 5.0 for i in again["state"])


def test_a_checkpoint_without_the_key_loads_with_nothing_skipped(model, monkeypatch):
    st, h = _Store(model), _FakeH()
    plain, _ = _opt(model, st, h, monkeypatch, guard=False)
    plain.step_count = 4
    sd = plain.state_dict()
    assert "segmm_skipped_steps" not in sd["param_groups"][0] and all(float(s["step"]) == 4.0 for s in sd["state"].values())
    dst, hd = _opt(model, st, h, monkeypatch)
    hd.skipped = 3          # (what an earlier run left in the state)
    dst.load_state_dict(sd)
    assert dst.step_count == 4 and hd.skipped == 0 and dst.applied_steps == 4
    # the other way round: counts an optimizer without the guard cannot keep apart are refused by name; 0 skipped loads
    src, hs = _opt(model, st, h, monkeypatch)
    src.step_count, hs.skipped = 6, 1
    with pytest.raises(ValueError, match="segmm_skipped_steps"):
        _opt(model, st, h, monkeypatch, guard=False)[0].load_state_dict(src.state_dict())
    hs.skipped = 0
    back, _ = _opt(model, st, h, monkeypatch, guard=False)
    back.load_state_dict(src.state_dict())
    assert back.step_count == 6
    bad = src.state_dict()
    bad["param_groups"][0]["segmm_skipped_steps"] = -1
    with pytest.raises(ValueError, match="segmm_skipped_steps"):
        _opt(model, st, h, monkeypatch)[0].load_state_dict(bad)


def test_torch_adamw_loads_a_guarded_state_dict(model, monkeypatch):
    from segmminterest_amd.trainer import no_decay_groups
    st = _Store(model)
    opt, h = _opt(model, st, _FakeH(), monkeypatch, groups=no_decay_groups(model))
    opt.step_count, h.skipped = 9, 3
    sd = opt.state_dict()
    clones = [torch.nn.Parameter(p.detach().clone()) for p in model.parameters()]
    topt = torch.optim.AdamW([{"params": [clones[i] for i in g["params"]]} for g in sd["param_groups"]], lr=1.0)
    topt.load_state_dict(sd)
    assert all(float(topt.state[c]["step"]) == 6.0 for c in clones) and len(topt.state) == len(clones)
    assert all(g["segmm_skipped_steps"] == 3 for g in topt.param_groups)          # an extra key torch carries along
    names = [n for n, _ in model.named_parameters()]
    o, k = st.index["stage_mlp1.weight"]
    assert torch.equal(topt.state[clones[names.index("stage_mlp1.weight")]]["exp_avg"].reshape(-1), opt.m[o:o + k])


# ------------------------------------------------------------------------------------------------ 4. the ABI tables
def test_new_entry_points_in_the_regenerated_tables():
    from segmminterest_amd import _abi
    from segmminterest_amd import hipabi as H
    L = H.lib()
    inc = open(os.path.join(ROOT, "segmminterest_amd", "csrc", "cmd_dispatch.inc")).read()
    ops = H.op_ids()
    for name in NEW:
        assert name in _abi.PROTOTYPES and name in H.SIGNATURES and hasattr(L, name), name
        assert '"%s",' % name in inc and name in ops, name
    # the guarded updates take the arguments of the entry points they are named after
    assert H.PARAMS["segmm_adamw_guarded"] == H.PARAMS["segmm_adamw_scaled"]
    for a, b in (("segmm_adamw_groups_guarded", "segmm_adamw_groups"), ("segmm_adamw_table_lrs_guarded", "segmm_adamw_table_lrs"),
                 ("segmm_ema_update_guarded", "segmm_ema_update"), ("segmm_step_advance_guarded", "segmm_step_advance")):
        assert _abi.PROTOTYPES[a] == _abi.PROTOTYPES[b], a
    # the two words were spare: the size of the state is what it was, and the header names where they sit
    assert _abi.CONSTANTS["SEGMM_STEP_SKIP_WORD"] == H.STEP_SKIP_WORD == 14 and L.segmm_step_state_bytes() == 64


def test_guarded_entry_points_need_the_live_state():
    """Refused before anything touches the device: a step by value, and what the unguarded entry points refuse."""
    from segmminterest_amd import hipabi as H
    L = H.lib()

    def err(rc):
        assert rc != 0
        return L.segmm_last_error().decode()

    p, g, m, v, c, ids, flags, seg = 4096, 8192, 12288, 16384, 20480, 24576, 28672, 32768
    hp = (0.9, 0.999, 1e-8)
    for step in (1, 7, 0, -2):
        assert "adamw_guarded: step=" in err(L.segmm_adamw_guarded(p, g, m, v, 8, 1e-3, *hp, 1e-2, step, None, None))
        assert "adamw_groups_guarded: step=" in err(L.segmm_adamw_groups_guarded(p, g, m, v, 0, 8, seg, seg, seg, None, 1, 1e-3, *hp, step, c, None))
        assert "adamw_table_lrs_guarded: step=" in err(L.segmm_adamw_table_lrs_guarded(p, g, m, v, 10, 8, ids, 3, flags, 1e-3, 1.0, *hp, 1e-2, step, 1, None, None))
        assert "ema_update_guarded: step=" in err(L.segmm_ema_update_guarded(p, g, 8, 0.1, 1, step, None))
    assert "pointer/alignment" in err(L.segmm_adamw_guarded(p + 4, g, m, v, 8, 1e-3, *hp, 1e-2, -1, None, None))
    assert "segment table" in err(L.segmm_adamw_groups_guarded(p, g, m, v, 0, 8, None, seg, seg, None, 1, 1e-3, *hp, -1, None, None))
    assert "phase" in err(L.segmm_adamw_table_lrs_guarded(p, g, m, v, 10, 8, ids, 3, flags, 1e-3, 1.0, *hp, 1e-2, -1, 2, None, None))
    assert "weight=" in err(L.segmm_ema_update_guarded(p, g, 8, 0.0, 1, -1, None))
    assert "overlap" in err(L.segmm_ema_update_guarded(p, p + 16, 8, 0.1, 1, -1, None))
    assert "out2" in err(L.segmm_step_guard(None, None))
    assert "skipped=" in err(L.segmm_step_set_skipped(0x80000000, None))
