"""Learning-rate schedules in the device step state, the parts that need no GPU: the closed form (tests/lr_ref.py) against
torch.optim.lr_scheduler, argument validation on both sides of the C ABI, PlateauLR against torch's ReduceLROnPlateau, the AdamW
yardstick under a moving rate (it accepts the fp32 emulation of the kernel and rejects a rate taken one step late), and the new
entry points' declarations."""
import ctypes
import itertools
import math
import warnings

import numpy as np
import pytest
import torch

import adamw_ref as A
import lr_ref as L
from helpers import build_model, load_case

F = np.float32
# the parameter sets the schedule was checked at when it was specified
SETS = [dict(kind=kind, base_lr=1e-3, warmup_steps=W, start_factor=0.1, decay_steps=30, eta_min=eta, gamma=gamma, step_size=7)
        for kind, W, eta, gamma in itertools.product(L.KINDS, (0, 5), (0.0, 1e-5, 1e-4), (0.5, 0.97))]
NEW = ("segmm_step_schedule", "segmm_step_set_base_lr", "segmm_step_get_lr")


def _model():
    cfg, _, _, _ = load_case("img_d32_N2")
    return build_model(cfg)


def _spec(kw):
    """The LRSchedule fields of an lr_ref parameter set."""
    return {k: v for k, v in kw.items() if k != "base_lr"}


# ------------------------------------------------------------------------------------------------ 1. the closed form
@pytest.mark.parametrize("kw", SETS, ids=lambda kw: "%s-W%d-eta%g-g%g" % (kw["kind"], kw["warmup_steps"], kw["eta_min"], kw["gamma"]))
def test_closed_form_equals_torch_schedulers(kw):
    """lr_ref.lr_at against LinearLR + {ConstantLR, CosineAnnealingLR, LinearLR, StepLR, ExponentialLR} joined by SequentialLR, for
    every step up to the end of the decay (k <= W + D): relative difference <= 1e-12 in float64 and equal after rounding to fp32.
    Beyond k = W + D cosine and linear hold eta_min by definition (torch's cosine is periodic there): checked against the definition
    alone.  LRSchedule.lr_at, the host's copy in trainer.py, gives the fp32 value of the float-rounded closed form exactly."""
    from segmminterest_amd.trainer import LRSchedule
    W, D = kw["warmup_steps"], kw["decay_steps"]
    n = W + D + 1
    mine, ref = L.lrs(n, **kw), L.torch_lrs(n, **kw)
    rel = max(abs(a - b) / b if b else abs(a - b) for a, b in zip(mine, ref))
    print("worst relative difference %.3g over %d steps" % (rel, n))
    assert rel <= 1e-12, rel
    assert [L.f32(a) for a in mine] == [L.f32(b) for b in ref]
    if W:
        assert mine[0] == kw["base_lr"] * kw["start_factor"]
    if kw["kind"] in ("cosine", "linear"):
        # (computed, not exact: the formulas reach eta_min through r = eta_min / base)
        assert all(L.lr_at(k, **kw) == pytest.approx(kw["eta_min"], rel=1e-14, abs=1e-19) for k in range(W + D, W + D + 12))
        assert len({L.lr_at(k, **kw) for k in range(W + D, W + D + 12)}) == 1
    sched = LRSchedule.parse(_spec(kw), kw["base_lr"])
    for k in range(n + 12):
        assert sched.lr_at(kw["base_lr"], k) == L.f32(L.lr_at(k, abi_rounded=True, **kw)), k


# ------------------------------------------------------------------------------------------------ 2. validation
BAD_SCHEDULES = [
    "warm", 7, ["cosine"], dict(kind="cosine"), dict(kind="linear", decay_steps=0), dict(kind="cosine", decay_steps=2.5),
    dict(kind="step", gamma=0.5), dict(kind="step", step_size=0, gamma=0.5), dict(kind="exp"), dict(kind="exp", gamma=0.0),
    dict(kind="exp", gamma=1.5), dict(kind="exp", gamma=float("nan")), dict(kind="constant", warmup_steps=-1),
    dict(kind="constant", warmup_steps=3, start_factor=0.0), dict(kind="constant", warmup_steps=3, start_factor=1.5),
    dict(kind="cosine", decay_steps=10, eta_min=-1e-6), dict(kind="cosine", decay_steps=10, eta_min=2e-3),
    dict(kind="constant", period=3), dict(kind="constant", warmup_steps="three"),
]


@pytest.mark.parametrize("bad", BAD_SCHEDULES, ids=repr)
def test_lr_schedule_validation(bad):
    from segmminterest_amd.trainer import FusedAdamW, Trainer
    model = _model()
    with pytest.raises(ValueError, match="lr_schedule"):
        FusedAdamW(model, lr=1e-3, lr_schedule=bad)
    with pytest.raises(ValueError, match="lr_schedule"):
        Trainer(model, lr=1e-3, device_state=True, lr_schedule=bad)


@pytest.mark.parametrize("lr", [0.0, -1e-3, float("nan"), math.inf, 1e39, 1e-50])          # (the last two: inf and 0 as floats)
def test_lr_schedule_needs_a_positive_base_rate(lr):
    from segmminterest_amd.trainer import FusedAdamW
    with pytest.raises(ValueError, match="base rate"):
        FusedAdamW(_model(), lr=lr, lr_schedule="constant")


def test_lr_schedule_accepted_forms_and_device_state_refusal():
    from segmminterest_amd.trainer import FusedAdamW, LRSchedule, Trainer
    model = _model()
    assert FusedAdamW(model).schedule is None and FusedAdamW(model, lr=3e-4).current_lr() == 3e-4
    s = FusedAdamW(model, lr_schedule="constant").schedule
    assert s == LRSchedule(kind="constant") == FusedAdamW(model, lr_schedule=dict(kind="constant")).schedule
    spec = dict(kind="cosine", warmup_steps=5, start_factor=0.1, decay_steps=30, eta_min=1e-5)
    opt = FusedAdamW(model, lr=1e-3, lr_schedule=spec)
    assert opt.schedule == LRSchedule(**spec) == FusedAdamW(model, lr_schedule=LRSchedule(**spec)).schedule
    assert opt.current_lr() == L.f32(L.lr_at(0, base_lr=1e-3, abi_rounded=True, **spec))          # no step yet: the rate of step 1
    # the rate lives in the device step state: refused without one, at construction by the trainer ...
    with pytest.raises(ValueError, match="device_state=True"):
        Trainer(model, lr_schedule="constant")
    with pytest.raises(ValueError, match="device_state=True"):
        Trainer(model, device_state=False, lr_schedule=spec)
    # ... and by an optimizer built on its own, at the first call that needs it
    for call in (opt._lr_arg, lambda: opt.set_base_lr(5e-4), opt.device_lr):          # (_lr_arg: what every AdamW launch asks first)
        with pytest.raises(RuntimeError, match="device step state"):
            call()
    with pytest.raises(RuntimeError, match="needs an lr_schedule"):
        FusedAdamW(model).set_base_lr(5e-4)
    with pytest.raises(ValueError, match="eta_min"):          # a base rate below the schedule's floor
        opt.schedule.check_base(1e-6)


def test_c_entry_points_validate_without_a_device():
    """segmm_step_schedule / segmm_step_set_base_lr refuse out-of-range descriptors, and the AdamW entry points refuse the
    live-rate sentinel without step = -1, before anything touches the device."""
    from segmminterest_amd import hipabi as H
    lib = H.lib()
    K = H.LR_KINDS

    def err(rc):
        assert rc != 0
        return lib.segmm_last_error().decode()

    ok = dict(kind=K["cosine"], base_lr=1e-3, warmup_steps=5, start_factor=0.1, decay_steps=30, eta_min=1e-5, gamma=1.0, step_size=1)
    for field, bad_values in (("kind", (-1, 0, 6)), ("base_lr", (0.0, -1e-3, math.nan, math.inf)), ("warmup_steps", (-1,)),
                              ("start_factor", (0.0, 1.5, math.nan)), ("decay_steps", (0, -3)), ("eta_min", (-1e-6, 2e-3, math.nan)),
                              ("gamma", (0.0, 1.5, math.nan)), ("step_size", (0,))):
        for bad in bad_values:
            args = dict(ok, **{field: bad})
            assert field in err(lib.segmm_step_schedule(*args.values(), None)), (field, bad)
    for bad in (0.0, -1e-3, math.nan, math.inf):
        assert "base_lr" in err(lib.segmm_step_set_base_lr(bad, None)), bad
    p, g, m, v, c, ids, flags = 4096, 8192, 12288, 16384, 20480, 24576, 28672
    hp = (0.9, 0.999, 1e-8, 1e-4)
    assert H.LIVE_LR == -1.0
    assert "lr=" in err(lib.segmm_adamw(p, g, m, v, 8, H.LIVE_LR, *hp, 1, None))
    assert "lr=" in err(lib.segmm_adamw_scaled(p, g, m, v, 8, H.LIVE_LR, *hp, 3, c, None))
    assert "lr=" in err(lib.segmm_adamw_table(p, g, m, v, 10, 8, ids, 3, flags, H.LIVE_LR, *hp, 1, 0, None))
    assert "lr=" in err(lib.segmm_adamw_table_scaled(p, g, m, v, 10, 8, ids, 3, flags, -0.5, *hp, 2, c, None))


BAD_PLATEAUS = [dict(factor=1.0), dict(factor=0.0), dict(factor=1.5), dict(factor="half"), dict(patience=-1), dict(patience=1.5),
                dict(min_lr=-1e-6), dict(mode="best"), dict(threshold_mode="ratio"), dict(cooldown=-2), dict(threshold=-1.0)]


class _Opt:
    """What PlateauLR needs of an optimizer."""

    def __init__(self, lr):
        self.lr, self.calls = lr, []

    def set_base_lr(self, lr):
        self.lr = lr
        self.calls.append(lr)


@pytest.mark.parametrize("bad", BAD_PLATEAUS, ids=repr)
def test_lr_plateau_validation(bad):
    from segmminterest_amd.trainer import PlateauLR
    with pytest.raises(ValueError, match="lr_plateau"):
        PlateauLR(_Opt(1e-3), **bad)


def test_fit_refuses_lr_plateau_it_cannot_serve():
    from segmminterest_amd.trainer import Trainer, fit
    tr = Trainer(_model())
    with pytest.raises(ValueError, match="needs Trainer\\(lr_schedule"):
        fit(tr, [], [], 1, lr_plateau=dict(factor=0.5))
    with pytest.raises(ValueError, match="lr_plateau must be a dict"):
        fit(tr, [], [], 1, lr_plateau=0.5)
    tr.opt.schedule = object()          # (a trainer with a schedule needs a device; the argument checks come first)
    with pytest.raises(ValueError, match="lr_plateau"):
        fit(tr, [], [], 1, lr_plateau=dict(factor=0.5, patient=2))
    with pytest.raises(ValueError, match="lr_plateau"):
        fit(tr, [], [], 1, lr_plateau=dict(factor=2.0))


# ------------------------------------------------------------------------------------------------ 3. reduce on plateau
def _series(seed, n=60):
    """A metric that improves, stalls, improves a little (inside and outside the relative threshold), then degrades."""
    rng = np.random.default_rng(seed)
    up = np.concatenate([np.linspace(0.1, 0.5, 8), np.full(9, 0.5), 0.5 * (1 + np.array([5e-5, 2e-4, 2e-4, 1e-5])), np.full(12, 0.45)])
    return np.concatenate([up, 0.45 + 0.02 * rng.standard_normal(n - up.size)]).tolist()


@pytest.mark.parametrize("mode", ["max", "min"])
@pytest.mark.parametrize("kw", [dict(factor=0.5, patience=2, min_lr=1e-6), dict(factor=0.1, patience=0, min_lr=2e-5),
                                dict(factor=0.5, patience=3, min_lr=0.0, cooldown=2), dict(factor=0.7, patience=1, threshold=1e-2, threshold_mode="abs")],
                         ids=lambda kw: "f%g-p%d" % (kw["factor"], kw["patience"]))
def test_plateau_equals_torch_reduce_on_plateau(mode, kw):
    """The same metric series through PlateauLR and torch.optim.lr_scheduler.ReduceLROnPlateau (on a dummy optimizer): the same
    rate after every validation, in both modes (mode "min" sees the negated series), through the floor at min_lr where the series
    reaches it, and no call once a reduction would move the rate by less than eps."""
    from segmminterest_amd.trainer import PlateauLR
    series = [x if mode == "max" else 1.0 - x for x in _series(3)]
    opt = _Opt(1e-3)
    mine = PlateauLR(opt, mode=mode, **kw)
    topt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1e-3)
    ref = torch.optim.lr_scheduler.ReduceLROnPlateau(topt, mode=mode, **kw)
    got, want = [], []
    for x in series:
        mine.step(x)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ref.step(x)
        got.append(opt.lr)
        want.append(topt.param_groups[0]["lr"])
    assert got == want
    assert len(opt.calls) == len(set(want)) - 1 >= 2          # one set_base_lr per reduction, none besides
    if kw.get("min_lr", 0.0) > 0:
        assert got[-1] == kw["min_lr"]          # the floor was reached and held


# ------------------------------------------------------------------------------------------------ 4. the AdamW yardstick under a moving rate
def test_yardstick_under_a_moving_rate():
    """Regime ``unit`` for 40 steps under the cosine schedule with a warm-up (lr_ref.MOVING): adamw_ref.emul32, the fp32 emulation
    of adamw_elem4, chained one step at a time at the fp32 rates the device state holds, against float64 chained the same way
    (R_abi) -- E_p, E_m, E_v within MARGIN x the errors of torch.optim.AdamW + torch's scheduler (fp32, CPU) against float64 at
    the double rates (R_true), at steps 1, 2, 3, 10, 40.  A mutant that runs step t at the rate of step t + 1 (k off by one) is
    rejected: at step 1 of a warm-up from 0.1 its update is 2.8 times too large."""
    y = L.moving_yardstick()
    got = L.chain(A.emul32, lambda t: y.lr_abi[t])
    late = L.chain(A.emul32, lambda t: y.lr_abi[t + 1])
    worst, worst_late = [0.0] * 3, 0.0
    for t in L.MOVING_CHECKPOINTS:
        ratios = y.ratios(got[t], t)
        print("RATIO %-44s E_p %5.2f  E_m %5.2f  E_v %5.2f" % (("emulation, moving rate, step %d" % t,) + ratios))
        assert max(ratios) <= A.MARGIN, (t, ratios)
        worst = [max(a, b) for a, b in zip(worst, ratios)]
        worst_late = max(worst_late, max(y.ratios(late[t], t)))
    print("RATIO %-44s E_p %5.2f  E_m %5.2f  E_v %5.2f" % (("emulation, moving rate, worst",) + tuple(worst)))
    print("rate one step late: worst ratio %.3g" % worst_late)
    assert worst_late > 4.0 * A.MARGIN
    # the double rates torch is handed and the fp32 rates of the device differ by fp32 rounding only
    assert all(abs(y.lr_abi[t] - L.lr_at(t - 1, **L.MOVING)) <= 2.0 ** -23 * y.lr_abi[t] for t in range(1, L.MOVING_STEPS + 1))


# ------------------------------------------------------------------------------------------------ 5. declarations
def test_new_entry_points_declared_and_exported():
    from segmminterest_amd import hipabi as H
    raw = ctypes.CDLL(H.LIB_PATH)
    lib = H.lib()
    ops = H.op_ids()
    for n in NEW:
        assert n in H.SIGNATURES and hasattr(raw, n) and n in ops, n
    assert [c.__name__ for c in H.SIGNATURES["segmm_step_schedule"]] == ["c_int", "c_float", "c_int", "c_float", "c_int", "c_float", "c_float",
                                                                        "c_int", "c_void_p"]
    assert H.PARAMS["segmm_step_schedule"] == ("kind", "base_lr", "warmup_steps", "start_factor", "decay_steps", "eta_min", "gamma", "step_size",
                                               "stream")
    assert H.PARAMS["segmm_step_set_base_lr"] == ("base_lr", "stream") and H.PARAMS["segmm_step_get_lr"] == ("lr", "base_lr", "stream")
    assert lib.segmm_abi_version() == H.ABI_VERSION == 30          # additive: no existing prototype moved
    assert len(H.SIGNATURES["segmm_adamw"]) == 12 and len(H.SIGNATURES["segmm_adamw_table"]) == 17
    assert H.LR_KINDS == dict(constant=1, cosine=2, linear=3, step=4, exp=5)
    # the state grew by the rate and its descriptor and is still a whole number of 16-byte units
    assert lib.segmm_step_state_bytes() == 64
    # a recorded AdamW command carries the sentinel like any other rate
    rec = H.Recorder(111, 222)
    rec.mark(H.PHASE_STEP_TAIL)
    rec.call("segmm_adamw", (4096, 8192, 12288, 16384, 10, H.LIVE_LR, 0.9, 0.999, 1e-8, 1e-4, -1, 111))
    rec.call("segmm_step_set_base_lr", (5e-4, 111))
    (ph, a), = rec.finish()
    assert H.cmd_arg(a[0], "segmm_adamw", "lr") == -1.0 and a[1].op == ops["segmm_step_set_base_lr"] and a[1].a[0].f == 5e-4
