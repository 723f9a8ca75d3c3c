"""The optimizer side of the training step: ``FusedAdamW`` (one AdamW kernel over the live range of the flat parameter buffer,
global-norm clipping, parameter groups), the learning-rate schedules the device evaluates (``LRSchedule``) or the host drives
(``PlateauLR``), and the device-side moving average of the weights (``WeightEMA``, owned by the optimizer)."""
from __future__ import annotations

import contextlib
import dataclasses
import fnmatch
import math
import struct
from typing import Optional

import torch
import torch.nn as nn

from . import hipabi as H


# ------------------------------------------------------------------------------------------------ optimizer
def _check_max_grad_norm(max_grad_norm):
    if max_grad_norm is None:
        return None
    try:
        m = float(max_grad_norm)
    except (TypeError, ValueError):
        raise ValueError("max_grad_norm must be a positive float, inf or None, not %r" % (max_grad_norm,))
    if not m > 0.0:          # (also NaN)
        raise ValueError("max_grad_norm must be a positive float, inf or None, not %r" % (max_grad_norm,))
    return m


def _f32(x):
    """``x`` rounded to float32, as a Python float: what the C ABI's ``float`` parameters carry."""
    try:
        return struct.unpack("f", struct.pack("f", float(x)))[0]
    except OverflowError:          # beyond the fp32 range
        return math.copysign(math.inf, x)


# ---- parameter groups (FusedAdamW(param_groups=...)): pure functions of names, sizes and offsets -- no device, no ParamStore
GROUP_KEYS = ("params", "lr_scale", "weight_decay", "frozen")


def _group_value(gi, key, x):
    """A group's ``lr_scale`` / ``weight_decay``: a finite float >= 0, as the fp32 number the device table holds."""
    if isinstance(x, bool) or not isinstance(x, (int, float)) or not (0.0 <= float(x) < math.inf) or _f32(x) == math.inf:
        raise ValueError("%s%s must be a finite float >= 0, not %r" % ("param_groups[%d]: " % gi if gi >= 0 else "", key, x))
    return _f32(x)


def resolve_param_groups(named, param_groups, weight_decay):
    """``param_groups`` (the list of dicts FusedAdamW takes) resolved over ``named`` = [(name, parameter)] in
    ``model.named_parameters()`` order (the parameter is only handed to callables; it may be None) -> a list of
    ``{"names", "lr_scale", "weight_decay", "frozen"}``: entry 0 is the DEFAULT group (every parameter no group selects: scale 1,
    the optimizer's ``weight_decay``; possibly empty), entry k + 1 is ``param_groups[k]``.  Refused by name: a parameter two groups
    select, a pattern or callable that selects nothing, an unknown key, a value out of range."""
    if not isinstance(param_groups, (list, tuple)) or not all(isinstance(g, dict) for g in param_groups):
        raise ValueError("param_groups must be a list of dicts, not %r" % (param_groups,))
    names = [n for n, _ in named]
    owner = {}
    out = [dict(names=[], lr_scale=1.0, weight_decay=_group_value(-1, "weight_decay (with param_groups)", weight_decay), frozen=False)]
    for gi, g in enumerate(param_groups):
        unknown = [k for k in g if k not in GROUP_KEYS]
        if unknown:
            raise ValueError("param_groups[%d]: unknown key %r (a group takes %s; betas and eps are the optimizer's, one pair for "
                             "every group)" % (gi, unknown[0], ", ".join(GROUP_KEYS)))
        if "params" not in g:
            raise ValueError("param_groups[%d]: no 'params' (a list of names / fnmatch patterns, or a callable (name, parameter) -> bool)" % gi)
        sel = g["params"]
        if callable(sel):
            picked = [n for n, p in named if sel(n, p)]
            if not picked:
                raise ValueError("param_groups[%d]: the callable %r selects no parameter" % (gi, getattr(sel, "__name__", sel)))
        else:
            if isinstance(sel, str):
                sel = [sel]
            picked, seen = [], set()
            for pat in sel:
                if not isinstance(pat, str):
                    raise ValueError("param_groups[%d]: 'params' holds %r; names / fnmatch patterns are strings" % (gi, pat))
                hit = [n for n in names if n == pat or fnmatch.fnmatchcase(n, pat)]
                if not hit:
                    raise ValueError("param_groups[%d]: the pattern %r selects no parameter" % (gi, pat))
                picked += [n for n in hit if n not in seen]
                seen.update(hit)
        frozen = g.get("frozen", False)
        if not isinstance(frozen, bool):
            raise ValueError("param_groups[%d]: frozen must be a bool, not %r" % (gi, frozen))
        for n in picked:
            if n in owner:
                raise ValueError("param_groups[%d] and param_groups[%d] both select the parameter %s" % (owner[n], gi, n))
            owner[n] = gi
        order = {n: i for i, n in enumerate(names)}
        out.append(dict(names=sorted(picked, key=order.__getitem__), lr_scale=_group_value(gi, "lr_scale", g.get("lr_scale", 1.0)),
                        weight_decay=_group_value(gi, "weight_decay", g.get("weight_decay", out[0]["weight_decay"])), frozen=frozen))
    out[0]["names"] = [n for n in names if n not in owner]
    return out


def group_segments(order, n_live, hyper_of):
    """The live range [0, n_live) cut into segments: ``order`` = [(name, offset, numel)] of the live parameters by ascending offset,
    ``hyper_of(name)`` = (lr_scale, weight_decay, frozen) -> [(end, lr_scale, weight_decay, frozen)], maximal runs of consecutive
    floats with equal values.  An alignment gap goes with the parameter in front of it (it holds zeros, and zeros stay zero under
    any update), so a segment ends where the next parameter with other values STARTS: at a multiple of 4 floats (ParamStore lays
    groups out at multiples of 32 and fused-group members have numel % 4 == 0) -- the 16-byte vectors of the kernels never
    straddle two segments.  Only the last end, n_live itself, may be anything."""
    segs = []
    for name, off, _ in order:
        h = tuple(hyper_of(name))
        if segs and segs[-1][1:] == h:
            continue
        if segs:
            if off % 4:
                raise AssertionError("parameter %s starts at float %d, not a multiple of 4: a segment cannot end there" % (name, off))
            segs[-1] = (off,) + segs[-1][1:]
        segs.append((None,) + h)
    if not segs:
        return [(n_live, 1.0, 0.0, False)]
    segs[-1] = (n_live,) + segs[-1][1:]
    assert all(a[0] < b[0] for a, b in zip(segs, segs[1:])), segs
    return segs


def no_decay_groups(model):
    """The usual AdamW recipe as a ``param_groups`` list: every bias, every LayerNorm weight and every positional table
    (the ``*_pe`` embeddings) at weight decay 0; everything else stays in the default group."""
    names = []
    for mname, mod in model.named_modules():
        for pname, _ in mod.named_parameters(recurse=False):
            if pname == "bias" or isinstance(mod, nn.LayerNorm) or (isinstance(mod, nn.Embedding) and mname.endswith("_pe")):
                names.append((mname + "." if mname else "") + pname)
    return [{"params": names, "weight_decay": 0.0}]


@dataclasses.dataclass(frozen=True)
class LRSchedule:
    """A learning-rate schedule the DEVICE evaluates every step (segmm_step_schedule): ``lr_schedule=`` of FusedAdamW / Trainer,
    given as an instance, a dict of these fields or just the kind's name.  The optimizer's ``lr`` is the base rate; with k the
    number of completed optimizer steps, W = warmup_steps and j = max(k - W, 0) the step runs at
    base * warm(k) * dec(j):  warm(k) = start_factor + (1 - start_factor) k / W for k < W, else 1 (torch's LinearLR; its default
    start_factor 1/3); dec by ``kind``: "constant" 1; "cosine" / "linear" down to ``eta_min`` over ``decay_steps`` steps and held
    there; "step" gamma^floor(j / step_size); "exp" gamma^j -- torch's CosineAnnealingLR / LinearLR / StepLR / ExponentialLR behind
    the warm-up in a SequentialLR, stepped once per optimizer step."""
    kind: str = "constant"
    warmup_steps: int = 0
    start_factor: float = 1.0 / 3
    decay_steps: int = 0
    eta_min: float = 0.0
    gamma: float = 1.0
    step_size: int = 1

    KINDS = ("constant", "cosine", "linear", "step", "exp")

    @classmethod
    def parse(cls, spec, base_lr):
        """``spec`` (None, a kind name, a dict of fields or an LRSchedule) validated against the base rate -> LRSchedule or None."""
        if spec is None:
            return None
        if isinstance(spec, str):
            spec = {"kind": spec}
        if isinstance(spec, cls):
            spec = dataclasses.asdict(spec)
        if not isinstance(spec, dict):
            raise ValueError("lr_schedule must be None, a kind name, a dict or an LRSchedule, not %r" % (spec,))
        unknown = set(spec) - {f.name for f in dataclasses.fields(cls)}
        if unknown:
            raise ValueError("lr_schedule: unknown field(s) %s" % sorted(unknown))
        kind = spec.get("kind", "constant")
        if kind not in cls.KINDS:
            raise ValueError("lr_schedule: kind %r is not one of %s" % (kind, cls.KINDS))
        need = {"cosine": ("decay_steps",), "linear": ("decay_steps",), "step": ("gamma", "step_size"), "exp": ("gamma",)}.get(kind, ())
        for f in need:
            if f not in spec:
                raise ValueError("lr_schedule: kind %r needs %s" % (kind, f))
        try:
            ints = {f: spec[f] for f in ("warmup_steps", "decay_steps", "step_size") if f in spec}
            for f, v in ints.items():
                if isinstance(v, bool) or int(v) != v:
                    raise ValueError
            s = cls(kind=kind, **{f: int(v) for f, v in ints.items()},
                    **{f: float(spec[f]) for f in ("start_factor", "eta_min", "gamma") if f in spec})
            base = float(base_lr)
        except (TypeError, ValueError):
            raise ValueError("lr_schedule: warmup_steps, decay_steps, step_size must be integers, the other fields and lr floats: %r" % (spec,))
        s.check_base(base)
        if s.warmup_steps < 0 or (s.warmup_steps > 0 and not 0.0 < s.start_factor <= 1.0):
            raise ValueError("lr_schedule: warmup_steps >= 0 and, with a warm-up, 0 < start_factor <= 1")
        if kind in ("cosine", "linear") and s.decay_steps < 1:
            raise ValueError("lr_schedule: decay_steps >= 1 for kind %r" % kind)
        if not 0.0 < s.gamma <= 1.0 or s.step_size < 1:
            raise ValueError("lr_schedule: 0 < gamma <= 1 and step_size >= 1")
        return s

    def check_base(self, base):
        """The base rate this schedule may run under: positive, finite and (as floats of the C ABI) not below eta_min."""
        if not (0.0 < _f32(base) < math.inf) or not 0.0 <= _f32(self.eta_min) <= _f32(base):
            raise ValueError("lr_schedule: the base rate must be positive and finite and 0 <= eta_min <= base rate (lr %r, eta_min %r)"
                             % (base, self.eta_min))

    def lr_at(self, base_lr, k):
        """The rate after ``k`` completed optimizer steps as the device computes it: float64 arithmetic on the float32 descriptor
        (csrc/common.h segmm_lr_at), rounded once to float32."""
        base, sf, eta, gamma = (_f32(x) for x in (base_lr, self.start_factor, self.eta_min, self.gamma))
        W, D, k = self.warmup_steps, max(self.decay_steps, 1), max(int(k), 0)
        warm = sf + (1.0 - sf) * k / W if (W > 0 and k < W) else 1.0
        j = max(k - W, 0)
        r = eta / base
        dec = 1.0
        if self.kind == "cosine":
            dec = r + (1.0 - r) * (1.0 + math.cos(math.pi * min(j, D) / D)) / 2.0
        elif self.kind == "linear":
            dec = 1.0 - (1.0 - r) * min(j, D) / D
        elif self.kind == "step":
            dec = gamma ** (j // self.step_size)
        elif self.kind == "exp":
            dec = gamma ** j
        return _f32(base * warm * dec)


class PlateauLR:
    """torch.optim.lr_scheduler.ReduceLROnPlateau in plain Python, driving ``opt.set_base_lr``: ``step(metric)`` after every
    validation; once the metric has not improved (by torch's relative / absolute ``threshold``) for more than ``patience``
    validations the base rate becomes max(rate * factor, min_lr), unless that moves it by no more than ``eps``.  ``opt`` needs an
    ``lr`` attribute (the base rate) and ``set_base_lr``."""

    def __init__(self, opt, factor=0.1, patience=10, min_lr=0.0, mode="min", threshold=1e-4, threshold_mode="rel", cooldown=0, eps=1e-8):
        if mode not in ("min", "max") or threshold_mode not in ("rel", "abs"):
            raise ValueError("lr_plateau: mode must be 'min' or 'max' and threshold_mode 'rel' or 'abs'")
        try:
            factor, min_lr, threshold, eps = float(factor), float(min_lr), float(threshold), float(eps)
            if isinstance(patience, bool) or isinstance(cooldown, bool) or int(patience) != patience or int(cooldown) != cooldown:
                raise ValueError
        except (TypeError, ValueError):
            raise ValueError("lr_plateau: factor, min_lr, threshold, eps must be floats, patience and cooldown integers")
        if not 0.0 < factor < 1.0:
            raise ValueError("lr_plateau: factor must lie in (0, 1), not %r" % factor)
        if not min_lr >= 0.0 or patience < 0 or cooldown < 0 or not threshold >= 0.0 or not eps >= 0.0:
            raise ValueError("lr_plateau: min_lr, patience, cooldown, threshold and eps must be >= 0")
        self.opt, self.factor, self.patience, self.min_lr, self.mode = opt, factor, int(patience), min_lr, mode
        self.threshold, self.threshold_mode, self.cooldown, self.eps = threshold, threshold_mode, int(cooldown), eps
        self.best = math.inf if mode == "min" else -math.inf
        self.num_bad, self.cooldown_counter = 0, 0

    def is_better(self, a, best):
        if self.mode == "min":
            return a < (best * (1.0 - self.threshold) if self.threshold_mode == "rel" else best - self.threshold)
        return a > (best * (self.threshold + 1.0) if self.threshold_mode == "rel" else best + self.threshold)

    def step(self, metric):
        """Feed one validation result; returns the new base rate if this call lowered it, else None."""
        current = float(metric)
        if self.is_better(current, self.best):
            self.best, self.num_bad = current, 0
        else:
            self.num_bad += 1
        if self.cooldown_counter > 0:
            self.cooldown_counter -= 1
            self.num_bad = 0
        if self.num_bad > self.patience:
            self.cooldown_counter, self.num_bad = self.cooldown, 0
            old = float(self.opt.lr)
            new = max(old * self.factor, self.min_lr)
            if old - new > self.eps:
                self.opt.set_base_lr(new)
                return new
        return None


def parse_skip_nonfinite(spec, device_state, lazy_tables):
    """``skip_nonfinite=`` of FusedAdamW / Trainer -> bool.  Refused by name: a value that is no bool; the guard without the device
    step state (``device_state``: True / False, or None when the caller cannot know yet -- FusedAdamW on its own checks at its first
    step); the guard beside ``lazy_tables`` (a skipped step has no g = 0 replay in the ring: a follow-up)."""
    if not isinstance(spec, bool):
        raise ValueError("skip_nonfinite must be a bool, not %r" % (spec,))
    if spec and device_state is not None and not device_state:
        raise ValueError("skip_nonfinite=True needs device_state=True: the verdict and the count of skipped steps live in the device step state")
    if spec and lazy_tables is not None:
        raise ValueError("skip_nonfinite=True with lazy_tables is not supported: a skipped step has no g = 0 replay in the lazy tables' "
                         "history ring (a follow-up); use one of the two")
    return spec


EMA_KEYS = ("decay", "warmup")


def parse_ema(spec):
    """``ema=`` of FusedAdamW / Trainer -> ``(decay, warmup)`` or None.  ``spec``: None, a float (the decay) or a dict
    ``dict(decay=0.999, warmup=True)``; an unknown key, a decay outside 0 <= decay < 1 and a non-bool warmup are refused by name."""
    if spec is None:
        return None
    if isinstance(spec, dict):
        unknown = [k for k in spec if k not in EMA_KEYS]
        if unknown:
            raise ValueError("ema: unknown key %r (an EMA takes %s)" % (unknown[0], ", ".join(EMA_KEYS)))
        decay, warmup = spec.get("decay", 0.999), spec.get("warmup", True)
    else:
        decay, warmup = spec, True
    if not isinstance(warmup, bool):
        raise ValueError("ema: warmup must be a bool, not %r" % (warmup,))
    return _check_ema_decay(decay), warmup


def _check_ema_decay(decay):
    if isinstance(decay, bool) or not isinstance(decay, (int, float)) or not 0.0 <= float(decay) < 1.0:          # (also NaN)
        raise ValueError("ema: decay must be a float with 0 <= decay < 1, not %r" % (decay,))
    return float(decay)


LAZY_KEYS = ("flush_every", "data_parallel", "ema")
LAZY_FLUSH_EVERY = 64          # lazy_tables=True (profiles/lazy_tables/)


def parse_lazy_tables(spec):
    """``lazy_tables=`` of FusedAdamW / Trainer -> ``flush_every`` (the history ring's capacity) or None.  ``spec``: None (dense, as
    ever), True (the default capacity) or ``dict(flush_every=int, data_parallel=bool, ema=bool)``; an unknown key, a flush_every < 1
    and a data_parallel or ema that is no bool are refused by name (:func:`parse_lazy_data_parallel` and :func:`parse_lazy_ema`
    return those flags)."""
    if spec is None:
        return None
    if spec is True:
        return LAZY_FLUSH_EVERY
    if not isinstance(spec, dict):
        raise ValueError("lazy_tables must be None, True or dict(flush_every=int), not %r" % (spec,))
    unknown = [k for k in spec if k not in LAZY_KEYS]
    if unknown:
        raise ValueError("lazy_tables: unknown key %r (lazy tables take %s)" % (unknown[0], ", ".join(LAZY_KEYS)))
    fe = spec.get("flush_every", LAZY_FLUSH_EVERY)
    if isinstance(fe, bool) or not isinstance(fe, int) or fe < 1:
        raise ValueError("lazy_tables: flush_every must be an int >= 1, not %r" % (fe,))
    parse_lazy_data_parallel(spec)
    parse_lazy_ema(spec)
    return fe


def parse_lazy_data_parallel(spec):
    """The ``data_parallel`` key of ``lazy_tables=`` (default False): the opt-in to lazy tables under an active DPComm, where the
    rows a step touches are all ranks' rows and are stepped by segmm_adamw_table_lazy_rows behind the row exchange."""
    dp = spec.get("data_parallel", False) if isinstance(spec, dict) else False
    if not isinstance(dp, bool):
        raise ValueError("lazy_tables: data_parallel must be a bool, not %r" % (dp,))
    return dp


def parse_lazy_ema(spec):
    """The ``ema`` key of ``lazy_tables=`` (default False): the opt-in to lazy tables beside a weight average (``ema=...``), where a
    lazy row's shadow is replayed with the row (segmm_adamw_table_catchup_ema / segmm_adamw_table_lazy_rows_ema).  Without an EMA
    the key changes nothing."""
    le = spec.get("ema", False) if isinstance(spec, dict) else False
    if not isinstance(le, bool):
        raise ValueError("lazy_tables: ema must be a bool, not %r" % (le,))
    return le


class WeightEMA:
    """An exponential moving average of the live parameters, kept on the device and owned by :class:`FusedAdamW`
    (``Trainer(ema=...)``; ``trainer.ema`` / ``opt.ema``): ``shadow <- shadow + (p - shadow) w`` after every optimizer step, one
    segmm_ema_update launch over the live range of the flat buffer, issued by ``FusedAdamW.end_step`` -- behind every AdamW launch
    of the step, whichever path took it (plain, clipped, two-pass id tables, data-parallel buckets, micro-batches: one update per
    OPTIMIZER step), and part of a recorded step's tail.  w = fp32(1 - decay) (host double); with ``warmup`` the step t runs at
    max(w, fp32(9 / (10 + t))), i.e. decay_t = min(decay, (1 + t) / (10 + t)), t = the optimizer's step count (the device step
    state's under ``device_state``: a resumed run continues its warm-up).

    ``shadow``: one float32 tensor of ``n_live`` floats beside ``opt.m`` / ``opt.v``; dead parameters never move and have none,
    frozen ones keep shadow = p.  It is made with the optimizer's state and SEEDED with the parameters at the head of the first
    optimizer step, before any of its AdamW launches (the id tables' early pass included) -- not lazily at the first update; read
    earlier (``applied()``, ``state_dict()`` before any step) it holds the parameters of that moment.  It is RE-SEEDED in the same way
    from the parameters of the moment whenever the store rebuilds its flat buffer, exactly where ``m`` and ``v`` are zeroed;
    ``load_state_dict`` replaces the seed.
    Data parallel: every rank computes the same shadow from its identical parameters, no collective.

    ``applied()``: a context manager that swaps the shadow INTO the live range (segmm_vec_swap) and back out on exit, bumping
    ``store.fused_version`` both times so that the weight planes are re-split for the averaged weights and again for the trained
    ones.  While applied, ``train_step`` / ``record`` / ``run_recorded`` are refused, and so is a nested ``applied()``.
    ``decay`` may be assigned between steps (a recorded step is then refused like after any hyperparameter change).

    Beside lazy id tables (``lazy_tables=dict(ema=True)``) the shadow rows of a lazy table are averaged LAZILY, with the row: the
    step's update walks around the table's range, and a row that replays its missed AdamW steps replays its lerps with them, each
    with the weight its step used (the ring's fourth float).  ``applied()``, ``state_dict()`` and ``load_state_dict()`` flush first
    (``opt.flush_tables()``), after which the shadow holds the dense run's bits; a RAW read of ``ema.shadow`` needs
    ``opt.flush_tables()`` first -- with steps pending, the rows outside the recent batches are behind."""

    def __init__(self, opt, decay=0.999, warmup=True):
        self.opt, self.warmup = opt, bool(warmup)
        self.decay = decay
        self.shadow = None
        self.is_applied = False

    @property
    def decay(self):
        return self._decay

    @decay.setter
    def decay(self, d):
        self._decay = _check_ema_decay(d)

    @property
    def weight(self):
        """The kernel's ``weight``: fp32(1 - decay), the subtraction in double."""
        return _f32(1.0 - self._decay)

    def hyper(self):
        return self.weight, self.warmup

    def weight_at(self, t):
        """w of optimizer step ``t`` as the kernel forms it (a Python float holding an fp32 value)."""
        return max(self.weight, _f32(9.0 / (10.0 + t))) if self.warmup else self.weight

    def _seed(self, st):
        """(FusedAdamW._state, where m and v are made) a fresh shadow for the store's live range.  It is FILLED with the parameters at the
        head of the next optimizer step (:meth:`step_head`) -- and, should anything read it before (``applied()``, ``state_dict()``),
        with the parameters of that moment, the step head then filling it again: weights loaded into the model between the
        construction of the optimizer's state and the first step are the ones averaged."""
        if self.is_applied:
            raise RuntimeError("ema: the flat parameter buffer was rebuilt inside ema.applied()")
        self.shadow = torch.empty(st.n_live, dtype=torch.float32, device=st.flat.device)
        self._pending = True

    def _fill(self, st):
        H.torch_fallback("seeding the EMA shadow (a step is recorded after the optimizer's first step)")
        self.shadow.copy_(st.flat[:st.n_live].detach())

    def step_head(self, st):
        """Head of an optimizer step (FusedAdamW.begin_step, or table_early when the id tables' early pass comes first): a shadow
        that is still to be seeded takes the parameters as they stand now, before any AdamW launch of the step."""
        if self.__dict__.get("_pending", False):
            self._fill(st)
            self._pending = False

    def _store(self):
        """The store, with the optimizer's state and a seeded shadow in place."""
        st = self.opt._state()
        if self.shadow is None or self.shadow.numel() != st.n_live:
            raise AssertionError("ema: no shadow for the live range")
        if self.__dict__.get("_pending", False):
            self._fill(st)          # (stays pending: the head of the first step seeds it again)
        return st

    def update(self):
        """The step's update (FusedAdamW.end_step): one launch on the current stream -- or, beside lazy id tables
        (``lazy_tables=dict(ema=True)``), one launch per range AROUND the tables stepped lazily this step (``opt._lazy_tail``, as
        ``step_ranges`` walks around them for AdamW): their listed rows took this step's lerp in segmm_adamw_table_lazy_rows_ema,
        every other row of theirs takes it when it next catches up.  Parameter offsets are multiples of 32 floats: every piece is
        16-byte aligned."""
        if self.is_applied:
            raise RuntimeError("ema: an optimizer step inside ema.applied() (the live range holds the averaged weights)")
        opt = self.opt
        st = self._store()
        live = opt.__dict__.get("device_state", False)
        if live and opt.__dict__.get("_step_state") is not None:
            H.step_bind(opt._step_state)
        pos, step = 0, -1 if live else opt.step_count
        tail = opt.__dict__.get("_lazy_tail")
        if not tail:
            # (skip_nonfinite: the guarded form -- the shadow of a skipped step keeps its bits)
            H.ema_update(self.shadow, st.flat, st.n_live, self.weight, self.warmup, step, **opt._guard_kw())
            return
        for o, n in sorted(tail.values()):
            if o > pos:
                H.ema_update(self.shadow, st.flat, o - pos, self.weight, self.warmup, step, shadow_off=pos, p_off=pos)
            pos = max(pos, o + n)
        if st.n_live > pos:
            H.ema_update(self.shadow, st.flat, st.n_live - pos, self.weight, self.warmup, step, shadow_off=pos, p_off=pos)

    def _swap(self, st):
        H.vec_swap(st.flat, self.shadow, st.n_live)
        st.fused_version += 1          # the weight planes follow the live range: ParamStore.ensure() re-splits them

    @contextlib.contextmanager
    def applied(self):
        if self.is_applied:
            raise RuntimeError("ema.applied() is already active (nested applied() is refused)")
        if H.RECORDER is not None:
            raise RuntimeError("ema.applied() inside a recorded step")
        self._flush_lazy()
        st = self._store()
        self._swap(st)
        self.is_applied = True
        flat_id = st.flat.data_ptr()
        try:
            yield self
        finally:
            self.is_applied = False
            if st.flat is None or st.flat.data_ptr() != flat_id:
                raise RuntimeError("ema.applied(): the flat parameter buffer was rebuilt while the averaged weights were applied; the "
                                   "trained weights are in ema.shadow")
            self._swap(st)

    def _flush_lazy(self):
        """Lazy id tables (``lazy_tables=dict(ema=True)``): every row and its shadow current before the shadow is read as a whole or
        replaced.  Nothing pending: no launch.  (``flush_tables`` refuses to run inside a recording.)"""
        flush = getattr(self.opt, "flush_tables", None)
        if flush is not None:
            flush()

    def _refuse_applied(self, who):
        if self.is_applied:
            raise RuntimeError("%s inside ema.applied(): the live range holds the averaged weights; leave the context first" % who)

    def state_dict(self):
        """The model's ``state_dict`` keys and shapes (host tensors): the live parameters from the shadow, everything else (dead
        parameters, buffers) copied from the model -- what the reference's model loads directly."""
        self._refuse_applied("ema.state_dict()")
        self._flush_lazy()
        st = self._store()
        out = {k: v.detach().cpu().clone() for k, v in self.opt.model.state_dict().items()}
        for n in st.live_names:
            o, k = st.index[n]
            out[n] = self.shadow[o:o + k].view(st._params[n].shape).cpu().clone()
        return out

    def load_state_dict(self, sd):
        """The inverse of :meth:`state_dict`: the live parameters' entries become the shadow (the seed is replaced)."""
        self._refuse_applied("ema.load_state_dict()")
        self._flush_lazy()          # (what is pending belongs to the old average: it is applied before the new one replaces it)
        st = self._store()
        for n in st.live_names:
            if n not in sd:
                raise KeyError("ema.load_state_dict: no entry for the parameter %s" % n)
            if tuple(sd[n].shape) != tuple(st._params[n].shape):
                raise ValueError("ema.load_state_dict: %s has shape %s, the model's parameter %s"
                                 % (n, tuple(sd[n].shape), tuple(st._params[n].shape)))
        for n in st.live_names:
            o, k = st.index[n]
            self.shadow[o:o + k].copy_(sd[n].reshape(-1).to(torch.float32))
        self._pending = False          # the loaded average replaces the seed


class FusedAdamW:
    """torch.optim.AdamW semantics (lr 1e-3, wd 1e-4, betas (.9,.999), eps 1e-8 at
    main_for_seq_leave_earlystop_SegMM.py:226) as ONE kernel over the contiguous live range of the
    flat parameter buffer.  Dead parameters (no gradient in the reference either) are never touched.

    ``max_grad_norm``: None (default) = no clipping, what the reference actually runs (its clip_grad_norm_ call at :298 gets an
    exhausted generator).  A positive float m (inf allowed) = ``torch.nn.utils.clip_grad_norm_(params, m)`` before every step:
    the 2-norm of every live gradient (segmm_grad_norm, fp64 sums, bitwise reproducible) and the coefficient
    min(1, m / (norm + 1e-6)) stay on the device, and AdamW multiplies the gradient by it as it reads it -- no host sync.
    ``grad_norm`` is the last step's norm as a 0-dim device tensor (valid until the next step; ``.item()`` syncs); m = inf
    reports the norm and never clips.  Unlike torch, ``.grad`` keeps the UNCLIPPED gradient after the step.  A non-finite norm
    propagates as in torch, except to the id-table rows without a gradient of a two-pass table update (stepped with g = 0).

    ``lr_schedule`` (:class:`LRSchedule`, a dict of its fields or a kind name; None = the rate travels by value, as ever): the
    rate of every step is evaluated on the DEVICE from ``lr`` (the base rate) and the schedule, inside the launch that advances
    the step state, and the AdamW kernels read it there -- so it may move under a recorded step.  Needs the device step state
    (``Trainer(device_state=True)``).  ``set_base_lr`` moves the base rate between two steps, ``current_lr`` is the host's value
    of the coming step's rate, ``device_lr`` reads the device's (a sync).

    ``param_groups`` (None = one rate and one decay for the whole live range, today's launches and bits): a list of dicts
    ``{"params": ..., "lr_scale": 1.0, "weight_decay": <the optimizer's>, "frozen": False}``.  ``params`` is a list of exact names
    or fnmatch patterns over ``model.named_parameters()``, or a callable ``(name, parameter) -> bool``; a parameter two groups
    select, a pattern that selects nothing and any other key (``betas`` and ``eps`` included: one pair for every group, the device
    step state's contract) are refused by name.  What no group selects is the default group (scale 1, the optimizer's decay).  A
    group steps at fp32(rate x lr_scale), the rate being ``lr`` or, under ``lr_schedule``, the device's rate of that step: every
    schedule, ``set_base_lr`` and PlateauLR move all groups at once.  The step stays ONE launch per range (segmm_adamw_groups): the
    groups become segments of the live range (``group_segments``), a small table in device memory that is rebuilt only with the
    flat buffer, so a recorded step replays with unchanged arguments; element for element the result is that of segmm_adamw on the
    element's segment alone.  A FROZEN parameter is neither read nor written by the step (no p, m, v), its gradient stays out of
    the clipping norm (torch: ``grad=None``) and ``state_dict()["state"]`` has no entry for it; its ``.grad`` is still what the
    backward delivers -- the backward's work for frozen parameters is NOT skipped, freezing saves optimizer traffic only.  Dead
    parameters may be listed; they stay untouched as ever.  ``no_decay_groups(model)`` is the usual no-decay recipe,
    ``group_of(name)`` a parameter's resolved values.

    ``ema`` (None = nothing is launched or allocated; a decay, or ``dict(decay=0.999, warmup=True)``): a :class:`WeightEMA` of the
    live parameters, ``opt.ema``, updated by ``end_step`` with one launch behind the step's last AdamW launch.

    ``lazy_tables`` (None = every launch as ever; True, or ``dict(flush_every=F)``): LAZY EXACT AdamW of the id-embedding tables
    the trainer hands to :meth:`table_lazy`.  A step touches only the batch's rows: at its head they replay the g = 0 steps they
    missed (segmm_adamw_table_catchup, from a ring of the last F steps' rate and bias corrections and a per-row step stamp), at its
    tail they take today's phase-1 launch and the stamp of the step; no other row is read or written.  Nothing is dropped or
    approximated: after :meth:`flush_tables` the table, both moments included, holds the bits of the dense update.  The host
    flushes between steps once F steps have passed since the last flush (the ring's capacity), and before a step whose betas, eps,
    decay or group scale differ from the pending steps' (the ring holds only what a schedule moves).  ``state_dict()`` flushes
    first: a checkpoint is byte for byte the dense one, with no new keys; ``load_state_dict`` and a rebuild of the flat buffer
    discard what is pending and set every stamp to ``step_count`` -- flush before loading weights into a model with pending rows
    (``CheckPointer`` and the trainer's evaluation passes do).  A rebuild of the flat buffer with rows pending LOSES their pending
    decay and momentum steps (the moments are zeroed there as ever): from then on the run is not the dense run's; call
    ``flush_tables()`` before anything that rebuilds the buffer.  ``tables_pending``: the steps since the last flush.  Refused by
    name: an EMA without the ``ema`` key below (its shadow would average stale rows), unknown keys, flush_every < 1, :meth:`table_lazy` with ``flush_every`` steps
    pending (the trainer calls :meth:`lazy_step_head` first).  A forward of the caller's own (not ``Trainer.train_step``) reads the
    table as it stands: call ``flush_tables()`` before it.  ``step()`` for a lazy table that did not come through
    :meth:`table_lazy` steps it densely and sets every stamp; with steps pending it raises, because that forward read stale rows.
    ``dict(data_parallel=True)`` (a bool, default False; combinable with ``flush_every``; ``opt.lazy_data_parallel``): the opt-in to
    lazy tables under an active DPComm.  The rows a step touches there are all ranks' rows, known after the row exchange: the head is
    ``table_lazy(name, own_ids, mark=False)`` -- the rank's own rows catch up, nothing is marked or queued -- and the tail
    :meth:`table_lazy_rows` on the gathered list (segmm_adamw_table_lazy_rows: replay, this step and the stamp in one launch), while
    the dense launches walk around the table (:meth:`step_ranges`).  Stamps, ring and flush rule depend on the step count only:
    every rank flushes at the same step and holds the same bits, without a collective.  Without an active comm the key changes nothing.
    ``dict(ema=True)`` (a bool, default False; combinable with both other keys; ``opt.lazy_ema``): the opt-in to lazy tables beside
    ``ema=...``.  A row's shadow depends on the row's own p_t and step t's weight only, so it is replayed with the row, in order, with
    segmm_ema_update's three rounded operations; the ring's fourth float holds the weight each step used (``ema.decay`` may move
    between steps without a flush).  A step is then, single process or data parallel: ``table_lazy(name, own_ids, mark=False)``
    (segmm_adamw_table_catchup_ema, behind the seeding of the shadow), the dense ranges around the table, the ring's entry
    (segmm_adamw_hist_push_ema), :meth:`table_lazy_rows` on the step's list -- ``step(lazy_rows={name: ids})``, single process the
    batch's own ids -- (segmm_adamw_table_lazy_rows_ema) and the EMA's update around the table; no phase 1, no stamp launch, no flags.
    ``flush_tables()`` brings the shadow up with the rows; ``ema.applied()`` / ``ema.state_dict()`` / ``ema.load_state_dict()`` flush
    first, so evaluation on the averaged weights and ``"model_ema"`` in a checkpoint are the dense trainer's, bit for bit.  Without
    an EMA the key changes nothing.

    ``skip_nonfinite`` (False = every launch and every bit as ever; True): the NON-FINITE GUARD, what torch.cuda.amp.GradScaler.step
    does for torch's optimizers.  When the global 2-norm of a step's live, non-frozen gradient is NaN or +-inf -- it is finite iff
    every such element is -- the step changes no parameter, no moment and no EMA shadow, and is counted as skipped; training goes on
    with the next batch.  No host round trip, eager or recorded: the norm of ``max_grad_norm`` (run as ``max_grad_norm=inf`` when none
    is set: coefficient 1, ``grad_norm`` reports the norm) is followed by a one-thread launch (segmm_step_guard) that leaves the
    verdict and the count in the device step state, and every update of the step takes its *_guarded entry point, whose workgroups
    read the verdict first and return.  An applied step has the bits of the unguarded step.  ``step_count`` goes on counting
    ATTEMPTED steps, and the scheduled rate, the EMA warm-up and the dropout streams follow it (torch: ``sched.step()`` runs every
    iteration); the bias corrections of step t are those of the applied index t - skipped (torch: ``state["step"]`` moves on applied
    steps only).  ``skipped_steps`` reads the count (a sync), ``applied_steps`` = ``step_count`` - ``skipped_steps``;
    ``state_dict()`` writes ``"step"`` = applied steps and ``segmm_skipped_steps`` into every ``param_groups`` entry, and
    ``load_state_dict`` restores both (a checkpoint without the key: 0 skipped).  Needs the device step state
    (``Trainer(device_state=True)``); refused beside ``lazy_tables``.  ``.grad`` keeps what the backward delivered."""

    def __init__(self, model, lr=1e-3, weight_decay=1e-4, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None, lr_schedule=None,
                 param_groups=None, ema=None, lazy_tables=None, skip_nonfinite=False):
        self.model, self.lr, self.wd, self.betas, self.eps = model, lr, weight_decay, betas, eps
        self.skip_nonfinite = parse_skip_nonfinite(skip_nonfinite, None, lazy_tables)
        ema = parse_ema(ema)
        self.ema = None if ema is None else WeightEMA(self, *ema)
        # flush_every (= the ring's capacity) or None; _lazy: name -> dict(stamps, flags, o, rows, width) of the tables stepped lazily
        self.lazy_flush_every = parse_lazy_tables(lazy_tables)
        self._lazy, self._lazy_hist, self._lazy_flushed, self._lazy_snap = {}, None, 0, None
        # lazy_tables=dict(data_parallel=True): the trainer may step the tables lazily under an active DPComm (table_lazy with
        # mark=False at the head, table_lazy_rows at the tail).  _lazy_tail: name -> (o, n) of the tables whose head has run that
        # way -- the ranges the dense launches of the step walk around (step_ranges); _lazy_pushed: the step whose ring entry is in
        self.lazy_data_parallel = parse_lazy_data_parallel(lazy_tables)
        self._lazy_tail, self._lazy_pushed = {}, 0
        # lazy_tables=dict(ema=True): lazy tables beside the weight average -- a lazy row's shadow is replayed with the row (the
        # *_ema launches); every lazy step then runs as table_lazy(mark=False) + table_lazy_rows, single process too.  Without an
        # EMA the key changes nothing (_lazy_ema_on: the mode itself)
        self.lazy_ema = parse_lazy_ema(lazy_tables)
        # resolved groups (resolve_param_groups; entry 0 = the default group) or None; _segs: their segment table on the device
        self.groups = None if param_groups is None else resolve_param_groups(list(model.named_parameters()), param_groups, weight_decay)
        self._group_idx = None if self.groups is None else {n: gi for gi, G in enumerate(self.groups) for n in G["names"]}
        self._segs = self._segs_host = None
        self.max_grad_norm = _check_max_grad_norm(max_grad_norm)
        self.schedule = LRSchedule.parse(lr_schedule, lr)
        self.step_count = 0
        self.m = self.v = None
        self._flat_id = None
        self._clip_out = self._clip_scratch = None          # {norm, coef} of the last step; the norm's fp64 partials

    def _state(self):
        st = self.model._store
        st.ensure()
        if self.m is None or self._flat_id != st.flat.data_ptr():
            self.m = torch.zeros(st.n_live, device=st.flat.device)
            self.v = torch.zeros(st.n_live, device=st.flat.device)
            self._flat_id = st.flat.data_ptr()
            self._segs = None
            self._lazy = {}          # (what was pending went with the old moments: the next table_lazy stamps every row step_count)
            self._lazy_tail = {}
            if self.ema is not None:          # (re-)seeded where m and v are zeroed: from the parameters of the moment
                self.ema._seed(st)
        if self.groups is not None and self._segs is None:
            self._build_segments(st)
        return st

    # ---- parameter groups
    def group_of(self, name):
        """``(lr_scale, weight_decay, frozen)`` of the parameter ``name`` as the step applies them (fp32 values)."""
        if self.groups is None:
            if name not in dict(self.model.named_parameters()):
                raise KeyError("group_of: the model has no parameter %s" % name)
            return 1.0, _f32(self.wd), False
        if name not in self._group_idx:
            raise KeyError("group_of: the model has no parameter %s" % name)
        G = self.groups[self._group_idx[name]]
        return G["lr_scale"], G["weight_decay"], G["frozen"]

    def group_table(self):
        """The resolved groups as a hashable value (Trainer._hyper: a recorded step is refused once it differs)."""
        return None if self.groups is None else tuple((tuple(G["names"]), G["lr_scale"], G["weight_decay"], G["frozen"]) for G in self.groups)

    def _build_segments(self, st):
        """The groups as segments of the store's live range, in persistent device tensors (ends int64, lr_scale and weight_decay
        float32, frozen bytes).  An existing table of the same length is rewritten in place: the launches of a recorded step name
        these tensors.  ``_segs_arg`` is what the AdamW launches get: without a frozen segment no flags at all, which lets the
        kernel load its elements without waiting for the table."""
        order = sorted((st.index[n] + (n,) for n in st.live_names))
        segs = group_segments([(n, o, k) for o, k, n in order], st.n_live, self.group_of)
        cols = list(zip(*segs))
        dev = st.flat.device
        new = tuple(torch.tensor(c, dtype=dt) for c, dt in zip(cols, (torch.int64, torch.float32, torch.float32, torch.uint8)))
        if self._segs is not None and self._segs[0].numel() == len(segs) and self._segs[0].device == dev:
            for old, t in zip(self._segs, new):
                old.copy_(t)
        else:
            self._segs = tuple(t.to(dev) for t in new)
        self._segs_host = segs
        self._any_frozen = any(s[3] for s in segs)
        self._segs_arg = self._segs if self._any_frozen else self._segs[:3] + (None,)

    def _frozen(self, name):
        return self.groups is not None and self.groups[self._group_idx[name]]["frozen"]

    def zero_grad(self, set_to_none=True):
        plist = self.__dict__.get("_plist")
        if plist is None:          # the Parameter objects of a model do not change; walking the module tree costs 0.3 ms per step
            plist = self._plist = list(self.model.parameters())
        for p in plist:
            p.grad = None

    @property
    def grad_norm(self) -> Optional[torch.Tensor]:
        """The 2-norm of the last step's gradients (before clipping) as a 0-dim device tensor, None without ``max_grad_norm``."""
        return None if (self.max_grad_norm is None and not self.skip_nonfinite) or self._clip_out is None else self._clip_out[0]

    # ---- the non-finite guard (skip_nonfinite=True)
    def _guard_state(self, what):
        """Binds the device step state for a call of the guard; refuses, by name, an optimizer that has none."""
        if not self.__dict__.get("device_state", False) or self.__dict__.get("_step_state") is None:
            raise RuntimeError("%s: skip_nonfinite needs the device step state -- build the optimizer through Trainer(device_state=True)" % what)
        H.step_bind(self._step_state)

    def _guard_kw(self):
        """What the step's update launches get on top of their arguments: ``guard=True`` under skip_nonfinite, else nothing."""
        return {"guard": True} if self.__dict__.get("skip_nonfinite", False) else {}

    @property
    def skipped_steps(self):
        """The steps the non-finite guard has skipped (the device's count: synchronises); 0 without the guard."""
        if not self.skip_nonfinite:
            return 0
        self._guard_state("skipped_steps")
        return H.step_get_skipped()[1]

    @property
    def applied_steps(self):
        """``step_count`` - ``skipped_steps``: torch's ``state["step"]``."""
        return self.step_count - self.skipped_steps

    @property
    def skipped(self):
        """This step's verdict as a 0-dim int32 device tensor (1: skipped), a view of the device step state: valid until the head of
        the next step.  None without the guard."""
        if not self.skip_nonfinite:
            return None
        self._guard_state("skipped")
        return self._step_state[H.STEP_SKIP_WORD]

    def _coef(self):
        return None if self.max_grad_norm is None else self._clip_out[1:2]

    # ---- the learning rate: by value, or (lr_schedule) the device step state's
    def _bound_state(self, what):
        """Binds this optimizer's device step state for a call that reads or writes the scheduled rate."""
        if not self.__dict__.get("device_state", False) or self.__dict__.get("_step_state") is None:
            raise RuntimeError("%s: lr_schedule needs the device step state -- build the optimizer through Trainer(device_state=True)" % what)
        H.step_bind(self._step_state)

    def _lr_arg(self):
        """The lr argument of the AdamW launches: the rate itself, or the sentinel that makes the kernels read the device's."""
        if self.schedule is None:
            return self.lr
        self._bound_state("step")
        return H.LIVE_LR

    def _install_schedule(self):
        """Writes the schedule and the base rate into the bound step state (whose step count is already set)."""
        s = self.schedule
        self._bound_state("lr_schedule")
        H.step_schedule(s.kind, self.lr, s.warmup_steps, s.start_factor, max(s.decay_steps, 1), s.eta_min, s.gamma, s.step_size)

    def set_base_lr(self, lr):
        """Moves the base rate (segmm_step_set_base_lr, stream-ordered, no sync): the schedule continues from the new base.  Legal
        between any two steps, eager or replayed from a recording."""
        if self.schedule is None:
            raise RuntimeError("set_base_lr needs an lr_schedule (\"constant\" suffices); without one assign opt.lr and record() again")
        self.schedule.check_base(float(lr))
        self._bound_state("set_base_lr")
        H.step_set_base_lr(float(lr))
        self.lr = float(lr)

    def current_lr(self):
        """The rate the NEXT step runs at, from the host's copy of the schedule (no sync); the device computes the same closed form
        with its own cos / pow, so ``device_lr`` after that step's launch may differ in the last fp32 bit."""
        return self.lr if self.schedule is None else self.schedule.lr_at(self.lr, self.step_count)

    def device_lr(self):
        """The rate in the device step state: that of the last step enqueued (of the first one before any).  Synchronises."""
        self._bound_state("device_lr")
        return H.step_get_lr()[0]

    def step(self, gbuf=None, lazy_rows=None):
        """``lazy_rows`` (data parallel, ``lazy_tables=dict(data_parallel=True)``): name -> the gathered id list of all ranks, for
        every table whose head ran as ``table_lazy(name, own_ids, mark=False)``; those tables take :meth:`table_lazy_rows` behind the
        dense ranges, which walk around them.  Single process such heads run under ``lazy_tables=dict(ema=True)`` beside an EMA: the
        list is the batch's own."""
        lazy_rows = lazy_rows or {}
        missing = sorted(n for n in self._lazy_tail if n not in lazy_rows)
        if missing:
            raise RuntimeError("lazy_tables: step() after table_lazy(..., mark=False) for %s needs the step's gathered id list "
                               "(step(lazy_rows={name: ids_all})): the dense ranges skip these tables" % ", ".join(missing))
        # a lazy table that did not come through table_lazy this step (a forward and backward of the caller's own): it is stepped
        # densely, with the rest of the live range -- which is the dense run's step only if every row was current when the forward
        # read the table.  Flushing here would be too late: the gradients are already those of stale rows
        covered = {e[7] for e in self.__dict__.get("_early", [])} | set(self._lazy_tail)
        dense_lazy = bool(self._lazy) and any(name not in covered for name in self._lazy)
        if dense_lazy and self.tables_pending:
            raise RuntimeError("lazy_tables: step() without table_lazy() for %s while %d steps are pending -- the forward read rows that "
                               "were behind; call flush_tables() BEFORE a forward that does not go through Trainer.train_step"
                               % (", ".join(sorted(self._lazy)), self.tables_pending))
        early = self.__dict__.pop("_early", [])
        if dense_lazy:
            for e in early:
                if e[7] is not None:
                    H.fill_zero(e[5])
            early = [e for e in early if e[7] is None]
        self.begin_step(gbuf)
        st = self._state()
        pos = 0
        live = self.__dict__.get("device_state", False)
        pushed = False
        # id tables whose rows without a gradient were already stepped at the head of the step (table_early) or are stepped
        # lazily (table_lazy): the listed rows now, with their gradients; everything else as contiguous ranges around them
        for o, n, rows, width, ids, flags, hyper, lazy in sorted(early, key=lambda e: e[0]):
            self.step_ranges(pos, o, gbuf)
            step = -1 if live else self.step_count
            if lazy is not None and not pushed:          # this step's entry of the ring: the rate and bias corrections phase 1 uses
                H.adamw_hist_push(self._lazy_hist, self._lr_arg(), self.betas[0], self.betas[1], step)
                pushed = True
            if hyper is None:
                H.adamw_table(st.flat, st.gflat if gbuf is None else gbuf, self.m, self.v, o, rows, width, ids, flags, self._lr_arg(), self.betas[0],
                              self.betas[1], self.eps, self.wd, step, 1, coef=self._coef())
            else:          # (an id table lies in one group by construction: it is one parameter)
                H.adamw_table_lrs(st.flat, st.gflat if gbuf is None else gbuf, self.m, self.v, o, rows, width, ids, flags, self._lr_arg(), hyper[0],
                                  self.betas[0], self.betas[1], self.eps, hyper[1], step, 1, coef=self._coef())
            if lazy is not None:
                H.adamw_table_stamp(ids, rows, self._lazy[lazy]["stamps"], 0 if live else self.step_count, relative=live)
            pos = o + n
        self.step_ranges(pos, st.n_live, gbuf)
        for name in sorted(lazy_rows):
            self.table_lazy_rows(name, lazy_rows[name], gbuf)
        if dense_lazy:
            self._lazy_restamp()
        self.end_step()

    # ---- lazy exact AdamW of the id tables (lazy_tables=...)
    @property
    def tables_pending(self):
        """The optimizer steps since the last flush of the lazy tables (0: every row is current)."""
        return self.step_count - self._lazy_flushed if self._lazy else 0

    @property
    def _lazy_ema_on(self):
        """``lazy_tables=dict(ema=True)`` beside an EMA: the lazy tables' shadow rows are replayed with the rows."""
        return self.lazy_ema and self.ema is not None and self.lazy_flush_every is not None

    def _lazy_hyper_now(self):
        """What a replayed step takes from the launch arguments, not from the ring: betas, eps and each lazy table's (scale, decay)."""
        tabs = tuple((n,) + ((1.0, self.wd) if self.groups is None else tuple(self.group_of(n)[:2])) for n in sorted(self._lazy))
        return (tuple(self.betas), self.eps, tabs)

    def _lazy_restamp(self):
        """Every row of every lazy table has taken ``step_count`` steps (a dense step, a loaded checkpoint)."""
        for e in self._lazy.values():
            H.adamw_table_stamp(None, e["rows"], e["stamps"], self.step_count)
        self._lazy_flushed = self.step_count
        self._lazy_pushed = 0          # (a loaded count may meet the number of a step whose entry is in the ring: it is pushed again)

    def flush_tables(self):
        """Brings every row of the lazy tables to ``step_count`` (segmm_adamw_table_catchup over all rows, with the hyperparameters of
        the pending steps); nothing is launched when nothing is pending.  Never part of a recorded step."""
        if self.tables_pending == 0:
            return
        if H.RECORDER is not None:
            raise RuntimeError("flush_tables() inside a recorded step: the flush of the lazy tables is a host decision between steps")
        st = self._state()
        if self.tables_pending == 0:          # (the flat buffer was rebuilt: nothing is pending any more)
            return
        betas, eps, tabs = self._lazy_snap
        for name, scale, wd in tabs:
            e = self._lazy[name]
            if self._lazy_ema_on:          # the rows' shadow catches up with them, lerp by lerp with the ring's weights
                H.adamw_table_catchup_ema(st.flat, self.m, self.v, self.ema.shadow, e["o"], e["o"], e["rows"], e["width"], None, e["stamps"],
                                          self._lazy_hist, self.step_count, scale, betas[0], betas[1], eps, wd)
            else:
                H.adamw_table_catchup(st.flat, self.m, self.v, e["o"], e["rows"], e["width"], None, e["stamps"], self._lazy_hist, self.step_count,
                                      scale, betas[0], betas[1], eps, wd)
        self._lazy_flushed = self.step_count

    def lazy_step_head(self):
        """Between two steps, before the next one begins (the trainer calls it; never inside a recording): the periodic flush, once
        ``flush_every`` steps are pending -- the ring holds no more -- and the flush ahead of a changed hyperparameter."""
        pending = self.tables_pending
        if pending and (pending >= self.lazy_flush_every or self._lazy_snap != self._lazy_hyper_now()):
            self.flush_tables()

    def table_lazy(self, name, ids, mark=True):
        """Head of a lazy step of the id-embedding table ``name``, on the current stream and AHEAD of the forward that reads the rows:
        the rows in ``ids`` replay the steps they missed, up to the one before this (segmm_adamw_table_catchup), and are marked for
        this step's phase 1, which ``step()`` runs with the ring's new entry and the rows' new stamp.  Correct whether or not the
        step then happens: a row caught up to step T - 1 holds what the dense run holds after T - 1.
        ``mark=False`` (data parallel: ``ids`` are this rank's own, the step's rows are known after the row exchange): the rows catch
        up and nothing else happens -- no flags, nothing queued; the table's range is left out of the step's dense launches
        (:meth:`step_ranges`) and the tail is :meth:`table_lazy_rows` on the gathered list."""
        if self.lazy_flush_every is None:
            raise RuntimeError("table_lazy needs FusedAdamW(lazy_tables=...)")
        if self.ema is not None and not self.lazy_ema:
            raise RuntimeError("lazy_tables with ema: the shadow would average the stale rows of the lazy table %s; use one of the two, or "
                               "opt in to the lazily averaged shadow with lazy_tables=dict(ema=True)" % name)
        if self._lazy_ema_on and mark:
            raise RuntimeError("table_lazy(%s): lazy_tables=dict(ema=True) steps its rows in one launch at the tail -- the head is "
                               "table_lazy(name, ids, mark=False), the tail step(lazy_rows={name: ids})" % name)
        st = self._state()
        if self._lazy_ema_on:
            self.ema.step_head(st)          # the shadow is seeded before anything moves the table's rows (or replays their shadow)
        if self.tables_pending >= self.lazy_flush_every:          # the ring rule: target - stamp <= cap, or a replay reads an overwritten slot
            raise RuntimeError("table_lazy: %d steps are pending and the ring holds %d -- call lazy_step_head() (or flush_tables()) "
                               "between steps, before the step begins" % (self.tables_pending, self.lazy_flush_every))
        if self._frozen(name):          # nothing to step, now or later
            return
        hyper = None if self.groups is None else self.group_of(name)[:2]
        o, n = st.index[name]
        rows, width = st._params[name].shape
        dev = st.flat.device
        e = self._lazy.get(name)
        if e is None:
            H.torch_fallback("the first lazy step of the table %s (its stamps are made; record() after one eager step)" % name)
            if not self._lazy:
                self._lazy_flushed = self.step_count
            e = self._lazy[name] = dict(o=o, rows=rows, width=width, flags=torch.zeros((rows,), dtype=torch.int32, device=dev),
                                        stamps=torch.full((rows,), self.step_count, dtype=torch.int32, device=dev))
        if self._lazy_hist is None or self._lazy_hist.device != dev:
            self._lazy_hist = torch.zeros((self.lazy_flush_every, 4), dtype=torch.float32, device=dev)
        live = self.__dict__.get("device_state", False)
        scale, wd = (1.0, self.wd) if hyper is None else hyper
        if self._lazy_ema_on:
            H.adamw_table_catchup_ema(st.flat, self.m, self.v, self.ema.shadow, o, o, rows, width, ids, e["stamps"], self._lazy_hist,
                                      -1 if live else self.step_count, scale, self.betas[0], self.betas[1], self.eps, wd, relative=live)
        else:
            H.adamw_table_catchup(st.flat, self.m, self.v, o, rows, width, ids, e["stamps"], self._lazy_hist, -1 if live else self.step_count, scale,
                                  self.betas[0], self.betas[1], self.eps, wd, relative=live, flags=e["flags"] if mark else None)
        self._lazy_snap = self._lazy_hyper_now()
        if mark:
            self.__dict__.setdefault("_early", []).append((o, n, rows, width, ids, e["flags"], hyper, name))
        else:
            self._lazy_tail[name] = (o, n)

    def table_lazy_rows(self, name, ids_all, gbuf=None):
        """Tail of a data-parallel lazy step of the table ``name``, between ``begin_step`` and ``end_step`` on the stream that holds
        the table's reduced gradient: the ring's entry of this step (once per step, whatever the number of tables), then ONE launch
        (segmm_adamw_table_lazy_rows) over ``ids_all``, the gathered id list of all ranks -- every listed row replays what it
        missed up to the step before, takes this step with its gradient row and is stamped.  A frozen table launches nothing."""
        if self._frozen(name):
            return
        if name not in self._lazy_tail or name not in self._lazy:
            raise RuntimeError("table_lazy_rows(%s) without table_lazy(%s, own_ids, mark=False) at the head of this step: the dense "
                               "launches of the step have covered the table's range" % (name, name))
        st = self._state()
        e = self._lazy[name]
        live = self.__dict__.get("device_state", False)
        step = -1 if live else self.step_count
        ema = self.ema if self._lazy_ema_on else None
        if self._lazy_pushed != self.step_count:
            if ema is not None:          # ... and the weight of this step's lerp: the launch below reads it from the ring
                H.adamw_hist_push_ema(self._lazy_hist, self._lr_arg(), self.betas[0], self.betas[1], step, ema.weight, ema.warmup)
            else:
                H.adamw_hist_push(self._lazy_hist, self._lr_arg(), self.betas[0], self.betas[1], step)
            self._lazy_pushed = self.step_count
        scale, wd = (1.0, self.wd) if self.groups is None else self.group_of(name)[:2]
        if ema is not None:
            H.adamw_table_lazy_rows_ema(st.flat, st.gflat if gbuf is None else gbuf, self.m, self.v, ema.shadow, e["o"], e["o"], e["rows"], e["width"],
                                        ids_all, e["stamps"], self._lazy_hist, self._lr_arg(), scale, self.betas[0], self.betas[1], self.eps, wd,
                                        step, coef=self._coef())
        else:
            H.adamw_table_lazy_rows(st.flat, st.gflat if gbuf is None else gbuf, self.m, self.v, e["o"], e["rows"], e["width"], ids_all, e["stamps"],
                                    self._lazy_hist, self._lr_arg(), scale, self.betas[0], self.betas[1], self.eps, wd, step, coef=self._coef())
        self._lazy_snap = self._lazy_hyper_now()

    def step_ranges(self, start, end, gbuf=None):
        """``step_range`` over [start, end) minus the ranges of the tables :meth:`table_lazy_rows` steps this step (none: the one
        launch of ``step_range``).  Every dense launch of a step goes through here: the per-bucket schedule, the clipped single
        range and ``step()``."""
        pos = start
        for o, n in sorted(self._lazy_tail.values()):
            if o + n <= pos or o >= end:
                continue
            self.step_range(pos, max(pos, o), gbuf)
            pos = min(end, o + n)
        self.step_range(pos, end, gbuf)

    def early_on_aux(self):
        """True while a two-pass table's phase 0 of this step is queued (on the auxiliary stream: join it before ``step()``)."""
        return any(e[7] is None for e in self.__dict__.get("_early") or ())

    def table_early(self, name, ids):
        """First pass of the two-pass update of the id-embedding table ``name`` (segmm_adamw_table): every row that is NOT in
        ``ids`` -- the rows the coming backward gives no gradient -- takes its AdamW step of THIS optimizer step now, with g = 0,
        on the current stream (the trainer calls this at the head of the step on a stream of its own: the forward and backward
        only read the listed rows).  ``step()`` then updates the listed rows and skips the table's range.  Element for element
        the arithmetic of the one-launch dense update."""
        if self.skip_nonfinite:
            raise RuntimeError("table_early(%s) under skip_nonfinite: the early pass runs before the step's verdict exists; the guarded "
                               "step takes the table densely at its tail (step() without an early entry)" % name)
        st = self._state()
        if self.ema is not None:
            self.ema.step_head(st)          # this pass is the step's first parameter write
        if self._frozen(name):          # nothing to step, now or later: step() walks over the table's range, which the kernel skips
            return
        hyper = None if self.groups is None else self.group_of(name)[:2]
        o, n = st.index[name]
        rows, width = st._params[name].shape
        fl = self.__dict__.setdefault("_table_flags", {})
        flags = fl.get(name)
        if flags is None or flags.numel() != rows or flags.device != st.flat.device:
            flags = fl[name] = torch.zeros((rows,), dtype=torch.int32, device=st.flat.device)
        step = -1 if self.__dict__.get("device_state", False) else self.step_count + 1
        if hyper is None:
            H.adamw_table(st.flat, None, self.m, self.v, o, rows, width, ids, flags, self._lr_arg(), self.betas[0], self.betas[1], self.eps, self.wd,
                          step, 0)
        else:
            H.adamw_table_lrs(st.flat, None, self.m, self.v, o, rows, width, ids, flags, self._lr_arg(), hyper[0], self.betas[0], self.betas[1],
                              self.eps, hyper[1], step, 0)
        self.__dict__.setdefault("_early", []).append((o, n, rows, width, ids, flags, hyper, None))

    # one optimizer step as several launches over disjoint ranges that together cover the live range: the data-parallel
    # trainer steps each gradient bucket as soon as ITS all-reduce has completed (begin_step, step_range ..., end_step)
    def begin_step(self, gbuf=None):
        st = self._state()
        if self.ema is not None:
            self.ema.step_head(st)
        self.step_count += 1
        if not st.__dict__.get("direct_grads", False):
            self._sync_grads(st)
        if self.skip_nonfinite:
            self._guard_state("step")
        if self.max_grad_norm is not None or self.skip_nonfinite:
            max_norm = math.inf if self.max_grad_norm is None else self.max_grad_norm          # (the guard alone: the norm, never a clip)
            # the global norm reads every live gradient: the caller enqueues this once all of them are complete (train_step: the
            # tail stream, after the side / auxiliary streams have joined and, under data parallelism, every bucket is reduced)
            if self._clip_out is None or self._clip_out.device != st.flat.device:
                self._clip_out = torch.zeros(2, dtype=torch.float32, device=st.flat.device)
                self._clip_scratch = torch.zeros(H.GRAD_NORM_SCRATCH, dtype=torch.float64, device=st.flat.device)
            if self.groups is not None and self._any_frozen:          # frozen gradients stay out of the norm (torch: grad = None)
                H.grad_norm_groups(st.gflat if gbuf is None else gbuf, st.n_live, self._segs, max_norm, self._clip_scratch, self._clip_out)
            else:
                H.grad_norm(st.gflat if gbuf is None else gbuf, st.n_live, max_norm, self._clip_scratch, self._clip_out)
            if self.skip_nonfinite:          # the verdict, behind the norm's finish on this stream and ahead of every update of the step
                H.step_guard(self._clip_out)

    def _sync_grads(self, st):
        """The kernel reads the FLAT gradient buffer.  After Trainer.train_step the parameters' ``.grad`` ARE views of it
        (engine.deliver_grads).  After any other backward (``loss.backward()``: gradients arrive through autograd, possibly
        rewritten by hooks, clipped or accumulated over several backwards) they are tensors of their own: copy them in."""
        base = st.gflat.data_ptr()
        for n in st.live_names:
            g = st._params[n].grad
            if g is not None:
                o, k = st.index[n]
                if g.data_ptr() != base + 4 * o or not g.is_contiguous():
                    H.torch_fallback("the copy of %s.grad into the flat gradient buffer" % n)
                    st.gflat[o:o + k].view(g.shape).copy_(g)

    def step_range(self, start, end, gbuf=None):
        st = self._state()
        if self.__dict__.get("device_state", False) and self.__dict__.get("_step_state") is not None:
            # the bound step state is a process-global host pointer read when a launch is MADE; a direct opt.step() /
            # step_range() between two trainers' steps must not pick up the other trainer's seed words and bias corrections
            H.step_bind(self._step_state)
        step = -1 if self.__dict__.get("device_state", False) else self.step_count
        if end > start and self.groups is not None:
            H.adamw_groups(st.flat, st.gflat if gbuf is None else gbuf, self.m, self.v, start, end - start, self._segs_arg, self._lr_arg(), self.betas[0],
                           self.betas[1], self.eps, step, coef=self._coef(), **self._guard_kw())
        elif end > start:
            # device_state: the bias corrections come from the device-side step count (segmm_step_advance), step = -1
            H.adamw(st.flat, st.gflat if gbuf is None else gbuf, self.m, self.v, end - start, self._lr_arg(), self.betas[0], self.betas[1],
                    self.eps, self.wd, step, p_off=start, coef=self._coef(), **self._guard_kw())

    def end_step(self):
        if self.ema is not None:
            # behind every AdamW launch of this step on this stream; the next step's first parameter write -- phase 0 of a two-pass
            # id table on the auxiliary stream -- is enqueued behind engine.aux_work's fork from this stream
            self.ema.update()
        self._lazy_tail = {}          # (the next step's head names its tables again)
        self.model._store.fused_version += 1          # the pre-split weight planes of the GEMM engines are now stale

    def state_dict(self):
        """torch.optim.AdamW-format state (keyed by the index of the parameter in model.parameters()),
        so a checkpoint written here resumes under the reference's optimizer and vice versa."""
        self.flush_tables()          # lazy tables: the checkpoint is the dense one
        st = self._state()
        names = [n for n, _ in self.model.named_parameters()]
        state = {}
        # skip_nonfinite: "step" is the APPLIED count, as torch keeps it (one read-back; state_dict synchronises already)
        skipped = self.skipped_steps
        for i, n in enumerate(names):
            if n in st.live_names and not self._frozen(n):
                o, k = st.index[n]
                shape = st._params[n].shape
                state[i] = {"step": torch.tensor(float(self.step_count - skipped)), "exp_avg": self.m[o:o + k].view(shape).clone(),
                            "exp_avg_sq": self.v[o:o + k].view(shape).clone()}
        group = {"lr": self.lr, "betas": self.betas, "eps": self.eps, "weight_decay": self.wd, "amsgrad": False,
                 "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
                 "params": list(range(len(names)))}
        if self.schedule is not None:
            # torch's schedulers keep the base rate in "initial_lr" and the running one in "lr"; the descriptor is an extra key
            # torch.optim.AdamW.load_state_dict carries along untouched
            group.update(lr=self.current_lr(), initial_lr=self.lr, segmm_lr_schedule=dataclasses.asdict(self.schedule))
        if self.skip_nonfinite:          # (an extra key like segmm_lr_scale: step_count = "step" + this)
            group["segmm_skipped_steps"] = skipped
        if self.groups is None:
            return {"state": state, "param_groups": [group]}
        # one torch-format entry per group, the default group first (scale 1: its "lr" / "initial_lr" are the optimizer's own, as in
        # a one-group checkpoint).  "params" leaves the frozen parameters out, as a torch optimizer built without them would;
        # "segmm_frozen_params" names them, so that load_state_dict can tell a grouping from another.
        out = []
        for gi, G in enumerate(self.groups):
            idx = [i for i, n in enumerate(names) if self._group_idx[n] == gi]
            e = dict(group, weight_decay=G["weight_decay"] if gi else self.wd, segmm_lr_scale=G["lr_scale"], params=[] if G["frozen"] else idx)
            if G["lr_scale"] != 1.0:
                e["lr"] = _f32(_f32(group["lr"]) * G["lr_scale"])
                if "initial_lr" in e:
                    e["initial_lr"] = _f32(_f32(self.lr) * G["lr_scale"])
            if G["frozen"]:
                e["segmm_frozen_params"] = idx
            out.append(e)
        return {"state": state, "param_groups": out}

    def _check_grouping(self, sd, names):
        """Refuses, by the name of the first parameter that differs, a checkpoint whose grouping is not this optimizer's."""
        mine = [self._group_idx[n] for n in names] if self.groups is not None else [0] * len(names)
        theirs = {}
        for gi, g in enumerate(sd["param_groups"]):
            for i in list(g["params"]) + list(g.get("segmm_frozen_params", ())):
                theirs[int(i)] = gi
        for i, n in enumerate(names):
            if theirs.get(i) != mine[i]:
                raise ValueError("load_state_dict: the checkpoint has the parameter %s in %s, this optimizer in param group %d%s -- build "
                                 "the optimizer with the checkpoint's param_groups"
                                 % (n, "no param group" if i not in theirs else "param group %d" % theirs[i], mine[i],
                                    " (the default group)" if mine[i] == 0 else ""))
        n_mine = len(self.groups) if self.groups is not None else 1
        if len(sd["param_groups"]) != n_mine:
            raise ValueError("load_state_dict: the checkpoint has %d param groups, this optimizer %d" % (len(sd["param_groups"]), n_mine))
        for gi, g in enumerate(sd["param_groups"]):
            frozen = "segmm_frozen_params" in g
            if frozen != (self.groups is not None and self.groups[gi]["frozen"]):
                raise ValueError("load_state_dict: param group %d (%s ...) is %s in the checkpoint and %s in this optimizer"
                                 % (gi, names[int((list(g["params"]) + list(g.get("segmm_frozen_params", ())) + [0])[0])],
                                    "frozen" if frozen else "trained", "trained" if frozen else "frozen"))

    def load_state_dict(self, sd):
        if "segmm_lr_schedule" in sd["param_groups"][0]:          # (refused before anything is overwritten)
            self._bound_state("load_state_dict of a checkpoint written under an lr_schedule")
        names = [n for n, _ in self.model.named_parameters()]
        if self.groups is not None or len(sd["param_groups"]) > 1:
            self._check_grouping(sd, names)
        skipped = sd["param_groups"][0].get("segmm_skipped_steps", 0)          # (a checkpoint without the key: nothing was skipped)
        if isinstance(skipped, bool) or not isinstance(skipped, int) or skipped < 0:
            raise ValueError("load_state_dict: segmm_skipped_steps must be an int >= 0, not %r" % (skipped,))
        if skipped and not self.skip_nonfinite:
            raise ValueError("load_state_dict: the checkpoint counts %d skipped steps (segmm_skipped_steps); it resumes under "
                             "skip_nonfinite=True, where the attempted and the applied count are kept apart" % skipped)
        if self.skip_nonfinite:          # (refused before anything is overwritten)
            self._guard_state("load_state_dict")
        st = self._state()
        self.m.zero_()
        self.v.zero_()
        steps = set()
        for i, s in sd["state"].items():
            n = names[int(i)]
            if n in st.live_names and not self._frozen(n):
                o, k = st.index[n]
                self.m[o:o + k].copy_(s["exp_avg"].reshape(-1))
                self.v[o:o + k].copy_(s["exp_avg_sq"].reshape(-1))
                steps.add(int(float(s["step"])))
        self.step_count = (max(steps) if steps else 0) + skipped          # "step" holds the applied count; the host's counts attempts
        self._lazy_restamp()          # lazy tables: the loaded moments are every row's, at the loaded count; nothing stays pending
        g = sd["param_groups"][0]
        self.lr, self.wd, self.betas, self.eps = g["lr"], g["weight_decay"], tuple(g["betas"]), g["eps"]
        if self.groups is not None:          # the groups' own values (entry 0, the default group, follows the optimizer's decay)
            for G, e in zip(self.groups, sd["param_groups"]):
                G["lr_scale"] = _group_value(-1, "load_state_dict: segmm_lr_scale", e.get("segmm_lr_scale", 1.0))
                G["weight_decay"] = _group_value(-1, "load_state_dict: weight_decay", e["weight_decay"])
            self._build_segments(st)
        if "segmm_lr_schedule" in g:          # written under a schedule: "lr" is the rate of the next step, "initial_lr" the base
            self.lr = g["initial_lr"]
            self.schedule = LRSchedule.parse(g["segmm_lr_schedule"], self.lr)
        elif self.schedule is not None:
            self.schedule.check_base(float(self.lr))
        if self.__dict__.get("device_state", False):          # the device-side step count (bias corrections) follows the checkpoint
            H.step_bind(self._step_state)
            seed, _, _ = H.step_get()
            H.step_set(seed, self.step_count, *self.betas)
            if self.skip_nonfinite:          # (the next step's head takes its corrections from step_count + 1 - skipped)
                H.step_set_skipped(skipped)
            if self.schedule is not None:
                self._install_schedule()
