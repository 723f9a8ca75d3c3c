"""Training step of ``MMinterest/main_for_seq_leave_earlystop_SegMM.py:269-300`` on the HIP engine,
single GPU or data-parallel over the GPUs of one node (one process per GPU, RCCL over xGMI).

The reference trainer is single-process (DistributedDataParallel is imported at :13 and never used);
data parallelism is what this build adds:

* rows of the global batch are sharded contiguously over ranks, parameters are replicated;
* every cross-row normaliser of the losses (valid-row count of interestBPR, batch size, mask count) is
  made GLOBAL before the loss kernel runs -- one tiny all-reduce of 3 floats and one all-gather of the
  per-row view lengths -- so the sum of the per-rank gradients equals the single-process gradient of
  the whole batch exactly (no averaging step afterwards);
* gradients live in one flat buffer laid out in backward-completion order; each bucket (head, layer
  N-2, ..., layer 0, embedding) is all-reduced (SUM) asynchronously the moment its last gradient has
  been written, overlapping the remaining backward; the fused AdamW waits for the last bucket.

``init_model`` mirrors the reference's model construction (:60-130).
"""
from __future__ import annotations

import argparse
import contextlib
import dataclasses
import fnmatch
import functools
import math
import struct
from typing import Dict, List, Optional

import os

import ctypes
import torch
import torch.nn as nn

from . import engine as E
from . import hipabi as H
from . import switches
from .decoder_leave_focal import _LIDX, LossSpec, MultiScaleTemporalDetrLeaveFocal
from .encoder import SegFormerX


# ------------------------------------------------------------------------------------------------ model factory
def init_model(args, reader=None, n_users: Optional[int] = None, n_items: Optional[int] = None,
               input_dim: int = 1024, max_vid_len: int = 40, max_usr_len: int = 100, ff_dim=None):
    """init_model(args, reader) of the reference trainer (main_for_seq_leave_earlystop_SegMM.py:60-130).
    ``reader`` only needs ``n_users`` / ``n_items``; feature width and lengths default to the
    reference's hard-coded 1024 / 40 / 100 and are overridable for synthetic configs.
    ``ff_dim``: the encoder layers' feed-forward width, an int (every layer) or a list of ``num_layers_enc`` ints.  ``None`` is
    the reference's behaviour: ``[d_model] * N`` whatever ``args.ff_dim`` says (main...SegMM.py:91 never reads that option, whose
    default is 512 for every d_model: honouring it implicitly would change existing runs)."""
    n_users = reader.n_users if reader is not None else n_users
    n_items = reader.n_items if reader is not None else n_items
    N, d, h = args.num_layers_enc, args.d_model, args.nhead
    if ff_dim is None:
        ff = [d] * N
    elif isinstance(ff_dim, int):
        ff = [ff_dim] * N
    else:
        ff = [int(f) for f in ff_dim]
        if len(ff) != N:
            raise ValueError("ff_dim lists %d widths for num_layers_enc = %d" % (len(ff), N))

    def backbone(user_id_max, video_id_max, usr_len):
        return SegFormerX(d_model_in=d, d_model_lvls=[d] * N, num_head_lvls=[h] * N, ff_dim_lvls=ff,
                          input_vid_dim=input_dim, input_usr_dim=input_dim, max_vid_len=max_vid_len, max_usr_len=usr_len,
                          sr_ratio_lvls=[1] * N, use_patch_merge=[False] * N, output_layers=[-1], model_cfg=args,
                          user_id_max=user_id_max, video_id_max=video_id_max, use_pe=getattr(args, "use_pe", 1))

    u, p = args.input_type["user"], args.input_type["photo"]
    if u == "both" or p == "both":
        um1, ul1, um2, ul2 = {"both": (-1, max_usr_len, n_users, 1), "id": (n_users, 1, n_users, 1),
                              "image": (-1, max_usr_len, -1, max_usr_len)}[u]
        vm1, vm2 = {"both": (-1, n_items), "id": (n_items, n_items), "image": (-1, -1)}[p]
        return MultiScaleTemporalDetrLeaveFocal(backbone(um1, vm1, ul1), backbone(um2, vm2, ul2), None, nn.Identity(), args)
    um1, ul1 = (n_users, 1) if u == "id" else (-1, max_usr_len)
    vm1 = n_items if p == "id" else -1
    return MultiScaleTemporalDetrLeaveFocal(backbone(um1, vm1, ul1), None, None, nn.Identity(), args)


def default_args(**over):
    """The reference's argparse defaults that the model reads (main_for_seq_leave_earlystop_SegMM.py:478-575)."""
    a = argparse.Namespace(debug=0, num_layers_enc=6, ablation_type="ours", d_model=512, nhead=16,
                           input_type={"user": "both", "photo": "both"}, learnable_bias=0, exposure_prob=[1.0] * 40,
                           fusion_heads=2, loss_type_list=["interestBPR"],
                           loss_weight={"focal": 1.0, "mse": 1.0, "hazard": 1.0, "surviveCE": 1.0, "interestBPR": 1.0,
                                        "interestCE": 1.0, "interestKL": 1.0},
                           mask_loss=0, use_pe=1, learning_rate=1e-3, weight_decay=1e-4)
    for k, v in over.items():
        setattr(a, k, v)
    return a


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
    ``decay`` may be assigned between steps (a recorded step is then refused like after any hyperparameter change)."""

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
        """The step's update (FusedAdamW.end_step): one launch on the current stream."""
        if self.is_applied:
            raise RuntimeError("ema: an optimizer step inside ema.applied() (the live range holds the averaged weights)")
        opt = self.opt
        st = self._store()
        live = opt.__dict__.get("device_state", False)
        if live and opt.__dict__.get("_step_state") is not None:
            H.step_bind(opt._step_state)
        H.ema_update(self.shadow, st.flat, st.n_live, self.weight, self.warmup, -1 if live else opt.step_count)

    def _swap(self, st):
        H.vec_swap(st.flat, self.shadow, st.n_live)
        st.fused_version += 1          # the weight planes follow the live range: ParamStore.ensure() re-splits them

    @contextlib.contextmanager
    def applied(self):
        if self.is_applied:
            raise RuntimeError("ema.applied() is already active (nested applied() is refused)")
        if H.RECORDER is not None:
            raise RuntimeError("ema.applied() inside a recorded step")
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

    def _refuse_applied(self, who):
        if self.is_applied:
            raise RuntimeError("%s inside ema.applied(): the live range holds the averaged weights; leave the context first" % who)

    def state_dict(self):
        """The model's ``state_dict`` keys and shapes (host tensors): the live parameters from the shadow, everything else (dead
        parameters, buffers) copied from the model -- what the reference's model loads directly."""
        self._refuse_applied("ema.state_dict()")
        st = self._store()
        out = {k: v.detach().cpu().clone() for k, v in self.opt.model.state_dict().items()}
        for n in st.live_names:
            o, k = st.index[n]
            out[n] = self.shadow[o:o + k].view(st._params[n].shape).cpu().clone()
        return out

    def load_state_dict(self, sd):
        """The inverse of :meth:`state_dict`: the live parameters' entries become the shadow (the seed is replaced)."""
        self._refuse_applied("ema.load_state_dict()")
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
    live parameters, ``opt.ema``, updated by ``end_step`` with one launch behind the step's last AdamW launch."""

    def __init__(self, model, lr=1e-3, weight_decay=1e-4, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None, lr_schedule=None,
                 param_groups=None, ema=None):
        self.model, self.lr, self.wd, self.betas, self.eps = model, lr, weight_decay, betas, eps
        ema = parse_ema(ema)
        self.ema = None if ema is None else WeightEMA(self, *ema)
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
        return None if self.max_grad_norm is None or self._clip_out is None else self._clip_out[0]

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

    def step(self, gbuf=None):
        self.begin_step(gbuf)
        st = self._state()
        pos = 0
        # id tables whose rows without a gradient were already stepped at the head of the step (table_early): the listed rows
        # now, with their gradients; everything else as contiguous ranges around them
        for o, n, rows, width, ids, flags, hyper in sorted(self.__dict__.pop("_early", []), key=lambda e: e[0]):
            self.step_range(pos, o, gbuf)
            step = -1 if self.__dict__.get("device_state", False) else self.step_count
            if hyper is None:
                H.adamw_table(st.flat, st.gflat if gbuf is None else gbuf, self.m, self.v, o, rows, width, ids, flags, self._lr_arg(), self.betas[0],
                              self.betas[1], self.eps, self.wd, step, 1, coef=self._coef())
            else:          # (an id table lies in one group by construction: it is one parameter)
                H.adamw_table_lrs(st.flat, st.gflat if gbuf is None else gbuf, self.m, self.v, o, rows, width, ids, flags, self._lr_arg(), hyper[0],
                                  self.betas[0], self.betas[1], self.eps, hyper[1], step, 1, coef=self._coef())
            pos = o + n
        self.step_range(pos, st.n_live, gbuf)
        self.end_step()

    def table_early(self, name, ids):
        """First pass of the two-pass update of the id-embedding table ``name`` (segmm_adamw_table): every row that is NOT in
        ``ids`` -- the rows the coming backward gives no gradient -- takes its AdamW step of THIS optimizer step now, with g = 0,
        on the current stream (the trainer calls this at the head of the step on a stream of its own: the forward and backward
        only read the listed rows).  ``step()`` then updates the listed rows and skips the table's range.  Element for element
        the arithmetic of the one-launch dense update."""
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
        self.__dict__.setdefault("_early", []).append((o, n, rows, width, ids, flags, hyper))

    # one optimizer step as several launches over disjoint ranges that together cover the live range: the data-parallel
    # trainer steps each gradient bucket as soon as ITS all-reduce has completed (begin_step, step_range ..., end_step)
    def begin_step(self, gbuf=None):
        st = self._state()
        if self.ema is not None:
            self.ema.step_head(st)
        self.step_count += 1
        if not st.__dict__.get("direct_grads", False):
            self._sync_grads(st)
        if self.max_grad_norm is not None:
            # the global norm reads every live gradient: the caller enqueues this once all of them are complete (train_step: the
            # tail stream, after the side / auxiliary streams have joined and, under data parallelism, every bucket is reduced)
            if self._clip_out is None or self._clip_out.device != st.flat.device:
                self._clip_out = torch.zeros(2, dtype=torch.float32, device=st.flat.device)
                self._clip_scratch = torch.zeros(H.GRAD_NORM_SCRATCH, dtype=torch.float64, device=st.flat.device)
            if self.groups is not None and self._any_frozen:          # frozen gradients stay out of the norm (torch: grad = None)
                H.grad_norm_groups(st.gflat if gbuf is None else gbuf, st.n_live, self._segs, self.max_grad_norm, self._clip_scratch, self._clip_out)
            else:
                H.grad_norm(st.gflat if gbuf is None else gbuf, st.n_live, self.max_grad_norm, self._clip_scratch, self._clip_out)

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
                           self.betas[1], self.eps, step, coef=self._coef())
        elif end > start:
            # device_state: the bias corrections come from the device-side step count (segmm_step_advance), step = -1
            H.adamw(st.flat, st.gflat if gbuf is None else gbuf, self.m, self.v, end - start, self._lr_arg(), self.betas[0], self.betas[1],
                    self.eps, self.wd, step, p_off=start, coef=self._coef())

    def end_step(self):
        if self.ema is not None:
            # behind every AdamW launch of this step on this stream; the next step's first parameter write -- phase 0 of a two-pass
            # id table on the auxiliary stream -- is enqueued behind engine.aux_work's fork from this stream
            self.ema.update()
        self.model._store.fused_version += 1          # the pre-split weight planes of the GEMM engines are now stale

    def state_dict(self):
        """torch.optim.AdamW-format state (keyed by the index of the parameter in model.parameters()),
        so a checkpoint written here resumes under the reference's optimizer and vice versa."""
        st = self._state()
        names = [n for n, _ in self.model.named_parameters()]
        state = {}
        for i, n in enumerate(names):
            if n in st.live_names and not self._frozen(n):
                o, k = st.index[n]
                shape = st._params[n].shape
                state[i] = {"step": torch.tensor(float(self.step_count)), "exp_avg": self.m[o:o + k].view(shape).clone(),
                            "exp_avg_sq": self.v[o:o + k].view(shape).clone()}
        group = {"lr": self.lr, "betas": self.betas, "eps": self.eps, "weight_decay": self.wd, "amsgrad": False,
                 "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
                 "params": list(range(len(names)))}
        if self.schedule is not None:
            # torch's schedulers keep the base rate in "initial_lr" and the running one in "lr"; the descriptor is an extra key
            # torch.optim.AdamW.load_state_dict carries along untouched
            group.update(lr=self.current_lr(), initial_lr=self.lr, segmm_lr_schedule=dataclasses.asdict(self.schedule))
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
        self.step_count = max(steps) if steps else 0
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
            if self.schedule is not None:
                self._install_schedule()


# ------------------------------------------------------------------------------------------------ communication
class DPComm:
    """The three collectives of a data-parallel step (engine-agnostic; works on any torch.distributed
    backend, ``nccl`` = RCCL on the GPU box, ``gloo`` in the CPU tests)."""

    def __init__(self, group=None):
        import torch.distributed as dist
        self.dist = dist
        self.group = group
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        # every collective of the step is issued iff ``active``: more than one rank -- or SEGMM_DP_FORCE=1 with an initialised
        # process group of ONE rank, which sends the single-GPU step through the real RCCL calls (tests/test_dp_gpu.py: the
        # only way to execute the nccl code path on a one-GPU box; results must equal the plain step bit for bit)
        self.active = self.world > 1 or (switches.read("comm")["force"] and dist.is_initialized())
        self.pending = []
        # gloo has no device collectives for every op: device tensors are staged through the host.
        # Only the test harness uses that (two ranks sharing one GPU); production is nccl = RCCL.
        self.host_staged = dist.is_initialized() and dist.get_backend(group) == "gloo"

    def _all_reduce(self, t, async_op=False):
        if self.host_staged and t.is_cuda:
            h = t.cpu()
            self.dist.all_reduce(h, op=self.dist.ReduceOp.SUM, group=self.group)
            t.copy_(h)
            return None
        return self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM, group=self.group, async_op=async_op)

    def _pbuf(self, key, shape, dtype, device):
        """Persistent staging buffer of a collective: the SAME tensor every step, so that a recorded step (Trainer.record),
        whose kernels name the results by address, can be replayed around the collectives."""
        bufs = self.__dict__.setdefault("_bufs", {})
        b = bufs.get(key)
        if b is None or tuple(b.shape) != tuple(shape) or b.dtype != dtype or b.device != device:
            b = bufs[key] = torch.empty(shape, dtype=dtype, device=device)
        return b

    def label_stats_buffers(self, B, device):
        """(v, v2, norms) as views of the persistent send record of :meth:`global_label_stats`: the statistics kernel writes where
        the all-gather reads, nothing is packed."""
        mine = self._pbuf("ls_mine", (2 * B + 3,), torch.float32, device)
        return mine[:B], mine[B:2 * B], mine[2 * B:]

    def global_label_stats(self, v, v2, norms):
        """(v_all, v2_all, norms_global): all-gather the per-row view lengths, sum the 3 normalisers.  Returns the triple
        (single process) or a closure that waits for the asynchronous collective and returns it."""
        if not self.active:
            return v, v2, norms
        # ONE collective: [v | v2 | norms] of every rank (every rank holds the same B_local); the three normalisers are
        # summed locally from the gathered copies, in rank order on every rank (identical results everywhere)
        # The collective is ASYNCHRONOUS: the caller gets a closure and calls it right before the loss kernel, so the
        # all-gather (and the rank skew it absorbs) runs under the backbone forward instead of in front of it.
        B, n, dev, G = v.shape[0], 2 * v.shape[0] + 3, v.device, self.world
        mine = self._pbuf("ls_mine", (n,), v.dtype, dev)
        gathered = self._pbuf("ls_gathered", (G * n,), v.dtype, dev)
        v_all, v2_all = self._pbuf("ls_v", (G * B,), v.dtype, dev), self._pbuf("ls_v2", (G * B,), v.dtype, dev)
        norms_g = self._pbuf("ls_norms", (3,), norms.dtype, dev)
        state = {}

        def start():
            # (the statistics kernel normally wrote straight into `mine` -- label_stats_buffers; a caller's own tensors are copied
            # by the library's copy kernel: no torch kernel inside the data-parallel step)
            if v.data_ptr() != mine.data_ptr():
                cp = H.copy_bytes if mine.is_cuda else (lambda d_, s_: d_.copy_(s_))
                cp(mine[:B], v.contiguous())
                cp(mine[B:2 * B], v2.contiguous())
                cp(mine[2 * B:], norms.contiguous())
            if self.host_staged and mine.is_cuda:
                hg = torch.empty((G * n,), dtype=mine.dtype)
                self.dist.all_gather_into_tensor(hg, mine.cpu(), group=self.group)
                gathered.copy_(hg)
                state["work"] = None
            else:
                state["work"] = self.dist.all_gather_into_tensor(gathered, mine, group=self.group, async_op=True)

        def finish():
            work = state.pop("work", None)
            if work is not None:
                work.wait()          # stream-level wait on the communication stream, no host sync
            if gathered.is_cuda:
                H.label_stats_unpack(gathered, G, B, v_all, v2_all, norms_g)          # one launch: split + rank-ordered sum of the counts
            else:
                g = gathered.view(G, n)
                v_all.view(G, B).copy_(g[:, :B])
                v2_all.view(G, B).copy_(g[:, B:2 * B])
                torch.sum(g[:, 2 * B:], 0, out=norms_g)          # counts: exact in fp32 below 2^24
            return v_all, v2_all, norms_g
        H.host_action(start)
        return lambda: H.host_action(finish)

    def gather_rows(self, ids, rows):
        """Sparse exchange of id-table gradients: returns a CLOSURE that yields (ids of all ranks [G*B], rows of all ranks
        [G*B, w]) in rank order (every rank holds the same B, like :meth:`global_label_stats`).

        ONE asynchronous all-gather of ``[rows | id]`` per rank (the int64 id rides in two float lanes of its row) on a process
        group OF ITS OWN: on the gradient group it would queue behind every bucket all-reduce still in flight on that group's
        RCCL stream.  The caller issues it as soon as the compact rows exist and calls the closure right before the segment sum
        (engine._embed_bwd), so the collective and the rank skew it absorbs run under the rest of the embedding backward."""
        if not self.active:
            return lambda: (ids, rows)
        ids, rows = ids.contiguous(), rows.contiguous()
        if ids.dtype != torch.int64:
            ids = ids.to(torch.int64)
        B, w = rows.shape
        G, dev = self.world, rows.device
        seq = self.__dict__.get("_gr_seq", 0)          # (which exchange of the step: reset by Trainer at the head of the backward)
        self._gr_seq = seq + 1
        packed = self._pbuf(("gr_packed", seq), (B, w + 2), torch.float32, dev)
        gathered = self._pbuf(("gr_gathered", seq), (G * B, w + 2), torch.float32, dev)
        ids_all = self._pbuf(("gr_ids", seq), (G * B,), torch.int64, dev)
        rows_all = self._pbuf(("gr_rows", seq), (G * B, w), torch.float32, dev)
        state = {}

        def start():
            packed[:, :w].copy_(rows)
            packed[:, w:].copy_(ids.view(B, 1).view(torch.float32))          # bit pattern of the id, not a conversion
            if self.host_staged and rows.is_cuda:
                hg = torch.empty((G * B, w + 2), dtype=torch.float32)
                self.dist.all_gather_into_tensor(hg, packed.cpu(), group=self.group)
                gathered.copy_(hg)
                state["work"] = None
            else:
                state["work"] = self.dist.all_gather_into_tensor(gathered, packed, group=self._row_group(), async_op=True)

        def finish():
            work = state.pop("work", None)
            if work is not None:
                work.wait()          # stream-level wait on the row group's communication stream, no host sync
            ids_all.copy_(gathered[:, w:].contiguous().view(torch.int64).view(-1))
            rows_all.copy_(gathered[:, :w])
            return ids_all, rows_all
        H.host_action(start)
        return lambda: H.host_action(finish)

    def _row_group(self):
        """Process group of the row exchange (same ranks as the gradient group; created on first use, by every rank at the
        same point of its first data-parallel backward).  A one-rank forced group (tests) shares the gradient group."""
        g = self.__dict__.get("_rowg")
        if g is None:
            if self.world > 1:
                ranks = self.dist.get_process_group_ranks(self.group) if self.group is not None else list(range(self.dist.get_world_size()))
                g = self.dist.new_group(ranks=ranks, backend=self.dist.get_backend(self.group))
            else:
                g = self.group if self.group is not None else self.dist.group.WORLD
            self._rowg = g
        return g

    def gather_ints(self, t):
        """[G*B] int32: the values of every rank in rank order (validation: leave ranks of the global batch)."""
        if not self.active:
            return t
        t = t.contiguous()
        if self.host_staged and t.is_cuda:
            h = torch.empty((self.world * t.shape[0],), dtype=t.dtype)
            self.dist.all_gather_into_tensor(h, t.cpu(), group=self.group)
            return h.to(t.device)
        out = torch.empty((self.world * t.shape[0],), dtype=t.dtype, device=t.device)
        self.dist.all_gather_into_tensor(out, t, group=self.group)
        return out

    def reduce_bucket(self, flat_grad, start, end):
        """Asynchronous SUM all-reduce of one contiguous gradient bucket (gradients are already
        normalised by global counts, so SUM -- not mean -- reproduces the single-process gradient)."""
        if not self.active or end <= start:
            return
        w = self._all_reduce(flat_grad[start:end], async_op=True)
        if w is not None:
            self.pending.append(w)

    def take_pending(self):
        """The outstanding asynchronous all-reduces (issue order); the caller waits for them (``work.wait()`` is a
        stream-level wait on the communication stream, no host sync)."""
        p, self.pending = self.pending, []
        return p

    def finish(self):
        for w in self.take_pending():
            w.wait()

    def sum_scalar(self, t):
        if self.active:
            self._all_reduce(t)
        return t


def shard_rows(n_rows: int, world: int, rank: int):
    """Contiguous row block of ``rank``; the first ``n_rows % world`` ranks get one more."""
    base, rem = divmod(n_rows, world)
    start = rank * base + min(rank, rem)
    return start, start + base + (1 if rank < rem else 0)


def batch_rows(batch) -> int:
    """Row count of a batch dict: that of its labels, else of its first tensor."""
    t = batch.get("label")
    if not torch.is_tensor(t):
        t = next(v for v in batch.values() if torch.is_tensor(v) and v.dim())
    return int(t.shape[0])


def micro_slices(batch, m: int):
    """The micro-batches of ``batch`` for ``Trainer(micro_batch=m)``: ceil(B / m) dicts whose tensors are row slices -- VIEWS along
    dim 0, contiguous where the batch's are -- of the batch's tensors of B rows, in row order, the last one possibly shorter;
    everything else is passed along as it is."""
    B = batch_rows(batch)
    return [{k: (v[r0:r0 + m] if torch.is_tensor(v) and v.dim() and v.shape[0] == B else v) for k, v in batch.items()}
            for r0 in range(0, B, m)]


# ------------------------------------------------------------------------------------------------ trainer
class Trainer:
    """zero_grad -> L1-normalise -> forward -> backward (-> bucketed all-reduce) -> AdamW, i.e. the body of
    the reference's hot loop (main_for_seq_leave_earlystop_SegMM.py:269-300) minus its host syncs.
    Gradient clipping is a no-op in the reference (exhausted generator at :298), so the default ``max_grad_norm=None`` does not
    clip; ``max_grad_norm=m`` clips to global norm m on the device before AdamW (see FusedAdamW; ``trainer.opt.grad_norm`` is the
    norm the reference logs), in the eager, recorded and data-parallel steps."""


    def __init__(self, model, lr=1e-3, weight_decay=1e-4, comm: Optional[DPComm] = None, overlap=True, dropout=True,
                 feature_table=None, sparse_tables=True, device_state=False, max_grad_norm=None, lr_schedule=None, micro_batch=None,
                 param_groups=None, ema=None):
        self.model = model
        # micro_batch=m: a batch of more than m rows is stepped in ceil(B / m) micro-batches with ONE optimizer step on the whole
        # batch's gradient (train_step / _train_step_micro); None, or m >= the batch's rows: the plain step, launch for launch
        if micro_batch is not None and (isinstance(micro_batch, bool) or not isinstance(micro_batch, int) or micro_batch < 1):
            raise ValueError("micro_batch must be a positive int or None, not %r" % (micro_batch,))
        self.micro_batch = micro_batch
        self._micro_on = False
        if lr_schedule is not None and not device_state:
            raise ValueError("Trainer(lr_schedule=...) needs device_state=True: the rate of a step is evaluated in the device step state")
        # device_state: what changes from step to step (dropout seed words, AdamW's step count and bias corrections, the
        # site-header rows of a step) lives on the device / is laid out per step, so the kernel arguments of a step never
        # change and ``record()`` can note its launch sequence once for ``run_recorded()`` to replay from C.  The eager step in
        # this mode and the recorded step are bit-identical.
        self.device_state = bool(device_state)
        # with a device-resident feature table the batch carries INDEX lists ("photo_idx" [B, S],
        # "user_idx" [B, Lt], -1 = padding) instead of feature tensors; gather + pad + mask + L1 normalisation is one
        # HBM-bound kernel (segmm_gather_l1) and the 573 KB/row host->device copy disappears
        self.feature_table = feature_table
        self.dropout = dropout      # False: run the step in eval mode (deterministic; used by the DP equivalence tests)
        self.opt = FusedAdamW(model, lr=lr, weight_decay=weight_decay, max_grad_norm=max_grad_norm, lr_schedule=lr_schedule,
                              param_groups=param_groups, ema=ema)          # per-group rate scale, decay and freezing: see FusedAdamW
        # ema=None | decay | dict(decay=0.999, warmup=True): a device-side moving average of the weights (WeightEMA), or None
        self.ema = self.opt.ema
        self.comm = comm if comm is not None else DPComm()
        self.overlap = overlap
        st = model._store
        model._dp_hook = self.comm.global_label_stats if self.comm.active else None
        model._dp_stats_bufs = self.comm.label_stats_buffers if self.comm.active else None
        st.bucket_hook = self._on_bucket if self.comm.active else None
        # id mode under DP: the embedding tables' gradients travel as B rows per rank (DPComm.gather_rows) and their flat
        # ranges are cut out of the dense all-reduce; ``sparse_tables=False`` keeps the dense all-reduce (A/B, tests)
        sw = switches.read("trainer")
        self.sparse_tables = bool(sparse_tables) and self.comm.active and sw["sparse_tables"]
        st.row_exchange = self.comm.gather_rows if self.sparse_tables else None
        if self.sparse_tables:
            # dist.new_group is COLLECTIVE over the default group: create the row-exchange group here, where every rank
            # constructs its Trainer, not lazily inside the first backward (ranks that skip the id-table path on
            # their first step, or a DPComm on a sub-group, would deadlock)
            self.comm._row_group()
        self.per_bucket_adamw, self.table_two_pass, self.begin_overlap = sw["per_bucket_adamw"], sw["table_two_pass"], sw["begin_overlap"]
        self.bucket_bytes = int(sw["bucket_mb"] * (1 << 20))      # merge threshold of _on_bucket
        self.side_priority = sw["side_priority"]
        self._bucket_works = []
        self._pending_range = None
        self._norm = {}
        self._norm_amax = None
        self._norm_planes = {}
        self._slot = 0
        self._pf = None
        self._pf_stream = None
        self._norm_fresh = False
        if self.device_state:
            # the device step state (seed words, step count, bias corrections) is a small struct in memory THIS trainer owns
            # (segmm_step_bind names it for the launches that follow): several device_state trainers coexist in one process
            self._step_state = torch.zeros((H.step_state_bytes() + 3) // 4, dtype=torch.int32, device=next(model.parameters()).device)
            H.step_bind(self._step_state)
            self.opt._step_state = self._step_state
            self.opt.device_state = True
            seed0 = int(torch.randint(0, 2 ** 62, (1,)).item())          # torch.manual_seed -> reproducible runs
            if self.comm.rank:          # data-parallel ranks seed torch identically: every rank drops different elements of its rows
                seed0 = (seed0 ^ (self.comm.rank * 0x9E3779B97F4A7C15)) & (2 ** 62 - 1)
            H.step_set(seed0, self.opt.step_count, *self.opt.betas)
            self._seed0 = seed0          # (the host's copy: the seeds of the recorded validation passes are mixed from it)
            if self.opt.schedule is not None:
                self.opt._install_schedule()
            st.live_seed = H.LIVE_SEED | 0x5E6D0001          # the (constant) seed argument of every dropout launch

    def _on_bucket(self, name, after_side=False):
        if self._micro_on:          # a micro-batched step reduces the SUMMED gradient once, after its last pass (_train_step_micro)
            return
        # a host action of the step: a recorded step (record / run_recorded) calls it again at the same point of the launch order
        H.host_action(functools.partial(self._on_bucket_now, name, after_side))

    def _reset_buckets(self):
        self._bucket_works = []
        self._pending_range = None
        self.comm._gr_seq = 0

    def _wait_buckets(self, idxs):
        for i in idxs:
            for w in self._bucket_works[i][2]:
                w.wait()

    def _on_bucket_now(self, name, after_side=False):
        """Called from inside the backward the moment the gradients of bucket ``name`` are written (``after_side``: part of
        them by launches still in flight on the engine's side stream).  Adjacent buckets are MERGED until ``bucket_bytes`` of
        gradients are pending (a collective call costs ~0.2 ms of host time, whatever its size), then one asynchronous
        all-reduce is issued for the merged range; its works are remembered so that AdamW can step the range as soon as THEY
        are done (train_step, which also flushes what is still pending when the backward returns)."""
        st = self.model._store
        if not self.overlap:
            return
        for b, s, e in st.buckets:
            if b == name:
                p = self._pending_range
                if p is not None and p[1] != s and p[0] != e:
                    self._flush_bucket()          # not adjacent (two backbones interleave): send what is pending first
                    p = None
                self._pending_range = [s, e, after_side] if p is None else [min(p[0], s), max(p[1], e), p[2] or after_side]
                if 4 * (self._pending_range[1] - self._pending_range[0]) >= self.bucket_bytes:
                    self._flush_bucket()
                return

    def _flush_bucket(self):
        p, self._pending_range = self._pending_range, None
        if p is None:
            return
        st = self.model._store
        s, e, after_side = p
        if after_side and st.overlap and st._side_stream is not None:
            # order the collective behind main AND side stream without stalling the main stream: issue it from the side
            # stream's context after making the side stream wait for the main stream's work so far
            main, side = torch.cuda.current_stream(), st.side_stream()
            ev = torch.cuda.Event()
            ev.record(main)
            side.wait_event(ev)
            with torch.cuda.stream(side):
                self._reduce_dense(s, e)
        else:
            self._reduce_dense(s, e)
        self._bucket_works.append((s, e, self.comm.take_pending()))

    def _reduce_dense(self, s, e):
        """All-reduce [s, e) of the flat gradient minus the row-exchanged table ranges."""
        st = self.model._store
        if self.sparse_tables:
            for ts, te in st.table_ranges():
                if ts < e and te > s:
                    self.comm.reduce_bucket(st.gflat, s, max(s, ts))
                    s = min(e, te)
        self.comm.reduce_bucket(st.gflat, s, e)

    def _n_users(self):
        """reader.n_users as the reference's init_model sizes the user table (Embedding(n_users + 1, d)); None in image mode."""
        for bb in (self.model.backbone1, getattr(self.model, "backbone2", None)):
            if bb is not None and bb.id_usr:
                return bb.usr_proj.num_embeddings - 1
        return None

    def _input_act(self, key, buf, planes_only=False):
        """Site header (+ planes, + plane output for the producer kernel) of an input feature tensor the trainer itself
        produces this step (L1 normalisation or table gather).  The Act travels WITH the tensor object (attribute
        ``_segmm_act``), never keyed by its device address: a tensor the trainer did not produce in this step (rand_like for
        'noUser', features handed straight to model()) has none and gets an absmax pass in engine.BackboneRun._input_act."""
        st = self.model._store
        if not st.engine_h:
            return None
        dev = buf.device
        if not self._norm_fresh:
            self._norm_amax = st.hdr_rows(2)          # two clean site headers per step from the store's ring (no fill launch)
            self._norm_fresh = True
        cols = buf.shape[-1]
        rows = buf.numel() // cols
        planes = None
        if st.engine_p and cols % 32 == 0:
            pk = (key, self._slot)
            planes = self._norm_planes.get(pk)
            if planes is None or planes.shape != (rows, 2 * cols) or planes.device != dev:
                planes = self._norm_planes[pk] = torch.empty((rows, 2 * cols), dtype=torch.float16, device=dev)
        act = E.Act(buf, self._norm_amax[0 if key == "user" else 1], rows, cols, planes)
        if planes is not None:
            delayed = (self.model.training and st.scaling != "exact") or st.scaling == "always"
            act.scale_ptr = st.scale_ptr("in." + key, delayed)
            if act.scale_ptr is not None:
                if planes_only and st.input_planes_only and self._plane_consumers_only(key):
                    # L1-normalised rows: 1/cols <= max |y| <= 1.  With the FIXED scale 2^14 the planes can neither overflow nor
                    # fall below the fp16 window, whatever the batch: no fp32 copy is written and the consumers get none
                    act.scale_ptr = st.const_f32(16384.0).data_ptr()
                    act.no_f32 = True
                act.po = H.PO(planes, 2 * cols, act.hdr, act.scale_ptr)
        buf._segmm_act = act
        return act

    def _tables_early(self, batch):
        """Id mode, single process: the dense AdamW over the item table (config 3: 352 494 x 256 floats = 2.5 GB of optimizer
        traffic, 0.54 ms alone at the END of the step) is split in two -- the rows of this batch (the only ones with a gradient,
        known from the batch's ids) are stepped after the backward as before, every other row now, with g = 0, on an auxiliary
        stream under the forward and backward, which never touch those rows.  (Data parallel: the listed rows are those of ALL
        ranks, known only after the row exchange -- the dense update stays.)"""
        # a step that failed between this pass and opt.step() (forward / backward error, OOM) left its entry queued and its rows
        # flagged: drop both before queueing this step's, or the table's range would be stepped twice and the failed batch's rows
        # skipped
        stale = self.opt.__dict__.pop("_early", None)
        if stale:
            E.join_aux(self.model._store)
            for _, _, _, _, _, flags, _ in stale:
                flags.zero_()
            #  the failed step had already advanced the DEVICE step count (segmm_step_advance at its head) while
            # opt.step_count never moved, and THIS step has advanced it once more: put it back to step_count + 1, the number of the
            # step that is running, so its bias corrections are right again.  What cannot be taken back and is accepted: the failed step's early pass applied one g = 0 AdamW
            # update (weight decay + moment decay) to the table rows outside its batch.
            if self.device_state:
                H.step_bind(self._step_state)
                seed, _, _ = H.step_get()
                H.step_set(seed, self.opt.step_count + 1, *self.opt.betas)
        if self.comm.active or not self.table_two_pass or self._param_hooks():
            return
        model, st = self.model, self.model._store
        ids = batch.get("photo_identity_id")
        if ids is None or ids.dtype != torch.int64 or not ids.is_contiguous():
            return
        for pre, bb in (("backbone1.", model.backbone1), ("backbone2.", getattr(model, "backbone2", None))):
            if bb is None or not bb.id_vid:
                continue
            name = pre + "vid_proj.weight"
            if name not in st.index or name not in st.live_names or st._params[name].shape[1] % 4:
                continue
            if self.opt.ema is not None:          # the shadow is made and seeded on the main stream, before the early pass moves the table's rows
                self.opt.ema.step_head(self.opt._state())
            with E.aux_work(st):
                self.opt.table_early(name, ids.reshape(-1))

    def _plane_consumers_only(self, key) -> bool:
        """Every launch that reads the input features of ``key`` is a plane GEMM (forward projection and its weight gradient):
        the plane engine, a P32 plane entry for the projection weight and d_model a multiple of 32 (else the weight gradient
        takes the on-the-fly kernel, which reads the fp32 copy -- ADVICE r3: d_model = 48 raised on the second step)."""
        st = self.model._store
        if not st.engine_p:
            return False
        kind = "usr" if key == "user" else "vid"
        for pre, bb in (("backbone1.", self.model.backbone1), ("backbone2.", getattr(self.model, "backbone2", None))):
            if bb is None or (bb.id_usr if kind == "usr" else bb.id_vid):
                continue
            if bb.d_model % 32 or (pre + kind + "_proj.weight") not in st.wpt:
                return False
        return True

    def normalize(self, key, x):
        """a1: x / (sum|x| + 1e-6) over the feature dim, into a persistent float32 buffer.  ``x``: float32, or float16 / bfloat16 (half
        the bytes over the host link; hipabi.l1norm widens exactly) -- the single point where a batch's feature dtype enters the step."""
        bk = (key, self._slot)
        buf = self._norm.get(bk)
        if buf is None or buf.shape != x.shape or buf.device != x.device:
            buf = self._norm[bk] = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        act = self._input_act(key, buf, planes_only=True)
        # the GEMM that reads ``buf`` needs max|buf| (and, on the plane engine, its fp16 planes): both are folded into this
        # kernel instead of separate passes over the features.  Planes only (training steps after the first): ``buf`` is then
        # just the handle that carries the Act -- its fp32 contents are NOT written
        only = act is not None and act.no_f32
        H.l1norm(x, None if only else buf, amax=None if act is None else act.slots, po=None if act is None else act.po)
        if act is not None:
            E.produced(act)
        return buf

    def _features(self, batch):
        """(usr, usr_mask, vid, vid_mask): L1-normalised feature tensors of a batch, from the tensors it carries or --
        index batches -- gathered from the resident table.  Taken from :meth:`prefetch` when that ran for this very batch."""
        st = self.model._store
        pf, self._pf = self._pf, None
        if pf is not None and pf["batch"] is batch:
            st.ensure()
            torch.cuda.current_stream().wait_event(pf["done"])          # the main stream waits for the prefetch stream's kernels
            usr, um, vid, vm = pf["out"]
            self._norm_amax, self._norm_fresh = pf["amax"], pf["fresh"]
        elif self.begin_overlap and st.flat is not None and st.overlap:
            # The head of the step is a serial chain on one stream: weight maxima + split (32 us at config 2), user features,
            # video features, label statistics -- and the user-token chain, which bounds the forward up to the first attention
            # (the side stream's embedding GEMM -> LayerNorm -> projection), cannot fork before the last of them is enqueued.
            # Only the weight planes and the user features are in ITS way: the video features and the label statistics go to the
            # auxiliary stream (low priority), which the main stream joins before the model's forward.  The stage is HBM-bound
            # (0.6 GB), so what this buys is the small launches and their gaps, not the copies.
            it = self.model.input_type
            both = it["user"] != "id" and it["photo"] != "id"
            rows = st.hdr_rows(2) if st.engine_h else None          # taken (and, at a ring quarter, cleared) in main-stream order
            with E.aux_work(st):
                early = self._features_compute(batch, hdr_rows=rows, only="photo") if both else None
                gt = batch.get("label")
                # (a micro-batched step hands every pass the WHOLE batch's statistics: never those of the slice)
                if (not self._micro_on and self.model._dp_hook is None and gt is not None and gt.dtype == torch.int64 and gt.is_contiguous() and gt.dim() == 2
                        and getattr(self.model, "_loss_spec", None) is not None):
                    self.model._stats_pre = self.model._label_stats(gt, gt.shape[0], gt.shape[1])
            st.ensure()          # first ParamStore.ensure() of the step: the full check, the weight planes of this step
            usr, um, vid, vm = self._features_compute(batch, hdr_rows=None if both else rows, only="user" if both else None, flip=not both)
            if early is not None:
                vid, vm = early[2], early[3]
            E.join_aux(st)
        else:
            st.ensure()
            usr, um, vid, vm = self._features_compute(batch)
        if st.engine_p and self._norm_amax is not None and self._norm_fresh:
            st.update_scales(self._norm_amax, ["in.user", "in.photo"], 2)          # the input sites' scales of the next step
        return usr, um, vid, vm

    def _features_compute(self, batch, hdr_rows=None, only=None, flip=True):
        """``only``: one of the two inputs ("user" / "photo"; _features enqueues them on different streams); ``flip``: alternate
        the output buffer set (once per step)."""
        it = self.model.input_type
        usr = vid = None
        um, vm = batch.get("user_mask"), batch.get("photo_mask")
        if flip:
            self._slot ^= 1                      # two sets of output buffers, alternated: see prefetch()
            self._norm_fresh = False
        if hdr_rows is not None:
            self._norm_amax, self._norm_fresh = hdr_rows, True
        for key, kind in (("user", it["user"]), ("photo", it["photo"])):
            if kind == "id" or (only is not None and key != only):
                continue
            if key + "_idx" in batch:
                out, mask = self.feature_table.buffers(key, batch[key + "_idx"], self._slot)
                act = self._input_act(key, out)
                self.feature_table.gather(key, batch[key + "_idx"], amax=None if act is None else act.slots,
                                          po=None if act is None else act.po, slot=self._slot)
                if act is not None:
                    E.produced(act)
                x, m = out, mask.view(torch.bool)
            else:
                x, m = self.normalize(key, batch[key]), (um if key == "user" else vm)
            if key == "user":
                usr, um = x, m
            else:
                vid, vm = x, m
        return usr, um, vid, vm

    def prefetch(self, batch):
        """Enqueue the input stage of ``batch`` (a1: L1 normalisation, or the table gather of an index batch; with the fp16 planes
        and maxima the first GEMM needs) on a low-priority stream of its own, NOW -- typically while the current step's backward
        is running.  The next ``train_step(batch)`` with this very dict picks the results up instead of running the stage at the
        head of its critical path (the reference overlaps the same work through its DataLoader workers).  Output buffers
        alternate between two sets, so the step in flight keeps reading its own."""
        st = self.model._store
        it = self.model.input_type
        if st.flat is None or (it["user"] == "id" and it["photo"] == "id"):
            return
        main = torch.cuda.current_stream()
        if self._pf_stream is None:          # lowest priority, like the engine's side stream: it must not starve the step in flight
            self._pf_stream = torch.cuda.Stream(device=st.flat.device, priority=self.side_priority)
        rows = st.hdr_rows(2) if st.engine_h else None          # taken (and, at a ring quarter, cleared) in main-stream order
        ev = torch.cuda.Event()
        ev.record(main)                                            # behind this step's scales_update of the input sites
        self._pf_stream.wait_event(ev)
        with torch.cuda.stream(self._pf_stream):
            out = self._features_compute(batch, hdr_rows=rows)
            done = torch.cuda.Event()
            done.record(self._pf_stream)
        self._pf = dict(batch=batch, out=out, done=done, amax=self._norm_amax, fresh=self._norm_fresh)

    def train_step(self, batch: Dict[str, torch.Tensor], next_batch: Optional[Dict[str, torch.Tensor]] = None):
        """One optimisation step on ``batch``.  ``next_batch``: the batch of the FOLLOWING step, if known -- its input stage is
        enqueued on a side stream right away (:meth:`prefetch`) and overlaps this step's backward.
        ``Trainer(micro_batch=m)`` and a batch of more than m rows: the step runs in micro-batches (:meth:`_train_step_micro`; nothing
        is prefetched then)."""
        if self.ema is not None:
            self.ema._refuse_applied("train_step()")
        if self.micro_batch is not None and batch_rows(batch) > self.micro_batch:
            return self._train_step_micro(batch, self.micro_batch)
        model, st = self.model, self.model._store
        if self.device_state:
            H.step_bind(self._step_state)          # (a host-side pointer: the launches below carry it in their arguments)
        if model.training != bool(self.dropout):
            model.train(self.dropout)          # (walks every sub-module: 0.35 ms of host time when done every step)
        self.opt.zero_grad()
        H.mark(H.PHASE_STEP_BEGIN)
        if self.device_state:          # first launches of the step: advance the device-side step state, fresh header rows
            H.step_advance(*self.opt.betas)
            st.hdr_step_begin()
        st._trusted = False
        try:
            usr, um, vid, vm = self._features(batch)          # first ParamStore.ensure() of the step: the full check
            st._trusted = True
            self._tables_early(batch)
            # (a next batch the micro-batched step will take in slices gets no prefetch: that step could not use a whole-batch input
            # stage, whose buffers would be those of all its rows)
            if next_batch is not None and not (self.micro_batch is not None and batch_rows(next_batch) > self.micro_batch):
                self.prefetch(next_batch)
            out = self._train_step(batch, usr, um, vid, vm)
            r = self.__dict__.get("_recorded")
            if r is not None and H.RECORDER is None:
                r["prev_batch"] = batch          # a recorded step that follows names this step's batch as "the previous one"
            return out
        finally:
            st._trusted = False
            model.__dict__.pop("_stats_pre", None)          # (a step that failed before its forward must not leave this batch's statistics behind)
            if self.device_state:
                st.hdr_step_end()          # evaluation passes between steps draw their headers from the wrapping ring

    # ---- one optimizer step over a batch taken in micro-batches (Trainer(micro_batch=m))
    def _micro_ranges(self, st):
        """[start, end) pieces of the live range OUTSIDE the id tables: what the flat gradient sum covers (the dense table
        gradients accumulate in place -- segmm_embed_id_bwd adds -- and never go through it)."""
        key = (st.flat.data_ptr(), st.n_live)
        c = self.__dict__.get("_micro_rng")
        if c is None or c[0] != key:
            out, pos = [], 0
            for ts, te in st.table_ranges():
                if ts > pos:
                    out.append((pos, min(ts, st.n_live)))
                pos = max(pos, te)
            if pos < st.n_live:
                out.append((pos, st.n_live))
            c = self._micro_rng = (key, out)
        return c[1]

    def _micro_accumulate(self, st, j, k):
        """After pass j of k, both streams joined: acc <- g (pass 0), acc <- acc + g (the middle passes), g <- acc + g (the last):
        the flat gradient buffer ends up holding the batch's gradient, summed in pass order -- the same bits every run."""
        acc = self.__dict__.get("_micro_acc")
        if acc is None or acc.numel() != st.n_live or acc.device != st.gflat.device:
            acc = self._micro_acc = torch.empty(st.n_live, dtype=torch.float32, device=st.gflat.device)
        g = st.gflat
        for s, e in self._micro_ranges(st):
            if j == 0:
                H.copy_bytes(acc[s:e], g[s:e])
            elif j < k - 1:
                H.vec_add(acc, acc, g, e - s, s, s, s)
            else:
                H.vec_add(g, acc, g, e - s, s, s, s)

    def _micro_reduce(self):
        """Data parallel: ONE all-reduce of the dense live ranges of the summed gradient, waited for (a host action of the step)."""
        self._reduce_dense(0, self.model._store.n_live)
        self.comm.finish()

    def _train_step_micro(self, batch, m):
        """One optimizer step on ``batch`` (B > m rows) in k = ceil(B / m) micro-batches, row slices of the batch's own tensors.
        The head of the step runs once (step state, header arena, the tables' first AdamW pass and the label statistics of the WHOLE
        batch); every pass gets those statistics, so its loss terms and gradients are already divided by the batch's normalisers and
        simply sum: the flat gradient outside the id tables through segmm_vec_add, the id tables in place.  Then one tail: (data
        parallel: one all-reduce of the sum,) norm / clip and AdamW on the whole batch's gradient.  Activation memory is that of m
        rows.  Dropout differs between the passes of a step (engine.live_seed).  Every pass draws its site headers from the step's
        arena: with the device step state k x the headers of a pass must fit ParamStore.HDR_RING_ROWS = 8192, a larger k is refused.
        Parameter hooks are refused: the gradients must stay in the flat buffer."""
        model, st = self.model, self.model._store
        if self._param_hooks():
            raise RuntimeError("Trainer(micro_batch=%d) does not support parameter hooks: the micro-batches' gradients are summed in "
                               "the flat gradient buffer, where autograd's hooks never see them" % m)
        for key, v in batch.items():
            if torch.is_tensor(v) and not v.is_contiguous():
                raise RuntimeError("train_step(micro_batch=%d): batch[%r] is not contiguous" % (m, key))
        slices = micro_slices(batch, m)
        k = len(slices)
        if self.device_state:
            H.step_bind(self._step_state)
        if model.training != bool(self.dropout):
            model.train(self.dropout)
        self.opt.zero_grad()
        H.mark(H.PHASE_STEP_BEGIN)
        if self.device_state:          # ONE count and one rate per optimizer step
            H.step_advance(*self.opt.betas)
            st.hdr_step_begin()
        st._trusted = False
        self._micro_on = True
        try:
            st.ensure()          # the full check and the weight planes of this step, once
            st._trusted = True
            if model._loss_spec is None:
                model._loss_spec = LossSpec(model.model_cfg)
            gt = E._as(batch["label"], torch.int64, "the labels")
            stats = model._label_stats(gt, gt.shape[0], gt.shape[1])          # of the whole batch (data parallel: all-gathered, once)
            if callable(stats):
                stats = stats()
            ids = {}
            for side, key in (("vid", "photo_identity_id"), ("usr", "user_identity_id")):
                t = batch.get(key)
                if torch.is_tensor(t) and t.dtype == torch.int64 and not (side == "usr" and "noUser" in getattr(model.backbone1, "ablation_type", "ours")):
                    ids[side] = t
            dev = st.flat.device
            sums = torch.empty(13, dtype=torch.float32, device=dev)          # the 12 loss slots, then the total
            logits = None
            hdr0 = st._arena_off if self.device_state else 0
            for j, mb in enumerate(slices):
                st.micro_pass = (j, ids)
                model._stats_pre = stats
                if j:
                    self.opt.zero_grad()          # (host only: the pass writes the flat buffer again and re-delivers the views)
                usr, um, vid, vm = self._features(mb)
                if j == 0:
                    self._tables_early(batch)          # the rows of the WHOLE batch are the ones left for the second pass
                out = self._fwd_bwd(mb, usr, um, vid, vm)
                if j == 0 and self.device_state:
                    per = st._arena_off - hdr0
                    if st._arena_off + (k - 1) * per > st.HDR_RING_ROWS:
                        raise RuntimeError("Trainer(micro_batch=%d): %d micro-batches of %d site headers each do not fit the step's header "
                                           "arena of %d rows; use a micro_batch of at least %d for this batch"
                                           % (m, k, per, st.HDR_RING_ROWS, -(-batch_rows(batch) // max((st.HDR_RING_ROWS - hdr0) // max(per, 1), 1))))
                self._micro_accumulate(st, j, k)
                lv, lg = model._losses_vec, out["logits"]
                if logits is None:
                    logits = torch.empty((gt.shape[0],) + tuple(lg.shape[1:]), dtype=lg.dtype, device=dev)
                    H.copy_bytes(sums[:12], lv)
                    H.copy_bytes(sums[12:], out["loss"].detach().view(1))
                else:
                    H.vec_add(sums, sums, lv, 12)
                    H.vec_add(sums, sums, out["loss"].detach().view(1), 1, 12, 12, 0)
                H.copy_bytes(logits[j * m:j * m + lg.shape[0]], lg)
                keys = list(out)
                del out
            if self.comm.active:
                H.host_action(self._micro_reduce)
            H.mark(H.PHASE_STEP_TAIL)
            if self.opt.__dict__.get("_early"):
                E.join_aux(st)          # the tables' first pass (aux stream) is complete before their listed rows are stepped
            self.opt.step()
            res = {}
            for key in keys:
                res[key] = logits if key == "logits" else batch["label"] if key == "gt" else sums[12] if key == "loss" else sums[_LIDX[key]]
            r = self.__dict__.get("_recorded")
            if r is not None and H.RECORDER is None:
                r["prev_batch"] = batch
            return res
        except BaseException:
            if self.device_state and self.opt.__dict__.get("_early") is None:
                # the step failed after the device step count had advanced: put it back, with its bias corrections and rate (a
                # queued table pass is undone, with the count, by the next step's _tables_early).  The seed words keep the failed
                # step's advance: the steps that follow draw another dropout stream of the same distribution
                try:
                    seed, _, _ = H.step_get()
                    H.step_set(seed, self.opt.step_count, *self.opt.betas)
                except RuntimeError:          # (the device itself failed: the first error is the one to report)
                    pass
            raise
        finally:
            self._micro_on = False
            st._trusted = False
            st.__dict__.pop("micro_pass", None)
            model.__dict__.pop("_stats_pre", None)
            if self.device_state:
                st.hdr_step_end()

    def _train_step(self, batch, usr, um, vid, vm):
        return self._finish_step(self._fwd_bwd(batch, usr, um, vid, vm))

    def _fwd_bwd(self, batch, usr, um, vid, vm):
        """Forward and backward of one pass: the whole batch of a plain step, one micro-batch of a micro-batched one."""
        model, st = self.model, self.model._store
        usr_id = batch["user_identity_id"]
        if "noUser" in getattr(model.backbone1, "ablation_type", "ours"):
            # 'noUser' / 'noUser_SelfAtt' (main...SegMM.py:275-280, main...KuaiRand.py:254-258): the TRAINING forward sees
            # uniform-random user features and random user ids in [1, n_users); validation keeps the real ones
            live = E.live_seed(st)
            n_users = self._n_users()
            if live is not None:
                # device-side step state (the step may be recorded): the draws come from the library's counter hash, into persistent
                # buffers -- the reference's distributions (U[0, 1) features, uniform ids), not torch's bit stream
                if usr is not None:
                    buf = self.__dict__.get("_nouser_feat")
                    if buf is None or buf.shape != usr.shape or buf.device != usr.device:
                        buf = self._nouser_feat = torch.empty_like(usr)
                    H.rand_uniform(buf, live, E.SITE_NOUSER_FEAT)
                    usr = buf
                if n_users is not None:
                    ib = self.__dict__.get("_nouser_ids")
                    if ib is None or ib.shape != usr_id.shape or ib.device != usr_id.device:
                        ib = self._nouser_ids = torch.empty_like(usr_id, dtype=torch.int64)
                    H.rand_ids(ib, 1, max(n_users, 2), live, E.SITE_NOUSER_IDS)
                    usr_id = ib
            else:
                if usr is not None:
                    usr = torch.rand_like(usr)
                if n_users is not None:
                    usr_id = torch.randint(1, max(n_users, 2), usr_id.shape, device=usr_id.device)
        out = model(usr_image=usr, usr_id=usr_id, usr_mask=um, vid_image=vid,
                    vid_id=batch["photo_identity_id"], vid_mask=vm, gt=batch["label"], mode="train")
        if self.comm.active:
            H.host_action(self._reset_buckets)          # (a host action of the recorded data-parallel step)
        else:
            self._reset_buckets()
        # seed the backward with the model's own constant-one tensor: the head recognises it (same storage) and skips both the
        # ones_like fill autograd would launch and the dlogits * 1 multiply
        if self._param_hooks():
            # tensor / post-accumulate-grad hooks on parameters (gradient scaling, clipping, DDP-style wrappers) only fire when
            # the gradients travel through autograd: take the plain path (engine.grads_out), FusedAdamW copies the results in
            if self.comm.active:
                raise RuntimeError("parameter hooks under data parallelism are not supported: the bucket all-reduces are "
                                   "issued from inside the backward, before autograd would run the hooks")
            out["loss"].backward()
        else:
            torch.autograd.backward(out["loss"], grad_tensors=[model.unit_grad(out["loss"].device)])
        return out

    def _finish_step(self, out):
        """The tail of the plain step: the data-parallel reductions still outstanding, then AdamW."""
        st = self.model._store
        if self.comm.active and self.overlap:
            H.host_action(self._flush_bucket)          # the tail of the backward (embedding gradients) that stayed below the merge threshold
        if self.comm.active and self.overlap and self.per_bucket_adamw and self._covers_live(st):
            # AdamW per bucket, in completion order: each launch waits (stream-level) only for its own bucket's all-reduce, so
            # the optimizer of the early buckets runs under the collectives of the late ones and only the last, small bucket
            # (the video-side embedding) is exposed
            # ... in TWO launches: every cross-stream wait costs ~15 us of queue time on the GPU, so the buckets that
            # completed early (a contiguous prefix of the flat buffer: head | layers ...) are stepped together, then the last one
            H.mark(H.PHASE_STEP_TAIL)
            works = self._bucket_works
            if self.opt.max_grad_norm is not None:
                # a global norm needs every bucket reduced: no per-bucket overlap, one norm over the reduced live range (each rank
                # computes it from its own, identical copy of the all-reduced gradient), then one AdamW launch
                H.host_action(functools.partial(self._wait_buckets, range(len(works))))
                self.opt.begin_step()
                self.opt.step_range(0, st.n_live)
                self.opt.end_step()
                return out
            self.opt.begin_step()
            order = sorted(range(len(works)), key=lambda i: works[i][0])
            last = len(works) - 1
            early = [i for i in order if i != last]
            if early and works[early[-1]][1] <= works[last][0] and all(works[a][1] == works[b][0] for a, b in zip(early, early[1:])):
                H.host_action(functools.partial(self._wait_buckets, early))
                self.opt.step_range(works[early[0]][0], works[early[-1]][1])
                H.host_action(functools.partial(self._wait_buckets, [last]))
                self.opt.step_range(works[last][0], works[last][1])
            else:          # not a prefix + tail (two backbones interleave their buckets): one launch per bucket
                for i in range(len(works)):
                    H.host_action(functools.partial(self._wait_buckets, [i]))
                    self.opt.step_range(works[i][0], works[i][1])
            self.opt.end_step()
            return out
        if self.comm.active:
            if H.RECORDER is not None:
                raise RuntimeError("record(): the data-parallel step is recorded in its default schedule only (overlapped bucket "
                                   "all-reduces, per-bucket AdamW)")
            if not self.overlap:
                self._reduce_dense(0, st.n_live)
            for _, _, works in self._bucket_works:
                for w in works:
                    w.wait()
            self.comm.finish()
        H.mark(H.PHASE_STEP_TAIL)
        if self.opt.__dict__.get("_early"):
            E.join_aux(st)          # the tables' first pass (aux stream) is complete before their listed rows are stepped
        self.opt.step()
        return out

    # ---- the step as recorded launch sequences replayed from C (include/segmm_hip.h "Recorded launch sequences")
    def record(self, batch: Dict[str, torch.Tensor], warmup: int = 3, prev_batch: Optional[Dict[str, torch.Tensor]] = None):
        """Record the launch sequence of one training step on ``batch``'s shapes: ``warmup`` eager steps (site scales calibrated,
        every persistent buffer allocated, both streams created), then ONE more eager step during which every C-ABI call is
        recorded -- entry point, arguments, stream slot, fork / join points of the two streams -- split into the phases of the
        step (step begin, embedding, each encoder layer, head + loss, their backwards, optimizer tail).  The step's allocations
        come from a private memory pool kept for the life of the recording, the per-step state lives on the device
        (``device_state``): the recorded arguments are valid for every later step, except the batch's own tensors, whose
        addresses are patched per step.  ``run_recorded(batch)`` then enqueues a step with one C call per phase
        (segmm_step_begin, segmm_embed_fwd, segmm_layer_fwd, ...): the eager two-stream schedule without the per-launch host
        work.  Results are bit-identical to ``train_step`` in the same mode.
        ``prev_batch``: the batch of the ``train_step`` that ran immediately before (same shapes, other tensors).  With it NO
        warm-up step runs -- the caller has already stepped (the sites are calibrated) -- so the only optimisation step ``record``
        takes is the recorded one, on ``batch``: what an epoch loop needs (:func:`fit` with ``recorded=True``)."""
        if not self.device_state:
            raise RuntimeError("record() needs Trainer(device_state=True): the per-step state must live on the device")
        if self.ema is not None:
            self.ema._refuse_applied("record()")
        model, st = self.model, self.model._store
        if self._param_hooks():
            raise RuntimeError("record(): parameter hooks only fire when the gradients travel through autograd; use train_step")
        self._refuse_unrecordable(batch, "record()", "step")
        # the step may name tensors of the PREVIOUS step's batch (id mode: the rows the last backward scattered into the table
        # gradient are cleared by id list): the last warm-up step runs on a copy of the batch, so that such pointers can be told
        # from the current batch's and re-based to the previous batch at replay
        if prev_batch is not None:
            for k, v in batch.items():
                if torch.is_tensor(v):
                    pv = prev_batch.get(k)
                    if not torch.is_tensor(pv) or pv.shape != v.shape or pv.dtype != v.dtype or (v.numel() and pv.data_ptr() == v.data_ptr()):
                        raise RuntimeError("record(prev_batch=...): prev_batch[%r] must be another tensor of the same shape and dtype" % k)
            prev = prev_batch
        else:
            prev = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()}
            for _ in range(max(warmup - 1, 0)):
                self.train_step(batch)
            self.train_step(prev)
        torch.cuda.synchronize()
        main = H._stream()
        side = st.side_stream().cuda_stream
        pool = torch.cuda.MemPool()
        aux = st.__dict__.get("_aux_stream")
        rec = H.Recorder(main, side, aux.cuda_stream if aux is not None else 0)
        H.RECORDER = rec
        # The recorded step must carry the per-step weight split (segmm_wsplit_p32): ParamStore.refresh_planes skips it when the planes
        # are current -- which they are when an EVALUATION pass ran since the last optimizer step (it split the new weights itself).
        # A step recorded in that state would replay on stale weight planes for ever (found by fit(recorded=True): validation, then
        # record).  Force the split into the recording.
        st._planes_key = None
        try:
            with st.rec_pool(pool):
                out = self.train_step(batch)
        finally:
            H.RECORDER = None
        torch.cuda.synchronize()
        phases = rec.finish()
        # the batch's tensors: every recorded pointer that falls inside one of them is re-based per step
        spans = [(k, v.data_ptr(), v.numel() * v.element_size(), tuple(v.shape), v.dtype) for k, v in batch.items() if torch.is_tensor(v) and v.numel()]
        pspans = [(k, v.data_ptr(), v.numel() * v.element_size()) for k, v in prev.items() if torch.is_tensor(v) and v.numel()]
        relocs = []
        for pi, (ph, arr) in enumerate(phases):
            if arr is None:
                continue
            # only the slots recorded as POINTER arguments (Recorder.pslots): an integer / float slot -- a seed, a byte count, the
            # bit pattern of lr -- that happens to fall inside a batch tensor's address range must never be rewritten
            for ci, ai in rec.pslots[pi]:
                pv = arr[ci].a[ai].p
                for k, base, nb, _, _ in spans:
                    if base <= pv < base + nb:
                        relocs.append((arr, ci, ai, k, pv - base, 0))
                        break
                else:
                    for k, base, nb in pspans:
                        if base <= pv < base + nb:
                            relocs.append((arr, ci, ai, k, pv - base, 1))
                            break
        # host-side state of the eager path that names a batch tensor (id mode: the id list whose table-gradient rows the NEXT
        # backward clears): kept current by run_recorded, so that eager steps and recorded steps can be mixed
        tab_keys = []
        for ek, (gptr, t) in getattr(st, "_tab_rows", {}).items():
            for k, base, nb, _, _ in spans:
                if base <= t.data_ptr() < base + nb and t.data_ptr() == base and t.numel() * t.element_size() == nb:
                    tab_keys.append((ek, gptr, k))
        evs = tuple(torch.cuda.Event() for _ in range(4))
        for e in evs:
            e.record()
        streams = [main, side] + ([aux.cuda_stream] if aux is not None else [])
        self._recorded = dict(phases=phases, keep=rec.keep, pool=pool, prev_batch=batch, tab_keys=tab_keys, out=out, relocs=relocs, spans={k: (sh, dt) for k, _, _, sh, dt in spans},
                              main=main, events=evs, table=H.stream_table(streams, [e.cuda_event for e in evs[:2 * (len(streams) - 1)]]),
                              n_cmds=sum(ph.n_cmds for ph, a in phases if a is not None),
                              hyper=self._hyper())
        return out

    @staticmethod
    def _refuse_unrecordable(batch, who, what):
        """What a replay would drop, refused by name (``who``: the caller in the message; ``what``: "step" / "validation batch")."""
        for k, v in batch.items():
            if torch.is_tensor(v) and not v.is_contiguous():
                raise RuntimeError("%s: batch[%r] is not contiguous" % (who, k))
            # the zero-copy paths of the step: anything else is converted by a torch kernel, which a replay would drop (the
            # conversions also raise by themselves while recording: hipabi.torch_fallback)
            # (16-bit features: only the two tensors that go through normalize(); the recorded commands carry their element size, and
            # run_recorded() refuses a batch of another dtype)
            if torch.is_tensor(v) and v.is_floating_point() and v.dtype != torch.float32 and not (
                    k in ("user", "photo") and v.dtype in (torch.float16, torch.bfloat16)):
                raise RuntimeError("%s: batch[%r] is %s; the recorded %s takes float32 features (batch['user'] / batch['photo']: "
                                   "float32, float16 or bfloat16)" % (who, k, v.dtype, what))
            if torch.is_tensor(v) and k.endswith("_mask") and v.dtype != torch.bool:
                raise RuntimeError("%s: batch[%r] is %s; the recorded %s takes bool masks" % (who, k, v.dtype, what))
            if torch.is_tensor(v) and not v.is_floating_point() and v.dtype not in (torch.bool, torch.int64):
                raise RuntimeError("%s: batch[%r] is %s; the recorded %s takes int64 ids and labels" % (who, k, v.dtype, what))
        # one feature dtype per recorded batch: a batch that carries 16-bit features carries both tensors so (a pipeline stores its
        # features in one format); a half-precision tensor next to a float32 one is the stray conversion record() has always refused
        fdt = {k: batch[k].dtype for k in ("user", "photo") if torch.is_tensor(batch.get(k)) and batch[k].is_floating_point()}
        if len(set(fdt.values())) > 1:
            raise RuntimeError("%s: batch['user'] is %s and batch['photo'] is %s; the recorded %s takes both feature tensors in "
                               "one dtype (float32, float16 or bfloat16)" % (who, fdt["user"], fdt["photo"], what))

    def _hyper(self):
        # under an lr_schedule the recorded commands carry the sentinel, not a rate: the rate may move, the schedule's presence not
        lr = self.opt.lr if self.opt.schedule is None else H.LIVE_LR
        # (the recorded segmm_ema_update carries the EMA's weight and warm-up flag by value)
        return (lr, self.opt.wd, tuple(self.opt.betas), self.opt.eps, self.opt.max_grad_norm, self.opt.group_table(),
                None if self.ema is None else self.ema.hyper())

    def _timed_plan(self, r):
        """The recorded phases cut at every GEMM / attention command (bench.py's timed replay): [("host", fn) | ("run", Phase) |
        ("timed", Phase of ONE command, stream slot, record)], record = the tuple hipabi's GEMM_PROFILE / ATTN_PROFILE entries
        start with.  The sub-phases alias the recorded command arrays (the per-step re-basing of batch pointers reaches them)."""
        plan = r.get("timed_plan")
        if plan is not None:
            return plan
        names = {v: k for k, v in H.op_ids().items()}
        plan = []
        for ph, arr in r["phases"]:
            if arr is None:
                plan.append(("host", ph))
                continue
            def sub(lo, hi, ph=ph, arr=arr):
                return H.Phase(kind=ph.kind, backbone=ph.backbone, layer=ph.layer, n_cmds=hi - lo,
                               cmds=ctypes.cast(ctypes.byref(arr, lo * ctypes.sizeof(H.Cmd)), ctypes.POINTER(H.Cmd)))
            lo = 0
            for ci in range(ph.n_cmds):
                c = arr[ci]
                nm = names.get(c.op)
                def args(*params, c=c, nm=nm):          # the command's arguments, by the header's parameter names
                    return [H.cmd_arg(c, nm, p) for p in params]
                rec = None
                if nm in ("segmm_gemm", "segmm_gemm_h"):
                    rec = ("gemm", H.gemm_record(*args("layout", "M", "N", "K")))
                elif nm == "segmm_gemm_p":
                    rec = ("gemm", H.gemm_record(*args("layout", "M", "N", "K", "write_c")))
                elif nm == "segmm_attn_fwd":
                    rec = ("attn", H.attn_record(*args("B", "H", "dh", "Lq", "La", "Lb")))
                elif nm == "segmm_attn_bwd":
                    planes, = args("planes")
                    rec = ("attn", H.attn_record(*args("B", "H", "dh", "Lq", "La", "Lb", "phase"), H.AttnPlanes.from_address(planes) if planes else None))
                if rec is None or rec[1] is None:          # (gemm_record: a repair launch is not timed)
                    continue
                if ci > lo:
                    plan.append(("run", sub(lo, ci)))
                plan.append(("timed", sub(ci, ci + 1), c.stream, rec))
                lo = ci + 1
            if ph.n_cmds > lo:
                plan.append(("run", sub(lo, ph.n_cmds)))
        r["timed_plan"] = plan
        return plan

    def run_recorded(self, batch: Dict[str, torch.Tensor], timed=None):
        """One training step from the recorded launch sequences (see :meth:`record`): patch the batch's addresses, then one C
        call per phase.  Must be called with torch's current stream = the stream ``record`` ran on.
        ``timed`` = (gemm list, attention list): the same launch sequence with the phases cut at every GEMM / attention command and
        a HIP-event pair around each on the command's own stream -- entries like hipabi.GEMM_PROFILE / ATTN_PROFILE; bench.py's
        roofline pass (a few more C calls and event records per step; results identical)."""
        r = self.__dict__.get("_recorded")
        if r is None:
            raise RuntimeError("run_recorded() before record()")
        if self.ema is not None:
            self.ema._refuse_applied("run_recorded()")
        H.step_bind(self._step_state)
        if self._hyper() != r["hyper"]:
            # the recorded segmm_adamw / segmm_adamw_table / segmm_grad_norm commands carry lr (without an lr_schedule), weight
            # decay, betas, eps and the clipping norm BY VALUE
            raise RuntimeError("run_recorded(): the optimizer's hyperparameters changed since record() (%r -> %r): record() again"
                               % (r["hyper"], self._hyper()))
        for k, (sh, dt) in r["spans"].items():
            v = batch[k]
            if tuple(v.shape) != sh or v.dtype != dt or not v.is_contiguous():
                raise RuntimeError("run_recorded(): batch[%r] is %s %s, the step was recorded for %s %s" % (k, tuple(v.shape), v.dtype, sh, dt))
        pb = r["prev_batch"]
        for arr, ci, ai, k, off, lag in r["relocs"]:
            arr[ci].a[ai].p = (pb if lag else batch)[k].data_ptr() + off
        r["prev_batch"] = batch          # (also keeps the tensors a lag-1 pointer names alive until the next step has run)
        main, table = r["main"], r["table"]
        if H._stream() != main:
            raise RuntimeError("run_recorded(): the current stream is not the stream the step was recorded on")
        if timed is not None:
            streams = r.get("timed_streams")
            if streams is None:
                streams = r["timed_streams"] = [torch.cuda.current_stream()] + [torch.cuda.ExternalStream(int(h)) for h in list(table[0])[1:]]
            for item in self._timed_plan(r):
                if item[0] == "host":
                    item[1]()
                elif item[0] == "run":
                    H.run_phase(item[1], table)
                else:
                    _, ph1, slot, (fam, head) = item
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(streams[slot])
                    H.run_phase(ph1, table)
                    e1.record(streams[slot])
                    timed[0 if fam == "gemm" else 1].append(head + (e0, e1))
        for ph, arr in (r["phases"] if timed is None else ()):
            if arr is None:
                ph()          # a host action of the step (data-parallel collective / wait), at its place in the launch order
            else:
                H.run_phase(ph, table)
        # mirror the host side effects of the eager step (FusedAdamW.begin_step / end_step; the id list of the table rows this
        # step's backward scattered into)
        self.opt.step_count += 1
        st = self.model._store
        st.fused_version += 1
        for ek, gptr, k in r["tab_keys"]:
            st._tab_rows[ek] = (gptr, batch[k].reshape(-1))
        return r["out"]

    def _param_hooks(self) -> bool:
        plist = self.__dict__.get("_hook_plist")
        if plist is None:
            plist = self._hook_plist = list(self.model.parameters())
        for p in plist:
            if p._backward_hooks or getattr(p, "_post_accumulate_grad_hooks", None):
                return True
        return False

    def _covers_live(self, st):
        """The buckets whose hooks fired tile [0, n_live) exactly (always, for a backward over the whole model)."""
        spans = sorted((s, e) for s, e, _ in self._bucket_works)
        pos = 0
        for s, e in spans:
            if s != pos:
                return False
            pos = e
        return pos == st.n_live

    def _ema_scope(self, ema, who):
        """The context an evaluation entry point runs in: ``ema.applied()`` for ``ema=True`` (refused by name without an EMA)."""
        if not ema:
            return contextlib.nullcontext()
        if self.ema is None:
            raise ValueError("%s(ema=True) needs Trainer(ema=...): this trainer keeps no weight average" % who)
        return self.ema.applied()

    @torch.no_grad()
    def test_model(self, test_batches, eval_type_list, ckpt: Optional["CheckPointer"] = None, threshold: float = 0.5, top_k_mask: int = 0,
                   top_k_permutation: int = 1, save_logits: bool = False, train_videos: Optional[set] = None, draw_case: int = 0,
                   device_metrics: bool = False, ema: bool = False):
        """The test phase of the reference trainer (main_for_seq_leave_earlystop_SegMM.py:365-459): reload the BEST checkpoint
        (``ckpt.load_checkpoint(model, optimizer, mode='best')``, :366-367), eval mode, ``mode="inference"`` over the test split,
        interests = sigmoid(logits) * exposure_prob (:402-403), pred_label = interests > threshold (:404), every batch through
        ``main_eval_batch`` (:415), then ``compute_final_result`` (:434).  ``train_videos`` (the reference's ``--eval_cold``
        set of photo ids seen in training, :417-427): also the cold / hot splits.  ``save_logits`` (:412-414): the
        [interests | gt | user_id | photo_id] rows.  Returns a dict {"final", "results_list"[, "cold_final", "hot_final",
        "cold_count_inter", "hot_count_inter"][, "saved_logits"]}.
        ``device_metrics=True``: the per-row metrics (JaccardSim, LeaveMSE, LeaveCTR, LeaveCTR_view) and the cold / hot split are
        computed and summed on the device (:meth:`_test_model_device`) instead of in the host row loop of ``main_eval_batch``;
        same keys, plus "extras".
        ``ema=True`` (needs ``Trainer(ema=...)``): the pass runs on the averaged weights (``ema.applied()``); a checkpoint's
        ``"model_ema"`` entry is restored into the EMA first."""
        scope = self._ema_scope(ema, "test_model")
        if ckpt is not None:
            load_dict = ckpt.load_checkpoint(self.model, self.opt, mode="best", **({"ema": self.ema} if ema else {}))
            self.model.load_state_dict(load_dict["model"])
        with scope:
            return self._test_model(test_batches, eval_type_list, threshold, top_k_mask, top_k_permutation, save_logits, train_videos, draw_case,
                                    device_metrics)

    def _test_model(self, test_batches, eval_type_list, threshold, top_k_mask, top_k_permutation, save_logits, train_videos, draw_case,
                    device_metrics):
        import argparse
        from .my_evaluation import main_eval_batch
        model = self.model
        model.eval()
        margs = argparse.Namespace(TOP_K_mask=top_k_mask, TOP_K_permutation=top_k_permutation, draw_case=draw_case)
        if device_metrics:
            return self._test_model_device(test_batches, eval_type_list, margs, threshold, save_logits, train_videos)

        def fresh():
            r = {}
            for eval_type in eval_type_list:
                r[eval_type] = []
                r["view_lengths"] = []
            return r

        results_list = fresh()
        cold = train_videos is not None
        cold_results, hot_results, cold_n, hot_n = (fresh(), fresh(), 0, 0) if cold else (None, None, 0, 0)
        saved = []
        exposure = None
        for batch in test_batches:
            out = self.eval_step(batch, mode="inference")
            logits = out["logits"]
            if exposure is None:
                exposure = torch.tensor(model.exposure_prob, dtype=torch.float32, device=logits.device)[: logits.shape[1]]
            interests = torch.sigmoid(logits) * exposure
            pred_label = torch.where(interests > threshold, 1.0, 0.0)
            gt = out["gt"]
            if save_logits:
                saved.append(torch.cat((interests.cpu(), gt.cpu().to(torch.float32), batch["user_id"].reshape(-1, 1).cpu().to(torch.float32),
                                        batch["photo_id"].reshape(-1, 1).cpu().to(torch.float32)), dim=1))
            results_list = main_eval_batch(margs, interests, gt, pred_label, results_list, type="inference")
            if cold:
                pids = batch["photo_id"].reshape(-1).cpu().tolist()
                ci = [i for i, p_ in enumerate(pids) if p_ not in train_videos]
                hi = [i for i, p_ in enumerate(pids) if p_ in train_videos]
                cold_n += len(ci)
                hot_n += len(hi)
                if ci:          # (the reference indexes with an empty tensor and lets main_eval_batch see 0 rows; nothing is appended then)
                    ix = torch.tensor(ci, device=interests.device)
                    cold_results = main_eval_batch(margs, interests[ix], gt[ix], pred_label[ix], cold_results, type="inference")
                if hi:
                    ix = torch.tensor(hi, device=interests.device)
                    hot_results = main_eval_batch(margs, interests[ix], gt[ix], pred_label[ix], hot_results, type="inference")
        res = {"final": compute_final_result(results_list), "results_list": results_list}
        if cold:
            res.update(cold_final=compute_final_result(cold_results), hot_final=compute_final_result(hot_results),
                       cold_count_inter=cold_n, hot_count_inter=hot_n)
        if save_logits:
            res["saved_logits"] = torch.cat(saved, dim=0) if saved else torch.empty((0, 0))
        return res

    def _test_model_device(self, test_batches, eval_type_list, margs, threshold, save_logits, train_videos):
        """The batch loop of :meth:`test_model` with the per-row metrics on the device: per batch one ``row_metrics_device`` call and
        one ``RowMetricAccumulator.add`` (csrc/evalops.h); ``main_eval_batch`` sees only the batch-level metrics (ProbAUC / TOP_K,
        device kernels already).  Cold / hot rows come from the kernel's ``group`` field and a byte table of ``train_videos``; no
        [B, S] tensor goes to the host unless ``save_logits`` asks for it.  Data parallel: every rank evaluates the batches it was
        given, the accumulator is all-reduced once at the end, so the per-row finals are those of all ranks' rows."""
        from .my_evaluation import RowMetricAccumulator, main_eval_batch, row_metrics_device, seen_table
        model = self.model
        per_row = ("JaccardSim", "LeaveMSE", "LeaveCTR", "LeaveCTR_view")
        batch_level = [e for e in eval_type_list if e not in per_row]

        def fresh():
            r = {}
            for eval_type in batch_level:
                r[eval_type] = []
            r["view_lengths"] = []
            return r

        results_list = fresh()
        cold = train_videos is not None
        cold_results, hot_results = (fresh(), fresh()) if cold else (None, None)
        subsets = cold and any(e in ("ProbAUC", "TOP_K") for e in batch_level)
        saved = []
        exposure = seen = acc = None
        for batch in test_batches:
            out = self.eval_step(batch, mode="inference")
            logits = out["logits"]
            if exposure is None:
                exposure = torch.tensor(model.exposure_prob, dtype=torch.float32, device=logits.device)[: logits.shape[1]]
                acc = RowMetricAccumulator(logits.device)
                if cold:
                    seen = seen_table(train_videos, logits.device)
            interests = torch.sigmoid(logits) * exposure
            pred_label = torch.where(interests > threshold, 1.0, 0.0)
            gt = out["gt"]
            if save_logits:
                saved.append(torch.cat((interests.cpu(), gt.cpu().to(torch.float32), batch["user_id"].reshape(-1, 1).cpu().to(torch.float32),
                                        batch["photo_id"].reshape(-1, 1).cpu().to(torch.float32)), dim=1))
            results_list = main_eval_batch(margs, interests, gt, pred_label, results_list, type="inference")
            rec = row_metrics_device(interests, gt, photo_id=batch["photo_id"] if cold else None, seen=seen)
            acc.add(rec)
            if subsets:          # the batch-level metrics of the cold / hot rows: today's indexed calls, the rows named by the kernel
                for grp, sub in ((1, cold_results), (0, hot_results)):
                    ix = torch.nonzero(rec["group"] == grp).reshape(-1)
                    if ix.numel():
                        main_eval_batch(margs, interests[ix], gt[ix], pred_label[ix], sub, type="inference")
        if acc is None:
            acc = RowMetricAccumulator(next(model.parameters()).device)
        acc.all_reduce(self.comm)

        def final(batch_results, group):
            f = compute_final_result(batch_results)
            rows = acc.extras(group)["rows"]
            for k, v in acc.final(eval_type_list, group).items():
                if rows or k == "LeaveMSE":          # compute_final_result leaves out the mean of an empty list; LeaveMSE is NaN there
                    f[k] = v
            return f, rows

        res = {"final": final(results_list, "all")[0], "results_list": results_list, "extras": acc.extras("all")}
        if cold:
            (cf, cn), (hf, hn) = final(cold_results, "cold"), final(hot_results, "hot")
            res.update(cold_final=cf, hot_final=hf, cold_count_inter=cn, hot_count_inter=hn)
        if save_logits:
            res["saved_logits"] = torch.cat(saved, dim=0) if saved else torch.empty((0, 0))
        return res

    def fit(self, train_batches, valid_batches, epochs, **kw):
        """The reference's train / validate / checkpoint / early-stop loop (module-level :func:`fit`)."""
        return fit(self, train_batches, valid_batches, epochs, **kw)

    @torch.no_grad()
    def eval_step(self, batch, mode="inference"):
        model = self.model
        model.eval()
        usr, um, vid, vm = self._features(batch)
        return model(usr_image=usr, usr_id=batch["user_identity_id"], usr_mask=um, vid_image=vid,
                     vid_id=batch["photo_identity_id"], vid_mask=vm, gt=batch["label"], mode=mode)

    @torch.no_grad()
    def dump_logits(self, splits, store=None, ema: bool = False):
        """The dump loop of the reference's inference script (inference/save_logits_for_all_leave_SegMM.py:105-146): eval mode,
        ``mode="inference"`` over every batch of every split in order, ``test_logits["<user_id>-<photo_id>-<time_ms>"] = logits`` --
        into a :class:`bridge.DeviceLogitStore`, so the logits stay on the device and no batch synchronises with the host.  ``splits``:
        an iterable of batch iterables (train, valid, test; ``DeviceBatches`` yields the three key columns on the device).
        ``ema=True`` (needs ``Trainer(ema=...)``): the logits of the averaged weights (``ema.applied()``)."""
        from .bridge import DeviceLogitStore
        with self._ema_scope(ema, "dump_logits"):
            for batches in splits:
                for batch in batches:
                    logits = self.eval_step(batch, mode="inference")["logits"]
                    if store is None:
                        store = DeviceLogitStore(S=logits.shape[1], device=logits.device)
                    store.add_batch(batch["user_id"], batch["photo_id"], batch["time_ms"], logits)
        if store is None:
            store = DeviceLogitStore(device=next(self.model.parameters()).device)
        return store

    @torch.no_grad()
    def valid_model(self, batches, metrics=("valid_loss", "HR@1", "HR@3", "HR@5", "HR@10", "NDCG@1", "NDCG@3", "NDCG@5", "NDCG@10"),
                    permutation=1, top_k_mask=False, recorded=False, seed=None, ema=False):
        """``valid_model`` of the reference trainer (main_for_seq_leave_earlystop_SegMM.py:132-186): eval-mode forward
        with ``mode="train"`` (loss + logits), interests = sigmoid(logits) * exposure_prob, leave-rank metrics per batch,
        mean over batches.  The ranks are computed on the device (csrc/evalops.h); only B integers per batch reach the
        host instead of the [B, S] interests, labels and masks.
        ``recorded=True`` (opt-in; single process): the pass never waits for the host between batches -- :meth:`valid_enqueue`
        followed by ``finish()`` of the accumulator it returns; ``seed``: the seed of the pass's candidate shuffles (see there).
        ``ema=True`` (needs ``Trainer(ema=...)``): the pass, eager or recorded, runs on the averaged weights (``ema.applied()``: the
        weight planes are re-split for them at the head of the pass and for the trained weights at the next step)."""
        if ema:
            with self._ema_scope(ema, "valid_model"):
                return self.valid_model(batches, metrics=metrics, permutation=permutation, top_k_mask=top_k_mask, recorded=recorded, seed=seed)
        if recorded:
            return self.valid_enqueue(batches, metrics=metrics, permutation=permutation, top_k_mask=top_k_mask, seed=seed).finish()
        from .my_evaluation import TOP_K_leave_device
        model = self.model
        exposure = None
        acc = {k: [] for k in metrics}
        for batch in batches:
            out = self.eval_step(batch, mode="train")
            logits, gt = out["logits"], out["gt"]
            if exposure is None:
                exposure = torch.tensor(model.exposure_prob, dtype=torch.float32, device=logits.device)[: logits.shape[1]]
            interests = torch.sigmoid(logits) * exposure
            dp = self.comm.active
            ev = TOP_K_leave_device(interests, gt, permutation=permutation, masked=top_k_mask,
                                    gather=self.comm.gather_ints if dp else None)
            for k in acc:
                # data parallel: every rank's loss terms are already divided by the GLOBAL normalisers, so the global value
                # is their sum over ranks; the rank metrics above are those of the global batch
                if k == "valid_loss":
                    acc[k].append(float(self.comm.sum_scalar(out["loss"].detach().clone())))
                elif k in out and k not in ("gt", "logits"):
                    acc[k].append(float(self.comm.sum_scalar(out[k].detach().clone())) if dp and k not in ("mse", "mse2") else float(out[k]))
                elif k in ev:
                    acc[k].append(float(ev[k]))
        return {k: (sum(v) / len(v) if v else float("nan")) for k, v in acc.items()}

    # ---- a validation pass that never waits for the host between batches (recorded eval forward + device tail)
    @staticmethod
    def _shapes_of(batch):
        return {k: (tuple(v.shape), v.dtype) for k, v in batch.items() if torch.is_tensor(v) and v.numel()}

    def _valid_seed(self, ordinal):
        """The seed of the candidate shuffles of the ``ordinal``-th recorded validation pass of this trainer: a splitmix64 mix of the
        model seed -- the seed word the device step state was initialised with (``device_state``), else ``torch.initial_seed()`` --
        and the pass ordinal.  Nothing is drawn from torch's generator."""
        base = self.__dict__.get("_seed0")
        if base is None:
            base = torch.initial_seed()
        m = (1 << 64) - 1
        z = (int(base) + 0x9E3779B97F4A7C15 * (int(ordinal) + 1)) & m
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
        return (z ^ (z >> 31)) & H.SEED_MASK

    def _valid_exposure(self, S, dev):
        """(key, tensor) of exposure_prob[:S] on the device, made once per value."""
        key = (tuple(float(x) for x in list(self.model.exposure_prob)[:S]), str(dev))
        c = self.__dict__.setdefault("_valid_expo", {})
        if key not in c:
            if len(key[0]) < S:
                raise RuntimeError("exposure_prob has %d entries, S=%d" % (len(key[0]), S))
            c[key] = torch.tensor(key[0], dtype=torch.float32, device=dev)
        return key, c[key]

    def _valid_tail(self, out, acc, i, cfg, seed):
        """The device tail of validation batch ``i``: ranks of its rows (segmm_valid_rows) at the batch's row offset of the pass's
        table, its loss scalars into the batch's row (two segmm_copy_bytes).  No synchronisation."""
        logits = out["logits"]
        H.mark(H.PHASE_STEP_TAIL)
        H.valid_rows(logits, self._valid_exposure(logits.shape[1], logits.device)[1], out["gt"], ranks=acc.rank_slice(i), masked=cfg[1],
                     permute=cfg[0], seed=seed, site=E.SITE_VALID_PERM, row0=acc.offsets[i])
        acc.add_scalars(i, self.model.__dict__["_losses_vec"], out["loss"])

    @torch.no_grad()
    def valid_enqueue(self, batches, metrics=("valid_loss", "HR@1", "HR@3", "HR@5", "HR@10", "NDCG@1", "NDCG@3", "NDCG@5", "NDCG@10"),
                      permutation=1, top_k_mask=False, seed=None, keep_logits=False):
        """The enqueue part of ``valid_model(recorded=True)``: every batch of the pass is put on the stream without one host
        synchronisation (the pass that records excepted) and a :class:`my_evaluation.ValidationAccumulator` is returned, whose
        ``finish()`` does the pass's single read-back and gives the dict ``valid_model`` returns.

        Per batch the eval-mode forward with ``mode="train"`` is followed by a device tail: ONE segmm_valid_rows launch (interests =
        sigmoid(logits) * exposure, the candidate shuffles, the leave ranks, written at the batch's row offset of the pass's rank
        table) and two segmm_copy_bytes (the 12 loss slots and the total into the batch's row of the scalar table).
        The FIRST batch of the first such pass runs launch by launch while it is recorded (``H.Recorder``, a private memory pool, the
        batch's tensors re-based per replay, as :meth:`record` does for the training step); every later batch of that shape, in this
        and in later passes, is replayed with one C call per phase.  A batch of any other shape (the short last batch) takes the
        eager launches with the same device tail: still no synchronisation, just not replayed -- one shape is recorded.
        * Site headers: the recorded batch draws its header rows from an arena of its own (``ParamStore.hdr_private_arena``), cleared
          by a fill command at the head of the replay; the training step's arena and the wrapping ring of the eager passes are not
          touched.  The recording also has its own memory pool and events, and shares the trainer's three streams: it coexists with
          a recorded training step.
        * Weight planes: the split runs EAGERLY ahead of each pass (``ParamStore.ensure`` at its head re-splits iff the weights moved
          since the last split); the recording carries no split, a replay reads the planes of the moment.
        * Per replay the named slots that change are rewritten (``hipabi.cmd_set_arg``, by op and parameter name): ``ranks``, ``row0``
          and ``seed`` of segmm_valid_rows, ``dst`` of the two copies.
        * ``permutation``: the shuffles are drawn in the kernel, keyed by (seed, site, row index in the pass): the reference's
          distribution, not numpy's bit stream.  ``seed``: None = :meth:`_valid_seed` of this trainer's pass counter (a new draw
          per pass, reproducible under torch.manual_seed); an int = that seed (bits 0 .. 62).
        Refused by name: data parallelism (``comm.active``: the per-batch rank gather and loss all-reduce need a design of their
        own), non-contiguous batch tensors, stray dtypes, any ``hipabi.torch_fallback`` while recording.  ``keep_logits``: the
        accumulator also keeps a copy of every batch's logits (debugging hook)."""
        from .decoder_leave_focal import _LIDX
        from .my_evaluation import ValidationAccumulator
        if self.comm.active:
            raise RuntimeError("valid_model(recorded=True) is not supported under data parallelism (an active DPComm): the per-batch "
                               "rank gather and loss all-reduce are host-driven collectives; use recorded=False")
        batches = list(batches)
        for b in batches:
            self._refuse_unrecordable(b, "valid_model(recorded=True)", "validation batch")
        model, st = self.model, self.model._store
        ordinal = self.__dict__.get("_valid_passes", 0)
        self._valid_passes = ordinal + 1
        seed = (self._valid_seed(ordinal) if seed is None else int(seed)) & H.SEED_MASK
        model.eval()
        acc = ValidationAccumulator([b["label"].shape[0] for b in batches], next(model.parameters()).device, metrics, keep_logits=keep_logits)
        if not batches:
            return acc
        st.ensure()          # the weights of the moment: their planes are split here, ahead of the pass's first replay
        self._pf = None      # (like eval_step: a prefetched input stage is dropped)
        for i, batch in enumerate(batches):
            S = batch["label"].shape[1]
            cfg = (bool(permutation), bool(top_k_mask), self._valid_exposure(S, st.flat.device)[0])
            r = self.__dict__.get("_valid_rec")
            if r is None:
                out = self._valid_record(batch, acc, i, cfg, seed)
            elif r["cfg"] == cfg and self._shapes_of(batch) == r["spans"]:
                out = self._valid_replay(r, batch, acc, i, seed)
            else:
                out = self.eval_step(batch, mode="train")
                self._valid_tail(out, acc, i, cfg, seed)
            if not acc.loss_slots:
                acc.loss_slots = dict({k: _LIDX[k] for k in out if k in _LIDX}, loss=acc.TOTAL)
            if acc.logits is not None:
                acc.logits.append(out["logits"].clone())
        return acc

    def _valid_record(self, batch, acc, i, cfg, seed):
        """Runs validation batch ``i`` launch by launch while recording it (see :meth:`valid_enqueue`) -> its output dict."""
        model, st = self.model, self.model._store
        side, aux = st.side_stream(), st.aux_stream()          # both exist before the recorder maps their handles to slots
        hold = self.__dict__.setdefault("_valid_hdr", {})
        torch.cuda.synchronize()
        main = H._stream()
        pool = torch.cuda.MemPool()
        rec = H.Recorder(main, side.cuda_stream, aux.cuda_stream)
        H.RECORDER = rec
        try:
            with st.rec_pool(pool), st.hdr_private_arena(hold) as arena:
                H.mark(H.PHASE_STEP_BEGIN)
                H.fill_zero(arena[:1])          # (the arena is clean now; the replays clear what this batch drew: size patched below)
                out = self.eval_step(batch, mode="train")
                self._valid_tail(out, acc, i, cfg, seed)
        finally:
            H.RECORDER = None
        torch.cuda.synchronize()
        phases = rec.finish()
        ops = H.op_ids()
        cmds = [(arr, ci) for ph, arr in phases if arr is not None for ci in range(ph.n_cmds)]
        tail = [(ph, arr) for ph, arr in phases if arr is not None][-1]
        named = {n: [tail[1][ci] for ci in range(tail[0].n_cmds) if tail[1][ci].op == ops[n]] for n in ("segmm_valid_rows", "segmm_copy_bytes")}
        fill = cmds[0][0][cmds[0][1]]
        if (fill.op != ops["segmm_fill_zero"] or tail[0].kind != H.PHASE_STEP_TAIL or len(named["segmm_valid_rows"]) != 1
                or len(named["segmm_copy_bytes"]) != 2):
            raise RuntimeError("valid_model(recorded=True): the recorded launch sequence does not have the expected head (header fill) "
                               "and tail (segmm_valid_rows, two segmm_copy_bytes)")
        H.cmd_set_arg(fill, "segmm_fill_zero", "bytes", hold["used"] * H.SITE_FLOATS * 4)
        # the batch's tensors: every recorded POINTER argument that falls inside one of them is re-based per replay (see record())
        spans = [(k, v.data_ptr(), v.numel() * v.element_size()) for k, v in batch.items() if torch.is_tensor(v) and v.numel()]
        relocs = []
        for pi, (ph, arr) in enumerate(phases):
            if arr is None:
                continue
            for ci, ai in rec.pslots[pi]:
                pv = arr[ci].a[ai].p
                for k, base, nb in spans:
                    if base <= pv < base + nb:
                        relocs.append((arr, ci, ai, k, pv - base))
                        break
        evs = tuple(torch.cuda.Event() for _ in range(4))
        for e in evs:
            e.record()
        self._valid_rec = dict(phases=phases, keep=rec.keep, pool=pool, out=out, relocs=relocs, spans=self._shapes_of(batch), cfg=cfg, main=main,
                               events=evs, table=H.stream_table([main, side.cuda_stream, aux.cuda_stream], [e.cuda_event for e in evs]),
                               valid_rows=named["segmm_valid_rows"][0], copies=named["segmm_copy_bytes"], losses=model.__dict__["_losses_vec"],
                               n_cmds=len(cmds), n_replays=0)
        return out

    def _valid_replay(self, r, batch, acc, i, seed):
        """Enqueues validation batch ``i`` from the recorded launch sequence: the batch's addresses and the per-batch slots of the
        tail are patched, then one C call per phase.  Returns the recording's output dict (rewritten by every replay)."""
        if H._stream() != r["main"]:
            raise RuntimeError("valid_model(recorded=True): the current stream is not the stream the validation batch was recorded on")
        for arr, ci, ai, k, off in r["relocs"]:
            arr[ci].a[ai].p = batch[k].data_ptr() + off
        vr = r["valid_rows"]
        H.cmd_set_arg(vr, "segmm_valid_rows", "ranks", acc.rank_slice(i).data_ptr())
        H.cmd_set_arg(vr, "segmm_valid_rows", "row0", acc.offsets[i])
        H.cmd_set_arg(vr, "segmm_valid_rows", "seed", seed)
        dst = acc.scalars[i].data_ptr()
        H.cmd_set_arg(r["copies"][0], "segmm_copy_bytes", "dst", dst)
        H.cmd_set_arg(r["copies"][1], "segmm_copy_bytes", "dst", dst + 4 * acc.TOTAL)
        for ph, arr in r["phases"]:
            if arr is None:
                ph()
            else:
                H.run_phase(ph, r["table"])
        r["n_replays"] += 1
        return r["out"]


def early_stop_reached(metric_history: List[float], early_stop: int) -> bool:
    """The two early-stop tests of the reference loop on the monitored validation metric (higher is better),
    main_for_seq_leave_earlystop_SegMM.py:336-352: (i) none of the last ``early_stop`` validations beat the first of that window,
    (ii) the best validation lies more than ``early_stop`` validations back."""
    m = list(metric_history)
    if early_stop <= 0 or not m:
        return False
    if len(m) > early_stop:
        lst = m[-early_stop:]
        if all(lst[0] >= y for y in lst[1:]):
            return True
    return len(m) - m.index(max(m)) > early_stop


def compute_final_result(results_list):
    """``compute_final_result`` of the reference trainer (main_for_seq_leave_earlystop_SegMM.py:188-210): LeaveMSE = mean squared
    error of the predicted against the true view lengths, every other list its mean; 'TOP_K' and 'view_lengths' carry no number."""
    final = {}
    if "LeaveMSE" in results_list:
        vl, pv = results_list["view_lengths"], results_list["LeaveMSE"]
        final["LeaveMSE"] = float(sum((float(a) - float(b)) ** 2 for a, b in zip(vl, pv)) / len(vl)) if vl else float("nan")
    for eval_type, vals in results_list.items():
        if eval_type in ("TOP_K", "LeaveMSE", "view_lengths"):
            continue
        if not isinstance(vals, list) or not vals:
            continue
        final[eval_type] = sum(vals) / len(vals)
    return final


def fit(trainer: "Trainer", train_batches, valid_batches, epochs: int, valid_step: int = 30, early_stop: int = 0,
        main_metric: str = "NDCG@5", ckpt: Optional["CheckPointer"] = None, logging_step: int = 0, log=None,
        permutation: int = 1, top_k_mask: bool = False, metrics=None, recorded: bool = False, eager_steps: int = 3,
        lr_plateau: Optional[dict] = None, recorded_valid: bool = False, ema_valid: bool = False):
    """The train / validate / checkpoint / early-stop loop of the reference trainer around ``Trainer.train_step``
    (main_for_seq_leave_earlystop_SegMM.py:247-354): one validation over ``valid_batches`` BEFORE training, then per epoch every
    ``valid_step`` local steps a validation whose ``main_metric`` (mean over the validation batches, :179-181) drives
    ``ckpt.save_checkpoint(..., metric_vals={"main_metric": ...})`` (:333) and the early-stop tests (:336-352).
    ``train_batches``: a list of batch dicts, or a callable ``epoch -> iterable of batch dicts`` (an epoch of the DataLoader).
    The loss is read on the host only where the reference's bookkeeping needs a number (validation points, logging steps).
    ``recorded=True`` (needs ``Trainer(device_state=True)``; single process or data parallel): the first ``eager_steps`` steps run
    launch by launch (they calibrate the delayed scales), the next step is RECORDED while it runs (``Trainer.record`` with the
    previous batch: no extra optimisation step), every later batch of the same shapes is enqueued from the recorded launch
    sequences (``run_recorded``: one C call per phase, bit-identical to the eager step); a batch of another shape (the short last
    batch of an epoch) takes the eager step.  Every batch is still stepped on exactly once, in order.
    ``lr_plateau`` (a dict of :class:`PlateauLR` arguments, e.g. ``dict(factor=0.5, patience=2, min_lr=1e-6)``; ``mode`` defaults to
    "max", the sense of the early-stop tests): reduce-on-plateau with torch.optim.lr_scheduler.ReduceLROnPlateau's rules, fed after
    every validation of the loop the number early stopping reads -- every data-parallel rank decides alike -- and acting through
    ``opt.set_base_lr``, so it needs ``Trainer(lr_schedule=...)`` ("constant" suffices) and works under ``recorded=True``.
    ``recorded_valid=True`` (independent of ``recorded``; single process): every validation of the loop goes through
    ``Trainer.valid_model(recorded=True)`` -- no host round trip between its batches, one read-back per validation; with
    ``permutation=0`` the history equals the eager validations' exactly, with ``permutation=1`` the shuffles come from the device.
    ``ema_valid=True`` (needs ``Trainer(ema=...)``): every validation of the loop runs on the averaged weights
    (``valid_model(ema=True)``), so the best checkpoint, early stopping and ``lr_plateau`` follow them.  With an EMA every checkpoint
    carries the average as ``"model_ema"`` (beside ``"model"``, the trained weights), whatever ``ema_valid`` says.
    Returns the history dict the reference calls ``total_valid_loss_metrics`` (+ "stopped_epoch", "global_step")."""
    metrics = list(metrics) if metrics is not None else ["valid_loss", "HR@1", "HR@3", "HR@5", "HR@10", "NDCG@1", "NDCG@3", "NDCG@5", "NDCG@10"]
    hist: Dict[str, list] = {"train_loss": [0.0]}
    for k in metrics:
        hist[k] = []

    def validate():
        vm = trainer.valid_model(valid_batches, metrics=tuple(metrics), permutation=permutation, top_k_mask=top_k_mask,
                                 **({"recorded": True} if recorded_valid else {}), **({"ema": True} if ema_valid else {}))
        for k in metrics:
            hist[k].append(vm[k])
        return vm

    if recorded and not trainer.device_state:
        raise RuntimeError("fit(recorded=True) needs Trainer(device_state=True)")
    if ema_valid and trainer.ema is None:
        raise ValueError("fit(ema_valid=True) needs Trainer(ema=...): this trainer keeps no weight average")
    plateau = None
    if lr_plateau is not None:
        if not isinstance(lr_plateau, dict):
            raise ValueError("lr_plateau must be a dict of PlateauLR arguments, not %r" % (lr_plateau,))
        if trainer.opt.schedule is None:
            raise ValueError("fit(lr_plateau=...) needs Trainer(lr_schedule=...): \"constant\" suffices")
        try:
            plateau = PlateauLR(trainer.opt, **{"mode": "max", **lr_plateau})
        except TypeError as e:
            raise ValueError("lr_plateau: %s" % e)

    def shapes_of(b):
        return {k: (tuple(v.shape), v.dtype) for k, v in b.items() if torch.is_tensor(v) and v.numel()}

    def step(batch, prev, n_done):
        """One optimisation step on ``batch``: eager, recording, or from the recording."""
        if not recorded:
            return trainer.train_step(batch)
        r = trainer.__dict__.get("_recorded")
        if r is not None:
            if shapes_of(batch) == r["spans"] and all(v.is_contiguous() for v in batch.values() if torch.is_tensor(v)):
                return trainer.run_recorded(batch)
            return trainer.train_step(batch)
        if n_done >= eager_steps and prev is not None and shapes_of(prev) == shapes_of(batch):
            return trainer.record(batch, prev_batch=prev)
        return trainer.train_step(batch)

    validate()                                           # "Evaluation Before Training" (:247-249)
    global_step, stop, stopped_epoch = 0, False, None
    prev_batch = None
    for epoch in range(epochs):
        if stop:
            break
        it = train_batches(epoch) if callable(train_batches) else train_batches
        epoch_losses = []
        for local_step, batch in enumerate(it):
            out = step(batch, prev_batch, global_step)
            prev_batch = batch
            # (a recorded step returns the SAME loss tensor every step: keep a copy where the epoch mean is going to be logged)
            epoch_losses.append(out["loss"].detach().clone() if (recorded and log is not None) else out["loss"].detach())
            global_step += 1
            if logging_step and (local_step + 1) % logging_step == 0 and log is not None:
                log("Train_loss: %f, Global_step: %d" % (float(epoch_losses[-1]), global_step))
            if (local_step + 1) % valid_step == 0:
                hist["train_loss"].append(float(epoch_losses[-1]))
                validate()
                avg = hist[main_metric][-1]
                if plateau is not None and plateau.step(avg) is not None and log is not None:
                    log("Base learning rate: %g, Global_step: %d" % (trainer.opt.lr, global_step))
                if log is not None:
                    log("Valid_loss: %s, %s: %s, Global_step: %d" % (hist["valid_loss"][-1] if "valid_loss" in hist else None, main_metric, avg, global_step))
                if ckpt is not None and trainer.comm.rank == 0:
                    ckpt.save_checkpoint(model=trainer.model, optimizer=trainer.opt, num_epochs=epoch, metric_vals={"main_metric": avg},
                                         **({"ema": trainer.ema} if trainer.ema is not None else {}))
                if early_stop_reached(hist[main_metric], early_stop):
                    stop, stopped_epoch = True, epoch
                    break
        if log is not None and epoch_losses:
            log("Epoch: %d, Epoch Loss: %f" % (epoch, float(torch.stack(epoch_losses).mean())))
    hist["stopped_epoch"] = stopped_epoch
    hist["global_step"] = global_step
    return hist


class CheckPointer:
    """kn_util CheckPointer file format (kn_util/nn_utils/checkpoint.py:11-75): a dict
    {model, optimizer, num_epochs, metrics} in ckpt-latest.pth and ckpt-best-ep{E}-{metric}.pth."""

    def __init__(self, monitor, work_dir, mode="min", **_ignored):
        import os
        self.monitor, self.work_dir, self.mode, self.best_metric = monitor, work_dir, mode, None
        os.makedirs(work_dir, exist_ok=True)
        self.ckpt_latest = os.path.join(work_dir, "ckpt-latest.pth")
        self.ckpt_best = os.path.join(work_dir, "ckpt-best-ep{}-{}.pth")

    def better(self, new, orig):
        if orig is None:
            return True
        return new < orig if self.mode == "min" else new > orig

    def save_checkpoint(self, model, optimizer, num_epochs, metric_vals=None, ema=None, **_):
        """``ema`` (a :class:`WeightEMA`): one more key, ``"model_ema"`` = ``ema.state_dict()`` -- the model's own keys and shapes."""
        import glob
        import os
        sd = dict(model={k: v.detach().cpu().clone() for k, v in model.state_dict().items()},
                  optimizer=optimizer.state_dict(), num_epochs=num_epochs, metrics=metric_vals)
        if ema is not None:
            sd["model_ema"] = ema.state_dict()
        torch.save(sd, self.ckpt_latest)
        if metric_vals and self.better(metric_vals[self.monitor], self.best_metric):
            self.best_metric = metric_vals[self.monitor]
            for f in glob.glob(self.ckpt_best.format("*", "*")):
                os.remove(f)
            torch.save(sd, self.ckpt_best.format(num_epochs, round(float(self.best_metric), 6)))
            return True
        return False

    def load_checkpoint(self, model, optimizer, mode="latest", ema=None, **_):
        """``ema`` (a :class:`WeightEMA`): restored from the file's ``"model_ema"``; a file without that key is refused by name
        (before anything is loaded).  Without ``ema`` the key is ignored and any file loads as ever."""
        import glob
        fn = self.ckpt_latest if mode == "latest" else glob.glob(self.ckpt_best.format("*", "*"))[0]
        sd = torch.load(fn, map_location="cpu", weights_only=False)
        if ema is not None and "model_ema" not in sd:
            raise KeyError("load_checkpoint(ema=...): %s has no \"model_ema\" entry (it was written without an EMA)" % fn)
        model.load_state_dict(sd["model"])
        if optimizer is not None:
            optimizer.load_state_dict(sd["optimizer"])
        if ema is not None:
            ema.load_state_dict(sd["model_ema"])          # (after the optimizer: its state, and with it the shadow, exists now)
        return sd
