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

This module holds the model factory and the step (``Trainer``); the optimizer, the schedules and the EMA are in optim.py, the
collectives in dp.py, capture / relocation / replay of a recorded launch sequence in recording.py, the evaluation passes in
eval_passes.py and the epoch loop in loop.py.  Their public names are re-exported here.
"""
from __future__ import annotations

import argparse
import contextlib
import functools
from typing import Dict, Optional

import torch
import torch.nn as nn

from . import engine as E
from . import hipabi as H
from . import recording as R
from . import switches
from .decoder_leave_focal import _LIDX, LossSpec, MultiScaleTemporalDetrLeaveFocal
from .dp import DPComm, shard_rows  # noqa: F401
from .encoder import SegFormerX
from .eval_passes import EvalPasses
from .loop import CheckPointer, compute_final_result, early_stop_reached, fit  # noqa: F401
from .optim import (GROUP_KEYS, FusedAdamW, LRSchedule, PlateauLR, WeightEMA, group_segments, no_decay_groups, parse_ema,  # noqa: F401
                    parse_lazy_data_parallel, parse_lazy_ema, parse_lazy_tables, parse_skip_nonfinite, resolve_param_groups)


# ------------------------------------------------------------------------------------------------ model factory
def init_model(args, reader=None, n_users: Optional[int] = None, n_items: Optional[int] = None,
               input_dim: int = 1024, max_vid_len: int = 40, max_usr_len: int = 100, ff_dim=None, sr_ratio=None):
    """init_model(args, reader) of the reference trainer (main_for_seq_leave_earlystop_SegMM.py:60-130).
    ``reader`` only needs ``n_users`` / ``n_items``; feature width and lengths default to the
    reference's hard-coded 1024 / 40 / 100 and are overridable for synthetic configs.
    ``ff_dim``: the encoder layers' feed-forward width, an int (every layer) or a list of ``num_layers_enc`` ints.  ``None`` is
    the reference's behaviour: ``[d_model] * N`` whatever ``args.ff_dim`` says (main...SegMM.py:91 never reads that option, whose
    default is 512 for every d_model: honouring it implicitly would change existing runs).
    ``sr_ratio``: the encoder layers' spatial-reduction ratio, an int (every layer) or a list of ``num_layers_enc`` ints; ``None`` is
    the reference trainers' ``[1] * N`` (main...SegMM.py:94).  A ratio above 1 needs ``args.sr_attn = 1`` (encoder.check_sr_ratio);
    the MLP ablations build no encoder and ignore it."""
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
    if sr_ratio is None or getattr(args, "ablation_type", "ours") in E.MLP_VARIANTS:
        sr = [1] * N
    elif isinstance(sr_ratio, int):
        sr = [sr_ratio] * N
    else:
        sr = [int(r) for r in sr_ratio]
        if len(sr) != N:
            raise ValueError("sr_ratio lists %d ratios for num_layers_enc = %d" % (len(sr), N))

    def backbone(user_id_max, video_id_max, usr_len):
        return SegFormerX(d_model_in=d, d_model_lvls=[d] * N, num_head_lvls=[h] * N, ff_dim_lvls=ff,
                          input_vid_dim=input_dim, input_usr_dim=input_dim, max_vid_len=max_vid_len, max_usr_len=usr_len,
                          sr_ratio_lvls=sr, use_patch_merge=[False] * N, output_layers=[-1], model_cfg=args,
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
class Trainer(EvalPasses):
    """zero_grad -> L1-normalise -> forward -> backward (-> bucketed all-reduce) -> AdamW, i.e. the body of
    the reference's hot loop (main_for_seq_leave_earlystop_SegMM.py:269-300) minus its host syncs.
    Gradient clipping is a no-op in the reference (exhausted generator at :298), so the default ``max_grad_norm=None`` does not
    clip; ``max_grad_norm=m`` clips to global norm m on the device before AdamW (see FusedAdamW; ``trainer.opt.grad_norm`` is the
    norm the reference logs), in the eager, recorded and data-parallel steps.
    ``skip_nonfinite=True`` (needs ``device_state=True``; see FusedAdamW): a step whose gradient norm is NaN or inf changes no
    parameter, moment or EMA shadow and is counted as skipped, without a host round trip -- ``out["skipped"]`` of ``train_step`` /
    ``run_recorded`` is this step's verdict (a 0-dim device tensor, 0 or 1, valid until the next step), ``opt.skipped_steps`` the count."""


    def __init__(self, model, lr=1e-3, weight_decay=1e-4, comm: Optional[DPComm] = None, overlap=True, dropout=True,
                 feature_table=None, sparse_tables=True, device_state=False, max_grad_norm=None, lr_schedule=None, micro_batch=None,
                 param_groups=None, ema=None, lazy_tables=None, mixed_precision=None, skip_nonfinite=False):
        self.model = model
        # skip_nonfinite=True: the non-finite guard (FusedAdamW).  A bool; needs the device step state; refused beside lazy_tables
        parse_skip_nonfinite(skip_nonfinite, bool(device_state), lazy_tables)
        # mixed_precision=None | False | True | dict(forward=True, dgrad=True, wgrad=True): the plane GEMMs of the named roles multiply
        # ONE product (hi . hi: fp16 operands, fp32 accumulate) in the passes of the optimisation step; master weights, AdamW and
        # every evaluation pass are untouched.  Lives on the model's ParamStore, where the GEMM helpers of engine.py read it.
        mixed_precision = E.resolve_mixed_precision(mixed_precision)          # (a malformed spec is refused before the model is touched)
        # lazy_tables=None | True | dict(flush_every=F): lazy exact AdamW of the item-id tables (FusedAdamW; _tables_early) -- a step
        # reads and writes only the batch's rows of the table.  Under data parallelism the rows touched are those of ALL ranks, known
        # only after the row exchange: that takes the opt-in lazy_tables=dict(data_parallel=True) -- the rank's own rows catch up at
        # the head, the gathered list is stepped by one fused launch at the tail (_tables_early, _finish_step).  Beside ema=... it takes
        # the opt-in lazy_tables=dict(ema=True): the table's shadow rows are then averaged lazily, with the rows (below)
        lazy_dp = False
        if lazy_tables is not None and comm is not None and comm.active:
            parse_lazy_tables(lazy_tables)          # (a malformed spec is refused for what it is, before anything below)
            lazy_dp = parse_lazy_data_parallel(lazy_tables)
            if not lazy_dp:
                raise ValueError("Trainer(lazy_tables=...) is not supported with an active DPComm (data parallel) as it stands: the rows a "
                                 "step touches are all ranks' rows, known only after the row exchange; the dense table update stays "
                                 "there.  lazy_tables=dict(data_parallel=True) opts in to the lazy step behind the row exchange")
            if not (bool(sparse_tables) and switches.read("trainer")["sparse_tables"]):
                raise ValueError("Trainer(lazy_tables=dict(data_parallel=True)) needs the sparse row exchange: with sparse_tables off "
                                 "(sparse_tables=False or SEGMM_SPARSE_TABLES=0) no gathered row list exists")
            if micro_batch is not None:
                raise ValueError("Trainer(lazy_tables=dict(data_parallel=True)) with micro_batch under an active DPComm is not supported: "
                                 "each micro-batch pass has its own row exchange (a follow-up); use one of the two")
        self._lazy_dp = lazy_dp
        # lazy tables beside a weight average take the opt-in lazy_tables=dict(ema=True): the shadow rows of the lazy table are then
        # replayed with the rows (FusedAdamW), and every lazy step, single process too, runs head + fused tail (_tables_early, _lazy_rows)
        if lazy_tables is not None and ema is not None and any(
                bb is not None and bb.id_vid for bb in (model.backbone1, getattr(model, "backbone2", None))):
            parse_lazy_tables(lazy_tables)          # (a malformed spec is refused for what it is)
            if not parse_lazy_ema(lazy_tables):
                raise ValueError("Trainer(lazy_tables=...) with ema: the EMA shadow would average the stale rows of the lazy item-id table; "
                                 "use one of the two, or opt in to the lazily averaged shadow with lazy_tables=dict(ema=True)")
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
                              param_groups=param_groups, ema=ema, lazy_tables=lazy_tables, skip_nonfinite=skip_nonfinite)          # per-group rate scale, decay and freezing: see FusedAdamW
        # ema=None | decay | dict(decay=0.999, warmup=True): a device-side moving average of the weights (WeightEMA), or None
        self.ema = self.opt.ema
        self.comm = comm if comm is not None else DPComm()
        self.overlap = overlap
        st = model._store
        st.mixed_precision = mixed_precision
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

    @property
    def _guard(self) -> bool:
        """The optimizer's non-finite guard (``skip_nonfinite=True``) is on."""
        return bool(getattr(self.opt, "skip_nonfinite", False))

    @property
    def mixed_precision(self):
        """The resolved setting: ``None`` (off), or a dict role -> bool over ``forward``, ``dgrad``, ``wgrad``."""
        mp = self.model._store.mixed_precision
        return None if mp is None else dict(mp)

    @mixed_precision.setter
    def mixed_precision(self, value):
        self.model._store.mixed_precision = E.resolve_mixed_precision(value)

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
        ranks, known only after the row exchange -- the dense update stays, unless lazy_tables=dict(data_parallel=True) opted in:
        then the rank's own rows catch up here and the gathered list is stepped at the tail.)"""
        # a step that failed between this pass and opt.step() (forward / backward error, OOM) left its entry queued and its rows
        # flagged: drop both before queueing this step's, or the table's range would be stepped twice and the failed batch's rows
        # skipped
        stale = self.opt.__dict__.pop("_early", None)
        if stale:
            if any(e[7] is None for e in stale):
                E.join_aux(self.model._store)
            for e in stale:
                e[5].zero_()
            #  the failed step had already advanced the DEVICE step count (segmm_step_advance at its head) while
            # opt.step_count never moved, and THIS step has advanced it once more: put it back to step_count + 1, the number of the
            # step that is running, so its bias corrections are right again.  What cannot be taken back and is accepted: the failed step's early pass applied one g = 0 AdamW
            # update (weight decay + moment decay) to the table rows outside its batch.
            if self.device_state:
                H.step_bind(self._step_state)
                seed, _, _ = H.step_get()
                H.step_set(seed, self.opt.step_count + 1, *self.opt.betas)
        if self._guard:
            # the early pass would run before the step's verdict exists: under the guard the tables are stepped densely at the tail,
            # with the rest of the live range (FusedAdamW.step without an early entry)
            return
        lazy = self.opt.lazy_flush_every is not None
        self._lazy_own = {}          # name -> the batch's own id list, of the tables whose head runs below with mark=False, single process
        if lazy and self._param_hooks():
            raise RuntimeError("Trainer(lazy_tables=...) does not support parameter hooks: a hook may rewrite the gradient of table rows "
                               "outside the batch, which a lazy step never reads")
        # (an active comm with lazy tables is the opt-in lazy_tables=dict(data_parallel=True): the constructor refused anything else)
        if (self.comm.active and not lazy) or not (self.table_two_pass or lazy) or self._param_hooks():
            return
        model, st = self.model, self.model._store
        ids = batch.get("photo_identity_id")
        if lazy and torch.is_tensor(ids):
            # the forward reads the batch's rows whatever the id list looks like (engine._as converts it there): a lazy step must
            # bring those rows up to date first, so an int32 or strided list is converted here the same way, never skipped
            ids = E._as(ids, torch.int64, "the item ids")
        elif lazy:
            self.opt.flush_tables()          # (no id list at all: every row current before anything reads the table)
            return
        if ids is None or ids.dtype != torch.int64 or not ids.is_contiguous():
            return
        for pre, bb in (("backbone1.", model.backbone1), ("backbone2.", getattr(model, "backbone2", None))):
            if bb is None or not bb.id_vid:
                continue
            name = pre + "vid_proj.weight"
            if name not in st.index or name not in st.live_names or st._params[name].shape[1] % 4:
                continue
            if lazy:
                # lazy exact AdamW takes the early pass's place: the batch's rows catch up to the step before this one, on the MAIN
                # stream -- the id-embedding forward reads them.  No repair is needed if the step then fails: rows caught up to
                # T - 1 are right whether or not step T happens
                # Data parallel: these are the rank's OWN rows -- the forward reads no others.  Nothing is marked or queued: the rows
                # of the step, all ranks', are stepped behind the row exchange by one fused launch (_finish_step)
                # Beside an EMA (lazy_tables=dict(ema=True)) the single process takes the same form: the fused tail also averages the
                # rows' shadow, on the batch's own list (_lazy_rows)
                own = ids.reshape(-1)
                self.opt.table_lazy(name, own, mark=not (self.comm.active or self.opt._lazy_ema_on))
                if name in self.opt._lazy_tail:
                    self._lazy_own[name] = own
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
        the bytes over the host link), or float8_e4m3fn / float8_e5m2 / int8 (a quarter; hipabi.l1norm widens exactly) -- the single
        point where a batch's feature dtype enters the step."""
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

    @contextlib.contextmanager
    def _step_scope(self, batch):
        """Head and tail of one optimisation step on ``batch``, plain or micro-batched: the step's first launches on entry; on exit,
        however the body ends, the store leaves the step.  An eager step -- of any shape, completed or not -- tells the recording
        that the step before its next replay is not one of its own (:meth:`run_recorded` then clears the id-table gradients itself)."""
        model, st = self.model, self.model._store
        r = self.__dict__.get("_recorded")
        if r is not None and H.RECORDER is None:
            r["prev_batch"] = None
        if self.device_state:
            H.step_bind(self._step_state)          # (a host-side pointer: the launches below carry it in their arguments)
        if model.training != bool(self.dropout):
            model.train(self.dropout)          # (walks every sub-module: 0.35 ms of host time when done every step)
        self.opt.zero_grad()
        H.mark(H.PHASE_STEP_BEGIN)
        if self.device_state:          # first launches of the step: advance the device-side step state (ONE count and one rate per
            # optimizer step), fresh header rows.  skip_nonfinite: the guarded form -- corrections of the applied index, verdict cleared
            (H.step_advance_guarded if self._guard else H.step_advance)(*self.opt.betas)
            st.hdr_step_begin()
        st._trusted = False
        st.in_train_step = True          # (the step's passes take Trainer(mixed_precision=...); evaluation passes never run in here)
        try:
            yield
        finally:
            st._trusted = False
            st.in_train_step = False
            model.__dict__.pop("_stats_pre", None)          # (a step that failed before its forward must not leave this batch's statistics behind)
            if self.device_state:
                st.hdr_step_end()          # evaluation passes between steps draw their headers from the wrapping ring

    def train_step(self, batch: Dict[str, torch.Tensor], next_batch: Optional[Dict[str, torch.Tensor]] = None):
        """One optimisation step on ``batch``.  ``next_batch``: the batch of the FOLLOWING step, if known -- its input stage is
        enqueued on a side stream right away (:meth:`prefetch`) and overlaps this step's backward.
        ``Trainer(micro_batch=m)`` and a batch of more than m rows: the step runs in micro-batches (:meth:`_train_step_micro`; nothing
        is prefetched then)."""
        if self.ema is not None:
            self.ema._refuse_applied("train_step()")
        if self.opt.lazy_flush_every is not None:
            self.opt.lazy_step_head()          # the periodic flush of the lazy tables: between steps, ahead of the step's first launch
        if self.micro_batch is not None and batch_rows(batch) > self.micro_batch:
            return self._train_step_micro(batch, self.micro_batch)
        st = self.model._store
        with self._step_scope(batch):
            usr, um, vid, vm = self._features(batch)          # first ParamStore.ensure() of the step: the full check
            st._trusted = True
            self._tables_early(batch)
            # (a next batch the micro-batched step will take in slices gets no prefetch: that step could not use a whole-batch input
            # stage, whose buffers would be those of all its rows)
            if next_batch is not None and not (self.micro_batch is not None and batch_rows(next_batch) > self.micro_batch):
                self.prefetch(next_batch)
            return self._train_step(batch, usr, um, vid, vm)

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
        if self._param_hooks():
            raise RuntimeError("Trainer(micro_batch=%d) does not support parameter hooks: the micro-batches' gradients are summed in "
                               "the flat gradient buffer, where autograd's hooks never see them" % m)
        for key, v in batch.items():
            if torch.is_tensor(v) and not v.is_contiguous():
                raise RuntimeError("train_step(micro_batch=%d): batch[%r] is not contiguous" % (m, key))
        slices = micro_slices(batch, m)
        with self._step_scope(batch):
            return self._micro_passes(batch, m, slices)

    def _micro_passes(self, batch, m, slices):
        """The body of :meth:`_train_step_micro`, between the step's head and its tail (:meth:`_step_scope`)."""
        model, st = self.model, self.model._store
        k = len(slices)
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
            if self.opt.early_on_aux():
                E.join_aux(st)          # the tables' first pass (aux stream) is complete before their listed rows are stepped
            self.opt.step(lazy_rows=self._lazy_rows(st))          # (lazy_tables=dict(ema=True): the whole batch's ids; otherwise none)
            res = {}
            for key in keys:
                res[key] = logits if key == "logits" else batch["label"] if key == "gt" else sums[12] if key == "loss" else sums[_LIDX[key]]
            if self._guard:
                res["skipped"] = self.opt.skipped
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
            st.__dict__.pop("micro_pass", None)

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
        lazy_rows = self._lazy_rows(st)
        if self._guard:
            out["skipped"] = self.opt.skipped          # (a view of the device step state: the verdict the step's tail leaves there)
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
            if self.opt.max_grad_norm is not None or self._guard:
                # (skip_nonfinite: the verdict is the norm's -- a per-bucket AdamW would run before it; every rank takes the norm of
                # the same all-reduced gradient, hence the same verdict, without a collective)
                # a global norm needs every bucket reduced: no per-bucket overlap, one norm over the reduced live range (each rank
                # computes it from its own, identical copy of the all-reduced gradient), then one AdamW launch
                H.host_action(functools.partial(self._wait_buckets, range(len(works))))
                self.opt.begin_step()
                self.opt.step_ranges(0, st.n_live)
                for name, ids_all in lazy_rows.items():          # (the clip coefficient is the norm's, computed in begin_step)
                    self.opt.table_lazy_rows(name, ids_all)
                self.opt.end_step()
                return out
            self.opt.begin_step()
            # the lazy tables first: their gradient is the row exchange's segment sum, complete on this stream since the backward --
            # no bucket to wait for (the table's range is in no all-reduce), so the launch runs under the collectives still in flight
            for name, ids_all in lazy_rows.items():
                self.opt.table_lazy_rows(name, ids_all)
            order = sorted(range(len(works)), key=lambda i: works[i][0])
            last = len(works) - 1
            early = [i for i in order if i != last]
            if early and works[early[-1]][1] <= works[last][0] and all(works[a][1] == works[b][0] for a, b in zip(early, early[1:])):
                H.host_action(functools.partial(self._wait_buckets, early))
                self.opt.step_ranges(works[early[0]][0], works[early[-1]][1])
                H.host_action(functools.partial(self._wait_buckets, [last]))
                self.opt.step_ranges(works[last][0], works[last][1])
            else:          # not a prefix + tail (two backbones interleave their buckets): one launch per bucket
                for i in range(len(works)):
                    H.host_action(functools.partial(self._wait_buckets, [i]))
                    self.opt.step_ranges(works[i][0], works[i][1])
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
        if self.opt.early_on_aux():
            E.join_aux(st)          # the tables' first pass (aux stream) is complete before their listed rows are stepped
        self.opt.step(lazy_rows=lazy_rows)
        return out

    def _lazy_rows(self, st):
        """Data parallel with lazy tables: name -> the gathered id list of all ranks, for every table whose head ran this step
        (FusedAdamW.table_lazy with mark=False).  The list is the row exchange's persistent buffer (DPComm.gather_rows), which the
        backward left in ``st._tab_rows``: the same tensor every step, so a recorded step names it by address.  Single process such
        heads run only beside an EMA (``lazy_tables=dict(ema=True)``): the list is the batch's own.  Otherwise empty."""
        out = {}
        if not self.comm.active:
            # single process (lazy_tables=dict(ema=True)): the step's rows are the batch's own, the list the head caught up -- a batch
            # tensor, which a recorded step names by its slot
            for name in self.opt._lazy_tail:
                own = self.__dict__.get("_lazy_own", {}).get(name)
                if own is None:
                    raise RuntimeError("lazy_tables=dict(ema=True): no id list of this step for %s (its head did not run)" % name)
                out[name] = own
            return out
        for name in self.opt._lazy_tail:
            ent = st._tab_rows.get(name[:-len("_proj.weight")])
            if ent is None:
                raise RuntimeError("lazy_tables=dict(data_parallel=True): the backward left no gathered row list for %s (the sparse "
                                   "row exchange did not run for this table)" % name)
            out[name] = ent[1]
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
        Eager steps of any shape (``train_step``: the short last batch of an epoch) and validation passes may run between replays.
        What the recorded step takes over from the step before it -- id mode: the list of the table-gradient rows that step
        scattered into, by which this one clears them; the site-header rows it used -- is right as recorded only behind a replay of
        this recording (or the recorded step itself).  Behind any other step ``run_recorded`` clears both itself, from the host
        state that step left, and points the recorded list at its own batch.  No replay names memory outside a tensor of the shape
        it was recorded with: ``run_recorded`` checks every batch tensor a pointer is about to name, on the host, before it
        launches.
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
        self.opt.flush_tables()          # lazy tables: a flush is never part of a recording -- the recorded step starts with none pending
        aux = st.__dict__.get("_aux_stream")
        hdr_cleared = st.__dict__.get("_arena_used", 0)          # the header rows the recorded step clears at its head (by value)
        with R.capture(st, st.side_stream().cuda_stream, aux.cuda_stream if aux is not None else 0) as cap:
            # The recorded step must carry the per-step weight split (segmm_wsplit_p32): ParamStore.refresh_planes skips it when the planes
            # are current -- which they are when an EVALUATION pass ran since the last optimizer step (it split the new weights itself).
            # A step recorded in that state would replay on stale weight planes for ever (found by fit(recorded=True): validation, then
            # record).  Force the split into the recording.
            st._planes_key = None
            out = self.train_step(batch)
        # the tensors of the batch and of the one before it: every recorded pointer that falls inside one of them is re-based per step
        r = R.finish(cap, (batch, prev))
        # host-side state of the eager path (id mode: the id list whose table-gradient rows the NEXT backward clears): kept current
        # by run_recorded, so that eager steps and recorded steps can be mixed.  A list that is a batch tensor is named by its key
        # (every replay leaves its own batch's); any other list is a persistent buffer the replays fill again (data parallel: the
        # gathered ids of DPComm.gather_rows) and is kept as the tensor itself -- a later eager step of another shape makes the
        # communicator allocate new buffers, the recording goes on using these
        tab_keys = []
        for ek, (gptr, t) in getattr(st, "_tab_rows", {}).items():
            k = next((k for k in r["spans"] if t.data_ptr() == batch[k].data_ptr()
                      and t.numel() * t.element_size() == batch[k].numel() * batch[k].element_size()), None)
            tab_keys.append((ek, gptr, k if k is not None else t))
        r.update(prev_batch=batch, tab_keys=tab_keys, out=out, hyper=self._hyper(), hdr_cleared=hdr_cleared, hdr_used=st._arena_used)
        self._recorded = r
        return out

    @staticmethod
    def _refuse_unrecordable(batch, who, what):
        """What a replay would drop, refused by name (``who``: the caller in the message; ``what``: "step" / "validation batch")."""
        for k, v in batch.items():
            if torch.is_tensor(v) and not v.is_contiguous():
                raise RuntimeError("%s: batch[%r] is not contiguous" % (who, k))
            # the zero-copy paths of the step: anything else is converted by a torch kernel, which a replay would drop (the
            # conversions also raise by themselves while recording: hipabi.torch_fallback)
            # (16-bit and 8-bit features: only the two tensors that go through normalize(); the recorded commands carry their element
            # type, and run_recorded() refuses a batch of another dtype.  int8 is a feature dtype there and nowhere else.)
            feat = k in ("user", "photo") and v.dtype in H.FEATURE_DTYPES if torch.is_tensor(v) else False
            if torch.is_tensor(v) and v.is_floating_point() and v.dtype != torch.float32 and not feat:
                raise RuntimeError("%s: batch[%r] is %s; the recorded %s takes float32 features (batch['user'] / batch['photo']: "
                                   "float32, float16 or bfloat16, or 8-bit: float8_e4m3fn, float8_e5m2 or int8)" % (who, k, v.dtype, what))
            if torch.is_tensor(v) and k.endswith("_mask") and v.dtype != torch.bool:
                raise RuntimeError("%s: batch[%r] is %s; the recorded %s takes bool masks" % (who, k, v.dtype, what))
            if torch.is_tensor(v) and not v.is_floating_point() and v.dtype not in (torch.bool, torch.int64) and not feat:
                raise RuntimeError("%s: batch[%r] is %s; the recorded %s takes int64 ids and labels" % (who, k, v.dtype, what))
        # one feature dtype per recorded batch: a batch that carries 16-bit or 8-bit features carries both tensors so (a pipeline stores
        # its features in one format); a half-precision tensor next to a float32 one is the stray conversion record() has always refused
        fdt = {k: batch[k].dtype for k in ("user", "photo")
               if torch.is_tensor(batch.get(k)) and (batch[k].is_floating_point() or batch[k].dtype == torch.int8)}
        if len(set(fdt.values())) > 1:
            raise RuntimeError("%s: batch['user'] is %s and batch['photo'] is %s; the recorded %s takes both feature tensors in "
                               "one dtype (float32, float16 or bfloat16, or one of the 8-bit dtypes)" % (who, fdt["user"], fdt["photo"], what))

    def _hyper(self):
        # under an lr_schedule the recorded commands carry the sentinel, not a rate: the rate may move, the schedule's presence not
        lr = self.opt.lr if self.opt.schedule is None else H.LIVE_LR
        # (the recorded segmm_ema_update carries the EMA's weight and warm-up flag by value)
        return (lr, self.opt.wd, tuple(self.opt.betas), self.opt.eps, self.opt.max_grad_norm, self.opt.group_table(),
                # (the recorded step carries the guard as its commands: segmm_step_guard and the *_guarded updates)
                self._guard,
                # (... and beside lazy tables the recorded *_ema launches stand for the key lazy_tables=dict(ema=True))
                None if self.ema is None else self.ema.hyper() + (bool(getattr(self.opt, "lazy_ema", False)),),
                # (the recorded plane GEMMs carry their product count in the command: segmm_gemm_p or segmm_gemm_pq(..., 1))
                None if self.mixed_precision is None else tuple(sorted(self.mixed_precision.items())))

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
        if self.opt.lazy_flush_every is not None:
            self.opt.lazy_step_head()          # the host's periodic flush, between two replays
        st = self.model._store
        # The recorded step clears the id-table gradients by the row list of the step before it: a lag-1 pointer into the previous
        # batch with the recorded count, or (data parallel) the recording's own gathered-id buffer.  Both are right only behind a
        # replay of this recording (or the recorded step itself).  Behind any other step -- an eager one, of whatever shape --
        # the rows that step left are cleared here, by its own list, ahead of the first phase; the lag-1 slots then name THIS
        # batch (the recorded shape), whose rows the recorded zero_rows finds clear already
        prev, before = r["prev_batch"], None
        if prev is None:
            prev, before = batch, functools.partial(self._after_foreign_step, st, r)
        # (a wrong current stream or a tensor of another shape behind a slot is refused before a slot is patched or anything is
        # enqueued: a refused call leaves the recording as it found it)
        R.replay(r, "run_recorded()", "step", batch, prev, timed, before=before)
        r["prev_batch"] = batch          # (also keeps the tensors a lag-1 pointer names alive until the next step has run)
        # mirror the host side effects of the eager step (FusedAdamW.begin_step / end_step; the id lists of the table rows this
        # step's backward scattered into -- exactly those the recorded step left, nothing of an earlier eager step)
        self.opt.step_count += 1
        st.fused_version += 1
        st._tab_rows = {ek: (gptr, batch[k].reshape(-1) if isinstance(k, str) else k) for ek, gptr, k in r["tab_keys"]}
        # (the site-header rows this step wrote: the next eager step clears what the step before it used, ParamStore.hdr_step_begin)
        st._arena_used = max(st._arena_used, r["hdr_used"])
        return r["out"]

    def _after_foreign_step(self, st, r):
        """Ahead of a replay that follows a step not of this recording: what the recorded step expects of the step before it, made so.
        The dense id-table gradients are cleared of what the last backward scattered into them, the way the next eager backward
        would (engine._embed_bwd): by the row list it left in ``st._tab_rows``, densely where it left none; the lists are used up.
        The site-header rows that step used beyond the ones the recorded step clears itself (a micro-batched step of more passes)
        are cleared too."""
        if st._arena_used > r["hdr_cleared"]:
            H.fill_zero(st._hdr_arena[r["hdr_cleared"]:st._arena_used])
        mods = dict(self.model.named_modules())
        for name in st.live_names:
            if name.endswith(("vid_proj.weight", "usr_proj.weight")) and isinstance(mods.get(name.rsplit(".", 1)[0]), torch.nn.Embedding):
                gtab = st.g(name)
                ent = st._tab_rows.pop(name[:-len("_proj.weight")], None)
                if ent is not None and ent[0] == gtab.data_ptr() and ent[1].device == gtab.device:
                    H.zero_rows(gtab, ent[1])
                else:
                    H.fill_zero(gtab)

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

    def fit(self, train_batches, valid_batches, epochs, **kw):
        """The reference's train / validate / checkpoint / early-stop loop (module-level :func:`fit`)."""
        return fit(self, train_batches, valid_batches, epochs, **kw)
