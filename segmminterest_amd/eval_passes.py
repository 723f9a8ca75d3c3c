"""The evaluation entry points of the trainer: the test phase, the logit dump and the validation passes, eager or recorded.
``EvalPasses`` is the base class ``Trainer`` inherits them from; it uses nothing but the trainer's own attributes."""
from __future__ import annotations

import contextlib
from typing import Optional

import torch

from . import engine as E
from . import hipabi as H
from . import recording as R
from .loop import compute_final_result


class EvalPasses:
    """Evaluation passes over the model, the optimizer, the EMA, the communicator and the input stage of a :class:`trainer.Trainer`
    (``self.model``, ``opt``, ``ema``, ``comm``, ``_features``, ``_refuse_unrecordable``)."""

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
        self.opt.flush_tables()          # lazy tables: every row current before weights are read (or replaced by the checkpoint's)
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

    @torch.no_grad()
    def eval_step(self, batch, mode="inference"):
        model = self.model
        model.eval()
        self.opt.flush_tables()          # lazy tables: the forward reads every listed row as the dense run holds it (nothing pending: no launch)
        usr, um, vid, vm = self._features(batch)
        return model(usr_image=usr, usr_id=batch["user_identity_id"], usr_mask=um, vid_image=vid,
                     vid_id=batch["photo_identity_id"], vid_mask=vm, gt=batch["label"], mode=mode)

    @torch.no_grad()
    def dump_logits(self, splits, store=None, ema: bool = False, recorded: bool = False):
        """The dump loop of the reference's inference script (inference/save_logits_for_all_leave_SegMM.py:105-146): eval mode,
        ``mode="inference"`` over every batch of every split in order, ``test_logits["<user_id>-<photo_id>-<time_ms>"] = logits`` --
        into a :class:`bridge.DeviceLogitStore`, so the logits stay on the device and no batch synchronises with the host.  ``splits``:
        an iterable of batch iterables (train, valid, test; ``DeviceBatches`` yields the three key columns on the device).
        ``ema=True`` (needs ``Trainer(ema=...)``): the logits of the averaged weights (``ema.applied()``).
        ``recorded=True`` (opt-in; single process): the inference forward is replayed from one recorded launch sequence and every
        batch ends in ONE ``segmm_store_append`` into a preallocated store (:meth:`_dump_recorded`); the same keys and values, bit
        for bit."""
        from .bridge import DeviceLogitStore
        if recorded:
            with self._ema_scope(ema, "dump_logits"):
                return self._dump_recorded(splits, store)
        with self._ema_scope(ema, "dump_logits"):
            self.opt.flush_tables()          # lazy tables: every row current before the forward reads them
            for batches in splits:
                for batch in batches:
                    logits = self.eval_step(batch, mode="inference")["logits"]
                    if store is None:
                        store = DeviceLogitStore(S=logits.shape[1], device=logits.device)
                    store.add_batch(batch["user_id"], batch["photo_id"], batch["time_ms"], logits)
        if store is None:
            store = DeviceLogitStore(device=next(self.model.parameters()).device)
        return store

    # ---- a logit dump whose batches are replayed from C (recorded inference forward + ONE segmm_store_append)
    _DUMP_WHO = "dump_logits(recorded=True)"
    _DUMP_KEYS = ("user_id", "photo_id", "time_ms")

    def _dump_refuse(self, batch):
        """What the recorded dump cannot take of a batch, refused by name before anything of it is enqueued."""
        self._refuse_unrecordable(batch, self._DUMP_WHO, "dump batch")
        dev = next(self.model.parameters()).device
        for k in self._DUMP_KEYS:
            v = batch.get(k)
            if not torch.is_tensor(v) or v.device != dev or v.dtype != torch.int64 or v.dim() != 1 or v.shape[0] != batch["label"].shape[0]:
                got = "missing" if v is None else ("%s %s on %s" % (tuple(v.shape), v.dtype, v.device) if torch.is_tensor(v) else type(v).__name__)
                raise RuntimeError("%s: batch[%r] is %s; the store's writer reads the three key columns (user_id, photo_id, time_ms) as int64 "
                                   "[B] tensors on %s (DeviceBatches yields them so); use recorded=False" % (self._DUMP_WHO, k, got, dev))

    def _dump_recorded(self, splits, store):
        """The batch loop of ``dump_logits(recorded=True)``, after :meth:`valid_enqueue`: lazy tables are flushed and the weight planes
        split (``ParamStore.ensure``) ahead of the pass; the FIRST batch of a shape runs launch by launch while it is recorded
        (``recording.capture``, a private memory pool and a private header arena: the recording lives beside the validation recording
        and a recorded training step), its tail ONE ``segmm_store_append``; every later batch of that shape, in this and in later
        calls, is replayed with one C call per phase.  Per replay the append command's ``row0`` / ``capacity`` / ``keys`` / ``vals``
        are rewritten by name (the store's tables may have grown in between) and the batch's feature, mask, id and key-column
        pointers are re-based by the recorder.  A batch of another shape (the short last batch of a split) takes the eager forward
        with the same append tail.  The evaluation forward keeps three GEMM products whatever ``mixed_precision`` says.
        Refused by name: data parallelism (an active ``DPComm``), batches the recorder cannot take, a batch without the three key
        columns on the device, a learnable position bias (its inference head adds the bias with torch kernels).
        The recording keeps the input-stage buffers of the recorded batch alive (``held``): the trainer replaces them when a batch
        of another shape is normalised, and a replay must never write memory that has gone back to the allocator."""
        from .bridge import DeviceLogitStore
        who = self._DUMP_WHO
        if self.comm.active:
            raise RuntimeError("%s is not supported under data parallelism (an active DPComm): every rank would record and fill a store "
                               "of its own rows; use recorded=False" % who)
        model, st = self.model, self.model._store
        if getattr(model, "bias_weight", None) is not None:
            raise RuntimeError("%s: the model has a learnable position bias, which the inference head adds with torch kernels a replay would "
                               "drop; use recorded=False" % who)
        self.opt.flush_tables()          # lazy tables: flushed ahead of the pass, never inside its recording
        model.eval()
        dev = next(model.parameters()).device
        ensured = False
        for batches in splits:
            for batch in batches:
                self._dump_refuse(batch)
                B, S = batch["label"].shape
                if store is None:
                    store = DeviceLogitStore(S=S, device=dev, capacity=max(4 * B, 1024))
                elif store.capacity is None:
                    store.reserve(len(store) + max(4 * B, 1024))
                if store.S != S:
                    raise ValueError("logits have %d segments, store expects %d" % (S, store.S))
                if not ensured:          # the weights of the moment: their planes are split here, ahead of the pass's first replay
                    st.ensure()
                    ensured = True
                self._pf = None          # (like eval_step: a prefetched input stage is dropped)
                store._room(B)           # growth happens here, on the stream, never inside the recording
                r = self.__dict__.get("_dump_rec")
                if r is None:
                    self._dump_record(batch, store)
                elif R.batch_shapes(batch) == r["spans"]:
                    self._dump_replay(r, batch, store)
                else:
                    self._dump_tail(batch, self.eval_step(batch, mode="inference")["logits"], store)
        if store is None:
            store = DeviceLogitStore(device=dev)
        return store

    def _dump_tail(self, batch, logits, store):
        """The device tail of a dump batch: ONE segmm_store_append at the store's row count.  No synchronisation."""
        H.mark(H.PHASE_STEP_TAIL)
        store.append(batch["user_id"], batch["photo_id"], batch["time_ms"], logits)

    def _dump_record(self, batch, store):
        """Runs a dump batch launch by launch while recording it (see :meth:`_dump_recorded`)."""
        st = self.model._store
        side, aux = st.side_stream(), st.aux_stream()          # both exist before the recorder maps their handles to slots
        hold = self.__dict__.setdefault("_dump_hdr", {})
        with R.capture(st, side.cuda_stream, aux.cuda_stream) as cap, st.hdr_private_arena(hold) as arena:
            H.mark(H.PHASE_STEP_BEGIN)
            H.fill_zero(arena[:1])          # (the arena is clean now; the replays clear what this batch drew: size patched below)
            logits = self.eval_step(batch, mode="inference")["logits"]
            self._dump_tail(batch, logits, store)
        # What the recorded commands name must outlive the recording.  The trainer's normalised-feature buffers and their planes are
        # kept per (input, slot) and REPLACED when a batch of another shape comes by (Trainer.normalize / _input_act): the short last
        # batch of a split would free the buffers every replay writes, and the store's next table would be allocated over them.
        held = (logits, dict(self.__dict__.get("_norm") or {}), dict(self.__dict__.get("_norm_planes") or {}))
        r = R.finish(cap, (batch,))
        ops = H.op_ids()
        launches = [(ph, arr) for ph, arr in r["phases"] if arr is not None]
        head, tail = launches[0], launches[-1]
        fill = head[1][0]
        appends = [arr[ci] for ph, arr in launches for ci in range(ph.n_cmds) if arr[ci].op == ops["segmm_store_append"]]
        if (fill.op != ops["segmm_fill_zero"] or tail[0].kind != H.PHASE_STEP_TAIL or tail[0].n_cmds != 1 or len(appends) != 1
                or tail[1][0].op != ops["segmm_store_append"]):
            raise RuntimeError("%s: the recorded launch sequence does not have the expected head (header fill) and tail (one "
                               "segmm_store_append)" % self._DUMP_WHO)
        H.cmd_set_arg(fill, "segmm_fill_zero", "bytes", hold["used"] * H.SITE_FLOATS * 4)
        r.update(append=appends[0], n_replays=0, held=held)
        self._dump_rec = r

    def _dump_replay(self, r, batch, store):
        """Enqueues a dump batch from the recorded launch sequence: the append command's per-batch slots and the batch's addresses are
        patched, then one C call per phase; the store's row count moves on the host."""
        B = batch["label"].shape[0]
        ap = r["append"]          # (slots that every replay rewrites: setting them ahead of a refused replay changes nothing)
        H.cmd_set_arg(ap, "segmm_store_append", "row0", store._n)
        H.cmd_set_arg(ap, "segmm_store_append", "capacity", store._ktab.shape[0])
        H.cmd_set_arg(ap, "segmm_store_append", "keys", store._ktab.data_ptr())
        H.cmd_set_arg(ap, "segmm_store_append", "vals", store._vtab.data_ptr())
        R.replay(r, self._DUMP_WHO, "dump batch", batch)
        store._n += B
        store._index = None
        r["n_replays"] += 1

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
        self.opt.flush_tables()          # lazy tables: every row current before the forward reads them (nothing pending: no launch)
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
        self.opt.flush_tables()          # lazy tables: flushed ahead of the pass, never inside its recording
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
            elif r["cfg"] == cfg and R.batch_shapes(batch) == r["spans"]:
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
        with R.capture(st, side.cuda_stream, aux.cuda_stream) as cap, st.hdr_private_arena(hold) as arena:
            H.mark(H.PHASE_STEP_BEGIN)
            H.fill_zero(arena[:1])          # (the arena is clean now; the replays clear what this batch drew: size patched below)
            out = self.eval_step(batch, mode="train")
            self._valid_tail(out, acc, i, cfg, seed)
        # the batch's tensors: every recorded POINTER argument that falls inside one of them is re-based per replay (see record())
        r = R.finish(cap, (batch,))
        ops = H.op_ids()
        launches = [(ph, arr) for ph, arr in r["phases"] if arr is not None]
        head, tail = launches[0], launches[-1]
        named = {n: [tail[1][ci] for ci in range(tail[0].n_cmds) if tail[1][ci].op == ops[n]] for n in ("segmm_valid_rows", "segmm_copy_bytes")}
        fill = head[1][0]
        if (fill.op != ops["segmm_fill_zero"] or tail[0].kind != H.PHASE_STEP_TAIL or len(named["segmm_valid_rows"]) != 1
                or len(named["segmm_copy_bytes"]) != 2):
            raise RuntimeError("valid_model(recorded=True): the recorded launch sequence does not have the expected head (header fill) "
                               "and tail (segmm_valid_rows, two segmm_copy_bytes)")
        H.cmd_set_arg(fill, "segmm_fill_zero", "bytes", hold["used"] * H.SITE_FLOATS * 4)
        r.update(out=out, cfg=cfg, valid_rows=named["segmm_valid_rows"][0], copies=named["segmm_copy_bytes"], losses=model.__dict__["_losses_vec"],
                 n_replays=0)
        self._valid_rec = r
        return out

    def _valid_replay(self, r, batch, acc, i, seed):
        """Enqueues validation batch ``i`` from the recorded launch sequence: the per-batch slots of the tail and the batch's addresses
        are patched, then one C call per phase.  Returns the recording's output dict (rewritten by every replay)."""
        vr = r["valid_rows"]          # (slots that every replay rewrites: setting them ahead of a refused replay changes nothing)
        H.cmd_set_arg(vr, "segmm_valid_rows", "ranks", acc.rank_slice(i).data_ptr())
        H.cmd_set_arg(vr, "segmm_valid_rows", "row0", acc.offsets[i])
        H.cmd_set_arg(vr, "segmm_valid_rows", "seed", seed)
        dst = acc.scalars[i].data_ptr()
        H.cmd_set_arg(r["copies"][0], "segmm_copy_bytes", "dst", dst)
        H.cmd_set_arg(r["copies"][1], "segmm_copy_bytes", "dst", dst + 4 * acc.TOTAL)
        R.replay(r, "valid_model(recorded=True)", "validation batch", batch)
        r["n_replays"] += 1
        return r["out"]
