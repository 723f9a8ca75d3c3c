"""The epoch loop around the training step: ``fit`` (train / validate / checkpoint / early stop, as the reference trainer's
main loop), its early-stop tests and final-result means, and the ``CheckPointer`` file format."""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from .optim import PlateauLR
from .recording import batch_shapes


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
    batch of an epoch) takes the eager step.  Every batch is still stepped on exactly once, in order.  The replay that follows
    such an eager step clears what that step left for its successor (id mode: the table-gradient rows it scattered into) by that
    step's own row list, single process or data parallel: image mode and id mode end bit-identical to ``recorded=False``.
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

    def step(batch, prev, n_done):
        """One optimisation step on ``batch``: eager, recording, or from the recording."""
        if not recorded:
            return trainer.train_step(batch)
        r = trainer.__dict__.get("_recorded")
        if r is not None:
            if batch_shapes(batch) == r["spans"] and all(v.is_contiguous() for v in batch.values() if torch.is_tensor(v)):
                return trainer.run_recorded(batch)
            return trainer.train_step(batch)
        if n_done >= eager_steps and prev is not None and batch_shapes(prev) == batch_shapes(batch):
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
                    if getattr(trainer.opt, "skip_nonfinite", False):         # (one read-back, where the validation has synchronised already)
                        log("Skipped_steps: %d (non-finite gradient norm), Global_step: %d" % (trainer.opt.skipped_steps, global_step))
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
        if hasattr(optimizer, "flush_tables"):
            optimizer.flush_tables()          # lazy id tables: the weights saved below are the dense run's
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
