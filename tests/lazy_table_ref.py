"""The lazy exact AdamW protocol of an id-embedding table restated on the host in numpy float32: per-row step stamps, the ring of the
last ``cap`` steps' scalars, the catch-up of the batch's rows at the head of a step, phase 1 and the stamp at its tail, the flush
and the periodic flush (csrc/rowops.h adamw_table_catchup_kernel, optim.FusedAdamW(lazy_tables=...)).  Every element update is
``adamw_ref.emul32``'s -- adamw_elem4 operation for operation -- so the statement to check is purely one of ORDER: a row that takes
its g = 0 steps late, from the ring, holds the bits of the row that took them on time.

``dense_run`` is the yardstick (the whole table every step); ``LazyTable`` the protocol, with planted ``DEFECTS``:
    start_early / start_late   the replay begins at stamp / stamp + 2 instead of stamp + 1
    end_early / end_late       the replay ends at target - 1 / target + 1
    current_rate / current_bc  replayed steps take the newest ring entry's rate / bias corrections
    no_decay                   replayed steps drop the weight decay
    dup_twice                  an id listed twice takes phase 1 twice
    stale_slot                 the periodic flush comes one step late: it reads a ring slot that was overwritten
"""
import numpy as np

import adamw_ref as A

F = np.float32
DEFECTS = ("start_early", "start_late", "end_early", "end_late", "current_rate", "current_bc", "no_decay", "dup_twice", "stale_slot")


def elem_step(p, m, v, g, t, lr, hp, lr_scale=1.0):
    """One adamw_elem4 step at step count t (host bias corrections) at the rate fp32(lr * lr_scale) -> (p, m, v)."""
    (out,) = A.emul32(p, [g], F(lr) * F(lr_scale), hp["b1"], hp["b2"], hp["eps"], hp["wd"], m0=m, v0=v, t0=t - 1).values()
    return out


def dense_run(p0, m0, v0, grads, rates, hp, t0=0, lr_scale=1.0):
    """The dense update: every element steps every step.  ``grads``: one [rows, width] array per step -> [(p, m, v) after each step]."""
    p, m, v = (np.array(x, dtype=F) for x in (p0, m0, v0))
    out = []
    for k, (g, lr) in enumerate(zip(grads, rates)):
        p, m, v = elem_step(p, m, v, g, t0 + k + 1, lr, hp, lr_scale)
        out.append((p, m, v))
    return out


def dense_grad(g, ids, rows):
    """``g`` with every row that ``ids`` does not list (ids outside [0, rows) list nothing) set to zero: what the backward delivers."""
    ids = np.asarray(ids, dtype=np.int64)
    keep = np.zeros(rows, dtype=bool)
    keep[ids[(ids >= 0) & (ids < rows)]] = True
    return np.where(keep[:, None], g, F(0.0)).astype(F)


class LazyTable:
    def __init__(self, p0, m0, v0, flush_every, hp, t0=0, lr_scale=1.0, defect=None):
        assert defect is None or defect in DEFECTS, defect
        self.p, self.m, self.v = (np.array(x, dtype=F) for x in (p0, m0, v0))
        self.rows = self.p.shape[0]
        self.cap, self.hp, self.lr_scale, self.defect = int(flush_every), dict(hp), lr_scale, defect
        self.t = self.flushed = int(t0)
        self.stamps = np.full(self.rows, t0, dtype=np.int32)
        self.ring = [(F(0.0), 0)] * self.cap          # slot t % cap: (rate, the step count whose bias corrections it holds)
        self.newest = (F(0.0), 0)
        self.n_flushes = 0

    def _replay(self, r, target):
        lo, hi = int(self.stamps[r]) + 1, target
        lo += {"start_early": -1, "start_late": 1}.get(self.defect, 0)
        hi += {"end_early": -1, "end_late": 1}.get(self.defect, 0)
        hp = dict(self.hp, wd=0.0) if self.defect == "no_decay" else self.hp
        z = np.zeros_like(self.p[r])
        for s in range(lo, hi + 1):
            lr, t = self.ring[s % self.cap]
            if self.defect == "current_rate":
                lr = self.newest[0]
            if self.defect == "current_bc":
                t = self.newest[1]
            self.p[r], self.m[r], self.v[r] = elem_step(self.p[r], self.m[r], self.v[r], z, max(t, 1), lr, hp, self.lr_scale)

    def catchup(self, ids, target):
        """Rows behind ``target`` replay stamp + 1 .. target; a row at the target (a duplicate's second entry too) is left alone."""
        for r in (range(self.rows) if ids is None else ids):
            if 0 <= r < self.rows and self.stamps[r] < target:
                self._replay(int(r), target)
                self.stamps[r] = target

    def flush(self):
        if self.t > self.flushed:
            self.catchup(None, self.t)
            self.flushed = self.t
            self.n_flushes += 1

    @property
    def pending(self):
        return self.t - self.flushed

    def step(self, ids, g, lr):
        """One optimizer step: ``ids`` the batch's rows (duplicates, ids out of range), ``g`` the dense [rows, width] gradient."""
        if self.pending >= self.cap + (1 if self.defect == "stale_slot" else 0):
            self.flush()
        T = self.t + 1
        self.catchup(ids, T - 1)
        self.ring[T % self.cap] = self.newest = (F(lr), T)
        done = set()
        for r in ids:
            r = int(r)
            if not 0 <= r < self.rows or (r in done and self.defect != "dup_twice"):
                continue
            done.add(r)
            self.p[r], self.m[r], self.v[r] = elem_step(self.p[r], self.m[r], self.v[r], g[r], T, lr, self.hp, self.lr_scale)
            self.stamps[r] = T
        self.t = T
