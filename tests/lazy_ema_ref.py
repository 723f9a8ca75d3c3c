"""The lazy exact AdamW protocol WITH the weight average (lazy_tables=dict(ema=True)) restated on the host in numpy float32:
``lazy_table_ref.LazyTable`` plus a shadow per row and the step's EMA weight w_t in the ring's fourth float (csrc/rowops.h
adamw_table_catchup_kernel<true> / adamw_table_lazy_rows_kernel<SCALED, true>).  Every AdamW element update is ``adamw_ref.emul32``'s, every
lerp ``ema_ref.lerp``'s, so the statement to check is again one of ORDER: a row that takes its g = 0 steps late takes the lerps of
those steps late too, each behind its own AdamW step and with its own step's weight, and then holds the bits of the shadow that
was averaged over the dense table after every step.

``dense_shadow`` is the yardstick (``lazy_table_ref.dense_run`` + ``ema_ref.replay``); ``LazyEmaTable`` the protocol -- head:
catch-up of the rank's own rows to T - 1; tail: the ring's entry of T with w_T, then every listed row not yet at T replays what it
still misses, takes step T with its gradient row and the lerp with w_T -- with planted ``DEFECTS``:
    lerp_first     the lerp of a step runs BEFORE its AdamW step (it averages p_{t-1})
    newest_w       replayed lerps take the newest ring entry's weight instead of their step's
    one_lerp       a replayed gap takes ONE lerp (its last step's) instead of one per step
    final_p        every lerp of a replayed gap averages the gap's FINAL p
    skip_T         step T's lerp is skipped for the listed rows
    dup_twice      an id listed twice takes step T's lerp twice
"""
import numpy as np

import ema_ref as E
import lazy_table_ref as L

F = np.float32
DEFECTS = ("lerp_first", "newest_w", "one_lerp", "final_p", "skip_T", "dup_twice")


def dense_shadow(p0, dense, decay, warmup=True, t0=0):
    """The shadow after every step of ``dense`` (= ``lazy_table_ref.dense_run``'s list), seeded with ``p0`` -> [shadow after step k]."""
    out, s = [], np.array(p0, dtype=F)
    for k, (p, _, _) in enumerate(dense):
        s = E.update(s, p, decay, t0 + k + 1, warmup)
        out.append(s)
    return out


class LazyEmaTable(L.LazyTable):
    def __init__(self, p0, m0, v0, flush_every, hp, decay, warmup=True, t0=0, lr_scale=1.0, defect=None):
        assert defect is None or defect in DEFECTS, defect
        super().__init__(p0, m0, v0, flush_every, hp, t0=t0, lr_scale=lr_scale)
        self.shadow = np.array(p0, dtype=F)          # seeded with the parameters before the first step
        self.decay, self.warmup, self.ema_defect = decay, warmup, defect
        self.wring = [F(0.0)] * self.cap          # the ring's fourth float: slot t % cap holds w_t
        self.newest_w = F(0.0)

    def _one(self, r, g, t, lr, w):
        """Step t of row r (g: its gradient row) and the step's lerp."""
        if self.ema_defect == "lerp_first":
            self.shadow[r] = E.lerp(self.shadow[r], self.p[r], w)
        self.p[r], self.m[r], self.v[r] = L.elem_step(self.p[r], self.m[r], self.v[r], g, max(t, 1), lr, self.hp, self.lr_scale)
        if self.ema_defect != "lerp_first":
            self.shadow[r] = E.lerp(self.shadow[r], self.p[r], w)

    def _replay(self, r, target):
        lo, hi = int(self.stamps[r]) + 1, target
        z = np.zeros_like(self.p[r])
        if self.ema_defect in ("one_lerp", "final_p"):
            ws = []
            for s in range(lo, hi + 1):
                lr, t = self.ring[s % self.cap]
                self.p[r], self.m[r], self.v[r] = L.elem_step(self.p[r], self.m[r], self.v[r], z, max(t, 1), lr, self.hp, self.lr_scale)
                ws.append(self.wring[s % self.cap])
            for w in (ws[-1:] if self.ema_defect == "one_lerp" else ws):
                self.shadow[r] = E.lerp(self.shadow[r], self.p[r], w)
            return
        for s in range(lo, hi + 1):
            lr, t = self.ring[s % self.cap]
            self._one(r, z, t, lr, self.newest_w if self.ema_defect == "newest_w" else self.wring[s % self.cap])

    def step(self, ids, g, lr, own_ids=None):
        """One optimizer step.  ``ids``: the step's rows (data parallel: all ranks'); ``own_ids`` (default ``ids``): the rows the
        head catches up; ``g`` the dense [rows, width] gradient."""
        if self.pending >= self.cap:
            self.flush()
        T = self.t + 1
        self.catchup(ids if own_ids is None else own_ids, T - 1)
        w = E.w_at(self.decay, T, self.warmup)
        self.ring[T % self.cap] = self.newest = (F(lr), T)
        self.wring[T % self.cap] = self.newest_w = w
        for r in ids:
            r = int(r)
            if not 0 <= r < self.rows:
                continue
            if self.stamps[r] >= T:          # a duplicate's second entry: the row was taken
                if self.ema_defect == "dup_twice":
                    self.shadow[r] = E.lerp(self.shadow[r], self.p[r], w)
                continue
            if self.stamps[r] < T - 1:          # (a row of another rank: the head did not list it)
                self._replay(r, T - 1)
            if self.ema_defect == "skip_T":
                self.p[r], self.m[r], self.v[r] = L.elem_step(self.p[r], self.m[r], self.v[r], g[r], T, lr, self.hp, self.lr_scale)
            else:
                self._one(r, g[r], T, lr, w)
            self.stamps[r] = T
        self.t = T
