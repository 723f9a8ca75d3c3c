"""The reference of a step under the non-finite guard (FusedAdamW(skip_nonfinite=True)).

A guarded step is decided by ONE number, the global 2-norm of the live, non-frozen gradient: NaN or +-inf skips the step, and a
skipped step is the identity on (p, m, v) and on the EMA shadow.  An applied step is ``adamw_ref.emul32``'s update -- adamw_elem4
operation for operation -- with the bias corrections of the APPLIED index (attempted steps minus skipped ones, torch's
``state["step"]``), while the scheduled rate and the EMA warm-up follow the attempted count."""
import math

import numpy as np

import adamw_ref as A

F = np.float32


def verdict(g, frozen=None):
    """1 if the step on gradient ``g`` is skipped: the norm (sum of squares in float64, which fp32 squares cannot overflow) of the
    elements outside ``frozen`` (a bool mask, or None) is NaN or inf -- i.e. one of those elements is."""
    g = np.asarray(g, dtype=np.float64)
    if frozen is not None:
        g = g[~np.asarray(frozen, dtype=bool)]
    with np.errstate(all="ignore"):
        norm = math.sqrt(float(np.sum(g * g)))
    return int(not math.isfinite(norm))


def step(p, m, v, g, applied, lr, b1, b2, eps, wd, frozen=None):
    """One guarded step from (p, m, v), ``applied`` steps applied so far: -> (p, m, v, skipped).  Skipped: the arrays themselves
    (the identity).  Applied: emul32 with the corrections of index applied + 1; frozen elements keep their bits."""
    if verdict(g, frozen):
        return p, m, v, 1
    (out,) = A.emul32(p, [g], lr, b1, b2, eps, wd, m0=m, v0=v, t0=applied).values()
    if frozen is not None:
        fz = np.asarray(frozen, dtype=bool)
        out = tuple(np.where(fz, old, new) for old, new in zip((p, m, v), out))
    return out + (0,)


def run(p, m, v, grads, lr, b1, b2, eps, wd, t0=0, skipped0=0):
    """``grads`` one after the other, ``lr`` a float or a function of the ATTEMPTED step number t (1-based): ->
    (p, m, v, attempted, skipped)."""
    t, skipped = t0, skipped0
    for g in grads:
        t += 1
        rate = lr(t) if callable(lr) else lr
        p, m, v, s = step(p, m, v, g, t - 1 - skipped, rate, b1, b2, eps, wd)
        skipped += s
    return p, m, v, t, skipped


def corrections(t, skipped, b1, b2):
    """(bc1, bc2_sqrt) of attempted step ``t`` with ``skipped`` steps skipped before it: segmm_step_set's at t - skipped."""
    return A.host_bc(b1, t - skipped)[0], A.host_bc(b2, t - skipped)[1]
