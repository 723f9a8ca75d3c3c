"""AdamW restated on the host (numpy and torch only): the yardstick of tests/test_adamw_cpu.py and tests/test_adamw_gpu.py for
``adamw_elem4`` (csrc/rowops.h), the one piece of arithmetic behind segmm_adamw, segmm_adamw_scaled, segmm_adamw_table (both phases)
and segmm_adamw_table_scaled, and for the bias corrections of the host (capi.hip adamw_flat) and of the device step state.

Three implementations of one step  p, m, v, g -> p', m', v'  at step count t, in torch's single-tensor order:

    p *= 1 - lr wd;   m = b1 m + (1 - b1) g;   v = b2 v + (1 - b2) g^2
    den = sqrt(v) / sqrt(1 - b2^t) + eps;      p -= lr / (1 - b1^t) * m / den

* ``ref64``: float64.  ``abi_rounded=True`` (R_abi) rounds lr, b1, b2, eps, wd to float32 first -- the C ABI takes them as
  ``float``, so that is the update the kernel is asked for; ``False`` (R_true) keeps the Python doubles, which is what torch
  implements.  In both the decay factor 1 - lr wd is the float32 number that reaches the multiplication (torch rounds the double
  1 - lr wd to the parameter's dtype, the kernel computes 1.0f - lr * wd): a property of fp32 storage, not of either side.
* ``torch32``: torch.optim.AdamW on the CPU in fp32 -- the optimizer the reference project runs, and the yardstick: a kernel is
  accepted when its error against R_abi is at most MARGIN x torch's own error against R_true in the same regime at the same step.
* ``emul32``: adamw_elem4 operation for operation in numpy float32 (every operation rounded, nothing contracted), bias
  corrections as the host computes them; ``mutant`` plants one of four defects.  test_adamw_cpu.py shows that the yardstick
  accepts the emulation and rejects every mutant, which is what keeps the GPU tests' margin honest.

Errors (``errors``): E_p = max |p - p_ref|, E_m = max |m - m_ref| / G, E_v = max |v - v_ref| / G^2 with G the element's running
maximum of |g| (m is a convex combination of the gradients seen so far and v one of their squares, so G and G^2 are their natural
scales whatever the gradient's magnitude).  Elements with G = 0 must hold m = v = 0 exactly.
"""
import functools
import math

import numpy as np
import torch

F = np.float32
MARGIN = 3.0
MUTANTS = ("eps_scaled", "bc2_no_sqrt", "wd_after", "bc_pow_fp32")
HP = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=1e-2)          # torch.optim.AdamW's defaults
N, T, ZEROS = 4099, 300, 64          # N is odd: the n & 3 tail runs; the first ZEROS elements of every gradient are zero
CHECKPOINTS = (1, 2, 3, 10, 100, 300)


def host_bc(b, t):
    """(bc, sqrt(bc)) as capi.hip computes them for step t >= 1: bc = 1 - double(float32(b))^t in double, each rounded to fp32 once."""
    bc = 1.0 - float(F(b)) ** int(t)
    return F(bc), F(math.sqrt(bc))


def decay_factor(lr, wd, abi_rounded):
    """The fp32 factor p is multiplied by: 1.0f - lr * wd in fp32 (kernel) / float32(1 - lr wd) computed in double (torch)."""
    if abi_rounded:
        return float(F(1.0) - F(F(lr) * F(wd)))
    return float(F(1.0 - lr * wd))


def ref64(p0, grads, lr, b1, b2, eps, wd, abi_rounded, checkpoints=None, m0=None, v0=None, t0=0):
    """float64 AdamW from (p0, m0, v0) at step count t0 over ``grads`` (an iterable of arrays): {t: (p, m, v)} at the requested
    absolute step counts (default: the last one)."""
    decay = decay_factor(lr, wd, abi_rounded)
    if abi_rounded:
        lr, b1, b2, eps = (float(F(x)) for x in (lr, b1, b2, eps))
    p = np.asarray(p0, dtype=np.float64).copy()
    m = np.zeros_like(p) if m0 is None else np.asarray(m0, dtype=np.float64).copy()
    v = np.zeros_like(p) if v0 is None else np.asarray(v0, dtype=np.float64).copy()
    out, t = {}, t0
    for g in grads:
        t += 1
        g = np.asarray(g, dtype=np.float64)
        with np.errstate(all="ignore"):
            p = p * decay
            m = m * b1 + g * (1.0 - b1)
            v = v * b2 + g * g * (1.0 - b2)
            den = np.sqrt(v) / math.sqrt(1.0 - b2 ** t) + eps
            p = p - (lr / (1.0 - b1 ** t)) * (m / den)
        if checkpoints is None or t in checkpoints:
            out[t] = (p.copy(), m.copy(), v.copy())
    return out if checkpoints is not None else {t: (p, m, v)}


def torch32(p0, grads, lr, b1, b2, eps, wd, checkpoints=None, m0=None, v0=None, t0=0):
    """torch.optim.AdamW (CPU, fp32, single-tensor) fed the same gradients: {t: (p, m, v)} as fp32 numpy arrays."""
    P = torch.nn.Parameter(torch.from_numpy(np.array(p0, dtype=F)))
    opt = torch.optim.AdamW([P], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
    if t0 or m0 is not None:
        opt.state[P] = {"step": torch.tensor(float(t0)),
                        "exp_avg": torch.zeros_like(P) if m0 is None else torch.from_numpy(np.array(m0, dtype=F)),
                        "exp_avg_sq": torch.zeros_like(P) if v0 is None else torch.from_numpy(np.array(v0, dtype=F))}
    out, t = {}, t0
    for g in grads:
        t += 1
        P.grad = torch.from_numpy(np.array(g, dtype=F))
        opt.step()
        if checkpoints is None or t in checkpoints:
            s = opt.state[P]
            out[t] = (P.detach().numpy().copy(), s["exp_avg"].numpy().copy(), s["exp_avg_sq"].numpy().copy())
    return out if checkpoints is not None else {t: out[t]}


def emul32(p0, grads, lr, b1, b2, eps, wd, checkpoints=None, m0=None, v0=None, t0=0, mutant=None):
    """adamw_elem4 in numpy float32, one rounding per operation, host bias corrections.  Mutants: ``eps_scaled``
    (sqrt(v) + eps) / bc2_sqrt; ``bc2_no_sqrt`` divides by bc2 instead of its root; ``wd_after`` decays after the update;
    ``bc_pow_fp32`` takes the bias corrections from fp32 powf."""
    assert mutant is None or mutant in MUTANTS, mutant
    p = np.array(p0, dtype=F)
    m = np.zeros_like(p) if m0 is None else np.array(m0, dtype=F)
    v = np.zeros_like(p) if v0 is None else np.array(v0, dtype=F)
    lr, b1, b2, eps, wd = F(lr), F(b1), F(b2), F(eps), F(wd)
    one = F(1.0)
    decay = one - lr * wd
    out, t = {}, t0
    for g in grads:
        t += 1
        g = np.asarray(g, dtype=F)
        bc1, bc2s = host_bc(b1, t)[0], host_bc(b2, t)[1]
        if mutant == "bc2_no_sqrt":
            bc2s = F(1.0 - float(b2) ** t)
        elif mutant == "bc_pow_fp32":
            bc1 = one - np.power(b1, F(t))
            bc2s = np.sqrt(one - np.power(b2, F(t)))
        step = lr / bc1
        with np.errstate(all="ignore"):
            if mutant != "wd_after":
                p = p * decay
            m = m + (g - m) * (one - b1)
            v = v * b2 + g * (one - b2) * g
            den = (np.sqrt(v) + eps) / bc2s if mutant == "eps_scaled" else np.sqrt(v) / bc2s + eps
            p = p - step * (m / den)
            if mutant == "wd_after":
                p = p * decay
        assert p.dtype == m.dtype == v.dtype == F and type(step) is F
        if checkpoints is None or t in checkpoints:
            out[t] = (p.copy(), m.copy(), v.copy())
    return out if checkpoints is not None else {t: out[t]}


def running_gmax(grads, checkpoints=None, G0=None):
    """{t: G}: per element the largest |g| seen up to step t (steps counted from 1 over ``grads``; G0: what earlier steps saw)."""
    G, out, t = None if G0 is None else np.asarray(G0, dtype=np.float64).copy(), {}, 0
    for g in grads:
        t += 1
        a = np.abs(np.asarray(g, dtype=np.float64))
        G = a if G is None else np.maximum(G, a)
        if checkpoints is None or t in checkpoints:
            out[t] = G.copy()
    return out


def state_gmax(m0, v0):
    """The smallest G a given state is consistent with: |m| <= G and v <= G^2 for moments that are convex combinations."""
    return np.maximum(np.abs(np.asarray(m0, dtype=np.float64)), np.sqrt(np.asarray(v0, dtype=np.float64)))


def errors(got, ref, G):
    """(E_p, E_m, E_v) of a (p, m, v) triple against a float64 one; asserts m = v = 0 exactly where G = 0."""
    p, m, v = (np.asarray(x, dtype=np.float64) for x in got)
    rp, rm, rv = ref
    G = np.asarray(G, dtype=np.float64)
    dead = G == 0
    assert not m[dead].any() and not v[dead].any(), "m, v must stay exactly 0 where every gradient was 0"
    assert not rm[dead].any() and not rv[dead].any()
    live = ~dead
    Gl = G[live]
    e_p = float(np.max(np.abs(p - rp))) if p.size else 0.0
    e_m = float(np.max(np.abs(m[live] - rm[live]) / Gl)) if live.any() else 0.0
    e_v = float(np.max(np.abs(v[live] - rv[live]) / Gl / Gl)) if live.any() else 0.0
    return e_p, e_m, e_v


# ------------------------------------------------------------------------------------------------ regimes
REGIMES = ("unit", "eps", "decades", "decay", "betas_fast", "betas_slow", "late")
LATE_T0, LATE_STEPS = 5000, 20


def _normal_grads(rng, n, T, scale):
    out = []
    for _ in range(T):
        g = (rng.standard_normal(n).astype(F) * scale).astype(F)
        g[:ZEROS] = 0
        out.append(g)
    return out


@functools.lru_cache(maxsize=None)
def regime(name, n=N, T=T, seed=0):
    """dict(hp, p0, m0, v0, t0, G0, grads, checkpoints) of one regime (built once, read-only).  p0 = 0 unless stated, so that p IS
    the accumulated update and the fp32 rounding of a parameter of size 1 cannot hide it.
    unit g ~ N(0, 1);  eps g ~ 3e-9 N(0, 1) (sqrt(v) comparable with eps);  decades: per-element scale 10^U(-12, 3);
    decay wd = 0.1, lr = 1e-2, p0 ~ 1e-2 N(0, 1);  betas_fast (0.8, 0.99), betas_slow (0.95, 0.9999), both wd = 0;
    late: the R_abi state after 5000 steps of g ~ N(0, 1), rounded to fp32, then 20 more steps (bias corrections near 1)."""
    rng = np.random.default_rng([seed, REGIMES.index(name)])
    hp = dict(HP)
    r = dict(hp=hp, p0=np.zeros(n, dtype=F), m0=None, v0=None, t0=0, G0=None, checkpoints=tuple(t for t in CHECKPOINTS if t < T) + (T,))
    scale, steps = F(1.0), T
    if name == "eps":
        scale = F(3e-9)
    elif name == "decades":
        scale = (10.0 ** rng.uniform(-12, 3, size=n)).astype(F)
    elif name == "decay":
        hp.update(wd=0.1, lr=1e-2)
        r["p0"] = (1e-2 * rng.standard_normal(n)).astype(F)
    elif name == "betas_fast":
        hp.update(b1=0.8, b2=0.99, wd=0.0)
    elif name == "betas_slow":
        hp.update(b1=0.95, b2=0.9999, wd=0.0)
    elif name == "late":
        G0 = np.zeros(n)

        def early():
            for _ in range(LATE_T0):
                g = rng.standard_normal(n).astype(F)
                g[:ZEROS] = 0
                np.maximum(G0, np.abs(g), out=G0)
                yield g
        (p, m, v), = ref64(r["p0"], early(), abi_rounded=True, **hp).values()
        r.update(p0=p.astype(F), m0=m.astype(F), v0=v.astype(F), t0=LATE_T0, G0=G0)
        r["checkpoints"] = tuple(LATE_T0 + t for t in (1, 2, 3, 10, LATE_STEPS))
        steps = LATE_STEPS
    r["grads"] = tuple(_normal_grads(rng, n, steps, scale))
    for x in (r["p0"], r["m0"], r["v0"], r["G0"]) + r["grads"]:
        if x is not None:
            x.setflags(write=False)
    return r


def run(r, impl, **kw):
    """``impl`` (ref64 / torch32 / emul32) on regime dict ``r``: {absolute step: (p, m, v)} at its checkpoints."""
    return impl(r["p0"], r["grads"], checkpoints=r["checkpoints"], m0=r["m0"], v0=r["v0"], t0=r["t0"], **r["hp"], **kw)


class Yardstick:
    """R_abi, R_true, torch32 and G of a regime dict at its checkpoints, and ``torch_err[t]`` = (E_p, E_m, E_v) of torch32 against
    R_true: what an implementation's error against R_abi may be MARGIN times."""

    def __init__(self, r):
        self.r_abi, self.r_true, self.t32 = run(r, ref64, abi_rounded=True), run(r, ref64, abi_rounded=False), run(r, torch32)
        self.G = {r["t0"] + t: G for t, G in running_gmax(r["grads"], None, r["G0"]).items() if r["t0"] + t in r["checkpoints"]}
        self.torch_err = {t: errors(self.t32[t], self.r_true[t], self.G[t]) for t in r["checkpoints"]}

    def ratios(self, got, t, n=None):
        """(E_p, E_m, E_v) of ``got`` against R_abi at step t, each divided by torch's own error against R_true.  ``n``: ``got``
        covers the first n elements only (torch's error is still the whole sample's: it measures the regime, not the subset)."""
        mine = errors(got, tuple(x[:n] for x in self.r_abi[t]), self.G[t][:n])
        return tuple(a / b if b > 0 else (0.0 if a == 0 else math.inf) for a, b in zip(mine, self.torch_err[t]))


@functools.lru_cache(maxsize=None)
def yardstick(name):
    return Yardstick(regime(name))
