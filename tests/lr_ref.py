"""The learning-rate schedule of the device step state restated on the host in float64: the yardstick of
tests/test_lr_schedule_cpu.py and tests/test_lr_schedule_gpu.py for ``segmm_lr_at`` (csrc/common.h), which segmm_step_advance,
segmm_step_set, segmm_step_schedule and segmm_step_set_base_lr evaluate, and for ``LRSchedule.lr_at`` (trainer.py).

With k the number of COMPLETED optimizer steps (torch's ``opt.step(); sched.step()`` loop: step t runs at k = t - 1),
W = warmup_steps, D = decay_steps, j = max(k - W, 0), r = eta_min / base_lr:

    lr(k) = base_lr * warm(k) * dec(j)
    warm(k) = start_factor + (1 - start_factor) k / W  for k < W,  else 1          (W = 0: no warm-up)
    constant  dec = 1
    cosine    dec = r + (1 - r) (1 + cos(pi min(j, D) / D)) / 2
    linear    dec = 1 - (1 - r) min(j, D) / D
    step      dec = gamma^floor(j / step_size)
    exp       dec = gamma^j

``abi_rounded=True`` rounds base_lr, start_factor, eta_min and gamma to float32 first -- the C ABI takes them as ``float``, so
that is the schedule the device is asked for (as ``adamw_ref.ref64`` does for AdamW's hyperparameters); ``False`` keeps the Python
doubles, which is what torch.optim.lr_scheduler implements.  ``torch_lrs`` is that implementation: LinearLR for the warm-up joined
by SequentialLR to ConstantLR(factor = 1) / CosineAnnealingLR / LinearLR / StepLR / ExponentialLR.
"""
import functools
import math
import warnings

import numpy as np
import torch

F = np.float32
KINDS = ("constant", "cosine", "linear", "step", "exp")


def lr_at(k, kind, base_lr, warmup_steps=0, start_factor=1.0, decay_steps=1, eta_min=0.0, gamma=1.0, step_size=1, abi_rounded=False):
    """lr after k completed steps, in float64 (a Python float)."""
    assert kind in KINDS, kind
    if abi_rounded:
        base_lr, start_factor, eta_min, gamma = (float(F(x)) for x in (base_lr, start_factor, eta_min, gamma))
    W, D = int(warmup_steps), int(decay_steps)
    warm = start_factor + (1.0 - start_factor) * k / W if (W > 0 and k < W) else 1.0
    j = max(k - W, 0)
    r = eta_min / base_lr
    if kind == "constant":
        dec = 1.0
    elif kind == "cosine":
        dec = r + (1.0 - r) * (1.0 + math.cos(math.pi * min(j, D) / D)) / 2.0
    elif kind == "linear":
        dec = 1.0 - (1.0 - r) * min(j, D) / D
    elif kind == "step":
        dec = gamma ** (j // int(step_size))
    else:
        dec = gamma ** j
    return base_lr * warm * dec


def lrs(n, **kw):
    """[lr(0), ..., lr(n - 1)]: the rates of optimizer steps 1 .. n."""
    return [lr_at(k, **kw) for k in range(n)]


def f32(x):
    return float(F(x))


def torch_scheduler(opt, kind, warmup_steps=0, start_factor=1.0, decay_steps=1, eta_min=0.0, gamma=1.0, step_size=1):
    """torch's scheduler for the schedule, on ``opt`` (whose lr is the base rate): call ``.step()`` after every ``opt.step()``."""
    S = torch.optim.lr_scheduler
    base_lr = opt.param_groups[0]["lr"]
    if kind == "constant":
        main = S.ConstantLR(opt, factor=1.0, total_iters=0)
    elif kind == "cosine":
        main = S.CosineAnnealingLR(opt, T_max=decay_steps, eta_min=eta_min)
    elif kind == "linear":
        main = S.LinearLR(opt, start_factor=1.0, end_factor=eta_min / base_lr, total_iters=decay_steps)
    elif kind == "step":
        main = S.StepLR(opt, step_size=step_size, gamma=gamma)
    else:
        main = S.ExponentialLR(opt, gamma=gamma)
    if warmup_steps > 0:
        warm = S.LinearLR(opt, start_factor=start_factor, end_factor=1.0, total_iters=warmup_steps)
        return S.SequentialLR(opt, [warm, main], milestones=[warmup_steps])
    return main


def torch_lrs(n, kind, base_lr, **kw):
    """The rates torch.optim.lr_scheduler gives optimizer steps 1 .. n (``opt.step(); sched.step()``), as Python floats."""
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=base_lr)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # (SequentialLR steps its members with the deprecated epoch argument)
        sched = torch_scheduler(opt, kind, **kw)
        out = []
        for _ in range(n):
            out.append(float(opt.param_groups[0]["lr"]))
            opt.step()
            sched.step()
    return out


# ------------------------------------------------------------------------------------------------ AdamW under a moving rate
# One sample shared by the CPU and the GPU test: regime ``unit`` of adamw_ref (g ~ N(0, 1), n = 4099, p0 = 0) for 40 steps under a
# cosine schedule with a warm-up, which covers the ramp, the decay and the hold at eta_min.
MOVING = dict(kind="cosine", base_lr=1e-3, warmup_steps=5, start_factor=0.1, decay_steps=30, eta_min=1e-5)
MOVING_STEPS = 40
MOVING_CHECKPOINTS = (1, 2, 3, 10, 40)


def chain(impl, lr_of, steps=MOVING_STEPS, **kw):
    """``impl`` (adamw_ref.ref64 / emul32) one step at a time over the first ``steps`` gradients of regime ``unit``, step t at the
    rate ``lr_of(t)``, each step started from the previous one's (p, m, v): {t: (p, m, v)} at MOVING_CHECKPOINTS."""
    import adamw_ref as A
    r = A.regime("unit")
    hp = {k: v for k, v in r["hp"].items() if k != "lr"}
    state, out = (r["p0"], None, None), {}
    for t in range(1, steps + 1):
        (state,) = impl(state[0], [r["grads"][t - 1]], lr=lr_of(t), m0=state[1], v0=state[2], t0=t - 1, **hp, **kw).values()
        if t in MOVING_CHECKPOINTS:
            out[t] = tuple(np.array(x) for x in state)
    return out


def torch_moving():
    """torch.optim.AdamW (CPU, fp32) with torch's scheduler for MOVING over the same gradients: {t: (p, m, v)}.  The scheduler is
    stepped up to the end of the decay (k = W + D, where it has reached eta_min) and left there: torch's CosineAnnealingLR would
    climb again (it is periodic), the schedule holds -- with the scheduler stepped on, torch's error against R_true at step 40
    would be the size of the rate itself and the yardstick there worthless."""
    import adamw_ref as A
    r = A.regime("unit")
    hp = r["hp"]
    P = torch.nn.Parameter(torch.from_numpy(np.array(r["p0"], dtype=F)))
    kw = {k: v for k, v in MOVING.items() if k not in ("kind", "base_lr")}
    opt = torch.optim.AdamW([P], lr=MOVING["base_lr"], betas=(hp["b1"], hp["b2"]), eps=hp["eps"], weight_decay=hp["wd"], foreach=False)
    out, hold = {}, MOVING["warmup_steps"] + MOVING["decay_steps"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sched = torch_scheduler(opt, MOVING["kind"], **kw)
        for t in range(1, MOVING_STEPS + 1):
            P.grad = torch.from_numpy(np.array(r["grads"][t - 1], dtype=F))
            opt.step()
            if t <= hold:
                sched.step()
            if t in MOVING_CHECKPOINTS:
                s = opt.state[P]
                out[t] = (P.detach().numpy().copy(), s["exp_avg"].numpy().copy(), s["exp_avg_sq"].numpy().copy())
    return out


class MovingYardstick:
    """R_abi (float64 at the fp32 rates the kernels are handed), R_true (float64 at the double rates torch is handed), torch's
    run and its errors against R_true: what an implementation's errors against R_abi may be adamw_ref.MARGIN times."""

    def __init__(self):
        import adamw_ref as A
        r = A.regime("unit")
        self.lr_abi = {t: f32(lr_at(t - 1, abi_rounded=True, **MOVING)) for t in range(1, MOVING_STEPS + 2)}
        self.r_abi = chain(A.ref64, lambda t: self.lr_abi[t], abi_rounded=True)
        self.r_true = chain(A.ref64, lambda t: lr_at(t - 1, **MOVING), abi_rounded=False)
        self.t32 = torch_moving()
        self.G = A.running_gmax(r["grads"][:MOVING_STEPS], MOVING_CHECKPOINTS)
        self.torch_err = {t: A.errors(self.t32[t], self.r_true[t], self.G[t]) for t in MOVING_CHECKPOINTS}

    def ratios(self, got, t):
        import adamw_ref as A
        mine = A.errors(got, self.r_abi[t], self.G[t])
        return tuple(a / b if b > 0 else (0.0 if a == 0 else math.inf) for a, b in zip(mine, self.torch_err[t]))


@functools.lru_cache(maxsize=None)
def moving_yardstick():
    return MovingYardstick()
