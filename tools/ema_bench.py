#!/usr/bin/env python
"""What the weight average costs (Trainer(ema=...)), measured on the GPU; writes nothing but its standard output
(profiles/ema/kernel_bench.txt and step_bench.txt are this tool's output, see profiles/README.md).

``--what kernel``: segmm_ema_update alone against segmm_vec_add in its ``acc <- acc + g`` form (both move 12 bytes per element) and
segmm_vec_swap (16), at n = the config-2 model's live parameter count and at 4 n.  Alternating windows in ONE process: a window is
``--reps`` launches of one kernel between two device events; ``--windows`` rounds over the kernels.  Per kernel: the median window's us
per launch and the window-to-window spread (max - min).  The update runs under both cache policies (knob EMA_NT: 1 the shadow
nontemporal, 0 everything with the default policy).  Condition: median(ema_update, the library's default policy) <= median(vec_add) +
2 x spread(vec_add).

``--what step``: the recorded training step with and without the EMA, two trainers in ONE process (same model, same batches), both
warmed up and recorded, then alternating windows of ``--steps`` run_recorded() calls between two device synchronisations, timed with
the host clock: plain, EMA under EMA_NT=1, EMA under EMA_NT=0 (the knob is read when the recorded command is dispatched).

    cfg2   BASELINE config 2's model (image mode, B = 512): condition added time <= the kernel alone at n_live + the plain step's spread
    cfg3   BASELINE config 3's model (id mode, B = 256, a 90 M float item table in the live range): reported, no target

    python tools/ema_bench.py --what kernel [--reps 200] [--windows 7]
    python tools/ema_bench.py --what step [--configs cfg2,cfg3] [--steps 40] [--windows 7]

Needs the GPU; there is no fallback."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name -> (id mode, S, Lt, D, N, B)
CONFIGS = {"cfg2": (False, 40, 100, 768, 2, 512), "cfg3": (True, 20, 1, 512, 4, 256)}
HEADS, N_USERS, N_ITEMS = 16, 1903, 352494
EMA = dict(decay=0.999, warmup=True)


def _model(torch, id_mode, S, Lt, D, N, dev):
    from segmminterest_amd.trainer import default_args, init_model
    kind = "id" if id_mode else "image"
    margs = default_args(num_layers_enc=N, d_model=D, nhead=HEADS, input_type={"user": kind, "photo": kind}, exposure_prob=[1.0] * S)
    torch.manual_seed(1234)
    return init_model(margs, n_users=N_USERS, n_items=N_ITEMS, input_dim=D, max_vid_len=S, max_usr_len=Lt).to(dev)


def _batches(torch, id_mode, S, Lt, D, B, n, dev):
    from segmminterest_amd.synth import make_batch
    return [{k: v.to(dev) for k, v in make_batch(B, S, Lt, D, n_users=N_USERS, n_items=N_ITEMS, seed=1234 + 1000 * i, features=not id_mode).items()}
            for i in range(n)]


def _events_us(torch, fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps


def kernel_legs(torch, H, n, dev):
    """[(label, bytes per element, knob value or None, launch)] over buffers of n floats; the update's weight is tiny and p = shadow + a
    little, so hundreds of launches stay finite."""
    acc, g, shadow = (torch.randn(n, device=dev) for _ in range(3))
    g.mul_(1e-3)
    p = shadow + 1e-3 * torch.randn(n, device=dev)
    a, b = torch.randn(n, device=dev), torch.randn(n, device=dev)
    return [("vec_add  acc <- acc + g", 12, None, lambda: H.vec_add(acc, acc, g, n)),
            ("ema_update  EMA_NT=1 (shadow nontemporal)", 12, 1, lambda: H.ema_update(shadow, p, n, 1e-3, True, 1000)),
            ("ema_update  EMA_NT=0 (default policy)", 12, 0, lambda: H.ema_update(shadow, p, n, 1e-3, True, 1000)),
            ("vec_swap  a <-> b", 16, None, lambda: H.vec_swap(a, b, n))]


def kernel(torch, reps, windows, dev):
    from segmminterest_amd import hipabi as H
    id_mode, S, Lt, D, N, _ = CONFIGS["cfg2"]
    model = _model(torch, id_mode, S, Lt, D, N, dev)
    model._store.ensure()
    n_live = model._store.n_live
    del model
    default_nt = H.knob("EMA_NT")
    print("ema kernel_bench: %s; config-2 model n_live = %d floats (%.1f MB per operand); %d alternating windows of %d launches; the library's "
          "default policy is EMA_NT=%d" % (torch.cuda.get_device_name(0), n_live, 4 * n_live / 2 ** 20, windows, reps, default_nt))
    ok = True
    for n in (n_live, 4 * n_live):
        legs = kernel_legs(torch, H, n, dev)
        us = [[] for _ in legs]
        try:
            for _, _, nt, fn in legs:          # warm
                if nt is not None:
                    H.config_set("EMA_NT", nt)
                for _ in range(10):
                    fn()
            for _ in range(windows):
                for k, (_, _, nt, fn) in enumerate(legs):
                    if nt is not None:
                        H.config_set("EMA_NT", nt)
                    us[k].append(_events_us(torch, fn, reps))
        finally:
            H.config_set("EMA_NT", default_nt)
        med = [statistics.median(v) for v in us]
        spr = [max(v) - min(v) for v in us]
        for (label, bpe, _, _), m, s in zip(legs, med, spr):
            print("n %10d  %-44s %8.2f us  spread %.2f us  %6.2f TB/s of %d n bytes" % (n, label, m, s, bpe * n / m / 1e6, bpe))
        mine = med[1 if default_nt else 2]
        good = mine <= med[0] + 2 * spr[0]
        ok = ok and good
        print("n %10d  condition ema_update (EMA_NT=%d) %.2f us <= vec_add %.2f us + 2 x %.2f us: %s"
              % (n, default_nt, mine, med[0], spr[0], "PASS" if good else "FAIL"))
        del legs
        torch.cuda.empty_cache()
    return ok


def step(torch, name, steps, windows, reps, dev):
    from segmminterest_amd import hipabi as H
    from segmminterest_amd.trainer import Trainer
    id_mode, S, Lt, D, N, B = CONFIGS[name]
    default_nt = H.knob("EMA_NT")
    trs = {}
    for leg, ema in (("plain", None), ("ema", EMA)):
        tr = Trainer(_model(torch, id_mode, S, Lt, D, N, dev), device_state=True, ema=ema)
        bs = _batches(torch, id_mode, S, Lt, D, B, 3, dev)
        tr.train_step(bs[0])
        tr.train_step(bs[1])
        tr.record(bs[2], prev_batch=bs[1])
        for i in range(6):          # replays of every batch: warm
            tr.run_recorded(bs[i % 3])
        trs[leg] = (tr, bs)
    n_live = trs["ema"][0].model._store.n_live
    legs = [("plain", "plain", None), ("ema  EMA_NT=1 (shadow nontemporal)", "ema", 1), ("ema  EMA_NT=0 (default policy)", "ema", 0)]
    ms = [[] for _ in legs]
    alone = {}
    try:
        torch.cuda.synchronize()
        for _ in range(windows):
            for k, (_, which, nt) in enumerate(legs):
                tr, bs = trs[which]
                if nt is not None:
                    H.config_set("EMA_NT", nt)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(steps):
                    tr.run_recorded(bs[i % 3])
                torch.cuda.synchronize()
                ms[k].append(1e3 * (time.perf_counter() - t0) / steps)
        # the update alone over the trainer's own live range and shadow (weight 1e-3, p = the parameters: the shadow barely moves)
        tr = trs["ema"][0]
        keep = tr.ema.shadow.clone()
        for nt in (1, 0):
            H.config_set("EMA_NT", nt)
            fn = lambda: H.ema_update(tr.ema.shadow, tr.model._store.flat, n_live, 1e-3, True, 1000)
            for _ in range(10):
                fn()
            alone[nt] = statistics.median(_events_us(torch, fn, reps) for _ in range(3))
        tr.ema.shadow.copy_(keep)
    finally:
        H.config_set("EMA_NT", default_nt)
    med = [statistics.median(v) for v in ms]
    spr = [max(v) - min(v) for v in ms]
    print("%s  %s mode, B %d, n_live %d floats (%.1f MB: the update moves %.1f MB per step); %d commands per plain step, %d with the EMA"
          % (name, "id" if id_mode else "image", B, n_live, 4 * n_live / 2 ** 20, 12 * n_live / 2 ** 20, trs["plain"][0]._recorded["n_cmds"],
             trs["ema"][0]._recorded["n_cmds"]))
    for (label, _, nt), m, s in zip(legs, med, spr):
        extra = "" if nt is None else "  added %+.1f us (%+.2f %%); the update alone %.1f us" % (1e3 * (m - med[0]), 100 * (m - med[0]) / med[0], alone[nt])
        print("%s  %-36s %8.3f ms/step  %9.0f rows/s  spread %.3f ms over %d windows of %d steps%s" % (name, label, m, 1e3 * B / m, s, windows, steps, extra))
    k = 1 if default_nt else 2
    added, bound = 1e3 * (med[k] - med[0]), alone[default_nt] + 1e3 * spr[0]
    good = added <= bound
    print("%s  added time under the library's default policy (EMA_NT=%d) %.1f us vs the update alone %.1f us + the plain step's spread %.1f us = %.1f us: %s"
          % (name, default_nt, added, alone[default_nt], 1e3 * spr[0], bound, ("PASS" if good else "FAIL") if name == "cfg2" else "reported, no target"))
    del trs, tr
    torch.cuda.empty_cache()
    return good or name != "cfg2"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=("kernel", "step"), required=True)
    ap.add_argument("--configs", default="cfg2,cfg3")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ema_bench: no GPU (this tool measures the HIP path; there is no fallback)")
    from segmminterest_amd import hipabi as H
    H.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if args.what == "kernel":
        return 0 if kernel(torch, args.reps, args.windows, dev) else 1
    print("ema step_bench: %s; recorded steps, %d alternating windows of %d steps per leg" % (torch.cuda.get_device_name(0), args.windows, args.steps))
    ok = True
    for name in args.configs.split(","):
        ok = step(torch, name, args.steps, args.windows, args.reps, dev) and ok
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
