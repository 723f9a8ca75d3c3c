#!/usr/bin/env python
"""What the non-finite guard costs (Trainer(skip_nonfinite=True)), measured on the GPU; writes nothing but its standard output
(profiles/nonfinite_guard/step_bench.txt is this tool's output, see profiles/README.md).

The recorded training step of three trainers in ONE process (same model, same batches), all warmed up and recorded, then
alternating windows of ``--steps`` run_recorded() calls between two device synchronisations, timed with the host clock:

    plain      Trainer(device_state=True): no norm; id mode steps the item table in two passes, the early one under the forward
    norm       ... max_grad_norm=inf: the norm's two launches, the coefficient is 1; the same table passes
    guarded    ... skip_nonfinite=True: the norm, segmm_step_guard, every update through its *_guarded entry point; id mode steps
               the table densely at the tail (the early pass would run before the verdict exists)

Per leg: the median window's ms per step and the window-to-window spread (max - min).  The guard's cost is reported against both
other legs; guarded - norm is the guard itself (one one-thread launch and one scalar load per workgroup of the updates) plus, in id
mode, the early table pass given up; norm - plain is the norm, which clipping pays as well.  Every batch is clean: no step is skipped
(a skipped step is cheaper: its update launches return at once).

    cfg2   BASELINE config 2's model (image mode, B = 512)
    cfg3   BASELINE config 3's model (id mode, B = 256, a 90 M float item table in the live range)

    python tools/nonfinite_guard_bench.py [--configs cfg2,cfg3] [--steps 40] [--windows 7]

Needs the GPU; there is no fallback.  No target is set: the figures are reported."""
import argparse
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name -> (id mode, S, Lt, D, N, B)
CONFIGS = {"cfg2": (False, 40, 100, 768, 2, 512), "cfg3": (True, 20, 1, 512, 4, 256)}
HEADS, N_USERS, N_ITEMS = 16, 1903, 352494
LEGS = (("plain", {}), ("norm  max_grad_norm=inf", dict(max_grad_norm=math.inf)), ("guarded  skip_nonfinite=True", dict(skip_nonfinite=True)))


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


def step(torch, name, steps, windows, dev):
    from segmminterest_amd.trainer import Trainer
    id_mode, S, Lt, D, N, B = CONFIGS[name]
    trs = []
    for label, kw in LEGS:
        tr = Trainer(_model(torch, id_mode, S, Lt, D, N, dev), device_state=True, **kw)
        bs = _batches(torch, id_mode, S, Lt, D, B, 3, dev)
        tr.train_step(bs[0])
        tr.train_step(bs[1])
        tr.record(bs[2], prev_batch=bs[1])
        for i in range(6):          # replays of every batch: warm
            tr.run_recorded(bs[i % 3])
        trs.append((tr, bs))
    ms = [[] for _ in LEGS]
    torch.cuda.synchronize()
    for _ in range(windows):
        for k, (tr, bs) in enumerate(trs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(steps):
                tr.run_recorded(bs[i % 3])
            torch.cuda.synchronize()
            ms[k].append(1e3 * (time.perf_counter() - t0) / steps)
    med = [statistics.median(v) for v in ms]
    spr = [max(v) - min(v) for v in ms]
    guarded = trs[2][0]
    skipped = guarded.opt.skipped_steps
    print("%s  %s mode, B %d, n_live %d floats (%.1f MB); commands per recorded step: %s; %d of the guarded trainer's %d steps skipped"
          % (name, "id" if id_mode else "image", B, guarded.model._store.n_live, 4 * guarded.model._store.n_live / 2 ** 20,
             ", ".join("%s %d" % (label.split()[0], tr._recorded["n_cmds"]) for (label, _), (tr, _) in zip(LEGS, trs)), skipped, guarded.opt.step_count))
    for (label, _), m, s in zip(LEGS, med, spr):
        print("%s  %-30s %8.3f ms/step  %9.0f rows/s  spread %.3f ms over %d windows of %d steps" % (name, label, m, 1e3 * B / m, s, windows, steps))
    for k, against in ((1, "the max_grad_norm=inf trainer"), (0, "the plain trainer")):
        print("%s  guarded against %-30s %+8.1f us (%+.2f %%); that leg's spread %.1f us, the guarded leg's %.1f us"
              % (name, against + ":", 1e3 * (med[2] - med[k]), 100 * (med[2] - med[k]) / med[k], 1e3 * spr[k], 1e3 * spr[2]))
    print("%s  the norm alone (max_grad_norm=inf against plain): %+.1f us (%+.2f %%)" % (name, 1e3 * (med[1] - med[0]), 100 * (med[1] - med[0]) / med[0]))
    del trs, guarded
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="cfg2,cfg3")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--windows", type=int, default=7)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("nonfinite_guard_bench: no GPU (this tool measures the HIP path; there is no fallback)")
    from segmminterest_amd import hipabi as H
    H.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    print("nonfinite_guard step_bench: %s; recorded steps, %d alternating windows of %d steps per leg" % (torch.cuda.get_device_name(0), args.windows, args.steps))
    for name in args.configs.split(","):
        step(torch, name, args.steps, args.windows, dev)
    return 0


if __name__ == "__main__":
    sys.exit(main())
