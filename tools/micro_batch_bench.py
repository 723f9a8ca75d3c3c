#!/usr/bin/env python
"""What a micro-batched step costs (Trainer(micro_batch=m)), measured on the GPU; writes nothing but its standard output
(profiles/micro_batch/step_bench.txt and vec_add_bench.txt are this tool's output, see profiles/README.md).

``--what step``: pairs of recorded steps in ONE process, alternating windows after both legs are warmed up and recorded:

    cfg2   A: the plain step at B = 512            B: micro_batch=512 at B = 2048 (k = 4)      BASELINE config 2's model
    cfg4   A: the plain step at B = 256            B: micro_batch=256 at B = 2048 (k = 8)      the same model, config 4's shard width
    cfg3   A: the plain step at B = 256 (id mode)  B: micro_batch=256 at B = 1024 (k = 4)      BASELINE config 3's model (id tables)

A window is ``--steps`` run_recorded() calls on rotating batches between two device synchronisations, timed with the host clock.
Per leg: the median window's ms per step, rows/s, and the window-to-window range (max - min of the windows' ms per step).  The
condition is t_B <= k t_A + spread, spread = the larger of the two ranges, each scaled to a B step (k x the range of A).  Then the peak
memory of one eager micro-batched step against one eager plain step on the same large batch, fresh trainers, the micro-batched one
first.

``--what vec_add``: segmm_vec_add alone at n = the config-2 model's live parameter count and at 4 n: device events around
``--reps`` launches, three operand patterns (acc <- acc + g, g <- acc + g, out <- a + b) and, for comparison, the same launches
rotating over enough buffer sets that the footprint exceeds 1 GB (past the last-level cache).  Bytes = 12 n per launch.

    python tools/micro_batch_bench.py --what step [--pairs cfg2,cfg4,cfg3] [--steps 40] [--windows 7]
    python tools/micro_batch_bench.py --what vec_add [--reps 200]

Needs the GPU; there is no fallback."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name -> (id mode, S, Lt, D, N, rows of leg A = micro_batch of leg B, rows of leg B)
PAIRS = {"cfg2": (False, 40, 100, 768, 2, 512, 2048), "cfg4": (False, 40, 100, 768, 2, 256, 2048), "cfg3": (True, 20, 1, 512, 4, 256, 1024)}
HEADS, N_USERS, N_ITEMS = 16, 1903, 352494


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


def step_pair(torch, name, steps, windows, dev):
    from segmminterest_amd.trainer import Trainer
    id_mode, S, Lt, D, N, Ba, Bb = PAIRS[name]
    k = Bb // Ba
    legs = {}
    for leg, B, m in (("A", Ba, None), ("B", Bb, Ba)):
        tr = Trainer(_model(torch, id_mode, S, Lt, D, N, dev), device_state=True, micro_batch=m)
        bs = _batches(torch, id_mode, S, Lt, D, B, 3, dev)
        tr.train_step(bs[0])
        tr.train_step(bs[1])
        tr.record(bs[2], prev_batch=bs[1])
        for i in range(6):          # replays of every batch: warm
            tr.run_recorded(bs[i % 3])
        legs[leg] = (tr, bs, B)
    torch.cuda.synchronize()
    ms = {"A": [], "B": []}
    for _ in range(windows):
        for leg in ("A", "B"):
            tr, bs, B = legs[leg]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(steps):
                tr.run_recorded(bs[i % 3])
            torch.cuda.synchronize()
            ms[leg].append(1e3 * (time.perf_counter() - t0) / steps)
    med = {leg: statistics.median(v) for leg, v in ms.items()}
    rng = {leg: max(v) - min(v) for leg, v in ms.items()}
    for leg in ("A", "B"):
        tr, bs, B = legs[leg]
        print("%s %s  %-22s B %4d  %8.3f ms/step  %9.0f rows/s  range %.3f ms over %d windows of %d steps  (%d commands per step)"
              % (name, leg, "plain" if leg == "A" else "micro_batch=%d (k=%d)" % (Ba, k), B, med[leg], 1e3 * B / med[leg], rng[leg], windows, steps,
                 tr._recorded["n_cmds"]))
    spread = max(k * rng["A"], rng["B"])
    ok = med["B"] <= k * med["A"] + spread
    print("%s    t_B %.3f ms vs %d t_A = %.3f ms (ratio %.3f); spread %.3f ms; condition t_B <= %d t_A + spread: %s; t_B < %d t_A: %s"
          % (name, med["B"], k, k * med["A"], med["B"] / (k * med["A"]), spread, k, "PASS" if ok else "FAIL", k, med["B"] < k * med["A"]))
    del legs, tr, bs
    torch.cuda.empty_cache()
    # peak memory of one eager step on the large batch: micro-batched first, then plain, fresh trainers
    peaks = []
    big = _batches(torch, id_mode, S, Lt, D, Bb, 1, dev)[0]
    for m in (Ba, None):
        tr = Trainer(_model(torch, id_mode, S, Lt, D, N, dev), micro_batch=m)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        try:
            tr.train_step(big)
            torch.cuda.synchronize()
            peaks.append((torch.cuda.max_memory_allocated(), before))
        except torch.OutOfMemoryError:
            peaks.append((None, before))
        del tr
        torch.cuda.empty_cache()
    (pm, b0), (pp, b1) = peaks
    print("%s    peak memory of one step at B %d: micro_batch=%d %.1f MB (%.1f MB held before the step: model, batch), plain %s; ratio %s"
          % (name, Bb, Ba, pm / 2 ** 20, b0 / 2 ** 20, "does not fit" if pp is None else "%.1f MB" % (pp / 2 ** 20),
             "-" if pp is None else "%.3f" % (pm / pp)))
    return ok


def vec_add(torch, reps, dev):
    from segmminterest_amd import hipabi as H
    id_mode, S, Lt, D, N, _, _ = PAIRS["cfg2"]
    model = _model(torch, id_mode, S, Lt, D, N, dev)
    model._store.ensure()
    n_live = model._store.n_live
    del model
    print("vec_add_bench: %s; config-2 model n_live = %d floats (%.1f MB per operand); %d launches per timing, 12 n bytes per launch"
          % (torch.cuda.get_device_name(0), n_live, 4 * n_live / 2 ** 20, reps))

    def timed(fn):
        for i in range(10):
            fn(i)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for i in range(reps):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        return 1e3 * e0.elapsed_time(e1) / reps          # us per launch

    for n in (n_live, 4 * n_live):
        sets = max(2, -(-(1 << 30) // (12 * n)) + 1)          # buffer sets whose footprint exceeds 1 GB
        bufs = [tuple(torch.randn(n + 4, device=dev) for _ in range(3)) for _ in range(sets)]
        o, a, b = bufs[0]
        for label, fn in (("acc <- acc + g", lambda i: H.vec_add(a, a, b, n)), ("g <- acc + g", lambda i: H.vec_add(b, a, b, n)),
                          ("out <- a + b", lambda i: H.vec_add(o, a, b, n)),
                          ("out <- a + b, 4-byte aligned only (+1 float)", lambda i: H.vec_add(o, a, b, n, 1, 1, 1)),
                          ("out <- a + b, offsets 0 / 1 / 2 (dword path)", lambda i: H.vec_add(o, a, b, n, 0, 1, 2)),
                          ("out <- a + b, rotating over %d buffer sets (%.2f GB)" % (sets, sets * 12 * n / 2 ** 30),
                           lambda i: H.vec_add(bufs[i % sets][0], bufs[i % sets][1], bufs[i % sets][2], n))):
            us = [timed(fn) for _ in range(3)]
            u = statistics.median(us)
            print("n %10d  %-52s %8.2f us  (min %.2f max %.2f of 3)  %6.2f TB/s of 12 n bytes" % (n, label, u, min(us), max(us), 12 * n / u / 1e6))
        del bufs, o, a, b
        torch.cuda.empty_cache()
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=("step", "vec_add"), required=True)
    ap.add_argument("--pairs", default="cfg2,cfg4,cfg3")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("micro_batch_bench: no GPU (this tool measures the HIP path; there is no fallback)")
    from segmminterest_amd import hipabi as H
    H.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if args.what == "vec_add":
        return 0 if vec_add(torch, args.reps, dev) else 1
    print("micro_batch_bench: %s; recorded steps, %d alternating windows of %d steps per leg" % (torch.cuda.get_device_name(0), args.windows, args.steps))
    ok = True
    for name in args.pairs.split(","):
        ok = step_pair(torch, name, args.steps, args.windows, dev) and ok
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
