#!/usr/bin/env python
"""What opt-in mixed precision (Trainer(mixed_precision=...): one-product fp16 plane GEMMs) buys, measured on the GPU; writes nothing
but its standard output (profiles/mixed_precision/kernel_bench.txt and step_bench.txt are this tool's output).

``--what kernel``: the plane GEMM stand-alone, products 1 against 3 through the same launcher (segmm_gemm_pq; segmm_gemm_p is its
products = 3 call), under the library's default kernel choice, at
    config 2's shapes   NT 20480 x 3072 x 768, 20480 x 768 x 768, 51200 x 768 x 768, 20480 x 768 x 3072;
                                     TN 768 x 768 x 20480, 768 x 768 x 51200 (M x N x tokens, the trainer's split count)
    config 3's K = 512 shapes        NT 5120 x 512 x 512, 5120 x 1536 x 512, 5120 x 2048 x 512 (gemm_pl_nt8)
Alternating windows in ONE process: a window is ``--reps`` launches of one leg between two device events; ``--windows`` rounds over
the two legs.  Per leg: the median window's us per launch and the window-to-window spread (max - min); the spread of the
three-product leg is the baseline's noise.  Also printed: the bytes a launch moves at least (operand planes once + the output) and
the time they take at 4 TB/s, the floor that the unchanged P32 staging sets for one product.

``--what step``: the recorded training step, BASELINE configs 2 and 3: option off (the default trainer: the parent commit's
arithmetic, bit for bit) against ``True``, then each role alone, every leg its own trainer in ONE process (same model seed, same
batches), all warmed up and recorded, then alternating windows of ``--steps`` run_recorded() calls between two device
synchronisations, timed with the host clock.  No ratio is a target: a role that does not pay is reported as such.

    python tools/mixed_precision_bench.py --what kernel [--reps 50] [--windows 7]
    python tools/mixed_precision_bench.py --what step [--configs cfg2,cfg3] [--steps 30] [--windows 7]

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
NT_SHAPES = [("cfg2", 20480, 3072, 768), ("cfg2", 20480, 768, 768), ("cfg2", 51200, 768, 768), ("cfg2", 20480, 768, 3072),
             ("cfg3", 5120, 512, 512), ("cfg3", 5120, 1536, 512), ("cfg3", 5120, 2048, 512)]
TN_SHAPES = [("cfg2", 768, 768, 20480), ("cfg2", 768, 768, 51200)]
STEP_LEGS = [("off", None), ("all", True), ("forward", dict(dgrad=False, wgrad=False)), ("dgrad", dict(forward=False, wgrad=False)),
             ("wgrad", dict(forward=False, dgrad=False))]
HBM_TBS = 4.0          # the rate the floor is quoted at


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


def _alternate(torch, legs, reps, windows):
    """legs: [launch]; -> (medians, spreads) of us per launch over alternating windows"""
    for fn in legs:
        for _ in range(5):
            fn()
    us = [[] for _ in legs]
    for _ in range(windows):
        for k, fn in enumerate(legs):
            us[k].append(_events_us(torch, fn, reps))
    return [statistics.median(v) for v in us], [max(v) - min(v) for v in us]


def kernel(torch, reps, windows, dev):
    from segmminterest_amd import engine as E, hipabi as H
    print("mixed_precision kernel_bench: %s; products 1 against 3, default kernel choice (PL_VAR=%d TN_VAR=%d); %d alternating windows of %d "
          "launches" % (torch.cuda.get_device_name(0), H.knob("PL_VAR"), H.knob("TN_VAR"), windows, reps))
    g = torch.Generator(device=dev).manual_seed(7)
    for cfg, M, N, K in NT_SHAPES:
        a = H.to_planes(torch.randn(M, K, device=dev, generator=g), M, K, keep_f32=False)
        b = H.to_planes(torch.randn(N, K, device=dev, generator=g) * 0.05, N, K, keep_f32=False)
        c = torch.empty(M, N, device=dev)
        legs = [lambda p=p: H.gemm_p(H.LAYOUT_NT, M, N, K, a, b, c, N, products=p) for p in (3, 1)]
        med, spr = _alternate(torch, legs, reps, windows)
        mb = (4 * M * K + 4 * N * K + 4 * M * N) / 1e6
        print("%s NT %6d x %5d x %5d  three %8.1f us (spread %.1f)  one %8.1f us (spread %.1f)  one / three %.3f  %6.1f / %6.1f TFLOP/s (useful)  "
              "moves >= %.0f MB = %.0f us at %g TB/s" % (cfg, M, N, K, med[0], spr[0], med[1], spr[1], med[1] / med[0], 2e-6 * M * N * K / med[0],
                                                          2e-6 * M * N * K / med[1], mb, mb / HBM_TBS, HBM_TBS))
        del a, b, c, legs
        torch.cuda.empty_cache()
    sw = E.switches.read("engine")
    for cfg, M, N, K in TN_SHAPES:
        a = H.to_planes(torch.randn(K, M, device=dev, generator=g) * 0.01, K, M, keep_f32=False)
        b = H.to_planes(torch.randn(K, N, device=dev, generator=g), K, N, keep_f32=False)
        c, cs = torch.empty(M, N, device=dev), torch.empty(M, device=dev)
        splits = E._splits_for_p(M, N, K, sw["split_target_p"], sw["split_target_few"])
        ws = torch.empty(max(splits, 1) * (M * N + M), device=dev)
        legs = [lambda p=p: H.gemm_p(H.LAYOUT_TN, M, N, K, a, b, c, N, splits=splits, workspace=ws, colsum_out=cs, products=p) for p in (3, 1)]
        med, spr = _alternate(torch, legs, reps, windows)
        mb = (4 * K * M + 4 * K * N + 4 * M * N * (2 * splits + 1 if splits > 1 else 1)) / 1e6
        print("%s TN %6d x %5d x %5d  splits %3d  three %8.1f us (spread %.1f)  one %8.1f us (spread %.1f)  one / three %.3f  moves >= %.0f MB = "
              "%.0f us at %g TB/s (with the bias column sums, split-K slabs and their combine)"
              % (cfg, M, N, K, splits, med[0], spr[0], med[1], spr[1], med[1] / med[0], mb, mb / HBM_TBS, HBM_TBS))
        del a, b, c, ws, legs
        torch.cuda.empty_cache()
    return 0


def step(torch, name, steps, windows, dev):
    from segmminterest_amd.trainer import Trainer
    id_mode, S, Lt, D, N, B = CONFIGS[name]
    trs = []
    for leg, mp in STEP_LEGS:
        tr = Trainer(_model(torch, id_mode, S, Lt, D, N, dev), device_state=True, mixed_precision=mp)
        bs = _batches(torch, id_mode, S, Lt, D, B, 3, dev)
        tr.train_step(bs[0])
        tr.train_step(bs[1])
        tr.record(bs[2], prev_batch=bs[1])
        for i in range(6):          # replays of every batch: warm
            tr.run_recorded(bs[i % 3])
        trs.append((tr, bs))
    ms = [[] for _ in trs]
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
    print("%s  %s mode, B %d, d %d, N %d; %d commands per recorded step" % (name, "id" if id_mode else "image", B, D, N, trs[0][0]._recorded["n_cmds"]))
    for (leg, _), m, s in zip(STEP_LEGS, med, spr):
        print("%s  mixed_precision %-8s %8.3f ms/step  %9.0f rows/s  spread %.3f ms over %d windows of %d steps  %+.2f %% step time against off"
              % (name, leg, m, 1e3 * B / m, s, windows, steps, 100 * (m - med[0]) / med[0]))
    del trs
    torch.cuda.empty_cache()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=("kernel", "step"), required=True)
    ap.add_argument("--configs", default="cfg2,cfg3")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("mixed_precision_bench: no GPU (this tool measures the HIP path; there is no fallback)")
    from segmminterest_amd import hipabi as H
    H.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if args.what == "kernel":
        return kernel(torch, args.reps, args.windows, dev)
    print("mixed_precision step_bench: %s; recorded steps, %d alternating windows of %d steps per leg; 'off' is the default trainer"
          % (torch.cuda.get_device_name(0), args.windows, args.steps))
    for name in args.configs.split(","):
        step(torch, name, args.steps, args.windows, dev)
    return 0


if __name__ == "__main__":
    sys.exit(main())
