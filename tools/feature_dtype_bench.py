#!/usr/bin/env python
"""What 16-bit input features buy, at BASELINE config 2 shapes (B 512, S 40, Lt 100, D_in = d = 768, N 2, 16 heads): one text record,
three legs, every comparison inside ONE process with the dtypes alternating (profiles/feature_dtype/feature_dtype_bench.txt).

  (a) gather    hipabi.gather_l1 alone, rows = 512 x 40 and 512 x 100, D = 768, from a 200 000-line table (the size of bench.py's index
                leg) stored as float32 / float16 / bfloat16: microseconds per launch (HIP events around a run of launches, after a
                warm-up) and GB/s of algorithmic bytes (rows (8 D + 9) for a float32 table, rows (6 D + 9) for a 16-bit one)
  (b) index     the recorded training step fed by index batches, float32 table against float16 table, timed windows alternating
  (c) host_fed  bench.py's host_fed scheme -- pinned host batches, a copy stream one batch ahead, two device buffers -- with float32
                against float16 host tensors: interactions/s, h2d_bytes_per_step, H2D GB/s

    python tools/feature_dtype_bench.py [--steps 20] [--warmup 3] [--windows 3] [--legs a,b,c]

Needs the GPU; there is no fallback."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, S, LT, D, N, HEADS, N_LINES = 512, 40, 100, 768, 2, 16, 200000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--legs", default="a,b,c")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("feature_dtype_bench: no GPU (this tool measures the HIP kernels; there is no fallback)")
    from segmminterest_amd import hipabi as H
    from segmminterest_amd.feature_store import ResidentFeatureTable
    from segmminterest_amd.synth import make_batch
    from segmminterest_amd.trainer import DPComm, Trainer, default_args, init_model
    H.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    legs = set(args.legs.split(","))
    print("feature_dtype_bench: %s, B %d S %d Lt %d D_in %d d %d N %d heads %d, table %d lines, steps %d warmup %d windows %d"
          % (torch.cuda.get_device_name(0), B, S, LT, D, D, N, HEADS, N_LINES, args.steps, args.warmup, args.windows))
    feats32 = torch.rand((N_LINES, D), generator=torch.Generator().manual_seed(99)).to(dev)
    tables = {"float32": feats32, "float16": feats32.half(), "bfloat16": feats32.bfloat16()}

    def spread(xs):
        return max(xs) - min(xs)

    # ------------------------------------------------------------------ (a) the gather alone
    if "a" in legs:
        reps, iters = 9, 24
        for rows_l in (S, LT):
            # eight index sets taken in turn, as the steps of a run rotate their batches: the lines of one set are 63 MB of a float32
            # table, eight sets 503 MB -- more than the 256 MB the last-level cache could keep from launch to launch
            gi = torch.Generator().manual_seed(7)
            idxs = [torch.randint(0, N_LINES, (B, rows_l), generator=gi).to(dev) for _ in range(8)]
            rows = B * rows_l
            out = torch.empty((B, rows_l, D), dtype=torch.float32, device=dev)
            mask = torch.empty((B, rows_l), dtype=torch.uint8, device=dev)
            us = {k: [] for k in tables}
            for k, t in tables.items():          # warm-up
                for i in range(8):
                    H.gather_l1(t, idxs[i], out=out, mask=mask)
            torch.cuda.synchronize()
            for _ in range(reps):          # the dtypes alternate inside every repetition
                for k, t in tables.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for i in range(iters):
                        H.gather_l1(t, idxs[i % 8], out=out, mask=mask)
                    e1.record()
                    e1.synchronize()
                    us[k].append(1e3 * e0.elapsed_time(e1) / iters)
            ref = statistics.median(us["float32"])
            for k, t in tables.items():
                nb = rows * ((8 if t.dtype == torch.float32 else 6) * D + 9)
                med = statistics.median(us[k])
                print("gather  rows %6d D %d table %-8s  %7.1f us (min %7.1f max %7.1f over %d runs of %d launches)  %6.1f GB/s of %d algorithmic bytes"
                      % (rows, D, k, med, min(us[k]), max(us[k]), reps, iters, nb / med / 1e3, nb))
            for k in ("float16", "bfloat16"):
                med = statistics.median(us[k])
                print("gate    rows %6d %-8s median %.1f us <= float32 median %.1f us + its spread %.1f us: %s"
                      % (rows, k, med, ref, spread(us["float32"]), "PASS" if med <= ref + spread(us["float32"]) else "FAIL"))
            del out, mask, idxs

    margs = default_args(num_layers_enc=N, d_model=D, nhead=HEADS, input_type={"user": "image", "photo": "image"}, exposure_prob=[1.0] * S)

    def trainer(table=None):
        torch.manual_seed(1234)
        model = init_model(margs, n_users=1903, n_items=352494, input_dim=D, max_vid_len=S, max_usr_len=LT).to(dev)
        return model, Trainer(model, lr=1e-3, weight_decay=1e-4, comm=DPComm(), feature_table=table, device_state=True)

    def windows(runs):
        """runs: {name: fn(n_steps)}; ``windows`` timed windows per name, alternating -> {name: [interactions/s per window]}"""
        rates = {k: [] for k in runs}
        for _ in range(args.windows):
            for k, fn in runs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(args.steps)
                torch.cuda.synchronize()
                rates[k].append(B * args.steps / (time.perf_counter() - t0))
        return rates

    # ------------------------------------------------------------------ (b) the recorded step on index batches
    if "b" in legs:
        ib = []
        for i in range(8):
            b = make_batch(B, S, LT, D, seed=1234 + 1000 * i, features=False)
            g2 = torch.Generator().manual_seed(4321 + 1000 * i)
            pidx = torch.randint(0, N_LINES, (B, S), generator=g2)
            pidx[~b["photo_mask"]] = -1
            uidx = torch.randint(0, N_LINES, (B, LT), generator=g2)
            uidx[~b["user_mask"]] = -1
            b["photo_idx"], b["user_idx"] = pidx, uidx
            ib.append({k: v.to(dev) for k, v in b.items()})
        runs, keep = {}, []
        for k in ("float32", "float16"):
            model, tr = trainer(ResidentFeatureTable(tables[k]))
            for i in range(3):
                tr.train_step(ib[i])
            tr.record(ib[0], warmup=2)
            state = {"i": 0}

            def fn(n, tr=tr, state=state):
                for _ in range(n):
                    tr.run_recorded(ib[state["i"] % len(ib)])
                    state["i"] += 1
            fn(args.warmup)
            runs[k] = fn
            keep.append((model, tr))
        rates = windows(runs)
        for k, r in rates.items():
            print("index   table %-8s  %9.1f interactions/s median of %d windows of %d steps (min %9.1f max %9.1f)  %.4f ms/step"
                  % (k, statistics.median(r), len(r), args.steps, min(r), max(r), 1e3 * B / statistics.median(r)))
        m32, m16 = statistics.median(rates["float32"]), statistics.median(rates["float16"])
        print("gate    index step float16 median %.1f >= float32 median %.1f - its spread %.1f: %s"
              % (m16, m32, spread(rates["float32"]), "PASS" if m16 >= m32 - spread(rates["float32"]) else "FAIL"))
        del runs, keep, ib
        torch.cuda.empty_cache()

    # ------------------------------------------------------------------ (c) the recorded step fed from pinned host memory
    if "c" in legs:
        fkeys = ("user", "photo")
        base = [{k: v for k, v in make_batch(B, S, LT, D, seed=1234 + 1000 * i).items()} for i in range(4)]
        runs, keep, nbytes = {}, [], {}
        for name, dt in (("float32", torch.float32), ("float16", torch.float16)):
            dbatches = [{k: (v.to(dt) if k in fkeys else v).to(dev) for k, v in b.items()} for b in base]
            host = [{k: b[k].to(dt).pin_memory() for k in fkeys} for b in base]
            dbuf = [{k: torch.empty_like(dbatches[0][k]) for k in fkeys} for _ in range(2)]
            nbytes[name] = sum(host[0][k].numel() * host[0][k].element_size() for k in fkeys)
            model, tr = trainer()
            for i in range(3):
                tr.train_step(dbatches[i])
            tr.record(dbatches[0], warmup=2)
            cstream = torch.cuda.Stream()
            ready = [torch.cuda.Event(), torch.cuda.Event()]
            consumed = [torch.cuda.Event(), torch.cuda.Event()]

            def run_host(n, tr=tr, dbatches=dbatches, host=host, dbuf=dbuf, cstream=cstream, ready=ready, consumed=consumed):
                def stage(i):
                    j = i & 1
                    with torch.cuda.stream(cstream):
                        cstream.wait_event(consumed[j])          # the step that read this buffer has finished
                        for k in fkeys:
                            dbuf[j][k].copy_(host[i % len(host)][k], non_blocking=True)
                        ready[j].record(cstream)
                for j in (0, 1):
                    consumed[j].record()
                stage(0)
                for i in range(n):
                    if i + 1 < n:
                        stage(i + 1)
                    j = i & 1
                    torch.cuda.current_stream().wait_event(ready[j])
                    b = dict(dbatches[i % len(dbatches)])
                    b.update(dbuf[j])
                    tr.run_recorded(b)
                    consumed[j].record()
            run_host(max(args.warmup, 2))
            runs[name] = run_host
            keep.append((model, tr, dbatches, host, dbuf))
        rates = windows(runs)
        for k, r in rates.items():
            med = statistics.median(r)
            print("host_fed batches %-8s  %9.1f interactions/s median of %d windows of %d steps (min %9.1f max %9.1f)  h2d_bytes_per_step %d  H2D %.1f GB/s"
                  % (k, med, len(r), args.steps, min(r), max(r), nbytes[k], nbytes[k] * med / B / 1e9))
        m32, m16 = statistics.median(rates["float32"]), statistics.median(rates["float16"])
        print("gate    host_fed h2d_bytes_per_step float16 %d == float32 %d / 2: %s; rate float16 %.1f >= float32 %.1f: %s"
              % (nbytes["float16"], nbytes["float32"], "PASS" if 2 * nbytes["float16"] == nbytes["float32"] else "FAIL", m16, m32,
                 "PASS" if m16 >= m32 else "FAIL"))
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
