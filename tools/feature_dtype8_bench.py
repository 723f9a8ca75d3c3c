#!/usr/bin/env python
"""What 8-bit input features (OCP e4m3fn, OCP e5m2, int8) cost and buy, at BASELINE config 2 shapes (B 512, S 40, Lt 100, D_in = d =
768, N 2, 16 heads): the sibling of tools/feature_dtype_bench.py, one text record per run (profiles/feature_dtype8/).
Every comparison is made inside ONE process with the dtypes alternating, and the float32 and float16 legs run in the same windows as
the yardstick: no number here is compared with a number of another run.

  (a) gather    hipabi.gather_l1 alone, rows = 512 x 40 and 512 x 100, D = 768, from a 200 000-line table stored as float32 / float16 /
                float8_e4m3fn / int8: microseconds per launch and GB/s of algorithmic bytes (rows ((4 + element size) D + 9))
  (b) index     the recorded training step fed by index batches, per table dtype, timed windows alternating
  (c) host_fed  bench.py's host_fed scheme (pinned host batches, a copy stream one batch ahead, two device buffers) per batch dtype:
                interactions/s, h2d_bytes_per_step, H2D GB/s -- against the resident-table rate of leg (b) of this very run
                -- and, in the same windows, the same recorded step on the same batches already on the device (no copy)
  (l) alone     hipabi.l1norm of 51 200 x 768 per x dtype (rows / planes only / both), and the pinned host -> device copy of that tensor
  (q) quantise  segmm_quantize_rows at 65 536 x 1024 per format, and ResidentFeatureTable.from_memmap wall time per GB of file
  (e) accuracy  of the STORAGE (a property of the formats, not of the kernels): eval logits of the config-2 model from the quantised
                table against the float32 table, max |delta| / max |logit| per format, seeds 0 .. 4; and 30-step loss curves of a tiny
                model per table format next to the float32 curve.  Reported, not asserted.

    python tools/feature_dtype8_bench.py [--steps 20] [--warmup 3] [--windows 3] [--legs a,b,c,l,q,e] [--dtypes float32,float16,e4m3,int8]

``--dtypes`` also fixes the ORDER in which the formats take turns (and in which their trainers and pinned buffers are created): a second
run with the order reversed tells a property of a format from a property of its place in the queue.

Needs the GPU; there is no fallback."""
import argparse
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, S, LT, D, N, HEADS, N_LINES = 512, 40, 100, 768, 2, 16, 200000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--legs", default="a,b,c,l,q,e")
    ap.add_argument("--dtypes", default="float32,float16,e4m3,int8", help="the storage formats of legs a, b, c, in the order they take turns")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("feature_dtype8_bench: no GPU (this tool measures the HIP kernels; there is no fallback)")
    from segmminterest_amd import hipabi as H
    from segmminterest_amd.feature_store import ResidentFeatureTable
    from segmminterest_amd.synth import make_batch
    from segmminterest_amd.trainer import DPComm, Trainer, default_args, init_model
    H.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    legs = set(args.legs.split(","))
    print("feature_dtype8_bench: %s, B %d S %d Lt %d D_in %d d %d N %d heads %d, table %d lines, steps %d warmup %d windows %d"
          % (torch.cuda.get_device_name(0), B, S, LT, D, D, N, HEADS, N_LINES, args.steps, args.warmup, args.windows))
    E4, E5, I8 = torch.float8_e4m3fn, torch.float8_e5m2, torch.int8
    names = {torch.float32: "float32", torch.float16: "float16", E4: "e4m3", E5: "e5m2", I8: "int8"}
    feats32 = torch.rand((N_LINES, D), generator=torch.Generator().manual_seed(99)).to(dev)

    def stored(f32, dt):
        return f32 if dt == torch.float32 else f32.half() if dt == torch.float16 else H.quantize_rows(f32, dt)

    by_name = {v: k for k, v in names.items()}
    order = [by_name[n] for n in args.dtypes.split(",")]
    if torch.float32 not in order or torch.float16 not in order:
        raise SystemExit("feature_dtype8_bench: --dtypes must keep float32 and float16, the yardstick legs of every window")
    tables = {names[dt]: stored(feats32, dt) for dt in order}
    print("table   bytes: " + ", ".join("%s %d" % (k, t.numel() * t.element_size()) for k, t in tables.items()))

    def spread(xs):
        return max(xs) - min(xs)

    # ------------------------------------------------------------------ (a) the gather alone
    if "a" in legs:
        reps, iters = 9, 24
        for rows_l in (LT, S):
            # eight index sets taken in turn (tools/feature_dtype_bench.py: more lines than the last-level cache keeps between launches)
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
            for k, t in tables.items():
                nb = rows * ((4 + t.element_size()) * D + 9)
                med = statistics.median(us[k])
                print("gather  rows %6d D %d table %-8s  %7.1f us (min %7.1f max %7.1f over %d runs of %d launches)  %6.1f GB/s of %d algorithmic bytes"
                      % (rows, D, k, med, min(us[k]), max(us[k]), reps, iters, nb / med / 1e3, nb))
            del out, mask, idxs

    margs = default_args(num_layers_enc=N, d_model=D, nhead=HEADS, input_type={"user": "image", "photo": "image"}, exposure_prob=[1.0] * S)

    def trainer(table=None, seed=1234):
        torch.manual_seed(seed)
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

    def index_batches(n, seed0=1234):
        ib = []
        for i in range(n):
            b = make_batch(B, S, LT, D, seed=seed0 + 1000 * i, features=False)
            g2 = torch.Generator().manual_seed(4321 + seed0 + 1000 * i)
            pidx = torch.randint(0, N_LINES, (B, S), generator=g2)
            pidx[~b["photo_mask"]] = -1
            uidx = torch.randint(0, N_LINES, (B, LT), generator=g2)
            uidx[~b["user_mask"]] = -1
            b["photo_idx"], b["user_idx"] = pidx, uidx
            ib.append({k: v.to(dev) for k, v in b.items()})
        return ib

    # ------------------------------------------------------------------ (b) the recorded step on index batches
    resident = None
    if "b" in legs or "c" in legs:
        ib = index_batches(8)
        runs, keep = {}, []
        for k in tables if "b" in legs else ("float32",):
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
        resident = statistics.median(rates["float32"])
        if "float16" in rates:
            m16, s16 = statistics.median(rates["float16"]), spread(rates["float16"])
            for k in (k for k in rates if k not in ("float32", "float16")):
                m = statistics.median(rates[k])
                print("note    index step %s median %.1f against float16 median %.1f, float16 spread %.1f: %s"
                      % (k, m, m16, s16, "within the spread" if m >= m16 - s16 else "SLOWER than float16 by more than its spread"))
        del runs, keep, ib
        torch.cuda.empty_cache()

    # ------------------------------------------------------------------ (c) the recorded step fed from pinned host memory
    if "c" in legs:
        fkeys = ("user", "photo")
        base = [{k: v for k, v in make_batch(B, S, LT, D, seed=1234 + 1000 * i).items()} for i in range(4)]
        runs, keep, nbytes = {}, [], {}
        for dt in order:
            name = names[dt]
            # (8-bit: quantised on the device, row by row, as a loader would; then back to pinned host memory)
            conv = [{k: stored(b[k].to(dev).contiguous(), dt) for k in fkeys} for b in base]
            dbatches = [dict({k: v.to(dev) for k, v in b.items() if k not in fkeys}, **c) for b, c in zip(base, conv)]
            host = [{k: c[k].cpu().pin_memory() for k in fkeys} for c in conv]
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
            def run_dev(n, tr=tr, dbatches=dbatches):          # the same recorded step on the same batches, already on the device: no copy
                for i in range(n):
                    tr.run_recorded(dbatches[i % len(dbatches)])
            run_host(max(args.warmup, 2))
            runs[name] = run_host
            runs[name + "/device"] = run_dev
            keep.append((model, tr, dbatches, host, dbuf))
        rates = windows(runs)
        for k, r in rates.items():
            med = statistics.median(r)
            if k.endswith("/device"):
                print("dev_fed  batches %-8s  %9.1f interactions/s median of %d windows of %d steps (min %9.1f max %9.1f)  no host copy: the step alone"
                      % (k[:-7], med, len(r), args.steps, min(r), max(r)))
                continue
            print("host_fed batches %-8s  %9.1f interactions/s median of %d windows of %d steps (min %9.1f max %9.1f)  h2d_bytes_per_step %d  "
                  "H2D %.1f GB/s  %.1f %% of the resident float32 table's %.1f of this run"
                  % (k, med, len(r), args.steps, min(r), max(r), nbytes[k], nbytes[k] * med / B / 1e9, 100.0 * med / resident, resident))
        del runs, keep
        torch.cuda.empty_cache()

    # ------------------------------------------------------------------ (l) the normalisation and the host copy, each alone
    if "l" in legs:
        x32 = torch.rand((B, LT, D), generator=torch.Generator().manual_seed(1)).to(dev)
        xs = {names[dt]: stored(x32, dt) for dt in order}
        rows = B * LT
        y = torch.empty((B, LT, D), dtype=torch.float32, device=dev)
        hdr = H.new_site(dev)[0]
        sc = torch.tensor([2.0 ** 14], dtype=torch.float32, device=dev)
        pl = torch.zeros((rows, 2 * D), dtype=torch.float16, device=dev)
        po = H.PO(pl, 2 * D, hdr, sc.data_ptr())

        def timeit(fn, reps=7, iters=16):
            for _ in range(3):
                fn()
            ts = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    fn()
                e1.record()
                e1.synchronize()
                ts.append(1e3 * e0.elapsed_time(e1) / iters)
            return statistics.median(ts), min(ts), max(ts)
        for mode in ("rows", "planes only", "rows + planes"):
            for k, x in xs.items():
                fn = {"rows": lambda: H.l1norm(x, y), "planes only": lambda: H.l1norm(x, None, po=po), "rows + planes": lambda: H.l1norm(x, y, po=po)}[mode]
                print("l1norm  rows %6d D %d x %-8s out %-13s %7.1f us (min %7.1f max %7.1f)" % ((rows, D, k, mode) + timeit(fn)))
        for k, x in xs.items():
            h = x.cpu().pin_memory()
            d = torch.empty_like(x)
            med, lo, hi = timeit(lambda: d.copy_(h, non_blocking=True), reps=5, iters=8)
            nb = x.numel() * x.element_size()
            print("h2d     %-8s pinned %s  %8.1f us (min %8.1f max %8.1f)  %.1f GB/s of %d bytes" % (k, h.is_pinned(), med, lo, hi, nb / med / 1e3, nb))
        del x32, xs, y, pl

    # ------------------------------------------------------------------ (q) the quantiser and the loader
    if "q" in legs:
        rows_q, d_q = 65536, 1024
        x = torch.randn((rows_q, d_q), generator=torch.Generator().manual_seed(3)).to(dev)
        for dt in (E4, E5, I8):
            q = torch.empty((rows_q, d_q), dtype=dt, device=dev)
            sc = torch.empty((rows_q,), dtype=torch.float32, device=dev)
            for _ in range(3):
                H.quantize_rows(x, dt, out=q, scale_out=sc)
            ts = []
            for _ in range(7):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(8):
                    H.quantize_rows(x, dt, out=q, scale_out=sc)
                e1.record()
                e1.synchronize()
                ts.append(1e3 * e0.elapsed_time(e1) / 8)
            nb = rows_q * (5 * d_q + 4)          # x read once from HBM (the second pass hits the cache or not: algorithmic bytes), codes written
            med = statistics.median(ts)
            print("quantize_rows %d x %d -> %-5s %7.1f us (min %7.1f max %7.1f over 7 runs of 8 launches)  %6.1f GB/s of %d algorithmic bytes"
                  % (rows_q, d_q, names[dt], med, min(ts), max(ts), nb / med / 1e3, nb))
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "features.bin")
            x.cpu().numpy().tofile(path)
            gb = rows_q * d_q * 4 / 1e9
            for rep in range(2):          # the second round reads the file from the page cache
                for dt in (torch.float32, torch.float16, E4, I8):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    t = ResidentFeatureTable.from_memmap(path, rows_q, d_q, dtype=dt, device=dev, chunk_rows=16384)
                    torch.cuda.synchronize()
                    dtm = time.perf_counter() - t0
                    print("from_memmap round %d  %-8s  %.3f s for a %.3f GB file = %.3f s/GB (chunks of 16384 lines)" % (rep, names[dt], dtm, gb, dtm / gb))
                    del t
        del x

    # ------------------------------------------------------------------ (e) accuracy of the storage
    if "e" in legs:
        fmts = (torch.float16, E4, E5, I8)
        for seed in range(5):
            f32 = torch.rand((N_LINES, D), generator=torch.Generator().manual_seed(1000 + seed)).to(dev)
            b = index_batches(1, seed0=77 + seed)[0]
            ref = None
            line = []
            for dt in (torch.float32,) + fmts:
                model, tr = trainer(ResidentFeatureTable(stored(f32, dt)), seed=seed)
                logits = tr.eval_step(b, mode="inference")["logits"].detach().float().clone()
                if ref is None:
                    ref = logits
                    continue
                line.append("%s %.3e" % (names[dt], float((logits - ref).abs().max() / ref.abs().max())))
                del model, tr
            print("logits  seed %d  max|logit| %.4f  max |delta| / max |logit| against the float32 table:  %s" % (seed, float(ref.abs().max()), "  ".join(line)))
            del f32
            torch.cuda.empty_cache()
        # 30-step loss curves of a tiny model (d 32, 4 heads, D_in 64, B 16, S 8, Lt 12), one table per format, the same batches
        tb, ts_, tl, td, tn = 16, 8, 12, 64, 512
        targs = default_args(num_layers_enc=2, d_model=32, nhead=4, input_type={"user": "image", "photo": "image"}, exposure_prob=[1.0] * ts_)
        tf32 = torch.rand((tn, td), generator=torch.Generator().manual_seed(5)).to(dev)
        tib = []
        for i in range(6):
            bb = make_batch(tb, ts_, tl, td, seed=900 + i, features=False)
            g2 = torch.Generator().manual_seed(950 + i)
            pidx = torch.randint(0, tn, (tb, ts_), generator=g2)
            pidx[~bb["photo_mask"]] = -1
            uidx = torch.randint(0, tn, (tb, tl), generator=g2)
            uidx[~bb["user_mask"]] = -1
            bb["photo_idx"], bb["user_idx"] = pidx, uidx
            tib.append({k: v.to(dev) for k, v in bb.items()})
        for dt in (torch.float32,) + fmts:
            torch.manual_seed(7)
            model = init_model(targs, n_users=64, n_items=512, input_dim=td, max_vid_len=ts_, max_usr_len=tl).to(dev)
            tr = Trainer(model, lr=1e-3, weight_decay=1e-4, comm=DPComm(), feature_table=ResidentFeatureTable(stored(tf32, dt)), dropout=False)
            losses = [float(tr.train_step(tib[i % len(tib)])["loss"].detach()) for i in range(30)]
            print("curve   tiny model, table %-8s  " % names[dt] + " ".join("%.5f" % v for v in losses))
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
