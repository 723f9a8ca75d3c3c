#!/usr/bin/env python
"""What lazy exact AdamW of the item-id table costs and saves (Trainer(lazy_tables=...)), measured on the GPU; prints its report and,
with ``--out FILE``, writes the same text there (profiles/lazy_tables/lazy_tables_bench.txt is this tool's output, see
profiles/README.md).

``--what step``: the recorded BASELINE config-3 step (id / id, B = 1024, S = 20, d = 512, N = 4, 352 494 items), lazy against the
dense two-pass trainer of the SAME build, in one process, in alternating windows of ``--steps`` replays (a host clock around replays
that end in a device synchronise).  Every leg walks the same pool of ``--pool`` id batches, so the gap between two visits of a row is
the workload's, not that of three rotating batches.  Two draws of the item ids: uniform over the catalogue, and skewed (id =
1 + floor(n_items u^4), u uniform: a quarter of the draws fall on 0.4 % of the items).  Lazy legs: flush_every 64, 256, 1024; their
windows hold the periodic flushes that fall into them (windows x steps is a multiple of 1024: the mean over the windows carries each
leg's flushes at their true share).  Before the timed windows every leg runs ``--settle`` steps, more than the largest flush_every:
the stamps are in their steady state.  Reported per leg: median and mean window, the dense leg's window spread, and whether the lazy
mean is slower than the dense mean by more than that spread.

``--what kernel``: segmm_adamw_table_catchup alone on a 352 494 x W table (W the model's table width): 1024 listed rows that are ``gap``
steps behind (the stamps are put back before every launch by a copy whose own time is measured and subtracted): at the batch's mean
gap in each of the step part's pools and for each flush_every, then for a sweep of gaps; and ONE flush of the whole table after flush_every untouched steps.

``--what dp_kernel``: segmm_adamw_table_lazy_rows (the data-parallel tail: replay + step T + stamp in one launch) against the three
launches it replaces on the same list -- catch-up to T - 1, phase 1 of segmm_adamw_table_lrs, the stamp -- on the config-3 table at
1024 / 2048 / 4096 listed ids (the gathered list of 1, 2 and 4 ranks) whose rows are 0, 16 and 58 steps behind T - 1 (58: the
uniform-id mean gap at flush_every = 64).  The ring push is in neither: both protocols make it.

``--what dp_step``: the recorded config-3 DATA-PARALLEL step (B = 1024 rows per rank), ``lazy_tables=dict(flush_every=64,
data_parallel=True)`` against the dense data-parallel trainer, in alternating windows in ONE process group; the periodic flushes fall
inside the windows.  Run it under ``torchrun --nproc_per_node=<GPUs>``; started plainly (one GPU) it makes a forced one-rank RCCL
group (SEGMM_DP_FORCE=1): every collective is really issued but is an identity, and the gathered list is the rank's own.  Rank 0
reports.  profiles/lazy_tables/dp_bench.txt is the output of ``--what dp_kernel,dp_step``.

``--what ema_kernel``: lazy tables beside a weight average (``lazy_tables=dict(ema=True)``): segmm_adamw_table_catchup_ema and
segmm_adamw_table_lazy_rows_ema alone, each against its sibling without the shadow, at 1024 / 2048 / 4096 listed ids whose rows are 0
and 58 steps behind T - 1, and ONE EMA-mode flush of the whole table after 64 untouched steps against today's flush.

``--what ema_step``: the recorded config-3 step with ``ema=0.999``: ``lazy_tables=dict(flush_every=64, ema=True)`` against the dense
two-pass trainer with the dense EMA launch and against the lazy trainer without an EMA, three legs in alternating windows in one
process, uniform and skewed ids, the periodic flushes inside the windows.  profiles/lazy_tables/ema_bench.txt is the output of
``--what ema_kernel,ema_step --settle 200``.

    python tools/lazy_tables_bench.py [--what step,kernel] [--windows 8] [--steps 256] [--pool 512] [--settle 1100] [--out FILE]

Needs the GPU; there is no fallback."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HEADS, N_USERS, N_ITEMS = 16, 1903, 352494
CFG3 = (20, 1, 512, 4, 1024)          # S, Lt, d, N, B of BASELINE config 3
FLUSH = (64, 256, 1024)
TABLE = "backbone1.vid_proj.weight"

LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def _model(torch, dev):
    from segmminterest_amd.trainer import default_args, init_model
    S, Lt, D, N, _ = CFG3
    margs = default_args(num_layers_enc=N, d_model=D, nhead=HEADS, input_type={"user": "id", "photo": "id"}, exposure_prob=[1.0] * S)
    torch.manual_seed(1234)
    return init_model(margs, n_users=N_USERS, n_items=N_ITEMS, input_dim=D, max_vid_len=S, max_usr_len=Lt).to(dev)


def _pool(torch, dev, n, skewed):
    from segmminterest_amd.synth import make_batch
    S, Lt, D, _, B = CFG3
    g = torch.Generator().manual_seed(77)
    out = []
    for i in range(n):
        b = make_batch(B, S, Lt, D, n_users=N_USERS, n_items=N_ITEMS, seed=1234 + 1000 * i, features=False)
        if skewed:
            b["photo_identity_id"] = (1 + (N_ITEMS * torch.rand(B, generator=g, dtype=torch.float64) ** 4).long()).clamp_(max=N_ITEMS)
            b["photo_id"] = b["photo_identity_id"].clone()
        out.append({k: v.to(dev) for k, v in b.items()})
    return out


def mean_gap(pool, cap):
    """Mean over the pool's listed rows of min(steps since the row's last visit, cap) while the pool is walked round and round."""
    last, tot, cnt = {}, 0, 0
    for rnd in range(2):
        for t, b in enumerate(pool):
            for r in set(b["photo_identity_id"].tolist()):
                if rnd:
                    tot += min(len(pool) + t - last.get(r, -10 ** 9), cap)
                    cnt += 1
                last[r] = len(pool) * rnd + t
    return tot / max(cnt, 1)


def step(torch, steps, windows, n_pool, settle, dev):
    from segmminterest_amd.trainer import Trainer
    ok = True
    for skewed in (False, True):
        pool = _pool(torch, dev, n_pool, skewed)
        legs = {}
        for leg in ("dense",) + tuple("lazy %d" % f for f in FLUSH):
            tr = Trainer(_model(torch, dev), device_state=True, lazy_tables=None if leg == "dense" else dict(flush_every=int(leg.split()[1])))
            tr.train_step(pool[0])
            tr.train_step(pool[1])
            tr.record(pool[2], prev_batch=pool[1])
            for i in range(settle):
                tr.run_recorded(pool[(3 + i) % n_pool])
            legs[leg] = [tr, 3 + settle]
        torch.cuda.synchronize()
        ms = {leg: [] for leg in legs}
        for _ in range(windows):
            for leg, e in legs.items():
                tr = e[0]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(steps):
                    tr.run_recorded(pool[(e[1] + i) % n_pool])
                torch.cuda.synchronize()
                ms[leg].append(1e3 * (time.perf_counter() - t0) / steps)
                e[1] += steps
        d = ms["dense"]
        spread, mean0 = max(d) - min(d), statistics.mean(d)
        rows = [len(set(b["photo_identity_id"].tolist())) for b in pool]
        say("recorded config-3 step (B = %d), item ids %s: pool of %d batches (%.0f distinct rows per batch), %d settling steps, %d alternating "
            "windows of %d replays" % (CFG3[4], "SKEWED (1 + floor(n u^4))" if skewed else "uniform", n_pool, statistics.mean(rows), settle, windows, steps))
        say("  dense two-pass    median %.4f ms  mean %.4f ms  (min %.4f max %.4f: spread %.4f ms = %.2f %%)"
            % (statistics.median(d), mean0, min(d), max(d), spread, 100 * spread / mean0))
        best = None
        for f in FLUSH:
            x = ms["lazy %d" % f]
            mean = statistics.mean(x)
            slower = mean - mean0 > spread
            say("  lazy flush_every %-5d median %.4f ms  mean %.4f ms  (min %.4f max %.4f)  mean / dense %.4f  mean gap of a listed row %.1f steps  "
                "slower than dense by more than its spread: %s" % (f, statistics.median(x), mean, min(x), max(x), mean / mean0, mean_gap(pool, f),
                                                                   "YES" if slower else "no"))
            if best is None or mean < best[1]:
                best = (f, mean)
        say("  smallest mean: flush_every = %d" % best[0])
        ok = ok and best[1] - mean0 <= spread
        del legs, pool
        torch.cuda.empty_cache()
    return ok


def _timed(torch, fn, reps):
    """us per call of ``fn``: ``reps`` calls between two device events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps


def kernel(torch, windows, n_pool, dev):
    from segmminterest_amd import hipabi as H
    model = _model(torch, dev)
    width = model.get_parameter(TABLE).shape[1]
    rows = model.get_parameter(TABLE).shape[0]
    del model
    n = rows * width
    p, m = (torch.randn(n, device=dev) * 1e-2 for _ in range(2))
    v = torch.rand(n, device=dev) * 1e-4
    cap = 1024
    hist = torch.zeros((cap, 4), device=dev)
    for t in range(1, cap + 1):
        H.adamw_hist_push(hist, 1e-3, 0.9, 0.999, 5000 + t)
    target = 5000 + cap
    stamps, behind = torch.zeros(rows, dtype=torch.int32, device=dev), torch.zeros(rows, dtype=torch.int32, device=dev)
    ids = torch.randperm(rows, device=dev)[:1024].to(torch.int64).contiguous()
    say("segmm_adamw_table_catchup alone: table %d x %d, 1024 distinct listed rows, each `gap` steps behind; us per launch (median of %d windows), "
        "the copy that puts the stamps back subtracted" % (rows, width, windows))
    hp = (1.0, 0.9, 0.999, 1e-8, 1e-2)
    # the batch's MEAN gap in the step part's two pools, per flush_every (a listed row is never further behind than that), then a sweep
    gaps = []
    for skewed in (False, True):
        pool = _pool(torch, "cpu", n_pool, skewed)
        gaps += [(max(1, round(mean_gap(pool, f))), "the batch's mean gap, %s ids, flush_every %d" % ("skewed" if skewed else "uniform", f)) for f in FLUSH]
    for gap, label in gaps + [(g, "") for g in (1, 8, 32, 64, 128, 344, 1024)]:
        behind.fill_(target - gap)

        def both():
            H.copy_bytes(stamps, behind)
            H.adamw_table_catchup(p, m, v, 0, rows, width, ids, stamps, hist, target, *hp)
        both()
        torch.cuda.synchronize()
        reps = 50 if gap <= 128 else 10
        full = statistics.median(_timed(torch, both, reps) for _ in range(windows))
        copy = statistics.median(_timed(torch, lambda: H.copy_bytes(stamps, behind), reps) for _ in range(windows))
        say("  gap %-5d %9.2f us (%.2f ns per row-step)%s" % (gap, full - copy, 1e3 * (full - copy) / (1024 * gap), "   " + label if label else ""))
    say("ONE flush of the whole table (%d x %d = %.0f M floats, 24 B per float = %.2f GB of traffic) after flush_every untouched steps:"
        % (rows, width, n / 1e6, 24.0 * n / 1e9))
    for f in FLUSH:
        behind.fill_(target - f)

        def flush():
            H.copy_bytes(stamps, behind)
            H.adamw_table_catchup(p, m, v, 0, rows, width, None, stamps, hist, target, *hp)
        flush()
        torch.cuda.synchronize()
        us = statistics.median(_timed(torch, flush, 2) for _ in range(3))
        say("  flush_every %-5d %9.3f ms = %.1f us per step it covers" % (f, 1e-3 * us, us / f))


DP_FLUSH = 64


def dp_kernel(torch, windows, dev):
    from segmminterest_amd import hipabi as H
    model = _model(torch, dev)
    rows, width = model.get_parameter(TABLE).shape
    del model
    n = rows * width
    p, m, g = (torch.randn(n, device=dev) * 1e-2 for _ in range(3))
    v = torch.rand(n, device=dev) * 1e-4
    cap = DP_FLUSH
    hist = torch.zeros((cap, 4), device=dev)
    T = 5000 + cap
    for t in range(T - cap + 1, T + 1):
        H.adamw_hist_push(hist, 1e-3, 0.9, 0.999, t)
    stamps, behind = (torch.zeros(rows, dtype=torch.int32, device=dev) for _ in range(2))
    flags = torch.zeros(rows, dtype=torch.int32, device=dev)
    hp = (0.9, 0.999, 1e-8, 1e-2)
    say("segmm_adamw_table_lazy_rows against catch-up + phase 1 + stamp: table %d x %d, distinct listed rows, each `gap` steps behind T - 1; "
        "us per step tail (median of %d windows of 50), the copy that puts the stamps back subtracted" % (rows, width, windows))
    for n_ids in (1024, 2048, 4096):
        ids = torch.randperm(rows, device=dev)[:n_ids].to(torch.int64).contiguous()
        for gap in (0, 16, 58):
            behind.fill_(T - 1 - gap)

            def fused():
                H.copy_bytes(stamps, behind)
                H.adamw_table_lazy_rows(p, g, m, v, 0, rows, width, ids, stamps, hist, 1e-3, 1.0, *hp, T)

            def three():
                H.copy_bytes(stamps, behind)
                H.adamw_table_catchup(p, m, v, 0, rows, width, ids, stamps, hist, T - 1, 1.0, *hp, flags=flags)
                H.adamw_table_lrs(p, g, m, v, 0, rows, width, ids, flags, 1e-3, 1.0, *hp, T, 1)
                H.adamw_table_stamp(ids, rows, stamps, T)
            res = {}
            for name, fn in (("three", three), ("fused", fused), ("copy", lambda: H.copy_bytes(stamps, behind))):
                fn()
                torch.cuda.synchronize()
                res[name] = statistics.median(_timed(torch, fn, 50) for _ in range(windows))
            a, b = res["three"] - res["copy"], res["fused"] - res["copy"]
            say("  ids %-5d gap %-3d three launches %8.2f us   fused %8.2f us   saved %7.2f us   fused / three %.3f" % (n_ids, gap, a, b, a - b, b / a))


def dp_step(torch, steps, windows, n_pool, settle):
    import torch.distributed as dist
    from segmminterest_amd.synth import make_batch
    world, rank, local = (int(os.environ.get(k, d)) for k, d in (("WORLD_SIZE", "1"), ("RANK", "0"), ("LOCAL_RANK", "0")))
    if world == 1:
        os.environ.update(SEGMM_DP_FORCE="1", MASTER_ADDR=os.environ.get("MASTER_ADDR", "127.0.0.1"), MASTER_PORT=os.environ.get("MASTER_PORT", "29777"),
                          RANK="0", WORLD_SIZE="1")
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    from segmminterest_amd.trainer import DPComm, Trainer
    try:
        S, Lt, D, _, B = CFG3
        pool = [{k: v.to(dev) for k, v in make_batch(B, S, Lt, D, n_users=N_USERS, n_items=N_ITEMS, seed=1234 + 1000 * i + 7919 * rank,
                                                     features=False).items()} for i in range(n_pool)]
        legs = {}
        for leg in ("dense", "lazy"):
            tr = Trainer(_model(torch, dev), comm=DPComm(), device_state=True,
                         lazy_tables=None if leg == "dense" else dict(flush_every=DP_FLUSH, data_parallel=True))
            assert tr.comm.active and tr.sparse_tables
            tr.train_step(pool[0])
            tr.train_step(pool[1])
            tr.record(pool[2], warmup=0, prev_batch=pool[1])
            for i in range(settle):
                tr.run_recorded(pool[(3 + i) % n_pool])
            legs[leg] = [tr, 3 + settle]
        torch.cuda.synchronize()
        dist.barrier()
        ms = {leg: [] for leg in legs}
        for _ in range(windows):
            for leg, e in legs.items():
                tr = e[0]
                torch.cuda.synchronize()
                dist.barrier()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(steps):
                    tr.run_recorded(pool[(e[1] + i) % n_pool])
                torch.cuda.synchronize()
                ms[leg].append(1e3 * (time.perf_counter() - t0) / steps)
                e[1] += steps
        if rank == 0:
            d, x = ms["dense"], ms["lazy"]
            spread, mean0, mean = max(d) - min(d), statistics.mean(d), statistics.mean(x)
            say("recorded config-3 DATA-PARALLEL step, %d rank%s x B = %d rows (RCCL%s), uniform item ids: pool of %d batches per rank, %d settling "
                "steps, %d alternating windows of %d replays in one process group; flush_every = %d, its flushes inside the windows"
                % (world, "" if world == 1 else "s", B, ", ONE FORCED RANK: every collective is issued and is an identity, the gathered list is "
                   "the rank's own" if world == 1 else "", n_pool, settle, windows, steps, DP_FLUSH))
            say("  dense data-parallel  median %.4f ms  mean %.4f ms  (min %.4f max %.4f: spread %.4f ms = %.2f %%)"
                % (statistics.median(d), mean0, min(d), max(d), spread, 100 * spread / mean0))
            say("  lazy data-parallel   median %.4f ms  mean %.4f ms  (min %.4f max %.4f)  mean / dense %.4f  saved %.4f ms per step"
                % (statistics.median(x), mean, min(x), max(x), mean / mean0, mean0 - mean))
            say("  lazy faster than dense by more than the dense leg's window spread: %s" % ("yes" if mean0 - mean > spread else "NO"))
    finally:
        dist.destroy_process_group()
    return rank


EMA_DECAY = 0.999


def ema_kernel(torch, windows, dev):
    """The *_ema launches against their siblings of the same build, and the EMA-mode flush against today's."""
    from segmminterest_amd import hipabi as H
    model = _model(torch, dev)
    rows, width = model.get_parameter(TABLE).shape
    del model
    n = rows * width
    p, m, g, sh = (torch.randn(n, device=dev) * 1e-2 for _ in range(4))
    v = torch.rand(n, device=dev) * 1e-4
    cap = DP_FLUSH
    hist = torch.zeros((cap, 4), device=dev)
    T = 5000 + cap
    for t in range(T - cap + 1, T + 1):
        H.adamw_hist_push_ema(hist, 1e-3, 0.9, 0.999, t, 1.0 - EMA_DECAY, True)
    stamps, behind = (torch.zeros(rows, dtype=torch.int32, device=dev) for _ in range(2))
    hp = (0.9, 0.999, 1e-8, 1e-2)
    say("the *_ema launches against their siblings: table %d x %d, distinct listed rows, each `gap` steps behind T - 1; us per launch (median of "
        "%d windows of 50), the copy that puts the stamps back subtracted" % (rows, width, windows))
    for n_ids in (1024, 2048, 4096):
        ids = torch.randperm(rows, device=dev)[:n_ids].to(torch.int64).contiguous()
        for gap in (0, 58):
            behind.fill_(T - 1 - gap)
            fns = {
                "catchup": lambda: H.adamw_table_catchup(p, m, v, 0, rows, width, ids, stamps, hist, T - 1, 1.0, *hp),
                "catchup_ema": lambda: H.adamw_table_catchup_ema(p, m, v, sh, 0, 0, rows, width, ids, stamps, hist, T - 1, 1.0, *hp),
                "lazy_rows": lambda: H.adamw_table_lazy_rows(p, g, m, v, 0, rows, width, ids, stamps, hist, 1e-3, 1.0, *hp, T),
                "lazy_rows_ema": lambda: H.adamw_table_lazy_rows_ema(p, g, m, v, sh, 0, 0, rows, width, ids, stamps, hist, 1e-3, 1.0, *hp, T),
                "copy": lambda: None}
            res = {}
            for name, fn in fns.items():
                def both(fn=fn):
                    H.copy_bytes(stamps, behind)
                    fn()
                both()
                torch.cuda.synchronize()
                res[name] = statistics.median(_timed(torch, both, 50) for _ in range(windows))
            c, ce, r, re_ = (res[k] - res["copy"] for k in ("catchup", "catchup_ema", "lazy_rows", "lazy_rows_ema"))
            say("  ids %-5d gap %-3d catchup %8.2f us  catchup_ema %8.2f us (x %.3f)   lazy_rows %8.2f us  lazy_rows_ema %8.2f us (x %.3f)"
                % (n_ids, gap, c, ce, ce / c if c > 0 else float("nan"), r, re_, re_ / r if r > 0 else float("nan")))
    say("ONE flush of the whole table after %d untouched steps (%d x %d = %.0f M floats; 24 B per float without the shadow, 32 B with it):"
        % (cap, rows, width, n / 1e6))
    behind.fill_(T - cap)
    for name, fn in (("segmm_adamw_table_catchup", lambda: H.adamw_table_catchup(p, m, v, 0, rows, width, None, stamps, hist, T, 1.0, *hp)),
                     ("segmm_adamw_table_catchup_ema", lambda: H.adamw_table_catchup_ema(p, m, v, sh, 0, 0, rows, width, None, stamps, hist, T, 1.0, *hp))):
        def flush(fn=fn):
            H.copy_bytes(stamps, behind)
            fn()
        flush()
        torch.cuda.synchronize()
        us = statistics.median(_timed(torch, flush, 2) for _ in range(3))
        say("  %-30s %9.3f ms = %.1f us per step it covers" % (name, 1e-3 * us, us / cap))


def ema_step(torch, steps, windows, n_pool, settle, dev):
    """The recorded config-3 step with a weight average: lazy tables + lazily averaged shadow against the dense two-pass trainer with the
    dense EMA launch (the parent's behaviour) and against the lazy trainer without an EMA, alternating windows in one process."""
    from segmminterest_amd.trainer import Trainer
    legs_kw = (("dense + ema", dict(ema=EMA_DECAY)), ("lazy, no ema", dict(lazy_tables=dict(flush_every=DP_FLUSH))),
               ("lazy + ema (key)", dict(ema=EMA_DECAY, lazy_tables=dict(flush_every=DP_FLUSH, ema=True))))
    for skewed in (False, True):
        pool = _pool(torch, dev, n_pool, skewed)
        legs = {}
        for leg, kw in legs_kw:
            tr = Trainer(_model(torch, dev), device_state=True, **kw)
            tr.train_step(pool[0])
            tr.train_step(pool[1])
            tr.record(pool[2], prev_batch=pool[1])
            for i in range(settle):
                tr.run_recorded(pool[(3 + i) % n_pool])
            legs[leg] = [tr, 3 + settle]
        torch.cuda.synchronize()
        ms = {leg: [] for leg in legs}
        for _ in range(windows):
            for leg, e in legs.items():
                tr = e[0]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(steps):
                    tr.run_recorded(pool[(e[1] + i) % n_pool])
                torch.cuda.synchronize()
                ms[leg].append(1e3 * (time.perf_counter() - t0) / steps)
                e[1] += steps
        d = ms["dense + ema"]
        spread, mean0 = max(d) - min(d), statistics.mean(d)
        say("recorded config-3 step (B = %d) with a weight average (decay %g, warm-up), item ids %s: pool of %d batches, %d settling steps, %d "
            "alternating windows of %d replays; flush_every = %d, the flushes inside the windows"
            % (CFG3[4], EMA_DECAY, "SKEWED (1 + floor(n u^4))" if skewed else "uniform", n_pool, settle, windows, steps, DP_FLUSH))
        for leg, _ in legs_kw:
            x = ms[leg]
            say("  %-18s median %.4f ms  mean %.4f ms  (min %.4f max %.4f: spread %.4f ms)  mean - (dense + ema) %+.4f ms"
                % (leg, statistics.median(x), statistics.mean(x), min(x), max(x), max(x) - min(x), statistics.mean(x) - mean0))
        x = ms["lazy + ema (key)"]
        say("  lazy + ema faster than dense + ema by more than the dense leg's window spread (%.4f ms): %s"
            % (spread, "yes" if mean0 - statistics.mean(x) > spread else "NO"))
        del legs, pool
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="step,kernel")
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--pool", type=int, default=512)
    ap.add_argument("--settle", type=int, default=1100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("lazy_tables_bench: no GPU (this tool measures the HIP path; there is no fallback)")
    from segmminterest_amd import hipabi as H
    H.lib()
    dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))          # (torchrun: --what dp_step, one GPU per rank)
    torch.cuda.set_device(dev)
    say("lazy_tables_bench: %s" % torch.cuda.get_device_name(0))
    ok = True
    what = args.what.split(",")
    if "kernel" in what:
        kernel(torch, min(args.windows, 5), args.pool, dev)
    if "step" in what:
        ok = step(torch, args.steps, args.windows, args.pool, args.settle, dev)
    if "step" in what or "kernel" in what:
        say("lazy (best flush_every) not slower than dense beyond the dense leg's window spread, both draws: %s" % ("yes" if ok else "NO"))
    rank = int(os.environ.get("RANK", "0"))
    if "dp_kernel" in what and rank == 0:
        dp_kernel(torch, min(args.windows, 5), dev)
    if "dp_step" in what:
        dp_step(torch, args.steps, args.windows, args.pool, args.settle)
    if "ema_kernel" in what and rank == 0:
        ema_kernel(torch, min(args.windows, 5), dev)
    if "ema_step" in what and rank == 0:
        ema_step(torch, args.steps, args.windows, args.pool, args.settle, dev)
    if args.out and rank == 0:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
