#!/usr/bin/env python
"""What parameter groups cost (FusedAdamW(param_groups=...)), measured on the GPU; prints its report and, with ``--out FILE``,
writes the same text there (profiles/param_groups/adamw_groups_bench.txt is this tool's output, see profiles/README.md).

``--what kernel``: segmm_adamw_groups against segmm_adamw on the SAME four buffers, in one process, in alternating windows: a window
is ``reps`` launches of one leg between two device events.  Sizes: the config-2 model's live range (6.6 M floats: 106 MB of p, g, m, v)
and config 3's item table (352 494 x 256 = 90 M floats: 1.4 GB).  Legs: plain (segmm_adamw, the yardstick -- the parent commit has the
same kernel), 1 / 8 / 64 segments with different scales and decays and no frozen one (ends off the 256-float wave boundaries), and 8
segments with two frozen ones that cover a quarter of the range.  Per leg: the median window's us per launch and TB/s of the bytes it
moves (28 B per stepped element), its ratio to plain, and whether it is slower than plain by more than plain's own window-to-window
range.  For the frozen leg also the ratio to expect from the bytes skipped (0.75).

``--what step``: the recorded config-2 step (B = 512) with no_decay_groups against the plain recorded step, alternating windows of
``--steps`` replays, as tools/micro_batch_bench.py times its pairs.

    python tools/param_groups_bench.py [--what kernel,step] [--windows 7] [--steps 40] [--out FILE]

Needs the GPU; there is no fallback."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HEADS, N_USERS, N_ITEMS = 16, 1903, 352494
CFG2 = (40, 100, 768, 2, 512)          # S, Lt, D, N, B of BASELINE config 2
TABLE = 352494 * 256                   # config 3's item table

LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def _model(torch, dev):
    from segmminterest_amd.trainer import default_args, init_model
    S, Lt, D, N, _ = CFG2
    margs = default_args(num_layers_enc=N, d_model=D, nhead=HEADS, input_type={"user": "image", "photo": "image"}, exposure_prob=[1.0] * S)
    torch.manual_seed(1234)
    return init_model(margs, n_users=N_USERS, n_items=N_ITEMS, input_dim=D, max_vid_len=S, max_usr_len=Lt).to(dev)


def segments(torch, n, k, frozen=(), dev="cuda"):
    """k segments over n floats, interior ends 68 floats past the k-th parts (multiples of 4, inside a wave's 256 floats)."""
    ends = [min(n, (n * (i + 1) // k) // 4 * 4 + 68) for i in range(k - 1)] + [n]
    scale = [(1.0, 0.1, 3.0, 0.5)[i % 4] for i in range(k)]
    wd = [(1e-2, 0.0, 0.1)[i % 3] for i in range(k)]
    if k == 1:
        scale, wd = [1.0], [1e-2]
    fz = [1 if i in frozen else 0 for i in range(k)]
    stepped = sum(e - s for s, e, f in zip([0] + ends[:-1], ends, fz) if not f)
    # no frozen segment: no flags (what FusedAdamW passes then; the kernel need not wait for the table before its loads)
    return (torch.tensor(ends, dtype=torch.int64, device=dev), torch.tensor(scale, dtype=torch.float32, device=dev),
            torch.tensor(wd, dtype=torch.float32, device=dev), torch.tensor(fz, dtype=torch.uint8, device=dev) if any(fz) else None), stepped


def kernel(torch, n, windows, dev):
    from segmminterest_amd import hipabi as H
    p, g, m = (torch.randn(n, device=dev) * 1e-2 for _ in range(3))
    v = torch.rand(n, device=dev) * 1e-4
    hp = (0.9, 0.999, 1e-8)
    legs = [("plain segmm_adamw", None, n)]
    for label, k, fz in (("groups, 1 segment", 1, ()), ("groups, 8 segments", 8, ()), ("groups, 64 segments", 64, ()),
                         ("groups, 8 segments, 2 frozen (1/4)", 8, (1, 5))):
        tab, stepped = segments(torch, n, k, fz, dev)
        legs.append((label, tab, stepped))

    # the C entry points directly, arguments built once: the host's share of a launch stays well below the kernel's time
    L, st = H.lib(), H._stream()
    ptrs = tuple(t.data_ptr() for t in (p, g, m, v))

    def launch(tab):
        if tab is None:
            rc = L.segmm_adamw(*ptrs, n, 1e-4, *hp, 1e-2, 7, st)
        else:
            rc = L.segmm_adamw_groups(*ptrs, 0, n, *(None if t is None else t.data_ptr() for t in tab), tab[0].numel(), 1e-4, *hp, 7, None, st)
        if rc:
            raise RuntimeError(L.segmm_last_error().decode())

    reps = max(20, int(0.06 / (28.0 * n / 3.5e12)))          # about 60 ms of launches per window at 3.5 TB/s
    for _, tab, _ in legs:
        for _ in range(5):
            launch(tab)
    torch.cuda.synchronize()
    us = {label: [] for label, _, _ in legs}
    for _ in range(windows):
        for label, tab, _ in legs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                launch(tab)
            e1.record()
            torch.cuda.synchronize()
            us[label].append(1e3 * e0.elapsed_time(e1) / reps)
    base = us[legs[0][0]]
    med0, spread = statistics.median(base), max(base) - min(base)
    say("n = %d floats (%.0f MB in p, g, m, v): %d alternating windows of %d launches per leg" % (n, 16.0 * n / 2 ** 20, windows, reps))
    say("  plain's own spread (max - min of its windows): %.2f us = %.2f %% of its median" % (spread, 100 * spread / med0))
    ok = True
    for label, tab, stepped in legs:
        med = statistics.median(us[label])
        line = "  %-36s %9.2f us  (min %.2f max %.2f)  %5.2f TB/s of %4.0f MB" % (label, med, min(us[label]), max(us[label]), 28.0 * stepped / med / 1e6,
                                                                                  28.0 * stepped / 2 ** 20)
        if tab is not None:
            within = med - med0 <= spread
            line += "  ratio to plain %.4f" % (med / med0)
            if stepped == n:
                line += "  slower than plain by more than plain's spread: %s" % ("no" if within else "YES (+%.2f us)" % (med - med0 - spread))
                ok = ok and within
            else:
                line += "  (bytes stepped / all bytes = %.4f)" % (stepped / n)
        say(line)
    del p, g, m, v
    torch.cuda.empty_cache()
    return ok


def step(torch, steps, windows, dev):
    from segmminterest_amd.synth import make_batch
    from segmminterest_amd.trainer import Trainer, no_decay_groups
    S, Lt, D, N, B = CFG2
    legs = {}
    # "plain again": a second trainer without groups -- what two instances of the SAME step differ by (their buffers lie elsewhere)
    for leg in ("plain", "no_decay_groups", "plain again"):
        model = _model(torch, dev)
        tr = Trainer(model, device_state=True, param_groups=no_decay_groups(model) if leg == "no_decay_groups" else None)
        bs = [{k: v.to(dev) for k, v in make_batch(B, S, Lt, D, n_users=N_USERS, n_items=N_ITEMS, seed=1234 + 1000 * i).items()} for i in range(3)]
        tr.train_step(bs[0])
        tr.train_step(bs[1])
        tr.record(bs[2], prev_batch=bs[1])
        for i in range(6):
            tr.run_recorded(bs[i % 3])
        legs[leg] = (tr, bs)
    torch.cuda.synchronize()
    ms = {leg: [] for leg in legs}
    for _ in range(windows):
        for leg, (tr, bs) in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(steps):
                tr.run_recorded(bs[i % 3])
            torch.cuda.synchronize()
            ms[leg].append(1e3 * (time.perf_counter() - t0) / steps)
    med = {leg: statistics.median(x) for leg, x in ms.items()}
    spread = max(ms["plain"]) - min(ms["plain"])
    tr = legs["no_decay_groups"][0]
    say("recorded config-2 step (B = %d), %d alternating windows of %d replays: plain %.3f ms (spread %.3f ms), no_decay_groups %.3f ms "
        "(%d segments over %d floats, %d commands per step against %d); ratio %.4f; slower by more than plain's spread: %s; a second "
        "plain trainer in the same windows: %.3f ms (ratio %.4f)"
        % (B, windows, steps, med["plain"], spread, med["no_decay_groups"], len(tr.opt._segs_host), tr.model._store.n_live, tr._recorded["n_cmds"],
           legs["plain"][0]._recorded["n_cmds"], med["no_decay_groups"] / med["plain"],
           "no" if med["no_decay_groups"] - med["plain"] <= spread else "YES", med["plain again"], med["plain again"] / med["plain"]))
    return med["no_decay_groups"] - med["plain"] <= spread


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="kernel,step")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("param_groups_bench: no GPU (this tool measures the HIP path; there is no fallback)")
    from segmminterest_amd import hipabi as H
    H.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    say("param_groups_bench: %s" % torch.cuda.get_device_name(0))
    ok = True
    what = args.what.split(",")
    if "kernel" in what:
        model = _model(torch, dev)
        model._store.ensure()
        n_live = model._store.n_live
        del model
        torch.cuda.empty_cache()
        for n in (n_live, TABLE):
            ok = kernel(torch, n, args.windows, dev) and ok
    if "step" in what:
        ok = step(torch, args.steps, args.windows, dev) and ok
    say("expectations met: %s" % ("yes" if ok else "NO (see the lines above)"))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
