#!/usr/bin/env python
"""What a logit dump costs, eager against recorded (Trainer.dump_logits(recorded=True)), and what the store's index build costs, on
the host against on the device (DeviceLogitStore.finalize(on_device=True)) -- profiles/dump_recorded/dump_bench.txt.

The dump: the BASELINE config-2 model (D_in = d = 768, N 2, S 40, Lt 100, 16 heads; image inputs on a resident table, index batches
with the three key columns on the device), a split of 64 batches at B = 128 and at B = 512, both kinds in ONE process, in
alternating windows.  Per batch size: ``--warmup`` passes of each kind (the second recorded-kind warm-up is all replays), then
``--reps`` repetitions of [eager pass, recorded pass].  A pass is timed with the host clock from its first launch to the end of a
device synchronise behind its last; the host time per batch is the time ``dump_logits`` takes to return (neither kind synchronises
inside the pass), over the batches.  Reported: the median wall time per pass, min and max (the spread), the host time per batch, and
the condition "the recorded median is not above the eager median by more than the eager leg's own spread (max - min) in this run".
The two stores are compared bit for bit first.

The index: 2^16, 2^20 and 2^22 random keys (time_ms near 1.7e12) of which about 1 % repeat an earlier key; ``finalize()`` (one copy
of the keys to the host, numpy's lexsort there, the index back up) against ``finalize(on_device=True)`` (segmm_store_index and an
8-byte read-back) on the same store, alternating, each from its call to the end of a device synchronise; the two indices are
compared first.

    python tools/dump_bench.py [--batches 64] [--reps 5] [--warmup 2] [--sizes 128,512] [--index-sizes 65536,1048576,4194304] [--index-reps 3]

Needs the GPU; there is no fallback."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S, LT, D, N, HEADS, N_LINES = 40, 100, 768, 2, 16, 200000
T0 = 1_700_000_000_000


def _same(a, b):
    import torch
    (ka, va), (kb, vb) = a._cat(), b._cat()
    return len(a) == len(b) and torch.equal(ka, kb) and torch.equal(va.view(torch.int32), vb.view(torch.int32))


def dump_part(args, torch, dev):
    from segmminterest_amd.feature_store import ResidentFeatureTable
    from segmminterest_amd.synth import make_batch
    from segmminterest_amd.trainer import Trainer, default_args, init_model
    table = ResidentFeatureTable(torch.rand((N_LINES, D), generator=torch.Generator().manual_seed(99)).to(dev))
    margs = default_args(num_layers_enc=N, d_model=D, nhead=HEADS, input_type={"user": "image", "photo": "image"}, exposure_prob=[1.0] * S)
    ok = True
    for B in (int(x) for x in args.sizes.split(",")):
        batches = []
        for i in range(args.batches):
            b = make_batch(B, S, LT, D, seed=1234 + 1000 * i, features=False)
            g2 = torch.Generator().manual_seed(4321 + 1000 * i)
            pidx = torch.randint(0, N_LINES, (B, S), generator=g2)
            pidx[~b["photo_mask"]] = -1
            uidx = torch.randint(0, N_LINES, (B, LT), generator=g2)
            uidx[~b["user_mask"]] = -1
            b["photo_idx"], b["user_idx"] = pidx, uidx
            b["time_ms"] = b["time_ms"] + T0
            batches.append({k: v.to(dev) for k, v in b.items()})
        torch.manual_seed(1234)
        model = init_model(margs, n_users=1903, n_items=352494, input_dim=D, max_vid_len=S, max_usr_len=LT).to(dev)
        tr = Trainer(model, feature_table=table, device_state=True)

        def one(recorded):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st = tr.dump_logits([batches], recorded=recorded)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            return t2 - t0, (t1 - t0) / len(batches), st

        for _ in range(args.warmup):
            se, sr = one(False)[2], one(True)[2]
        same = _same(se, sr)
        if not same:
            ok = False
            print("B %4d  MISMATCH: the recorded store is not the eager store" % B)
        del se, sr
        t = {"eager": [], "recorded": []}
        host = {"eager": [], "recorded": []}
        for _ in range(args.reps):          # the two kinds alternate inside every repetition
            for k, rec in (("eager", False), ("recorded", True)):
                wall, per_batch, _st = one(rec)
                del _st
                t[k].append(wall)
                host[k].append(per_batch)
        for k in ("eager", "recorded"):
            print("B %4d  %-8s pass  median %8.2f ms  (min %8.2f max %8.2f over %d passes of %d batches)  %7.3f ms/batch  host %7.3f ms/batch"
                  % (B, k, 1e3 * statistics.median(t[k]), 1e3 * min(t[k]), 1e3 * max(t[k]), args.reps, args.batches,
                     1e3 * statistics.median(t[k]) / args.batches, 1e3 * statistics.median(host[k])))
        me_, mr_ = statistics.median(t["eager"]), statistics.median(t["recorded"])
        spread = max(t["eager"]) - min(t["eager"])
        good = mr_ <= me_ + spread
        print("B %4d  recorded / eager = %.3f; condition recorded median %.2f ms <= eager median %.2f ms + eager spread %.2f ms: %s; stores equal: %s; "
              "%d commands per replay, %d replays" % (B, mr_ / me_, 1e3 * mr_, 1e3 * me_, 1e3 * spread, "PASS" if good else "FAIL", same,
                                                      tr._dump_rec["n_cmds"], tr._dump_rec["n_replays"]))
        ok = ok and good
        del tr, model, batches
        torch.cuda.empty_cache()
    return ok


def index_part(args, torch, dev):
    import numpy as np
    from segmminterest_amd.bridge import DeviceLogitStore
    ok = True
    for n in (int(x) for x in args.index_sizes.split(",")):
        rng = np.random.default_rng(n)
        k = np.stack([rng.integers(1, 2_000_000, n), rng.integers(1, 400_000, n), T0 + rng.integers(0, 10 ** 10, n)], 1).astype(np.int64)
        d = np.nonzero(rng.random(n) < 0.01)[0]
        d = d[d > 0]
        k[d] = k[rng.integers(0, d)]          # about 1 % of the rows repeat an EARLIER row's key
        st = DeviceLogitStore(S=1, device=dev)
        st._keys, st._vals = [torch.from_numpy(k).to(dev)], [torch.zeros((n, 1), device=dev)]

        def one(on_device):
            st._index = None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st.finalize(on_device=on_device)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, st._index

        (_, ih), (_, idv) = one(False), one(True)          # (also the warm-up of both)
        same = torch.equal(ih[0], idv[0]) and torch.equal(ih[1], idv[1])
        ok = ok and same
        m = ih[0].shape[0]
        del ih, idv
        t = {"host": [], "device": []}
        for _ in range(args.index_reps):
            for kind, od in (("host", False), ("device", True)):
                t[kind].append(one(od)[0])
        print("index n %8d (%8d distinct)  host finalize() median %9.2f ms (min %9.2f max %9.2f)  on_device median %8.3f ms (min %8.3f max %8.3f) "
              "over %d alternating runs; indices equal: %s"
              % (n, m, 1e3 * statistics.median(t["host"]), 1e3 * min(t["host"]), 1e3 * max(t["host"]), 1e3 * statistics.median(t["device"]),
                 1e3 * min(t["device"]), 1e3 * max(t["device"]), args.index_reps, same))
        del st
        torch.cuda.empty_cache()
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="128,512")
    ap.add_argument("--index-sizes", default="65536,1048576,4194304")
    ap.add_argument("--index-reps", type=int, default=3)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("dump_bench: no GPU (this tool measures the HIP path; there is no fallback)")
    from segmminterest_amd import hipabi as H
    H.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    print("dump_bench: %s, S %d Lt %d D_in %d d %d N %d heads %d, table %d lines, %d batches per pass, %d repetitions after %d warm-ups"
          % (torch.cuda.get_device_name(0), S, LT, D, D, N, HEADS, N_LINES, args.batches, args.reps, args.warmup))
    ok = dump_part(args, torch, dev) if args.sizes else True
    ok = (index_part(args, torch, dev) if args.index_sizes else True) and ok
    torch.cuda.synchronize()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
