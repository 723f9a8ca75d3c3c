"""Time of the SegRec head's three ways from stored logits to [B, I] predictions at S = 40, for a training shape (B = 256, I = 2) and a
test_all-like shape (B = 256, I = 20 000: 0.8 GB of pred), no negatives file:
  (a) DeviceLogitStore: segmm_store_lookup + segmm_store_head (weights read from the store's rows, no [B, I, S] weight tensor),
  (b) segmm_segment_weighted_sum on a [B, I, S] weight tensor that is already on the device (the head alone, as it was),
  (c) LogitStore.weights(..., device=) + weighted_head per batch, wall time (numpy lookup, [B, I, S] built on the host and copied).
(a) and (b) alternate inside every repeat.  Writes the record kept as profiles/r7/store_head_rate.txt to stdout.

    python tools/time_store_head.py [--keys 1000000] [--commit HASH]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from segmminterest_amd import hipabi as H
from segmminterest_amd.bridge import DeviceLogitStore, weighted_head

ap = argparse.ArgumentParser()
ap.add_argument("--keys", type=int, default=1000000)
ap.add_argument("--commit", default="unknown")
ap.add_argument("--shapes", default="256x2,256x20000")
a = ap.parse_args()
S = 40
if not torch.cuda.is_available():
    raise SystemExit("time_store_head: needs the GPU (a host-only run would time nothing that matters)")
dev = torch.device("cuda:0")
print("SegRec head from stored logits, S = %d; store of %d keys (users < 2^20, items < 2^22, time_ms near 10^12) added in batches of 4096; commit %s"
      % (S, a.keys, a.commit))
print("box: %s (%s), torch %s, hip %s, %s host threads" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName, torch.__version__,
                                                            torch.version.hip, torch.get_num_threads()))

g = torch.Generator(device=dev).manual_seed(1234)
store = DeviceLogitStore(S=S, device=dev)
ku = torch.randint(0, 1 << 20, (a.keys,), generator=g, device=dev)
kp = torch.randint(0, 1 << 22, (a.keys,), generator=g, device=dev)
kt = 10 ** 12 + torch.randint(0, 1 << 30, (a.keys,), generator=g, device=dev)
for k0 in range(0, a.keys, 4096):
    store.add_batch(ku[k0:k0 + 4096], kp[k0:k0 + 4096], kt[k0:k0 + 4096], torch.randn(min(4096, a.keys - k0), S, generator=g, device=dev))
t0 = time.perf_counter()
store.finalize()
torch.cuda.synchronize()
print("    DeviceLogitStore.finalize (keys to the host, lexsort, index back up): %.2f s once" % (time.perf_counter() - t0))
host = store.to_store()
host._build_index()


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / inner


def line(tag, what, us, nbytes, note):
    m = statistics.median(us)
    print("%s %-78s median %9.1f us  = %7.1f GB/s of pred   (%s; min %.1f max %.1f us)" % (tag, what, m, nbytes / m * 1e-3, note, min(us), max(us)))
    return m


for shape in a.shapes.split(","):
    B, I = (int(x) for x in shape.split("x"))
    pick = torch.randint(0, a.keys, (B,), generator=g, device=dev)
    user, time_ms = ku[pick].clone(), kt[pick].clone()
    item = torch.randint(0, 1 << 22, (B, I), generator=g, device=dev)
    item[:, 0] = kp[pick]
    user[::10] = (1 << 20) + 5          # one target in ten is not in the store: ones
    pred = torch.randn(B, I, S, generator=g, device=dev)
    dur = torch.randint(1, S + 1, (B, I), generator=g, device=dev)
    vals = store._cat()[1]
    nbytes = pred.numel() * 4
    print("---- B = %d, I = %d: pred %.1f MB, duration int64 [B, I]" % (B, I, nbytes / 1e6))

    def new_path():
        rowidx, miss = store.lookup(user, item, time_ms, check=False)
        return H.store_head(pred, rowidx, vals, None, dur)

    weight = store.weights(user, item, time_ms)

    def old_head():
        return H.segment_weighted_sum(pred, weight, dur)

    rowidx = store.lookup(user, item, time_ms)
    inner = max(3, min(200, int(2e9 // nbytes)))
    for _ in range(3):
        got, ref = new_path(), old_head()
    torch.cuda.synchronize()
    diff = float((got - ref).abs().max())
    ra, rb, rl, rh = [], [], [], []
    for rep in range(7):
        ra.append(timed(new_path, inner))
        rb.append(timed(old_head, inner))
        rl.append(timed(lambda: store.lookup(user, item, time_ms, check=False), inner))
        rh.append(timed(lambda: H.store_head(pred, rowidx, vals, None, dur), inner))
    ma = line("(a)", "device segmm_store_lookup + segmm_store_head (reads pred + rowidx + duration)", ra, nbytes, "HIP events over %d calls, 7 repeats" % inner)
    line("   ", "    of which segmm_store_lookup (+ its two output allocations)", rl, nbytes, "same")
    line("   ", "    of which segmm_store_head", rh, nbytes, "same")
    mb = line("(b)", "device segmm_segment_weighted_sum on a resident [B, I, S] weight (reads pred + weight)", rb, nbytes, "alternating with (a)")
    spread = max(max(ra) - min(ra), max(rb) - min(rb))
    print("    (a) - (b) = %+.1f us, run-to-run spread of the repeats %.1f us: (a) is %s; max |(a) - (b)| over the outputs %.2e"
          % (ma - mb, spread, "no slower than (b)" if ma - mb <= spread else "SLOWER than (b)", diff))
    tc = []
    for rep in range(2 if nbytes > 1e8 else 6):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = weighted_head(pred, host.weights(user.cpu().numpy(), item.cpu().numpy(), time_ms.cpu().numpy(), device=dev), dur)
        torch.cuda.synchronize()
        tc.append((time.perf_counter() - t0) * 1e6)
    tc = tc[1:]
    print("(c) host  LogitStore.weights(..., device=) + weighted_head, wall time per batch %39s %9.1f us  (for the record; %d batches after one of warm-up)"
          % ("median", statistics.median(tc), len(tc)))
    del weight, pred, out, got, ref
