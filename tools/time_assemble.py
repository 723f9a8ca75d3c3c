"""Rate of the two ways to an index batch at config 2's shape (B = 512, S = 40, Lt = 100, histories of 10 items x up to 40 watched
segments, synthetic interaction table): (a) IndexBatchBuilder.row + .batch on the host, (b) feature_store.DeviceBatches on the
device -- the assemble kernel alone and a whole epoch with its permutation.  Writes the record kept as
profiles/r7/assemble_rate.txt to stdout.

    python tools/time_assemble.py [--rows 32768] [--host-batches 4] [--commit HASH]
"""
import argparse
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from segmminterest_amd import hipabi as H
from segmminterest_amd.feature_store import SITE_ASSEMBLE, DeviceBatches, IndexBatchBuilder, InteractionTable, KeyIndex

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=32768)
ap.add_argument("--host-batches", type=int, default=4)
ap.add_argument("--commit", default="unknown")
a = ap.parse_args()
B, S, Lt, N_ITEMS, N_USERS, N_HIST = 512, 40, 100, 4000, 1000, 10
if a.rows < 55 * B:
    raise SystemExit("time_assemble: --rows >= %d (50 timed batches after 5 of warm-up)" % (55 * B))
if not torch.cuda.is_available():
    raise SystemExit("time_assemble: needs the GPU (a host-only run would time nothing that matters)")

g = np.random.RandomState(1234)
n_fr = g.randint(1, 61, size=N_ITEMS)                                   # segments per item; videos of more than 40 are drawn from
keys = ["%d-%d" % (p, f) for p in range(N_ITEMS) for f in range(n_fr[p]) if f == 0 or g.rand() > 0.01]          # 1 % holes, never frame 0
uid = {str(u): ["%d_0" % g.randint(N_ITEMS) for _ in range(g.randint(0, 9))] for u in range(N_USERS)}
builder = IndexBatchBuilder(KeyIndex(keys), uid, {u: int(u) + 1 for u in uid}, {str(p): p + 1 for p in range(N_ITEMS)}, S=S, Lt=Lt)
line = builder.line
full = [p for p in range(N_ITEMS) if all("%d-%d" % (p, f) in line for f in range(n_fr[p]))]          # videos have every frame
rows = []
for k in range(a.rows):
    p = full[g.randint(len(full))]
    n = int(n_fr[p])
    v = int(g.randint(n))
    hist = g.randint(N_ITEMS, size=N_HIST)
    rows.append(dict(user_id=int(g.randint(N_USERS)), video_id=p, time_ms=k, duration_ms=5000 * n, playing_time=5000 * v,
                     label_1D=[1] * v + [0] + [-1] * (n - v - 1), history_items=[int(x) for x in hist],
                     history_playing=[5000 * int(g.randint(1, min(40, n_fr[x]) + 1)) for x in hist]))
print("index batches at config 2's shape: B = %d, S = %d, Lt = %d; %d synthetic interactions over %d items (1 .. 60 segments, 1 %% holes) and %d users"
      % (B, S, Lt, a.rows, N_ITEMS, N_USERS))
print("(0 .. 8 own frames), histories of %d items x 1 .. 40 watched segments; commit %s" % (N_HIST, a.commit))
print("box: %s (%s), torch %s, hip %s, %s host threads" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName, torch.__version__,
                                                            torch.version.hip, torch.get_num_threads()))

# ---- (a) the host path: IndexBatchBuilder.row per interaction + .batch per 512 (what a user has without the compiled table)
random.seed(1)
np.random.seed(1)
ts = []
for i in range(a.host_batches + 1):
    t0 = time.perf_counter()
    out = builder.batch([builder.row(**r) for r in rows[i * B:(i + 1) * B]])
    ts.append(time.perf_counter() - t0)
ts = ts[1:]
print("(a) host  IndexBatchBuilder.row + .batch: median %8.1f ms per batch of %d  = %9.0f rows/s   (%d batches after one of warm-up; min %.1f max %.1f ms)"
      % (statistics.median(ts) * 1e3, B, B / statistics.median(ts), len(ts), min(ts) * 1e3, max(ts) * 1e3))

# ---- (b) the device path
t0 = time.perf_counter()
table = InteractionTable.compile(builder, rows)
t_compile = time.perf_counter() - t0
dev = torch.device("cuda:0")
table = table.to(dev)
print("    InteractionTable.compile: %.2f s once per split (%.0f rows/s); largest candidate count of a row %d -> the %d-candidate kernel instance"
      % (t_compile, a.rows / t_compile, table.max_cand, 1024 if table.max_cand <= 1024 else H.ASSEMBLE_MAX_CAND))
db = DeviceBatches(table, B, S, Lt, shuffle=True, seed=7)
perm = db.permutation(0)
n_b = len(db)
ids = [perm[k * B:(k + 1) * B] for k in range(n_b)]
desc = table.descriptor()
for k in range(5):
    H.assemble_rows(desc, ids[k], S, Lt, 11, SITE_ASSEMBLE)
torch.cuda.synchronize()
reps = []
for rep in range(5):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(5, n_b):
        keep = H.assemble_rows(desc, ids[k], S, Lt, 11, SITE_ASSEMBLE)
    e1.record()
    torch.cuda.synchronize()
    reps.append(e0.elapsed_time(e1) * 1e3 / (n_b - 5))
us = statistics.median(reps)
drawn_u = float((keep[1] >= 0).sum(1).eq(Lt).float().mean())
print("(b) device segmm_assemble_rows alone (+ its four output allocations): median %7.1f us per batch of %d = %11.0f rows/s   (HIP events over %d batches, "
      "5 repeats: min %.1f max %.1f us; %.0f %% of the last batch's rows have a full user list)"
      % (us, B, B / us * 1e6, n_b - 5, min(reps), max(reps), 100 * drawn_u))
reps = []
for epoch in range(1, 6):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for batch in db(epoch):
        pass
    e1.record()
    torch.cuda.synchronize()
    reps.append(e0.elapsed_time(e1) * 1e3 / n_b)
us_e = statistics.median(reps)
print("    DeviceBatches, a whole epoch (permutation: segmm_rand_ids + segmm_argsort_ids_ws over %d rows; per batch the kernel + the two masks):"
      % a.rows)
print("                                                                   median %7.1f us per batch of %d = %11.0f rows/s   (HIP events around %d batches, "
      "5 epochs: min %.1f max %.1f us)" % (us_e, B, B / us_e * 1e6, n_b, min(reps), max(reps)))
print("one training step at config 2 consumes a batch of 512 in 3.55 - 3.80 ms (README)")
