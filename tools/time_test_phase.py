"""Wall time of Trainer.test_model over the same test batches with the per-row metrics on the host (the reference's row loop in
main_eval_batch) and on the device (device_metrics=True).  Writes the record kept as profiles/test_phase_metrics.txt to stdout.

    python tools/time_test_phase.py [--batches 20] [--repeats 5]
"""
import argparse
import contextlib
import io
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from segmminterest_amd.synth import make_batch
from segmminterest_amd.trainer import Trainer, default_args, init_model

ap = argparse.ArgumentParser()
ap.add_argument("--batches", type=int, default=20)
ap.add_argument("--repeats", type=int, default=5)
a = ap.parse_args()

dev = torch.device("cuda:0")
B, S, D, Lt, N, h = 512, 40, 768, 100, 2, 16
EVALS = ["JaccardSim", "LeaveMSE", "LeaveCTR", "LeaveCTR_view", "TOP_K"]          # the reference's default --eval_type_list
margs = default_args(num_layers_enc=N, d_model=D, nhead=h, input_type={"user": "image", "photo": "image"}, exposure_prob=[1.0] * S)
torch.manual_seed(1234)
model = init_model(margs, n_users=1, n_items=1, input_dim=D, max_vid_len=S, max_usr_len=Lt).to(dev)
batches = [{k: v.to(dev) for k, v in make_batch(B, S, Lt, D, n_items=20000, seed=1234 + i).items()} for i in range(a.batches)]
seen = set(int(p) for b in batches[: a.batches // 2] for p in b["photo_id"].tolist())
tr = Trainer(model)


def timed(**kw):
    ts = []
    with contextlib.redirect_stdout(io.StringIO()):          # (TOP_K prints its dict per batch, like the reference)
        tr.test_model(batches, EVALS, top_k_permutation=0, **kw)          # warm-up pass
        torch.cuda.synchronize()
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            res = tr.test_model(batches, EVALS, top_k_permutation=0, **kw)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
    return ts, res


print("Trainer.test_model, %d batches of %d x %d rows (config 2: D = d = %d, h = %d, N = %d, Lt = %d, image / image), eval_type_list %s,"
      % (a.batches, B, S, D, h, N, Lt, ",".join(EVALS)))
print("top_k_permutation=0; one warm-up pass, then %d timed passes over the same batches; wall ms per pass, synchronised." % a.repeats)
print("box: %s (%s), torch %s, hip %s, %s host threads" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName, torch.__version__,
                                                            torch.version.hip, torch.get_num_threads()))
for cold in (False, True):
    kw = {"train_videos": seen} if cold else {}
    out = {}
    for flag in (False, True):
        ts, res = timed(device_metrics=flag, **kw)
        out[flag] = res
        print("%-26s device_metrics=%-5s median %9.1f ms  min %9.1f  max %9.1f  (%.2f ms per batch)"
              % ("with train_videos (cold/hot)" if cold else "plain", flag, statistics.median(ts), min(ts), max(ts), statistics.median(ts) / a.batches))
    for part in ("final", "cold_final", "hot_final") if cold else ("final",):
        print("  %-10s host   %s" % (part, {k: round(float(v), 6) for k, v in sorted(out[False][part].items()) if k in EVALS}))
        print("  %-10s device %s" % (part, {k: round(float(v), 6) for k, v in sorted(out[True][part].items()) if k in EVALS}))
