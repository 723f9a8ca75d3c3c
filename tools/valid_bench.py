#!/usr/bin/env python
"""What a validation pass costs, eager against recorded (Trainer.valid_model(recorded=True)), at the BASELINE config-2 model (D_in = d =
768, N 2, S 40, Lt 100, 16 heads; image inputs on a resident table, index batches): a validation set of 64 batches at B = 128 and at
B = 512, both passes in ONE process, interleaved (profiles/valid_recorded/valid_bench.txt).

Per batch size: two warm-up passes of each kind (the second recorded-kind warm-up is all replays), then ``--reps`` repetitions of
[eager pass, recorded pass].  A pass is timed with the host clock from its first launch to the end of its read-back (both kinds end
in a synchronising copy); the host time per batch of the recorded pass is the time ``valid_enqueue`` takes to return, over the
batches; of the eager pass -- which synchronises inside every batch -- it is the pass over the batches.  Reported: the median wall
time per pass, min and max (the spread), the host time per batch, and the condition "the recorded median is not above the eager
median".  ``permutation=1`` (the default of ``fit``) in both; the shuffles of the eager pass are numpy's, of the recorded pass the
kernel's.

    python tools/valid_bench.py [--batches 64] [--reps 5] [--warmup 2] [--sizes 128,512]

Needs the GPU; there is no fallback."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S, LT, D, N, HEADS, N_LINES = 40, 100, 768, 2, 16, 200000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="128,512")
    args = ap.parse_args()
    import contextlib
    import io
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("valid_bench: no GPU (this tool measures the HIP path; there is no fallback)")
    from segmminterest_amd import hipabi as H
    from segmminterest_amd.feature_store import ResidentFeatureTable
    from segmminterest_amd.synth import make_batch
    from segmminterest_amd.trainer import Trainer, default_args, init_model
    H.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    print("valid_bench: %s, S %d Lt %d D_in %d d %d N %d heads %d, table %d lines, %d batches per pass, %d repetitions after %d warm-ups, permutation=1"
          % (torch.cuda.get_device_name(0), S, LT, D, D, N, HEADS, N_LINES, args.batches, args.reps, args.warmup))
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
            batches.append({k: v.to(dev) for k, v in b.items()})
        torch.manual_seed(1234)
        model = init_model(margs, n_users=1903, n_items=352494, input_dim=D, max_vid_len=S, max_usr_len=LT).to(dev)
        tr = Trainer(model, feature_table=table, device_state=True)

        def eager():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):          # (the eager pass prints every batch's metrics)
                m = tr.valid_model(batches, permutation=1)
            t1 = time.perf_counter()
            return t1 - t0, (t1 - t0) / len(batches), m

        def recorded():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            acc = tr.valid_enqueue(batches, permutation=1)
            t1 = time.perf_counter()
            m = acc.finish()
            t2 = time.perf_counter()
            return t2 - t0, (t1 - t0) / len(batches), m

        for _ in range(args.warmup):
            me, mr = eager()[2], recorded()[2]
        if me["valid_loss"] != mr["valid_loss"]:
            ok = False
            print("B %4d  MISMATCH: valid_loss eager %r recorded %r" % (B, me["valid_loss"], mr["valid_loss"]))
        t = {"eager": [], "recorded": []}
        host = {"eager": [], "recorded": []}
        for _ in range(args.reps):          # the two kinds alternate inside every repetition
            for k, fn in (("eager", eager), ("recorded", recorded)):
                wall, per_batch, _m = fn()
                t[k].append(wall)
                host[k].append(per_batch)
        for k in ("eager", "recorded"):
            print("B %4d  %-8s pass  median %8.2f ms  (min %8.2f max %8.2f over %d passes of %d batches)  %7.3f ms/batch  host %7.3f ms/batch"
                  % (B, k, 1e3 * statistics.median(t[k]), 1e3 * min(t[k]), 1e3 * max(t[k]), args.reps, args.batches,
                     1e3 * statistics.median(t[k]) / args.batches, 1e3 * statistics.median(host[k])))
        me_, mr_ = statistics.median(t["eager"]), statistics.median(t["recorded"])
        print("B %4d  recorded / eager = %.3f; condition recorded median %.2f ms <= eager median %.2f ms: %s; valid_loss equal: %s; "
              "NDCG@5 eager %.4f recorded %.4f; %d commands per replay"
              % (B, mr_ / me_, 1e3 * mr_, 1e3 * me_, "PASS" if mr_ <= me_ else "FAIL", me["valid_loss"] == mr["valid_loss"], me["NDCG@5"], mr["NDCG@5"],
                 tr._valid_rec["n_cmds"]))
        ok = ok and mr_ <= me_
        del tr, model, batches
        torch.cuda.empty_cache()
    torch.cuda.synchronize()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
