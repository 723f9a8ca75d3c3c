"""What the streamed attention kernels (csrc/attention_stream.h) cost: forward and phase-0 backward stand-alone, knob ATT_STREAM = 1
against the default at a shape both forms take, and the streamed kernels alone at the largest shape of the opt-in.

    python tools/attn_stream_bench.py [iters] [rounds] [p_drop]

Device events around `iters` back-to-back launches after a warm-up of every form; the two forms alternate over `rounds` so that a
drift of the machine shows as spread, not as a difference.  Operands are column slices of fused projection buffers, as in the engine."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from segmminterest_amd import hipabi as H  # noqa: E402

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 20
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
p_drop = float(sys.argv[3]) if len(sys.argv) > 3 else 0.1
dev = "cuda"


def case(B, Hh, dh, Lq, La, Lb):
    d = Hh * dh
    Yv = torch.randn(B * La, 4 * d, device=dev)
    Yu = torch.randn(B * Lb, 2 * d, device=dev)
    Qs = Yv if Lq == La else torch.randn(B * Lq, 4 * d, device=dev)
    vm = (torch.rand(B, La, device=dev) < 0.8).to(torch.uint8)
    um = (torch.rand(B, Lb, device=dev) < 0.8).to(torch.uint8)
    qm = vm if Lq == La else (torch.rand(B, Lq, device=dev) < 0.8).to(torch.uint8)
    O, lse = torch.empty(B * Lq, d, device=dev), torch.empty(2, B, Hh, Lq, device=dev)
    dO, Dv = torch.randn(B * Lq, d, device=dev), torch.empty(B, Hh, Lq, device=dev)
    dYv, dYu = torch.empty_like(Yv), torch.empty_like(Yu)
    dQs = dYv if Lq == La else torch.empty_like(Qs)
    views = ((Qs, 0), (Qs, d), 4 * d, (Yv, 2 * d), (Yv, 3 * d), 4 * d, (Yu, 0), (Yu, d), 2 * d, qm, vm, um)
    fwd = lambda: H.attn_fwd(B, Hh, dh, Lq, La, Lb, *views, O, d, lse, drop_p=p_drop, seed=1, site=3)
    bwd = lambda: H.attn_bwd(B, Hh, dh, Lq, La, Lb, *views, lse, O, d, dO, d, Dv, (dQs, 0), (dQs, d), 4 * d, (dYv, 2 * d), (dYv, 3 * d),
                             4 * d, (dYu, 0), (dYu, d), 2 * d, drop_p=p_drop, seed=1, site=3, phase=0)
    return fwd, bwd


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def run(shape, forms):
    fwd, bwd = case(*shape)
    res = {(f, k): [] for f in forms for k in ("fwd", "bwd")}
    for r in range(rounds + 1):          # round 0: warm-up of every form
        for f in forms:
            prev = H.config_set("ATT_STREAM", f)
            try:
                for k, fn in (("fwd", fwd), ("bwd", bwd)):
                    us = timed(fn)
                    if r:
                        res[(f, k)].append(us)
            finally:
                H.config_set("ATT_STREAM", prev)
    B, Hh, dh, Lq, La, Lb = shape
    for (f, k), v in res.items():
        flop = (4.0 if k == "fwd" else 14.0) * dh * Lq * (La + Lb) * B * Hh
        print("attn %s %-3s ATT_STREAM=%d p=%.2f  median %9.1f us  (min %9.1f  max %9.1f over %d rounds of %d)  %6.2f TFLOP/s algorithmic"
              % (shape, k, f, p_drop, sorted(v)[len(v) // 2], min(v), max(v), rounds, iters, flop / sorted(v)[len(v) // 2] / 1e6), flush=True)


run((512, 16, 48, 80, 80, 100), (0, 1))          # the largest config-2-like shape the held kernels take
run((512, 16, 48, 256, 256, 100), (0,))          # the opt-in's largest: streamed whatever the knob says
