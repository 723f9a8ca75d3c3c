"""What the attention kernels cost at wide heads: forward and fused (phase 4) backward stand-alone at (B, H, dh) = (512, 8, 96),
(512, 8, 128) and, for comparison, (512, 16, 48) and (512, 16, 64) -- dh = 128, H = 8 against dh = 64, H = 16 is d = 1024 both
ways: equal FLOPs, equal bytes -- for video queries (Lq, La, Lb) = (40, 40, 100) and user queries (100, 40, 100).

    python tools/attn_wide_bench.py [iters] [rounds] [p_drop]

The timing scheme of tools/attn_stream_bench.py: device events around `iters` back-to-back launches after a warm-up of every
form; the widths alternate over `rounds` so that a drift of the machine shows as spread, not as a difference.  Operands are column
slices of fused projection buffers, as in the engine.  Every library knob at its default."""
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
HEADS = ((512, 8, 96), (512, 8, 128), (512, 16, 48), (512, 16, 64))
TOKENS = ((40, 40, 100), (100, 40, 100))


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
                             4 * d, (dYu, 0), (dYu, d), 2 * d, drop_p=p_drop, seed=1, site=3, phase=4)
    return fwd, bwd


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


for tok in TOKENS:
    cases = {hd: case(*hd, *tok) for hd in HEADS}
    res = {(hd, k): [] for hd in HEADS for k in ("fwd", "bwd4")}
    for r in range(rounds + 1):          # round 0: warm-up of every form
        for hd in HEADS:
            for k, fn in zip(("fwd", "bwd4"), cases[hd]):
                us = timed(fn)
                if r:
                    res[(hd, k)].append(us)
    med = {}
    for (hd, k), v in res.items():
        B, Hh, dh = hd
        Lq, La, Lb = tok
        flop = (4.0 if k == "fwd" else 14.0) * dh * Lq * (La + Lb) * B * Hh
        med[(hd, k)] = sorted(v)[len(v) // 2]
        print("attn (B, H, dh) = %-14s (Lq, La, Lb) = %-14s %-4s p=%.2f  median %9.1f us  (min %9.1f  max %9.1f over %d rounds of %d)  %6.2f TFLOP/s algorithmic"
              % (hd, tok, k, p_drop, med[(hd, k)], min(v), max(v), rounds, iters, flop / med[(hd, k)] / 1e6), flush=True)
    for k in ("fwd", "bwd4"):
        print("attn ratio dh = 128, H = 8 over dh = 64, H = 16 at d = 1024, %s, %-4s: %.2f" % (tok, k, med[((512, 8, 128), k)] / med[((512, 16, 64), k)]), flush=True)
    del cases
    torch.cuda.empty_cache()
