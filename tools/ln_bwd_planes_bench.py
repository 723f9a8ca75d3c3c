"""What the fp32 copy of an embedding LayerNorm's input gradient costs: segmm_layernorm_bwd_pos stand-alone at the two config-2
embedding shapes, with dx and planes-only (dx = None), plus the repair launch of a good site (workgroups that leave at once).

    python tools/ln_bwd_planes_bench.py [iters] [rounds] [p_drop]

Device events around `iters` back-to-back launches after a warm-up of every form; the forms alternate over `rounds` so that a
drift of the machine shows as spread, not as a difference (tools/attn_stream_bench.py)."""
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


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def run(rows, d, period):
    x, dy = torch.randn(rows, d, device=dev), torch.randn(rows, d, device=dev) * 0.01
    gamma, beta = torch.ones(d, device=dev), torch.zeros(d, device=dev)
    y, mean, rstd = torch.empty(rows, d, device=dev), torch.empty(rows, device=dev), torch.empty(rows, device=dev)
    H.layernorm_fwd(x, gamma, beta, y, mean, rstd)
    parts = H.layernorm_bwd_pos_parts(rows, period, d)
    dx = torch.empty(rows, d, device=dev)
    pg, pb, pp = (torch.empty(n, d, device=dev) for n in (parts, parts, 4 * parts))
    planes = torch.empty(rows, 2 * d, dtype=torch.float16, device=dev)
    hdr = H.new_site(dev)[0]
    sc = torch.ones(1, device=dev)
    po = H.PO(planes, 2 * d, hdr, sc.data_ptr())
    kw = dict(drop_y_p=p_drop, drop_y_site=3, seed=1)

    def bwd(out):
        return lambda: H.layernorm_bwd_pos(dy, x, mean, rstd, gamma, out, None, pg, pb, pp, period, amax=hdr[H.SITE_HDR:], po=po, **kw)
    bwd(dx)()          # the scale that fits this dx: 2^14 <= max * s < 2^15
    torch.cuda.synchronize()
    m = float(hdr[H.SITE_HDR:].max())
    sc.fill_(2.0 ** (14 - int(torch.tensor(m).log2().floor())))
    hdr.zero_()
    forms = (("with dx", bwd(dx)), ("planes only", bwd(None)), ("repair, good site", lambda: H.layernorm_bwd_pos_repair(dy, x, mean, rstd, gamma, period, po, **kw)))
    res = {k: [] for k, _ in forms}
    for r in range(rounds + 1):          # round 0: warm-up of every form
        for k, fn in forms:
            us = timed(fn)
            if r:
                res[k].append(us)
    assert float(hdr[1]) == 0.0 and float(hdr[2]) == 0.0
    mb = rows * d * 4 / 1e6
    for k, v in res.items():
        med = sorted(v)[len(v) // 2]
        moved = {"with dx": 4 * mb, "planes only": 3 * mb, "repair, good site": 0.0}[k]
        print("layernorm_bwd_pos (%d, %d, period %d) p=%.2f  %-18s median %7.1f us  (min %7.1f  max %7.1f over %d rounds of %d)  %5.2f TB/s"
              % (rows, d, period, p_drop, k, med, min(v), max(v), rounds, iters, moved / med), flush=True)


run(51200, 768, 100)          # config 2, user side
run(20480, 768, 40)           # config 2, video side
