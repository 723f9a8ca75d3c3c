"""What a feed-forward width other than d_model costs at BASELINE config 2 (B = 512, S = 40, Lt = 100, d = D_in = 768, h = 16,
N = 2: the video side of layer 0 is the only live FFN, M = 20480 tokens), for ff in {768, 1536, 3072}.

    python tools/ffn_width_bench.py [iters] [rounds]  >  profiles/ffn_width_bench.txt

Part 1, stand-alone launches: the four FFN GEMMs of a side (forward W0 with GELU + aux + dropout + plane output, forward W1 with bias
+ residual + dropout, the DGELU input gradient, dX1 with the residual) and the two weight gradients (split-K + splitk_reduce; W0's
with the folded bias gradient), each with the arguments the engine passes.  Device events around ``iters`` back-to-back launches;
the forms alternate over ``rounds`` (+ one warm-up round) so that a drift of the machine shows as spread, not as a difference.
TFLOP/s are algorithmic (2 M N K) against the 833 TF bound of three fp16 MFMA products per fp32 product.  The kernel named is the
one the launcher's rule gives for the shape (``nt_kernel`` / ``tn_kernel`` below restate segmm_gemm_p's choice, capi.hip).

Part 2, the whole recorded train step (Trainer(device_state=True).record(), FusedAdamW, dropout on) at the same widths: ms per
step next to the algorithmic FLOPs per step (bench.f_train_flops + 12 d (ff - d) S per interaction), both relative to ff = d."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from segmminterest_amd import engine as E  # noqa: E402
from segmminterest_amd import hipabi as H  # noqa: E402

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 20
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
dev = "cuda"
PEAK_F16X3 = 833.0
B, S, Lt, D, HEADS, N = 512, 40, 100, 768, 16, 2
WIDTHS = (768, 1536, 3072)


def nt_kernel(M, N_, K):
    """segmm_gemm_p, NT form, default knobs (PL_VAR 4): gemm_pl_nt4 for K >= 768 and N >= 768, else gemm_pl_nt8 at the tile width
    (64 NJ columns) that needs the fewest CU rounds."""
    if K >= 768 and N_ >= 768:
        return "gemm_pl_nt4"
    best, best_cost, bm = 4, 0.0, (M + 255) // 256
    for nj in (4, 3, 2):
        tiles = bm * ((N_ + 64 * nj - 1) // (64 * nj))
        cost = ((tiles + 255) // 256) * (15.0 + 11.4 * nj * (K / 768.0))
        if nj == 4 or cost < 0.93 * best_cost:
            best, best_cost = nj, cost
    return "gemm_pl_nt8<%d>" % best


def tn_kernel(M, N_):
    """segmm_gemm_p, TN form, default knobs (TN_VAR 8): gemm_pl_tn4 (whole 128 x 256 tiles) for few-tile matrices of width >= 768 and
    for what is no whole 256 x 256 tiling, gemm_pl_tn8 for whole 256 x 256 tiles, else the round-2 gemm_pl_tn."""
    fits8, fits4 = M % 256 == 0 and N_ % 256 == 0, M % 128 == 0 and N_ % 256 == 0
    few = ((M + 255) // 256) * ((N_ + 255) // 256) <= 9 and M >= 768 and N_ >= 768
    if fits4 and (few or not fits8):
        return "gemm_pl_tn4"
    return "gemm_pl_tn8" if fits8 else "gemm_pl_tn"


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def po_for(x, rows, cols):
    """A plane output with the scale that fits ``x`` (2^14 <= max * s < 2^15), as a calibrated site has it."""
    hdr = H.new_site(dev)[0]
    s = 2.0 ** (14 - int(torch.log2(x.abs().max()).floor()))
    sc = torch.tensor([s], dtype=torch.float32, device=dev)
    pl = torch.empty((rows, 2 * cols), dtype=torch.float16, device=dev)
    return pl, hdr, sc


def standalone(M, d, ff, split_target, split_few):
    g = torch.Generator(device="cpu").manual_seed(ff)
    r = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(dev)
    X1, W0, W1, b0, b1 = r(M, d), r(ff, d, scale=0.04), r(d, ff, scale=0.04), r(ff, scale=0.02), r(d, scale=0.02)
    dM, res = r(M, d, scale=0.01), r(M, d)
    pX1, pdM = H.to_planes(X1, M, d), H.to_planes(dM, M, d)
    pW0, pW1 = H.to_planes(W0, ff, d, keep_f32=False), H.to_planes(W1, d, ff, keep_f32=False)
    pW0T, pW1T = H.to_planes(W0.t().contiguous(), d, ff, keep_f32=False), H.to_planes(W1.t().contiguous(), ff, d, keep_f32=False)
    Hh, G, R2, dG, dX1 = (torch.empty(M, n, device=dev) for n in (ff, ff, d, ff, d))
    gW0, gW1, gb0 = torch.empty(ff, d, device=dev), torch.empty(d, ff, device=dev), torch.empty(ff, device=dev)
    # one exact pass of the two plane-output launches: the values the delayed scales are taken from
    H.gemm(H.LAYOUT_NT, M, ff, d, X1, d, W0, d, Hh, ff, bias=b0, activation=H.ACT_GELU, aux=G, ldaux=ff, drop_p=0.1, seed=3, site=7)
    H.gemm(H.LAYOUT_NN, M, ff, d, dM, d, W1, ff, dG, ff, activation=H.ACT_DGELU, aux=G, ldaux=ff, drop_p=0.1, seed=3, site=7)
    torch.cuda.synchronize()
    plH, hdrH, scH = po_for(Hh, M, ff)
    plG, hdrG, scG = po_for(dG, M, ff)
    ptH, ptG = H.PT(plH, hdrH, M, ff, f32=Hh), H.PT(plG, hdrG, M, ff, f32=dG)
    s1 = E._splits_for_p(d, ff, M, split_target, split_few)
    s0 = E._splits_for_p(ff, d, M, split_target, split_few)
    ws = torch.empty(max(s0, s1, 1) * (ff * d + ff + d), device=dev)
    forms = (
        ("fwd W0  gelu+aux+drop+planes", (M, ff, d), nt_kernel(M, ff, d),
         lambda: H.gemm_p(H.LAYOUT_NT, M, ff, d, pX1, pW0, Hh, ff, c_pt=ptH, c_scale_ptr=scH.data_ptr(), bias=b0, activation=H.ACT_GELU,
                          aux=G, ldaux=ff, drop_p=0.1, seed=3, site=7)),
        ("fwd W1  bias+res+drop", (M, d, ff), nt_kernel(M, d, ff),
         lambda: H.gemm_p(H.LAYOUT_NT, M, d, ff, ptH, pW1, R2, d, bias=b1, residual=res, ldr=d, res_period=M, drop_p=0.1, seed=3, site=9)),
        ("dgrad W1  dgelu+drop+planes", (M, ff, d), nt_kernel(M, ff, d),
         lambda: H.gemm_p(H.LAYOUT_NT, M, ff, d, pdM, pW1T, dG, ff, c_pt=ptG, c_scale_ptr=scG.data_ptr(), activation=H.ACT_DGELU, aux=G,
                          ldaux=ff, drop_p=0.1, seed=3, site=7)),
        ("dgrad W0  +res (dX1)", (M, d, ff), nt_kernel(M, d, ff),
         lambda: H.gemm_p(H.LAYOUT_NT, M, d, ff, ptG, pW0T, dX1, d, residual=res, ldr=d, res_period=M)),
        ("wgrad W1 [d, ff]  splits %d" % s1, (d, ff, M), tn_kernel(d, ff) + (" + splitk_reduce" if s1 > 1 else ""),
         lambda: H.gemm_p(H.LAYOUT_TN, d, ff, M, pdM, ptH, gW1, ff, splits=s1, workspace=ws if s1 > 1 else None)),
        ("wgrad W0 [ff, d] + bias  splits %d" % s0, (ff, d, M), tn_kernel(ff, d) + (" + splitk_reduce" if s0 > 1 else ""),
         lambda: H.gemm_p(H.LAYOUT_TN, ff, d, M, ptG, pX1, gW0, d, splits=s0, workspace=ws if s0 > 1 else None, colsum_out=gb0)),
    )
    res_us = {k: [] for k, *_ in forms}
    for rnd in range(rounds + 1):          # round 0: warm-up of every form
        for k, _, _, fn in forms:
            us = timed(fn)
            if rnd:
                res_us[k].append(us)
    assert float(hdrH[1]) == 0.0 and float(hdrG[1]) == 0.0, "a plane output left its scale window"
    total = 0.0
    for k, (m_, n_, k_), kern, _ in forms:
        v = res_us[k]
        med = sorted(v)[len(v) // 2]
        total += med
        tf = 2.0 * m_ * n_ * k_ / med / 1e6
        print("ff %4d  %-34s (%5d, %4d, %5d)  %-30s median %7.1f us  (min %7.1f  max %7.1f over %d rounds of %d)  %6.1f TFLOP/s = %4.1f %% of %d"
              % (ff, k, m_, n_, k_, kern, med, min(v), max(v), rounds, iters, tf, 100 * tf / PEAK_F16X3, PEAK_F16X3), flush=True)
    return total


def step_flops(ff):
    import bench
    return B * (bench.f_train_flops(D, D, S, Lt, N) + 12 * D * (ff - D) * S)


def whole_step(ff):
    from segmminterest_amd.synth import make_batch
    from segmminterest_amd.trainer import Trainer, default_args, init_model
    margs = default_args(num_layers_enc=N, d_model=D, nhead=HEADS, input_type={"user": "image", "photo": "image"}, exposure_prob=[1.0] * S)
    torch.manual_seed(1234)
    model = init_model(margs, n_users=1903, n_items=352494, input_dim=D, max_vid_len=S, max_usr_len=Lt, ff_dim=[ff] * N).to(dev)
    tr = Trainer(model, lr=1e-3, weight_decay=1e-4, device_state=True)
    batches = [{k: v.to(dev) for k, v in make_batch(B, S, Lt, D, n_users=1903, n_items=352494, seed=1234 + 1000 * i).items()} for i in range(4)]
    for i in range(3):
        tr.train_step(batches[i % 4])
    tr.record(batches[0], warmup=2)
    ms = []
    for rnd in range(rounds + 1):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(iters):
            out = tr.run_recorded(batches[i % 4])
        e1.record()
        torch.cuda.synchronize()
        if rnd:
            ms.append(e0.elapsed_time(e1) / iters)
    assert bool(torch.isfinite(out["loss"]).all())
    return sorted(ms)[len(ms) // 2], min(ms), max(ms), model._store.overflow_count()


def main():
    H.lib()
    st_target, st_few = None, None
    from segmminterest_amd import switches
    sw = switches.read("engine")
    st_target, st_few = sw["split_target_p"], sw["split_target_few"]
    print("# ffn_width_bench: M = %d video tokens, d = %d; %d rounds of %d launches; %s" % (B * S, D, rounds, iters, torch.cuda.get_device_name(0)))
    print("# part 1: stand-alone FFN launches of one side")
    totals = {}
    for ff in WIDTHS:
        totals[ff] = standalone(B * S, D, ff, st_target, st_few)
        print("ff %4d  sum of the six medians %8.1f us  (x %.2f of ff = %d; FFN FLOPs x %.2f)" % (ff, totals[ff], totals[ff] / totals[WIDTHS[0]], WIDTHS[0], ff / WIDTHS[0]), flush=True)
    print("# part 2: whole recorded train step, config 2 with ff_dim = ff")
    base = None
    for ff in WIDTHS:
        med, lo, hi, ovf = whole_step(ff)
        fl = step_flops(ff)
        base = base or (med, fl)
        print("ff %4d  recorded step median %7.3f ms  (min %7.3f  max %7.3f over %d rounds of %d)  %8.0f interactions/s  x %.3f time for x %.3f "
              "algorithmic FLOPs of ff = %d  (%.1f TFLOP/s, overflow count %d)"
              % (ff, med, lo, hi, rounds, iters, B / med * 1e3, med / base[0], fl / base[1], WIDTHS[0], fl / med / 1e9, ovf), flush=True)


if __name__ == "__main__":
    main()
