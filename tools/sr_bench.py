"""What spatial-reduction attention (model_cfg.sr_attn = 1, sr_ratio > 1) costs and saves at BASELINE config 2 (B = 512, S = 40,
Lt = 100, d = D_in = 768, h = 16, N = 2: layer 0, video side, is the only live layer).

    python tools/sr_bench.py [iters] [rounds]  >  profiles/sr_attention/sr_bench.txt

Part 1, the two window kernels alone (csrc/srops.h) at B = 512, S = 40, d = 768, r in {2, 4}, each next to a device-to-device copy of
the same bytes: device events around ``iters`` back-to-back launches, the forms alternating over ``rounds`` windows (+ one warm-up
window) in this one process, so that a drift of the machine shows as spread, not as a difference.  GB/s are algorithmic bytes (every
operand once) over the median.

Part 2, the whole recorded train step (Trainer(device_state=True).record(), FusedAdamW, dropout on): the default model (built
without the key: the step every earlier release takes) against sr_ratio = [2, 1] and [4, 1], the three legs alternating window by
window.  Then one eager step per leg with the per-launch event lists of hipabi (ATTN_PROFILE, GEMM_PROFILE): the sum of the attention
launches and of the GEMM launches -- where the time went.  The launches overlap across streams in the real step: the sums say which
kernels grew, not what the step waits for."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from segmminterest_amd import hipabi as H  # noqa: E402

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 20
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
dev = "cuda"
B, S, Lt, D, HEADS, N = 512, 40, 100, 768, 16, 2


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n          # us per call


def stats(v):
    return sorted(v)[len(v) // 2], min(v), max(v)


def kernels():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B * S, D, generator=g).to(dev)
    m = (torch.rand(B, S, generator=g) < 0.7).to(dev).view(torch.uint8)
    res = torch.randn(B * S, D, generator=g).to(dev)
    for r in (2, 4):
        Ls = H.sr_len(S, r)
        A = torch.empty(B * Ls, r * D, device=dev)
        dA = torch.randn(B * Ls, r * D, generator=g).to(dev)
        msr = torch.empty(B, Ls, dtype=torch.uint8, device=dev)
        G = torch.empty(B * S, D, device=dev)
        hdr = H.new_site(dev)[0]
        pack_bytes = 4 * (B * S * D + A.numel())
        unpack_bytes = 4 * (dA.numel() + 2 * B * S * D)
        c_src = torch.empty(max(pack_bytes, unpack_bytes) // 8, device=dev)
        c_dst = torch.empty_like(c_src)
        forms = (
            ("sr_pack   r=%d (+ maxima, pooled mask)" % r, pack_bytes, lambda: H.sr_pack(x, D, m, A, msr, hdr[H.SITE_HDR:], B, S, D, r)),
            ("copy      of the pack's bytes", pack_bytes, lambda: H.copy_bytes(c_dst[:pack_bytes // 8], c_src[:pack_bytes // 8])),
            ("sr_unpack r=%d (+ residual)" % r, unpack_bytes, lambda: H.sr_unpack(dA, res, G, B, S, D, r)),
            ("copy      of the unpack's bytes", unpack_bytes, lambda: H.copy_bytes(c_dst[:unpack_bytes // 8], c_src[:unpack_bytes // 8])),
        )
        us = {k: [] for k, *_ in forms}
        for rnd in range(rounds + 1):
            for k, _, fn in forms:
                t = timed(fn, iters)
                if rnd:
                    us[k].append(t)
        for k, nbytes, _ in forms:
            med, lo, hi = stats(us[k])
            print("%-40s %6.1f MB  median %7.1f us  (min %7.1f  max %7.1f over %d windows of %d)  %6.0f GB/s"
                  % (k, nbytes / 1e6, med, lo, hi, rounds, iters, nbytes / med / 1e3), flush=True)


def make_leg(sr):
    from segmminterest_amd.trainer import Trainer, default_args, init_model
    over = {} if sr is None else dict(sr_attn=1)
    margs = default_args(num_layers_enc=N, d_model=D, nhead=HEADS, input_type={"user": "image", "photo": "image"}, exposure_prob=[1.0] * S, **over)
    torch.manual_seed(1234)
    model = init_model(margs, n_users=1903, n_items=352494, input_dim=D, max_vid_len=S, max_usr_len=Lt, sr_ratio=sr).to(dev)
    return model, Trainer(model, lr=1e-3, weight_decay=1e-4, device_state=True)


def steps():
    from segmminterest_amd.synth import make_batch
    batches = [{k: v.to(dev) for k, v in make_batch(B, S, Lt, D, n_users=1903, n_items=352494, seed=1234 + 1000 * i).items()} for i in range(4)]
    legs = [("default (no key)", None), ("sr_ratio [2, 1]", [2, 1]), ("sr_ratio [4, 1]", [4, 1])]
    trs, where = {}, {}
    for name, sr in legs:
        model, tr = make_leg(sr)
        for i in range(3):
            tr.train_step(batches[i % 4])
        # one eager step with per-launch events: what the attention and the GEMM launches sum to
        H.ATTN_PROFILE, H.GEMM_PROFILE = [], []
        tr.train_step(batches[3])
        torch.cuda.synchronize()
        att = sum(e[-2].elapsed_time(e[-1]) for e in H.ATTN_PROFILE)
        gem = sum(e[-2].elapsed_time(e[-1]) for e in H.GEMM_PROFILE)
        calls = sorted({tuple(e[:7]) for e in H.ATTN_PROFILE})
        where[name] = (att, len(H.ATTN_PROFILE), gem, len(H.GEMM_PROFILE), calls, H.ATTN_PIN_CALLS)
        H.ATTN_PROFILE = H.GEMM_PROFILE = None
        tr.record(batches[0], warmup=2)
        trs[name] = (model, tr)
    ms = {name: [] for name, _ in legs}
    for rnd in range(rounds + 1):
        for name, _ in legs:
            tr = trs[name][1]
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(iters):
                out = tr.run_recorded(batches[i % 4])
            e1.record()
            torch.cuda.synchronize()
            assert bool(torch.isfinite(out["loss"]).all())
            if rnd:
                ms[name].append(e0.elapsed_time(e1) / iters)
    base = stats(ms[legs[0][0]])[0]
    for name, _ in legs:
        med, lo, hi = stats(ms[name])
        print("%-18s recorded step median %7.3f ms  (min %7.3f  max %7.3f over %d windows of %d)  %8.0f interactions/s  x %.3f of the default"
              "  (overflow count %d)" % (name, med, lo, hi, rounds, iters, B / med * 1e3, med / base, trs[name][0]._store.overflow_count()), flush=True)
    for name, _ in legs:
        att, na, gem, ng, calls, _ = where[name]
        print("%-18s eager step, sums of per-launch times: attention %6.3f ms in %d launches, GEMMs %6.3f ms in %d launches; attention calls %s"
              % (name, att, na, gem, ng, ", ".join("%s(Lq=%d, La=%d, Lb=%d)" % (c[0], c[4], c[5], c[6]) for c in calls)), flush=True)


def main():
    H.lib()
    print("# sr_bench: B = %d, S = %d, Lt = %d, d = %d; %d windows of %d launches / steps per form; %s"
          % (B, S, Lt, D, rounds, iters, torch.cuda.get_device_name(0)))
    print("# part 1: the window kernels next to a device-to-device copy of the same bytes")
    kernels()
    print("# part 2: recorded train step at config 2, the legs alternating window by window")
    steps()


if __name__ == "__main__":
    main()
