#!/usr/bin/env python
"""The streaming forms of the LayerNorm forward, the column sums and the split-K combine against what they replace, kernel by kernel,
in ONE process; writes nothing but its standard output (profiles/row_stream/kernel_bench.txt is this tool's output).

A window is ``reps`` back-to-back launches of one leg between two device events; ``--windows`` rounds alternate over the legs of a
group.  Every launch of a window takes the NEXT of several buffer sets, together larger than the 256 MB last-level cache (the
method of profiles/micro_batch/vec_add_bench.txt), so a leg never reads what its previous launch left in the cache.  Per leg: the
median window's us per launch, the window-to-window spread (max - min) and the rate over the bytes the launch must move.
Condition per kernel: median(new) <= median(old) - 2 x spread(old).

* LayerNorm forward: old and new form of THIS library (knob LN_FWD_PARTS: 1 = one wave per row, 0 = the row-walking form on its
  default grid; ``--ln-grids`` adds explicit grids).
* segmm_colsum / segmm_colsum3 / the split-K combine: the PARENT library (``--parent-lib``, the library built from the commit before
  the change, loaded by path beside this one) against this one.  The combine has no entry point of its own: the leg is
  segmm_gemm_p TN + splitk_reduce, and the difference of the two legs is the combine's.
* For scale: l1norm (register form, 8 B per element) and segmm_vec_add (12 B per element) measured the same way.

    python tools/row_stream_bench.py --parent-lib /path/to/parent/libsegmm_hip.so [--windows 7] [--ln-grids 768,1024,1536]

Needs the GPU; there is no fallback."""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LLC = 256 << 20


def _second_lib(H, path):
    """a second handle with the binding's prototypes (RTLD_LOCAL: its symbols do not mix with the first library's)"""
    L = C.CDLL(path)
    L.segmm_last_error.restype = C.c_char_p
    L.segmm_last_error.argtypes = []
    for name, at in H.SIGNATURES.items():
        fn = getattr(L, name, None)
        if fn is not None:
            fn.argtypes = at
            fn.restype = C.c_int
    return L


class Legs:
    """alternating windows over (label, bytes, launch(set index)) legs; ``pre`` runs before each window of a leg (knob, library)"""

    def __init__(self, torch, windows):
        self.torch, self.windows = torch, windows

    def _window(self, fn, reps, nsets, start):
        t = self.torch
        e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        t.cuda.synchronize()
        e0.record()
        for i in range(reps):
            fn((start + i) % nsets)
        e1.record()
        t.cuda.synchronize()
        return 1e3 * e0.elapsed_time(e1) / reps

    def run(self, title, legs, reps, nsets, old=0, new=()):
        """legs: [(label, bytes, pre, fn)]; prints every leg and the condition of each ``new`` index against ``old``"""
        us = [[] for _ in legs]
        for _, _, pre, fn in legs:
            pre()
            for i in range(min(nsets, 4)):
                fn(i)
        for w in range(self.windows):
            for k, (_, _, pre, fn) in enumerate(legs):
                pre()
                us[k].append(self._window(fn, reps, nsets, w * reps))
        med = [statistics.median(v) for v in us]
        spr = [max(v) - min(v) for v in us]
        print("%s  (%d windows of %d launches over %d buffer sets)" % (title, self.windows, reps, nsets))
        for (label, nbytes, _, _), m, s in zip(legs, med, spr):
            print("    %-58s %9.2f us  spread %6.2f us  %5.2f TB/s of %.1f MB" % (label, m, s, nbytes / m / 1e6, nbytes / 1e6))
        for k in new:
            good = med[k] <= med[old] - 2 * spr[old]
            print("    condition  %-46s %9.2f <= %.2f - 2 x %.2f: %s" % (legs[k][0], med[k], med[old], spr[old], "PASS" if good else "FAIL"))
        sys.stdout.flush()
        return med, spr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--ln-grids", default="")
    ap.add_argument("--only", default="", help="comma list of ln, colsum, splitk, scale")
    a = ap.parse_args()
    import torch
    from segmminterest_amd import hipabi as H
    dev = "cuda"
    head = H._lib_real()
    parent = _second_lib(H, a.parent_lib) if a.parent_lib else None
    only = set(filter(None, a.only.split(",")))
    bench = Legs(torch, a.windows)
    print("row_stream kernel bench: %s" % torch.cuda.get_device_name(0))

    def use(lib):
        def pre():
            H._lib = lib
        return pre

    def knob(v):
        def pre():
            H._lib = head
            H.config_set("LN_FWD_PARTS", v)
        return pre

    def nsets_for(per_set):
        return max(2, -(-int(1.5 * LLC) // per_set))

    grids = [int(g) for g in a.ln_grids.split(",") if g]
    try:
        # ---------------------------------------------------------------- LayerNorm forward
        if not only or "ln" in only:
            d = 768
            gamma, beta = 1 + 0.1 * torch.randn(d, device=dev), 0.1 * torch.randn(d, device=dev)
            w, b = 0.05 * torch.randn(d, device=dev), torch.zeros(1, device=dev)
            sc = torch.tensor([256.0], device=dev)
            for title, rows, with_y, with_pl, drop, dot, reps in (
                    ("layernorm_fwd (20 480, 768) fp32 + planes", 20480, True, True, 0.0, False, 40),
                    ("layernorm_fwd (51 200, 768) planes only, dropout 0.1", 51200, False, True, 0.1, False, 20),
                    ("layernorm_fwd_dot (20 480, 768) fp32 + head dot", 20480, True, False, 0.0, True, 40)):
                nbytes = rows * d * 4 * (1 + int(with_y) + int(with_pl))
                ns = nsets_for(nbytes)
                xs = [torch.randn(rows, d, device=dev) for _ in range(ns)]
                ys = [torch.empty(rows, d, device=dev) for _ in range(ns)] if with_y else None
                pls = [torch.empty(rows, 2 * d, dtype=torch.float16, device=dev) for _ in range(ns)] if with_pl else None
                hdr = H.new_site(dev)[0]
                amax = torch.zeros(H.SITE_FLOATS, device=dev)
                mean, rstd, dout = torch.empty(rows, device=dev), torch.empty(rows, device=dev), torch.empty(rows, device=dev)

                def launch(i, xs=xs, ys=ys, pls=pls, with_pl=with_pl, drop=drop, dot=dot, hdr=hdr, amax=amax, mean=mean, rstd=rstd, dout=dout):
                    po = H.PO(pls[i], 2 * d, hdr, sc.data_ptr()) if with_pl else None
                    y = ys[i] if ys is not None else None
                    if dot:
                        H.layernorm_fwd_dot(xs[i], gamma, beta, y, mean, rstd, w, b, dout, drop_p=drop, seed=3, site=5, amax=None if with_pl else amax, po=po)
                    else:
                        H.layernorm_fwd(xs[i], gamma, beta, y, mean, rstd, drop_p=drop, seed=3, site=5, amax=None if with_pl else amax, po=po)
                legs = [("old: one wave per row (LN_FWD_PARTS=1)", nbytes, knob(1), launch), ("new: row-walking, default grid (LN_FWD_PARTS=0)", nbytes, knob(0), launch)]
                legs += [("new: row-walking, %d workgroups" % g, nbytes, knob(g), launch) for g in grids]
                bench.run(title, legs, reps, ns, old=0, new=range(1, len(legs)))
                del xs, ys, pls
                torch.cuda.empty_cache()

        # ---------------------------------------------------------------- column sums
        if parent is not None and (not only or "colsum" in only):
            for M, N, weighted, reps in ((20480, 768, True, 60), (100, 768, False, 200)):
                nbytes = M * N * 4
                ns = min(64, nsets_for(nbytes))
                Xs = [torch.randn(M, N, device=dev) for _ in range(ns)]
                wv = torch.randn(M, device=dev) if weighted else None
                out, ws = torch.empty(N, device=dev), torch.empty(H.colsum_chunks(M) * N, device=dev)

                def launch(i, Xs=Xs, wv=wv, out=out, ws=ws, M=M, N=N):
                    H.colsum(Xs[i], N, M, N, out, ws, w=wv)
                bench.run("segmm_colsum (%d, %d%s)" % (M, N, ", weighted" if weighted else ""),
                          [("parent", nbytes, use(parent), launch), ("head", nbytes, use(head), launch)], reps, ns, old=0, new=(1,))
                del Xs
                torch.cuda.empty_cache()
            M = N = 768
            ns = 64
            X3 = [[torch.randn(M, N, device=dev) for _ in range(3)] for _ in range(ns)]
            outs, ws = [torch.empty(N, device=dev) for _ in range(3)], torch.empty(3 * H.colsum_chunks(M) * N, device=dev)

            def launch3(i):
                H.colsum3(X3[i], N, M, N, outs, ws)
            bench.run("segmm_colsum3 (768, 768) x 3", [("parent", 3 * M * N * 4, use(parent), launch3), ("head", 3 * M * N * 4, use(head), launch3)],
                      200, ns, old=0, new=(1,))
            del X3
            torch.cuda.empty_cache()

        # ---------------------------------------------------------------- split-K combine (inside segmm_gemm_p TN)
        if parent is not None and (not only or "splitk" in only):
            K = 20480
            for M, N, splits, reps in ((768, 768, 28, 60), (3072, 768, 7, 40)):
                H._lib = head
                dY, X = 0.01 * torch.randn(K, M, device=dev), torch.randn(K, N, device=dev)
                pdy, px = H.to_planes(dY, K, M, keep_f32=False), H.to_planes(X, K, N, keep_f32=False)
                nbytes = (splits + 1) * M * N * 4
                ns = nsets_for(splits * M * N * 4)
                wss = [torch.empty(splits * (M * N + M), device=dev) for _ in range(ns)]
                Cs = [torch.empty(M, N, device=dev) for _ in range(ns)]

                def launch(i, pdy=pdy, px=px, wss=wss, Cs=Cs, M=M, N=N, splits=splits):
                    H.gemm_p(H.LAYOUT_TN, M, N, K, pdy, px, Cs[i], N, splits=splits, workspace=wss[i])
                med, _ = bench.run("segmm_gemm_p TN %d x %d x %d, %d slabs: GEMM + splitk_reduce (bytes: the combine's)" % (M, N, K, splits),
                                   [("parent", nbytes, use(parent), launch), ("head", nbytes, use(head), launch)], reps, ns, old=0, new=(1,))
                print("    the combine's share of the difference: %.2f us" % (med[0] - med[1]))
                del wss, Cs
                torch.cuda.empty_cache()

        # ---------------------------------------------------------------- for scale
        if not only or "scale" in only:
            H._lib = head
            rows, d = 20480, 768
            ns = nsets_for(rows * d * 8)
            xs = [torch.rand(rows, d, device=dev) for _ in range(ns)]
            ys = [torch.empty(rows, d, device=dev) for _ in range(ns)]
            bench.run("for scale: l1norm register form (20 480, 768), 8 B per element",
                      [("l1norm_reg", rows * d * 8, use(head), lambda i: H.l1norm(xs[i], ys[i]))], 40, ns, old=0)
            n = rows * d
            bench.run("for scale: segmm_vec_add, 12 B per element",
                      [("vec_add out <- a + b", n * 12, use(head), lambda i: H.vec_add(ys[i].view(-1), xs[i].view(-1), xs[(i + 1) % ns].view(-1), n))], 40, ns, old=0)
    finally:
        H._lib = head
        H.config_set("LN_FWD_PARTS", 0)


if __name__ == "__main__":
    main()
