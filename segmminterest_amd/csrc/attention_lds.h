// Dynamic-LDS layouts of the two attention backward kernels that take their pointers from them -- attn_bwd_fused_kernel
// (attention.h) and attn_bwd_pl_kernel (attention_pl.h, the kernel of the default model path) -- stated once: the kernel reads a
// layout's offsets and the launcher takes bytes() of the same layout, so a region added to one and not the other cannot happen.
// (The fp16x3, wide and dK/dV kernels carve their LDS in their own pointer arithmetic and the launcher keeps their formulas: with
// offsets from a struct the compiler spills more or changes an occupancy in some of their instances, profiles/README.md.)
// Plain C++17, no HIP types: tests/test_attn_lds_cpu.py compiles this header alone with the host compiler, prints bytes() over the
// launcher's whole domain and checks every layout's regions (order, alignment of the regions accessed 16 bytes at a time).
#pragma once
#include <cstddef>

namespace segmm {

constexpr int ATT_LDS_TS = 20;                                   // row stride (floats) of a wave's 16 x 16 transpose scratch
constexpr size_t ATT_LDS_TR_WAVE = 16 * ATT_LDS_TS * 4;          // ... its bytes
constexpr int att_lds_rs(int DH) { return DH + 4; }              // row stride (floats) of the staged query side: 16-byte aligned rows,
                                                                 // conflict-free fragment reads
constexpr int att_lds_ktp(int DH) { return DH * 2 + 8; }         // planes-in: row pitch (bytes) of a wave's K tile image, [16 keys][DH fp16] + pad
constexpr size_t att_lds_kimg_pl_wave(int DH) { return (size_t)2 * 16 * att_lds_ktp(DH); }           // ... hi image then lo image

// A layout is a struct of byte offsets, filled in order by its function below; bytes() is the end of the last region.  regions(f)
// names every region for a checker: f(name, begin, end, align), align = the widest access the kernel makes to it (16: float4 / uint4).

// attn_bwd_fused_kernel: a query chunk of QC rows (16 / 32 / 48), nw waves, Tp padded keys; merged (p.hpb == 3): both blocks' Q rows,
// dQ accumulators and turn counters
struct AttLdsFused {
    size_t q, dO, dq, mx, inv, D, tr, turn, dp, qm, km, end;
    constexpr size_t bytes() const { return end; }
    template <class F> void regions(F f) const {
        f("Q rows", q, dO, 16); f("dO rows", dO, dq, 16); f("dQ accumulators", dq, mx, 16); f("row max", mx, inv, 16);
        f("1 / row sum", inv, D, 16); f("D", D, tr, 16); f("transpose scratch", tr, turn, 16); f("dQ turns", turn, dp, 4);
        f("D partials", dp, qm, 4); f("query flags", qm, km, 4); f("key flags", km, end, 1);
    }
};
constexpr AttLdsFused att_lds_fused(int DH, int QC, int nw, int Tp, bool merged) {
    const size_t rows = (size_t)QC * att_lds_rs(DH) * 4, nQ = merged ? 2 : 1;
    AttLdsFused L = {};
    size_t at = 0;
    L.q = at; at += nQ * rows;                                    // [nQ][QC][RS] query rows of the current chunk
    L.dO = at; at += rows;
    L.dq = at; at += nQ * rows;                                   // [nQ][QC][RS] dQ accumulators
    L.mx = at; at += (size_t)QC * 4;
    L.inv = at; at += (size_t)QC * 4;
    L.D = at; at += (size_t)QC * 4;
    L.tr = at; at += nw * ATT_LDS_TR_WAVE;
    L.turn = at; at += nQ * 16;                                   // [nQ][4] whose turn it is to add dQ of query tile qt
    L.dp = at; at += (size_t)QC * (DH / 4) * 4;                   // [QC][DH/4] partial products dO . O
    L.qm = at; at += QC;                                          // [QC] 1 valid query, 0 masked, 2 pad
    L.km = at; at += Tp;                                          // [Tp]
    L.end = at;
    return L;
}

// attn_bwd_pl_kernel (attention_pl.h): the D partials live in the dQ accumulators' space (dead before those are zeroed), a wave's
// transpose scratch in its K image (the fragments are in registers by then); the key flags come with the K fragments
struct AttLdsPl {
    size_t q, dO, dq, mx, inv, D, kimg, turn, wm, qm, end;
    constexpr size_t bytes() const { return end; }
    template <class F> void regions(F f) const {
        f("Q rows", q, dO, 16); f("dO rows", dO, dq, 16); f("dQ accumulators / D partials", dq, mx, 16); f("row max", mx, inv, 16);
        f("1 / row sum", inv, D, 16); f("D", D, kimg, 16); f("K images / transpose scratch", kimg, turn, 16); f("dQ turns", turn, wm, 4);
        f("wave maxima", wm, qm, 4); f("query flags", qm, end, 4);
    }
};
constexpr AttLdsPl att_lds_pl(int DH, int QC, int nw) {
    const size_t rows = (size_t)QC * att_lds_rs(DH) * 4;
    AttLdsPl L = {};
    size_t at = 0;
    L.q = at; at += rows;
    L.dO = at; at += rows;
    L.dq = at; at += rows;
    L.mx = at; at += (size_t)QC * 4;
    L.inv = at; at += (size_t)QC * 4;
    L.D = at; at += (size_t)QC * 4;
    L.kimg = at; at += nw * att_lds_kimg_pl_wave(DH);
    L.turn = at; at += 16;
    L.wm = at; at += 36 * 4;
    L.qm = at; at += QC;
    L.end = at;
    return L;
}
constexpr bool att_lds_pl_scratch_fits(int DH) { return ATT_LDS_TR_WAVE <= att_lds_kimg_pl_wave(DH); }

}  // namespace segmm
