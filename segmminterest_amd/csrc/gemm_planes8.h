// NT plane GEMM, round-3 form: C[M,N] = A[M,K] . B[N,K]^T on v_mfma_f32_16x16x32_f16 with the two wave groups of a
// workgroup running OUT OF PHASE ("ping-pong").
//
// Same arithmetic, operand format (P32 planes), LDS image and fallback protocol as gemm_pl_nt (gemm_planes.h); tile
// 256 x (64 NJ) x 32 with NJ = 2, 3 or 4 chosen per launch (the host picks the width that wastes the fewest CU-rounds),
// 8 waves as 2 (m) x 4 (n), 128 x 16 NJ per wave.  What changed against gemm_pl_nt, and why:
//
//  * MFMA shape 16x16x32 instead of 32x32x16: same cycles per FLOP, same LDS fragment traffic -- but the chip, which is
//    power-limited in a dense fp16 MFMA loop on real data, holds a ~13 % higher clock on it (tools/probe/mfma_shape.hip on this
//    pool: 1 683 vs 1 492 TFLOP/s with every operand re-read from LDS; MI355X_MICROARCH.md "DVFS give-back" item 7).
//  * The operands of an MFMA are swapped (a := B fragment, b := A fragment), so an accumulator tile is C^T: a lane holds
//    FOUR CONSECUTIVE COLUMNS of one row of C.  The epilogue's arithmetic works on float4s straight from the accumulators;
//    only the finished values pass through a small per-wave LDS transpose patch so that every store instruction covers
//    4 rows x 256 B instead of 16 rows x 64 B (tools/probe/store_rate.hip: 3.5x fewer cycles to drain a tile).
//  * The epilogue's stores are buffer stores (32-bit offsets, rows beyond M dropped by the range check, no 64-bit address
//    arithmetic per store); its extra operand (residual / aux) comes through LDS by LDS-DMA.  The epilogue is nt_epilogue
//    (gemm_planes_epi.h), the one gemm_pl_nt4 runs too; the operand state and the repair verdict are site_state (common.h),
//    the rare path stages through nt_slow_stage / nt_dma_rows (gemm_planes_epi.h).  This file keeps the k-loops.
//  * Wave groups g0 = waves 0-3 (rows 0-127 of the tile) and g1 = waves 4-7 (rows 128-255) -- one wave of each per SIMD --
//    alternate LOAD and COMPUTE segments separated by s_barrier, g1 one segment behind g0: while one wave of a SIMD issues
//    its MFMAs its partner reads the next fragments out of LDS and issues its share of the LDS-DMA.
//    A k-tile is two phases per wave (P0: upper 64 rows of its 128, P1: lower 64), four segments:
//        L(t,P0): 8 A + 2 NJ B fragment reads of tile t; DMA of this group's share of A(t+1)   | lgkmcnt(0), barrier
//        C(t,P0): 12 NJ MFMAs                                                                  | vmcnt(4),   barrier
//        L(t,P1): 8 A fragment reads; DMA of this group's share of B(t+2)                      | lgkmcnt(0), barrier
//        C(t,P1): 12 NJ MFMAs                                                                  | vmcnt(NJ),  barrier
//    LDS-DMA stays in flight ACROSS barriers: the counted wait at the end of a compute segment only asks for the pieces
//    issued TWO load segments earlier (every piece has ~3 segments, > 1 us, to land), instead of draining vmcnt(0) before one
//    barrier per k-tile.  Hazards (global segment s; g0 loads in even, g1 in odd segments):
//      RAW  a piece is waited for by its issuing wave at the end of a compute segment and read, by any wave, in a LATER
//           segment (one barrier in between at least);
//      WAR  a region of a stage is refilled at least one full segment after the last segment that read it, and every
//           load segment retires its ds_reads (lgkmcnt(0)) BEFORE its closing barrier.
//    Who reads / refills what (stage = t & 1; A rows 0-63 / 64-127 = g0's P0 / P1 rows, 128-191 / 192-255 = g1's):
//      B(t) all rows : read in L(t,P0) of g0 (s = 4t) and g1 (4t+1);  refilled with B(t+2) in L(t,P1): lower half by g0
//                      (4t+2), upper half by g1 (4t+3)
//      A(t+1) rows 0-63, 128-191  : issued by g0 in L(t,P0) (s = 4t; last read of that stage region: 4t-4, 4t-3)
//      A(t+1) rows 64-127, 192-255: issued by g1 in L(t,P0) (s = 4t+1; last read: 4t-2, 4t-1)
//  * The first DMA pieces leave before the site headers are read (their addresses depend on blockIdx only); the headers
//    (two dependent global reads under load) are fetched while the first k-tiles fly.
#pragma once
#include "gemm_planes_tn.h"

namespace segmm {

__device__ __forceinline__ f32x4 mfma16(f32x4 a, f32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
// PROD: matrix-core products per k32 block.  3: hl + lh + hh (fp32-accurate, the default).  1: hh only -- every operand is its hi
// term (ordinary fp16 mixed precision); the lo fragments are staged (same P32 rows, same pieces and counted waits) but never read.
template <int NJ, int PROD>
__global__ __launch_bounds__(512, 2) void gemm_pl_nt8(const GemmArgs p, const PGemmX q) {
    static_assert(NJ >= 2 && NJ <= 4, "tile widths 128, 192, 256");
    static_assert(PROD == 1 || PROD == 3, "one product (hi . hi) or three (hl + lh + hh)");
    constexpr int BNW = 64 * NJ;                                         // tile columns
    // 128 KB: two stages x (A 32 KB | B 16 NJ KB); + 32 KB: a 16-row x 256-byte transpose patch per wave for the epilogue's stores
    __shared__ __attribute__((aligned(16))) char smem[2 * PSTAGE + 8 * 4096];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = wave >> 2, wn = wave & 3;          // grp = wm: rows [128 grp, +128) of the tile; columns [16 NJ wn, +16 NJ)
    const int l15 = lane & 15, lq = lane >> 4;
    const int nkt = p.K >> 5;
    const int lb = xcd_remap(blockIdx.x, p.nbm * p.nbn);
    const int m0 = (lb / p.nbn) * PBM, n0 = (lb % p.nbn) * BNW;
    STAMP(0);
    // ---- REPAIR launch of a planes-only output (no fp32 C to fall back on): the first launch wrote the planes with the site's
    // delayed scale and recorded maxima + overflow flag in c_hdr.  Judge the site like a consumer would: usable -> every workgroup
    // leaves at once (one header read); unusable (flag up, maximum below the fp16 window, no scale yet) -> recompute the tile and
    // rewrite the planes with the EXACT scale of the recorded maxima.  The header is left as it is: consumers derive the same
    // scale from the same maxima (attention_pl.h), and segmm_scales_update counts the site as refused.
    float c_repair = 0.f;
    if (q.repair) {
        const SiteState sc = site_state(site_words(q.c_hdr, lane));
        if (sc.ok) return;
        c_repair = f16_scale_of(sc.amax);
    }

    // ---- LDS-DMA: a wave-instruction moves 8 rows x 128 B.  Per load segment a wave issues
    //   A share of its group (4 pieces): piece pi = 4 wn + i of 16; tile rows 128 (pi >> 3) + 64 grp + 8 (pi & 7) .. + 7
    //   B share of its group (NJ pieces): tile rows 32 NJ grp + 8 (NJ wn + i) .. + 7
    const __amdgpu_buffer_rsrc_t rsA = make_rsrc(q.A.p, q.A.bytes), rsB = make_rsrc(q.B.p, q.B.bytes);
    const int r8 = lane >> 3;
    uint32_t voa[4], vob[NJ];
    uint32_t lda_off[4], ldb_off[NJ];          // wave-uniform LDS byte offsets of the pieces inside a stage
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int pi = 4 * wn + i;
        const int ra0 = 128 * (pi >> 3) + 64 * grp + 8 * (pi & 7);
        const int ra = ra0 + r8;
        voa[i] = (uint32_t)min(m0 + ra, p.M - 1) * (uint32_t)q.A.ld2 * 2u + (uint32_t)(((lane & 7) ^ ((ra >> 1) & 7)) * 16);
        lda_off[i] = (uint32_t)ra0 * 128u;
    }
#pragma unroll
    for (int i = 0; i < NJ; ++i) {
        const int rb0 = 32 * NJ * grp + 8 * (NJ * wn + i);
        const int rb = rb0 + r8;
        vob[i] = (uint32_t)min(n0 + rb, p.N - 1) * (uint32_t)q.B.ld2 * 2u + (uint32_t)(((lane & 7) ^ ((rb >> 1) & 7)) * 16);
        ldb_off[i] = (uint32_t)(PBM * 128) + (uint32_t)rb0 * 128u;
    }
    auto dmaA = [&](int kt) {
        char* st = smem + (kt & 1) * PSTAGE;
#pragma unroll
        for (int i = 0; i < 4; ++i) lds_dma16(rsA, st + lda_off[i], voa[i], (uint32_t)kt * 128u);
    };
    auto dmaB = [&](int kt) {
        char* st = smem + (kt & 1) * PSTAGE;
#pragma unroll
        for (int i = 0; i < NJ; ++i) lds_dma16(rsB, st + ldb_off[i], vob[i], (uint32_t)kt * 128u);
    };
    // ---- the first k-tiles leave NOW (harmless if the slow path is taken below: it restages synchronously)
    dmaA(0);
    dmaB(0);
    if (nkt > 1) dmaB(1);

    // ---- operand state (block-uniform): planes usable?  Every header word is requested at once (one round trip under load instead
    // of three dependent ones), then judged by the rule of common.h: scale > 0, flag down, max * s inside the fp16 window
    const SiteWords wa = site_words(q.A.hdr, lane), wb = site_words(q.B.hdr, lane);
    const float cs_in = (q.Cp && q.c_scale_in) ? *q.c_scale_in : 0.f;
    const float sa_hdr = site_scale(wa), sb_hdr = site_scale(wb);
    const bool slowA = q.A.f32 != nullptr && !site_usable(wa);          // (no fp32 copy: nothing to fall back on, not judged)
    const bool slowB = q.B.f32 != nullptr && !site_usable(wb);
    const float c_scale = q.repair ? wave_uniform(c_repair) : wave_uniform(cs_in);

    // ---- fragment read addressing (lane: row l15 of a 16-row block, logical chunk 4 plane + lq; physical = logical ^ swz)
    const int swz = (l15 >> 1) & 7;
    uint32_t fa[2], fb[2];
#pragma unroll
    for (int pl = 0; pl < 2; ++pl) {
        const int ch = ((4 * pl + lq) ^ swz) << 4;
        fa[pl] = (uint32_t)((grp * 128 + l15) * 128 + ch);
        fb[pl] = (uint32_t)(PBM * 128 + (wn * 16 * NJ + l15) * 128 + ch);
    }

    f32x4 acc[8][NJ];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 ah[4], al[4], bh[NJ], bl[NJ];
    auto readA = [&](const char* st, int mh) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            ah[i] = *(const f32x4*)(st + fa[0] + (mh * 4 + i) * 2048);
            if constexpr (PROD == 3) al[i] = *(const f32x4*)(st + fa[1] + (mh * 4 + i) * 2048);
        }
    };
    auto readB = [&](const char* st) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            bh[j] = *(const f32x4*)(st + fb[0] + j * 2048);
            if constexpr (PROD == 3) bl[j] = *(const f32x4*)(st + fb[1] + j * 2048);
        }
    };
    auto mma = [&](auto mh_tag) {
        constexpr int mh = decltype(mh_tag)::value;
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                f32x4 c = acc[mh * 4 + i][j];
                if constexpr (PROD == 3) {
                    c = mfma16(bh[j], al[i], c);          // (B fragment, A fragment): the accumulator tile is C^T
                    c = mfma16(bl[j], ah[i], c);
                }
                c = mfma16(bh[j], ah[i], c);
                acc[mh * 4 + i][j] = c;
            }
        __builtin_amdgcn_s_setprio(0);
    };

    float sa = sa_hdr, sb = sb_hdr;
    if (!(slowA || slowB)) {
        // ---- everyone waits for A(0), B(0); B(1) may still fly
        if (nkt > 1) end_compute_segment<NJ>(); else end_compute_segment<0>();
        if (grp == 1) { __builtin_amdgcn_s_barrier(); __builtin_amdgcn_sched_barrier(0); }          // g1 runs one segment behind g0
        STAMP(1);
#pragma unroll 1
        for (int t = 0; t < nkt; ++t) {
            const char* st = smem + (t & 1) * PSTAGE;
            // L(t, P0)
            readB(st);
            readA(st, 0);
            if (t + 1 < nkt) dmaA(t + 1);
            end_load_segment();
            // C(t, P0)
            mma(std::integral_constant<int, 0>{});
            if (t + 1 < nkt) end_compute_segment<4>(); else end_compute_segment<0>();
            // L(t, P1)
            readA(st, 1);
            if (t + 2 < nkt) dmaB(t + 2);
            end_load_segment();
            // C(t, P1)
            mma(std::integral_constant<int, 1>{});
            if (t + 2 < nkt) end_compute_segment<NJ>(); else end_compute_segment<0>();
        }
        if (grp == 0) { __builtin_amdgcn_s_barrier(); __builtin_amdgcn_sched_barrier(0); }          // barrier counts of g0 and g1 match
    } else {
        // ---- rare path (a delayed scale left its window): synchronous, stage 0 only, operands split from the fp32 copies
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // the early pieces have landed before anything is restaged
        if (slowA) sa = site_exact_scale(q.A.hdr, (float*)(smem + 2 * PSTAGE - 64), tid, 512);
        if (slowB) sb = site_exact_scale(q.B.hdr, (float*)(smem + 2 * PSTAGE - 64), tid, 512);
#pragma unroll 1
        for (int t = 0; t < nkt; ++t) {
            __syncthreads();
            if (slowA) nt_slow_stage<512>(q.A, sa, m0, p.M, PBM, t, smem, tid); else nt_dma_rows<512>(rsA, q.A, m0, p.M, PBM, t, smem, wave, lane);
            if (slowB) nt_slow_stage<512>(q.B, sb, n0, p.N, BNW, t, smem + PBM * 128, tid);
            else nt_dma_rows<512>(rsB, q.B, n0, p.N, BNW, t, smem + PBM * 128, wave, lane);
            dma_wait_barrier();
            readB(smem);
            readA(smem, 0);
            end_load_segment();
            mma(std::integral_constant<int, 0>{});
            readA(smem, 1);
            end_load_segment();
            mma(std::integral_constant<int, 1>{});
        }
        __syncthreads();
    }
    STAMP(2);

    // ---- epilogue (gemm_planes_epi.h): two wave groups, each read of the transpose patch in front of its store
    using G = NtEpiGeom<NJ, 2, false>;
    static_assert(G::BM == PBM && G::PATCH == 2 * PSTAGE && G::LDS == sizeof(smem), "the epilogue's LDS image: two 64 KB E halves, then the patches");
    nt_epilogue<G>(p, q, acc, smem, sa, sb, c_scale, m0, n0, wave, lane);
}

}  // namespace segmm

namespace segmm {

// =============================================================================== TN, round-3 form
// Weight gradients gW[M, N] = A[K, M]^T . B[K, N] over the token axis K (the SLOW axis of both operands), split-K over
// blockIdx.z -- the same ping-pong structure as gemm_pl_nt8 on v_mfma_f32_16x16x32_f16, with the operand handling of
// gemm_pl_tn (gemm_planes.h): a k-tile is 32 token rows of 1 KB per operand (256 features x [hi | lo]), one LDS-DMA
// wave-instruction per row, fragments by ds_read_b64_tr_b16 (hardware transpose: per 16-lane group 4 tokens x 16 features,
// a lane ends up with 8 consecutive tokens of ITS feature -- the 16 x 16 x 32 operand form directly).
//
// LDS image of a token row (1 KB = 16 pieces of 64 B): the token-row image of gemm_planes_tn.h, which also holds its DMA source
// rule, the fallback's writer, the fragment-read offsets and the output code (shared with gemm_pl_tn4).
//
// Schedule per k-tile t (stage t & 1; g0 = waves 0-3 = features 0-127 of A, g1 one segment behind):
//     L(t,P0): tr-reads of B (all 64 columns of the wave) and A sub-tile 0; DMA of the group's 16 token rows of A(t+1)
//     C(t,P0): 48 MFMAs                                   | vmcnt(4): B(t+1) has landed
//     L(t,P1): tr-reads of A sub-tile 1; DMA of the group's 16 rows of B(t+2)   | vmcnt(4): A(t+1) has landed
//     C(t,P1): 48 MFMAs
// Every wave reads ALL 32 token rows of a stage (its own feature columns), so a row of A(t+1) may be requested only after both
// groups' L(t-1,P1) (true from L(t,P0) on) and must have landed before g0's L(t+1,P0): the issuing wave waits for it at the
// end of its own L(t,P1).  B(t+2) replaces B(t), last read in L(t,P0) of both groups.
//
// The bias gradient (column sums of A over k) rides along in the workgroups of the first column tile: wave (wm, wn) adds
// one MFMA pair per phase against an all-ones fragment for its m-tile wn.  Output: split-K slabs (plain float4 stores from the
// accumulators, C^T trick as in gemm_pl_nt8) combined by splitk_reduce, or C itself for a single split.
template <int PROD>          // products per k32 block, as in gemm_pl_nt8; the column sums take the hi term alone at PROD = 1
__global__ __launch_bounds__(512, 2) void gemm_pl_tn8(const GemmArgs p, const PGemmX q) {
    static_assert(PROD == 1 || PROD == 3, "one product (hi . hi) or three (hl + lh + hh)");
    // two stages x (A: 32 tokens x 1 KB | B: 32 tokens x 1 KB) + a 4 KB transpose patch per wave for the output stores
    __shared__ __attribute__((aligned(16))) char smem[2 * PSTAGE + 8 * 4096];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = wave >> 2, wn = wave & 3;
    const int lq = lane >> 4;
    const TnTile<PBM> T(p, q);          // tiles of one token slab meet in one L2
    const int m0 = T.m0, n0 = T.n0, kbeg = T.kbeg, kend = T.kend, nkt = T.nkt;
    const bool do_colsum = T.do_colsum;

    // ---- LDS-DMA: piece = one token row (1 KB); group g fetches rows t = 16 g + 4 wn + i (i < 4) of both operands.  The row
    // and the tile's feature offset are wave-uniform (scalar offset of the instruction); per lane only the position inside the row,
    // tn_image_src(lane, t).  Here t & 3 = i and bit 3 of t = wn >> 1, and i enters the formula only as an XOR on the piece index
    // (bits 6, 7 of the offset): tn_image_src(lane, t0 + i) = tn_image_src(lane, t0) ^ (i << 6)
    const __amdgpu_buffer_rsrc_t rsA = make_rsrc(q.A.p, q.A.bytes), rsB = make_rsrc(q.B.p, q.B.bytes);
    const int t0 = 16 * grp + 4 * wn;
    const uint32_t inrow0 = tn_image_src(lane, t0);
    auto dmaA_pl = [&](int kt) {
        char* st = smem + (kt & 1) * PSTAGE + t0 * 1024;
        const uint32_t so = (uint32_t)(kbeg + kt * 32 + t0) * (uint32_t)q.A.ld2 * 2u + (uint32_t)m0 * 4u;
#pragma unroll
        for (int i = 0; i < 4; ++i) lds_dma16t(rsA, st + i * 1024, inrow0 ^ (uint32_t)(i << 6), so + (uint32_t)i * (uint32_t)q.A.ld2 * 2u);
    };
    auto dmaB_pl = [&](int kt) {
        char* st = smem + (kt & 1) * PSTAGE + 32768 + t0 * 1024;
        const uint32_t so = (uint32_t)(kbeg + kt * 32 + t0) * (uint32_t)q.B.ld2 * 2u + (uint32_t)n0 * 4u;
#pragma unroll
        for (int i = 0; i < 4; ++i) lds_dma16t(rsB, st + i * 1024, inrow0 ^ (uint32_t)(i << 6), so + (uint32_t)i * (uint32_t)q.B.ld2 * 2u);
    };
    dmaA_pl(0);
    dmaB_pl(0);
    if (nkt > 1) dmaB_pl(1);

    // ---- operand state (all header words requested at once, judged by the rule of common.h)
    const SiteWords wa = site_words(q.A.hdr, lane), wb = site_words(q.B.hdr, lane);
    const float sa0 = site_scale(wa), sb0 = site_scale(wb);
    const bool slowA = q.A.f32 != nullptr && !site_usable(wa);          // delayed scale outside its window: fp32 fallback
    const bool slowB = q.B.f32 != nullptr && !site_usable(wb);
    const bool slow = slowA || slowB;
    // Fallback (rare): the SAME schedule, with the group's share of a stage written by ds_write from the operand's fp32 copy --
    // split with the exact scale of its recorded maxima -- instead of by LDS-DMA; every counted vmcnt wait becomes vmcnt(0) then
    // (the counts assume four pieces of the other operand behind them).  A wave converts its 4 token rows, 4 features per lane and row.
    float sa = sa0, sb = sb0;
    if (slow) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // the early pieces have landed before anything is restaged
        if (slowA) sa = site_exact_scale(q.A.hdr, (float*)(smem + 2 * PSTAGE - 64), tid, 512);
        if (slowB) sb = site_exact_scale(q.B.hdr, (float*)(smem + 2 * PSTAGE - 64), tid, 512);
    }
    auto stage_f32 = [&](const PlaneOperand& op, float sc, int kt, int f0, int nfeat, char* dst) {
#pragma unroll 1
        for (int i = 0; i < 4; ++i) {
            const int t = t0 + i, gk = kbeg + kt * 32 + t, gf = f0 + lane * 4;
            f32x4 x = {0.f, 0.f, 0.f, 0.f};
            if (gk < kend && gf < nfeat) x = *(const f32x4*)(op.f32 + (size_t)gk * op.ldf + gf);
            tn_image_put(dst + t * 1024, lane * 4, x, sc, t);
        }
    };
    auto dmaA = [&](int kt) { if (slowA) stage_f32(q.A, sa, kt, m0, p.M, smem + (kt & 1) * PSTAGE); else dmaA_pl(kt); };
    auto dmaB = [&](int kt) { if (slowB) stage_f32(q.B, sb, kt, n0, p.N, smem + (kt & 1) * PSTAGE + 32768); else dmaB_pl(kt); };
    if (slow) {          // restage what the early pieces brought
        __syncthreads();
        dmaA(0);
        dmaB(0);
        if (nkt > 1) dmaB(1);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          // (the ds_writes of the fallback are retired before the first barrier)
    }

    // ---- transposed fragment reads: lane = (g = lq: token octet, qq = (lane >> 2) & 3: token inside a 4-block, pp = lane & 3)
    // A tile i (16 features) of phase mh, plane pl: lane part fr(i, pl), uniform part (2 wm + mh) * 256; B tile j: the same lane
    // part, uniform part 32768 + 256 wn
    const TnFrag fr = tn_frag_off(lane, lq, 1024);
    const int ua = grp * 2 * 256, ub = 32768 + wn * 256;          // wave-uniform parts

    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 accb[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    f32x4 ah[4], al[4], bh[4], bl[4];
    auto readA = [&](const char* st, int mh) {
        const char* sa_ = st + ua + mh * 256;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            ah[i] = lds_tr8<4096>(sa_ + fr.x[2 * (i >> 1)] + fr.h[i & 1]);
            if constexpr (PROD == 3) al[i] = lds_tr8<4096>(sa_ + fr.x[2 * (i >> 1) + 1] + fr.h[i & 1]);
        }
    };
    auto readB = [&](const char* st) {
        const char* sb_ = st + ub;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            bh[j] = lds_tr8<4096>(sb_ + fr.x[2 * (j >> 1)] + fr.h[j & 1]);
            if constexpr (PROD == 3) bl[j] = lds_tr8<4096>(sb_ + fr.x[2 * (j >> 1) + 1] + fr.h[j & 1]);
        }
    };
    auto mma = [&](auto mh_tag, auto cs_tag) {
        constexpr int mh = decltype(mh_tag)::value;
        constexpr bool CS = decltype(cs_tag)::value;
        __builtin_amdgcn_s_setprio(1);
        if (CS) {
            const f32x4 ones = __builtin_bit_cast(f32x4, make_uint4(0x3C003C00u, 0x3C003C00u, 0x3C003C00u, 0x3C003C00u));      // 8 x fp16 1.0
            // the column sums of this wave's A tile i = wn of the phase (a wave-uniform choice among fragments it holds anyway)
            f32x4 cb = accb[mh];
            switch (wn) {
                case 0: if constexpr (PROD == 3) cb = mfma16(ones, al[0], cb); cb = mfma16(ones, ah[0], cb); break;
                case 1: if constexpr (PROD == 3) cb = mfma16(ones, al[1], cb); cb = mfma16(ones, ah[1], cb); break;
                case 2: if constexpr (PROD == 3) cb = mfma16(ones, al[2], cb); cb = mfma16(ones, ah[2], cb); break;
                default: if constexpr (PROD == 3) cb = mfma16(ones, al[3], cb); cb = mfma16(ones, ah[3], cb); break;
            }
            accb[mh] = cb;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                f32x4 c = acc[mh * 4 + i][j];
                if constexpr (PROD == 3) {
                    c = mfma16(bh[j], al[i], c);
                    c = mfma16(bl[j], ah[i], c);
                }
                c = mfma16(bh[j], ah[i], c);
                acc[mh * 4 + i][j] = c;
            }
        __builtin_amdgcn_s_setprio(0);
    };
    auto end_load_vm4 = [&](bool wait4, bool wait0) {          // close a load segment; A(t+1) must have landed when asked
        __builtin_amdgcn_sched_barrier(0);
        if (wait4 && !slow) asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory");
        else if (wait0) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
    };
    auto k_loop = [&](auto cs_tag) {
        constexpr bool CS = decltype(cs_tag)::value;
        if (nkt > 1 && !slow) end_compute_segment<4>(); else end_compute_segment<0>();          // A(0), B(0) landed; B(1) may fly
        if (grp == 1) { __builtin_amdgcn_s_barrier(); __builtin_amdgcn_sched_barrier(0); }
#pragma unroll 1
        for (int t = 0; t < nkt; ++t) {
            const char* st = smem + (t & 1) * PSTAGE;
            readB(st);
            readA(st, 0);
            if (t + 1 < nkt) dmaA(t + 1);
            end_load_segment();
            mma(std::integral_constant<int, 0>{}, cs_tag);
            if (t + 1 < nkt && !slow) end_compute_segment<4>(); else end_compute_segment<0>();          // B(t+1) landed (A(t+1) may fly)
            readA(st, 1);
            if (t + 2 < nkt) dmaB(t + 2);
            end_load_vm4(t + 2 < nkt, t + 1 < nkt);                                             // A(t+1) landed (B(t+2) may fly)
            mma(std::integral_constant<int, 1>{}, cs_tag);
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);
        }
        if (grp == 0) { __builtin_amdgcn_s_barrier(); __builtin_amdgcn_sched_barrier(0); }
    };
    if (do_colsum) k_loop(std::true_type{}); else k_loop(std::false_type{});

    // ---- outputs (gemm_planes_tn.h): two wave groups, each read of the transpose patch in front of its store
    using G = TnOutGeom<2, false>;
    static_assert(G::BM == PBM && G::LDS == sizeof(smem), "the patches behind the two stages");
    tn_outputs<G>(p, q, acc, accb, smem, sa, sb, T, wave, lane);
}

}  // namespace segmm
