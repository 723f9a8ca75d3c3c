// Plane GEMMs, round-6 form: FOUR-wave workgroups with a 128 x 256 output tile and 80 KB of LDS, so that TWO workgroups are
// resident per CU (2 x 80 KB = the CU's 160 KB, 2 x 1 wave per SIMD at <= 256 registers).
//
// Why.  gemm_pl_nt8 / gemm_pl_tn8 (gemm_planes8.h) own their CU: 160 KB of LDS, 8 waves.  Their k-loop runs at 0.875 of the MFMA
// issue rate, but 16 % of a tile's time is prologue (first operand pieces from a cold L2, two dependent header reads) and
// epilogue (512 KB of stores through a 64 B / clock path) during which the matrix pipe of the CU has nothing to do
// (profiles/r5/gemm_pl_nt_20480x3072x768_pmc.csv: 58 % MFMA busy).  Here the two resident workgroups are independent: their
// tiles drift out of phase, one workgroup's prologue / epilogue runs beside the other's k-loop, and the pairing that
// gemm_planes8.h builds with barriers between its two wave groups (one wave of a SIMD loads while its partner computes) is
// what the hardware arbitration produces between the two workgroups' waves on a SIMD.  A tile of half the size also halves
// the quantisation loss of launches with few tiles (config 4's 256-row shard: 120 tiles of 256 x 256 on 256 CUs).
//
// Same arithmetic, operand format (P32 planes), MFMA shape and order (v_mfma_f32_16x16x32_f16, hl + lh + hh per k32 block,
// swapped operands: the accumulator tile is C^T) as gemm_pl_nt8; the fallback / repair verdicts (site_usable / site_state, common.h), the rare
// path's staging and the epilogue (nt_epilogue, gemm_planes_epi.h) ARE gemm_pl_nt8's, instantiated for this tile: the results
// are BITWISE those of gemm_pl_nt8 (same accumulation chain per element).
//
// NT kernel gemm_pl_nt4: waves as 1 (m) x 4 (n), 128 x 64 per wave (128 accumulator registers).  LDS:
//     [0, 32 K)            A: two stages of 128 rows x 128 B (a k-tile of 32: [32 hi | 32 lo] per row), shared by the four waves
//     [32 K, 80 K)         B: PRIVATE to each wave (wave wn reads only the rows [64 wn, +64) of the B tile): 12 KB per wave = a ring of
//                          three half-tiles (32 rows x 128 B); a k-tile is two halves, so the ring holds 1.5 k-tiles
// Because B is private, only A needs barriers: ONE s_barrier per k-tile (four in gemm_pl_nt8).  Per k-tile t and wave:
//     X(t)                 s_waitcnt vmcnt(4): own pieces of A(t), B halves 2t, 2t+1 have landed; s_barrier
//     4 pieces of A(t+1) -> stage (t+1) & 1            (last read before X(t): every wave retired its reads of tile t-1)
//     8 + 8 ds_read_b128: B fragments of both halves, A fragments of rows 0-63; lgkmcnt(0)
//     48 MFMAs (rows 0-63), with 4 + 4 pieces of B halves 2t+3, 2t+4 issued between them into the two slots just read
//     8 ds_read_b128: A fragments of rows 64-127; lgkmcnt(0); 48 MFMAs
// Every piece has a whole k-tile period (~2 us) to land; vmcnt counts in issue order: at X(t+1) only the 4 youngest pieces
// (half 2t+4) may still be in flight.
#pragma once
#include "gemm_planes8.h"

namespace segmm {

constexpr int P4_BM = 128, P4_BN = 256;
constexpr int P4_ASTAGE = P4_BM * 128;                 // 16 KB
constexpr int P4_BOFF = 2 * P4_ASTAGE;                 // private B rings start here
constexpr int P4_BHALF = 32 * 128;                     // 4 KB: 32 rows
constexpr int P4_BRING = 3 * P4_BHALF;                 // 12 KB per wave
#ifndef P4_LDS_PAD
#define P4_LDS_PAD 0          // probe: extra LDS bytes (> 0 leaves ONE workgroup per CU)
#endif
#ifndef P4_EPI_PRIO
#define P4_EPI_PRIO 3          // wave priority outside the k-loop (prologue, epilogue): their few instructions go in front of the partner workgroup's MFMA stream
#endif
#ifndef P4_NGROUP
#define P4_NGROUP 4          // column tiles per group of the NT tile order (0: one row-major sweep over all column tiles)
#endif
#ifndef P4_STAGGER
#define P4_STAGGER 0          // units of 512 cycles per k-tile that the late half of the first round sleeps (0: no stagger)
#endif
constexpr int P4_LDS = P4_BOFF + 4 * P4_BRING + P4_LDS_PAD;         // 80 KB
constexpr int P4_PATCH = NtEpiGeom<4, 1, true>::PATCH;              // output code: 4 KB transpose patch per wave, where the NT epilogue has its own

template <int N>
__device__ __forceinline__ void wait_vm_barrier() {          // close a k-tile: all but the N youngest pieces landed, then the workgroup's barrier
    __builtin_amdgcn_sched_barrier(0);
    if (N == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
}
__device__ __forceinline__ void wait_lgkm() {
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
}

// PROD: matrix-core products per k32 block.  3: hl + lh + hh (fp32-accurate, the default).  1: hh only -- every operand is its hi
// term (ordinary fp16 mixed precision); the lo fragments are staged (same P32 rows, same DMA pieces and counted waits) but never read.
template <int PROD>
__global__ __launch_bounds__(256, 2) void gemm_pl_nt4(const GemmArgs p, const PGemmX q) {
    static_assert(PROD == 1 || PROD == 3, "one product (hi . hi) or three (hl + lh + hh)");
    constexpr int NJ = 4;
    __shared__ __attribute__((aligned(16))) char smem[P4_LDS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wn = wave;                               // columns [64 wn, +64) of the tile; every wave owns all 128 rows
    const int l15 = lane & 15, lq = lane >> 4;
    const int nkt = p.K >> 5;
    const int lb = xcd_remap(blockIdx.x, p.nbm * p.nbn);
    // tile order: groups of P4_NGROUP column tiles, row-major inside a group.  An XCD's 64 resident workgroups then cover
    // 64 / P4_NGROUP row panels x P4_NGROUP column panels: the B panels of the group (786 KB each at K = 768) stay in its 4 MB L2
    // while the A panels stream past once per group -- with all 12 column tiles of N = 3072 in one row-major sweep the 9.4 MB of
    // B fell out of L2 between row panels and was fetched again ~30 times per launch (profiles/r6/gemm4_tile_order.txt).
    int mt = lb / p.nbn, nt_ = lb - mt * p.nbn;
    {
#ifdef SEGMM_GEMM_PROBE
        const int gc = ((q.dbg >> 20) & 15) ? ((q.dbg >> 20) & 15) - 1 : P4_NGROUP;          // probe: dbg bits 20-23 = group width + 1
#else
        constexpr int gc = P4_NGROUP;
#endif
        if (gc > 0 && p.nbn > gc) {
            const int gsz = gc * p.nbm, g = lb / gsz, rem = lb - g * gsz;
            const int wdt = min(gc, p.nbn - g * gc);
            mt = rem / wdt;
            nt_ = g * gc + (rem - mt * wdt);
        }
    }
    const int m0 = mt * P4_BM, n0 = nt_ * P4_BN;
    STAMP(0);
    if (P4_EPI_PRIO) __builtin_amdgcn_s_setprio(P4_EPI_PRIO);
    // ---- REPAIR launch of a planes-only output (see gemm_pl_nt8): usable site -> leave at once, else recompute with the exact scale
    float c_repair = 0.f;
    if (q.repair) {
        const SiteState sc = site_state(site_words(q.c_hdr, lane));
        if (sc.ok) return;
        c_repair = f16_scale_of(sc.amax);
    }

    // ---- stagger: the workgroups of a launch start within a microsecond of each other, so the two that share a CU would run
    // their prologues, k-loops and epilogues IN PHASE (measured: the epilogue then costs the same 14 % as in gemm_pl_nt8).  Half
    // of the first round sleeps for about half a tile's k-loop; the offset then carries through the later rounds (a slot is
    // refilled when its workgroup retires).  Speed only: nothing depends on which workgroups share a CU.
#ifdef SEGMM_GEMM_PROBE
    const int stag_units = (q.dbg >> 8) & 0xff, stag_pat = (q.dbg >> 16) & 3;
#else
    constexpr int stag_units = P4_STAGGER, stag_pat = 0;
#endif
    if (stag_units > 0 && (int)blockIdx.x < 512) {
        if (stag_pat == 3) {          // every workgroup of the first round: a sixteenth-grained delay from a hash of its id
            const int sx = (int)(((uint32_t)blockIdx.x * 2654435761u) >> 28);
#pragma unroll 1
            for (int i = 0; i < (nkt * stag_units * sx) >> 4; ++i) __builtin_amdgcn_s_sleep(8);
        } else {
            const bool late = stag_pat == 0 ? (blockIdx.x & 256) != 0 : stag_pat == 1 ? (blockIdx.x & 8) != 0 : (blockIdx.x & 128) != 0;
            if (late) {
#pragma unroll 1
                for (int i = 0; i < nkt * stag_units; ++i) __builtin_amdgcn_s_sleep(8);          // 8 x 64 cycles per unit and k-tile
            }
        }
    }

    // ---- LDS-DMA pieces (a wave-instruction moves 8 rows x 128 B).  A: piece 4 wave + i of 16 (tile rows 8 piece .. + 7);
    // B: the wave's own 64 rows, piece pc of 8 (rows 64 wn + 8 pc .. + 7), half = pc >> 2.  Chunk swizzle on the SOURCE address.
    const __amdgpu_buffer_rsrc_t rsA = make_rsrc(q.A.p, q.A.bytes), rsB = make_rsrc(q.B.p, q.B.bytes);
    const int r8 = lane >> 3;
    uint32_t voa[4], vob[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int ra = 8 * (4 * wave + i) + r8;
        voa[i] = (uint32_t)min(m0 + ra, p.M - 1) * (uint32_t)q.A.ld2 * 2u + (uint32_t)(((lane & 7) ^ ((ra >> 1) & 7)) * 16);
    }
#pragma unroll
    for (int pc = 0; pc < 8; ++pc) {
        const int rb = 64 * wn + 8 * pc + r8;
        vob[pc] = (uint32_t)min(n0 + rb, p.N - 1) * (uint32_t)q.B.ld2 * 2u + (uint32_t)(((lane & 7) ^ ((rb >> 1) & 7)) * 16);
    }
    char* const bring = smem + P4_BOFF + wave * P4_BRING;
    auto dmaA = [&](int kt) {
        char* st = smem + (kt & 1) * P4_ASTAGE + wave * 4096;
#pragma unroll
        for (int i = 0; i < 4; ++i) lds_dma16(rsA, st + i * 1024, voa[i], (uint32_t)kt * 128u);
    };
    auto dmaB1 = [&](int kt, int pc, int slot) {          // one piece of B(kt) into half-slot `slot`
        lds_dma16(rsB, bring + slot * P4_BHALF + (pc & 3) * 1024, vob[pc], (uint32_t)kt * 128u);
    };
    // ---- the first k-tiles leave NOW: A(0), B halves 0, 1 (slots 0, 1) and half 2 = lower half of tile 1 (slot 2)
    dmaA(0);
#pragma unroll
    for (int pc = 0; pc < 8; ++pc) dmaB1(0, pc, pc >> 2);
    if (nkt > 1) {
#pragma unroll
        for (int pc = 0; pc < 4; ++pc) dmaB1(1, pc, 2);
    }

    // ---- operand state (block-uniform): planes usable?  (all header words requested at once, judged by the rule of common.h)
    const SiteWords wa = site_words(q.A.hdr, lane), wb = site_words(q.B.hdr, lane);
    const float cs_in = (q.Cp && q.c_scale_in) ? *q.c_scale_in : 0.f;
    const float sa_hdr = site_scale(wa), sb_hdr = site_scale(wb);
    const bool slowA = q.A.f32 != nullptr && !site_usable(wa);          // (no fp32 copy: nothing to fall back on, not judged)
    const bool slowB = q.B.f32 != nullptr && !site_usable(wb);
    const float c_scale = q.repair ? wave_uniform(c_repair) : wave_uniform(cs_in);

    // ---- fragment read addressing (lane: row l15 of a 16-row block, logical chunk 4 plane + lq; physical = logical ^ swz)
    const int swz = (l15 >> 1) & 7;
    uint32_t fr[2];
#pragma unroll
    for (int pl = 0; pl < 2; ++pl) fr[pl] = (uint32_t)(l15 * 128 + (((4 * pl + lq) ^ swz) << 4));

    f32x4 acc[8][NJ];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // fragments: B of the whole k-tile (4 column blocks, hi + lo: 32 registers), A of TWO row blocks (the one being multiplied and
    // the next one: 16 registers)
    f32x4 bh[NJ], bl[NJ], ah[2], al[2];
    auto rdA = [&](const char* st, int i, int buf) {
        ah[buf] = *(const f32x4*)(st + fr[0] + i * 2048);
        if constexpr (PROD == 3) al[buf] = *(const f32x4*)(st + fr[1] + i * 2048);
    };
    auto rdB = [&](int j, const char* lo_half, const char* hi_half) {          // rows 0-31 / 32-63 of the wave's B rows
        const char* b = ((j >> 1) ? hi_half : lo_half) + (j & 1) * 2048;
        bh[j] = *(const f32x4*)(b + fr[0]);
        if constexpr (PROD == 3) bl[j] = *(const f32x4*)(b + fr[1]);
    };
    auto mma1 = [&](int r, int j, int buf) {
        f32x4 c = acc[r][j];
        if constexpr (PROD == 3) {
            c = mfma16(bh[j], al[buf], c);          // (B fragment, A fragment): the accumulator tile is C^T
            c = mfma16(bl[j], ah[buf], c);
        }
        c = mfma16(bh[j], ah[buf], c);
        acc[r][j] = c;
    };

    float sa = sa_hdr, sb = sb_hdr;
    if (!(slowA || slowB)) {
        // ---- the software-pipelined stream.  A wave is self-sufficient: between its own MFMAs it issues the two ds_reads of the
        // NEXT row block's A fragments (double-buffered), the LDS-DMA pieces of later k-tiles (<= 2 per row block) and, in the last
        // row block of a k-tile, the next tile's B fragments -- each right behind the last MFMA that reads the registers it
        // replaces (the compiler places the counted lgkmcnt waits: program order below is pinned by sched_barriers).  Per k-tile t:
        //     row blocks 0-1: pieces of B half 2t+3 -> the slot of half 2t;   2-3: B half 2t+4 -> the slot of half 2t+1
        //     end of row block 6: vmcnt(4) lgkmcnt(0), s_barrier = X(t+1): A(t+1) is in LDS, every wave has read the last of A(t)
        //     row block 7: A fragments of row block 0 of tile t+1; pieces of A(t+2) -> stage t & 1; B fragments of tile t+1
        // Tiles beyond the last are requested through a zero-length descriptor (zeros land in slots nobody reads).
        if (nkt > 1) dmaA(1); else { const __amdgpu_buffer_rsrc_t z = make_rsrc(q.A.p, 0); 
#pragma unroll
            for (int i = 0; i < 4; ++i) lds_dma16(z, smem + P4_ASTAGE + wave * 4096 + i * 1024, voa[i], 0u); }
        if (nkt <= 1) {          // (keep the issue count of the prologue fixed: 4 + 8 + 4 + 4 pieces)
            const __amdgpu_buffer_rsrc_t z = make_rsrc(q.B.p, 0);
#pragma unroll
            for (int pc = 0; pc < 4; ++pc) lds_dma16(z, bring + 2 * P4_BHALF + pc * 1024, vob[pc], 0u);
        }
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt vmcnt(8)" ::: "memory");          // A(0), B halves 0, 1 landed; half 2 and A(1) may fly
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        STAMP(1);
        if (P4_EPI_PRIO) __builtin_amdgcn_s_setprio(0);
        rdA(smem, 0, 0);
#pragma unroll
        for (int j = 0; j < NJ; ++j) rdB(j, bring, bring + P4_BHALF);
        int s_lo = 0, s_hi = 1, s_nx = 2;          // half-slots of B halves 2t, 2t+1, 2t+2
#pragma unroll 1
        for (int t = 0; t < nkt; ++t) {
            const char* sta = smem + (t & 1) * P4_ASTAGE;
            const char* stn = smem + ((t + 1) & 1) * P4_ASTAGE;
            const __amdgpu_buffer_rsrc_t rsB1 = make_rsrc(q.B.p, t + 1 < nkt ? q.B.bytes : 0u);
            const __amdgpu_buffer_rsrc_t rsB2 = make_rsrc(q.B.p, t + 2 < nkt ? q.B.bytes : 0u);
            const __amdgpu_buffer_rsrc_t rsA2 = make_rsrc(q.A.p, t + 2 < nkt ? q.A.bytes : 0u);
            const uint32_t k1 = (uint32_t)(t + 1) * 128u, k2 = (uint32_t)(t + 2) * 128u;
            char* const slot_lo = bring + s_lo * P4_BHALF;
            char* const slot_hi = bring + s_hi * P4_BHALF;
            const char* const slot_nx = bring + s_nx * P4_BHALF;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (i < 7) rdA(sta, i + 1, (i + 1) & 1);
                else rdA(stn, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    mma1(i, j, i & 1);
                    if (i == 7) rdB(j, slot_nx, slot_lo);          // tile t+1: half 2t+2 (slot_nx) | half 2t+3 (slot_lo, refilled in row blocks 0-1)
                    if (i < 2 && (j & 1)) { const int pc = 2 * i + (j >> 1); lds_dma16(rsB1, slot_lo + pc * 1024, vob[4 + pc], k1); }
                    if ((i == 2 || i == 3) && (j & 1)) { const int pc = 2 * (i - 2) + (j >> 1); lds_dma16(rsB2, slot_hi + pc * 1024, vob[pc], k2); }
                    if (i == 7) lds_dma16(rsA2, smem + (t & 1) * P4_ASTAGE + wave * 4096 + j * 1024, voa[j], k2);
                    __builtin_amdgcn_sched_barrier(0);
                }
                if (i == 6) {          // X(t+1)
                    asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory");
                    __builtin_amdgcn_s_barrier();
                    asm volatile("" ::: "memory");
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            const int s = s_lo; s_lo = s_nx; s_nx = s_hi; s_hi = s;          // halves 2t+2, 2t+3, 2t+4 sit in slot_nx, slot_lo, slot_hi
        }
        __builtin_amdgcn_sched_barrier(0);
        if (P4_EPI_PRIO) __builtin_amdgcn_s_setprio(P4_EPI_PRIO);
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");          // the last (empty) requests have landed before the epilogue reuses the LDS
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
    } else {
        // ---- rare path (a delayed scale left its window): synchronous, operands split from the fp32 copies at the exact scale;
        // A at [0, 16 K), B (all 256 rows, shared layout) at [16 K, 48 K)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // the early pieces have landed before anything is restaged
        if (slowA) sa = site_exact_scale(q.A.hdr, (float*)(smem + P4_LDS - 64), tid, 256);
        if (slowB) sb = site_exact_scale(q.B.hdr, (float*)(smem + P4_LDS - 64), tid, 256);
        const char* bsh = smem + P4_ASTAGE + wn * 64 * 128;
#pragma unroll 1
        for (int t = 0; t < nkt; ++t) {
            __syncthreads();
            if (slowA) nt_slow_stage<256>(q.A, sa, m0, p.M, P4_BM, t, smem, tid); else nt_dma_rows<256>(rsA, q.A, m0, p.M, P4_BM, t, smem, wave, lane);
            if (slowB) nt_slow_stage<256>(q.B, sb, n0, p.N, P4_BN, t, smem + P4_ASTAGE, tid);
            else nt_dma_rows<256>(rsB, q.B, n0, p.N, P4_BN, t, smem + P4_ASTAGE, wave, lane);
            dma_wait_barrier();
#pragma unroll
            for (int j = 0; j < NJ; ++j) rdB(j, bsh, bsh + P4_BHALF);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                rdA(smem, i, i & 1);
#pragma unroll
                for (int j = 0; j < NJ; ++j) mma1(i, j, i & 1);
            }
        }
        __syncthreads();
    }
    STAMP(2);

    // ---- epilogue (gemm_planes_epi.h): gemm_pl_nt8's for one wave group, with the four reads of the transpose patch requested
    // before the first store of a row block.  E halves of 32 KB at the bottom of the LDS, the patches behind them.
    using G = NtEpiGeom<NJ, 1, true>;
    static_assert(G::BM == P4_BM && G::BN == P4_BN && G::LDS <= P4_LDS, "the epilogue's LDS image fits the k-loop's");
    nt_epilogue<G>(p, q, acc, smem, sa, sb, c_scale, m0, n0, wave, lane);
}

}  // namespace segmm

namespace segmm {

// =============================================================================== TN, round-6 form
// Weight gradients gW[M, N] = A[K, M]^T . B[K, N] over the token axis K (split-K over blockIdx.z), in the structure of gemm_pl_nt4:
// 128 (A features) x 256 (B features) tile, four waves as 1 x 4, two workgroups per CU, the software-pipelined stream.  Operand
// handling is gemm_pl_tn8's: a k-tile is 32 token rows, fragments by ds_read_b64_tr_b16 (hardware transpose: a lane ends up with
// 8 consecutive tokens of ITS feature).  What is laid out differently:
//     A (shared):  32 tokens x 512 B (128 features x [hi | lo]) per stage; one LDS-DMA instruction moves TWO token rows
//     B (private): wave wn stages only ITS 64 features: 256 B per token; the ring's three half-slots hold 16 tokens each (4 KB; a
//                  k-tile is the halves 2t = tokens 0-15 and 2t+1 = tokens 16-31); one LDS-DMA instruction moves FOUR token rows
// LDS image of a token row (512 / 256 B): gemm_pl_tn8's, the token-row image of gemm_planes_tn.h at these two row pitches.
// Same MFMA order per element and the same split ranges as gemm_pl_tn8: the results are BITWISE its results.
// LDS-DMA written as inline asm.  hipcc's waitcnt pass puts an s_waitcnt vmcnt(0) in front of every ds_read_b64_tr_b16 that follows an
// LDS-DMA builtin it has seen (it cannot tell which LDS bytes the DMA writes; plain ds_read_b128 loads are not treated that way) --
// inside a loop that keeps 12 pieces in flight that drains the whole prefetch at every fragment read (first build of this kernel:
// 0.55x of gemm_pl_tn8).  The asm form is invisible to the pass; every RAW / WAR between a piece and the reads of its bytes is
// ordered by the explicit s_waitcnt vmcnt(N) + s_barrier of the stream, as in the NT kernel.  (No other code of the kernel uses M0.
// "m0" cannot go on the clobber list: hipcc treats it as a reserved register it does not preserve around the statement, and warns.)
__device__ __forceinline__ u32x4_t rsrc_words(const void* p, uint32_t bytes) {
    const uint64_t a = (uint64_t)p;
    return u32x4_t{(uint32_t)a, (uint32_t)(a >> 32) & 0xffffu, bytes, 0x00020000u};
}
__device__ __forceinline__ void lds_dma16_asm(u32x4_t r, const void* lds_wave_base, uint32_t voff, uint32_t soff) {
    const uint32_t la = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const char*)lds_wave_base;
    #if SEGMM_TN_AUX == 2
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, %3 offen nt lds" :: "v"(voff), "s"(r), "s"(la), "s"(soff) : "memory");
#else
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, %3 offen lds" :: "v"(voff), "s"(r), "s"(la), "s"(soff) : "memory");
#endif
}

template <int PROD>          // products per k32 block, as in gemm_pl_nt4; the column sums take the hi term alone at PROD = 1
__global__ __launch_bounds__(256, 2) void gemm_pl_tn4(const GemmArgs p, const PGemmX q) {
    static_assert(PROD == 1 || PROD == 3, "one product (hi . hi) or three (hl + lh + hh)");
    constexpr int NJ = 4;
    __shared__ __attribute__((aligned(16))) char smem[P4_LDS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wn = wave;
    const int lq = lane >> 4;
    const TnTile<P4_BM> T(p, q);          // tiles of one token slab meet in one L2
    const int m0 = T.m0, n0 = T.n0, kbeg = T.kbeg, kend = T.kend, nkt = T.nkt;
    const bool do_colsum = T.do_colsum;
    if (P4_EPI_PRIO) __builtin_amdgcn_s_setprio(P4_EPI_PRIO);

    // ---- LDS-DMA.  A: piece 4 wave + i of 16 = tokens 2 piece, 2 piece + 1 (lanes 0-31 / 32-63), 32 chunks of 16 B per token;
    // B: piece pc of 8 = tokens 4 pc .. 4 pc + 3 (16 lanes each), 16 chunks per token, half = pc >> 2.
    // Physical chunk l of token t fetches tn_image_src(l, t).
    const u32x4_t rsA = rsrc_words(q.A.p, q.A.bytes), rsB = rsrc_words(q.B.p, q.B.bytes);
    uint32_t voa[4], vob[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int tok = 2 * (4 * wave + i) + (lane >> 5), l = lane & 31;
        voa[i] = (uint32_t)tok * (uint32_t)q.A.ld2 * 2u + (uint32_t)m0 * 4u + tn_image_src(l, tok);
    }
#pragma unroll
    for (int pc = 0; pc < 8; ++pc) {
        const int tok = 4 * pc + (lane >> 4), l = lane & 15;
        vob[pc] = (uint32_t)tok * (uint32_t)q.B.ld2 * 2u + (uint32_t)(n0 + 64 * wn) * 4u + tn_image_src(l, tok);
    }
    char* const bring = smem + P4_BOFF + wave * P4_BRING;
    const uint32_t ka = (uint32_t)q.A.ld2 * 64u, kb = (uint32_t)q.B.ld2 * 64u;          // bytes per k-tile of 32 token rows
    const uint32_t ka0 = (uint32_t)kbeg * (uint32_t)q.A.ld2 * 2u, kb0 = (uint32_t)kbeg * (uint32_t)q.B.ld2 * 2u;
    // ---- the first k-tiles leave NOW: A(0), B halves 0, 1 (slots 0, 1), half 2 = tokens 0-15 of tile 1 (slot 2), A(1)
#pragma unroll
    for (int i = 0; i < 4; ++i) lds_dma16_asm(rsA, smem + wave * 4096 + i * 1024, voa[i], ka0);
#pragma unroll
    for (int pc = 0; pc < 8; ++pc) lds_dma16_asm(rsB, bring + (pc >> 2) * P4_BHALF + (pc & 3) * 1024, vob[pc], kb0);
    {
        const u32x4_t rsB1 = rsrc_words(q.B.p, nkt > 1 ? q.B.bytes : 0u), rsA1 = rsrc_words(q.A.p, nkt > 1 ? q.A.bytes : 0u);
#pragma unroll
        for (int pc = 0; pc < 4; ++pc) lds_dma16_asm(rsB1, bring + 2 * P4_BHALF + pc * 1024, vob[pc], kb0 + kb);
#pragma unroll
        for (int i = 0; i < 4; ++i) lds_dma16_asm(rsA1, smem + P4_ASTAGE + wave * 4096 + i * 1024, voa[i], ka0 + ka);
    }

    // ---- operand state (all header words requested at once, judged by the rule of common.h)
    const SiteWords wa = site_words(q.A.hdr, lane), wb = site_words(q.B.hdr, lane);
    const float sa0 = site_scale(wa), sb0 = site_scale(wb);
    const bool slowA = q.A.f32 != nullptr && !site_usable(wa);          // delayed scale outside its window: fp32 fallback
    const bool slowB = q.B.f32 != nullptr && !site_usable(wb);
    float sa = sa0, sb = sb0;

    // ---- transposed fragment reads: lane = (lq: token octet, qq = (lane >> 2) & 3: token inside a 4-block, pp = lane & 3)
    // A tile i (16 features), plane pl: xa(i, pl) in rows of 512 B; B tile j: xb(j, pl) in rows of 256 B inside the half-slot of
    // token octets (lq >> 1)
    const TnFrag xa = tn_frag_off(lane, lq, 512), xb = tn_frag_off(lane, lq & 1, 256);

    f32x4 acc[8][NJ];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 accb[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    f32x4 bh[NJ], bl[NJ], ah[2], al[2];
    auto rdA = [&](const char* st, int i, int buf) {
        ah[buf] = lds_tr8<2048>(st + xa(i, 0));
        if constexpr (PROD == 3) al[buf] = lds_tr8<2048>(st + xa(i, 1));
    };
    // B: token octets 0, 1 (lanes lq < 2) in half `h0`, octets 2, 3 in half `h1`: a per-lane base
    auto rdB = [&](int j, const char* lane_half) {
        bh[j] = lds_tr8<1024>(lane_half + xb(j, 0));
        if constexpr (PROD == 3) bl[j] = lds_tr8<1024>(lane_half + xb(j, 1));
    };
    auto mma1 = [&](int r, int j, int buf) {
        f32x4 c = acc[r][j];
        if constexpr (PROD == 3) {
            c = mfma16(bh[j], al[buf], c);
            c = mfma16(bl[j], ah[buf], c);
        }
        c = mfma16(bh[j], ah[buf], c);
        acc[r][j] = c;
    };
    const f32x4 ones = __builtin_bit_cast(f32x4, make_uint4(0x3C003C00u, 0x3C003C00u, 0x3C003C00u, 0x3C003C00u));      // 8 x fp16 1.0
    auto colsum1 = [&](int i, int buf) {          // the column sums of A tile i ride along in wave i >> 1 of the first column tile's workgroup
        if ((i >> 1) == wn) {
            f32x4 cb = accb[i & 1];
            if constexpr (PROD == 3) cb = mfma16(ones, al[buf], cb);
            cb = mfma16(ones, ah[buf], cb);
            accb[i & 1] = cb;
        }
    };

    auto k_loop = [&](auto cs_tag) {
        constexpr bool CS = decltype(cs_tag)::value;
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt vmcnt(8)" ::: "memory");          // A(0), B halves 0, 1 landed; half 2 and A(1) may fly
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        if (P4_EPI_PRIO) __builtin_amdgcn_s_setprio(0);
        int s_lo = 0, s_hi = 1, s_nx = 2;          // half-slots of B halves 2t, 2t+1, 2t+2
        rdA(smem, 0, 0);
        {
            const char* lh = bring + ((lq >> 1) ? s_hi : s_lo) * P4_BHALF;
#pragma unroll
            for (int j = 0; j < NJ; ++j) rdB(j, lh);
        }
#pragma unroll 1
        for (int t = 0; t < nkt; ++t) {
            const char* sta = smem + (t & 1) * P4_ASTAGE;
            const char* stn = smem + ((t + 1) & 1) * P4_ASTAGE;
            const u32x4_t rsB1 = rsrc_words(q.B.p, t + 1 < nkt ? q.B.bytes : 0u);
            const u32x4_t rsB2 = rsrc_words(q.B.p, t + 2 < nkt ? q.B.bytes : 0u);
            const u32x4_t rsA2 = rsrc_words(q.A.p, t + 2 < nkt ? q.A.bytes : 0u);
            const uint32_t kb1 = kb0 + (uint32_t)(t + 1) * kb, kb2 = kb0 + (uint32_t)(t + 2) * kb, ka2 = ka0 + (uint32_t)(t + 2) * ka;
            char* const slot_lo = bring + s_lo * P4_BHALF;
            char* const slot_hi = bring + s_hi * P4_BHALF;
            // tile t+1: tokens 0-15 = half 2t+2 (slot s_nx), tokens 16-31 = half 2t+3 (slot s_lo, refilled below)
            const char* const next_half = bring + ((lq >> 1) ? s_lo : s_nx) * P4_BHALF;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (i < 7) rdA(sta, i + 1, (i + 1) & 1);
                else rdA(stn, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (CS) colsum1(i, i & 1);
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    mma1(i, j, i & 1);
                    if (i == 7) rdB(j, next_half);
                    // pieces: every B fragment of tile t has been read once mma(0, 3) is issued -- both half-slots are free from there
                    const int sl = 4 * i + j - 3;          // 0, 2, 4, .. 14 -> pieces 0 .. 7
                    if (sl >= 0 && sl < 16 && (sl & 1) == 0) {
                        const int pc = sl >> 1;
                        if (pc < 4) lds_dma16_asm(rsB1, slot_lo + pc * 1024, vob[4 + pc], kb1);          // half 2t+3: tokens 16-31 of tile t+1
                        else lds_dma16_asm(rsB2, slot_hi + (pc - 4) * 1024, vob[pc - 4], kb2);          // half 2t+4: tokens 0-15 of tile t+2
                    }
                    if (i == 7) lds_dma16_asm(rsA2, smem + (t & 1) * P4_ASTAGE + wave * 4096 + j * 1024, voa[j], ka2);
                    __builtin_amdgcn_sched_barrier(0);
                }
                if (i == 6) {          // X(t+1)
                    asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory");
                    __builtin_amdgcn_s_barrier();
                    asm volatile("" ::: "memory");
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            const int s = s_lo; s_lo = s_nx; s_nx = s_hi; s_hi = s;
        }
        __builtin_amdgcn_sched_barrier(0);
        if (P4_EPI_PRIO) __builtin_amdgcn_s_setprio(P4_EPI_PRIO);
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
    };

    if (!(slowA || slowB)) {
        if (do_colsum) k_loop(std::true_type{}); else k_loop(std::false_type{});
    } else {
        // ---- rare path (a delayed scale left its window): synchronous; the stage is written by ds_write from the operand's fp32 copy,
        // split with the exact scale of its recorded maxima (A: 32 tokens x 128 features by the workgroup; B: each wave its own 64 features)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // the early pieces have landed before anything is restaged
        if (slowA) sa = site_exact_scale(q.A.hdr, (float*)(smem + P4_LDS - 64), tid, 256);
        if (slowB) sb = site_exact_scale(q.B.hdr, (float*)(smem + P4_LDS - 64), tid, 256);
#pragma unroll 1
        for (int t = 0; t < nkt; ++t) {
            __syncthreads();
            const int k0 = kbeg + t * 32;
            if (slowA) {
#pragma unroll 1
                for (int e = tid; e < 32 * 32; e += 256) {          // 32 tokens x 32 float4
                    const int tk = e >> 5, f = (e & 31) * 4;
                    f32x4 x = {0.f, 0.f, 0.f, 0.f};
                    if (k0 + tk < kend && m0 + f < p.M) x = *(const f32x4*)(q.A.f32 + (size_t)(k0 + tk) * q.A.ldf + m0 + f);
                    tn_image_put(smem + tk * 512, f, x, sa, tk);
                }
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) lds_dma16_asm(rsA, smem + wave * 4096 + i * 1024, voa[i], ka0 + (uint32_t)t * ka);
            }
            if (slowB) {
#pragma unroll 1
                for (int e = lane; e < 32 * 16; e += 64) {          // 32 tokens x 16 float4 of the wave's 64 features
                    const int tk = e >> 4, f = (e & 15) * 4;
                    f32x4 x = {0.f, 0.f, 0.f, 0.f};
                    if (k0 + tk < kend && n0 + 64 * wn + f < p.N) x = *(const f32x4*)(q.B.f32 + (size_t)(k0 + tk) * q.B.ldf + n0 + 64 * wn + f);
                    tn_image_put(bring + (tk >> 4) * P4_BHALF + (tk & 15) * 256, f, x, sb, tk);
                }
            } else {
#pragma unroll
                for (int pc = 0; pc < 8; ++pc) lds_dma16_asm(rsB, bring + (pc >> 2) * P4_BHALF + (pc & 3) * 1024, vob[pc], kb0 + (uint32_t)t * kb);
            }
            dma_wait_barrier();
            const char* lh = bring + (lq >> 1) * P4_BHALF;
#pragma unroll
            for (int j = 0; j < NJ; ++j) rdB(j, lh);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                rdA(smem, i, i & 1);
                if (do_colsum) colsum1(i, i & 1);
#pragma unroll
                for (int j = 0; j < NJ; ++j) mma1(i, j, i & 1);
            }
        }
        __syncthreads();
    }

    // ---- outputs (gemm_planes_tn.h): gemm_pl_tn8's for one wave group, the four patch reads of a row block before its first store
    using G = TnOutGeom<1, true>;
    static_assert(G::BM == P4_BM && G::PATCH == P4_PATCH && G::LDS <= P4_LDS, "the patches where the NT epilogue has its own");
    tn_outputs<G>(p, q, acc, accb, smem, sa, sb, T, wave, lane);
}

}  // namespace segmm
