// What the round-3 and round-6 NT plane GEMMs (gemm_planes8.h, gemm_planes4.h) share outside their k-loops, stated once:
//   * the buffer-store helpers of the epilogue and the probe stamps,
//   * nt_slow_stage / nt_dma_rows: the staging of the NT kernels' rare path (an operand whose delayed scale left its window),
//   * nt_epilogue: the whole NT epilogue, from the accumulators to the site header's commit.
// The operand state and the repair verdict of the kernels come from common.h (site_words / site_scale / site_usable / site_state);
// the rule is site_window_ok everywhere.  The segment closers of gemm_pl_nt8 live here because the epilogue uses one.
#pragma once
#include "gemm_planes.h"

namespace segmm {

typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
// 16-byte buffer store.  The data registers of a store wider than 8 bytes must not be overwritten for a few cycles after it
// issues; hipcc pads that hazard only when the scalar-offset field is an immediate (GCNHazardRecognizer assumes it does not
// exist with a register there) -- on gfx950 it does: with soffset in an SGPR and the next v_pk_fma_f32 reusing the data
// registers, lanes 12-15 stored the NEXT float4's .y/.w (tools/probe/dbg_fast.py).  The wait states are written out, in an asm
// statement that READS the data registers, so no write to them can be scheduled in front of it.
// Cache policy of the NT kernels' epilogue stores: nt (aux bit 1).  The outputs of a GEMM are written once and read by a LATER kernel;
// kept in the XCD's L2 like ordinary stores they push out the operand panels the other workgroups of the launch are still reading
// (tools/probe/gemm4_bench.hip, -DSEGMM_STORE_AUX=0 / 2 / 16: gemm_pl_nt4 20480 x 3072 x 768 228.4 -> 215.7 us, 51200 x 768 x 768
// 150.0 -> 133.8 us; gemm_pl_nt8 +2 .. 7 %; sc1 alone +1.5 %; in the step +0.4 % -- the consumers find the data in the Infinity
// Cache).  The split-K slabs of the TN kernels are read back by splitk_reduce at once: they keep the default policy (buf_store4k).
#ifndef SEGMM_STORE_AUX
#define SEGMM_STORE_AUX 2          // 0 default policy, 1 sc0, 2 nt, 16 sc1
#endif
#ifndef SEGMM_PLANE_AUX
#define SEGMM_PLANE_AUX SEGMM_STORE_AUX          // probe: cache policy of the plane OUTPUT stores (the next GEMM / attention reads them at once)
#endif
template <int AUX>
__device__ __forceinline__ void buf_store4u_aux(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff, u32x4_t v) {
    __builtin_amdgcn_raw_buffer_store_b128(v, r, (int)voff, (int)soff, AUX);
    asm volatile("s_nop 3" :: "v"(v));
}
// (same-box check of small outputs, 20480 x 768 x 768 = 63 MB: 60.3 us default, 57.9 us nt -- no size threshold needed)
__device__ __forceinline__ void buf_store4u(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff, u32x4_t v) { buf_store4u_aux<SEGMM_STORE_AUX>(r, voff, soff, v); }
__device__ __forceinline__ void buf_store4(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff, f32x4 v) {
    buf_store4u(r, voff, soff, __builtin_bit_cast(u32x4_t, v));
}
__device__ __forceinline__ void buf_store4k(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff, f32x4 v) {          // "keep": default cache policy
    buf_store4u_aux<0>(r, voff, soff, __builtin_bit_cast(u32x4_t, v));
}
__device__ __forceinline__ float buf_load1(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff) {
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, (int)voff, (int)soff, 0));
}
constexpr uint32_t BUF_OOB = 0x80000000u;          // a byte offset no descriptor of ours covers: the access is dropped / reads 0

#ifdef SEGMM_STAMPS
// diagnostic build only: shader-clock / real-time stamps of the kernel's sections, 8 x u64 per workgroup
#define STAMP(k) do { if (q.stamps && threadIdx.x == 0) { q.stamps[(size_t)blockIdx.x * 8 + (k)] = __builtin_amdgcn_s_memtime(); \
                                                           if ((k) == 0 || (k) == 3) q.stamps[(size_t)blockIdx.x * 8 + 4 + ((k) ? 1 : 0)] = __builtin_amdgcn_s_memrealtime(); \
                                                           if ((k) == 0) q.stamps[(size_t)blockIdx.x * 8 + 6] = (unsigned long long)__builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11)) | ((unsigned long long)__builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (3 << 11)) << 32); \
                                                           if ((k) == 2) q.stamps[(size_t)blockIdx.x * 8 + 7] = __builtin_amdgcn_s_memrealtime(); } } while (0)
// second region (16 x u64 per workgroup behind the 8 x u64 records): finer stamps inside a section
#define STAMPX(k) do { if (q.stamps && threadIdx.x == 0) q.stamps[(size_t)gridDim.x * 8 + (size_t)blockIdx.x * 16 + (k)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define STAMP(k) do { } while (0)
#define STAMPX(k) do { } while (0)
#endif

// ---- closers of gemm_pl_nt8's load / compute segments; the epilogue of both NT kernels closes its E quarters with end_load_segment
#ifndef SEGMM_SETPRIO
#define SEGMM_SETPRIO 0          // probe: raise the wave priority for the compute segments (s_setprio 1 ... 0)
#endif
template <int NOUT>          // number of LDS-DMA pieces this wave may leave in flight (0 .. 4)
__device__ __forceinline__ void end_compute_segment() {
    __builtin_amdgcn_sched_barrier(0);
    if (SEGMM_SETPRIO) __builtin_amdgcn_s_setprio(0);
    if (NOUT == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else if (NOUT == 3) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
    else if (NOUT == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
}
__device__ __forceinline__ void end_load_segment() {
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (SEGMM_SETPRIO) __builtin_amdgcn_s_setprio(1);
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
}

// ================================================================ rare path of the NT kernels: staging of one k-tile
// (a delayed scale left its window: synchronous, one stage).  NTHR = threads of the workgroup.  An operand whose planes are
// unusable is split from its fp32 copy at the exact scale (nt_slow_stage), the other one comes by LDS-DMA (nt_dma_rows); both
// fill `dst` with ntrows rows of 128 B in the k-loop's image (chunk c of row r at physical chunk c ^ ((r >> 1) & 7)).
template <int NTHR>
__device__ __forceinline__ void nt_slow_stage(const PlaneOperand& op, float sc, int row0, int nrows, int ntrows, int kt, char* dst, int tid) {
#pragma unroll 1
    for (int j = tid; j < ntrows * 4; j += NTHR) {
        const int row = j >> 2, kc = j & 3;
        const float* src = op.f32 + (size_t)min(row0 + row, nrows - 1) * op.ldf + kt * 32 + kc * 8;
        const f32x4 x0 = *(const f32x4*)src, x1 = *(const f32x4*)(src + 4);
        uint32_t h0, l0, h1, l1, h2, l2, h3, l3;
        splith_pair(x0.x, x0.y, sc, h0, l0); splith_pair(x0.z, x0.w, sc, h1, l1);
        splith_pair(x1.x, x1.y, sc, h2, l2); splith_pair(x1.z, x1.w, sc, h3, l3);
        const int sw = (row >> 1) & 7;
        *(uint4*)(dst + row * 128 + ((kc ^ sw) << 4)) = make_uint4(h0, h1, h2, h3);
        *(uint4*)(dst + row * 128 + (((4 + kc) ^ sw) << 4)) = make_uint4(l0, l1, l2, l3);
    }
}
template <int NTHR>
__device__ __forceinline__ void nt_dma_rows(__amdgpu_buffer_rsrc_t rs, const PlaneOperand& op, int row0, int nrows, int ntrows, int kt, char* dst,
                                            int wave, int lane) {
    const int r8 = lane >> 3;
#pragma unroll 1
    for (int pc = wave; pc < ntrows / 8; pc += NTHR / 64) {
        const int row = pc * 8 + r8;
        lds_dma16(rs, dst + pc * 1024, (uint32_t)min(row0 + row, nrows - 1) * (uint32_t)op.ld2 * 2u +
                  (uint32_t)(((lane & 7) ^ ((row >> 1) & 7)) * 16), (uint32_t)kt * 128u);
    }
}

// ================================================================ the NT epilogue
// Geometry of a kernel's tile, fixed at compile time.  A workgroup is GROUPS wave groups of four waves; group g owns rows
// [128 g, +128) of the tile, wave wn of a group the columns [16 NJ wn, +16 NJ): gemm_pl_nt8<NJ> has two groups (tile 256 x 64 NJ),
// gemm_pl_nt4 one (128 x 256).  Everything else follows: a quarter of the tile's extra operand is 32 rows x 1 KB per group
// (EHALF), the per-wave transpose patches sit behind the two E halves (PATCH), the commit keys count WAVES per workgroup.
// READS_FIRST: request all four reads of the transpose patch before the first store of a row block.  A read issued right in front
// of the store that needs it exposes one LDS round trip per store -- 32 per tile, ~130 cycles each on an idle LDS and three times
// that beside the partner workgroup's k-loop (gemm_pl_nt4, measured: 13.7 k cycles per epilogue); gemm_pl_nt8 owns its CU and
// keeps the interleaved order it was tuned with.
template <int NJ_, int GROUPS_, bool READS_FIRST_>
struct NtEpiGeom {
    static constexpr int NJ = NJ_, GROUPS = GROUPS_, WAVES = 4 * GROUPS_;
    static constexpr int BM = 128 * GROUPS_, BN = 64 * NJ_;          // tile extents
    static constexpr int EHALF = 32 * GROUPS_ * 1024;                // one of the two LDS halves a quarter of E lands in
    static constexpr int PATCH = 2 * EHALF;                          // 4 KB transpose patch per wave from here
    static constexpr int LDS = PATCH + WAVES * 4096;                 // what the epilogue needs of the kernel's LDS
    static constexpr bool READS_FIRST = READS_FIRST_;
};

// lane holds C[gm = m0 + 128 grp + 16 i + l15][gn = n0 + 16 NJ wn + 16 j + 4 lq .. + 3] of accumulator tile (i, j) (the MFMA
// operands are swapped: the tile is C^T, a lane has four consecutive columns of one row).  Row blocks i are walked in a rolled
// loop (the element-wise body is emitted NJ times, not 8 NJ).  Every wave has passed the k-loop's last barrier with its LDS
// reads retired, so the whole of smem[0, G::LDS) is free.
//
// The "extra operand" E of an element -- the residual, or the aux tensor an activation gradient reads (the host routes
// launches that would need both to gemm_pl_nt) -- is staged through LDS by LDS-DMA, a quarter of the tile (32 rows x 1 KB of
// every wave group: row blocks 2 q, 2 q + 1) at a time into the two halves at the bottom of the LDS.  Why not plain
// loads: vmcnt returns in ISSUE ORDER on gfx9, stores included -- a load queued behind the stores of the previous row block
// cannot come back before those stores are acknowledged (~2 us under load), which serialised the whole epilogue (20 us per
// tile).  Quarters 0 and 1 are requested before the first store, quarter q + 2 after the stores of quarter q: every wait
// is for pieces that sit in front of stores issued a quarter earlier at least.  No extra operand: no loads, no waits, no
// barriers.  Registers: none (the ring of prefetched rows it replaces spilled).
//
// sa, sb: the scales the operands were multiplied with; c_scale: the scale of the plane output (0: none; on a repair launch the
// exact scale of the recorded maxima).  Ends with the commit of the tile's maximum to the site header (not on a repair
// launch: the header keeps the first launch's verdict).
template <class G>
__device__ __forceinline__ void nt_epilogue(const GemmArgs& p, const PGemmX& q, f32x4 (&acc)[8][G::NJ], char* smem, float sa, float sb,
                                            float c_scale, int m0, int n0, int wave, int lane) {
    constexpr int NJ = G::NJ;
    const int grp = G::GROUPS > 1 ? wave >> 2 : 0, wn = G::GROUPS > 1 ? wave & 3 : wave;
    const int l15 = lane & 15, lq = lane >> 4;
    float am = 0.f;
    if (SEGMM_GEMM_DBG(q) & 2) {
        float t = 0.f;          // timing ablation: keep every accumulator alive, skip the epilogue
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j) t += acc[i][j].x + acc[i][j].y + acc[i][j].z + acc[i][j].w;
        if (t == 1.2345f) p.C[0] = 1.f;
    } else {
        const float inv_ab = (1.f / sa) * (1.f / sb);          // exact powers of two
        const int epi = p.epi;
        const bool has_res = p.residual != nullptr, has_drop = p.drop.p > 0.f;
        const DropCfg drop_e = drop_live(p.drop);
        const bool aux_r = epi == EPI_DGELU || epi == EPI_DRELU, aux_w = epi == EPI_GELU;
        const bool planes = c_scale > 0.f && q.Cp != nullptr;
        const bool store_c = q.write_c && !(SEGMM_GEMM_DBG(q) & 1);
        const bool periodic = has_res && p.res_period < p.M;
        const int res_rows = has_res ? min(p.res_period, p.M) : 0;
        const bool has_e = has_res || aux_r;
        auto ext = [&](bool on, long long rows, long long ld, long long elt) -> uint32_t {      // view extent in bytes (0: absent)
            if (!on || rows <= 0) return 0u;
            return (uint32_t)(((rows - 1) * ld + p.N) * elt);          // < 2^31 (checked by the host)
        };
        const __amdgpu_buffer_rsrc_t rsC = make_rsrc(p.C, ext(store_c, p.M, p.ldc, 4));
        const __amdgpu_buffer_rsrc_t rsAuxW = make_rsrc(p.aux, ext(aux_w, p.M, p.ldaux, 4));
        const __amdgpu_buffer_rsrc_t rsE = aux_r ? make_rsrc(p.aux, ext(true, p.M, p.ldaux, 4)) : make_rsrc(p.residual, ext(has_res, res_rows, p.ldr, 4));
        const int ldE = aux_r ? p.ldaux : p.ldr;
        // planes: [M][ldc2] halves, a row holds 2 N halves
        const __amdgpu_buffer_rsrc_t rsPl = make_rsrc(q.Cp, planes ? (uint32_t)((((long long)p.M - 1) * q.ldc2 + 2ll * p.N) * 2) : 0u);
        const int ns = (store_c ? 1 : 0) + (planes ? 1 : 0) + (aux_w ? 1 : 0);          // store instructions per float4

        const int gm0 = m0 + grp * 128 + l15;
        const int gn0 = n0 + wn * 16 * NJ + 4 * lq;
        uint32_t colmask[NJ];          // 0 or BUF_OOB: columns beyond N are pushed out of every descriptor's range
        f32x4 bias4[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int gn = gn0 + 16 * j;
            colmask[j] = gn < p.N ? 0u : BUF_OOB;
            bias4[j] = (p.bias && gn < p.N) ? *(const f32x4*)(p.bias + gn) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
        const bool full_tile = m0 + G::BM <= p.M && n0 + G::BN <= p.N;
        // E quarter qq -> LDS half (qq & 1): slot s = 32 g + r (g = wave group, r = row inside the group's 32 rows of the quarter) at
        // byte s * 1024; 16-byte chunk c of the row at physical chunk c ^ (row & 15) (conflict-free ds_read_b128 of the accumulator
        // layout: 16 rows x 4 chunks per instruction); the permutation is applied to the DMA source address
        auto dmaE = [&](int qq) {
            char* dst = smem + (qq & 1) * G::EHALF;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int slot = wave * 8 + k;
                const int R = G::GROUPS > 1 ? (slot >> 5) * 128 + qq * 32 + (slot & 31) : qq * 32 + slot;          // tile row (wave-uniform)
                const int gmR = m0 + R;
                const int er = aux_r ? gmR : (periodic ? gmR % p.res_period : gmR);
                const int ch = lane ^ (R & 15);
                const uint32_t vo = (ch < 16 * NJ && n0 + 4 * ch < p.N) ? (uint32_t)ch * 16u : BUF_OOB;
                lds_dma16e(rsE, dst + slot * 1024, vo, ((uint32_t)er * (uint32_t)ldE + (uint32_t)n0) * 4u);
            }
        };
        auto vmwait = [&](int kind) {          // kind 0: 8 newer ops; 1: S + 8; 2: S newer ops, S = 8 ns store instructions of the last quarter
            __builtin_amdgcn_sched_barrier(0);          // (2 row blocks x 4 row-segment stores per output tensor)
            if (kind == 0) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
            else if (ns == 1) { if (kind == 1) asm volatile("s_waitcnt vmcnt(16)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); }
            else if (ns == 2) { if (kind == 1) asm volatile("s_waitcnt vmcnt(24)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(16)" ::: "memory"); }
            else if (ns == 3) { if (kind == 1) asm volatile("s_waitcnt vmcnt(32)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(24)" ::: "memory"); }
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
        };
        // ---- stores.  In the accumulator layout a lane owns 16 bytes of ITS row: the 16 lanes of a quarter-wave touch 16
        // different cache lines, 64 sixteen-byte transactions per store instruction -- 18.8 k cycles to drain a 256 KB tile on an
        // otherwise idle chip against 5.4 k for stores that cover 256 contiguous bytes per quarter-wave (tools/probe/store_rate.hip).
        // Each 16-row x 16 NJ-column strip therefore takes a detour through a wave-private 4 KB LDS patch (chunk c of row r at
        // physical chunk c ^ r: conflict-free both ways) and is stored as whole 64 NJ-byte row segments: lane (lq, l15) of pass t
        // stores row 4 t + lq, columns 4 l15 .. 4 l15 + 3 of the strip.
        char* trp = smem + G::PATCH + wave * 4096;
        const uint32_t tr_w = (uint32_t)(l15 * 256);                                   // + ((lq + 4 j) ^ l15) << 4
        const int gnT = n0 + wn * 16 * NJ + 4 * l15;
        const uint32_t tmask = (l15 < 4 * NJ && gnT < p.N) ? 0u : BUF_OOB;
        const uint32_t oCT = (((uint32_t)(m0 + grp * 128 + lq) * (uint32_t)p.ldc + (uint32_t)gnT) * 4u) | tmask;
        const uint32_t oAuxT = (((uint32_t)(m0 + grp * 128 + lq) * (uint32_t)p.ldaux + (uint32_t)gnT) * 4u) | tmask;
        auto tr_put = [&](int j, f32x4 v) { *(f32x4*)(trp + tr_w + (((lq + 4 * j) ^ l15) << 4)) = v; };
        auto tr_get = [&](int t) { const int r = 4 * t + lq; return *(const f32x4*)(trp + r * 256 + (((l15 ^ r) & 15) << 4)); };
        // the four row segments of the strip in the patch: all requested here (READS_FIRST), or each in front of its store
        auto tr_rows = [&](f32x4 (&g)[4]) {
            if (G::READS_FIRST) {
#pragma unroll
                for (int t = 0; t < 4; ++t) g[t] = tr_get(t);
            }
        };
        // planes of a transposed float4: adjacent lanes hold adjacent column groups of one row (plane_store4_pair's pattern)
        const uint32_t oPlT = (((uint32_t)(m0 + grp * 128 + lq) * (uint32_t)q.ldc2 + (uint32_t)((((gnT & ~7) >> 5) << 6) + ((gnT & ~7) & 31) + ((l15 & 1) ? 32 : 0))) * 2u) | tmask;

        // The row-block loop exists in twelve copies -- activation class (none / ReLU-type / GELU-type) x dropout x plane output
        // fixed at compile time -- picked once per tile: with every option tested inside ONE body, the dozen taken branches per
        // float4 (each hopping over an inlined erf) and ~60 VALU instructions cost more than the stores (21 k cycles per tile,
        // the same on an idle chip).
        if (has_e) { dmaE(0); dmaE(1); }
        const uint32_t e_lane = (uint32_t)((grp * 32 + l15) * 1024);          // + 16384 for odd row blocks; chunk ((4 NJ wn + 4 j + lq) ^ l15) * 16
        auto row_loop = [&](auto act_tag, auto drop_tag, auto pl_tag) {
            constexpr int ACT = decltype(act_tag)::value;          // 0 none, 1 ReLU / ReLU', 2 GELU / GELU'
            constexpr bool DROP = decltype(drop_tag)::value, PLANES = decltype(pl_tag)::value;
#pragma unroll 1
            for (int i = 0; i < 8; ++i) {
                if (has_e && (i & 1) == 0) vmwait(i == 0 ? 0 : (i == 6 ? 2 : 1));          // quarter i / 2 has landed (all waves: barrier)
                f32x4 c[NJ];
                switch (i) {
                    case 0: for (int j = 0; j < NJ; ++j) c[j] = acc[0][j]; break;
                    case 1: for (int j = 0; j < NJ; ++j) c[j] = acc[1][j]; break;
                    case 2: for (int j = 0; j < NJ; ++j) c[j] = acc[2][j]; break;
                    case 3: for (int j = 0; j < NJ; ++j) c[j] = acc[3][j]; break;
                    case 4: for (int j = 0; j < NJ; ++j) c[j] = acc[4][j]; break;
                    case 5: for (int j = 0; j < NJ; ++j) c[j] = acc[5][j]; break;
                    case 6: for (int j = 0; j < NJ; ++j) c[j] = acc[6][j]; break;
                    default: for (int j = 0; j < NJ; ++j) c[j] = acc[7][j]; break;
                }
                const int gm = gm0 + 16 * i;
                const uint32_t rowmask = gm < p.M ? 0xffffffffu : 0u;
                const uint32_t soC = (uint32_t)i * 16u * (uint32_t)p.ldc * 4u, soAux = (uint32_t)i * 16u * (uint32_t)p.ldaux * 4u;
                const char* ebuf = smem + ((i >> 1) & 1) * G::EHALF + e_lane + (i & 1) * 16384;
                f32x4 e[NJ];
#pragma unroll
                for (int j = 0; j < NJ; ++j) e[j] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (has_e) {
#pragma unroll
                    for (int j = 0; j < NJ; ++j) e[j] = *(const f32x4*)(ebuf + (((4 * NJ * wn + 4 * j + lq) ^ l15) << 4));
                }
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    f32x4 v = c[j] * inv_ab + bias4[j];
                    if (ACT == 2) {
                        if (epi == EPI_GELU) {
                            tr_put(j, v);          // the pre-activation leaves through the transpose patch below
                            v.x = gelu_erf(v.x); v.y = gelu_erf(v.y); v.z = gelu_erf(v.z); v.w = gelu_erf(v.w);
                        } else {
                            v.x *= gelu_erf_grad(e[j].x); v.y *= gelu_erf_grad(e[j].y); v.z *= gelu_erf_grad(e[j].z); v.w *= gelu_erf_grad(e[j].w);
                        }
                    } else if (ACT == 1) {
                        if (epi == EPI_RELU) {
                            v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
                        } else {
                            v.x = e[j].x > 0.f ? v.x : 0.f; v.y = e[j].y > 0.f ? v.y : 0.f; v.z = e[j].z > 0.f ? v.z : 0.f; v.w = e[j].w > 0.f ? v.w : 0.f;
                        }
                    }
                    if (DROP) v = drop_apply4(drop_e, ((uint64_t)gm * (uint64_t)p.N + (uint64_t)(gn0 + 16 * j)) >> 2, v);
                    if (ACT == 0) v += e[j];                    // e = 0 without a residual
                    else if (has_res) v += e[j];                // (e is the aux tensor of an activation gradient otherwise)
                    c[j] = v;
                    {          // running max |v| over the elements that exist (branch-free: rows / columns beyond the matrix are masked to 0)
                        const uint32_t mk = rowmask & ~((int32_t)colmask[j] >> 31);
                        const float mx = __uint_as_float(__float_as_uint(v.x) & mk), my = __uint_as_float(__float_as_uint(v.y) & mk);
                        const float mz = __uint_as_float(__float_as_uint(v.z) & mk), mw = __uint_as_float(__float_as_uint(v.w) & mk);
                        asm("v_max3_f32 %0, |%1|, |%2|, %0" : "+v"(am) : "v"(mx), "v"(my));
                        asm("v_max3_f32 %0, |%1|, |%2|, %0" : "+v"(am) : "v"(mz), "v"(mw));
                    }
                }
                f32x4 g4[4];
                if (ACT == 2 && epi == EPI_GELU) {          // the pre-activations (put above), as whole row segments
                    tr_rows(g4);
#pragma unroll
                    for (int t = 0; t < 4; ++t)
                        buf_store4(rsAuxW, oAuxT, soAux + (uint32_t)(4 * t) * (uint32_t)p.ldaux * 4u, G::READS_FIRST ? g4[t] : tr_get(t));
                }
#pragma unroll
                for (int j = 0; j < NJ; ++j) tr_put(j, c[j]);
                tr_rows(g4);
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const f32x4 v = G::READS_FIRST ? g4[t] : tr_get(t);
                    buf_store4(rsC, oCT, soC + (uint32_t)(4 * t) * (uint32_t)p.ldc * 4u, v);
                    if (PLANES) {
                        // adjacent lanes hold adjacent float4 column groups of one row: the pair trades half of its terms through
                        // DPP -- the even lane stores the 8 hi terms, the odd lane the 8 lo terms of the aligned 8 columns
                        uint32_t h0, l0, h1, l1;
                        splith_pair(v.x, v.y, c_scale, h0, l0);
                        splith_pair(v.z, v.w, c_scale, h1, l1);
                        const bool oddl = (l15 & 1) != 0;
                        const uint32_t r0 = dpp_swap1(oddl ? h0 : l0), r1 = dpp_swap1(oddl ? h1 : l1);
                        const u32x4_t w = oddl ? u32x4_t{r0, r1, l0, l1} : u32x4_t{h0, h1, r0, r1};
                        buf_store4u_aux<SEGMM_PLANE_AUX>(rsPl, oPlT, (uint32_t)(16 * i + 4 * t) * (uint32_t)q.ldc2 * 2u, w);
                    }
                }
                if (has_e && (i & 1) == 1 && i < 5) {          // both row blocks of the quarter are read: refill its half with quarter + 2
                    end_load_segment();
                    dmaE((i >> 1) + 2);
                }
            }
        };
        // The common case -- a whole tile, no activation, no dropout, no plane output (the fused projections, the input-gradient
        // GEMMs): fully unrolled, ~6 instructions per float4 (the rolled loop spends ~1 200 cycles per row block on its 8-way
        // accumulator switch and scalar bookkeeping: 9.5 k cycles per tile before the first byte is stored)
        auto fast_loop = [&](auto e_tag) {
            constexpr bool HAS_E = decltype(e_tag)::value;
            const bool raw = (SEGMM_GEMM_DBG(q) & 8) != 0;          // timing ablation: no LDS transposition (wrong layout)
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (HAS_E && (i & 1) == 0) vmwait(i == 0 ? 0 : (i == 6 ? 2 : 1));
                const uint32_t soC = (uint32_t)i * 16u * (uint32_t)p.ldc * 4u;
                const char* ebuf = smem + ((i >> 1) & 1) * G::EHALF + e_lane + (i & 1) * 16384;
                f32x4 g4[4];
                if (raw) {
#pragma unroll
                    for (int t = 0; t < 4; ++t) { g4[t] = acc[i][t % NJ] * inv_ab + bias4[t % NJ]; am = fmaxf(am, g4[t].x); }
                } else {
#pragma unroll
                    for (int j = 0; j < NJ; ++j) {
                        f32x4 v = acc[i][j] * inv_ab + bias4[j];
                        if (HAS_E) v += *(const f32x4*)(ebuf + (((4 * NJ * wn + 4 * j + lq) ^ l15) << 4));
                        asm("v_max3_f32 %0, |%1|, |%2|, %0" : "+v"(am) : "v"(v.x), "v"(v.y));
                        asm("v_max3_f32 %0, |%1|, |%2|, %0" : "+v"(am) : "v"(v.z), "v"(v.w));
                        tr_put(j, v);
                    }
                    tr_rows(g4);
                }
                auto row = [&](int t) { return (G::READS_FIRST || raw) ? g4[t] : tr_get(t); };
                if (SEGMM_GEMM_DBG(q) & 4) {          // timing ablation: no store instructions
#pragma unroll
                    for (int t = 0; t < 4; ++t) { const f32x4 v = row(t); am = fmaxf(am, v.x + v.y + v.z + v.w); }
                } else {
#pragma unroll
                    for (int t = 0; t < 4; ++t) buf_store4(rsC, oCT, soC + (uint32_t)(4 * t) * (uint32_t)p.ldc * 4u, row(t));
                }
                STAMPX(i);
                if (HAS_E && (i & 1) == 1 && i < 5) {
                    end_load_segment();
                    dmaE((i >> 1) + 2);
                }
            }
        };
        const bool fast = full_tile && epi == EPI_NONE && !has_drop && !planes;
        if (fast) {
            if (has_e) fast_loop(std::true_type{}); else fast_loop(std::false_type{});
        } else {
            using A0 = std::integral_constant<int, 0>; using A1 = std::integral_constant<int, 1>; using A2 = std::integral_constant<int, 2>;
            using T = std::true_type; using F = std::false_type;
            auto pick = [&](auto act_tag) {
                if (has_drop) { if (planes) row_loop(act_tag, T{}, T{}); else row_loop(act_tag, T{}, F{}); }
                else { if (planes) row_loop(act_tag, F{}, T{}); else row_loop(act_tag, F{}, F{}); }
            };
            if (epi == EPI_GELU || epi == EPI_DGELU) pick(A2{});
            else if (epi == EPI_RELU || epi == EPI_DRELU) pick(A1{});
            else pick(A0{});
        }
    }
    STAMP(3);
    if (q.repair) return;          // (the header keeps the first launch's verdict)
    if (q.c_hdr) {
        site_commit(q.c_hdr, am, blockIdx.x * G::WAVES + wave, c_scale);
        if (c_scale > 0.f && scale_writer(blockIdx.x * G::WAVES + wave)) q.c_hdr[0] = c_scale;
    } else if (p.amax_out) amax_commit(p.amax_out, am, blockIdx.x * G::WAVES + wave);
}

}  // namespace segmm
