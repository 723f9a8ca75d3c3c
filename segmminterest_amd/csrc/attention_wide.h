// Fused attention backward (dQ + dK + dV) for WIDE heads: DH = 96 and 128.
//
// attn_bwd_fused_kernel (attention.h) keeps, per wave, the K and V row fragments and the K column fragments of its key tile
// and the dK / dV accumulators of that tile: 5 DH / 4 registers, 80 at DH = 64, under a bound of 128 (four waves per SIMD).  At
// DH = 128 the same set is 160 registers, the row fragments of a query tile another 64: instantiated as it stands the kernel
// pushes 300 - 600 bytes per lane through scratch.  This is the same kernel -- the same staging of the query side in chunks of
// 48 rows, the same products, the same ordered dQ accumulation in LDS, the same plane outputs and repair protocol, see the
// comment there -- with a register budget of its own:
//   * bounded for TWO waves per SIMD: a wave may use 256 registers, a workgroup has at most 8 waves (ATT_WIDE_MAXW);
//   * K is needed in both fragment forms (rows for S = Q K^T, columns for dQ = dS K).  Each wave copies the 16 whole rows of
//     its key tile into an LDS image of its own ([16][DH + 4], the row pitch of the staged query side) and reads both forms
//     from there, a 16-float segment or one key row at a time under the MFMAs of the one before.  Held in registers: the V row
//     fragments and the dK / dV accumulators, 3 DH / 4 = 96 at DH = 128;
//   * the wave index sits in a scalar register (readfirstlane), so tile offsets, block choices and buffer descriptors are
//     scalars; the row fragments of the query side are read segment by segment behind scheduling barriers, the query-tile loop
//     stays rolled, and the addresses of the staging and store loops are formed per chunk (opaque copies of the chunk start and
//     the thread index) -- each of these kept the compiler from stacking loads or hoisted addresses on top of the held set;
//   * a key block of more than 8 tiles (more than 128 keys) is taken in PASSES: wave w owns tiles w, w + nw, ... one after the
//     other.  A pass runs over all query chunks with its tile's fragments and accumulators in registers, exactly like the single
//     pass.  dQ sums over every key tile of the block, so a pass after the first starts a chunk's LDS accumulator from the sum
//     the pass before left in the fp32 dQ buffer instead of from zero (the thread that stored a float4 is the one that reads it
//     back); the last pass stores the result, the planes and the maxima.  A launch with several passes therefore writes the fp32
//     dQ buffer even under ATT_PLANES_ONLY / ATT_REPAIR (it carries the partial sums; consumers of a planes-only site do not
//     read it).  The order of every sum is fixed: bitwise reproducible.
// LDS at DH = 128 with 48 staged rows: 3 x [48][132] floats + 8.25 KB of K image and 1.25 KB of transpose scratch per wave +
// partials: 110 KB for the 3 waves of a 40-key block, 148 KB for the 7 of a 100-key block, 157 KB for 8 (125 KB for the merged
// short-head form with 32 rows and 4 waves; 84 / 114 / 122 KB at DH = 96): every launch below 160 KB, ONE workgroup per CU --
// all the registers allow an 8-wave workgroup, but a 3-wave workgroup leaves the CU at under one wave per SIMD.
// Compiler's view of every instance: profiles/attn_wide_heads_resources.txt (tools/attn_resource_table.py).
#pragma once
#include "attention.h"

namespace segmm {

constexpr int ATT_WIDE_MAXW = 8;

template <int DH, int NW, bool ONE, int QCH = ATT_FUSED_QCHUNK>
__global__ __launch_bounds__(64 * NW, 2) void attn_bwd_fused_wide_kernel(const AttnArgs p) {
    static_assert(att_wide(DH) && DH % 16 == 0 && NW <= ATT_WIDE_MAXW, "wide heads only");
    using C = AttnCfg<DH>;
    const DropCfg drop_ = drop_live(p.drop);
    constexpr int RS = att_lds_rs(DH);         // LDS row stride (floats)
    constexpr int TS = ATT_LDS_TS;             // row stride of the 16 x 16 transpose scratch
    constexpr int QC = QCH;                    // queries staged at a time (1 - 3 query tiles)
    constexpr int MAXQT = QC / 16;
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nw = blockDim.x >> 6;      // (wave: in a scalar register -- tile offsets and block choices are wave-uniform)
    const int l15 = lane & 15, g = lane >> 4;
    // p.hpb as in attn_bwd_fused_kernel: 0 / 1 one key block per launch, 2 both blocks (workgroup 2 bh + blk), 3 merged short heads
    constexpr bool CAN_MERGE = ONE && QCH < ATT_FUSED_QCHUNK;
    const bool merged = CAN_MERGE && p.hpb == 3;
    const int wg = xcd_remap(blockIdx.x, gridDim.x), bh = p.hpb == 2 ? wg >> 1 : wg, b = bh / p.H, h = bh % p.H;
    const int La_p = round16(p.La), Lb_p = round16(p.Lb), Tp = La_p + Lb_p, nta = La_p >> 4, ntb = Lb_p >> 4;
    const bool isa = merged ? wave < nta : (p.hpb == 2 ? (wg & 1) == 0 : p.hpb == 0);
    const int ntk = merged ? nta + ntb : (isa ? nta : ntb);          // key tiles of the workgroup
    if (wave >= ntk) return;                               // surplus wave, or empty block (CrossAtt / SelfAtt ablations)
    const int npass = merged ? 1 : (ntk + nw - 1) / nw;    // (the host merges only what fits one pass)
    const int wib = (merged && !isa) ? wave - nta : wave;  // this wave's place among the waves of ITS key block (the dQ turn order)
    const int nthr = 64 * min(ntk, nw);                    // surviving threads
    const int col0 = h * DH;
    const float* Qg = (isa || merged) ? p.Qa : p.Qb;      // (merged: Qa and Qb are both staged)
    float* dQg = isa ? p.dQa : p.dQb;
    _Float16* dQgp = isa ? p.dQap : p.dQbp;
    float s_q = ((merged ? (p.dQap || p.dQbp) : dQgp != nullptr) && p.sin_q) ? *p.sin_q : 0.f;
    const float* sin_k = isa ? p.sin_ka : p.sin_kb;
    float s_k = ((isa ? p.dKap : p.dKbp) && sin_k) ? *sin_k : 0.f;
    const bool repair = (p.pflags & ATT_REPAIR) != 0;
    const bool want_q = (merged ? (p.dQap || p.dQbp) : dQgp != nullptr) && p.sin_q, want_k = (isa ? p.dKap : p.dKbp) && sin_k;          // sites with plane outputs
    if (repair && merged) {          // (the decision to leave must be the same in every wave of the workgroup: both blocks' sites)
        const bool need_q = want_q && p.hdr_q[2] != 0.f;
        const bool need_ka = p.dKap && p.sin_ka && p.hdr_ka[2] != 0.f, need_kb = p.dKbp && p.sin_kb && p.hdr_kb[2] != 0.f;
        if (!need_q && !need_ka && !need_kb) return;
        s_q = need_q ? p.hdr_q[0] : 0.f;
        s_k = (isa ? need_ka : need_kb) ? (isa ? p.hdr_ka : p.hdr_kb)[0] : 0.f;
    } else if (repair) {
        const float* hk_ = isa ? p.hdr_ka : p.hdr_kb;
        const bool need_q = want_q && p.hdr_q[2] != 0.f, need_k = want_k && hk_[2] != 0.f;
        if (!need_q && !need_k) return;
        s_q = need_q ? p.hdr_q[0] : 0.f;
        s_k = need_k ? hk_[0] : 0.f;
    }
    const bool f32_q = !repair && !((p.pflags & ATT_PLANES_ONLY) && want_q);          // fp32 copies of dQ / of dK, dV
    const bool f32_k = !repair && !((p.pflags & ATT_PLANES_ONLY) && want_k);
    const int nQ = merged ? 2 : 1;                         // staged Q projections / dQ accumulators
    float* sQ0 = smem_f;                                   // [nQ][QC][RS] query rows of the current chunk
    float* sdO = sQ0 + nQ * QC * RS;
    float* sdQ0 = sdO + QC * RS;
    float* sQ = sQ0 + ((merged && !isa) ? QC * RS : 0);   // this wave's block: its Q rows, its dQ accumulator
    float* sdQ = sdQ0 + ((merged && !isa) ? QC * RS : 0);
    float* sKw = sdQ0 + nQ * QC * RS + wave * (16 * RS);                    // [16][RS] this wave's key tile: K rows, read in both fragment forms
    float* s_mx = sdQ0 + nQ * QC * RS + nw * (16 * RS);
    float* s_inv = s_mx + QC;
    float* s_D = s_inv + QC;
    float* s_tr = s_D + QC + wave * (16 * TS);                              // this wave's transpose scratch
    int* s_turn0 = (int*)(s_D + QC + nw * (16 * TS));                       // [nQ][4] whose turn it is to add dQ of query tile qt
    int* s_turn = s_turn0 + ((merged && !isa) ? 4 : 0);
    float* s_Dp = (float*)(s_turn0 + 4 * nQ);                               // [QC][DH/4] partial products dO . O
    uint8_t* qm = (uint8_t*)(s_Dp + QC * (DH / 4));                         // [QC] 1 valid query, 0 masked, 2 pad
    uint8_t* km = qm + QC;                                                  // [Tp]
    KeyBlocks<DH> kbk;
    kbk.init(p, b, col0, l15, g);
    stage_kmask(km, p.mka, p.mkb, b, p.La, p.Lb, La_p, Lb_p, nthr);
    const float fscale = p.scale;
    float am_q = 0.f, am_k = 0.f;

    for (int pass = 0; pass < npass; ++pass) {
        // ---- this wave's key tile of the pass; the waves WITH a tile are a prefix 0 .. k-1 (the dQ turn order counts them), the
        // others only stage and store
        const bool has = wave + pass * nw < ntk;
        const bool carry = pass > 0, last = pass + 1 == npass;
        const int jt = (isa ? 0 : nta) + wib + pass * nw;                       // padded key tile of this wave
        const int jp = 16 * jt + l15;                                           // this lane's key (padded index)
        const uint32_t tile_so = isa ? (uint32_t)(16 * jt) * kbk.pitch_a : (uint32_t)(16 * (jt - nta)) * kbk.pitch_b;
        float vf[C::KS];
        if (has) {                // V row fragments of the tile (global, fragment form) and its K rows (whole rows -> this wave's LDS image; pad
                                  // keys read the rows behind the block or, past the end of the tensor, zeros, like frag_load): their latency
                                  // hides under the staging
            const __amdgpu_buffer_rsrc_t rk = isa ? kbk.ka : kbk.kb;
            const uint32_t pitch = isa ? kbk.pitch_a : kbk.pitch_b;
            // (lane offsets from the tensor's start, the tile as the uniform offset: the addressing and range check of frag_load)
            const uint32_t kbase = (isa ? (uint32_t)(b * p.La) * (uint32_t)p.ldka : (uint32_t)(b * p.Lb) * (uint32_t)p.ldkb) * 4u + (uint32_t)col0 * 4u;
            if (isa) frag_load<DH>(vf, kbk.va, kbk.row_a, tile_so);
            else frag_load<DH>(vf, kbk.vb, kbk.row_b, tile_so);
#pragma unroll
            for (int i = 0; i < DH / 16; ++i) {          // 16 rows x DH / 4 float4 = DH / 16 per lane
                const int idx = 64 * i + lane, row = idx / (DH / 4), c4 = idx - row * (DH / 4);
                const f32x4 v = buf_load4(rk, kbase + (uint32_t)row * pitch + (uint32_t)c4 * 16u, tile_so);
                *(f32x4*)(sKw + row * RS + 4 * c4) = v;
            }
        } else {
#pragma unroll
            for (int c = 0; c < C::KS; ++c) vf[c] = 0.f;
        }
        f32x4 dk[C::CT], dv[C::CT];
#pragma unroll
        for (int ct = 0; ct < C::CT; ++ct) { dk[ct] = f32x4{0.f, 0.f, 0.f, 0.f}; dv[ct] = f32x4{0.f, 0.f, 0.f, 0.f}; }

        for (int q0_ = 0; ONE ? q0_ < 1 : q0_ < p.Lq; q0_ += QC) {
            // (opaque copy: the addresses of the staging and store loops are formed here, per chunk -- hoisted out of the pass loop they
            // would be carried through the products in registers the fragments and accumulators need)
            int q0 = q0_, tid = threadIdx.x;
            asm volatile("" : "+s"(q0), "+v"(tid));
            const int nq = min(QC, p.Lq - q0);                 // real queries of the chunk
            const int nqt = (nq + 15) >> 4;
            // stage whole rows (float4), rows >= nq zero; the dQ accumulator starts from zero or from the sum of the passes before;
            // partial products of D = rowsum(dO * O)
            for (int i = tid; i < QC * (DH / 4); i += nthr) {
                const int q = i / (DH / 4), c = (i - q * (DH / 4)) * 4;
                f32x4 va = {0.f, 0.f, 0.f, 0.f}, vo = va, oo = va, vb = va, acc0 = va;
                if (q < nq) {
                    const size_t row = (size_t)b * p.Lq + q0 + q;
                    va = *(const f32x4*)(Qg + row * p.ldq + col0 + c);
                    if (merged) vb = *(const f32x4*)(p.Qb + row * p.ldq + col0 + c);
                    vo = *(const f32x4*)(p.dO + row * p.lddo + col0 + c);
                    oo = *(const f32x4*)(p.O + row * p.ldo + col0 + c);
                    if (carry) acc0 = *(const f32x4*)(dQg + row * p.lddq + col0 + c);
                }
                *(f32x4*)((merged ? sQ0 : sQ) + q * RS + c) = va;
                *(f32x4*)(sdO + q * RS + c) = vo;
                *(f32x4*)((merged ? sdQ0 : sdQ) + q * RS + c) = acc0;
                if (merged) {
                    *(f32x4*)(sQ0 + (QC + q) * RS + c) = vb;
                    *(f32x4*)(sdQ0 + (QC + q) * RS + c) = f32x4{0.f, 0.f, 0.f, 0.f};
                }
                s_Dp[i] = (vo.x * oo.x + vo.y * oo.y) + (vo.z * oo.z + vo.w * oo.w);
            }
            for (int q = threadIdx.x; q < QC; q += nthr) {
                const bool in = q < nq;
                s_mx[q] = in ? p.lse[(size_t)bh * p.Lq + q0 + q] : 0.f;
                s_inv[q] = in ? p.lse[(size_t)p.B * p.H * p.Lq + (size_t)bh * p.Lq + q0 + q] : 0.f;
                qm[q] = in ? (p.mq[(size_t)b * p.Lq + q0 + q] ? 1 : 0) : 2;
            }
            if (threadIdx.x < 4 * nQ) s_turn0[threadIdx.x] = 0;
            __syncthreads();
            for (int q = threadIdx.x; q < QC; q += nthr) {     // D[q]: the DH/4 partials of the row in index order (deterministic)
                float d_ = 0.f;
#pragma unroll
                for (int j = 0; j < DH / 4; ++j) d_ += s_Dp[q * (DH / 4) + j];
                s_D[q] = d_;
            }
            __syncthreads();
            if (has) {
                const uint8_t kflag = km[jp];
#pragma unroll 1          // (unrolled, the next query tile's loads are moved up into this one's register peak: scratch at DH = 128)
                for (int qt = 0; qt < MAXQT; ++qt) {
                    if (qt < nqt) {
                        f32x4 sv = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
                        {   // row fragments (lane&15 = query): element k = 16 i + 4 g + e of the row, like frag_load -- taken one 16-float
                            // segment at a time, the next segment's LDS reads in flight under this one's 8 MFMAs.  The scheduling
                            // barriers keep the compiler from gathering all 2 KS reads in front of the products (64 more live
                            // registers at DH = 128: scratch)
                            const float* qrow_ = sQ + (16 * qt + l15) * RS + C::row_off(g);
                            const float* drow_ = sdO + (16 * qt + l15) * RS + C::row_off(g);
                            const float* krow_ = sKw + l15 * RS + C::row_off(g);          // (lane&15 = key)
                            f32x4 qv = *(const f32x4*)qrow_, dv_ = *(const f32x4*)drow_, kv = *(const f32x4*)krow_;
#pragma unroll
                            for (int i = 0; i < C::KS / 4; ++i) {
                                f32x4 qn = qv, dn = dv_, kn = kv;
                                if (i + 1 < C::KS / 4) {
                                    qn = *(const f32x4*)(qrow_ + 16 * (i + 1)); dn = *(const f32x4*)(drow_ + 16 * (i + 1));
                                    kn = *(const f32x4*)(krow_ + 16 * (i + 1));
                                }
#pragma unroll
                                for (int e = 0; e < 4; ++e) {
                                    sv = MFMA16(qv[e], kv[e], sv);
                                    dp = MFMA16(dv_[e], vf[4 * i + e], dp);
                                }
                                __builtin_amdgcn_sched_barrier(0);
                                qv = qn; dv_ = dn; kv = kn;
                            }
                        }
                        const f32x4 mxq = *(const f32x4*)(s_mx + 16 * qt + 4 * g), invq = *(const f32x4*)(s_inv + 16 * qt + 4 * g);
                        const f32x4 Dq = *(const f32x4*)(s_D + 16 * qt + 4 * g);
                        const uint32_t qfl = *(const uint32_t*)(qm + 16 * qt + 4 * g);
                        f32x4 Pv, dSv;
                        // dropout multipliers of this lane's 4 (query, key) elements: one hash per lane, exchanged inside the
                        // aligned 4-lane group (attn_bwd_fused_kernel); bit-identical to drop_mult1
                        uint32_t dw[4] = {0u, 0u, 0u, 0u};
                        if (drop_.p > 0.f) {
                            const int rr = l15 & 3;
                            const uint2 hw = drop_rand_quad(drop_, (((uint64_t)bh * p.Lq + (q0 + 16 * qt + 4 * g + rr)) * Tp + jp) >> 2);
                            const uint32_t a0 = quad_bcast<0>(hw.x), a1 = quad_bcast<1>(hw.x), a2 = quad_bcast<2>(hw.x), a3 = quad_bcast<3>(hw.x);
                            const uint32_t b0 = quad_bcast<0>(hw.y), b1 = quad_bcast<1>(hw.y), b2 = quad_bcast<2>(hw.y), b3 = quad_bcast<3>(hw.y);
                            const bool lo_word = rr < 2, hi_half = rr & 1;
                            const uint32_t w0 = lo_word ? a0 : b0, w1 = lo_word ? a1 : b1, w2 = lo_word ? a2 : b2, w3 = lo_word ? a3 : b3;
                            dw[0] = hi_half ? (w0 >> 16) : (w0 & 0xffffu); dw[1] = hi_half ? (w1 >> 16) : (w1 & 0xffffu);
                            dw[2] = hi_half ? (w2 >> 16) : (w2 & 0xffffu); dw[3] = hi_half ? (w3 >> 16) : (w3 & 0xffffu);
                        }
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const uint32_t qf_ = (qfl >> (8 * r)) & 0xff;
                            const bool valid = (qf_ == 1) && (kflag == 1);
                            float mult = 1.f;
                            if (drop_.p > 0.f && qf_ != 2) mult = (dw[r] >= drop_.thresh) ? drop_.scale : 0.f;
                            const float v = logit_xform(sv[r], valid, mult, fscale);
                            const float pr = (kflag == 2 || qf_ == 2) ? 0.f : fast_exp(v - mxq[r]) * invq[r];
                            Pv[r] = pr;
                            dSv[r] = valid ? pr * (dp[r] - Dq[r]) * mult * fscale : 0.f;
                        }
                        // column fragments from LDS: lane (c, g) takes rows 16 qt + 4 g + s4, head columns 16 ct + c
                        // (=> result register r of tile ct is head column 16 ct + 4 g + r: one float4 per tile)
#pragma unroll
                        for (int s4 = 0; s4 < 4; ++s4) {
                            const float* qr = sQ + (16 * qt + 4 * g + s4) * RS;
                            const float* dr = sdO + (16 * qt + 4 * g + s4) * RS;
#pragma unroll
                            for (int ct = 0; ct < C::CT; ++ct) {
                                const int cc = 16 * ct + l15;
                                dv[ct] = MFMA16(dr[cc], Pv[s4], dv[ct]);
                                dk[ct] = MFMA16(qr[cc], dSv[s4], dk[ct]);
                            }
                            __builtin_amdgcn_sched_barrier(0);          // (one query row's 2 CT LDS reads at a time, not all 8 CT)
                        }
                        // dS[query 4g+r][key l15] -> dS^T fragments (lane&15 = query, registers = keys 4g..4g+3) through the scratch
#pragma unroll
                        for (int r = 0; r < 4; ++r) s_tr[(4 * g + r) * TS + l15] = dSv[r];
                        __builtin_amdgcn_s_waitcnt(0xc07f);        // lgkmcnt(0): this wave's own LDS writes have landed
                        __builtin_amdgcn_wave_barrier();
                        const f32x4 dST = *(const f32x4*)(s_tr + l15 * TS + 4 * g);
                        __builtin_amdgcn_wave_barrier();
                        // dQ^T[c][query] = sum_key K[key][c] dS^T[key][query]: K column fragments from the LDS image -- lane (c, g) takes key
                        // row 4 g + s4, head columns CT c .. CT c + CT - 1 -- one key row at a time, the next one's reads under the MFMAs
                        f32x4 dqt[C::CT];
#pragma unroll
                        for (int ct = 0; ct < C::CT; ++ct) dqt[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
                        {
                            const float* kcol_ = sKw + (4 * g) * RS + C::CT * l15;
                            auto kc_row = [&](float (&f)[C::CT], int s4) {
                                if (C::CT % 4 == 0) {
#pragma unroll
                                    for (int i = 0; i < C::CT / 4; ++i) {
                                        const f32x4 v = *(const f32x4*)(kcol_ + s4 * RS + 4 * i);
                                        f[4 * i] = v.x; f[(4 * i + 1) % C::CT] = v.y; f[(4 * i + 2) % C::CT] = v.z; f[(4 * i + 3) % C::CT] = v.w;
                                    }
                                } else {          // CT = 6: 8-byte aligned
#pragma unroll
                                    for (int i = 0; i < C::CT / 2; ++i) {
                                        const float2 v = *(const float2*)(kcol_ + s4 * RS + 2 * i);
                                        f[2 * i] = v.x; f[2 * i + 1] = v.y;
                                    }
                                }
                            };
                            float kc0[C::CT], kc1[C::CT];
                            kc_row(kc0, 0);
#pragma unroll
                            for (int s4 = 0; s4 < 4; s4 += 2) {
                                kc_row(kc1, s4 + 1);
#pragma unroll
                                for (int ct = 0; ct < C::CT; ++ct) dqt[ct] = MFMA16(kc0[ct], dST[s4], dqt[ct]);
                                __builtin_amdgcn_sched_barrier(0);
                                if (s4 + 2 < 4) kc_row(kc0, s4 + 2);
#pragma unroll
                                for (int ct = 0; ct < C::CT; ++ct) dqt[ct] = MFMA16(kc1[ct], dST[s4 + 1], dqt[ct]);
                                __builtin_amdgcn_sched_barrier(0);
                            }
                        }
                        // ordered accumulation: lane (query l15, g) holds head columns CT*(4g + r) + ct (col_load mapping of kc),
                        // i.e. the 4*CT contiguous columns from 4*CT*g of row 16 qt + l15
                        if (wib > 0)
                            while (__hip_atomic_load(s_turn + qt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != wib) __builtin_amdgcn_s_sleep(1);
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                        {
                            float* row = sdQ + (16 * qt + l15) * RS + 4 * C::CT * g;
                            float t[4 * C::CT];
#pragma unroll
                            for (int r = 0; r < 4; ++r)
#pragma unroll
                                for (int ct = 0; ct < C::CT; ++ct) t[C::CT * r + ct] = dqt[ct][r];
#pragma unroll
                            for (int i = 0; i < C::CT; ++i) {
                                f32x4 a = *(f32x4*)(row + 4 * i);
                                a += f32x4{t[4 * i], t[4 * i + 1], t[4 * i + 2], t[4 * i + 3]};
                                *(f32x4*)(row + 4 * i) = a;
                            }
                        }
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                        if (lane == 0) __hip_atomic_store(s_turn + qt, wib + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                }
            }
            __syncthreads();                                   // every wave has added its dQ partials of this chunk
            asm volatile("" : "+v"(tid));                      // (the store addresses are formed here, not carried through the products)
            for (int blk = 0; blk < nQ; ++blk) {              // (merged: dQa from the first accumulator, dQb from the second)
                const float* acc_ = merged ? sdQ0 + blk * QC * RS : sdQ;
                float* dq_ = merged ? (blk == 0 ? p.dQa : p.dQb) : dQg;
                _Float16* dqp_ = merged ? (blk == 0 ? p.dQap : p.dQbp) : dQgp;
                for (int i = tid; i < nq * (DH / 4); i += nthr) {
                    const int q = i / (DH / 4), c = (i - q * (DH / 4)) * 4;
                    const size_t row = (size_t)b * p.Lq + q0 + q;
                    const f32x4 v = *(const f32x4*)(acc_ + q * RS + c);
                    if (f32_q || !last) *(f32x4*)(dq_ + row * p.lddq + col0 + c) = v;          // (!last: the sum so far, for the next pass)
                    if (last) {
                        if (s_q > 0.f && dqp_) {          // adjacent threads hold adjacent float4 groups of one row (DH / 4 even, col0 % 8 == 0)
                            if ((col0 & 7) == 0) plane_store4_pair(dqp_, p.lddq2, (long long)row, col0 + c, v, s_q);
                            else plane_store4(dqp_, p.lddq2, (long long)row, col0 + c, v, s_q);
                        }
                        am_q = absmax4(am_q, v);
                    }
                }
            }
            if ((!ONE && q0_ + QC < p.Lq) || !last) __syncthreads();       // the next staging overwrites what was just read
        }
        // dK / dV rows of this tile: lane (key l15, g), tile ct register r = head column 16 ct + 4 g + r
        if (has) {
            const bool ka = jp < La_p;
            const int jloc = ka ? jp : jp - La_p;
            const bool real = ka ? (jloc < p.La) : (jloc < p.Lb);
            if (real) {
                float* dKp = (ka ? p.dKa + (size_t)(b * p.La + jloc) * p.lddka : p.dKb + (size_t)(b * p.Lb + jloc) * p.lddkb) + col0;
                float* dVp = (ka ? p.dVa + (size_t)(b * p.La + jloc) * p.lddka : p.dVb + (size_t)(b * p.Lb + jloc) * p.lddkb) + col0;
                const long long krow = ka ? (long long)b * p.La + jloc : (long long)b * p.Lb + jloc;
                _Float16* dKpp = ka ? p.dKap : p.dKbp;
                _Float16* dVpp = ka ? p.dVap : p.dVbp;
                const int ldk2 = ka ? p.lddka2 : p.lddkb2;
#pragma unroll
                for (int ct = 0; ct < C::CT; ++ct) {
                    if (f32_k) {
                        *(f32x4*)(dKp + 16 * ct + 4 * g) = dk[ct];
                        *(f32x4*)(dVp + 16 * ct + 4 * g) = dv[ct];
                    }
                    if (s_k > 0.f) {          // lane (key, g) and lane (key, g ^ 1) hold the two halves of an aligned 8
                        if ((col0 & 7) == 0) {
                            plane_store4_x16(dKpp, ldk2, krow, col0 + 16 * ct + 4 * g, split4(dk[ct], s_k));
                            plane_store4_x16(dVpp, ldk2, krow, col0 + 16 * ct + 4 * g, split4(dv[ct], s_k));
                        } else {
                            plane_store4(dKpp, ldk2, krow, col0 + 16 * ct + 4 * g, dk[ct], s_k);
                            plane_store4(dVpp, ldk2, krow, col0 + 16 * ct + 4 * g, dv[ct], s_k);
                        }
                    }
                    am_k = absmax4(absmax4(am_k, dk[ct]), dv[ct]);
                }
            }
        }
    }
    {
        float* hk = isa ? p.hdr_ka : p.hdr_kb;
        float* slot = isa ? p.amax_ka : p.amax_kb;
        // the scale the planes were written with is recorded by ONE deterministic surviving wave per header (attn_bwd_fused_kernel)
        const bool hdr_writer = bh == 0 && wib == 0 && lane == 0;          // (merged: the first wave of each block for its key header)
        if (!repair) {          // (the repair pass leaves the headers as they are: every workgroup of it must read the same ones)
            if (s_k > 0.f) { site_commit(hk, am_k, blockIdx.x * nw + wave, s_k); if (hdr_writer) hk[0] = s_k; }
            else if (slot) amax_commit(slot, am_k, blockIdx.x * nw + wave);
            if (s_q > 0.f) { site_commit(p.hdr_q, am_q, blockIdx.x * nw + wave, s_q); if (hdr_writer) p.hdr_q[0] = s_q; }
            else if (p.amax_q) amax_commit(p.amax_q, am_q, blockIdx.x * nw + wave);
        }
    }
}

}  // namespace segmm
