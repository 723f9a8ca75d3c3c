// Streamed attention: any number of key tiles (up to 16 + 16: two key blocks of at most 256 tokens), nothing held per tile.
//
// The forward and the dQ kernel of attention.h keep one thing per key tile in registers -- attn_fwd_kernel its scores
// (f32x4 acc[NT]), attn_bwd_dq_kernel only an unroll bound -- and are built for NT <= 12.  The two kernels here are the same
// kernels with the key tiles in a RUN-TIME loop: one wave per 16-query tile, operands straight from global memory in fragment
// form (KeyBlocks / frag_load / col_load), key flags from stage_kmask, no LDS beyond the flags, no barrier after the staging
// barrier, no atomics (attn_D_stream_kernel: no LDS at all).  The dK/dV kernel (attn_bwd_dkv_kernel<DH, 0>) already walks its query tiles in a run-time loop, one wave
// per key tile, and serves any tile count as it stands.
//
// Forward: online softmax.  Per key tile t: S^T_t = K_t.Q^T, logit_xform / pad rule / dropout exactly as attn_fwd_kernel (same
// dropout index, so the backward kernels regenerate the same mask), tile row max (register-local + two shuffles), then
//     m' = max(m, max_t);  a = exp(m - m');  l = a l + rowsum(exp(S_t - m'));  O^T = a O^T + V_t^T exp(S_t - m')
// The O^T accumulators have the query on lane & 15 -- the lane that holds its m -- so the rescale is a per-lane multiply.  The
// row sum is kept as a per-lane partial (the lane's four keys of every tile; a is the same in the four lanes of a query) and
// reduced once at the end.  O = O^T / l at the end; the statistics are stored as the pair (final row max, 1 / sum) in the lse
// layout of attn_fwd_kernel, so every backward kernel reads them unchanged.
// Non-finite intermediates: m starts at -inf.  Every padded tile holds at least one real key (its first) and a masked key is the
// finite -10000 fill, so a tile max -- and with it every m' -- is finite; a is taken as 0 for the first tile instead of evaluating
// exp(-inf - m'), and (-inf) - (-inf) never occurs.  A pad key is -inf - m' = -inf -> probability exactly 0.  A padded query row
// and a row whose keys are all masked see equal finite logits: the uniform average, as in the held kernel.
// Register arrays: the K / V prefetch buffers are two NAMED halves, the loop is unrolled by two, every index is a constant.
#pragma once
#include "attention.h"

namespace segmm {

template <int DH>
__global__ __launch_bounds__(att_stream_fwd_threads(DH)) void attn_fwd_stream_kernel(const AttnArgs p) {
    using C = AttnCfg<DH>;
    const DropCfg drop_ = drop_live(p.drop);
    extern __shared__ uint8_t km[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wpb = blockDim.x >> 6, wq = wpb / p.hpb;
    const int l15 = lane & 15, g = lane >> 4;
    const int bh = xcd_remap(blockIdx.x, gridDim.x) * p.hpb + wave / wq, b = bh / p.H, h = bh % p.H;
    const int La_p = round16(p.La), Lb_p = round16(p.Lb), Tp = La_p + Lb_p, nta = La_p >> 4, nt = Tp >> 4;
    const int col0 = h * DH;
    stage_kmask(km, p.mka, p.mkb, b, p.La, p.Lb, La_p, Lb_p, blockDim.x);
    __syncthreads();
    const int qt = blockIdx.y * wq + wave % wq;      // this wave's query tile
    if (16 * qt >= p.Lq) return;
    const int qi = 16 * qt + l15;                    // this lane's query
    const bool q_in = qi < p.Lq;
    const size_t qrow = (size_t)b * p.Lq + min(qi, p.Lq - 1);
    const bool q_ok = q_in && p.mq[qrow] != 0;
    KeyBlocks<DH> kbk;
    kbk.init(p, b, col0, l15, g);

    float qa[C::KS], qb[C::KS];
    frag_load_ptr<DH>(qa, p.Qa + qrow * p.ldq + col0 + C::row_off(g));
    frag_load_ptr<DH>(qb, p.Qb + qrow * p.ldq + col0 + C::row_off(g));

    // K row fragments and V column fragments of tile t + 1 are in flight under tile t's MFMAs and softmax
    float kf0[C::KS], kf1[C::KS], vf0[4][C::CT], vf1[4][C::CT];
    auto fetch = [&](float (&kf)[C::KS], float (&vf)[4][C::CT], int t) {
        if (t < nta) {
            frag_load<DH>(kf, kbk.ka, kbk.row_a, (uint32_t)(16 * t) * kbk.pitch_a);
#pragma unroll
            for (int s = 0; s < 4; ++s) col_load<DH>(vf[s], kbk.va, kbk.col_a, (uint32_t)(16 * t + s) * kbk.pitch_a, l15);
        } else {
            frag_load<DH>(kf, kbk.kb, kbk.row_b, (uint32_t)(16 * (t - nta)) * kbk.pitch_b);
#pragma unroll
            for (int s = 0; s < 4; ++s) col_load<DH>(vf[s], kbk.vb, kbk.col_b, (uint32_t)(16 * (t - nta) + s) * kbk.pitch_b, l15);
        }
    };
    float m = -INFINITY, l = 0.f;      // running row max (the same in the four lanes of a query); this lane's part of the row sum
    f32x4 o[C::CT];                    // O^T[c][query], unnormalised
#pragma unroll
    for (int ct = 0; ct < C::CT; ++ct) o[ct] = f32x4{0.f, 0.f, 0.f, 0.f};

    auto step = [&](const float (&kf)[C::KS], const float (&vf)[4][C::CT], int t) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};      // acc[r] = sum_c K[16t + 4g + r][c] Q[query][c]
        if (t < nta) {       // wave-uniform: no per-element select of the query projection
#pragma unroll
            for (int c = 0; c < C::KS; ++c) acc = MFMA16(kf[c], qa[c], acc);
        } else {
#pragma unroll
            for (int c = 0; c < C::KS; ++c) acc = MFMA16(kf[c], qb[c], acc);
        }
        const uint32_t kb = *(const uint32_t*)(km + 16 * t + 4 * g);
        f32x4 mult = {1.f, 1.f, 1.f, 1.f};
        if (drop_.p > 0.f)
            mult = drop_apply4(drop_, (((uint64_t)bh * p.Lq + (q_in ? qi : 0)) * Tp + 16 * t + 4 * g) >> 2,
                               f32x4{1.f, 1.f, 1.f, 1.f});
        float tm = -INFINITY;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint32_t k = (kb >> (8 * r)) & 0xff;
            float v = logit_xform(acc[r], q_ok && k == 1, mult[r], p.scale);
            if (k == 2) v = -INFINITY;
            acc[r] = v;
            tm = fmaxf(tm, v);
        }
        tm = fmaxf(tm, __shfl_xor(tm, 16, 64));
        tm = fmaxf(tm, __shfl_xor(tm, 32, 64));      // finite: the tile's first key is a real one
        const float mn = fmaxf(m, tm);
        const float a = (t == 0) ? 0.f : fast_exp(m - mn);
        m = mn;
        float ts = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float e = fast_exp(acc[r] - mn);
            acc[r] = e;
            ts += e;
        }
        l = l * a + ts;
#pragma unroll
        for (int ct = 0; ct < C::CT; ++ct) o[ct] *= a;
        // O^T[c][query] += sum_key V[key][c] E^T[key][query]; step s contracts keys 16t + 4g + s
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int ct = 0; ct < C::CT; ++ct) o[ct] = MFMA16(vf[s][ct], acc[s], o[ct]);
    };
    fetch(kf0, vf0, 0);
    for (int t = 0; t < nt; t += 2) {
        if (t + 1 < nt) fetch(kf1, vf1, t + 1);
        step(kf0, vf0, t);
        if (t + 1 < nt) {
            if (t + 2 < nt) fetch(kf0, vf0, t + 2);
            step(kf1, vf1, t + 1);
        }
    }
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    const float inv = 1.0f / l;
    if (g == 0 && q_in) {
        p.lse[(size_t)bh * p.Lq + qi] = m;
        p.lse[(size_t)p.B * p.H * p.Lq + (size_t)bh * p.Lq + qi] = inv;
    }
#pragma unroll
    for (int ct = 0; ct < C::CT; ++ct) o[ct] *= inv;
    float am = 0.f;
    const float ps = plane_scale(p.po_o);
    if (q_in) {
        if (ps > 0.f) am = col_store_p<DH>(p.O + qrow * p.ldo + col0, p.po_o.p, p.po_o.ld2, (long long)qrow, col0, ps, o, g, am);
        else am = col_store<DH>(p.O + qrow * p.ldo + col0, o, g, am);
    }
    plane_finish(p.po_o, p.amax_o, am, (blockIdx.x * gridDim.y + blockIdx.y) * wpb + wave, ps,
                 blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0);
}

// ------------------------------------------------------------------------------------------ backward: D, streamed
// D[query] = sum_c dO[query][c] O[query][c] from the row fragments of a query tile, in ONE stated order (explicit fused
// multiply-adds over the lane's fragment, then the four lanes of the query), shared by the dQ kernel below (phase 0: it stores D
// for the dK/dV kernel) and by attn_D_stream_kernel (phase 1): the split backward (phases 1 + 2 + 3, dQ and dK/dV on two streams)
// then gives the bits of phase 0.  (attn_D_kernel sums the products in another order, so at <= 192 keys the two differ in the
// last bits of dK; those kernels stay as they are.)
template <int DH>
__device__ __forceinline__ float attn_row_D(const float (&dof)[DH / 4], const float (&of)[DH / 4]) {
    float D = 0.f;
#pragma unroll
    for (int c = 0; c < DH / 4; ++c) D = __builtin_fmaf(dof[c], of[c], D);
    D += __shfl_xor(D, 16, 64);
    D += __shfl_xor(D, 32, 64);
    return D;
}

// one wave per 16-query tile of a (b, h), four tiles per workgroup
template <int DH>
__global__ __launch_bounds__(256) void attn_D_stream_kernel(const AttnArgs p) {
    using C = AttnCfg<DH>;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
    const int nqt = (p.Lq + 15) >> 4;
    const long long tile = (long long)blockIdx.x * 4 + wave;
    if (tile >= (long long)p.B * p.H * nqt) return;
    const int bh = (int)(tile / nqt), qt = (int)(tile % nqt), b = bh / p.H, h = bh % p.H;
    const int qi = 16 * qt + l15;
    const size_t qrow = (size_t)b * p.Lq + min(qi, p.Lq - 1);
    const size_t ro = h * DH + C::row_off(g);
    float dof[C::KS], of[C::KS];
    frag_load_ptr<DH>(dof, p.dO + qrow * p.lddo + ro);
    frag_load_ptr<DH>(of, p.O + qrow * p.ldo + ro);
    const float D = attn_row_D<DH>(dof, of);
    if (g == 0 && qi < p.Lq) p.Dvec[(size_t)bh * p.Lq + qi] = D;
}

// ------------------------------------------------------------------------------------------ backward: dQ (+ D), streamed
// attn_bwd_dq_kernel with the key tiles in a run-time loop: the same body, the same accumulation order over the tiles.  A
// kernel of its own rather than an NT = 0 instance so that the unrolled instances compile from untouched source.  The K / V row-fragment double buffer is two named
// halves, the loop is unrolled by two.
template <int DH>
__global__ __launch_bounds__(att_bwd_threads(DH)) void attn_bwd_dq_stream_kernel(const AttnArgs p) {
    using C = AttnCfg<DH>;
    const DropCfg drop_ = drop_live(p.drop);
    extern __shared__ uint8_t km[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wpb = blockDim.x >> 6, wq = wpb / p.hpb;
    const int l15 = lane & 15, g = lane >> 4;
    const int bh = xcd_remap(blockIdx.x, gridDim.x) * p.hpb + wave / wq, b = bh / p.H, h = bh % p.H;
    const int La_p = round16(p.La), Lb_p = round16(p.Lb), Tp = La_p + Lb_p, nta = La_p >> 4, nt = Tp >> 4;
    const int col0 = h * DH;
    stage_kmask(km, p.mka, p.mkb, b, p.La, p.Lb, La_p, Lb_p, blockDim.x);
    __syncthreads();
    const int qt = blockIdx.y * wq + wave % wq;
    if (16 * qt >= p.Lq) return;
    const int qi = 16 * qt + l15;
    const bool q_in = qi < p.Lq;
    const size_t qrow = (size_t)b * p.Lq + min(qi, p.Lq - 1);
    const bool q_ok = q_in && p.mq[qrow] != 0;
    const float row_mx = q_in ? p.lse[(size_t)bh * p.Lq + qi] : 0.f;
    const float row_inv = q_in ? p.lse[(size_t)p.B * p.H * p.Lq + (size_t)bh * p.Lq + qi] : 0.f;
    KeyBlocks<DH> kbk;
    kbk.init(p, b, col0, l15, g);

    float qa[C::KS], qb[C::KS], dof[C::KS];
    float Dq;
    {
        const size_t ro = col0 + C::row_off(g);
        float of[C::KS];
        frag_load_ptr<DH>(qa, p.Qa + qrow * p.ldq + ro);
        frag_load_ptr<DH>(qb, p.Qb + qrow * p.ldq + ro);
        frag_load_ptr<DH>(dof, p.dO + qrow * p.lddo + ro);
        frag_load_ptr<DH>(of, p.O + qrow * p.ldo + ro);
        Dq = attn_row_D<DH>(dof, of);
        if (p.write_D && g == 0 && q_in) p.Dvec[(size_t)bh * p.Lq + qi] = Dq;
    }
    const float fac = drop_.scale * p.scale;        // d(logit)/d(raw) of a live, kept element

    float kf0[C::KS], kf1[C::KS], vr0[C::KS], vr1[C::KS], kc[4][C::CT];
    auto fetch_rows = [&](float (&kf)[C::KS], float (&vr)[C::KS], int t) {
        if (t < nta) {
            const uint32_t so = (uint32_t)(16 * t) * kbk.pitch_a;
            frag_load<DH>(kf, kbk.ka, kbk.row_a, so);
            frag_load<DH>(vr, kbk.va, kbk.row_a, so);
        } else {
            const uint32_t so = (uint32_t)(16 * (t - nta)) * kbk.pitch_b;
            frag_load<DH>(kf, kbk.kb, kbk.row_b, so);
            frag_load<DH>(vr, kbk.vb, kbk.row_b, so);
        }
    };
    auto fetch_cols = [&](int t) {
        if (t < nta) {
#pragma unroll
            for (int s = 0; s < 4; ++s) col_load<DH>(kc[s], kbk.ka, kbk.col_a, (uint32_t)(16 * t + s) * kbk.pitch_a, l15);
        } else {
#pragma unroll
            for (int s = 0; s < 4; ++s) col_load<DH>(kc[s], kbk.kb, kbk.col_b, (uint32_t)(16 * (t - nta) + s) * kbk.pitch_b, l15);
        }
    };
    f32x4 da[C::CT], db[C::CT];
#pragma unroll
    for (int ct = 0; ct < C::CT; ++ct) { da[ct] = f32x4{0.f, 0.f, 0.f, 0.f}; db[ct] = f32x4{0.f, 0.f, 0.f, 0.f}; }

    auto step = [&](const float (&kf)[C::KS], const float (&vr)[C::KS], int t) {
        fetch_cols(t);
        const bool isa = t < nta;
        f32x4 P = {0.f, 0.f, 0.f, 0.f}, dS = {0.f, 0.f, 0.f, 0.f};
        if (isa) {
#pragma unroll
            for (int c = 0; c < C::KS; ++c) {
                P = MFMA16(kf[c], qa[c], P);
                dS = MFMA16(vr[c], dof[c], dS);
            }
        } else {
#pragma unroll
            for (int c = 0; c < C::KS; ++c) {
                P = MFMA16(kf[c], qb[c], P);
                dS = MFMA16(vr[c], dof[c], dS);
            }
        }
        const uint32_t kb = *(const uint32_t*)(km + 16 * t + 4 * g);
        f32x4 mult = {1.f, 1.f, 1.f, 1.f};
        if (drop_.p > 0.f)
            mult = drop_apply4(drop_, (((uint64_t)bh * p.Lq + (q_in ? qi : 0)) * Tp + 16 * t + 4 * g) >> 2,
                               f32x4{1.f, 1.f, 1.f, 1.f});
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint32_t k = (kb >> (8 * r)) & 0xff;
            const bool valid = q_ok && k == 1;
            const float v = logit_xform(P[r], valid, mult[r], p.scale);
            const float pr = (k == 2) ? 0.f : fast_exp(v - row_mx) * row_inv;
            dS[r] = (valid && mult[r] != 0.f) ? pr * (dS[r] - Dq) * fac : 0.f;
        }
        // dQ^T[c][query] += sum_key K[key][c] dS^T[key][query]; block a keys -> dQa, block b keys -> dQb
        if (isa) {
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int ct = 0; ct < C::CT; ++ct) da[ct] = MFMA16(kc[s][ct], dS[s], da[ct]);
        } else {
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int ct = 0; ct < C::CT; ++ct) db[ct] = MFMA16(kc[s][ct], dS[s], db[ct]);
        }
    };
    fetch_rows(kf0, vr0, 0);
    for (int t = 0; t < nt; t += 2) {
        if (t + 1 < nt) fetch_rows(kf1, vr1, t + 1);
        step(kf0, vr0, t);
        if (t + 1 < nt) {
            if (t + 2 < nt) fetch_rows(kf0, vr0, t + 2);
            step(kf1, vr1, t + 1);
        }
    }
    float am = 0.f;
    if (q_in) {
        if (p.dQa) am = col_store<DH>(p.dQa + qrow * p.lddq + col0, da, g, am);      // null: empty key block (ablations)
        if (p.dQb) am = col_store<DH>(p.dQb + qrow * p.lddq + col0, db, g, am);
    }
    if (p.amax_q) amax_commit(p.amax_q, am, (blockIdx.x * gridDim.y + blockIdx.y) * wpb + wave);
}

}  // namespace segmm
