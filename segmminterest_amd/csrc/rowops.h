// HBM-bound row kernels of the path: L1 normalisation, LayerNorm forward/backward, column sums,
// the Linear(d,1) interest head, id-embedding gather, fused multi-tensor AdamW.  All are one-wave-
// per-row (wave64 shuffle reductions, float4 coalesced traffic, no LDS for the row reduce).
#pragma once
#include "common.h"

namespace segmm {
constexpr int ROW_MAXV = 8;      // float4 per lane kept in registers => d <= 2048

// ---------------------------------------------------------------- a1: x / (sum|x| + 1e-6)
// trainer-side normalisation, main_for_seq_leave_earlystop_SegMM.py:272-273.  If y == null only the
// reciprocal scale is written (consumed by the GEMM row_scale epilogue: the fused a1+a2 path).
__global__ __launch_bounds__(256) void l1norm_kernel(const float* __restrict__ x, float* y, float* inv_scale, long long rows, int D,
                                                     float* amax, PlaneOut po) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* xr = x + row * D;
    float s = 0.f;
    for (int c = lane * 4; c < D; c += 256) {
        const f32x4 v = *(const f32x4*)(xr + c);
        s += fabsf(v.x) + fabsf(v.y) + fabsf(v.z) + fabsf(v.w);
    }
    s = wave_sum(s);
    const float inv = 1.0f / (s + 1e-6f);
    if (inv_scale && lane == 0) inv_scale[row] = inv;
    const float ps = plane_scale(po);
    if (y || ps > 0.f) {          // y == null with a plane output: the normalised rows are written as planes ONLY
        const float den = s + 1e-6f;
        float am = 0.f;
        for (int c = lane * 4; c < D; c += 256) {
            f32x4 v = *(const f32x4*)(xr + c);
            v.x /= den; v.y /= den; v.z /= den; v.w /= den;
            if (y) *(f32x4*)(y + row * D + c) = v;
            if (ps > 0.f) plane_store4_pair(po.p, po.ld2, row, c, v, ps);
            am = absmax4(am, v);
        }
        plane_finish(po, amax, am, (unsigned)row, ps, row == 0 && lane == 0);      // partial maxima of |y| for the GEMM that reads y
    }
}

// The same with the row held in registers between the two passes (V float4 per lane, D <= 1024 V): one read of x instead of two --
// the second pass of the loop form came back from HBM for ~45 % of its bytes (PMC: 160 MB read per launch for 110 MB of rows).
// Element for element the arithmetic of l1norm_kernel (same summation order per lane, same wave reduction, true division).
template <int V>
__global__ __launch_bounds__(256) void l1norm_reg_kernel(const float* __restrict__ x, float* y, float* inv_scale, long long rows, int D,
                                                         float* amax, PlaneOut po) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* xr = x + row * D;
    f32x4 v[V];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const int c = lane * 4 + i * 256;
        v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (c < D) { v[i] = ld_row4b(xr + c); s += fabsf(v[i].x) + fabsf(v[i].y) + fabsf(v[i].z) + fabsf(v[i].w); }
    }
    s = wave_sum(s);
    const float inv = 1.0f / (s + 1e-6f);
    if (inv_scale && lane == 0) inv_scale[row] = inv;
    const float ps = plane_scale(po);
    if (y || ps > 0.f) {
        const float den = s + 1e-6f;
        float am = 0.f;
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const int c = lane * 4 + i * 256;
            if (c < D) {
                f32x4 o = v[i];
                o.x /= den; o.y /= den; o.z /= den; o.w /= den;
                if (y) st_row4b(y + row * D + c, o);
                if (ps > 0.f) plane_store4_pair(po.p, po.ld2, row, c, o, ps);
                am = absmax4(am, o);
            }
        }
        plane_finish(po, amax, am, (unsigned)row, ps, row == 0 && lane == 0);
    }
}

// The same for a 16-bit x (ELEM: IEEE half or bfloat16, common.h widen4): every element is widened to fp32 exactly, then the
// arithmetic above -- the same four columns per lane, summation order, wave reduction, true division, plane calls -- so the result
// is segmm_l1norm's on the widened tensor, bit for bit.  V > 0: the row's RAW words stay in registers between the two passes (2 VGPRs
// per 4 elements, D <= 256 V <= 2048) and x is read once; V == 0: l1norm_kernel's two-pass loop, for wider rows.
template <int ELEM, int V>
__global__ __launch_bounds__(256) void l1norm_h_kernel(const uint16_t* __restrict__ x, float* y, float* inv_scale, long long rows, int D,
                                                       float* amax, PlaneOut po) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const uint16_t* xr = x + row * D;
    uint32_t ra[V > 0 ? V : 1], rb[V > 0 ? V : 1];
    float s = 0.f;
    if constexpr (V > 0) {
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const int c = lane * 4 + i * 256;
            ra[i] = rb[i] = 0u;
            if (c < D) {
                const u32x2 w = ld_row4h(xr + c);
                ra[i] = w.x; rb[i] = w.y;
                const f32x4 v = widen4<ELEM>(ra[i], rb[i]);
                s += fabsf(v.x) + fabsf(v.y) + fabsf(v.z) + fabsf(v.w);
            }
        }
    } else {
        for (int c = lane * 4; c < D; c += 256) {
            const f32x4 v = widen4<ELEM>(ld_row4h(xr + c));
            s += fabsf(v.x) + fabsf(v.y) + fabsf(v.z) + fabsf(v.w);
        }
    }
    s = wave_sum(s);
    const float inv = 1.0f / (s + 1e-6f);
    if (inv_scale && lane == 0) inv_scale[row] = inv;
    const float ps = plane_scale(po);
    if (y || ps > 0.f) {
        const float den = s + 1e-6f;
        float am = 0.f;
        if constexpr (V > 0) {
#pragma unroll
            for (int i = 0; i < V; ++i) {
                const int c = lane * 4 + i * 256;
                if (c < D) {
                    f32x4 o = widen4<ELEM>(ra[i], rb[i]);
                    o.x /= den; o.y /= den; o.z /= den; o.w /= den;
                    if (y) st_row4b(y + row * D + c, o);
                    if (ps > 0.f) plane_store4_pair(po.p, po.ld2, row, c, o, ps);
                    am = absmax4(am, o);
                }
            }
        } else {
            for (int c = lane * 4; c < D; c += 256) {
                f32x4 o = widen4<ELEM>(ld_row4h(xr + c));
                o.x /= den; o.y /= den; o.z /= den; o.w /= den;
                if (y) *(f32x4*)(y + row * D + c) = o;
                if (ps > 0.f) plane_store4_pair(po.p, po.ld2, row, c, o, ps);
                am = absmax4(am, o);
            }
        }
        plane_finish(po, amax, am, (unsigned)row, ps, row == 0 && lane == 0);
    }
}

// The same for an 8-bit x (ELEM: OCP e4m3fn, e5m2 or int8, common.h widen4 of one dword): widened exactly, then the arithmetic
// above, so the result is segmm_l1norm's on the widened tensor, bit for bit.  V > 0: the row's raw dwords stay in registers between
// the two passes (1 VGPR per 4 elements, D <= 256 V <= 2048) and x is read once; V == 0: the two-pass loop, for wider rows.
template <int ELEM, int V>
__global__ __launch_bounds__(256) void l1norm_b_kernel(const uint8_t* __restrict__ x, float* y, float* inv_scale, long long rows, int D,
                                                       float* amax, PlaneOut po) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const uint8_t* xr = x + row * D;
    uint32_t rw[V > 0 ? V : 1];
    float s = 0.f;
    if constexpr (V > 0) {
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const int c = lane * 4 + i * 256;
            rw[i] = 0u;
            if (c < D) {
                rw[i] = ld_row4q(xr + c);
                const f32x4 v = widen4<ELEM>(rw[i]);
                s += fabsf(v.x) + fabsf(v.y) + fabsf(v.z) + fabsf(v.w);
            }
        }
    } else {
        for (int c = lane * 4; c < D; c += 256) {
            const f32x4 v = widen4<ELEM>(ld_row4q(xr + c));
            s += fabsf(v.x) + fabsf(v.y) + fabsf(v.z) + fabsf(v.w);
        }
    }
    s = wave_sum(s);
    const float inv = 1.0f / (s + 1e-6f);
    if (inv_scale && lane == 0) inv_scale[row] = inv;
    const float ps = plane_scale(po);
    if (y || ps > 0.f) {
        const float den = s + 1e-6f;
        float am = 0.f;
        if constexpr (V > 0) {
#pragma unroll
            for (int i = 0; i < V; ++i) {
                const int c = lane * 4 + i * 256;
                if (c < D) {
                    f32x4 o = widen4<ELEM>(rw[i]);
                    o.x /= den; o.y /= den; o.z /= den; o.w /= den;
                    if (y) st_row4b(y + row * D + c, o);
                    if (ps > 0.f) plane_store4_pair(po.p, po.ld2, row, c, o, ps);
                    am = absmax4(am, o);
                }
            }
        } else {
            for (int c = lane * 4; c < D; c += 256) {
                f32x4 o = widen4<ELEM>(ld_row4q(xr + c));
                o.x /= den; o.y /= den; o.z /= den; o.w /= den;
                if (y) *(f32x4*)(y + row * D + c) = o;
                if (ps > 0.f) plane_store4_pair(po.p, po.ld2, row, c, o, ps);
                am = absmax4(am, o);
            }
        }
        plane_finish(po, amax, am, (unsigned)row, ps, row == 0 && lane == 0);
    }
}

// ---------------------------------------------------------------- float32 rows -> 8-bit codes (the loader of an 8-bit feature table)
// One wave per row.  a = max|x_j|, taken on the bit patterns (an unsigned compare orders |x| and puts NaN above inf, so a non-finite
// element is seen whatever its place); a < 2^-100 or non-finite: all-zero codes, scale 0.  Otherwise the row is multiplied by
//   e4m3: s = 2^(8-e), e5m2: s = 2^(15-e)  (a = m 2^e, 0.5 <= m < 1: a power of two, the product is exact, |x s| < 256 / 32768)
//   int8: r = 127 / a  (a true division; |rint(x r)| <= 127)
// and each product becomes its code by quant8_code (common.h): round to nearest even.  Four codes are one dword store (q rows are
// 4-byte aligned: D % 4 == 0).  The scale is not kept with the codes: the rows are L1-normalised as they are read, which cancels it.
// The rule is stated in numpy in tests/feature8_ref.py; this kernel gives its bytes.
template <int ELEM>
__global__ __launch_bounds__(256) void quantize_rows_kernel(const float* __restrict__ x, long long rows, int D, uint8_t* __restrict__ q,
                                                            float* __restrict__ scale_out) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* xr = x + row * D;
    uint32_t a = 0u;
    for (int c = lane * 4; c < D; c += 256) {
        const f32x4 v = *(const f32x4*)(xr + c);
        const uint32_t m0 = max(__float_as_uint(v.x) & 0x7fffffffu, __float_as_uint(v.y) & 0x7fffffffu);
        const uint32_t m1 = max(__float_as_uint(v.z) & 0x7fffffffu, __float_as_uint(v.w) & 0x7fffffffu);
        a = max(a, max(m0, m1));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a = max(a, (uint32_t)__shfl_xor((int)a, o, 64));
    const bool live = a >= ((127u - 100u) << 23) && a < 0x7f800000u;
    float s = 0.f;
    if (live) {
        if constexpr (ELEM == ELEM_I8) s = 127.0f / __uint_as_float(a);
        else s = __uint_as_float((uint32_t)((ELEM == ELEM_E4M3 ? 261 : 268) - (int)(a >> 23)) << 23);      // e = (a >> 23) - 126
    }
    if (scale_out && lane == 0) scale_out[row] = s;
    uint32_t* qr = (uint32_t*)(q + row * D);
    for (int c = lane * 4; c < D; c += 256) {
        uint32_t w = 0u;
        if (live) {
            const f32x4 v = *(const f32x4*)(xr + c);
            w = quant8_code<ELEM>(v.x * s) | (quant8_code<ELEM>(v.y * s) << 8) | (quant8_code<ELEM>(v.z * s) << 16) |
                (quant8_code<ELEM>(v.w * s) << 24);
        }
        qr[c >> 2] = w;
    }
}

// ---------------------------------------------------------------- LayerNorm forward (eps 1e-12, encoder.py:39-40)
// y = LN(x) * gamma + beta, optional dropout on y (embedding, encoder.py:461,471); saves mean / rstd.
// V = float4 per lane (d <= 256 V): the row lives in 4V registers, so the register count -- and with it the
// number of rows in flight per CU, which is what hides the HBM latency of this streaming kernel -- follows d.
template <int V>
__global__ __launch_bounds__(256) void layernorm_fwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                     const float* __restrict__ beta, float* __restrict__ y, float* mean_out,
                                     float* rstd_out, long long rows, int d, float eps, DropCfg drop, float* amax, PlaneOut po,
                                     const float* __restrict__ dot_w = nullptr, const float* __restrict__ dot_b = nullptr,
                                     float* __restrict__ dot_out = nullptr) {
    // dot_w != null: also dot_out[row] = y[row, :] . dot_w (+ dot_b[0]) -- the Linear(d, 1) interest head on the backbone's last
    // LayerNorm (decoder_leave_focal.py:451,596), taken from the registers that hold y instead of by a pass over y (rowdot_kernel's
    // per-lane order and wave reduction)
    drop = drop_live(drop);
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* xr = x + row * d;
    float ps = plane_scale(po);
    f32x4 v[V];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const int c = lane * 4 + i * 256;
        v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (c < d) { v[i] = ld_row4(xr + c); s += v[i].x + v[i].y + v[i].z + v[i].w; }
    }
    if (y == nullptr) {
        // PLANES ONLY (no fp32 copy a consumer could fall back on): the planes are written with the scale of the output's BOUND,
        // |y| <= (max|gamma| sqrt(d - 1) + max|beta|) / (1 - p) for any input row -- it cannot overflow whatever the batch, needs no
        // history and no repair pass, and sits ~sqrt(d) / 4 above the typical maximum (3 of the 9 binades of the consumers' window)
        float gm = 0.f, bm = 0.f;
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const int c = lane * 4 + i * 256;
            if (c < d) { gm = absmax4(gm, *(const f32x4*)(gamma + c)); bm = absmax4(bm, *(const f32x4*)(beta + c)); }
        }
        ps = f16_scale_of((wave_max(gm) * sqrtf((float)d) + wave_max(bm)) * drop.scale);
    }
    const float mean = wave_sum(s) / d;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const int c = lane * 4 + i * 256;
        if (c < d) {
            const f32x4 t = v[i] - mean;
            q += t.x * t.x + t.y * t.y + t.z * t.z + t.w * t.w;
        }
    }
    const float rstd = rsqrtf(wave_sum(q) / d + eps);
    if (lane == 0) { mean_out[row] = mean; rstd_out[row] = rstd; }
    float am = 0.f, dsum = 0.f;
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const int c = lane * 4 + i * 256;
        if (c < d) {
            f32x4 o = (v[i] - mean) * rstd * *(const f32x4*)(gamma + c) + *(const f32x4*)(beta + c);
            if (drop.p > 0.f) o = drop_apply4(drop, ((uint64_t)row * d + c) >> 2, o);
            if (y) st_row4(y + row * d + c, o);
            if (ps > 0.f) plane_store4_pair(po.p, po.ld2, row, c, o, ps);
            am = absmax4(am, o);
            if (dot_w) {
                const f32x4 b = *(const f32x4*)(dot_w + c);
                dsum += o.x * b.x + o.y * b.y + o.z * b.z + o.w * b.w;
            }
        }
    }
    if (dot_w) {
        dsum = wave_sum(dsum);
        if (lane == 0) dot_out[row] = dot_b ? dsum + dot_b[0] : dsum;
    }
    plane_finish(po, amax, am, (unsigned)row, ps, row == 0 && lane == 0);
}

// The same as ONE ROUND of resident workgroups whose waves WALK rows (wave w of W takes rows w, w + W, ...: the launch form of
// layernorm_bwd_kernel).  The loads of a wave's NEXT row are issued before the two reductions of the current one (one more row of
// registers), so a wave always has a row in flight while it reduces and stores; gamma, beta, the head weight (DOT) and the planes-only
// scale are the same for every row and are fetched once per wave.  Per row the arithmetic is layernorm_fwd_kernel's, expression for
// expression: the lane-to-column map, the summation orders, o, the dropout index, the plane stores, and the maxima in the slots
// that one plane_finish per row with the row as key leaves them in (see one_slot) -- every output is bit for bit that kernel's.
template <int V, bool DOT>
__global__ __launch_bounds__(256) void layernorm_fwd_walk_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                     const float* __restrict__ beta, float* __restrict__ y, float* mean_out,
                                     float* rstd_out, long long rows, int d, float eps, DropCfg drop, float* amax, PlaneOut po,
                                     const float* __restrict__ dot_w, const float* __restrict__ dot_b, float* __restrict__ dot_out) {
    drop = drop_live(drop);
    const int lane = threadIdx.x & 63;
    const long long stride = (long long)gridDim.x * (blockDim.x >> 6);
    long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= rows) return;
    f32x4 nx[V];                      // the next row of this wave, in flight
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const int c = lane * 4 + i * 256;
        nx[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (c < d) nx[i] = ld_row4(x + row * d + c);
    }
    f32x4 gmv[V], btv[V], dw[DOT ? V : 1];
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const int c = lane * 4 + i * 256;
        gmv[i] = f32x4{0.f, 0.f, 0.f, 0.f}; btv[i] = gmv[i];
        if (DOT) dw[i] = gmv[i];
        if (c < d) {
            gmv[i] = *(const f32x4*)(gamma + c); btv[i] = *(const f32x4*)(beta + c);
            if (DOT) dw[i] = *(const f32x4*)(dot_w + c);
        }
    }
    float ps = plane_scale(po);
    if (y == nullptr) {               // planes only: the scale of the output's bound (layernorm_fwd_kernel), the same for every row
        float gm = 0.f, bm = 0.f;
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const int c = lane * 4 + i * 256;
            if (c < d) { gm = absmax4(gm, gmv[i]); bm = absmax4(bm, btv[i]); }
        }
        ps = f16_scale_of((wave_max(gm) * sqrtf((float)d) + wave_max(bm)) * drop.scale);
    }
    float db = 0.f;
    if (DOT && dot_b) db = dot_b[0];
    // The maxima: a row's maximum goes to slot row % AMAX_SLOTS.  Where the wave stride is a multiple of AMAX_SLOTS (every default
    // grid is a multiple of 64 workgroups) all rows of a wave share ONE slot, and the wave keeps a running maximum and commits it once,
    // keyed by its first row: max is exact and order-free, the overflow flag is monotone in it, and the wave of row 0 still writes the
    // scale -- the header and the slots end up with the bits of one commit per row, at one atomic per wave instead of one per row.
    const bool one_slot = (stride & (AMAX_SLOTS - 1)) == 0 || row + stride >= rows;          // (wave-uniform)
    const long long row0 = row;
    float am = 0.f;
    for (; row < rows; row += stride) {
        f32x4 v[V];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const int c = lane * 4 + i * 256;
            v[i] = nx[i];
            if (c < d) s += v[i].x + v[i].y + v[i].z + v[i].w;
        }
        if (row + stride < rows) {          // (wave-uniform) the next row's loads go out before this row's reductions
#pragma unroll
            for (int i = 0; i < V; ++i) {
                const int c = lane * 4 + i * 256;
                if (c < d) nx[i] = ld_row4(x + (row + stride) * d + c);
            }
        }
        const float mean = wave_sum(s) / d;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const int c = lane * 4 + i * 256;
            if (c < d) {
                const f32x4 t = v[i] - mean;
                q += t.x * t.x + t.y * t.y + t.z * t.z + t.w * t.w;
            }
        }
        const float rstd = rsqrtf(wave_sum(q) / d + eps);
        if (lane == 0) { mean_out[row] = mean; rstd_out[row] = rstd; }
        float dsum = 0.f;
        if (!one_slot) am = 0.f;
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const int c = lane * 4 + i * 256;
            if (c < d) {
                f32x4 o = (v[i] - mean) * rstd * gmv[i] + btv[i];
                if (drop.p > 0.f) o = drop_apply4(drop, ((uint64_t)row * d + c) >> 2, o);
                if (y) st_row4(y + row * d + c, o);
                if (ps > 0.f) plane_store4_pair(po.p, po.ld2, row, c, o, ps);
                am = absmax4(am, o);
                if (DOT) {
                    const f32x4 b = dw[i];
                    dsum += o.x * b.x + o.y * b.y + o.z * b.z + o.w * b.w;
                }
            }
        }
        if (DOT) {
            dsum = wave_sum(dsum);
            if (lane == 0) dot_out[row] = dot_b ? dsum + db : dsum;
        }
        if (!one_slot) plane_finish(po, amax, am, (unsigned)row, ps, row == 0 && lane == 0);
    }
    if (one_slot) plane_finish(po, amax, am, (unsigned)row0, ps, row0 == 0 && lane == 0);
}

// ---------------------------------------------------------------- LayerNorm backward
// dy_eff = dy (.) dropmask (if the forward dropped y);  dx = rstd (g dy - mean(g dy) - xhat mean(g dy xhat)).
// Outputs: dx; optionally dx_drop = dx (.) dropmask2 (the gradient that continues through the
// residual branch "x = res + dropout(z)": dz = dx_drop); per-workgroup partial dgamma / dbeta and, optionally,
// the partial COLUMN SUMS of the forwarded gradient (dx_drop, or dx without it) -- the bias gradient of the
// Linear that produced z, which would otherwise cost a second pass over that tensor.
// dx == null (with a plane output, no dx_drop): PLANES ONLY -- the gradient leaves as planes, maxima and partials, exactly the ones
// of the launch with dx, and no fp32 copy is stored (the embedding LayerNorms: their dx is read by a plane TN GEMM alone, the
// positional sums come from part_pos; 157 MB of stores at 51 200 x 768).  The consumer then has no fp32 copy to fall back on, so
// the REPAIR form of the same launch follows segmm_site_fixup (the protocol of the attention backward, attention.h ATT_REPAIR):
// hdr[2] == 0 = the planes are usable, every workgroup leaves after one scalar load; otherwise the rows are recomputed and ONLY
// the planes rewritten, with the exact scale fixup left in hdr[0] -- no dx, no partials, no maxima, no flag (the column sums of the
// first launch's partials may be running on the side stream, and every workgroup must read the same header).
template <int V, bool REPAIR = false>
__global__ __launch_bounds__(256) void layernorm_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                     const float* __restrict__ mean, const float* __restrict__ rstd,
                                     const float* __restrict__ gamma, float* __restrict__ dx,
                                     float* __restrict__ dx_drop, float* __restrict__ part_dgamma,
                                     float* __restrict__ part_dbeta, float* __restrict__ part_dsum, long long rows, int d,
                                     DropCfg drop_y, DropCfg drop_branch, float* amax, PlaneOut po, float* __restrict__ part_pos = nullptr,
                                     const float* __restrict__ dy_col = nullptr) {
    // dy_col != null: the incoming gradient is an OUTER PRODUCT dy[row, c] = dy[row] * dy_col[c] (``dy`` then holds one value per
    // row) -- the gradient the Linear(d, 1) interest head sends into the last LayerNorm (d logits[row] * w[c],
    // decoder_leave_focal.py:451,596): formed here instead of being written out by one kernel and read back by this one.
    drop_y = drop_live(drop_y); drop_branch = drop_live(drop_branch);
    __shared__ f32x4 red[4][64];
    float ps = plane_scale(po);
    if (REPAIR) {
        if (po.hdr[2] == 0.f) return;          // (block-uniform: one header word)
        ps = po.hdr[0];
    }
    float am = 0.f;          // max |dx_drop| (or |dx| when there is no dropped copy): the tensor the GEMMs consume
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    // part_pos (embedding LayerNorms): this WAVE's sum of dx over the rows it walks, one partial row per wave.  The host picks the
    // grid so that the wave stride gridDim * nw is a multiple of the sequence length L: every row of a wave then sits at the
    // same position s = (blockIdx * nw + wave) % L, and d pe[s, :] = the sum of the partial rows p = s (mod L) (segmm_colsum_pos)
    // -- 12 MB of partials instead of a second pass over the 157 MB gradient (the positional-embedding gradient, encoder.py:450-471)
    f32x4 ag[V], ab[V], as[V], gm[V], ap[V];
#pragma unroll
    for (int i = 0; i < V; ++i) {
        ag[i] = f32x4{0.f, 0.f, 0.f, 0.f}; ab[i] = ag[i]; as[i] = ag[i]; ap[i] = ag[i];
        const int c = lane * 4 + i * 256;
        gm[i] = (c < d) ? *(const f32x4*)(gamma + c) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (long long row = (long long)blockIdx.x * nw + wave; row < rows; row += (long long)gridDim.x * nw) {
        const float mu = mean[row], rs = rstd[row];
        f32x4 g[V], xh[V];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const int c = lane * 4 + i * 256;
            g[i] = f32x4{0.f, 0.f, 0.f, 0.f}; xh[i] = g[i];
            if (c < d) {
                f32x4 t = dy_col ? *(const f32x4*)(dy_col + c) * dy[row] : ld_row4(dy + row * d + c);
                if (drop_y.p > 0.f) t = drop_apply4(drop_y, ((uint64_t)row * d + c) >> 2, t);
                xh[i] = (ld_row4(x + row * d + c) - mu) * rs;
                if (!REPAIR) { ab[i] += t; ag[i] += t * xh[i]; }
                g[i] = t * gm[i];
                s1 += g[i].x + g[i].y + g[i].z + g[i].w;
                const f32x4 u = g[i] * xh[i];
                s2 += u.x + u.y + u.z + u.w;
            }
        }
        s1 = wave_sum(s1) / d;
        s2 = wave_sum(s2) / d;
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const int c = lane * 4 + i * 256;
            if (c < d) {
                const f32x4 o = (g[i] - s1 - xh[i] * s2) * rs;
                if (!REPAIR && dx) st_row4(dx + row * d + c, o);
                f32x4 od = o;
                if (!REPAIR && dx_drop) {
                    if (drop_branch.p > 0.f) od = drop_apply4(drop_branch, ((uint64_t)row * d + c) >> 2, o);
                    st_row4(dx_drop + row * d + c, od);
                }
                if (ps > 0.f) plane_store4_pair(po.p, po.ld2, row, c, od, ps);
                if (!REPAIR) { as[i] += od; ap[i] += o; am = absmax4(am, od); }
            }
        }
    }
    if (REPAIR) return;
    plane_finish(po, amax, am, blockIdx.x * nw + wave, ps, blockIdx.x == 0 && threadIdx.x == 0);
    if (part_pos) {
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const int c = lane * 4 + i * 256;
            if (c < d) *(f32x4*)(part_pos + ((size_t)blockIdx.x * nw + wave) * d + c) = ap[i];
        }
    }
    // cross-wave reduce of the partials, one partial row per workgroup.  One 256-column chunk at a time through a 4 KB
    // buffer: the kernel usually runs NEXT TO a GEMM that holds 120 of the CU's 160 KB of LDS, and a 12 KB buffer
    // would cap it at three workgroups per CU there.
    for (int pass = 0; pass < (part_dsum ? 3 : 2); ++pass) {
        float* out = (pass == 0 ? part_dgamma : (pass == 1 ? part_dbeta : part_dsum)) + (size_t)blockIdx.x * d;
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const int c = lane * 4 + i * 256;
            __syncthreads();
            red[wave][lane] = pass == 0 ? ag[i] : (pass == 1 ? ab[i] : as[i]);
            __syncthreads();
            if (wave == 0 && c < d) {
                f32x4 s4 = red[0][lane];
                for (int w = 1; w < nw; ++w) s4 += red[w][lane];
                *(f32x4*)(out + c) = s4;
            }
        }
    }
}

// ---------------------------------------------------------------- column sums (bias grads, head weight grad)
// One thread's walk of the column sums below: acc += p[r * pitch] for r = r, r + step, ... < r1 (w: each row times w[r] first), added in
// ROW ORDER into the one accumulator.  Only the loads are batched: COLSUM_INFLIGHT of them are issued before the dependent adds (one
// dependent load per add left a thread waiting a full memory round trip per row: 1.3 TB/s on the head's weight gradient), then a
// remainder loop.  Contraction is off: the product with w[r] is rounded before the add, whatever the unrolled body would let the
// compiler fuse -- bit for bit the plain loop "v = load; v *= w[r]; acc += v".
constexpr int COLSUM_INFLIGHT = 8;
template <bool NT>
__device__ __forceinline__ f32x4 colsum_ld(const float* p) { return NT ? ld_row4b(p) : *(const f32x4*)p; }
template <bool NT>
__device__ __forceinline__ f32x4 colsum_walk(const float* __restrict__ p, size_t pitch, const float* __restrict__ w, long long r, long long r1,
                                             long long step, f32x4 acc) {
#pragma clang fp contract(off)
    for (; r + (COLSUM_INFLIGHT - 1) * step < r1; r += COLSUM_INFLIGHT * step) {
        f32x4 v[COLSUM_INFLIGHT];
#pragma unroll
        for (int k = 0; k < COLSUM_INFLIGHT; ++k) v[k] = colsum_ld<NT>(p + (size_t)(r + k * step) * pitch);
        if (w) {
            float wk[COLSUM_INFLIGHT];
#pragma unroll
            for (int k = 0; k < COLSUM_INFLIGHT; ++k) wk[k] = w[r + k * step];
#pragma unroll
            for (int k = 0; k < COLSUM_INFLIGHT; ++k) v[k] *= wk[k];
        }
#pragma unroll
        for (int k = 0; k < COLSUM_INFLIGHT; ++k) acc += v[k];
    }
    for (; r < r1; r += step) {
        f32x4 v = colsum_ld<NT>(p + (size_t)r * pitch);
        if (w) v *= w[r];
        acc += v;
    }
    return acc;
}
// partial[chunk][n] = sum over the chunk's rows of w[m] * X[m][n]   (w optional)
__global__ __launch_bounds__(256) void colsum_partial_kernel(const float* __restrict__ X, int ld, const float* __restrict__ w, long long M,
                                      int N, float* __restrict__ partial, int rows_per_chunk) {
    __shared__ f32x4 red[4][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int n = (blockIdx.x * 64 + tx) * 4;
    const long long r0 = (long long)blockIdx.y * rows_per_chunk;
    const long long r1 = min(M, r0 + rows_per_chunk);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (n < N) acc = colsum_walk<true>(X + n, (size_t)ld, w, r0 + ty, r1, 4, acc);
    red[ty][tx] = acc;
    __syncthreads();
    if (ty == 0 && n < N) {
        const f32x4 s = red[0][tx] + red[1][tx] + red[2][tx] + red[3][tx];
        *(f32x4*)(partial + (size_t)blockIdx.y * N + n) = s;
    }
}
// out[n] (+)= sum_p partial[p][n]
__global__ __launch_bounds__(256) void colsum_final_kernel(const float* __restrict__ partial, int P, int N, float* out, int accumulate) {
    // 64 float4 columns x 4 partial-row lanes per workgroup: the P partials of a column are summed by 4
    // threads in a fixed order (deterministic), not by one thread walking P dependent loads.
    __shared__ f32x4 red[4][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int n = (blockIdx.x * 64 + tx) * 4;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (n < N) acc = colsum_walk<false>(partial + n, (size_t)N, nullptr, ty, P, 4, acc);
    red[ty][tx] = acc;
    __syncthreads();
    if (ty == 0 && n < N) {
        f32x4 s = (red[0][tx] + red[1][tx]) + (red[2][tx] + red[3][tx]);
        if (accumulate) s += *(const f32x4*)(out + n);
        *(f32x4*)(out + n) = s;
    }
}

// up to three column sums of same-shaped matrices in ONE launch pair (blockIdx.z selects the matrix): the per-workgroup
// partials that a LayerNorm backward leaves behind (d gamma, d beta, column sums of the forwarded gradient) were six tiny
// dependent launches per LayerNorm; this makes them two
struct Colsum3 { const float* X[3]; float* out[3]; };
__global__ __launch_bounds__(256) void colsum_partial3_kernel(Colsum3 a, int ld, long long M, int N, float* __restrict__ partial,
                                                              int rows_per_chunk) {
    __shared__ f32x4 red[4][64];
    const float* X = a.X[blockIdx.z];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int n = (blockIdx.x * 64 + tx) * 4;
    const long long r0 = (long long)blockIdx.y * rows_per_chunk;
    const long long r1 = min(M, r0 + rows_per_chunk);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (n < N) acc = colsum_walk<true>(X + n, (size_t)ld, nullptr, r0 + ty, r1, 4, acc);
    red[ty][tx] = acc;
    __syncthreads();
    if (ty == 0 && n < N)
        *(f32x4*)(partial + ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * N + n) = red[0][tx] + red[1][tx] + red[2][tx] + red[3][tx];
}
__global__ __launch_bounds__(256) void colsum_final3_kernel(const float* __restrict__ partial, int P, int N, Colsum3 a) {
    __shared__ f32x4 red[4][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int n = (blockIdx.x * 64 + tx) * 4;
    const float* part = partial + (size_t)blockIdx.z * P * N;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (n < N) acc = colsum_walk<false>(part + n, (size_t)N, nullptr, ty, P, 4, acc);
    red[ty][tx] = acc;
    __syncthreads();
    if (ty == 0 && n < N) *(f32x4*)(a.out[blockIdx.z] + n) = (red[0][tx] + red[1][tx]) + (red[2][tx] + red[3][tx]);
}

// out[s][n] = sum over the partial rows p = s, s + period, s + 2 period, ... of part[p][n] (a fixed order: deterministic):
// the per-position sums of a LayerNorm backward's per-wave partials (layernorm_bwd_kernel part_pos).  A workgroup takes 64
// columns of one position; 16 row lanes share the position's partial rows (a short sequence has few positions and many rows
// each: one thread per column walked 1 024 dependent loads at period 1), then one lane adds the 16 partials in lane order.
__global__ __launch_bounds__(256) void colsum_pos_kernel(const float* __restrict__ part, int P, int period, int N, float* __restrict__ out) {
    __shared__ f32x4 red[16][16];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int n = (blockIdx.x * 16 + tx) * 4, s_ = blockIdx.y;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (n < N) acc = colsum_walk<false>(part + n, (size_t)N, nullptr, s_ + (long long)period * ty, P, 16ll * period, acc);
    red[ty][tx] = acc;
    __syncthreads();
    if (ty == 0 && n < N) {
        f32x4 t = red[0][tx];
#pragma unroll
        for (int k = 1; k < 16; ++k) t += red[k][tx];
        *(f32x4*)(out + (size_t)s_ * N + n) = t;
    }
}

// ---------------------------------------------------------------- interest head: Linear(d,1)  (decoder_leave_focal.py:451,596)
// out[m] (+)= x[m,:].w (+ bias)
__global__ __launch_bounds__(256) void rowdot_kernel(const float* __restrict__ x, int ld, const float* __restrict__ w,
                              const float* __restrict__ bias, float* out, long long rows, int d, int accumulate) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= rows) return;
    float s = 0.f;
    for (int c = lane * 4; c < d; c += 256) {
        const f32x4 a = *(const f32x4*)(x + row * ld + c), b = *(const f32x4*)(w + c);
        s += a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
    }
    s = wave_sum(s);
    if (lane == 0) {
        if (bias) s += bias[0];
        out[row] = accumulate ? out[row] + s : s;
    }
}
// dx[m,:] (+)= g[m] * w
__global__ __launch_bounds__(256) void rowscale_bcast_kernel(const float* __restrict__ g, const float* __restrict__ w, float* dx, int ld,
                                      long long rows, int d, int accumulate) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float gv = g[row];
    for (int c = lane * 4; c < d; c += 256) {
        f32x4 v = *(const f32x4*)(w + c) * gv;
        float* o = dx + row * ld + c;
        if (accumulate) v += *(const f32x4*)o;
        *(f32x4*)o = v;
    }
}
// out[m] (+)= sum_n a[m,n] * b[m,n]      (bilinear fusion head, decoder_leave_focal.py:417-421)
__global__ __launch_bounds__(256) void rowdot_pair_kernel(const float* __restrict__ a, int lda, const float* __restrict__ b,
                                                          int ldb, float* out, long long rows, int d, int accumulate) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= rows) return;
    float s = 0.f;
    for (int c = lane * 4; c < d; c += 256) {
        const f32x4 x = *(const f32x4*)(a + row * lda + c), y = *(const f32x4*)(b + row * ldb + c);
        s += x.x * y.x + x.y * y.y + x.z * y.z + x.w * y.w;
    }
    s = wave_sum(s);
    if (lane == 0) out[row] = accumulate ? out[row] + s : s;
}
// out[m,:] (+)= g[m] * X[m,:]
__global__ __launch_bounds__(256) void rowscale_mat_kernel(const float* __restrict__ g, const float* __restrict__ X, int ldx,
                                                           float* out, int ldo, long long rows, int d, int accumulate) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float gv = g[row];
    for (int c = lane * 4; c < d; c += 256) {
        f32x4 v = *(const f32x4*)(X + row * ldx + c) * gv;
        float* o = out + row * ldo + c;
        if (accumulate) v += *(const f32x4*)o;
        *(f32x4*)o = v;
    }
}
// deterministic single-workgroup sum of a vector: out[0] (+)= sum v
__global__ __launch_bounds__(1024) void vecsum_kernel(const float* __restrict__ v, long long n, float* out, int accumulate) {
    __shared__ float red[16];
    float s = 0.f;
    for (long long i = threadIdx.x; i < n; i += blockDim.x) s += v[i];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += red[w];
        out[0] = accumulate ? out[0] + t : t;
    }
}

// ---------------------------------------------------------------- id-mode embedding (encoder.py:426-435,445,484-486)
// vid[b,s,:] = cat(E_item[item_id[b]], frame_w * pos[b,s] + frame_b) + pe[s]     (pre-LayerNorm; pos[b,s] = s unless given)
__global__ __launch_bounds__(256) void embed_id_vid_kernel(const long long* __restrict__ item_id, const float* __restrict__ table, int dhalf,
                                    const float* __restrict__ frame_w, const float* __restrict__ frame_b,
                                    const float* __restrict__ pe, const float* __restrict__ frame_pos,
                                    float* __restrict__ out, int B, int S, long long n_rows) {
    const int d = 2 * dhalf;
    const long long row = blockIdx.x;       // b*S + s
    const int b = (int)(row / S), s = (int)(row % S);
    const float fpos = frame_pos ? frame_pos[row] : (float)s;     // 'noPos' ablation: shuffled positions (encoder.py:428-429)
    const long long id = item_id[b];
    const bool ok = id >= 0 && id < n_rows;  // torch.nn.Embedding raises on such an id; here the row is poisoned with NaN
    const float nan = __uint_as_float(0x7fc00000u);
    for (int c = threadIdx.x * 4; c < d; c += blockDim.x * 4) {
        f32x4 v;
        if (c < dhalf) v = ok ? *(const f32x4*)(table + id * dhalf + c) : f32x4{nan, nan, nan, nan};
        else v = *(const f32x4*)(frame_w + (c - dhalf)) * fpos + *(const f32x4*)(frame_b + (c - dhalf));
        if (pe) v += *(const f32x4*)(pe + (size_t)s * d + c);          // pe == null: --use_pe 0 (encoder.py:450-458)
        *(f32x4*)(out + row * d + c) = v;
    }
}
// usr[b,0,:] = E_user[user_id[b]] + pe[0]
__global__ __launch_bounds__(256) void embed_id_usr_kernel(const long long* __restrict__ user_id, const float* __restrict__ table, int d,
                                    const float* __restrict__ pe, float* __restrict__ out, int B, long long n_rows) {
    const int b = blockIdx.x;
    const long long id = user_id[b];
    const bool ok = id >= 0 && id < n_rows;
    const float nan = __uint_as_float(0x7fc00000u);
    for (int c = threadIdx.x * 4; c < d; c += blockDim.x * 4) {
        f32x4 v = ok ? *(const f32x4*)(table + id * d + c) : f32x4{nan, nan, nan, nan};
        if (pe) v += *(const f32x4*)(pe + c);
        *(f32x4*)(out + (size_t)b * d + c) = v;
    }
}
// order[k] = index of the k-th smallest id, ties in index order (a STABLE argsort, like torch.argsort(ids, stable=True)): one
// workgroup, bitonic network over the 64-bit keys (id << 32 | index) in LDS, n <= 8192 (a data-parallel node of 8 ranks x 1024
// rows).  Replaces the five ATen launches of torch.argsort on the id-mode step path.
constexpr int ARGSORT_MAX = 8192;
__global__ __launch_bounds__(1024) void argsort_ids_kernel(const long long* __restrict__ ids, int n, int npow2, int* __restrict__ order) {
    extern __shared__ unsigned long long keys[];
    for (int i = threadIdx.x; i < npow2; i += blockDim.x) {
        // ids are row numbers of an embedding table (< 2^31); out-of-range ones sort by their low 31 bits + the sign bit, any
        // fixed order is fine for them (the scatter kernel skips them).  Padding keys are larger than every real key.
        const unsigned long long id = i < n ? ((unsigned long long)ids[i] & 0xFFFFFFFFull) ^ 0x80000000ull : 0xFFFFFFFFull;
        keys[i] = i < n ? ((id << 32) | (unsigned)i) : 0xFFFFFFFFFFFFFFFFull;
    }
    __syncthreads();
    for (int k = 2; k <= npow2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < (npow2 >> 1); t += blockDim.x) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));          // lower index of the pair (bit j clear)
                const int l = i | j;
                const bool up = (i & k) == 0;
                const unsigned long long a = keys[i], b = keys[l];
                if ((a > b) == up) { keys[i] = b; keys[l] = a; }
            }
            __syncthreads();
        }
    }
    for (int i = threadIdx.x; i < n; i += blockDim.x) order[i] = (int)(keys[i] & 0xFFFFFFFFull);
}

// ---- the same argsort for MORE than ARGSORT_MAX ids (a data-parallel node whose gathered id list outgrows one workgroup: 8 ranks x
// 2048 rows and up): the bitonic network over a key array in global memory (caller's workspace, npow2 x u64), chunks of
// ARGSORT_MAX keys sorted / merged in LDS by one workgroup each, the strides >= ARGSORT_MAX as one global compare-exchange
// launch per stride.  Directions come from the GLOBAL index, so the chunk kernels are the single-workgroup network restricted
// to a chunk.  Deterministic, no host sync: 5 launches for 16 384 ids, 8 for 32 768.
__global__ __launch_bounds__(256) void argsort_keys_init_kernel(const long long* __restrict__ ids, int n, int npow2, unsigned long long* __restrict__ keys) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= npow2) return;
    const unsigned long long id = i < n ? ((unsigned long long)ids[i] & 0xFFFFFFFFull) ^ 0x80000000ull : 0xFFFFFFFFull;
    keys[i] = i < n ? ((id << 32) | (unsigned)i) : 0xFFFFFFFFFFFFFFFFull;
}
// one chunk of ARGSORT_MAX keys per workgroup: kfirst == 2: the whole network up to k = ARGSORT_MAX (a sorted chunk, ascending or
// descending by the chunk's position); kfirst > ARGSORT_MAX: only the strides j < ARGSORT_MAX of stage k = kfirst (the tail of a merge)
__global__ __launch_bounds__(1024) void argsort_chunk_kernel(unsigned long long* __restrict__ gkeys, int kfirst) {
    extern __shared__ unsigned long long keys[];
    const int base = blockIdx.x * ARGSORT_MAX;
    for (int i = threadIdx.x; i < ARGSORT_MAX; i += blockDim.x) keys[i] = gkeys[base + i];
    __syncthreads();
    const int klast = kfirst == 2 ? ARGSORT_MAX : kfirst;
    for (int k = kfirst; k <= klast; k <<= 1) {
        for (int j = (k > ARGSORT_MAX ? ARGSORT_MAX : k) >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < (ARGSORT_MAX >> 1); t += blockDim.x) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int l = i | j;
                const bool up = ((base + i) & k) == 0;
                const unsigned long long a = keys[i], b = keys[l];
                if ((a > b) == up) { keys[i] = b; keys[l] = a; }
            }
            __syncthreads();
        }
        if (k >= ARGSORT_MAX) break;
    }
    for (int i = threadIdx.x; i < ARGSORT_MAX; i += blockDim.x) gkeys[base + i] = keys[i];
}
__global__ __launch_bounds__(256) void argsort_global_step_kernel(unsigned long long* __restrict__ keys, int npow2, int k, int j) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= (npow2 >> 1)) return;
    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
    const int l = i | j;
    const bool up = (i & k) == 0;
    const unsigned long long a = keys[i], b = keys[l];
    if ((a > b) == up) { keys[i] = b; keys[l] = a; }
}
__global__ __launch_bounds__(256) void argsort_keys_finish_kernel(const unsigned long long* __restrict__ keys, int n, int* __restrict__ order) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) order[i] = (int)(keys[i] & 0xFFFFFFFFull);
}

// Data-parallel label statistics: `gathered` = G records [v (B) | v2 (B) | norms (3)] in rank order (one all-gather).  Splits them
// into the contiguous v_all / v2_all [G * B] the loss kernel takes and sums the three normalisers over the ranks, in rank order
// (counts: exact in fp32).  One launch instead of three strided ATen kernels inside the step.
__global__ __launch_bounds__(256) void label_stats_unpack_kernel(const float* __restrict__ gathered, int G, int B, float* __restrict__ v_all,
                                                                  float* __restrict__ v2_all, float* __restrict__ norms) {
    const int n = 2 * B + 3;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < G * B; i += gridDim.x * 256) {
        const int g = i / B, b = i - g * B;
        v_all[i] = gathered[(size_t)g * n + b];
        v2_all[i] = gathered[(size_t)g * n + B + b];
    }
    if (blockIdx.x == 0 && threadIdx.x < 3) {
        float s = 0.f;
        for (int g = 0; g < G; ++g) s += gathered[(size_t)g * n + 2 * B + threadIdx.x];
        norms[threadIdx.x] = s;
    }
}

// table[ids[k]][:] = 0 for every k (ids outside the table are skipped): clears the rows the previous step scattered into a
// dense embedding-table gradient instead of re-filling the whole table
__global__ __launch_bounds__(64) void zero_rows_kernel(float* __restrict__ table, int width, const long long* __restrict__ ids, long long n_rows) {
    const long long id = ids[blockIdx.x];
    if (id < 0 || id >= n_rows) return;
    for (int c = threadIdx.x * 4; c < width; c += 256) *(f32x4*)(table + id * width + c) = f32x4{0.f, 0.f, 0.f, 0.f};
}

// backward of the gathers: dense table gradients (torch.nn.Embedding semantics), deterministic and
// sync-free: `order` = batch rows sorted by id (host-side torch.sort, no size-dependent output).
// Workgroup k owns sorted position k; it is a segment head iff its id differs from position k-1,
// and then sums every following row with the same id, in sorted order.
__global__ __launch_bounds__(256) void embed_id_bwd_kernel(const float* __restrict__ dpre, int tok_per_row, int ld,
                                    int col0, int width, const int* __restrict__ order,
                                    const long long* __restrict__ ids, float* __restrict__ dtable, int B, long long n_rows) {
    const int k0 = blockIdx.x;
    const long long id = ids[order[k0]];
    if (id < 0 || id >= n_rows) return;      // out-of-range id: its forward row was poisoned, nothing to scatter
    if (k0 > 0 && ids[order[k0 - 1]] == id) return;
    for (int c = threadIdx.x * 4; c < width; c += blockDim.x * 4) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int k = k0; k < B && ids[order[k]] == id; ++k) {
            const long long tok0 = (long long)order[k] * tok_per_row;
            for (int t = 0; t < tok_per_row; ++t) acc += *(const f32x4*)(dpre + (tok0 + t) * ld + col0 + c);
        }
        float* o = dtable + id * width + c;
        *(f32x4*)o = *(const f32x4*)o + acc;
    }
}
// frame-position Linear(1, d/2) grads and positional-embedding grads need column sums over b with s fixed:
// dpe[s, :] = sum_b dpre[b*S+s, :]   (one workgroup per s; deterministic)
__global__ __launch_bounds__(256) void pe_grad_kernel(const float* __restrict__ dpre, int ld, int B, int S, int d, float* __restrict__ dpe,
                               int accumulate) {
    const int s = blockIdx.x;
    for (int c = threadIdx.x * 4; c < d; c += blockDim.x * 4) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int b = 0; b < B; ++b) acc += *(const f32x4*)(dpre + ((size_t)b * S + s) * ld + c);
        float* o = dpe + (size_t)s * d + c;
        if (accumulate) acc += *(const f32x4*)o;
        *(f32x4*)o = acc;
    }
}

// One AdamW update of four elements.  Floating-point contraction is OFF: adamw_kernel and the two table kernels below must give
// bit-identical results for the same element whatever the surrounding code lets the compiler fuse.
// The moments are updated in torch's operation order, which decides what a non-finite or huge gradient leaves behind
// (tests/test_adamw_gpu.py): m as exp_avg.lerp_(g, 1 - b1) = m + (g - m) (1 - b1) -- an infinite gradient makes m NaN on the next
// step, as in torch; m b1 + g (1 - b1) would keep it at inf -- and v as exp_avg_sq.mul_(b2).addcmul_(g, g, value = 1 - b2) =
// v b2 + ((1 - b2) g) g: g g alone overflows from |g| = 1.8e19 on, where (1 - b2) g^2 still fits fp32; v would become inf and the
// element would never move again (sqrt(v) = inf in every later denominator).
__device__ __forceinline__ void adamw_elem4(f32x4& pp, const f32x4 gg, f32x4& mm, f32x4& vv, float lr, float b1, float b2, float eps, float wd,
                                            float step, float bc2_sqrt) {
#pragma clang fp contract(off)
    pp *= (1.0f - lr * wd);
    mm = mm + (gg - mm) * (1.0f - b1);
    vv = vv * b2 + gg * (1.0f - b2) * gg;
    f32x4 den;
    den.x = sqrtf(vv.x) / bc2_sqrt + eps; den.y = sqrtf(vv.y) / bc2_sqrt + eps;
    den.z = sqrtf(vv.z) / bc2_sqrt + eps; den.w = sqrtf(vv.w) / bc2_sqrt + eps;
    pp.x -= step * (mm.x / den.x); pp.y -= step * (mm.y / den.y);
    pp.z -= step * (mm.z / den.z); pp.w -= step * (mm.w / den.w);
}
// the gradient seen by a clipped step: g * coef rounded to fp32, as torch's g.mul_(clip_coef) leaves it (SCALED = false: g as is)
template <bool SCALED>
__device__ __forceinline__ f32x4 adamw_grad4(f32x4 gg, const float* coef) {
#pragma clang fp contract(off)
    if constexpr (SCALED) { const float c = *coef; gg *= c; }
    return gg;
}
// The scalars of one step, stated once for every kernel of the family: the by-value arguments, or with `live` the bias corrections
// and the count of the device-side step state, and for lr < 0 (SEGMM_LIVE_LR) the scheduled rate of that step as well.  A kernel
// that has no use for the count passes 0 and never reads it (the load is dead).
struct StepScalars { float lr, bc1, bc2_sqrt; int t; };
__device__ __forceinline__ StepScalars step_scalars(float lr, float bc1, float bc2_sqrt, int t, const StepState* live) {
    if (live) { t = live->step; bc1 = live->bc1; bc2_sqrt = live->bc2_sqrt; if (lr < 0.f) lr = live->lr; }
    return {lr, bc1, bc2_sqrt, t};
}
// the rate fp32(lr * lr_scale) and the step fp32(rate / bc1), in this order and with these two roundings everywhere (lr_scale = 1
// leaves every bit of lr as it is: adamw_kernel passes the literal, and the multiply folds away)
struct StepRate { float lr, step; };
__device__ __forceinline__ StepRate step_rate(float lr, float lr_scale, float bc1) {
#pragma clang fp contract(off)
    lr = lr * lr_scale;
    return {lr, lr / bc1};
}
// ---------------------------------------------------------------- fused AdamW over a flat range (a13 / K9)
// torch.optim.AdamW single-tensor update order (decoupled decay first), bias corrections passed in.
// SCALED: the gradient is multiplied by *coef first (segmm_adamw_scaled: the clip coefficient segmm_grad_norm wrote)
// GUARD (the *_guarded entry points; `live` is then never null): one wave-uniform read of the live state's verdict -- a scalar load --
// and the workgroup of a skipped step returns before it loads anything else.  GUARD = false is the kernel as it always was: it does
// not read the word.  The same parameter, with the same meaning, on the groups, id-table and EMA kernels below.
__device__ __forceinline__ bool step_skipped(const StepState* live) { return live->skip != 0u; }
template <bool SCALED, bool GUARD = false>
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                             float* __restrict__ v, long long n, float lr, float b1, float b2, float eps, float wd,
                             float bc1, float bc2_sqrt, const StepState* live, const float* __restrict__ coef) {
    if constexpr (GUARD) { if (step_skipped(live)) return; }
    const StepScalars sc = step_scalars(lr, bc1, bc2_sqrt, 0, live);
    const long long n4 = n >> 2;
    const StepRate r = step_rate(sc.lr, 1.0f, sc.bc1);
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        f32x4 pp = ((f32x4*)p)[i];
        const f32x4 gg = adamw_grad4<SCALED>(((const f32x4*)g)[i], coef);
        f32x4 mm = ((f32x4*)m)[i], vv = ((f32x4*)v)[i];
        adamw_elem4(pp, gg, mm, vv, r.lr, b1, b2, eps, wd, r.step, sc.bc2_sqrt);
        ((f32x4*)p)[i] = pp; ((f32x4*)m)[i] = mm; ((f32x4*)v)[i] = vv;
    }
    // tail (n % 4)
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const long long i = (n4 << 2) + threadIdx.x;
        f32x4 pp = {p[i], 0.f, 0.f, 0.f}, mm = {m[i], 0.f, 0.f, 0.f}, vv = {v[i], 0.f, 0.f, 0.f};
        adamw_elem4(pp, adamw_grad4<SCALED>(f32x4{g[i], 0.f, 0.f, 0.f}, coef), mm, vv, r.lr, b1, b2, eps, wd, r.step, sc.bc2_sqrt);
        p[i] = pp.x; m[i] = mm.x; v[i] = vv.x;
    }
}

// ---------------------------------------------------------------- AdamW over a flat range cut into parameter-group segments
// (segmm_adamw_groups).  Segment s covers the floats [seg_end[s - 1], seg_end[s]) counted from the buffers' base (seg_end[-1] = 0);
// floats at or beyond seg_end[n_seg - 1] go with the last segment.  Every end but the last is a multiple of 4, so a 16-byte vector
// never straddles two segments.
// seg_find: the segment of float offset e, searched in [lo, n_seg): the first s with seg_end[s] > e.  Callers pass wave-uniform
// arguments (the search runs on the scalar unit) and a lower bound that only grows as a grid-stride loop advances.
__device__ __forceinline__ int seg_find(const long long* __restrict__ seg_end, int n_seg, int lo, long long e) {
    int hi = n_seg - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (seg_end[mid] > e) hi = mid; else lo = mid + 1;
    }
    return lo;
}
// The walk over the range is adamw_kernel's (same grid, same stride: 28 B per element of HBM traffic either way).  A wave's 64
// vectors of one iteration are 256 consecutive floats: their segment is resolved ONCE per wave and iteration; where all 256 lie in
// one segment (every wave but the few that sit on a segment end) the rate lr * lr_scale[s], the step and the decay are computed
// once, wave-uniform.  A wave that sits on an end lets each lane walk on from the wave's segment to its own.  Per element the
// arithmetic is adamw_elem4 with lr = fp32(lr * lr_scale[s]) and wd = seg_wd[s]: bit for bit adamw_kernel launched on that
// segment alone.  Elements of a frozen segment are neither loaded nor stored.
// FROZEN = false (seg_frozen == NULL: the caller knows that no segment is frozen): the loads of p, g, m, v do not wait for the table --
// with a frozen flag to honour, a wave must have read the table before it may touch its elements, one dependent round trip more than
// adamw_kernel has and at a cache-resident size (a wave runs one or two iterations) about half a microsecond of a 28 us launch
// (profiles/param_groups/adamw_groups_bench.txt and profiles/README.md).
template <bool SCALED, bool FROZEN, bool GUARD = false>
__global__ __launch_bounds__(256) void adamw_groups_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                             float* __restrict__ v, long long start, long long n, const long long* __restrict__ seg_end,
                             const float* __restrict__ seg_lr_scale, const float* __restrict__ seg_wd,
                             const unsigned char* __restrict__ seg_frozen, int n_seg, float lr, float b1, float b2, float eps,
                             float bc1, float bc2_sqrt, const StepState* live, const float* __restrict__ coef) {
#pragma clang fp contract(off)
    if constexpr (GUARD) { if (step_skipped(live)) return; }
    const StepScalars st = step_scalars(lr, bc1, bc2_sqrt, 0, live);
    const long long n4 = n >> 2;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    f32x4* p4 = (f32x4*)(p + start); const f32x4* g4 = (const f32x4*)(g + start);
    f32x4* m4 = (f32x4*)(m + start); f32x4* v4 = (f32x4*)(v + start);
    int s = 0;
    for (long long w0 = blockIdx.x * (long long)blockDim.x + wave * 64; w0 < n4; w0 += (long long)gridDim.x * blockDim.x) {
        const long long e0 = start + (w0 << 2);                                   // the wave's first float, from the buffers' base
        long long e1 = e0 + 256;                                                  // one past its last
        if (e1 > start + (n4 << 2)) e1 = start + (n4 << 2);
        s = seg_find(seg_end, n_seg, s, e0);
        const long long i = w0 + lane;
        // the wave's segment: its four table entries in one round of scalar loads (nothing below waits for one after the other)
        const long long end_s = seg_end[s];
        unsigned char fz = 0;
        if constexpr (FROZEN) fz = seg_frozen[s];
        float sc = seg_lr_scale[s], wd = seg_wd[s];
        if (end_s < e1 && s < n_seg - 1) {                                        // a segment ends inside the wave's 256 floats
            const long long e = e0 + (lane << 2);
            int ls = s;
            while (ls < n_seg - 1 && seg_end[ls] <= e) ++ls;
            if constexpr (FROZEN) fz = seg_frozen[ls];
            sc = seg_lr_scale[ls]; wd = seg_wd[ls];
        }
        if (i >= n4 || fz) continue;
        const StepRate r = step_rate(st.lr, sc, st.bc1);
        f32x4 pp = p4[i];
        const f32x4 gg = adamw_grad4<SCALED>(g4[i], coef);
        f32x4 mm = m4[i], vv = v4[i];
        adamw_elem4(pp, gg, mm, vv, r.lr, b1, b2, eps, wd, r.step, st.bc2_sqrt);
        p4[i] = pp; m4[i] = mm; v4[i] = vv;
    }
    // tail (n % 4): the last segment the range touches
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const long long i = start + (n4 << 2) + threadIdx.x;
        const int ls = seg_find(seg_end, n_seg, 0, start + n - 1);
        if (!FROZEN || !seg_frozen[ls]) {
            const StepRate r = step_rate(st.lr, seg_lr_scale[ls], st.bc1);
            f32x4 pp = {p[i], 0.f, 0.f, 0.f}, mm = {m[i], 0.f, 0.f, 0.f}, vv = {v[i], 0.f, 0.f, 0.f};
            adamw_elem4(pp, adamw_grad4<SCALED>(f32x4{g[i], 0.f, 0.f, 0.f}, coef), mm, vv, r.lr, b1, b2, eps, seg_wd[ls], r.step, st.bc2_sqrt);
            p[i] = pp.x; m[i] = mm.x; v[i] = vv.x;
        }
    }
}

// AdamW of an id-embedding table in two passes (segmm_adamw_table): the arithmetic of adamw_kernel, element for element
// (lr_scale: the rate is fp32(lr * lr_scale), lr being the argument or the device state's -- segmm_adamw_table_lrs; 1 elsewhere,
// which leaves every bit of lr as it is)
// (GUARD: a skipped step marks nothing -- its phase 1 returns as well and would leave the marks standing)
template <bool GUARD = false>
__global__ __launch_bounds__(256) void table_mark_kernel(const long long* __restrict__ ids, int n, long long n_rows, unsigned int* __restrict__ flags,
                                                         const StepState* live) {
    if constexpr (GUARD) { if (step_skipped(live)) return; }
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) {
        const long long id = ids[k];
        if (id >= 0 && id < n_rows) flags[id] = 1u;
    }
}
// every row WITHOUT a mark, g = 0
template <bool GUARD = false>
__global__ __launch_bounds__(256) void adamw_table_rest_kernel(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v, long long n_rows,
                                                               int w4, const unsigned int* __restrict__ flags, float lr, float b1, float b2,
                                                               float eps, float wd, float bc1, float bc2_sqrt, const StepState* live,
                                                               float lr_scale) {
#pragma clang fp contract(off)
    if constexpr (GUARD) { if (step_skipped(live)) return; }
    const StepScalars sc = step_scalars(lr, bc1, bc2_sqrt, 0, live);
    const StepRate r = step_rate(sc.lr, lr_scale, sc.bc1);
    const long long n4 = n_rows * w4;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        if (flags[i / w4] != 0u) continue;
        f32x4 pp = ((f32x4*)p)[i], mm = ((f32x4*)m)[i], vv = ((f32x4*)v)[i];
        adamw_elem4(pp, zero, mm, vv, r.lr, b1, b2, eps, wd, r.step, sc.bc2_sqrt);
        ((f32x4*)p)[i] = pp; ((f32x4*)m)[i] = mm; ((f32x4*)v)[i] = vv;
    }
}
// the marked rows, each once: one wave per list entry; lane 0 claims (and clears) the row's mark
template <bool SCALED, bool GUARD = false>
__global__ __launch_bounds__(256) void adamw_table_rows_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                               float* __restrict__ v, long long n_rows, int w4, const long long* __restrict__ ids,
                                                               int n_ids, unsigned int* __restrict__ flags, float lr, float b1, float b2, float eps,
                                                               float wd, float bc1, float bc2_sqrt, const StepState* live,
                                                               const float* __restrict__ coef, float lr_scale) {
#pragma clang fp contract(off)
    if constexpr (GUARD) { if (step_skipped(live)) return; }
    const StepScalars sc = step_scalars(lr, bc1, bc2_sqrt, 0, live);
    const StepRate r = step_rate(sc.lr, lr_scale, sc.bc1);
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (k >= n_ids) return;
    const long long id = ids[k];
    if (id < 0 || id >= n_rows) return;
    unsigned int mine = 0u;
    if (lane == 0) mine = atomicExch(flags + id, 0u);
    mine = (unsigned int)__builtin_amdgcn_readfirstlane((int)mine);
    if (mine == 0u) return;          // another entry of the list holds the same id and has taken the row
    for (int c = lane; c < w4; c += 64) {
        const long long i = id * w4 + c;
        f32x4 pp = ((f32x4*)p)[i], mm = ((f32x4*)m)[i], vv = ((f32x4*)v)[i];
        adamw_elem4(pp, adamw_grad4<SCALED>(((const f32x4*)g)[i], coef), mm, vv, r.lr, b1, b2, eps, wd, r.step, sc.bc2_sqrt);
        ((f32x4*)p)[i] = pp; ((f32x4*)m)[i] = mm; ((f32x4*)v)[i] = vv;
    }
}

// ---------------------------------------------------------------- global 2-norm of a flat gradient range (segmm_grad_norm)
// torch.nn.utils.clip_grad_norm_(params, max_norm) without a host sync: sum of squares in fp64 (the square of an fp32 value is
// exact in fp64, so fp32 gradients near 1e-20 or 1e19 neither underflow nor overflow), one partial per workgroup into caller-owned
// scratch, then a fixed-order sum in a second one-workgroup launch.  No atomics: the same gradient gives the same bits every run.
constexpr int GRAD_NORM_PARTS = 1024;          // workgroups (and fp64 partials) at most
__device__ __forceinline__ double sq4(f32x4 x) {
    return ((double)x.x * x.x + (double)x.y * x.y) + ((double)x.z * x.z + (double)x.w * x.w);
}
// fixed-order sum of one value per thread of a 256-thread workgroup; the result is valid in thread 0
__device__ __forceinline__ double block_sum256(double acc, double* red) {
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
// g: the range from its first 16-byte boundary (`lead` < 4 floats before it are read by workgroup 0), n4 whole vectors, then `tail`
__global__ __launch_bounds__(256) void sumsq_parts_kernel(const float* __restrict__ g, int lead, long long n4, int tail,
                                                          double* __restrict__ parts) {
    __shared__ double red[4];
    const f32x4* g4 = (const f32x4*)(g + lead);
    const long long stride = (long long)gridDim.x * blockDim.x;
    long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    double acc = 0.0;
    for (; i + 3 * stride < n4; i += 4 * stride) {          // four independent 16-B loads in flight per lane
        const f32x4 a = g4[i], b = g4[i + stride], c = g4[i + 2 * stride], d = g4[i + 3 * stride];
        acc += (sq4(a) + sq4(b)) + (sq4(c) + sq4(d));
    }
    for (; i < n4; i += stride) acc += sq4(g4[i]);
    if (blockIdx.x == 0) {
        if (threadIdx.x < lead) acc += (double)g[threadIdx.x] * g[threadIdx.x];
        if (threadIdx.x < tail) {
            const float x = g[lead + (n4 << 2) + threadIdx.x];
            acc += (double)x * x;
        }
    }
    acc = block_sum256(acc, red);
    if (threadIdx.x == 0) parts[blockIdx.x] = acc;
}
// segmm_grad_norm_groups: the partials of g[0, n) WITHOUT the frozen segments (the table of adamw_groups_kernel; g is the buffers'
// base, 16-byte aligned).  A wave resolves the segment of its 256 consecutive floats once per iteration, as adamw_groups_kernel does;
// a frozen element is not loaded, so whatever it holds (NaN, inf) cannot reach a partial.  Fixed order: same gradient, same bits.
__global__ __launch_bounds__(256) void sumsq_parts_groups_kernel(const float* __restrict__ g, long long n, const long long* __restrict__ seg_end,
                                                                 const unsigned char* __restrict__ seg_frozen, int n_seg,
                                                                 double* __restrict__ parts) {
    __shared__ double red[4];
    const f32x4* g4 = (const f32x4*)g;
    const long long n4 = n >> 2;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    double acc = 0.0;
    int s = 0;
    for (long long w0 = blockIdx.x * (long long)blockDim.x + wave * 64; w0 < n4; w0 += (long long)gridDim.x * blockDim.x) {
        const long long e0 = w0 << 2;
        long long e1 = e0 + 256;
        if (e1 > (n4 << 2)) e1 = n4 << 2;
        s = seg_find(seg_end, n_seg, s, e0);
        const long long i = w0 + lane;
        int ls = s;
        if (seg_end[s] < e1 && s < n_seg - 1) {
            const long long e = e0 + (lane << 2);
            while (ls < n_seg - 1 && seg_end[ls] <= e) ++ls;
        }
        if (i < n4 && !seg_frozen[ls]) acc += sq4(g4[i]);
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3) && !seg_frozen[seg_find(seg_end, n_seg, 0, n - 1)]) {
        const float x = g[(n4 << 2) + threadIdx.x];
        acc += (double)x * x;
    }
    acc = block_sum256(acc, red);
    if (threadIdx.x == 0) parts[blockIdx.x] = acc;
}
// out2 = {total_norm, coef}: coef = min(1, max_norm / (total_norm + 1e-6)) in fp32 the way torch evaluates it
// (clip_grad_norm_: max_norm / t is t.reciprocal() * max_norm; torch.clamp keeps a NaN); max_norm = inf: coef = 1, never a clip
__global__ __launch_bounds__(256) void grad_norm_finish_kernel(const double* __restrict__ parts, int nparts, float max_norm,
                                                               float* __restrict__ out2) {
#pragma clang fp contract(off)
    __shared__ double red[4];
    double acc = 0.0;
    for (int k = threadIdx.x; k < nparts; k += 256) acc += parts[k];
    acc = block_sum256(acc, red);
    if (threadIdx.x == 0) {
        const float t = (float)sqrt(acc);
        float c = 1.0f;
        if (!__builtin_isinf(max_norm)) {
            c = (1.0f / (t + 1e-6f)) * max_norm;
            if (c > 1.0f) c = 1.0f;
        }
        out2[0] = t;
        out2[1] = c;
    }
}
// segmm_step_guard: the verdict of the step, one thread behind grad_norm_finish_kernel on the same stream.  The norm is finite iff
// every live, non-frozen gradient element is (fp64 partials of fp32 squares cannot overflow), so NaN or inf here is the whole test.
// Ordinary stores, as the other one-thread state kernels make them.
__global__ void step_guard_kernel(StepState* st, const float* __restrict__ out2) {
    const float t = out2[0];
    const uint32_t bad = (__builtin_isnan(t) || __builtin_isinf(t)) ? 1u : 0u;
    st->skip = bad;
    st->skipped = st->skipped + bad;
}

// ---------------------------------------------------------------- out = a + b over a flat range (segmm_vec_add)
// The gradient sum of a micro-batched step (Trainer(micro_batch=m)): one IEEE fp32 add per element, nothing to contract.  12 bytes of
// traffic per element and no arithmetic worth the name, so the kernel is its loads: one round of resident workgroups (eight of 256
// threads per CU, <= 64 registers) walks the range.  A lane with four or more grid-stride steps left issues four 16-byte loads of each
// operand before its first add; what is left after that goes one vector per iteration (load, load, add, store: `out` may alias an
// operand, so the compiler keeps the next loads behind the store).  With 8 CUs' worth of workgroups the stride is 2048 x CUs lanes: at the
// config-2 model's 1.65 M vectors on 256 CUs only the lanes below n4 - 3 stride (about one in seven) take the unrolled loop, the others
// three single iterations -- there the 32 resident waves per CU are what covers the load latency (profiles/micro_batch/vec_add_bench.txt);
// from 4 x that size on every lane unrolls.
// `out` may be exactly `a` or exactly `b` (no __restrict__): a lane reads the elements it owns before it writes them and owns them alone.
// VEC: the three pointers share their offset from a 16-byte boundary -- `lead` (< 4) scalar elements, n4 whole vectors, `tail` (< 4)
// scalar elements, the scalars by workgroup 0.  Otherwise (the pointers disagree mod 16 bytes; no caller in the step) one dword per
// lane: coalesced, and no unaligned vector access.
constexpr int VEC_ADD_WG_PER_CU = 8;
template <bool VEC>
__global__ __launch_bounds__(256, VEC_ADD_WG_PER_CU) void vec_add_kernel(float* out, const float* a, const float* b, int lead, long long n4, int tail) {
#pragma clang fp contract(off)
    const long long stride = (long long)gridDim.x * blockDim.x;
    long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if constexpr (VEC) {
        f32x4* o4 = (f32x4*)(out + lead);
        const f32x4 *a4 = (const f32x4*)(a + lead), *b4 = (const f32x4*)(b + lead);
        for (; i + 3 * stride < n4; i += 4 * stride) {
            const f32x4 a0 = a4[i], a1 = a4[i + stride], a2 = a4[i + 2 * stride], a3 = a4[i + 3 * stride];
            const f32x4 b0 = b4[i], b1 = b4[i + stride], b2 = b4[i + 2 * stride], b3 = b4[i + 3 * stride];
            o4[i] = a0 + b0; o4[i + stride] = a1 + b1; o4[i + 2 * stride] = a2 + b2; o4[i + 3 * stride] = a3 + b3;
        }
        for (; i < n4; i += stride) o4[i] = a4[i] + b4[i];
        if (blockIdx.x == 0) {
            const int t = threadIdx.x;
            if (t < lead) out[t] = a[t] + b[t];
            if (t < tail) {
                const long long k = lead + (n4 << 2) + t;
                out[k] = a[k] + b[k];
            }
        }
    } else {          // n4 counts single elements here
        for (; i + 3 * stride < n4; i += 4 * stride) {
            const float a0 = a[i], a1 = a[i + stride], a2 = a[i + 2 * stride], a3 = a[i + 3 * stride];
            const float b0 = b[i], b1 = b[i + stride], b2 = b[i + 2 * stride], b3 = b[i + 3 * stride];
            out[i] = a0 + b0; out[i + stride] = a1 + b1; out[i + 2 * stride] = a2 + b2; out[i + 3 * stride] = a3 + b3;
        }
        for (; i < n4; i += stride) out[i] = a[i] + b[i];
    }
}

// ---------------------------------------------------------------- shadow += (p - shadow) w over a flat range (segmm_ema_update)
// The weight average of Trainer(ema=...): three IEEE fp32 operations per element (subtract, multiply, add; nothing contracted), 12
// bytes of traffic per element -- vec_add_kernel's `acc <- acc + g` form, and its shape: one round of resident workgroups, four
// 16-byte loads of each operand in flight before the first store, then single vectors, the n % 4 tail by workgroup 0.  Both pointers
// are 16-byte aligned and the ranges disjoint (the entry point refuses anything else), so there is no scalar head and no dword form.
// w is wave-uniform: the weight, or under warm-up max(weight, fp32(9 / (10 + t))) with t the step by value or `live->step` -- one
// double division per lane, issued beside the first loads.
// NT (knob EMA_NT, off by default): the shadow loaded and stored nontemporally, p with the default policy.  The shadow is touched once
// per step and by nothing else, which is what made nontemporal traffic pay for the row kernels that run BESIDE the GEMMs; this launch
// runs alone at the end of the step's tail, and measured in the recorded config-2 step the two policies tie within the step's spread,
// while alone at 4 x the config-2 size the nontemporal form is 6-8 % slower (profiles/ema/): the default policy stays.
__device__ __forceinline__ float ema_weight(float weight, int warmup, int step, const StepState* live) {
#pragma clang fp contract(off)
    if (!warmup) return weight;
    const int t = live ? live->step : step;
    const float wt = (float)(9.0 / (10.0 + (double)t));
    return wt > weight ? wt : weight;
}
template <bool NT>
__device__ __forceinline__ f32x4 ema_ld(const f32x4* q) {
    if constexpr (NT) return __builtin_nontemporal_load(q);
    else return *q;
}
template <bool NT>
__device__ __forceinline__ void ema_st(f32x4* q, f32x4 v) {
    if constexpr (NT) __builtin_nontemporal_store(v, q);
    else *q = v;
}
__device__ __forceinline__ f32x4 ema_lerp(f32x4 s, f32x4 p, float w) {
#pragma clang fp contract(off)
    const f32x4 d = p - s;
    const f32x4 dw = d * w;
    return s + dw;
}
template <bool NT, bool GUARD = false>
__global__ __launch_bounds__(256, VEC_ADD_WG_PER_CU) void ema_update_kernel(float* __restrict__ shadow, const float* __restrict__ p, long long n4, int tail,
                                                                            float weight, int warmup, int step, const StepState* live) {
#pragma clang fp contract(off)
    if constexpr (GUARD) { if (step_skipped(live)) return; }
    const long long stride = (long long)gridDim.x * blockDim.x;
    long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    f32x4* s4 = (f32x4*)shadow;
    const f32x4* p4 = (const f32x4*)p;
    const float w = ema_weight(weight, warmup, step, live);
    for (; i + 3 * stride < n4; i += 4 * stride) {
        const f32x4 s0 = ema_ld<NT>(s4 + i), s1 = ema_ld<NT>(s4 + i + stride), s2 = ema_ld<NT>(s4 + i + 2 * stride), s3 = ema_ld<NT>(s4 + i + 3 * stride);
        const f32x4 p0 = p4[i], p1 = p4[i + stride], p2 = p4[i + 2 * stride], p3 = p4[i + 3 * stride];
        ema_st<NT>(s4 + i, ema_lerp(s0, p0, w)); ema_st<NT>(s4 + i + stride, ema_lerp(s1, p1, w));
        ema_st<NT>(s4 + i + 2 * stride, ema_lerp(s2, p2, w)); ema_st<NT>(s4 + i + 3 * stride, ema_lerp(s3, p3, w));
    }
    for (; i < n4; i += stride) ema_st<NT>(s4 + i, ema_lerp(ema_ld<NT>(s4 + i), p4[i], w));
    if (blockIdx.x == 0 && (int)threadIdx.x < tail) {
        const long long k = (n4 << 2) + threadIdx.x;
        const float s = shadow[k];
        const float d = p[k] - s;
        const float dw = d * w;
        shadow[k] = s + dw;
    }
}

// ---------------------------------------------------------------- lazy exact AdamW of an id table (segmm_adamw_table_catchup)
// A row without a gradient takes a step that depends on nothing but its own (p, m, v) and the step's scalars, so the step can be
// taken LATER, in order, with the same fp32 operations: bit for bit adamw_table_rest_kernel's update of that row.  Each row carries
// a stamp (int32: the optimizer steps already applied to it); the scalars of step t that move from step to step -- the rate
// before lr_scale, bc1, bc2_sqrt -- sit in slot t % cap of a device ring, one 16-byte entry per step (adamw_hist_push_kernel).
// With the EMA shadow replayed beside the row (EMA = true: segmm_adamw_hist_push_ema, segmm_adamw_table_catchup_ema,
// segmm_adamw_table_lazy_rows_ema): what holds for a row's (p, m, v) holds for its shadow.  shadow_t = shadow_{t-1} +
// (p_t - shadow_{t-1}) w_t depends on the row's own p_t and on the step's weight only, so a row that replays its missed steps
// replays its shadow with them, in order, with ema_lerp's three rounded operations: after a flush the shadow holds the bits
// ema_update_kernel leaves when it runs over the dense table every step.  w_t sits in the fourth float of the ring's entry of
// step t -- the weight that step actually used, so the EMA's decay may move between steps (0 where no EMA is kept).  The shadow is
// a fourth vector per lane; its lerp does not feed the next AdamW step, so it is independent work beside the dependent sqrt /
// divide chain.
struct AdamwHist { float lr, bc1, bc2_sqrt, ema_w; };
template <bool EMA>
__global__ void adamw_hist_push_kernel(AdamwHist* __restrict__ hist, int cap, int t, float lr, float bc1, float bc2_sqrt, float weight, int warmup,
                                       const StepState* live) {
    float w = 0.f;
    if constexpr (EMA) w = ema_weight(weight, warmup, t, live);          // (ema_update_kernel's call: t by value, or the state's count)
    const StepScalars sc = step_scalars(lr, bc1, bc2_sqrt, t, live);
    if (sc.t < 0) return;          // (a step state that was never set)
    hist[sc.t % cap] = AdamwHist{sc.lr, sc.bc1, sc.bc2_sqrt, w};
}
// the stamps of the listed rows become at least `target` (the rows phase 1 has just stepped); ids == NULL: every stamp IS target
__global__ __launch_bounds__(256) void table_stamp_kernel(const long long* __restrict__ ids, long long n, long long n_rows, int* __restrict__ stamps,
                                                          int target, const StepState* live) {
    if (live) target += live->step;
    for (long long k = blockIdx.x * (long long)blockDim.x + threadIdx.x; k < n; k += (long long)gridDim.x * blockDim.x) {
        if (!ids) { stamps[k] = target; continue; }
        const long long id = ids[k];
        if (id >= 0 && id < n_rows) atomicMax(stamps + id, target);
    }
}
// The g = 0 steps from .. end - 1 of this lane's four elements, from the ring: per step the AdamW step with that step's scalars, then
// (EMA) the shadow's lerp with that step's weight.  Whatever `from` holds, the slot is in the ring (a stamp is never negative).
template <bool EMA>
__device__ __forceinline__ void adamw_replay4(f32x4& pp, f32x4& mm, f32x4& vv, f32x4& ss, const AdamwHist* __restrict__ hist, int cap, int from,
                                              int end, float lr_scale, float b1, float b2, float eps, float wd) {
#pragma clang fp contract(off)
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    int slot = (int)((unsigned)from % (unsigned)cap);
    for (int s = from; s < end; ++s) {
        const AdamwHist h = hist[slot];
        slot = slot + 1 == cap ? 0 : slot + 1;
        const StepRate r = step_rate(h.lr, lr_scale, h.bc1);
        adamw_elem4(pp, zero, mm, vv, r.lr, b1, b2, eps, wd, r.step, h.bc2_sqrt);
        if constexpr (EMA) ss = ema_lerp(ss, pp, h.ema_w);
    }
}
// The row claim of the row-per-wave kernels below: lane 0 raises the row's stamp to `target` with an atomic max and the wave learns
// what the stamp was.  A second list entry with the same id, or a row already at target, finds old >= target and leaves the row
// alone (no load, no store); so does a wave whose id is outside the table (valid = false: nothing is touched, old = target).
__device__ __forceinline__ int row_claim(int* __restrict__ stamps, long long id, int target, bool valid, int lane) {
    int old = target;
    if (lane == 0 && valid) old = atomicMax(stamps + id, target);
    return __builtin_amdgcn_readfirstlane(old);
}
// Rows behind `target` replay their missed steps stamp + 1 .. target with g = 0 from the ring and are written once.  One wave per
// row, four rows per workgroup, four floats per lane (adamw_table_rows_kernel's shape).  ids == NULL: the rows 0 .. n_items - 1
// themselves (the flush; the grid is capped and strides).  flags != NULL (EMA = false only; the EMA form takes none and compiles
// them out): every valid listed row is marked for phase 1 of segmm_adamw_table, which the lazy step runs without a phase 0.
// target - stamp <= cap is the caller's rule (a slot is overwritten cap steps later).  The replay is a dependent chain of sqrt and
// divide per element and step; four independent elements per lane keep the VALU busy from one wave: a whole workgroup per row with
// one float per thread (four waves per row at width 256) measured 2.7-2.9x SLOWER per row-step at every gap from 32 to 1024 and
// 3.9x in the flush (profiles/lazy_tables/), and was dropped.
// (`flags` stays the LAST argument: ahead of `hist` it moved the kernel arguments of the EMA form, which never reads it, and that
// form compiled to 65 VGPRs instead of 50 -- one occupancy step down; profiles/adamw_once/kernel_resources.txt)
template <bool EMA>
__global__ __launch_bounds__(256) void adamw_table_catchup_kernel(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                                  float* __restrict__ shadow, long long n_rows, int width,
                                                                  const long long* __restrict__ ids, long long n_items, int* __restrict__ stamps,
                                                                  const AdamwHist* __restrict__ hist, int cap, int target, const StepState* live,
                                                                  float lr_scale, float b1, float b2, float eps, float wd,
                                                                  unsigned int* __restrict__ flags) {
    if (live) target += live->step;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int w4 = width >> 2;
    for (long long k = blockIdx.x * 4LL + wave; k < n_items; k += gridDim.x * 4LL) {
        const long long id = ids ? ids[k] : k;
        const bool valid = id >= 0 && id < n_rows;
        if constexpr (!EMA) { if (lane == 0 && valid && flags) flags[id] = 1u; }
        const int old = row_claim(stamps, id, target, valid, lane);
        if (old >= target) continue;
        for (int c = lane; c < w4; c += 64) {
            const long long i = id * w4 + c;
            f32x4 pp = ((f32x4*)p)[i], mm = ((f32x4*)m)[i], vv = ((f32x4*)v)[i], ss = {0.f, 0.f, 0.f, 0.f};
            if constexpr (EMA) ss = ((f32x4*)shadow)[i];
            adamw_replay4<EMA>(pp, mm, vv, ss, hist, cap, old + 1, target + 1, lr_scale, b1, b2, eps, wd);
            ((f32x4*)p)[i] = pp; ((f32x4*)m)[i] = mm; ((f32x4*)v)[i] = vv;
            if constexpr (EMA) ((f32x4*)shadow)[i] = ss;
        }
    }
}
// The data-parallel tail of a lazy step (segmm_adamw_table_lazy_rows): the listed rows -- those of ALL ranks, known only after the
// row exchange -- replay the g = 0 steps old + 1 .. T - 1 from the ring and then take step T with their gradient row and step T's
// own scalars (adamw_table_rows_kernel's), in one pass over the row: p, m, v are read once and written once, where catch-up +
// phase 1 + stamp read and write them twice in three launches on the exposed end of the step.  The same shape, one wave per list
// entry and four floats per lane; the claim is made with T itself, so no flags are involved: a duplicate entry, or a row already
// at T, is neither loaded nor stored.  The gradient vector is loaded ahead of the replay: nothing needs it before the dependent
// sqrt / divide chain of the replayed steps has run, which hides its latency (at a gap of 0 it travels with p, m, v in one round).
// EMA: after step T the shadow's lerp with w_T -- read from the ring's entry of T, which adamw_hist_push_kernel<true> wrote on
// this stream ahead of this launch.
template <bool SCALED, bool EMA>
__global__ __launch_bounds__(256) void adamw_table_lazy_rows_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                                    float* __restrict__ v, float* __restrict__ shadow, long long n_rows, int w4,
                                                                    const long long* __restrict__ ids, int n_ids, int* __restrict__ stamps,
                                                                    const AdamwHist* __restrict__ hist, int cap, int T, float lr, float b1, float b2,
                                                                    float eps, float wd, float bc1, float bc2_sqrt, const StepState* live,
                                                                    const float* __restrict__ coef, float lr_scale) {
    const StepScalars sc = step_scalars(lr, bc1, bc2_sqrt, T, live);
    const StepRate r = step_rate(sc.lr, lr_scale, sc.bc1);
    T = sc.t;
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (k >= n_ids) return;
    const long long id = ids[k];
    if (id < 0 || id >= n_rows) return;
    const int old = row_claim(stamps, id, T, true, lane);
    if (old >= T) return;          // another entry of the list holds the same id and has taken the row, or the row was stepped already
    float w_T = 0.f;
    if constexpr (EMA) w_T = hist[(unsigned)T % (unsigned)cap].ema_w;
    for (int c = lane; c < w4; c += 64) {
        const long long i = id * w4 + c;
        const f32x4 graw = ((const f32x4*)g)[i];
        f32x4 pp = ((f32x4*)p)[i], mm = ((f32x4*)m)[i], vv = ((f32x4*)v)[i], ss = {0.f, 0.f, 0.f, 0.f};
        if constexpr (EMA) ss = ((f32x4*)shadow)[i];
        adamw_replay4<EMA>(pp, mm, vv, ss, hist, cap, old + 1, T, lr_scale, b1, b2, eps, wd);
        adamw_elem4(pp, adamw_grad4<SCALED>(graw, coef), mm, vv, r.lr, b1, b2, eps, wd, r.step, sc.bc2_sqrt);
        ((f32x4*)p)[i] = pp; ((f32x4*)m)[i] = mm; ((f32x4*)v)[i] = vv;
        if constexpr (EMA) { ss = ema_lerp(ss, pp, w_T); ((f32x4*)shadow)[i] = ss; }
    }
}

// ---------------------------------------------------------------- a <-> b over a flat range (segmm_vec_swap)
// WeightEMA.applied(): the shadow goes into the live range of the flat parameter buffer and back.  16 bytes of traffic per element;
// the shape of the two kernels above (a lane reads the elements it owns from both ranges before it writes them).
__global__ __launch_bounds__(256, VEC_ADD_WG_PER_CU) void vec_swap_kernel(float* __restrict__ a, float* __restrict__ b, long long n4, int tail) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    f32x4 *a4 = (f32x4*)a, *b4 = (f32x4*)b;
    for (; i + 3 * stride < n4; i += 4 * stride) {
        const f32x4 a0 = a4[i], a1 = a4[i + stride], a2 = a4[i + 2 * stride], a3 = a4[i + 3 * stride];
        const f32x4 b0 = b4[i], b1 = b4[i + stride], b2 = b4[i + 2 * stride], b3 = b4[i + 3 * stride];
        a4[i] = b0; a4[i + stride] = b1; a4[i + 2 * stride] = b2; a4[i + 3 * stride] = b3;
        b4[i] = a0; b4[i + stride] = a1; b4[i + 2 * stride] = a2; b4[i + 3 * stride] = a3;
    }
    for (; i < n4; i += stride) {
        const f32x4 x = a4[i], y = b4[i];
        a4[i] = y;
        b4[i] = x;
    }
    if (blockIdx.x == 0 && (int)threadIdx.x < tail) {
        const long long k = (n4 << 2) + threadIdx.x;
        const float x = a[k], y = b[k];
        a[k] = y;
        b[k] = x;
    }
}

// ---------------------------------------------------------------- CrossMLP ablation: AdaptiveAvgPool1d over tokens
// out[b, i, :] = mean over t in [floor(i T / bins), ceil((i+1) T / bins)) of cat(U[b], V[b])[t, :], T = Lu + Lv
// (encoder.py:396,503-506: nn.AdaptiveAvgPool1d(40) over the token axis of the concatenated user and video tokens;
// neighbouring bins overlap when T is not a multiple of bins).
__device__ __forceinline__ void pool_bin(int i, int T, int bins, int& t0, int& t1) {
    t0 = (int)(((long long)i * T) / bins);
    t1 = (int)((((long long)(i + 1)) * T + bins - 1) / bins);
}
__global__ __launch_bounds__(256) void pool_tokens_kernel(const float* __restrict__ U, int Lu, const float* __restrict__ V, int Lv,
                                                          float* __restrict__ out, int d, int bins) {
    const int b = blockIdx.x / bins, i = blockIdx.x % bins, T = Lu + Lv;
    int t0, t1;
    pool_bin(i, T, bins, t0, t1);
    for (int c = threadIdx.x * 4; c < d; c += blockDim.x * 4) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int t = t0; t < t1; ++t)
            acc += t < Lu ? *(const f32x4*)(U + ((size_t)b * Lu + t) * d + c) : *(const f32x4*)(V + ((size_t)b * Lv + (t - Lu)) * d + c);
        const float n = (float)(t1 - t0);
        *(f32x4*)(out + (size_t)blockIdx.x * d + c) = f32x4{acc.x / n, acc.y / n, acc.z / n, acc.w / n};
    }
}
// dU / dV[b, t, :] = sum over the bins i that contain t of dOut[b, i, :] / |bin i|   (fixed order: deterministic)
__global__ __launch_bounds__(256) void pool_tokens_bwd_kernel(const float* __restrict__ dOut, float* __restrict__ dU, int Lu,
                                                              float* __restrict__ dV, int Lv, int d, int bins) {
    const int T = Lu + Lv, b = blockIdx.x / T, t = blockIdx.x % T;
    float* dst = t < Lu ? dU + ((size_t)b * Lu + t) * d : dV + ((size_t)b * Lv + (t - Lu)) * d;
    for (int c = threadIdx.x * 4; c < d; c += blockDim.x * 4) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int i = 0; i < bins; ++i) {
            int t0, t1;
            pool_bin(i, T, bins, t0, t1);
            if (t >= t0 && t < t1) {
                const f32x4 g = *(const f32x4*)(dOut + ((size_t)b * bins + i) * d + c);
                const float n = (float)(t1 - t0);
                acc += f32x4{g.x / n, g.y / n, g.z / n, g.w / n};
            }
        }
        *(f32x4*)(dst + c) = acc;
    }
}

}  // namespace segmm
