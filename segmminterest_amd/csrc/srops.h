// Spatial-reduction attention (sr_ratio > 1, encoder.py:23-31,84-102): the strided Conv1d(d, d, r, stride = r, padding = (r-1)/2) that
// shortens the video-key sequence has kernel_size == stride, so its windows do not overlap and the conv is ONE GEMM over the
// windows laid side by side.  Two copy kernels do the laying:
//   sr_pack     A[b Ls + j, c r + t] = x[b, j r - p + t, c]   (0 outside [0, S)),  K index c r + t = the conv weight [d, d, r] as stored,
//               read as a row-major [d, r d] matrix;  + partial maxima of |A|;  + the pooled key mask m_sr[b, j] = OR_t m[b, j r + t]
//               (NOT shifted by p: max_pool1d(kernel = stride = r) of the reference);
//   sr_unpack   G[b, i, c] = res[b, i, c] + dA[b Ls + (i + p) / r, c r + (i + p) % r]   (rows in no window: res, or 0) -- one fp32 add
//               per element in a fixed order.
// A lane owns 4 channels of every tap of one window: r 16-byte accesses on the token side, r 16-byte accesses of the 4 r contiguous
// floats on the window side.  The tap count is a template parameter: the interleave is register renaming, no LDS, no scratch.
#pragma once
#include "common.h"

namespace segmm {

template <int R>
__global__ __launch_bounds__(256) void sr_pack_kernel(const float* __restrict__ x, long long ldx, const unsigned char* __restrict__ m,
                                                      float* __restrict__ A, unsigned char* __restrict__ m_sr, float* amax,
                                                      long long items, int S, int Ls, int d4) {
    constexpr int P = (R - 1) / 2;
    const long long it = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    float am = 0.f;
    if (it < items) {
        const int c4 = (int)(it % d4);
        const long long row = it / d4;          // b Ls + j
        const long long b = row / Ls;
        const int j = (int)(row % Ls);
        f32x4 v[R];
#pragma unroll
        for (int t = 0; t < R; ++t) {
            const int i = j * R - P + t;
            v[t] = (i >= 0 && i < S) ? *(const f32x4*)(x + (b * S + i) * ldx + c4 * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
            am = absmax4(am, v[t]);
        }
        float o[4 * R];
#pragma unroll
        for (int t = 0; t < R; ++t) {
            o[0 * R + t] = v[t].x; o[1 * R + t] = v[t].y; o[2 * R + t] = v[t].z; o[3 * R + t] = v[t].w;
        }
        float* dst = A + row * ((long long)d4 * 4 * R) + (long long)c4 * 4 * R;
#pragma unroll
        for (int q = 0; q < R; ++q) *(f32x4*)(dst + 4 * q) = f32x4{o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]};
        if (m_sr && c4 == 0) {
            unsigned char any = 0;
#pragma unroll
            for (int t = 0; t < R; ++t) any |= m[b * S + j * R + t];          // j R + t < Ls R <= S
            m_sr[row] = any ? 1 : 0;
        }
    }
    if (amax) amax_commit(amax, am, blockIdx.x * 4u + (threadIdx.x >> 6));          // every lane of the wave arrives here
}

// One lane per (b, window j <= Ls, 4 channels); the extra window j == Ls stands for the rows behind the last window.
template <int R>
__global__ __launch_bounds__(256) void sr_unpack_kernel(const float* __restrict__ dA, const float* __restrict__ res, float* __restrict__ G,
                                                        long long items, int S, int Ls, int d4) {
    constexpr int P = (R - 1) / 2;
    const long long it = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (it >= items) return;
    const int c4 = (int)(it % d4);
    const long long w = it / d4;          // b (Ls + 1) + j
    const long long b = w / (Ls + 1);
    const int j = (int)(w % (Ls + 1));
    const long long d = (long long)d4 * 4;
    if (j == Ls) {
        for (int i = Ls * R - P; i < S; ++i) {
            const long long o = (b * S + i) * d + c4 * 4;
            *(f32x4*)(G + o) = res ? *(const f32x4*)(res + o) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
        return;
    }
    const float* src = dA + (b * Ls + j) * (d * R) + (long long)c4 * 4 * R;
    float o[4 * R];
#pragma unroll
    for (int q = 0; q < R; ++q) {
        const f32x4 v = *(const f32x4*)(src + 4 * q);
        o[4 * q] = v.x; o[4 * q + 1] = v.y; o[4 * q + 2] = v.z; o[4 * q + 3] = v.w;
    }
#pragma unroll
    for (int t = 0; t < R; ++t) {
        const int i = j * R - P + t;
        if (i < 0) continue;          // the left zero pad of window 0 (i < S always: (Ls - 1) R - P + R - 1 < Ls R <= S)
        const long long off = (b * S + i) * d + c4 * 4;
        f32x4 g = f32x4{o[0 * R + t], o[1 * R + t], o[2 * R + t], o[3 * R + t]};
        if (res) {
            const f32x4 rr = *(const f32x4*)(res + off);
            g = f32x4{rr.x + g.x, rr.y + g.y, rr.z + g.z, rr.w + g.w};
        }
        *(f32x4*)(G + off) = g;
    }
}

}  // namespace segmm
