// Device-resident logit store (include/segmm_hip.h: segmm_store_lookup / segmm_store_head / segmm_store_head_bwd state
// the index format, the reader rule and the row-index convention; tests/store_ref.py restates them in numpy).
#pragma once
#include "../../include/segmm_hip.h"
#include "common.h"

namespace segmm {

#ifndef SEGMM_STORE_HEAD_U
#define SEGMM_STORE_HEAD_U 4          // row groups a wave of the one-round head takes per trip (capi.hip sizes the grid by it)
#endif

// row of the value matrix for the key (a, b, c) in the sorted, unique index keys [n, 3], -1 when absent: lower bound by
// lexicographic signed comparison of the three 64-bit words, then one equality test
__device__ __forceinline__ int store_find(const long long* __restrict__ keys, const int* __restrict__ rows, long long n, long long a,
                                          long long b, long long c) {
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        const long long* k = keys + 3 * mid;
        const long long ka = k[0];
        bool less = ka < a;
        if (ka == a) {
            const long long kb = k[1];
            less = kb < b;
            if (kb == b) less = k[2] < c;
        }
        if (less) lo = mid + 1; else hi = mid;
    }
    if (lo < n) {
        const long long* k = keys + 3 * lo;
        if (k[0] == a && k[1] == b && k[2] == c) return rows[lo];
    }
    return -1;
}
// the reference's id2user / id2item step as a dense map; false: the id has no entry
__device__ __forceinline__ bool store_map(const long long* __restrict__ map, long long n_map, long long& id) {
    if (!map) return true;
    if (id < 0 || id >= n_map) return false;
    id = map[id];
    return id >= 0;
}

// One workgroup per query row b: thread 0 resolves the user and searches the target key once, the threads then share the items.
__global__ __launch_bounds__(256) void store_lookup_kernel(const long long* __restrict__ user, const long long* __restrict__ item,
                                                           const long long* __restrict__ time, int I, const long long* __restrict__ keys,
                                                           const int* __restrict__ rows, long long n, const long long* __restrict__ neg_keys,
                                                           const int* __restrict__ neg_rows, long long n_neg,
                                                           const long long* __restrict__ user_map, long long n_um,
                                                           const long long* __restrict__ item_map, long long n_im, int* __restrict__ rowidx,
                                                           long long* miss) {
    __shared__ int s_t;
    __shared__ long long s_u;
    const long long b = blockIdx.x;
    const long long base = b * I;
    const long long tm = time[b];
    if (threadIdx.x == 0) {
        long long u = user[b], it0 = item[base];
        const bool uok = store_map(user_map, n_um, u), iok = store_map(item_map, n_im, it0);
        if (!(uok && iok)) atomicMin(miss + 1, base);
        s_t = (uok && iok) ? store_find(keys, rows, n, u, it0, tm) : -1;
        s_u = u;
    }
    __syncthreads();
    const int t = s_t;
    const long long u = s_u;
    const bool own = n_neg >= 0 && I > 2 && t >= 0;          // the reference's len(item_ids) > 2: at I == 2 a negatives file is ignored
    for (int j = threadIdx.x; j < I; j += blockDim.x) {
        int v = t;
        if (j > 0 && (item_map || own)) {
            long long it = item[base + j];
            if (!store_map(item_map, n_im, it)) {
                atomicMin(miss + 1, base + j);
                v = -1;
            } else if (own) {
                const int r = store_find(neg_keys, neg_rows, n_neg, u, it, tm);
                if (r < 0) atomicMin(miss, base + j);
                v = r < 0 ? -1 : -2 - r;
            }
        }
        rowidx[base + j] = v;
    }
}

// ---------------------------------------------------------------- the head over the store's rows
// V floats of a row at p (V = 4: one 16-byte access; the host side picks V = 4 only when S % 4 == 0 and every base is aligned)
template <int V, bool NT>
__device__ __forceinline__ void store_ld(const float* p, float (&x)[V]) {
    if constexpr (V == 4) {
        f32x4 v;
        if constexpr (NT) v = __builtin_nontemporal_load((const f32x4*)p);
        else v = *(const f32x4*)p;
        x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
    } else {
        if constexpr (NT) x[0] = __builtin_nontemporal_load(p);
        else x[0] = *p;
    }
}
template <int V>
__device__ __forceinline__ void store_st(float* p, const float (&x)[V]) {
    if constexpr (V == 4) __builtin_nontemporal_store(f32x4{x[0], x[1], x[2], x[3]}, (f32x4*)p);
    else __builtin_nontemporal_store(x[0], p);
}
// where the weights of a (b, i) row come from
struct StoreW {
    const int* rowidx;                   // null: `weight` or ones
    const float* vals; long long m;      // rowidx r >= 0  -> vals[r]
    const float* neg; long long m_neg;   // rowidx r <= -2 -> neg[-2 - r]
    const float* weight;                 // explicit [rows, S] (backward only)
};
// the source row of the weights named by row index ri: null = a constant, ones or -- an index outside its value matrix -- NaN; no
// memory is touched then
__device__ __forceinline__ const float* store_wrow_of(const StoreW& w, int ri, int S, float& fill) {
    fill = 1.f;
    if (ri >= 0) {
        if (w.vals && (long long)ri < w.m) return w.vals + (size_t)ri * S;
        fill = __builtin_nanf("");
    } else if (ri <= -2) {
        const long long nr = -2ll - (long long)ri;
        if (w.neg && nr < w.m_neg) return w.neg + (size_t)nr * S;
        fill = __builtin_nanf("");
    }
    return nullptr;
}
__device__ __forceinline__ const float* store_wrow(const StoreW& w, long long r, int S, float& fill) {
    fill = 1.f;
    if (w.weight) return w.weight + (size_t)r * S;
    if (!w.rowidx) return nullptr;
    return store_wrow_of(w, w.rowidx[r], S, fill);
}

// G = 2^lg lanes share a row (64 / G rows per wave): lane g of the group takes the V-float chunks g, g + G, ... in order and adds their
// products in element order; the G partial sums then meet in a fixed xor tree.  The order depends on (S, V, G) only, so the sums are
// bit-identical from run to run.
// ONE: every row is a single round of chunks (S / V <= G).  A trip takes U row groups and issues their loads front to back -- row
// indices first; then, without a branch, the value rows they name (from cache), the durations and pred (nontemporal: read once)
// -- so that a wave keeps U value rows and U pred lines in flight together instead of one chain of three latencies.  Rows past the end read row
// `rows - 1` and write nothing.
template <int V>
__device__ __forceinline__ float store_head_chunk(const float* __restrict__ pred, const float* wsrc, float fill, long long dur, long long r,
                                                  int S, int c, float* __restrict__ weight_out) {
    const int s0 = c * V;
    float w[V], acc = 0.f;
    if (wsrc) store_ld<V, false>(wsrc + s0, w);
    else
        for (int k = 0; k < V; ++k) w[k] = fill;
    if (weight_out) store_st<V>(weight_out + (size_t)r * S + s0, w);
    if (pred) {
        float p[V];
        store_ld<V, true>(pred + (size_t)r * S + s0, p);
#pragma unroll
        for (int k = 0; k < V; ++k) acc += (p[k] * w[k]) * ((long long)(s0 + k) < dur ? 1.f : 0.f);
    }
    return acc;
}
template <int V, bool ONE>
__global__ __launch_bounds__(256) void store_head_kernel(const float* __restrict__ pred, StoreW w, const long long* __restrict__ duration,
                                                         long long rows, int S, int lg, float* __restrict__ out,
                                                         float* __restrict__ weight_out) {
    const int lane = threadIdx.x & 63, G = 1 << lg, g = lane & (G - 1), sub = lane >> lg, rpw = 64 >> lg, nch = S / V;
    constexpr int U = ONE ? SEGMM_STORE_HEAD_U : 1;
    const long long wave = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), step = (long long)gridDim.x * (blockDim.x >> 6) * rpw * U;
    for (long long r0 = wave * rpw * U; r0 < rows; r0 += step) {
        float acc[U];
        if constexpr (ONE) {
            const int s0 = (g < nch ? g : 0) * V;
            long long rc[U], dur[U];
            int ri[U];
            float p[U][V];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                rc[u] = min(r0 + u * rpw + sub, rows - 1);
                ri[u] = w.rowidx[rc[u]];
            }
            const float* wsrc[U];
            float fill[U], x[U][V];
#pragma unroll
            for (int u = 0; u < U; ++u) wsrc[u] = store_wrow_of(w, ri[u], S, fill[u]);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                // no branch around the load: a constant row reads its own pred (or weight_out) chunk -- memory the call owns -- and drops it
                const float* own = (pred ? pred : weight_out) + (size_t)rc[u] * S;
                store_ld<V, false>((wsrc[u] ? wsrc[u] : own) + s0, x[u]);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) dur[u] = duration ? duration[rc[u]] : (long long)S;
            if (pred) {
#pragma unroll
                for (int u = 0; u < U; ++u) store_ld<V, true>(pred + (size_t)rc[u] * S + s0, p[u]);
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int k = 0; k < V; ++k) x[u][k] = wsrc[u] ? x[u][k] : fill[u];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool live = r0 + u * rpw + sub < rows && g < nch;
                if (weight_out && live) store_st<V>(weight_out + (size_t)rc[u] * S + s0, x[u]);
                acc[u] = 0.f;
                if (pred) {
#pragma unroll
                    for (int k = 0; k < V; ++k) acc[u] += (p[u][k] * x[u][k]) * ((long long)(s0 + k) < dur[u] ? 1.f : 0.f);
                }
                if (!live) acc[u] = 0.f;
            }
        } else {
            const long long r = r0 + sub;
            acc[0] = 0.f;
            if (r < rows) {
                float fill;
                const float* wsrc = store_wrow(w, r, S, fill);
                const long long dur = duration ? duration[r] : (long long)S;
                for (int c = g; c < nch; c += G) acc[0] += store_head_chunk<V>(pred, wsrc, fill, dur, r, S, c, weight_out);
            }
        }
        if (out) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                float s = acc[u];
                for (int o = G >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o);
                const long long r = r0 + u * rpw + sub;
                if (g == 0 && r < rows) out[r] = s;
            }
        }
    }
}

// dpred[r, s] = (g[r] * w(r)[s]) * (s < duration[r]): one rounded product, then a multiplication by 0 or 1
template <int V>
__global__ __launch_bounds__(256) void store_head_bwd_kernel(const float* __restrict__ gout, StoreW w, const long long* __restrict__ duration,
                                                             long long rows, int S, int lg, float* __restrict__ dpred) {
    const int lane = threadIdx.x & 63, G = 1 << lg, g = lane & (G - 1), sub = lane >> lg, rpw = 64 >> lg, nch = S / V;
    const long long wave = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), step = (long long)gridDim.x * (blockDim.x >> 6) * rpw;
    for (long long r = wave * rpw + sub; r < rows; r += step) {
        float fill;
        const float* wsrc = store_wrow(w, r, S, fill);
        const long long dur = duration ? duration[r] : (long long)S;
        const float gr = gout[r];
        for (int c = g; c < nch; c += G) {
            const int s0 = c * V;
            float x[V];
            if (wsrc) store_ld<V, false>(wsrc + s0, x);
            else
                for (int k = 0; k < V; ++k) x[k] = fill;
#pragma unroll
            for (int k = 0; k < V; ++k) x[k] = (gr * x[k]) * ((long long)(s0 + k) < dur ? 1.f : 0.f);
            store_st<V>(dpred + (size_t)r * S + s0, x);
        }
    }
}

}  // namespace segmm
