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


// ---------------------------------------------------------------- the writer: one batch of the inference pass into the tables
// keys[row0 + r] = (user[r], photo[r], time[r]); vals[row0 + r, :] = logits[r * ld .. + S), bit copies.  The work items are flat:
// first the B * S / V value chunks (V = 4: one 16-byte access; the host picks it only when S % 4 == 0, ld % 4 == 0 and both bases
// are 16-byte aligned), then the 3 B key words.  The host has checked row0 + B <= capacity: `kdst` / `vdst` are the tables at row0.
typedef unsigned int u32x4s __attribute__((ext_vector_type(4)));
template <int V>
__global__ __launch_bounds__(256) void store_append_kernel(const long long* __restrict__ user, const long long* __restrict__ photo,
                                                           const long long* __restrict__ time, const unsigned* __restrict__ logits, int ld,
                                                           long long B, int S, long long* __restrict__ kdst, unsigned* __restrict__ vdst) {
    const int nch = S / V;
    const long long n_val = B * nch, total = n_val + 3 * B;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        if (i < n_val) {
            const long long r = i / nch;
            const int c = (int)(i - r * nch) * V;
            if constexpr (V == 4) *(u32x4s*)(vdst + r * S + c) = *(const u32x4s*)(logits + r * ld + c);
            else vdst[r * S + c] = logits[r * ld + c];
        } else {
            const long long w = i - n_val, r = w / 3;
            const int col = (int)(w - 3 * r);
            kdst[w] = (col == 0 ? user : col == 1 ? photo : time)[r];
        }
    }
}

// ---------------------------------------------------------------- the index of a store, built where the keys are
// include/segmm_hip.h: segmm_store_index.  The keys' rows are sorted as 4-word tuples (user, item, time, row) by a bitonic network of
// the shape of argsort_chunk_kernel / argsort_global_step_kernel (rowops.h), kept as four arrays in the caller's workspace:
// k0, k1, k2 (int64 [np2]) and row (int32 [np2]), np2 = the power of two >= max(n, STORE_SORT_CHUNK).  The order (three signed words,
// then the row) is total over the real tuples, so the result does not depend on the network.  A padding slot has row = -1 and compares
// above every real tuple by that test alone -- never by a key value: (INT64_MAX, INT64_MAX, INT64_MAX) is a legal key.
// Then: last-of-run flags counted per block (store_index_count_kernel), the block counts scanned by one workgroup
// (store_index_scan_kernel, which also writes n_unique), and the scatter of every run's last tuple to its rank
// (store_index_scatter_kernel).  No kernel waits for another workgroup.
constexpr int STORE_SORT_CHUNK = 2048;          // tuples a workgroup sorts / merges in LDS (28 bytes each: 56 KB)
constexpr int STORE_SCAN_BLOCK = 1024;          // tuples per workgroup of the count / scatter kernels (256 threads x 4 in a row)

struct StoreTuple { long long a, b, c; int row; };
// a sorts strictly above b
__device__ __forceinline__ bool store_tuple_above(const StoreTuple& x, const StoreTuple& y) {
    if (x.row < 0 || y.row < 0) return x.row < 0 && y.row >= 0;          // padding: above every real tuple, equal to other padding
    if (x.a != y.a) return x.a > y.a;
    if (x.b != y.b) return x.b > y.b;
    if (x.c != y.c) return x.c > y.c;
    return x.row > y.row;
}
struct StoreSortWs { long long *k0, *k1, *k2; int* row; };

__global__ __launch_bounds__(256) void store_index_init_kernel(const long long* __restrict__ keys, int n, int np2, StoreSortWs ws) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= np2) return;
    const bool real = i < n;
    ws.k0[i] = real ? keys[3 * (long long)i] : 0;
    ws.k1[i] = real ? keys[3 * (long long)i + 1] : 0;
    ws.k2[i] = real ? keys[3 * (long long)i + 2] : 0;
    ws.row[i] = real ? i : -1;
}
// one chunk per workgroup; kfirst == 2: the whole network up to k = STORE_SORT_CHUNK; kfirst > STORE_SORT_CHUNK: the strides
// j < STORE_SORT_CHUNK of stage k = kfirst.  Directions come from the global index.
__global__ __launch_bounds__(1024) void store_index_chunk_kernel(StoreSortWs ws, int kfirst) {
    constexpr int C = STORE_SORT_CHUNK;
    __shared__ long long s0[C], s1[C], s2[C];
    __shared__ int sr[C];
    const int base = blockIdx.x * C;
    for (int i = threadIdx.x; i < C; i += blockDim.x) {
        s0[i] = ws.k0[base + i]; s1[i] = ws.k1[base + i]; s2[i] = ws.k2[base + i]; sr[i] = ws.row[base + i];
    }
    __syncthreads();
    const int klast = kfirst == 2 ? C : kfirst;
    for (int k = kfirst; k <= klast; k <<= 1) {
        for (int j = (k > C ? C : k) >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < (C >> 1); t += blockDim.x) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int l = i | j;
                const bool up = ((base + i) & k) == 0;
                const StoreTuple x{s0[i], s1[i], s2[i], sr[i]}, y{s0[l], s1[l], s2[l], sr[l]};
                const bool swap = up ? store_tuple_above(x, y) : store_tuple_above(y, x);
                if (swap) {
                    s0[i] = y.a; s1[i] = y.b; s2[i] = y.c; sr[i] = y.row;
                    s0[l] = x.a; s1[l] = x.b; s2[l] = x.c; sr[l] = x.row;
                }
            }
            __syncthreads();
        }
        if (k >= C) break;
    }
    for (int i = threadIdx.x; i < C; i += blockDim.x) {
        ws.k0[base + i] = s0[i]; ws.k1[base + i] = s1[i]; ws.k2[base + i] = s2[i]; ws.row[base + i] = sr[i];
    }
}
__global__ __launch_bounds__(256) void store_index_global_step_kernel(StoreSortWs ws, int np2, int k, int j) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= (np2 >> 1)) return;
    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
    const int l = i | j;
    const bool up = (i & k) == 0;
    const StoreTuple x{ws.k0[i], ws.k1[i], ws.k2[i], ws.row[i]}, y{ws.k0[l], ws.k1[l], ws.k2[l], ws.row[l]};
    const bool swap = up ? store_tuple_above(x, y) : store_tuple_above(y, x);
    if (swap) {
        ws.k0[i] = y.a; ws.k1[i] = y.b; ws.k2[i] = y.c; ws.row[i] = y.row;
        ws.k0[l] = x.a; ws.k1[l] = x.b; ws.k2[l] = x.c; ws.row[l] = x.row;
    }
}
// 1 when sorted tuple i < n is the last of its run of equal keys (the tuple with the largest row of that key)
__device__ __forceinline__ int store_index_last(const StoreSortWs& ws, int i, int n) {
    if (i >= n) return 0;
    if (i == n - 1) return 1;
    return (ws.k0[i] != ws.k0[i + 1] || ws.k1[i] != ws.k1[i + 1] || ws.k2[i] != ws.k2[i + 1]) ? 1 : 0;
}
// flags of the workgroup's STORE_SCAN_BLOCK tuples (thread t: tuples 4 t .. 4 t + 3 of the block) and, in `excl`, the number of flags
// in front of the thread's first tuple inside the block; returns the block's total to every thread
__device__ __forceinline__ int store_index_block_scan(const StoreSortWs& ws, int n, int (&f)[4], int& excl) {
    __shared__ int s[256];
    const int first = blockIdx.x * STORE_SCAN_BLOCK + 4 * threadIdx.x;
    int mine = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) { f[u] = store_index_last(ws, first + u, n); mine += f[u]; }
    s[threadIdx.x] = mine;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const int v = threadIdx.x >= o ? s[threadIdx.x - o] : 0;
        __syncthreads();
        s[threadIdx.x] += v;
        __syncthreads();
    }
    excl = s[threadIdx.x] - mine;
    return s[255];
}
__global__ __launch_bounds__(256) void store_index_count_kernel(StoreSortWs ws, int n, int* __restrict__ sums) {
    int f[4], excl;
    const int total = store_index_block_scan(ws, n, f, excl);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}
// sums[0 .. nb) -> their exclusive scan in place, by ONE workgroup (rounds of 1024 with a running carry); n_unique = the total
__global__ __launch_bounds__(1024) void store_index_scan_kernel(int* __restrict__ sums, int nb, long long* __restrict__ n_unique) {
    __shared__ int s[1024];
    __shared__ int carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int b0 = 0; b0 < nb; b0 += 1024) {
        const int i = b0 + threadIdx.x;
        const int mine = i < nb ? sums[i] : 0;
        s[threadIdx.x] = mine;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {
            const int v = threadIdx.x >= o ? s[threadIdx.x - o] : 0;
            __syncthreads();
            s[threadIdx.x] += v;
            __syncthreads();
        }
        const int c = carry;
        if (i < nb) sums[i] = c + s[threadIdx.x] - mine;
        __syncthreads();
        if (threadIdx.x == 1023) carry = c + s[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) *n_unique = carry;
}
__global__ __launch_bounds__(256) void store_index_scatter_kernel(StoreSortWs ws, int n, const int* __restrict__ sums,
                                                                  long long* __restrict__ out_keys, int* __restrict__ out_rows) {
    int f[4], excl;
    store_index_block_scan(ws, n, f, excl);
    const int first = blockIdx.x * STORE_SCAN_BLOCK + 4 * threadIdx.x;
    long long pos = (long long)sums[blockIdx.x] + excl;          // < n: a flagged tuple's rank among the flagged ones
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        if (f[u]) {
            const int i = first + u;
            out_keys[3 * pos] = ws.k0[i]; out_keys[3 * pos + 1] = ws.k1[i]; out_keys[3 * pos + 2] = ws.k2[i];
            out_rows[pos] = ws.row[i];
            ++pos;
        }
    }
}

}  // namespace segmm
