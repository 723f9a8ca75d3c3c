// Index batches from a compiled interaction table (include/segmm_hip.h: segmm_assemble_rows states the table, the candidate
// lists and the draw rule; tests/assemble_ref.py restates them in numpy).
#pragma once
#include "../../include/segmm_hip.h"
#include "common.h"

namespace segmm {

// LDS traffic of ONE wave with itself: DS instructions of a wave complete in order, so a compiler fence is all that is needed
// between the lanes' writes and the other lanes' reads (the waves of a workgroup take different paths: no __syncthreads here)
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ uint32_t assemble_key(const DropCfg& d, long long r, uint32_t stream, uint32_t j) {
    return drop_rand_quad(d, ((uint64_t)r << 13) | ((uint64_t)stream << 12) | (uint64_t)j).y;
}
// keys[0 .. count) of the row's list (count <= C), padded to a multiple of 4 with the largest key, which never counts
__device__ __forceinline__ void assemble_draw_keys(uint32_t* keys, int count, const DropCfg& d, long long r, uint32_t stream, int lane) {
    for (int j = lane; j < ((count + 3) & ~3); j += 64) keys[j] = j < count ? assemble_key(d, r, stream, (uint32_t)j) : 0xFFFFFFFFu;
}
// rank by counting, as rand_perm_rows_kernel does: lane l owns candidates l, l + 64, ... and counts the (key, index) pairs below
// each (four broadcast keys per LDS read); the candidates of rank < cap are the draw, emit(rank, j) places them
template <class F>
__device__ __forceinline__ void assemble_ranked(const uint32_t* keys, int count, int cap, int lane, F emit) {
    for (int c0 = 0; c0 < count; c0 += 64) {
        const int j = c0 + lane;
        const uint32_t k = j < count ? keys[j] : 0u;
        int rank = 0;
        for (int i = 0; i < count; i += 4) {
            const uint4 q = *(const uint4*)(keys + i);
            rank += (q.x < k || (q.x == k && i < j)) ? 1 : 0;
            rank += (q.y < k || (q.y == k && i + 1 < j)) ? 1 : 0;
            rank += (q.z < k || (q.z == k && i + 2 < j)) ? 1 : 0;
            rank += (q.w < k || (q.w == k && i + 3 < j)) ? 1 : 0;
        }
        if (j < count && rank < cap) emit(rank, j);
    }
}

// One wave per batch slot, W slots per workgroup; C = candidates a row's LDS (keys + lines) holds.
template <int C, int W>
__global__ __launch_bounds__(64 * W) void assemble_rows_kernel(segmm_itable_t t, const long long* __restrict__ row_ids, int B, int S, int Lt,
                                                               DropCfg d, long long* __restrict__ photo_idx, long long* __restrict__ user_idx,
                                                               long long* __restrict__ label, long long* __restrict__ cols) {
    __shared__ __attribute__((aligned(16))) uint32_t s_keys[W][C];
    __shared__ int s_lines[W][C];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, b = blockIdx.x * W + w;
    if (b >= B) return;
    uint32_t* keys = s_keys[w];
    int* lines = s_lines[w];
    long long* po = photo_idx + (size_t)b * S;
    long long* uo = user_idx + (size_t)b * Lt;
    long long* lo = label + (size_t)b * S;
    const long long r = row_ids[b];
    bool bad = r < 0 || r >= (long long)t.n_rows;

    // ---- the row's video: n frames of item v, a contiguous run of item_line without holes
    long long vs = 0;
    int n = 0, user = -1;
    if (!bad) {
        const int4 info = *(const int4*)(t.row_info + 4 * r);
        user = info.z;
        if (info.x >= 0 && info.x < t.n_items) {
            vs = t.item_ptr[info.x];
            n = (int)min((long long)max(info.y, 0), (long long)t.item_ptr[info.x + 1] - vs);
        }
        bad = n > C;
    }
    // ---- the user's candidates into LDS: history items in order (holes skipped), then the own lines; m counts them all
    int m = 0;
    if (!bad) {
        const long long h0 = t.hist_ptr[r], h1 = t.hist_ptr[r + 1];
        for (long long hb = h0; hb < h1; hb += 64) {
            // lane i resolves pair hb + i: where its item's lines start and how many of them were watched
            const long long h = hb + lane;
            uint32_t st_lo = 0, st_hi = 0;
            int cnt = 0;
            if (h < h1) {
                const int item = t.hist_pair[2 * h], nf = t.hist_pair[2 * h + 1];
                if (item >= 0 && item < t.n_items) {
                    const long long st = t.item_ptr[item];
                    cnt = (int)min((long long)max(nf, 0), (long long)t.item_ptr[item + 1] - st);
                    st_lo = (uint32_t)st;
                    st_hi = (uint32_t)((unsigned long long)st >> 32);
                }
            }
            const int nh = (int)min(64ll, h1 - hb);
            for (int i = 0; i < nh; ++i) {
                const int c_i = __builtin_amdgcn_readlane(cnt, i);
                const long long s_i = (long long)(((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)st_hi, i) << 32) |
                                                  (uint32_t)__builtin_amdgcn_readlane((int)st_lo, i));
                for (int f0 = 0; f0 < c_i; f0 += 64) {
                    const int f = f0 + lane;
                    const int line = f < c_i ? t.item_line[s_i + f] : -1;
                    const bool ok = line >= 0;
                    const unsigned long long bal = __ballot(ok);
                    const int pos = m + __popcll(bal & ((1ull << lane) - 1ull));
                    if (ok && pos < C) lines[pos] = line;
                    m += __popcll(bal);
                    if (m > C) break;
                }
                if (m > C) break;
            }
            if (m > C) break;
        }
        if (m <= C && user >= 0 && user < t.n_users) {
            const long long o0 = t.own_ptr[user];
            const long long no = t.own_ptr[user + 1] - o0;
            if (no > (long long)(C - m)) {
                m = C + 1;
            } else {
                for (int f = lane; f < (int)no; f += 64) lines[m + f] = t.own_line[o0 + f];
                m += (int)no;
            }
        }
        bad = m > C;
    }
    if (bad) {
        for (int p = lane; p < S; p += 64) { po[p] = -1; lo[p] = -2; }
        for (int p = lane; p < Lt; p += 64) uo[p] = -1;
        if (lane < 7) cols[(size_t)lane * B + b] = 0;
        return;
    }
    wave_lds_sync();
    // ---- user list
    if (m <= Lt) {
        for (int p = lane; p < Lt; p += 64) uo[p] = p < m ? (long long)lines[p] : -1ll;
    } else {
        assemble_draw_keys(keys, m, d, r, 1u, lane);
        wave_lds_sync();
        assemble_ranked(keys, m, Lt, lane, [&](int rank, int j) { uo[rank] = (long long)lines[j]; });
        wave_lds_sync();
    }
    // ---- video list
    const int* vl = t.item_line + vs;
    if (n <= S) {
        for (int p = lane; p < S; p += 64) po[p] = p < n ? (long long)vl[p] : -1ll;
    } else {
        assemble_draw_keys(keys, n, d, r, 0u, lane);
        wave_lds_sync();
        assemble_ranked(keys, n, S, lane, [&](int rank, int j) { po[rank] = (long long)vl[j]; });
    }
    const signed char* lab = (const signed char*)t.label + (size_t)r * S;
    for (int p = lane; p < S; p += 64) lo[p] = (long long)lab[p];
    if (lane < 7) cols[(size_t)lane * B + b] = t.row_cols[r * 7 + lane];
}

}  // namespace segmm
