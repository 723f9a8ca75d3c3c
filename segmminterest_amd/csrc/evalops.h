// the callers on either side of the training step, as integer/byte kernels.
//
//  * on-device evaluation (my_evaluation.py:73-231, SegRec/main.py:101-117): the rank of the leave segment is an
//    INTEGER count ("how many positions sort before the target, ties by the lower index" -- what np.argsort gives),
//    AUC is the Mann-Whitney statistic as INTEGER pair counts (2*less + equal), so both are bit-exact against the
//    numpy/sklearn reference for the same float inputs; nothing here rounds.  The reference moves the whole dev set
//    to the host every 30 steps to do this with numpy.  valid_rows_kernel is the whole tail of a validation batch (interests, the
//    candidate shuffles, the rank) in one launch, for a pass that never waits for the host between batches.
//  * feature gather (dataloader_SegMM.py:271-362): per row up to S + Lt feature vectors picked from a resident
//    [n_lines, D] table by index, padded, L1-normalised (main...SegMM.py:272-273) and masked -- HBM-bound,
//    (S + Lt) * D * 4 bytes per row in, the same out, instead of a 573 KB/row host->device copy.
#pragma once
#include "common.h"

namespace segmm {

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---------------------------------------------------------------- leave-segment rank (TOP_K_leave / TOP_K_leave_mask)
// One wave per row.  gt in {1, 0, -1, -2} (watched, leave, unwatched, padding).  view_len = #(gt == 1).
//   plain  (my_evaluation.py:180-231): row valid iff view_len < seq_valid; candidates = all S positions as they are
//   masked (my_evaluation.py:137-178): row valid iff view_len != #(gt != -2); padded positions score 1.1
// perm (optional, [B, S] int32): pred[j] = x[perm[j]], target = position of view_len in perm (the reference shuffles
// the candidates with np.random; the host supplies the very same permutations, so ranks stay bit-exact).
// rank = 1 + #{j : pred[j] < pred[t]  or  (pred[j] == pred[t] and j < t)};  ranks[b] = 0 for invalid rows.
// hist[r] += 1 (integer atomics: order-independent) for r in 1..S; hist[0] counts invalid rows.
__global__ __launch_bounds__(256) void rank_leave_kernel(const float* __restrict__ x, int ldx, const long long* __restrict__ gt,
                                                         const int* __restrict__ perm, int B, int S, int masked,
                                                         int seq_valid, int* __restrict__ ranks, int* __restrict__ hist) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (b >= B) return;
    const long long* g = gt + (size_t)b * S;
    int vl = 0, dur = 0;
    for (int j = lane; j < S; j += 64) {
        const long long v = g[j];
        vl += v == 1;
        dur += v != -2;
    }
    vl = wave_sum_i(vl);
    dur = wave_sum_i(dur);
    const bool valid = masked ? (vl != dur) : (vl < seq_valid);
    int rank = 0;
    if (valid) {
        const float* xr = x + (size_t)b * ldx;
        const int* pr = perm ? perm + (size_t)b * S : nullptr;
        // target position t in candidate order
        int t = vl;
        if (pr) {
            int found = S;
            for (int j = lane; j < S; j += 64)
                if (pr[j] == vl) found = min(found, j);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) found = min(found, __shfl_xor(found, o, 64));
            t = min(found, S - 1);          // (a permutation always contains view_len; a malformed one must not index out of range)
        }
        const int ts = pr ? min(max(pr[t], 0), S - 1) : t;      // source index of the target
        float tv = xr[ts];
        if (masked && g[ts] == -2) tv = 1.1f;
        int cnt = 0;
        for (int j = lane; j < S; j += 64) {
            const int js = pr ? min(max(pr[j], 0), S - 1) : j;
            float v = xr[js];
            if (masked && g[js] == -2) v = 1.1f;
            cnt += (v < tv) || (v == tv && j < t);
        }
        rank = wave_sum_i(cnt) + 1;
    }
    if (lane == 0) {
        ranks[b] = rank;
        atomicAdd(hist + rank, 1);
    }
}

// ---------------------------------------------------------------- the tail of a validation batch in one launch
// (Trainer.valid_model: interests = sigmoid(logits) * exposure, the candidate shuffles of TOP_K_leave, the leave rank).  One wave
// per row, four rows per workgroup.  interest[b, s] = sigmoidf_(logits[b, s]) * exposure[s] in fp32 (the loss kernels' sigmoid);
// validity, the 1.1 fill of padded positions (masked), the target and the rank are rank_leave_kernel's, on those interests.
// R > 0 (permute, S <= 64 R <= 256): the row's candidate permutation is drawn here by perm_row_draw (common.h), keyed by
// (seed, site, row0 + b) -- a row draws the same permutation in whichever batch or slot it sits.  Lane l owns the source indices
// i = l, l + 64, ...; rank[r] is the candidate position j of index i (perm[j] = i), so the permuted row is never materialised: the
// target sits at the position of index view_len, every lane compares its own values at their positions.  R == 0: candidates as
// they are (j = i), any S.  interests [B, S] / perm_out [B, S] (the permutation used; the identity for R == 0) are optional.
__device__ __forceinline__ float valid_interest(float logit, float expo) { return sigmoidf_(logit) * expo; }
template <int R>
__global__ __launch_bounds__(256) void valid_rows_kernel(const float* __restrict__ logits, int ld, const float* __restrict__ exposure,
                                                         const long long* __restrict__ gt, int B, int S, int masked, int seq_valid,
                                                         DropCfg d0, long long row0, int* __restrict__ ranks,
                                                         float* __restrict__ interests, int* __restrict__ perm_out) {
    constexpr int RR = R > 0 ? R : 1;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int b = blockIdx.x * 4 + w;
    int pos[RR];
    if constexpr (R > 0) {
        __shared__ uint32_t keys[4][64 * RR];
        perm_row_draw<RR>(drop_live(d0), (uint64_t)(row0 + b), S, lane, keys[w], b < B, pos);
    }
    if (b >= B) return;
    const long long* g = gt + (size_t)b * S;
    const float* xr = logits + (size_t)b * ld;
    int vl = 0, dur = 0;
    for (int i = lane; i < S; i += 64) {
        const long long v = g[i];
        vl += v == 1;
        dur += v != -2;
    }
    vl = wave_sum_i(vl);
    dur = wave_sum_i(dur);
    const bool valid = masked ? (vl != dur) : (vl < seq_valid);
    const int ts = min(vl, S - 1);          // source index of the target (a valid row has view_len < S)
    float tv = valid_interest(xr[ts], exposure[ts]);
    if (masked && g[ts] == -2) tv = 1.1f;
    int t = ts;                             // ... and its candidate position
    if constexpr (R > 0) {
        int mine = 0;
#pragma unroll
        for (int r = 0; r < RR; ++r)
            if (r == (ts >> 6)) mine = pos[r];
        t = __shfl(mine, ts & 63, 64);
    }
    int cnt = 0;
    float* ir = interests ? interests + (size_t)b * S : nullptr;
    int* pr = perm_out ? perm_out + (size_t)b * S : nullptr;
    if constexpr (R > 0) {
#pragma unroll
        for (int r = 0; r < RR; ++r) {
            const int i = r * 64 + lane;
            if (i < S) {
                float v = valid_interest(xr[i], exposure[i]);
                if (ir) ir[i] = v;
                if (masked && g[i] == -2) v = 1.1f;
                const int j = pos[r];          // < S: only indices < S were counted
                if (pr) pr[j] = i;
                cnt += (v < tv) || (v == tv && j < t);
            }
        }
    } else {
        for (int i = lane; i < S; i += 64) {
            float v = valid_interest(xr[i], exposure[i]);
            if (ir) ir[i] = v;
            if (masked && g[i] == -2) v = 1.1f;
            if (pr) pr[i] = i;
            cnt += (v < tv) || (v == tv && i < t);
        }
    }
    cnt = wave_sum_i(cnt);
    if (lane == 0) ranks[b] = valid ? cnt + 1 : 0;
}

// ---------------------------------------------------------------- AUC as integer pair counts, per segment
// seg_off[s] .. seg_off[s+1]: elements of segment s (a user for wuAUC; one segment = the batch for ProbAUC).
// label: 1 positive, 0 negative, anything else ignored (padding cells).  out[s] = {U2, npos, nneg} with
// U2 = sum over positives of (2 * #negatives below + #negatives equal)  =>  AUC = U2 / (2 npos nneg), exactly the
// midrank Mann-Whitney value sklearn.roc_auc_score computes.  One workgroup per segment; every thread owns a strided
// set of positives and streams the segment's negatives through LDS.
__global__ __launch_bounds__(256) void auc_counts_kernel(const float* __restrict__ score, const signed char* __restrict__ label,
                                                         const long long* __restrict__ seg_off, long long* __restrict__ out) {
    __shared__ float tile[1024];
    __shared__ unsigned long long red[3][4];
    const long long a = seg_off[blockIdx.x], e = seg_off[blockIdx.x + 1];
    unsigned long long u2 = 0, npos = 0, nneg = 0;
    for (long long base = a; base < e; base += 1024) {             // negatives of this chunk -> LDS (+inf marks "not a negative")
        const int n = (int)min((long long)1024, e - base);
        __syncthreads();
        for (int i = threadIdx.x; i < 1024; i += 256) {
            float v = INFINITY;
            if (i < n && label[base + i] == 0) { v = score[base + i]; ++nneg; }
            tile[i] = v;
        }
        __syncthreads();
        for (long long p = a + threadIdx.x; p < e; p += 256) {     // every positive of the segment against the chunk
            if (label[p] != 1) continue;
            const float sp = score[p];
            unsigned int less = 0, eq = 0;
            for (int i = 0; i < n; ++i) {
                const float v = tile[i];
                less += v < sp;
                eq += v == sp;
            }
            u2 += 2ull * less + eq;
        }
    }
    for (long long p = a + threadIdx.x; p < e; p += 256) npos += label[p] == 1;
    // integer reductions: exact
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long v[3] = {u2, npos, nneg};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
        if (lane == 0) red[k][wave] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < 3) out[(size_t)blockIdx.x * 3 + threadIdx.x] = (long long)(red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3]);
}

// survival[b, s] = exp(sum_{j <= s} log interest[b, j]) (main_eval_batch, my_evaluation.py:270: the running sum is the
// sequential fp32 cumsum) and the AUC label of the cell: 1 watched, 0 leave/unwatched, -1 (ignored) padding.
__global__ __launch_bounds__(256) void survival_kernel(const float* __restrict__ interest, int ld, const long long* __restrict__ gt,
                                                       float* __restrict__ surv, signed char* __restrict__ label, int B, int S) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    float h = 0.f;
    for (int s = 0; s < S; ++s) {
        h += logf(interest[(size_t)b * ld + s]);
        surv[(size_t)b * S + s] = expf(h);
        const long long g = gt[(size_t)b * S + s];
        label[(size_t)b * S + s] = g == -2 ? (signed char)-1 : (g == 1 ? (signed char)1 : (signed char)0);
    }
}

// ---------------------------------------------------------------- per-row metrics of the test phase (main_eval_batch,
// my_evaluation.py:249-266: JaccardSim / LeaveMSE / LeaveCTR / LeaveCTR_view, the argmin of TOP_K_leave(test=1), --eval_cold)
// One thread per row, like survival_kernel and with ITS recurrence (h += logf(x); surv = expf(h), in position order), so that
// surv is bit-identical to segmm_survival; the whole input is a few hundred KB, the kernel is bound by latency.  Records are
// stored field-major: irec [RM_NI, B] = view_length, duration, top1, group; frec [RM_NF, B] = jaccard, pred_view_length,
// leave_ctr, leave_ctr_view.
//   view_length = #(gt == 1), duration = #(gt != -2), top1 = argmin interest (lowest index on ties: np.argmin)
//   group = 1 (cold) iff photo_id is outside [0, n_seen) or seen[photo_id] == 0; 0 (hot) otherwise and without a table
//   jaccard = (sum_{t < view_length} (1 - |gt[t] - surv[t]|) + (duration - view_length)) / duration   (IoU_Sim "length_aware";
//             NaN for duration == 0), pred_view_length = sum_{gt[t] != -2} surv[t]   (predict_view_length)
//   leave_ctr = 1 - interest[k], leave_ctr_view = 1 - surv[k], k = view_length - 1, or S - 1 for view_length == 0 (the
//             reference indexes [-1] there)
// The terms are fp32 like the host's; their sums run in double (the host sums the .tolist() of the terms in Python floats).
constexpr int RM_NI = 4, RM_NF = 4;
__global__ __launch_bounds__(256) void row_metrics_kernel(const float* __restrict__ interest, int ld, const long long* __restrict__ gt,
                                                          const long long* __restrict__ photo_id, const unsigned char* __restrict__ seen,
                                                          long long n_seen, int B, int S, int* __restrict__ irec, float* __restrict__ frec) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const long long* g = gt + (size_t)b * S;
    const float* x = interest + (size_t)b * ld;
    int vl = 0, dur = 0;
    for (int s = 0; s < S; ++s) {
        const long long v = g[s];
        vl += v == 1;
        dur += v != -2;
    }
    const int k = vl > 0 ? vl - 1 : S - 1;
    float h = 0.f, best = x[0], xk = 0.f, sk = 0.f;
    int top1 = 0;
    double jac = 0.0, pred = 0.0;
    for (int s = 0; s < S; ++s) {
        const float xi = x[s];
        h += logf(xi);
        const float surv = expf(h);
        const long long v = g[s];
        if (xi < best) { best = xi; top1 = s; }
        if (s < vl) jac += (double)(1.f - fabsf((float)v - surv));
        if (v != -2) pred += (double)surv;
        if (s == k) { xk = xi; sk = surv; }
    }
    int group = 0;
    if (seen) {
        const long long p = photo_id[b];
        group = (p < 0 || p >= n_seen || seen[p] == 0) ? 1 : 0;
    }
    irec[b] = vl;
    irec[(size_t)B + b] = dur;
    irec[2 * (size_t)B + b] = top1;
    irec[3 * (size_t)B + b] = group;
    frec[b] = (float)((jac + (double)(dur - vl)) / (double)dur);
    frec[(size_t)B + b] = (float)pred;
    frec[2 * (size_t)B + b] = 1.f - xk;
    frec[3 * (size_t)B + b] = 1.f - sk;
}

// acc [3, RM_F] double (caller-owned; groups: all rows, cold rows, hot rows) += the sums of a batch's records:
//   n, jaccard, pred, (pred - vl)^2, |pred - vl|, leave_ctr, leave_ctr_view, (top1 - vl)^2, |top1 - vl|, #(vl == duration).
// Deterministic: ONE workgroup, every thread sums a fixed strided set of rows in row order, a fixed-order tree in LDS, one
// thread reads, adds and writes the accumulator (no floating-point atomics); batches are serialised by stream order.
constexpr int RM_F = 10;
__global__ __launch_bounds__(256) void row_metrics_accumulate_kernel(const int* __restrict__ irec, const float* __restrict__ frec, int B,
                                                                     double* acc) {
    __shared__ double sm[RM_F][256];
    const int tid = threadIdx.x;
    for (int grp = 0; grp < 3; ++grp) {
        double a[RM_F];
#pragma unroll
        for (int f = 0; f < RM_F; ++f) a[f] = 0.0;
        for (int b = tid; b < B; b += 256) {
            const bool cold = irec[3 * (size_t)B + b] != 0;
            if (grp != 0 && (grp == 1) != cold) continue;
            const int vl = irec[b], dur = irec[(size_t)B + b], top1 = irec[2 * (size_t)B + b];
            const double pred = (double)frec[(size_t)B + b];
            const double dp = pred - (double)vl, dt = (double)(top1 - vl);
            a[0] += 1.0;
            a[1] += (double)frec[b];
            a[2] += pred;
            a[3] += dp * dp;
            a[4] += fabs(dp);
            a[5] += (double)frec[2 * (size_t)B + b];
            a[6] += (double)frec[3 * (size_t)B + b];
            a[7] += dt * dt;
            a[8] += fabs(dt);
            a[9] += vl == dur ? 1.0 : 0.0;
        }
        __syncthreads();          // (the previous group's sums have been read)
#pragma unroll
        for (int f = 0; f < RM_F; ++f) sm[f][tid] = a[f];
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (tid < o) {
#pragma unroll
                for (int f = 0; f < RM_F; ++f) sm[f][tid] += sm[f][tid + o];
            }
            __syncthreads();
        }
        if (tid == 0) {
            for (int f = 0; f < RM_F; ++f) acc[grp * RM_F + f] += sm[f][0];
        }
    }
}

// ---------------------------------------------------------------- resident-table feature gather (+ pad, mask, L1 norm)
// out[r, :] = table[idx[r], :] / (sum|table[idx[r], :]| + 1e-6) for idx[r] in [0, n_lines), zeros and mask 0 otherwise
// (negative index = padding slot of the collator, dataloader_SegMM.py:345-350).  One wave per output row.
__global__ __launch_bounds__(256) void gather_l1_kernel(const float* __restrict__ table, long long n_lines, int D,
                                                        const long long* __restrict__ idx, long long rows, int normalize,
                                                        float* __restrict__ out, unsigned char* __restrict__ mask, float* amax,
                                                        PlaneOut po) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (r >= rows) return;
    const long long i = idx[r];
    const bool ok = i >= 0 && i < n_lines;
    if (mask && lane == 0) mask[r] = ok ? 1 : 0;
    float* o = out + r * D;
    const float ps = plane_scale(po);
    if (!ok) {
        for (int c = lane * 4; c < D; c += 256) {
            *(f32x4*)(o + c) = f32x4{0.f, 0.f, 0.f, 0.f};
            if (ps > 0.f) plane_store4_pair(po.p, po.ld2, r, c, f32x4{0.f, 0.f, 0.f, 0.f}, ps);
        }
        plane_finish(po, amax, 0.f, (unsigned)r, ps, r == 0 && lane == 0);
        return;
    }
    const float* t = table + i * D;
    float s = 0.f;
    if (normalize) {
        for (int c = lane * 4; c < D; c += 256) {
            const f32x4 v = *(const f32x4*)(t + c);
            s += fabsf(v.x) + fabsf(v.y) + fabsf(v.z) + fabsf(v.w);
        }
        s = wave_sum(s) + 1e-6f;
    }
    float am = 0.f;
    for (int c = lane * 4; c < D; c += 256) {
        f32x4 v = *(const f32x4*)(t + c);
        if (normalize) { v.x /= s; v.y /= s; v.z /= s; v.w /= s; }
        *(f32x4*)(o + c) = v;
        if (ps > 0.f) plane_store4_pair(po.p, po.ld2, r, c, v, ps);
        am = absmax4(am, v);
    }
    plane_finish(po, amax, am, (unsigned)r, ps, r == 0 && lane == 0);
}

// The same for a table of 16-bit elements (ELEM: IEEE half or bfloat16, common.h widen4): half the table bytes per row.  Every
// element is widened to fp32 exactly, then the arithmetic above (columns per lane, summation order, wave reduction, true division,
// plane calls): the result is gather_l1_kernel's on the widened table, bit for bit.  V > 0: the row's raw words stay in registers
// between the sum and the divide (2 VGPRs per 4 elements, D <= 256 V <= 2048), one read of the table row; V == 0: two passes.
// Table rows are 8-byte aligned only (D % 4 == 0): 8-byte loads.
template <int ELEM, int V>
__global__ __launch_bounds__(256) void gather_l1_h_kernel(const uint16_t* __restrict__ table, long long n_lines, int D,
                                                          const long long* __restrict__ idx, long long rows, int normalize,
                                                          float* __restrict__ out, unsigned char* __restrict__ mask, float* amax,
                                                          PlaneOut po) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (r >= rows) return;
    const long long i = idx[r];
    const bool ok = i >= 0 && i < n_lines;
    if (mask && lane == 0) mask[r] = ok ? 1 : 0;
    float* o = out + r * D;
    const float ps = plane_scale(po);
    if (!ok) {
        for (int c = lane * 4; c < D; c += 256) {
            *(f32x4*)(o + c) = f32x4{0.f, 0.f, 0.f, 0.f};
            if (ps > 0.f) plane_store4_pair(po.p, po.ld2, r, c, f32x4{0.f, 0.f, 0.f, 0.f}, ps);
        }
        plane_finish(po, amax, 0.f, (unsigned)r, ps, r == 0 && lane == 0);
        return;
    }
    const uint16_t* t = table + i * D;
    float s = 0.f, am = 0.f;
    if constexpr (V > 0) {
        uint32_t ra[V], rb[V];
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const int c = lane * 4 + k * 256;
            ra[k] = rb[k] = 0u;
            if (c < D) {
                const u32x2 w = ld_row4h(t + c);
                ra[k] = w.x; rb[k] = w.y;
                const f32x4 v = widen4<ELEM>(ra[k], rb[k]);
                s += fabsf(v.x) + fabsf(v.y) + fabsf(v.z) + fabsf(v.w);
            }
        }
        if (normalize) s = wave_sum(s) + 1e-6f;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const int c = lane * 4 + k * 256;
            if (c < D) {
                f32x4 v = widen4<ELEM>(ra[k], rb[k]);
                if (normalize) { v.x /= s; v.y /= s; v.z /= s; v.w /= s; }
                *(f32x4*)(o + c) = v;
                if (ps > 0.f) plane_store4_pair(po.p, po.ld2, r, c, v, ps);
                am = absmax4(am, v);
            }
        }
    } else {
        if (normalize) {
            for (int c = lane * 4; c < D; c += 256) {
                const f32x4 v = widen4<ELEM>(ld_row4h(t + c));
                s += fabsf(v.x) + fabsf(v.y) + fabsf(v.z) + fabsf(v.w);
            }
            s = wave_sum(s) + 1e-6f;
        }
        for (int c = lane * 4; c < D; c += 256) {
            f32x4 v = widen4<ELEM>(ld_row4h(t + c));
            if (normalize) { v.x /= s; v.y /= s; v.z /= s; v.w /= s; }
            *(f32x4*)(o + c) = v;
            if (ps > 0.f) plane_store4_pair(po.p, po.ld2, r, c, v, ps);
            am = absmax4(am, v);
        }
    }
    plane_finish(po, amax, am, (unsigned)r, ps, r == 0 && lane == 0);
}

// The same for a table of 8-bit elements (ELEM: OCP e4m3fn, e5m2 or int8, common.h widen4 of one dword): a quarter of the float32
// table's bytes per row.  Widened exactly, then gather_l1_kernel's arithmetic: its result on the widened table, bit for bit, with
// either ``normalize``.  V > 0: the raw dwords stay in registers between the sum and the divide (1 VGPR per 4 elements, D <= 256 V <=
// 2048); V == 0: two passes.  Table rows are 4-byte aligned only (D % 4 == 0): 4-byte loads.
template <int ELEM, int V>
__global__ __launch_bounds__(256) void gather_l1_b_kernel(const uint8_t* __restrict__ table, long long n_lines, int D,
                                                          const long long* __restrict__ idx, long long rows, int normalize,
                                                          float* __restrict__ out, unsigned char* __restrict__ mask, float* amax,
                                                          PlaneOut po) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (r >= rows) return;
    const long long i = idx[r];
    const bool ok = i >= 0 && i < n_lines;
    if (mask && lane == 0) mask[r] = ok ? 1 : 0;
    float* o = out + r * D;
    const float ps = plane_scale(po);
    if (!ok) {
        for (int c = lane * 4; c < D; c += 256) {
            *(f32x4*)(o + c) = f32x4{0.f, 0.f, 0.f, 0.f};
            if (ps > 0.f) plane_store4_pair(po.p, po.ld2, r, c, f32x4{0.f, 0.f, 0.f, 0.f}, ps);
        }
        plane_finish(po, amax, 0.f, (unsigned)r, ps, r == 0 && lane == 0);
        return;
    }
    const uint8_t* t = table + i * D;
    float s = 0.f, am = 0.f;
    if constexpr (V > 0) {
        uint32_t rw[V];
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const int c = lane * 4 + k * 256;
            rw[k] = 0u;
            if (c < D) {
                rw[k] = ld_row4q(t + c);
                const f32x4 v = widen4<ELEM>(rw[k]);
                s += fabsf(v.x) + fabsf(v.y) + fabsf(v.z) + fabsf(v.w);
            }
        }
        if (normalize) s = wave_sum(s) + 1e-6f;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const int c = lane * 4 + k * 256;
            if (c < D) {
                f32x4 v = widen4<ELEM>(rw[k]);
                if (normalize) { v.x /= s; v.y /= s; v.z /= s; v.w /= s; }
                *(f32x4*)(o + c) = v;
                if (ps > 0.f) plane_store4_pair(po.p, po.ld2, r, c, v, ps);
                am = absmax4(am, v);
            }
        }
    } else {
        if (normalize) {
            for (int c = lane * 4; c < D; c += 256) {
                const f32x4 v = widen4<ELEM>(ld_row4q(t + c));
                s += fabsf(v.x) + fabsf(v.y) + fabsf(v.z) + fabsf(v.w);
            }
            s = wave_sum(s) + 1e-6f;
        }
        for (int c = lane * 4; c < D; c += 256) {
            f32x4 v = widen4<ELEM>(ld_row4q(t + c));
            if (normalize) { v.x /= s; v.y /= s; v.z /= s; v.w /= s; }
            *(f32x4*)(o + c) = v;
            if (ps > 0.f) plane_store4_pair(po.p, po.ld2, r, c, v, ps);
            am = absmax4(am, v);
        }
    }
    plane_finish(po, amax, am, (unsigned)r, ps, r == 0 && lane == 0);
}

// ---------------------------------------------------------------- delayed scaling: end-of-pass update of the site scales
// arena: n_rows site headers of the pass that just ended; site_idx[r] = index of row r's tensor site in site_scale (< 0:
// none).  For every row that was produced (max > 0): site_scale[idx] = the power of two s with max * s in
// [2^(target-1), 2^target) -- the scale the NEXT pass writes this site's planes with (fp16 tops out at 2^16: target 12
// leaves head-room for step-to-step growth AND shrinkage; a tensor that leaves the window is refused by the consumers, which
// take their fp32 path).  stats[0] += rows whose planes were outside the window (diagnostics / tests).
// gain != null (the BACKWARD pass): also gain[idx] = max|x| / gmax[0], the site's size relative to the largest d loss / d logits
// of the step it was measured in -- every backward tensor is linear in d loss / d logits, so the next step predicts its maximum
// as gain * (that step's gmax) (loss_finish_kernel) instead of assuming it repeats.
__global__ __launch_bounds__(256) void scales_update_kernel(const float* __restrict__ arena, const int* __restrict__ site_idx, int n_rows,
                                                            float* site_scale, float* stats, int target, float* gain, const float* gmax) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (r >= n_rows) return;
    const int idx = site_idx[r];
    if (idx < 0) return;
    const float* hdr = arena + (size_t)r * SITE_FLOATS;
    float m = 0.f;
    for (int i = lane; i < AMAX_SLOTS; i += 64) m = fmaxf(m, hdr[SITE_HDR + i]);
    m = wave_max(m);
    if (lane == 0) {
        const uint32_t u = __float_as_uint(m);
        if (m > 0.f && (u >> 23) != 0xff) {
            int se = (target - 1) - ((int)(u >> 23) - 127);
            se = max(-60, min(60, se));
            site_scale[idx] = __uint_as_float((uint32_t)(se + 127) << 23);
            if (gain) gain[idx] = gmax[0] > 0.f ? m / gmax[0] : 0.f;
        }
        // tensors whose planes the consumers had to refuse: overflow flag up, or the maximum below the window (site_planes_ok)
        const float s_used = hdr[0];
        if (__float_as_uint(hdr[1]) != 0u || (s_used > 0.f && s_used < 0x1p60f && m > 0.f && m * s_used < 0.25f)) atomicAdd(stats, 1.0f);
    }
}

// ---------------------------------------------------------------- SegRec weighted head (ClipRec.forward, ClipRec.py:134-198)
// out[b, i] = sum_seg pred[b, i, seg] * weight[b, i, seg] * (seg < duration[b, i]): the per-segment interest logits
// written by the inference script re-enter the recommender as segment weights ('c_interest_weight',
// SegRec/models/BaseModel.py:262-408; weight == null = all ones, duration == null = no duration mask).
// One wave per (b, i).
__global__ __launch_bounds__(256) void segment_weighted_sum_kernel(const float* __restrict__ pred, const float* __restrict__ weight,
                                                                   const long long* __restrict__ duration, long long rows, int S,
                                                                   float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (r >= rows) return;
    const long long dur = duration ? duration[r] : (long long)S;
    float s = 0.f;
    for (int j = lane; j < S; j += 64) {
        const float m = j < dur ? 1.f : 0.f;
        s += pred[r * S + j] * (weight ? weight[r * S + j] : 1.f) * m;
    }
    s = wave_sum(s);
    if (lane == 0) out[r] = s;
}

}  // namespace segmm
