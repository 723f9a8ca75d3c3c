// Shared device helpers for the gfx950 (CDNA4, wave64) kernels of the segment-interest path.
#pragma once
#ifndef SEGMM_NT_STORES
#define SEGMM_NT_STORES 0          // 1: streaming (nontemporal) stores for the big write-once outputs
#endif
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#define SEGMM_WAVE 64

// ---------------------------------------------------------------- error plumbing (host)
extern thread_local char g_segmm_err[512];
int segmm_fail(int code, const char* fmt, ...);
#define SEGMM_CHECK_HIP(expr)                                                         \
    do {                                                                              \
        hipError_t _e = (expr);                                                       \
        if (_e != hipSuccess) return segmm_fail(-100 - (int)_e, "%s: %s", #expr, hipGetErrorString(_e)); \
    } while (0)
#define SEGMM_REQUIRE(cond, ...)                         \
    do {                                                 \
        if (!(cond)) return segmm_fail(-1, __VA_ARGS__); \
    } while (0)

static inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15u) == 0; }

// ---- streaming row traffic.  The row kernels read and write every byte once; with the default cache policy those bytes pass through
// the XCD's L2 like anything else and push out the operand panels of the GEMMs that run beside them on the other stream.
// SEGMM_ROW_NT: 0 default policy, 1 nontemporal loads / stores for the LayerNorm kernels' fp32 rows, 2 also for the L1 normalisation,
// the column sums and the split-K combine (plane outputs stay cacheable: the next GEMM reads them at once)
#ifndef SEGMM_ROW_NT
#define SEGMM_ROW_NT 2
#endif
#ifndef SEGMM_ATT_AUX
#define SEGMM_ATT_AUX 0          // probe: cache policy of the planes-in attention kernels' operand loads (2 nt)
#endif
#ifndef SEGMM_E_AUX
#define SEGMM_E_AUX 0          // probe: cache policy of the GEMM epilogue's extra-operand loads (2 nt)
#endif
__device__ __forceinline__ f32x4 ld_row4(const float* p) {
#if SEGMM_ROW_NT >= 1
    return __builtin_nontemporal_load((const f32x4*)p);
#else
    return *(const f32x4*)p;
#endif
}
__device__ __forceinline__ void st_row4(float* p, f32x4 v) {
#if SEGMM_ROW_NT >= 1
    __builtin_nontemporal_store(v, (f32x4*)p);
#else
    *(f32x4*)p = v;
#endif
}
__device__ __forceinline__ f32x4 ld_row4b(const float* p) {
#if SEGMM_ROW_NT >= 2
    return __builtin_nontemporal_load((const f32x4*)p);
#else
    return *(const f32x4*)p;
#endif
}
__device__ __forceinline__ void st_row4b(float* p, f32x4 v) {
#if SEGMM_ROW_NT >= 2
    __builtin_nontemporal_store(v, (f32x4*)p);
#else
    *(f32x4*)p = v;
#endif
}

// ---- 16-bit input features (ELEM = SEGMM_ELEM_F16 / SEGMM_ELEM_BF16 of the header): four consecutive elements are ONE 8-byte load
// (a row of a 16-bit [n, D] tensor with D % 4 == 0 is 8-byte aligned, not 16: D = 260 has a 520-byte pitch), ld_row4b's cache
// policy; the raw words stay in registers (2 VGPRs per 4 elements, as two scalar arrays: an array of 2-vectors is promoted to
// one wide vector whose every update copies the whole row) and are widened where they are used.  Both formats embed in
// fp32 exactly: IEEE half through the hardware convert (subnormals included), bfloat16 as bits << 16 -- so a kernel that widens and
// then does its fp32 twin's arithmetic gives that twin's result on the widened tensor, bit for bit.
constexpr int ELEM_F16 = 1, ELEM_BF16 = 2;
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ u32x2 ld_row4h(const uint16_t* p) {
#if SEGMM_ROW_NT >= 2
    return __builtin_nontemporal_load((const u32x2*)p);
#else
    return *(const u32x2*)p;
#endif
}
template <int ELEM>
__device__ __forceinline__ f32x4 widen4(uint32_t a, uint32_t b) {
    if constexpr (ELEM == ELEM_F16) {
        // the convert instruction itself, on the 32-bit words: written as (float)half the compiler turns the row's raw words into one
        // wide vector of halves and copies it whole at every update (120 VGPRs at D = 2048 instead of 44)
        f32x4 v;
        asm("v_cvt_f32_f16_e32 %0, %1" : "=v"(v.x) : "v"(a));
        asm("v_cvt_f32_f16_sdwa %0, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1" : "=v"(v.y) : "v"(a));
        asm("v_cvt_f32_f16_e32 %0, %1" : "=v"(v.z) : "v"(b));
        asm("v_cvt_f32_f16_sdwa %0, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1" : "=v"(v.w) : "v"(b));
        return v;
    } else {
        return f32x4{__uint_as_float(a << 16), __uint_as_float(a & 0xffff0000u), __uint_as_float(b << 16), __uint_as_float(b & 0xffff0000u)};
    }
}
template <int ELEM>
__device__ __forceinline__ f32x4 widen4(u32x2 r) { return widen4<ELEM>(r.x, r.y); }

// ---- 8-bit input features (ELEM = SEGMM_ELEM_E4M3 / _E5M2 / _I8 of the header): four consecutive elements are ONE 4-byte load (a row
// of an 8-bit [n, D] tensor with D % 4 == 0 is 4-byte aligned only: D = 12 has a 12-byte pitch), ld_row4b's cache policy; the raw dword
// stays in a register (1 VGPR per 4 elements) and is widened where it is used.  Every OCP e4m3fn / e5m2 code and every int8 is an exact
// fp32 value and gfx950 converts each with one instruction (v_cvt_f32_fp8 / v_cvt_f32_bf8 with a byte select -- OCP on this part, not
// MI300's fnuz --, v_cvt_f32_i32 of the sign-extended byte), so the rule of the 16-bit forms carries over: widen, then the fp32 twin's
// arithmetic, gives that twin's result on the widened tensor, bit for bit.  What a code MEANS is fixed by tests/feature8_ref.py.
constexpr int ELEM_E4M3 = 3, ELEM_E5M2 = 4, ELEM_I8 = 5;
__device__ __forceinline__ uint32_t ld_row4q(const uint8_t* p) {
#if SEGMM_ROW_NT >= 2
    return __builtin_nontemporal_load((const uint32_t*)p);
#else
    return *(const uint32_t*)p;
#endif
}
template <int ELEM>
__device__ __forceinline__ f32x4 widen4(uint32_t w) {
    static_assert(ELEM == ELEM_E4M3 || ELEM == ELEM_E5M2 || ELEM == ELEM_I8, "widen4(dword): an 8-bit element type");
    const int i = (int)w;
    if constexpr (ELEM == ELEM_E4M3) {
        return f32x4{__builtin_amdgcn_cvt_f32_fp8(i, 0), __builtin_amdgcn_cvt_f32_fp8(i, 1), __builtin_amdgcn_cvt_f32_fp8(i, 2),
                     __builtin_amdgcn_cvt_f32_fp8(i, 3)};
    } else if constexpr (ELEM == ELEM_E5M2) {
        return f32x4{__builtin_amdgcn_cvt_f32_bf8(i, 0), __builtin_amdgcn_cvt_f32_bf8(i, 1), __builtin_amdgcn_cvt_f32_bf8(i, 2),
                     __builtin_amdgcn_cvt_f32_bf8(i, 3)};
    } else {
        return f32x4{(float)(int8_t)(w), (float)(int8_t)(w >> 8), (float)(int8_t)(w >> 16), (float)(i >> 24)};
    }
}

// The row quantiser's code of one SCALED value v (|v| <= 256 / 32768 / 127.5 by the row rule of segmm_quantize_rows, far inside each
// format's range): round to nearest, ties to even, in integer and exactly-rounded fp32 operations only, so that the host reference
// (tests/feature8_ref.py) states the same thing in numpy.  fp8 (EB exponent bias, M mantissa bits): at or above the smallest normal
// 2^(1-EB) the fp32 mantissa is rounded to M bits in place (a carry walks into the exponent by itself); below it the code is the
// count of subnormal steps, rint(|v| 2^(EB-1+M)), which reaches the smallest normal's code 2^M on its own.
template <int ELEM>
__host__ __device__ __forceinline__ uint32_t quant8_code(float v) {
    if constexpr (ELEM == ELEM_I8) {
        return (uint32_t)(int)rintf(v) & 0xffu;
    } else {
        constexpr int EB = ELEM == ELEM_E4M3 ? 7 : 15, M = ELEM == ELEM_E4M3 ? 3 : 2;
        union { float f; uint32_t u; } b;
        b.f = v;
        const uint32_t sign = (b.u >> 24) & 0x80u;
        uint32_t u = b.u & 0x7fffffffu;
        uint32_t code;
        if (u >= ((uint32_t)(127 + 1 - EB) << 23)) {
            u += ((u >> (23 - M)) & 1u) + ((1u << (22 - M)) - 1u);
            code = (u >> (23 - M)) - ((uint32_t)(127 - EB) << M);
        } else {
            b.u = u;
            union { float f; uint32_t u; } k;
            k.u = (uint32_t)(127 + EB - 1 + M) << 23;
            code = (uint32_t)(int)rintf(b.f * k.f);
        }
        return sign | code;
    }
}

// ---------------------------------------------------------------- counter-based dropout stream
// Dropout masks are a pure function of (seed, site, element index), so the backward kernels
// regenerate them instead of storing them.  The generator is a stateless integer hash (two chained
// rounds of a 32-bit avalanche mix, ~14 VALU ops) that yields 4 x 16 random bits for the 4 consecutive
// elements of one "quad"; the first version used Philox4x32-10 (~120 ops per quad), which made the
// attention kernels VALU-bound (rocprof: 23 VALU instructions per MFMA).  16 bits per element
// quantise the drop probability to 1/65536 (0.1 -> 6554/65536 = 0.100006); the rescale uses the
// quantised value, so E[mask] = 1 exactly.
struct DropCfg {
    float p;              // drop probability (0 => disabled)
    float scale;          // 1/(1-p_quantised)
    uint32_t thresh;      // keep iff r16 >= thresh, thresh = round(p * 65536)
    uint32_t seed_lo, seed_hi;
    uint32_t site;        // distinct per dropout site in the model
    uint32_t live;        // != 0: the seed is XORed with the DEVICE-side step words (*st) when the kernel starts
    const struct StepState* st;          // the step state bound when the launch was made (segmm_step_bind); null unless live
};

// ---- device-side step state.  A training step captured in a hipGraph replays the SAME kernel arguments every step, so what
// must change from step to step lives in device memory and is advanced by a one-thread kernel at the head of the step
// (segmm_step_advance): two seed words for the dropout streams (kernels launched with a "live" seed -- bit 63 of the seed
// argument -- XOR them into their seed) and AdamW's bias corrections (segmm_adamw with step < 0 reads them).
// The state is a small struct in CALLER-OWNED device memory (segmm_step_state_bytes; segmm_step_bind names the one the following
// launches use -- two trainers in one process each bind their own before they step); with nothing bound the library falls back to
// one default state of its own.  The pointer travels inside the launch's arguments: no __device__ global.
// The learning rate of the step lives here too (segmm_step_schedule): `lr` is the rate of the step whose count is `step`, evaluated
// by the same one-thread kernels from the schedule descriptor behind it; the AdamW kernels read it when they are handed the
// sentinel lr < 0.  An all-zero state has no schedule (kind 0) and lr = 0.
struct StepState {
    uint32_t seed_lo, seed_hi; int step; float bc1, bc2_sqrt;
    float lr;                                  // rate of step `step` (of step 1 while step = 0), fp32(schedule in double)
    int kind;                                  // SEGMM_LR_* (0: no schedule)
    float base_lr; int warmup_steps; float start_factor; int decay_steps; float eta_min, gamma; int step_size;
    // The non-finite guard (segmm_step_guard and the *_guarded entry points; every other kernel leaves these two words alone and never
    // reads them: a caller of the older entry points was never promised that they are zero).  `step` goes on counting ATTEMPTED steps;
    // the bias corrections of a guarded step are those of the applied index step - skipped (segmm_step_advance_guarded).
    uint32_t skip;                             // this step's verdict: 1 = its gradient norm is NaN or inf, the guarded launches return
    uint32_t skipped;                          // the steps skipped so far
};
static_assert(sizeof(StepState) == 64, "StepState: its size is part of the ABI (segmm_step_state_bytes)");
static_assert(sizeof(StepState) % 16 == 0, "StepState: a multiple of 16 bytes");
extern StepState* g_segmm_step;          // host: the bound state (capi.hip)
StepState* segmm_step_current();         // host: the bound state, or the library's default one (allocated on first use)
// lr after k completed optimizer steps (torch's opt.step(); sched.step() loop: step t runs at k = t - 1), in double from the fp32
// descriptor: base_lr warm(k) dec(max(k - W, 0)); warm ramps linearly from start_factor to 1 over W steps, dec by kind
// (1 constant, 2 cosine and 3 linear down to eta_min over decay_steps and held there, 4 gamma^floor(j / step_size), 5 gamma^j).
// tests/lr_ref.py states the same expression operation for operation; nothing may be contracted into an fma.
__host__ __device__ inline double segmm_lr_at(const StepState& s, int k) {
#pragma clang fp contract(off)
    if (s.kind == 0) return 0.0;
    const double base = (double)s.base_lr, sf = (double)s.start_factor;
    const int W = s.warmup_steps, D = s.decay_steps;
    if (k < 0) k = 0;
    const double warm = (W > 0 && k < W) ? sf + (1.0 - sf) * (double)k / (double)W : 1.0;
    const int j = k > W ? k - W : 0;
    const double r = (double)s.eta_min / base;
    const double jd = (double)(j < D ? j : D);
    double dec = 1.0;
    if (s.kind == 2) dec = r + (1.0 - r) * (1.0 + cos(3.14159265358979323846 * jd / (double)D)) / 2.0;
    else if (s.kind == 3) dec = 1.0 - (1.0 - r) * jd / (double)D;
    else if (s.kind == 4) dec = pow((double)s.gamma, (double)(j / s.step_size));
    else if (s.kind == 5) dec = pow((double)s.gamma, (double)j);
    return base * warm * dec;
}
__device__ __forceinline__ DropCfg drop_live(DropCfg d) {
    if (d.live) { d.seed_lo ^= d.st->seed_lo; d.seed_hi ^= d.st->seed_hi; }
    return d;
}

__device__ __forceinline__ uint32_t mix32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
// 64 random bits for the 4 elements [4*q, 4*q+3] of a site (q = element_index / 4)
__device__ __forceinline__ uint2 drop_rand_quad(const DropCfg& d, uint64_t q) {
    const uint32_t k = d.seed_lo ^ (d.site * 0x9E3779B9u) ^ ((uint32_t)(q >> 32) * 0x85EBCA6Bu);
    const uint32_t a = mix32((uint32_t)q ^ k);
    const uint32_t b = mix32(a ^ d.seed_hi ^ 0x68E31DA4u);
    return make_uint2(a, b);
}
// One row's uniformly random permutation of 0 .. S-1 by rank counting (rand_perm_rows_kernel, valid_rows_kernel): one wave per row,
// lane l draws the 32-bit keys of the indices l, l + 64, ... (R = ceil(S / 64) of them, counters row * stride + index of the site's
// stream) and counts, for each, the (key, index) pairs of the row below it: rank[r] = the position of index r * 64 + lane in the
// permutation.  The row's keys go through ``keys`` (this wave's 64 R words of LDS): every lane reads key j at the same address, a
// broadcast read.  Contains a workgroup barrier: EVERY thread of the workgroup calls it, ``active`` = false skips the counting.
// Counter stride of a row: 64 for S <= 64 (R = 1), 256 beyond -- rows of up to 64 keep the stream recorded noPos steps drew from.
template <int R>
__device__ __forceinline__ void perm_row_draw(const DropCfg& d, uint64_t row, int S, int lane, uint32_t* keys, bool active, int (&rank)[R]) {
    constexpr uint64_t kStride = R == 1 ? 64u : 256u;
    uint32_t key[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint2 x = drop_rand_quad(d, row * kStride + (uint64_t)(r * 64 + lane));
        key[r] = x.x;
        rank[r] = 0;
        keys[r * 64 + lane] = x.x;
    }
    __syncthreads();
    if (!active) return;
    for (int j = 0; j < S; ++j) {
        const uint32_t kj = keys[j];
#pragma unroll
        for (int r = 0; r < R; ++r)
            rank[r] += (kj < key[r] || (kj == key[r] && j < r * 64 + lane)) ? 1 : 0;
    }
}
// the logistic function of the loss kernels (loss.h) and of the validation tail (evalops.h valid_rows_kernel)
__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

__device__ __forceinline__ f32x4 drop_apply4(const DropCfg& d, uint64_t q, f32x4 v) {
    const uint2 r = drop_rand_quad(d, q);
    v.x = ((r.x & 0xffffu) >= d.thresh) ? v.x * d.scale : 0.f;
    v.y = ((r.x >> 16) >= d.thresh) ? v.y * d.scale : 0.f;
    v.z = ((r.y & 0xffffu) >= d.thresh) ? v.z * d.scale : 0.f;
    v.w = ((r.y >> 16) >= d.thresh) ? v.w * d.scale : 0.f;
    return v;
}
// multiplier (0 or scale) of one element
__device__ __forceinline__ float drop_mult1(const DropCfg& d, uint64_t elem) {
    const uint2 r = drop_rand_quad(d, elem >> 2);
    const uint32_t lane = (uint32_t)(elem & 3);
    const uint32_t w = lane < 2 ? r.x : r.y;
    const uint32_t x = (lane & 1) ? (w >> 16) : (w & 0xffffu);
    return (x >= d.thresh) ? d.scale : 0.f;
}

static inline DropCfg make_drop(float p, uint64_t seed, uint32_t site) {
    DropCfg d;
    d.p = p;
    double t = (double)p * 65536.0 + 0.5;
    d.thresh = p <= 0.f ? 0u : (t >= 65535.0 ? 65535u : (uint32_t)t);
    d.scale = p > 0.f ? (float)(65536.0 / (65536.0 - (double)d.thresh)) : 1.0f;
    d.seed_lo = (uint32_t)seed;
    d.seed_hi = (uint32_t)(seed >> 32) & 0x7fffffffu;
    d.site = site;
    d.live = (uint32_t)(seed >> 63);
    d.st = d.live ? segmm_step_current() : nullptr;
    return d;
}

// ---------------------------------------------------------------- math
__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752f)); }
__device__ __forceinline__ float gelu_erf_grad(float x) {
    const float cdf = 0.5f * (1.0f + erff(x * 0.70710678118654752f));
    const float pdf = 0.39894228040143268f * __expf(-0.5f * x * x);
    return cdf + x * pdf;
}

// ---------------------------------------------------------------- wave64 reductions (shuffle, no LDS)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// max over the wave, the same value in every lane.  Not the xor butterfly of wave_sum: six ds_bpermute round trips (the LDS
// crossbar, ~100 cycles each and serial) are what the attention kernels' per-tile scale derivation waited on.  Inside a row
// of 16 lanes the partners come through DPP (lane xor 1, xor 2, then the mirrored half-row and row: every lane of a row ends
// with the row's maximum), the four rows meet through v_readlane.  max is exact and order-independent, so nothing changes
// numerically.  Needs every lane of the wave active (like the shuffle form).
template <int CTRL>
__device__ __forceinline__ float dpp_row_move(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}
__device__ __forceinline__ float wave_max(float v) {
    v = fmaxf(v, dpp_row_move<0xB1>(v));           // quad_perm [1,0,3,2]
    v = fmaxf(v, dpp_row_move<0x4E>(v));           // quad_perm [2,3,0,1]
    v = fmaxf(v, dpp_row_move<0x141>(v));          // row_half_mirror
    v = fmaxf(v, dpp_row_move<0x140>(v));          // row_mirror
    const int i = __float_as_int(v);
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(i, 0)), r1 = __int_as_float(__builtin_amdgcn_readlane(i, 16));
    const float r2 = __int_as_float(__builtin_amdgcn_readlane(i, 32)), r3 = __int_as_float(__builtin_amdgcn_readlane(i, 48));
    return fmaxf(fmaxf(r0, r1), fmaxf(r2, r3));
}
// ---- running max|x| of a tensor, for the fp16x3 GEMM engine's per-tensor scale.  A producer kernel keeps a
// per-lane running maximum of what it stores and folds it, once per wave, into one of AMAX_SLOTS partial maxima
// with an INTEGER atomic max on the float bits (non-negative floats order like unsigned ints: exact, and
// independent of the order of arrival).  The slot array is zeroed by the host before the producer runs; the
// consuming GEMM reduces the slots itself.
constexpr int AMAX_SLOTS = 256;
__device__ __forceinline__ float absmax4(float m, f32x4 v) {
    return fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
}
__device__ __forceinline__ void amax_commit(float* slots, float m, unsigned key) {
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) atomicMax((unsigned int*)slots + (key & (AMAX_SLOTS - 1)), __float_as_uint(m));
}
// ---- "site header" of a plane tensor (gemm_planes.h): SITE_HDR floats followed by the AMAX_SLOTS partial maxima.
// hdr[0] = power-of-two scale the fp16 (hi, lo) planes were written with (0: no planes written), hdr[1] (as an
// integer) != 0: some element left the fp16 range under that scale -> consumers take the fp32 copy instead.
constexpr int SITE_HDR = 8;
constexpr int SITE_FLOATS = SITE_HDR + AMAX_SLOTS;
__device__ __forceinline__ void site_commit(float* hdr, float m, unsigned key, float s_used) {
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) {
        atomicMax((unsigned int*)hdr + SITE_HDR + (key & (AMAX_SLOTS - 1)), __float_as_uint(m));
        if (s_used > 0.f && !(m * s_used < 65504.f)) ((volatile unsigned int*)hdr)[1] = 1u;      // NaN raises it too
    }
}
// power of two s with amax * s in [2^14, 2^15); exponent clamped to +-60 so that 1/(sa sb) stays finite
__device__ __forceinline__ float f16_scale_of(float amax) {
    const uint32_t u = __float_as_uint(amax);
    if (!(amax > 0.f) || (u >> 23) == 0xff) return 1.f;
    int se = 14 - ((int)(u >> 23) - 127);
    se = max(-60, min(60, se));
    return __uint_as_float((uint32_t)(se + 127) << 23);
}
// largest |x| the producers of a site recorded (AMAX_SLOTS partial maxima, four per lane): the same value in every wave
__device__ __forceinline__ float site_amax(const float* hdr, int lane) {
    static_assert(AMAX_SLOTS == 256, "one float4 per lane");
    const f32x4 v = *(const f32x4*)(hdr + SITE_HDR + lane * 4);
    return wave_max(fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
}
// Planes written with the (delayed) scale s are usable iff the tensor's maximum sits inside the fp16 window: below 65504 -- the
// producers' overflow flag says the same -- AND not so far below it that the lo terms sink into the subnormals: a tensor that
// SHRANK by more than ~2^9 since its scale was derived (the gradients of a batch whose loss has collapsed) would silently keep
// 12 bits instead of 22.  max * s >= 2^-2 keeps every element's absolute error below 2^-22 max.  Checked by the CONSUMER, which
// sees the complete maxima (one 1 KB read per wave); block-uniform.
//
// THE RULE IS STATED HERE ONCE.  A producer's repair launch (gemm_planes_epi.h) and the consumers of the repaired planes
// (attention_pl.h) must reach the same verdict from the same header words, or the consumer reads planes at the wrong scale:
// every kernel judges a site through site_window_ok, or -- on votes -- through window_cmp + window_holds.
struct WindowCmp { bool pos, big, over; };          // a maximum m against the window of scale s
__device__ __forceinline__ WindowCmp window_cmp(float s, float m) { return {m > 0.f, m * s >= 0.25f, !(m * s < 65504.f)}; }
// (s at its upper clamp 2^60 -- f16_scale_of / scales_update keep 1/(sa sb) finite: the fallback would use the same scale)
__device__ __forceinline__ bool window_holds(float s, WindowCmp c) { return !c.pos || ((c.big || s >= 0x1p60f) && !c.over); }
__device__ __forceinline__ bool site_live(float s, uint32_t flag) { return s > 0.f && flag == 0u; }          // planes written, no overflow recorded
__device__ __forceinline__ bool site_window_ok(float s, uint32_t flag, float m) {
    return site_live(s, flag) && window_holds(s, window_cmp(s, m));
}
__device__ __forceinline__ bool site_planes_ok(const float* hdr, float s, int lane) {
    if (!site_live(s, __float_as_uint(hdr[1]))) return false;          // (no read of the maxima then)
    return site_window_ok(s, 0u, site_amax(hdr, lane));
}
// The same verdict for kernels that cannot wait for three dependent reads: site_words REQUESTS every header word of a site
// (scale, flag, this lane's four partial maxima) -- call it for all sites of a kernel before the first use, so that the loads
// share one round trip.  site_scale is the wave-uniform scale; site_usable judges the words under it (needs the maxima: ask
// only where there is an fp32 copy to fall back on); site_state is both plus the site's maximum, for the repair verdict.
__device__ __forceinline__ float wave_uniform(float x) {          // same in every lane: keep it scalar
    return __uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane((int)__float_as_uint(x)));
}
struct SiteWords { float scale, flag; f32x4 amax4; };
struct SiteState { float scale, amax; bool ok; };
__device__ __forceinline__ SiteWords site_words(const float* hdr, int lane) {
    return {hdr[0], hdr[1], *(const f32x4*)(hdr + SITE_HDR + lane * 4)};
}
__device__ __forceinline__ float site_scale(const SiteWords& w) { return wave_uniform(w.scale); }
__device__ __forceinline__ SiteState site_state(const SiteWords& w) {
    const float s = site_scale(w);
    const float m = wave_max(fmaxf(fmaxf(w.amax4.x, w.amax4.y), fmaxf(w.amax4.z, w.amax4.w)));
    return {s, m, site_window_ok(s, __float_as_uint(wave_uniform(w.flag)), m)};
}
__device__ __forceinline__ bool site_usable(const SiteWords& w) { return site_state(w).ok; }
// (x0, x1) * s -> packed fp16 (hi0, hi1), (lo0, lo1); hi + lo = x s up to 2^-22 |x s|.
// Four VALU instructions per pair: v_fma_mix{lo,hi}_f16 multiply in fp32, round ONCE to fp16 and write one half
// of the destination, and take the fp16 hi term straight back as the addend of the lo term
// (lo = rn16(x s - hi), the fma is exact before that rounding).  fp16 subnormal lo terms are kept.  The hi term is x s + 0:
// x = -0 is stored as hi = +0, lo = -0 (tests/p32_ref.py states the format on the host; the cast-and-fmaf form of
// gemm_planes.h's weight split compiles to the same two instructions).
__device__ __forceinline__ void splith_pair(float x0, float x1, float s, uint32_t& ph, uint32_t& pl) {
    uint32_t h, l;
    asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "=v"(h) : "v"(x0), "v"(s));
    asm("v_fma_mixhi_f16 %0, %1, %2, 0" : "+v"(h) : "v"(x1), "v"(s));
    asm("v_fma_mixlo_f16 %0, %1, %2, -%3 op_sel_hi:[0,0,1]" : "=v"(l) : "v"(x0), "v"(s), "v"(h));
    asm("v_fma_mixhi_f16 %0, %1, %2, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(l) : "v"(x1), "v"(s), "v"(h));
    ph = h;
    pl = l;
}

// ---- producer side of a plane tensor.  A kernel that writes a GEMM operand also writes its P32 fp16 planes (gemm_planes.h:
// per row and per 32 columns [32 hi | 32 lo]) with the DELAYED scale *scale_in (a power of two derived from the maxima this
// tensor site had on earlier steps; null or 0: no planes yet -> the host runs an exact split pass instead), records that
// scale in hdr[0] and folds the partial maxima / the overflow flag into the header.  Consumers fall back to the fp32 copy
// when the flag is up, so a scale that has become too large costs time, never correctness.
struct PlaneOut {
    _Float16* p; int ld2;         // plane view (null: no plane output)
    float* hdr;                   // site header of the tensor
    const float* scale_in;        // device scalar: the scale to write with
};
__device__ __forceinline__ float plane_scale(const PlaneOut& po) {
    return (po.p && po.scale_in) ? *po.scale_in : 0.f;
}
// 4 consecutive columns c .. c+3 (c % 4 == 0) of row `row`
__device__ __forceinline__ void plane_store4(_Float16* p, int ld2, long long row, int c, f32x4 v, float s) {
    uint32_t h0, l0, h1, l1;
    splith_pair(v.x, v.y, s, h0, l0);
    splith_pair(v.z, v.w, s, h1, l1);
    _Float16* o = p + row * ld2 + ((c >> 5) << 6) + (c & 31);
    *(uint2*)o = make_uint2(h0, h1);
    *(uint2*)(o + 32) = make_uint2(l0, l1);
}
// The same for kernels in which ADJACENT LANES hold ADJACENT float4 column groups of one row (lane l: columns c, lane l ^ 1:
// columns c ^ 4; both lanes of a pair active): the pair trades half of its terms through DPP (quad_perm 1,0,3,2), the even
// lane stores the 8 hi terms of columns [c & ~7, +8) and the odd lane the 8 lo terms -- ONE 16-byte store per lane, eight
// adjacent lanes write one whole 128-byte [32 hi | 32 lo] block.  (8-byte stores issued twice per lane ran the fused
// producers at a third of the HBM rate: 1.4 TB/s for the plane bytes.)
__device__ __forceinline__ uint32_t dpp_swap1(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, true);
}
__device__ __forceinline__ void plane_store4_pair(_Float16* p, int ld2, long long row, int c, f32x4 v, float s) {
    uint32_t h0, l0, h1, l1;
    splith_pair(v.x, v.y, s, h0, l0);
    splith_pair(v.z, v.w, s, h1, l1);
    const bool odd = (c & 4) != 0;
    const uint32_t r0 = dpp_swap1(odd ? h0 : l0), r1 = dpp_swap1(odd ? h1 : l1);      // odd lanes give away hi, even lanes lo
    const int cb = c & ~7;
    _Float16* o = p + row * ld2 + ((cb >> 5) << 6) + (cb & 31) + (odd ? 32 : 0);
    const uint4 w = odd ? make_uint4(r0, r1, l0, l1) : make_uint4(h0, h1, r0, r1);
#if SEGMM_NT_STORES
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    __builtin_nontemporal_store(u32x4{w.x, w.y, w.z, w.w}, (u32x4*)o);          // written once, read by a later kernel after GBs of other traffic
#else
    *(uint4*)o = w;
#endif
}
// end of a producer wave: partial maxima (+ flag) and the scale used.  The scale is stored by the waves whose key is a
// multiple of 1024 (key 0 always exists and always gets here; EVERY wave storing to that one word serialised the stores of
// a 51 200-row kernel at the memory side and more than doubled its run time).
__device__ __forceinline__ bool scale_writer(unsigned key) { return (threadIdx.x & 63) == 0 && (key & 1023u) == 0u; }
__device__ __forceinline__ void plane_finish(const PlaneOut& po, float* amax_slots, float am, unsigned key, float s, bool) {
    if (s > 0.f) {
        site_commit(po.hdr, am, key, s);
        if (scale_writer(key)) po.hdr[0] = s;
    } else if (amax_slots) {
        amax_commit(amax_slots, am, key);
    }
}
// inclusive prefix sum across the 64 lanes
__device__ __forceinline__ float wave_scan_incl(float v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}
// inclusive suffix sum over the wave: lane k gets v_k + v_(k+1) + ... + v_63
__device__ __forceinline__ float wave_suffix_incl(float v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float t = __shfl_down(v, o, 64);
        if (lane + o < 64) v += t;
    }
    return v;
}

// ---- raw buffer addressing: one resource descriptor (4 SGPRs) per tensor, a 32-bit per-lane byte offset and a
// scalar byte offset per access -- no 64-bit per-lane address arithmetic, and reads beyond [p, p + bytes) return 0
// (hardware range check) instead of faulting.  Tensors addressed this way must be smaller than 4 GiB.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* p, uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ f32x4 buf_load4(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, (int)soff, 0));
}

// XCD-aware bijective remap of a linear workgroup id (hardware deals consecutive ids round-robin over
// the 8 XCDs): gives every XCD a contiguous chunk of logical ids so tiles that share an operand panel
// hit the same L2.  Speed only; any mapping is correct.
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
    const int q = nwg >> 3, r = nwg & 7, x = bid & 7;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (bid >> 3);
}
