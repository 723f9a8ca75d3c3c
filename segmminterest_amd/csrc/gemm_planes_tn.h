// What the round-3 and round-6 TN plane GEMMs (gemm_pl_tn8, gemm_pl_tn4) share outside their k-loops, stated once: the LDS
// image of a token row (DMA source, fp32-fallback writer, fragment-read offsets) and the output code.  The transposed
// fragment read lds_tr8 and the tile / split prologue TnTile sit in gemm_planes.h, where the round-2 gemm_pl_tn sees them too.
#pragma once
#include "gemm_planes_epi.h"

namespace segmm {

// ================================================================ the token-row image
// A token row of a stage is 64-byte pieces (piece = 2 * feature block + plane; 32 features per block).  Piece c of token t sits
// at physical piece c ^ (t & 3): the four token rows of a transposed read fall into four different 64-byte bank windows.  Inside
// a piece the two 32-byte halves (16 features each) are swapped for tokens with bit 3 set: the two 16-lane groups of a 32-lane
// half read the SAME 16 features of tokens 8 apart, which would otherwise hit the same banks twice.  Row pitches of 1024, 512
// and 256 B are multiples of the 256-byte bank period: the transposed reads are conflict-free.  Producers and consumer below.

// LDS-DMA writes lane-linear, so the permutation goes on the SOURCE: byte offset in the token row that physical chunk l (16 B) fetches
__device__ __forceinline__ uint32_t tn_image_src(int l, int tok) {
    return (uint32_t)((((l >> 2) ^ (tok & 3)) << 6) + (((l & 3) ^ (((tok >> 3) & 1) << 1)) << 4));
}
// fallback writer: features f .. f + 3 (f % 4 == 0, relative to the staged row) of token t, split at scale sc, to their two pieces
__device__ __forceinline__ void tn_image_put(char* row, int f, f32x4 x, float sc, int t) {
    uint32_t h0, l0, h1, l1;
    splith_pair(x.x, x.y, sc, h0, l0); splith_pair(x.z, x.w, sc, h1, l1);
    // 8-byte group g8 of feature block b: 16-byte chunk g8 >> 1, the inverse of tn_image_src
    const int b = f >> 5, g8 = (f & 31) >> 2, cp = (g8 >> 1) ^ (((t >> 3) & 1) << 1), sw = t & 3;
    *(uint2*)(row + (((2 * b) ^ sw) << 6) + (cp << 4) + ((g8 & 1) << 3)) = make_uint2(h0, h1);
    *(uint2*)(row + (((2 * b + 1) ^ sw) << 6) + (cp << 4) + ((g8 & 1) << 3)) = make_uint2(l0, l1);
}
// Transposed fragment reads: lane = (lq = lane >> 4: token octet, qq = (lane >> 2) & 3: token inside a 4-block, pp = lane & 3).
// Lane part of the offset of 16-feature tile i, plane pl, in rows of `pitch` bytes, the lane's tokens starting at octet `oct`:
// the XOR with qq touches the two low bits of the piece index only -- x[v], v = 2 (feature block & 1) + plane, then a constant
// 256 B per feature-block pair and the half offset h[i & 1] (swapped for octets 1, 3: tokens with bit 3 set).
struct TnFrag {
    uint32_t x[4], h[2];
    __device__ __forceinline__ uint32_t operator()(int i, int pl) const { return x[2 * ((i >> 1) & 1) + pl] + (uint32_t)((i >> 2) * 256) + h[i & 1]; }
};
__device__ __forceinline__ TnFrag tn_frag_off(int lane, int oct, int pitch) {
    const int qq = (lane >> 2) & 3, pp = lane & 3;
    const uint32_t base = (uint32_t)((8 * oct + qq) * pitch + 8 * pp), hsw = (uint32_t)((oct & 1) << 5);
    TnFrag f;
#pragma unroll
    for (int v = 0; v < 4; ++v) f.x[v] = base + (uint32_t)((v ^ qq) << 6);
    f.h[0] = hsw; f.h[1] = 32u ^ hsw;
    return f;
}

// ================================================================ the TN outputs
// Tile extents, wave groups and the patch offset are the NT epilogue's (the k-loops share their LDS); what TN adds is the tile
// row of the column sum accb[e] that wave (grp, wn) holds: gemm_pl_tn8 sums A tile wn of its phase e, gemm_pl_tn4 A tile 2 wn + e.
template <int GROUPS_, bool READS_FIRST_>
struct TnOutGeom : NtEpiGeom<4, GROUPS_, READS_FIRST_> {
    static __device__ __forceinline__ int cs_row(int grp, int wn, int e) { return GROUPS_ > 1 ? grp * 128 + e * 64 + 16 * wn : 16 * (2 * wn + e); }
};
// Column sums (every row of accb holds them: lanes of column group 0 own 16 features each), then the split-K slab or C itself:
// acc / (sa sb), eight row blocks as whole 256-byte row segments through the wave's transpose patch (see nt_epilogue), default
// cache policy (splitk_reduce reads the slabs back at once).  Lane layout of acc as in nt_epilogue.
template <class G>
__device__ __forceinline__ void tn_outputs(const GemmArgs& p, const PGemmX& q, const f32x4 (&acc)[8][4], const f32x4 (&accb)[2], char* smem,
                                           float sa, float sb, const TnTile<G::BM>& T, int wave, int lane) {
    const int grp = G::GROUPS > 1 ? wave >> 2 : 0, wn = G::GROUPS > 1 ? wave & 3 : wave;
    const int l15 = lane & 15, lq = lane >> 4;
    const bool split = gridDim.z > 1;
    const float inv_a = 1.f / sa;
    if (T.do_colsum && lq == 0) {
        float* dst = split ? q.colsum_ws + (size_t)T.kz * p.M : q.colsum_out;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int m = T.m0 + G::cs_row(grp, wn, e) + l15;
            if (m < p.M) dst[m] = accb[e].x * inv_a;
        }
    }
    const float inv_ab = inv_a * (1.f / sb);
    float* Cout = split ? p.C + (size_t)T.kz * (size_t)p.slab_stride : p.C;
    const __amdgpu_buffer_rsrc_t rsC = make_rsrc(Cout, (uint32_t)((((long long)p.M - 1) * p.ldc + p.N) * 4));
    char* trp = smem + G::PATCH + wave * 4096;
    const int gnT = T.n0 + wn * 64 + 4 * l15;
    const uint32_t oCT = (((uint32_t)(T.m0 + grp * 128 + lq) * (uint32_t)p.ldc + (uint32_t)gnT) * 4u) | (gnT < p.N ? 0u : BUF_OOB);
    auto tr_get = [&](int t) { const int r = 4 * t + lq; return *(const f32x4*)(trp + r * 256 + (((l15 ^ r) & 15) << 4)); };
#pragma unroll
    for (int i = 0; i < 8; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) *(f32x4*)(trp + l15 * 256 + (((lq + 4 * j) ^ l15) << 4)) = acc[i][j] * inv_ab;
        f32x4 g4[4];          // READS_FIRST: the four reads before the first store (see NtEpiGeom)
        if (G::READS_FIRST) {
#pragma unroll
            for (int t = 0; t < 4; ++t) g4[t] = tr_get(t);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) buf_store4k(rsC, oCT, (uint32_t)(16 * i + 4 * t) * (uint32_t)p.ldc * 4u, G::READS_FIRST ? g4[t] : tr_get(t));
    }
}

}  // namespace segmm
