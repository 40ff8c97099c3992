// mmq_dev.hpp -- the int8-MFMA block bodies of the K-quant mat-muls against a tile of up to 32 activation columns: what k_mmq_kquant (mmq.hip, dense MUL_MAT) and
// k_mmq_id (mmq_id.hip, expert-grouped MUL_MAT_ID) share.  One wave = 32 weight rows (lane % 32) x the column tile; a kernel hands over this lane's weight row and this
// lane's COLUMN (the Q8_K image of tile column lane % 32), runs mmq_blocks over the K blocks of its wave, folds the KS waves with mmq_fold and stores on its own.
// The arithmetic and the register layout are described at the head of mmq.hip.
#pragma once
#include "../kernels.hpp"

namespace mi {

typedef int i32x4  __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

// Q6_K blocks are 210 bytes: only 2-byte aligned.  Global memory takes unaligned vector loads (as the mat-vec kernels' ld_w relies on)
static __device__ __forceinline__ u32x4 ld16u(const char * p) { return *(const u32x4 *) p; }
static __device__ __forceinline__ u32x2 ld8u (const char * p) { return *(const u32x2 *) p; }

// The K blocks wave, wave + KS, ... of one 32-row x 32-column tile, accumulated into out[]: register 4 * g + i = column 8 * g + 4 * hb + i of this lane's row.
//   wrow  this lane's weight row (blocks of `type`: Q4_K / Q5_K / Q6_K)
//   acol  the Q8_K image of this lane's column (a lane past the tile's columns passes any valid image: its outputs are never stored)
//   yd    LDS [nblk][32]: the columns' block scales, filled by stage_scales() -- called once by EVERY wave, behind the first blocks' loads, and ending in a barrier
// NT: column groups of 8 in use (1..4), KS: waves per workgroup splitting K.
template <int NT, int KS, typename Stage>
static __device__ __forceinline__ void mmq_blocks(const int type, const char * wrow, const char * acol, const int nblk, const int wave, const int hb, const float * yd,
                                                  float (&out)[NT * 4], Stage stage_scales) {
    if (type == GGML_TYPE_Q4_K || type == GGML_TYPE_Q5_K) {
        // Q5_K (176-byte blocks: d, dmin, scales[12], qh[32], qs[128]): the same sub-block structure, bit j of qh[l] is the fifth bit of
        // sub-block j's weight l -- OR-ed into the unpacked nibbles, everything else as Q4_K
        const bool q5 = type == GGML_TYPE_Q5_K;
        const int bs = q5 ? 176 : 144, qoff = q5 ? 48 : 16;
        const char * arow = acol + 16 * hb;
        struct wblk { u32x4 hdr, qs[4], qh; };                         // one block of this lane's row (its half of the nibbles)
        struct ablk { u32x4 av[8]; };                                  // the token's int8 of one block (this lane's 16 of every 32)
        auto fetch = [&](int b, wblk & G) {
            const char * p = wrow + (size_t) b * bs;
            G.hdr = *(const u32x4 *) p;
#pragma unroll
            for (int q = 0; q < 4; ++q) G.qs[q] = *(const u32x4 *) (p + qoff + q * 32 + 16 * hb);
            if (q5) G.qh = *(const u32x4 *) (p + 16 + 16 * hb);
        };
        auto fetch_a = [&](int b, ablk & G) {
            const char * ab = arow + (size_t) b * 256;
#pragma unroll
            for (int j = 0; j < 8; ++j) G.av[j] = *(const u32x4 *) (ab + j * 32);
        };
        auto reduce = [&](int b, const wblk & G, const ablk & GA) {
            // scales / mins of the 8 sub-blocks (get_scale_min_k4, ggml-quants.c:703-710)
            const uint32_t s0 = G.hdr[1], s1 = G.hdr[2], s2 = G.hdr[3];          // scales[0..3], [4..7], [8..11]
            int sc[8], mn[8];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t lo = (s0 >> (8 * j)) & 0xff, mid = (s1 >> (8 * j)) & 0xff, hi = (s2 >> (8 * j)) & 0xff;
                sc[j]     = (int) (lo & 63);                 mn[j]     = (int) (mid & 63);
                sc[j + 4] = (int) ((hi & 0xf) | ((lo >> 6) << 4));   mn[j + 4] = (int) ((hi >> 4) | ((mid >> 6) << 4));
            }
            i32x16 acc, mins;
#pragma unroll
            for (int e = 0; e < 16; ++e) { acc[e] = 0; mins[e] = 0; }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const u32x4 av = GA.av[j];                          // (lanes past the tile's columns carry another column's bytes: their outputs are never stored)
                const u32x4 wq = G.qs[j >> 1];
                i32x4 wv, mv, aa;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    uint32_t w5 = (wq[e] >> (4 * (j & 1))) & 0x0f0f0f0fu;
                    if (q5) w5 |= ((G.qh[e] >> j) & 0x01010101u) << 4;
                    wv[e] = (int) w5;
                    mv[e] = mn[j] * 0x01010101;
                    aa[e] = (int) av[e];
                }
                i32x16 z;
#pragma unroll
                for (int e = 0; e < 16; ++e) z[e] = 0;
                const i32x16 sj = __builtin_amdgcn_mfma_i32_32x32x32_i8(aa, wv, z, 0, 0, 0);
                mins = __builtin_amdgcn_mfma_i32_32x32x32_i8(aa, mv, mins, 0, 0, 0);
#pragma unroll
                for (int e = 0; e < NT * 4; ++e) acc[e] += __mul24(sj[e], sc[j]);
            }
            const float d = h2f((uint16_t) (G.hdr[0] & 0xffff)), dmin = h2f((uint16_t) (G.hdr[0] >> 16));
#pragma unroll
            for (int g = 0; g < NT; ++g) {
                const f32x4 y4 = *(const f32x4 *) (yd + b * 32 + 8 * g + 4 * hb);
#pragma unroll
                for (int i = 0; i < 4; ++i) out[4 * g + i] += y4[i] * (d * (float) acc[4 * g + i] - dmin * (float) mins[4 * g + i]);
            }
        };
        // weights ring: RD - 1 blocks of this lane's row in flight ahead of the one being reduced (HBM latency ~2 us, a block's
        // arithmetic well under 1 us); the tokens' int8 come from L2 at use
        constexpr int RD = 4;
        wblk R[RD]; ablk GA;
        const int nb_w = wave < nblk ? (nblk - wave + KS - 1) / KS : 0;         // this wave's blocks: wave, wave + KS, ...
#pragma unroll
        for (int u = 0; u < RD - 1; ++u) if (u < nb_w) fetch(wave + u * KS, R[u]);
        stage_scales();
        for (int i0 = 0; i0 < nb_w; i0 += RD) {
#pragma unroll
            for (int u = 0; u < RD; ++u) {
                const int i = i0 + u;
                if (i < nb_w) {
                    if (i + RD - 1 < nb_w) fetch(wave + (i + RD - 1) * KS, R[(u + RD - 1) % RD]);
                    fetch_a(wave + i * KS, GA);
                    reduce(wave + i * KS, R[u], GA);
                }
            }
        }
    } else {                                                             // GGML_TYPE_Q6_K
        struct wblk { u32x2 ql[8], qh[4]; u32x4 sc; uint32_t d; };
        struct ablk { u32x2 av[16]; };
        auto fetch = [&](int b, wblk & G) {
            const char * p = wrow + (size_t) b * 210;
            // ql chunk c = n*4 + par*2 + is -> bytes n*64 + par*32 + is*16 + 8*hb ; qh chunk c = n*2 + is -> bytes 128 + n*32 + is*16 + 8*hb
#pragma unroll
            for (int c = 0; c < 8; ++c) G.ql[c] = ld8u(p + (c >> 2) * 64 + ((c >> 1) & 1) * 32 + (c & 1) * 16 + 8 * hb);
#pragma unroll
            for (int c = 0; c < 4; ++c) G.qh[c] = ld8u(p + 128 + (c >> 1) * 32 + (c & 1) * 16 + 8 * hb);
            G.sc = ld16u(p + 192);
            G.d  = (uint32_t) *(const uint16_t *) (p + 208);
        };
        auto fetch_a = [&](int b, ablk & G) {
            const char * ab = acol + (size_t) b * 256 + 8 * hb;
#pragma unroll
            for (int t = 0; t < 16; ++t) G.av[t] = *(const u32x2 *) (ab + t * 16);
        };
        auto reduce = [&](int b, const wblk & G, const ablk & GA) {
            i32x16 acc, corr;
#pragma unroll
            for (int e = 0; e < 16; ++e) { acc[e] = 0; corr[e] = 0; }
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                // sub-block s: half n = s/8, value group q = (s%8)/2 (ql nibble / qh bit pair), is = s%2  (dequantize_row_q6_K, ggml-quants.c:1762-1791)
                const int n = s >> 3, q = (s & 7) >> 1, is = s & 1;
                const u32x2 av = GA.av[s];
                const u32x2 l = G.ql[n * 4 + (q & 1) * 2 + is], h = G.qh[n * 2 + is];
                const int scs = (int) (int8_t) ((G.sc[s >> 2] >> (8 * (s & 3))) & 0xff);
                union { u32x2 u; long l; } wv, sv, aa;
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    wv.u[e] = ((l[e] >> (4 * (q >> 1))) & 0x0f0f0f0fu) | (((h[e] >> (2 * q)) & 0x03030303u) << 4);
                    sv.u[e] = (uint32_t) (scs & 0xff) * 0x01010101u;
                }
                aa.u = av;
                i32x16 z;
#pragma unroll
                for (int e = 0; e < 16; ++e) z[e] = 0;
                const i32x16 sj = __builtin_amdgcn_mfma_i32_32x32x16_i8(aa.l, wv.l, z, 0, 0, 0);
                corr = __builtin_amdgcn_mfma_i32_32x32x16_i8(aa.l, sv.l, corr, 0, 0, 0);
#pragma unroll
                for (int e = 0; e < NT * 4; ++e) acc[e] += __mul24(sj[e], scs);
            }
            const float d = h2f((uint16_t) G.d);
#pragma unroll
            for (int g = 0; g < NT; ++g) {
                const f32x4 y4 = *(const f32x4 *) (yd + b * 32 + 8 * g + 4 * hb);
#pragma unroll
                for (int i = 0; i < 4; ++i) out[4 * g + i] += y4[i] * (d * (float) (acc[4 * g + i] - 32 * corr[4 * g + i]));
            }
        };
        // weights ring: RD - 1 blocks of this lane's row in flight ahead of the one being reduced (HBM latency ~2 us, a block's
        // arithmetic well under 1 us); the tokens' int8 come from L2 at use
        constexpr int RD = 3;
        wblk R[RD]; ablk GA;
        const int nb_w = wave < nblk ? (nblk - wave + KS - 1) / KS : 0;         // this wave's blocks: wave, wave + KS, ...
#pragma unroll
        for (int u = 0; u < RD - 1; ++u) if (u < nb_w) fetch(wave + u * KS, R[u]);
        stage_scales();
        for (int i0 = 0; i0 < nb_w; i0 += RD) {
#pragma unroll
            for (int u = 0; u < RD; ++u) {
                const int i = i0 + u;
                if (i < nb_w) {
                    if (i + RD - 1 < nb_w) fetch(wave + (i + RD - 1) * KS, R[(u + RD - 1) % RD]);
                    fetch_a(wave + i * KS, GA);
                    reduce(wave + i * KS, R[u], GA);
                }
            }
        }
    }
}

// Folds the KS waves' partial sums (same lane layout) into wave 0's out[] through `red` (LDS [KS - 1][64][NT * 4]), in wave order; false: this wave is done
template <int NT, int KS>
static __device__ __forceinline__ bool mmq_fold(float * red, float (&out)[NT * 4], const int wave, const int lane) {
    if (KS > 1) {
        if (wave > 0) {
            float * mine = red + ((size_t) (wave - 1) * 64 + lane) * (NT * 4);
#pragma unroll
            for (int g = 0; g < NT; ++g) *(f32x4 *) (mine + 4 * g) = f32x4{ out[4 * g], out[4 * g + 1], out[4 * g + 2], out[4 * g + 3] };
        }
        __syncthreads();
        if (wave > 0) return false;
#pragma unroll
        for (int w = 1; w < KS; ++w) {
            const float * oth = red + ((size_t) (w - 1) * 64 + lane) * (NT * 4);
#pragma unroll
            for (int g = 0; g < NT; ++g) {
                const f32x4 o4 = *(const f32x4 *) (oth + 4 * g);
#pragma unroll
                for (int i = 0; i < 4; ++i) out[4 * g + i] += o4[i];
            }
        }
    }
    return true;
}

} // namespace mi
