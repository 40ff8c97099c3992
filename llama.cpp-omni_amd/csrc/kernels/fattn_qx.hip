// fattn_qx.hip -- FLASH_ATTN_EXT on the matrix cores over a quantised KV cache whose K and V types DIFFER, or are Q4_1 / Q5_0 / Q5_1: K one of Q8_0 / Q4_0 /
// Q4_1 / Q5_0 / Q5_1, V one of those or F16 (what -ctk / -ctv give: -ctk q8_0 alone leaves V in F16), head size 64 or 128, f32 Q.  The pairs Q8_0 / Q8_0 and
// Q4_0 / Q4_0 are NOT taken: they stay on k_fattn_q (fattn_q.hip).  What fa_qx_plan (fattn.hip) refuses -- ALiBi, a mask per head, other head sizes, F16 K
// over a quantised V -- stays on k_fattn_any.
//
// The frame is fattn_q.hip's, line by line: column tiles of 32 (token, head) pairs, four waves on four column tiles, 32-row KV tiles staged once per workgroup
// by the 256 threads, S^T = K . Q^T with ONE __builtin_amdgcn_mfma_i32_32x32x32_i8 per 32-element block and the float fold per block, the online base-2
// soft-max, the live-tile bitmap, KV slices folded by k_fattn_merge, clamped indices, a non-finite block scale (or min) staged as 0.  What differs:
//   K staging decoders.  Every K type lands in LDS in ONE tile format, so the score loop has no type in it: int8 rows (pitch D + 16) plus f32 d [32][NB], and
//     f32 m beside d ([32][NB][2]) where the type has a min (template KM).  Q8_0: the bytes; Q4_0: n - 8; Q5_0: (n | bit << 4) - 16 with the block's qh bit;
//     Q4_1: n = 0 .. 15; Q5_1: n | bit << 4 = 0 .. 31 -- the integers ggml_vec_dot_q{8_0,4_0,5_0}_q8_0 / _q{4_1,5_1}_q8_1 multiply (ggml-cpu/quants.c:152-303).
//     The decoder is chosen by a wave-uniform switch on the type (a kernel argument), under the template's "has a min" class.
//   Query image.  For Q4_1 / Q5_1 K the query is quantised in Q8_1 form (quantize_row_q8_1 as the x86 build compiles it): the Q8_0 quants and d, and
//     s = f16(d * sum(qs)) per (column, block) with d NOT yet rounded; the sum comes over the same lane ^ 32 exchange as amax.  A block's score is
//     (d_k * d_q) * (float) sumi + m_k * s_q (ggml_vec_dot_q4_1_q8_1), folded in f32 block by block.
//   V tile.  V is de-quantised ONCE, while the tile is staged, to f32 rows in LDS: d * q [+ m] (dequantize_row_q*, ggml-quants.c:307-398), (float) h for F16
//     (an inf / NaN half behind the mask is staged as 0, like a scale).  P . V on __builtin_amdgcn_mfma_f32_32x32x2f32 then reads ready A operands: one
//     ds_read_b32 per MFMA, and the four waves no longer each convert the same bytes.  V is accumulated in f32 for every V type -- the reference does so for
//     every type but F16, where it rounds its accumulator to f16 at each cell; that node's bar is the F16 cache's NMSE 5e-4, the others' 1e-9.
// Staging: thread c takes (row c / (2 NB), block (c / 2) % NB, half c % 2) of the K tile and of the V tile: 16 quants (one 16-byte load: the half's bytes of
//   Q8_0, the block's 16 nibble bytes otherwise, from which the half takes its nibble) or 16 halfs (two 16-byte loads), plus d [, m] [, qh] as 2-byte loads.
//   Register-staged and overlapped as in fattn_q.hip: V(t) in flight under K(t) . Q, K(t + 1) under P . V(t); two barriers per live tile, single-buffered LDS.
// LDS: K 32 x (D + 16) + 32 x NB x 4 (x 2 with a min), V 32 x (D + 8) x 4, bitmap 512: 128: 23 040 + 512 (KM) bytes, 64: 12 544 + 256 (KM).  Static, no attribute.
//   At 128 the register budget (one wave per SIMD, below) already limits a CU to one workgroup per four SIMDs' worth of waves; LDS is not the limit.
// LDS banks (bank = dword address mod 64).  K fragment and K scales: fattn_q.hip's ((D + 16) / 16 odd; d / (d, m) reads are two addresses per wave: broadcast).
//   V operand: lane (lq, hb) of step j reads dword (r + 4 hb) * (D + 8) + 32 db + lq, r = (j & 3) + 8 (j >> 2): the 32 lanes of a half read 32 consecutive
//   dwords, and the halves lie 4 x (D + 8) = 544 / 288 dwords = 32 mod 64 apart: the 64 lanes take the 64 banks once.  This is why the pitch is D + 8 and not
//   D: at pitch D the halves would collide bank for bank.  The staging writes are four 16-byte writes per thread to consecutive slots of one row.  Derived from
//   the bank rule, not counted: no counter run was made.
// Alignment: blocks are 34 / 18 / 20 / 22 / 24 bytes, so rows, head strides and the base are only 2-byte aligned (the plan refuses odd ones); every load stays
//   inside one block at whatever alignment it has.  An F16 V row is read as 16-byte loads of 2-byte alignment as well.
// Bounds: rows past n_kv and columns past the last (token, head) pair are CLAMPED to a valid index before any address is formed; such a row is staged as zeros,
//   its probability is zero (mask word 0xfc00) and such a column's output is not stored.
// Mask, live-tile bitmap and KV slices: as fattn_q.hip (a.part [column][slice][D + 2], natural-log M; k_fattn_merge<64 / 128> folds).
// Instances: head size x soft-cap x "K has a min" x "V has a min" = 16 kernels; the object builds in 9 s (one hipcc, -O3).  Registers
//   (-Rpass-analysis=kernel-resource-usage, gfx950; VGPR / AGPR, plain and soft-cap instance; scratch 0 in EVERY instance: the AGPRs are the spill space, no memory):
//   128, K no min: V no min 256 / 100, 256 / 101; V min 256 / 98, 256 / 100      128, K min: V no min 256 / 158, 256 / 160; V min 256 / 156, 256 / 158
//    64, K no min: V no min 172 / 64, 174 / 64;   V min 170 / 64, 172 / 64        64, K min: V no min 206 / 48, 208 / 48;   V min 202 / 48, 204 / 48
//   (one wave per SIMD at 128, two at 64, as k_fattn_q).  LDS as reported: 23 040 / 23 552 (128, without / with a K min), 12 544 / 12 800 (64).  Built with
//   -packed-fp32-ops off (Makefile): no packed-f32 instruction in the object.
#include "fattn_dev.hpp"

namespace mi {

typedef float fx_f16a __attribute__((ext_vector_type(16)));
typedef int   fx_i16a __attribute__((ext_vector_type(16)));
typedef int   fx_i4   __attribute__((ext_vector_type(4)));
typedef float fx_f2   __attribute__((ext_vector_type(2)));
typedef u32x4 __attribute__((aligned(2))) fx_u32x4a2;   // (blocks and rows of the f16-header formats are 2-byte aligned)

constexpr int   FX_KT = 32;                      // KV rows per tile
constexpr int   FX_NW = 4;                       // waves per workgroup = column tiles per workgroup
constexpr int   FX_MAXT = 4096;                  // live-tile bitmap capacity: n_kv <= 131072
constexpr float FX_LOG2E = 1.4426950408889634f;

static __host__ __device__ __forceinline__ int fx_block_bytes(const int type) {          // F16: the 32 halfs a "block" of the staging is
    return type == GGML_TYPE_Q8_0 ? 34 : type == GGML_TYPE_Q4_0 ? 18 : type == GGML_TYPE_Q4_1 ? 20 : type == GGML_TYPE_Q5_0 ? 22 : type == GGML_TYPE_Q5_1 ? 24 : 64;
}

// what a staging thread holds of its (row, block, half): quantised -- a = the 16 quant bytes (Q8_0: of the half, else the block's nibble bytes), b[0] = d | m << 16,
// b[1] = qh; F16 -- a, b = the half's 16 halfs
struct fx_chunk { u32x4 a, b; };

// bp: the block (quantised) or the half's first element (F16); every load inside the block
static __device__ __forceinline__ fx_chunk fx_load(const int type, const char * bp, const int shb) {
    fx_chunk c;
    if (type == GGML_TYPE_F16) { c.a = *(const fx_u32x4a2 *) bp; c.b = *(const fx_u32x4a2 *) (bp + 16); return c; }
    const bool has_m = type == GGML_TYPE_Q4_1 || type == GGML_TYPE_Q5_1, has_h = type == GGML_TYPE_Q5_0 || type == GGML_TYPE_Q5_1;
    const int  hoff = has_m ? 4 : 2, qoff = hoff + (has_h ? 4 : 0);
    c.a = *(const fx_u32x4a2 *) (bp + qoff + (type == GGML_TYPE_Q8_0 ? 16 * shb : 0));
    uint32_t dm = (uint32_t) *(const uint16_t *) bp, qh = 0u;
    if (has_m) dm |= (uint32_t) *(const uint16_t *) (bp + 2) << 16;
    if (has_h) qh = (uint32_t) *(const uint16_t *) (bp + hoff) | ((uint32_t) *(const uint16_t *) (bp + hoff + 2) << 16);
    c.b = u32x4{ dm, qh, 0u, 0u };
    return c;
}

// the half's 16 quants, one per byte, as the integers the reference's vec_dot / dequantize_row use: int8 for Q8_0, n - 8 for Q4_0, (n | bit << 4) - 16 for Q5_0,
// 0 .. 15 for Q4_1, 0 .. 31 for Q5_1.  The fifth bits of elements 16 shb + 4 e + {0..3} are qh's bits at that position: spread to bit 4 of the four bytes by a
// multiply (bit i -> bit 7 i + i = 8 i).  The sign: with y = v ^ top, y with its top bit copied into the bits above (mmq_id.hip q40_dec)
static __device__ __forceinline__ u32x4 fx_bytes(const int type, const fx_chunk & c, const int shb) {
    if (type == GGML_TYPE_Q8_0) return c.a;
    u32x4 w;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        uint32_t y = (c.a[e] >> (4 * shb)) & 0x0f0f0f0fu;
        if (type == GGML_TYPE_Q5_0 || type == GGML_TYPE_Q5_1) y |= ((((c.b[1] >> (16 * shb + 4 * e)) & 0xfu) * 0x00204081u) & 0x01010101u) << 4;
        if (type == GGML_TYPE_Q4_0) { y ^= 0x08080808u; y |= (y & 0x08080808u) * 30u; }
        if (type == GGML_TYPE_Q5_0) { y ^= 0x10101010u; y |= (y & 0x10101010u) * 14u; }
        w[e] = y;
    }
    return w;
}
static __device__ __forceinline__ float fx_scale(const uint32_t h) { return (h & 0x7c00u) == 0x7c00u ? 0.0f : h2f((uint16_t) h); }      // inf / NaN (a cell never written): 0

template <int D, bool CAP, bool KM, bool VM>
__global__ void __launch_bounds__(64 * FX_NW) k_fattn_qx(const fa_dev a, const int nct, const int kt, const int vt) {
    static_assert(D == 64 || D == 128, "head size");
    constexpr int NB  = D / 32;                  // blocks per row = MFMA steps of the scores = 32-dim blocks of O^T
    constexpr int LD  = D + 16;                  // K tile row pitch in bytes ((D + 16) / 16 odd)
    constexpr int LDV = D + 8;                   // V tile row pitch in floats (4 LDV = 32 mod 64)
    constexpr int KS  = KM ? 2 : 1;              // floats per (row, block) of the K scales: d [, m]
    constexpr int NT  = 64 * FX_NW;
    constexpr int NCH = FX_KT * NB * 2;          // 16-element chunks per tile: 256 (128) or 128 (64) -- at most one per thread
    static_assert(NCH <= NT, "one chunk per thread");
    __shared__ __attribute__((aligned(16))) int8_t Kq[FX_KT * LD];
    __shared__ __attribute__((aligned(16))) float  Kd[FX_KT * NB * KS];
    __shared__ __attribute__((aligned(16))) float  Vf[FX_KT * LDV];
    __shared__ uint32_t live[FX_MAXT / 32];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lq = lane & 31, hb = lane >> 5;
    int b = (int) blockIdx.x;
    const int ncg = (nct + FX_NW - 1) / FX_NW;
    const int sp  = b % a.nsplit; b /= a.nsplit;
    const int cg  = b % ncg;      b /= ncg;
    const int ikv = b % a.nhkv;   const int is3 = b / a.nhkv;
    const int ct  = cg * FX_NW + wave;
    const bool active = ct < nct;                         // (wave-uniform)
    int tok, hh; bool row_ok;
    if (a.gq >= 32) { const int tpt = (a.gq + 31) / 32; tok = ct / tpt; hh = (ct % tpt) * 32 + lq; row_ok = active && hh < a.gq && tok < a.nq; }
    else            { tok = ct * a.qpw + lq / a.gq; hh = lq % a.gq; row_ok = active && lq < a.qpw * a.gq && tok < a.nq; }
    const int q = row_ok ? tok : 0;
    const int h = ikv * a.gq + (row_ok ? hh : 0);

    const int ntile = (a.nkv + FX_KT - 1) / FX_KT;
    const int tps  = (ntile + a.nsplit - 1) / a.nsplit;
    const int t_lo = sp * tps < ntile ? sp * tps : ntile;
    const int t_hi = (sp + 1) * tps < ntile ? (sp + 1) * tps : ntile;

    const float c2 = CAP ? a.scale * 2.0f * FX_LOG2E : a.scale * FX_LOG2E;      // CAP: 2 x log2(e) x the score before the cap, for tanh below
    const float cap2 = a.logit_softcap * FX_LOG2E;
    const uint16_t * mrow = a.mask ? (const uint16_t *) (a.mask + q * a.mnb1 + (is3 % (int) a.mne3) * a.mnb3) : nullptr;   // (plan: mask ne2 == 1)
    const bool mask_vec = a.mask && a.mnb1 % 8 == 0 && a.mnb3 % 8 == 0 && ((uintptr_t) a.mask) % 8 == 0;     // (uniform: every column's row is 8-byte aligned)

    // mask words of this lane's column in tile t: word pair g = cells t*32 + 4*hb + 8*g + {0..3}; cells past n_kv read as -inf
    auto load_mask = [&](const int t, u32x2 (&mw)[4]) {
        if (t * FX_KT + FX_KT <= a.nkv && (!mrow || mask_vec)) {             // (uniform) a whole tile, vector loads
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                if (mrow) mw[g] = *(const u32x2 *) (mrow + t * FX_KT + 4 * hb + 8 * g); else { mw[g][0] = 0u; mw[g][1] = 0u; }
            }
        } else {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int kvb = t * FX_KT + 4 * hb + 8 * g;
                uint32_t hv[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) { const int kc = kvb + i < a.nkv ? kvb + i : a.nkv - 1; hv[i] = mrow ? (uint32_t) mrow[kc] : 0u; if (kvb + i >= a.nkv) hv[i] = 0xfc00u; }
                mw[g][0] = hv[0] | (hv[1] << 16); mw[g][1] = hv[2] | (hv[3] << 16);
            }
        }
    };

    // ---- live-tile bitmap of this slice (bit t - t_lo)
    for (int i = tid; i < FX_MAXT / 32; i += NT) live[i] = a.mask ? 0u : 0xffffffffu;
    __syncthreads();
    if (a.mask && active) {
        for (int t = t_lo; t < t_hi; ++t) {
            u32x2 mw[4];
            load_mask(t, mw);
            bool any = false;
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int i = 0; i < 2; ++i) any |= (mw[g][i] & 0xffffu) != 0xfc00u || (mw[g][i] >> 16) != 0xfc00u;
            any = any && row_ok;
            if (__any(any) && lane == 0) atomicOr(&live[(t - t_lo) >> 5], 1u << ((t - t_lo) & 31));
        }
    }
    __syncthreads();
    auto next_live = [&](int t) {
        while (t < t_hi && !((live[(t - t_lo) >> 5] >> ((t - t_lo) & 31)) & 1u)) ++t;
        return t;
    };

    // ---- staging: this thread's chunk (row, block, half) of a tile
    const int  srow = tid / (2 * NB), sblk = (tid >> 1) % NB, shb = tid & 1;
    const bool stager = NCH == NT || tid < NCH;
    const char * kbase = a.k + ikv * a.knb2 + is3 * a.knb3 + sblk * fx_block_bytes(kt);
    const char * vbase = a.v + ikv * a.vnb2 + is3 * a.vnb3 + sblk * fx_block_bytes(vt) + (vt == GGML_TYPE_F16 ? 32 * shb : 0);
    auto load_chunk = [&](const int type, const char * base, const int64_t nb1, const int t) {
        fx_chunk c = { u32x4{ 0u, 0u, 0u, 0u }, u32x4{ 0u, 0u, 0u, 0u } };
        if (!stager) return c;
        const int  kv = t * FX_KT + srow;
        const bool ok = kv < a.nkv;
        c = fx_load(type, base + (int64_t) (ok ? kv : a.nkv - 1) * nb1, shb);
        if (!ok) { c.a = u32x4{ 0u, 0u, 0u, 0u }; c.b = u32x4{ 0u, 0u, 0u, 0u }; }
        return c;
    };
    // K: int8 quants + d [, m]
    auto store_k = [&](const fx_chunk & c) {
        if (!stager) return;
        u32x4 w;
        if (KM) w = kt == GGML_TYPE_Q4_1 ? fx_bytes(GGML_TYPE_Q4_1, c, shb) : fx_bytes(GGML_TYPE_Q5_1, c, shb);
        else    w = kt == GGML_TYPE_Q8_0 ? fx_bytes(GGML_TYPE_Q8_0, c, shb) : kt == GGML_TYPE_Q4_0 ? fx_bytes(GGML_TYPE_Q4_0, c, shb) : fx_bytes(GGML_TYPE_Q5_0, c, shb);
        *(u32x4 *) (Kq + srow * LD + sblk * 32 + shb * 16) = w;
        if (shb == 0) {
            Kd[(srow * NB + sblk) * KS] = fx_scale(c.b[0] & 0xffffu);
            if (KM) Kd[(srow * NB + sblk) * KS + 1] = fx_scale(c.b[0] >> 16);
        }
    };
    // V: f32 values
    auto store_v = [&](const fx_chunk & c) {
        if (!stager) return;
        float * vr = Vf + srow * LDV + sblk * 32 + shb * 16;
        if (!VM && vt == GGML_TYPE_F16) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const uint32_t w0 = g < 2 ? c.a[2 * g] : c.b[2 * g - 4], w1 = g < 2 ? c.a[2 * g + 1] : c.b[2 * g - 3];
                *(f32x4 *) (vr + 4 * g) = f32x4{ fx_scale(w0 & 0xffffu), fx_scale(w0 >> 16), fx_scale(w1 & 0xffffu), fx_scale(w1 >> 16) };
            }
            return;
        }
        u32x4 w;
        if (VM) w = vt == GGML_TYPE_Q4_1 ? fx_bytes(GGML_TYPE_Q4_1, c, shb) : fx_bytes(GGML_TYPE_Q5_1, c, shb);
        else    w = vt == GGML_TYPE_Q8_0 ? fx_bytes(GGML_TYPE_Q8_0, c, shb) : vt == GGML_TYPE_Q4_0 ? fx_bytes(GGML_TYPE_Q4_0, c, shb) : fx_bytes(GGML_TYPE_Q5_0, c, shb);
        const float d = fx_scale(c.b[0] & 0xffffu), m = VM ? fx_scale(c.b[0] >> 16) : 0.0f;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f32x4 o4;
#pragma unroll
            for (int i = 0; i < 4; ++i) { const float x = d * (float) (int) (int8_t) (w[g] >> (8 * i)); o4[i] = VM ? x + m : x; }
            *(f32x4 *) (vr + 4 * g) = o4;
        }
    };

    int t = next_live(t_lo);
    fx_chunk kc = { u32x4{ 0u, 0u, 0u, 0u }, u32x4{ 0u, 0u, 0u, 0u } }, vc;
    if (t < t_hi) kc = load_chunk(kt, kbase, a.knb1, t);   // in flight under the Q loads

    // ---- Q fragment: B operand, lane (column lq, half hb) holds elements 32 b + 16 hb + {0..15} of its query row as Q8_0 quants, the blocks' d and -- KM -- their s
    fx_i4 qf[NB]; float qd[NB], qs[NB];
#pragma unroll
    for (int bk = 0; bk < NB; ++bk) { qf[bk] = fx_i4{ 0, 0, 0, 0 }; qd[bk] = 0.0f; qs[bk] = 0.0f; }
    if (active) {
        const char * qr = a.q + q * a.qnb1 + h * a.qnb2 + is3 * a.qnb3;
#pragma unroll
        for (int bk = 0; bk < NB; ++bk) {
            f32x4 x[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) x[g] = *(const f32x4 *) (qr + (bk * 32 + hb * 16 + g * 4) * 4);
            float amax = 0.0f;
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int i = 0; i < 4; ++i) amax = fmaxf(amax, fabsf(x[g][i]));
            amax = fmaxf(amax, __shfl_xor(amax, 32, 64));
            const float dq = amax / 127.0f, id = amax != 0.0f ? 127.0f / amax : 0.0f;
            qd[bk] = h2f(f2h(dq));
            int sum = 0;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                uint32_t w = 0u;
#pragma unroll
                for (int i = 0; i < 4; ++i) { const int qi = (int) rintf(x[g][i] * id); sum += qi; w |= ((uint32_t) qi & 0xffu) << (8 * i); }
                qf[bk][g] = (int) w;
            }
            if (KM) { sum += __shfl_xor(sum, 32, 64); qs[bk] = h2f(f2h(dq * (float) sum)); }          // block_q8_1.s
        }
    }

    fx_f16a acc_o[NB];
#pragma unroll
    for (int db = 0; db < NB; ++db)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc_o[db][e] = 0.0f;
    float M = -INFINITY, S = 0.0f;

    while (t < t_hi) {
        store_k(kc);
        vc = load_chunk(vt, vbase, a.vnb1, t);             // in flight under the score product
        u32x2 mw[4];
        if (active) load_mask(t, mw);
        __syncthreads();                                   // K(t) visible; every wave is past P.V(t - 1): the V tile may be overwritten below
        float alpha = 1.0f;
        fx_f16a sc;
#pragma unroll
        for (int e = 0; e < 16; ++e) sc[e] = 0.0f;
        if (active) {
            // ---- S^T = K . Q^T: the integer sum of every block, then its scales; sc[e] is cell (e & 3) + 8 * (e >> 2) + 4 * hb of the tile
#pragma unroll
            for (int bk = 0; bk < NB; ++bk) {
                const u32x4 kw = *(const u32x4 *) (Kq + lq * LD + bk * 32 + hb * 16);
                const fx_i4 kf = fx_i4{ (int) kw[0], (int) kw[1], (int) kw[2], (int) kw[3] };
                fx_i16a z;
#pragma unroll
                for (int e = 0; e < 16; ++e) z[e] = 0;
                const fx_i16a sumi = __builtin_amdgcn_mfma_i32_32x32x32_i8(kf, qf[bk], z, 0, 0, 0);
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const float * ks = Kd + (((e & 3) + 8 * (e >> 2) + 4 * hb) * NB + bk) * KS;
                    if (KM) { const fx_f2 dm = *(const fx_f2 *) ks; sc[e] += (dm[0] * qd[bk]) * (float) sumi[e] + dm[1] * qs[bk]; }
                    else    sc[e] += (float) sumi[e] * (ks[0] * qd[bk]);
                }
            }
            // ---- scale / softcap / mask, base-2 online soft-max
            float tmax = -INFINITY;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const uint32_t w = mw[e >> 2][(e >> 1) & 1];
                const uint16_t hbits = (uint16_t) ((e & 1) ? (w >> 16) : (w & 0xffffu));
                float v = sc[e] * c2;
                if (CAP) v = cap2 - 2.0f * cap2 * __builtin_amdgcn_rcpf(__builtin_amdgcn_exp2f(v) + 1.0f);     // cap * tanh(x) = cap * (1 - 2 / (e^2x + 1)), branch-free; +-cap at +-inf
                v = (hbits == 0xfc00u || !row_ok) ? -INFINITY : v + FX_LOG2E * h2f(hbits);
                sc[e] = v;
                tmax = fmaxf(tmax, v);
            }
            tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
            const float Mn = fmaxf(M, tmax);
            const float Mu = Mn == -INFINITY ? 0.0f : Mn;  // a column with nothing visible so far: exp2(-inf - 0) = 0, never -inf - -inf
            alpha = __builtin_amdgcn_exp2f(M - Mu);
            float psum = 0.0f;
#pragma unroll
            for (int e = 0; e < 16; ++e) { sc[e] = __builtin_amdgcn_exp2f(sc[e] - Mu); psum += sc[e]; }    // sc is P^T from here on
            S = S * alpha + psum;
            M = Mn;
        }
        store_v(vc);
        const int tn = next_live(t + 1);
        if (tn < t_hi) kc = load_chunk(kt, kbase, a.knb1, tn);     // in flight under P.V
        __syncthreads();                                   // V(t) visible; every wave is past K(t).Q: the K tile may be overwritten at the top
        if (active) {
            if (!__all(alpha == 1.0f)) {
#pragma unroll
                for (int db = 0; db < NB; ++db)
#pragma unroll
                    for (int e = 0; e < 16; ++e) acc_o[db][e] *= alpha;
            }
            // ---- O^T += V^T . P^T in f32: step j contracts cache rows (j & 3) + 8 * (j >> 2) (k = 0: the hb = 0 lanes) and + 4 (k = 1: the hb = 1 lanes);
            //      A: lane (dim lq of block db, hb) supplies the f32 value of its row, B: register j of P^T
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int r = (j & 3) + 8 * (j >> 2) + 4 * hb;
#pragma unroll
                for (int db = 0; db < NB; ++db) acc_o[db] = __builtin_amdgcn_mfma_f32_32x32x2f32(Vf[r * LDV + db * 32 + lq], sc[j], acc_o[db], 0, 0, 0);
            }
        }
        t = tn;
    }

    if (!row_ok) return;                                   // (no barrier below)
    S += __shfl_xor(S, 32, 64);                            // (row_ok is the same in both lane halves)
    if (a.nsplit > 1) {                                    // partial state of this slice, natural-log convention (k_fattn_merge)
        float * pr = a.part + ((((int64_t) is3 * a.nq + q) * a.nh + h) * a.nsplit + sp) * (D + 2);
#pragma unroll
        for (int db = 0; db < NB; ++db)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4 o4;
#pragma unroll
                for (int i = 0; i < 4; ++i) o4[i] = acc_o[db][4 * g + i];
                *(f32x4 *) (pr + db * 32 + 8 * g + 4 * hb) = o4;
            }
        if (hb == 0) { pr[D] = M * 0.6931471805599453f; pr[D + 1] = S; }
        return;
    }
    // ---- one slice: finish here -- sinks (ops.cpp:8116-8130), normalise, store permuted
    float osc = 1.0f;
    if (a.sinks) {
        const float sk = a.sinks[h] * FX_LOG2E;
        if (sk > M) { const float f = __builtin_amdgcn_exp2f(M - sk); S = S * f + 1.0f; osc = f; }
        else S += __builtin_amdgcn_exp2f(sk - M);
    }
    const float inv = S == 0.0f ? 0.0f : osc / S;
    char * out = a.dst + h * a.dnb1 + q * a.dnb2 + is3 * a.dnb3;
#pragma unroll
    for (int db = 0; db < NB; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f32x4 o4;
#pragma unroll
            for (int i = 0; i < 4; ++i) o4[i] = acc_o[db][4 * g + i] * inv;
            *(f32x4 *) (out + (db * 32 + 8 * g + 4 * hb) * 4) = o4;
        }
}

static long g_fx_launches = 0;
long fattn_qx_launches() { return g_fx_launches; }
int  fattn_qx_max_tiles() { return FX_MAXT; }

template <int D, bool KM, bool VM>
static void fx_go(const fa_dev & a0, int kt, int vt, hipStream_t st) {
    fa_dev a = a0;
    a.qpw = a.gq < 32 ? 32 / a.gq : 1;                                         // tokens per column tile
    const int nct = a.gq >= 32 ? a.nq * ((a.gq + 31) / 32) : (a.nq + a.qpw - 1) / a.qpw;
    const int ncg = (nct + FX_NW - 1) / FX_NW;                                 // workgroups per (KV head, sequence, slice)
    const dim3 grid((unsigned) ((int64_t) a.nsplit * ncg * a.nhkv * a.ns));
    if (a.logit_softcap != 0.0f) k_fattn_qx<D, true, KM, VM><<<grid, dim3(64 * FX_NW), 0, st>>>(a, nct, kt, vt);
    else                         k_fattn_qx<D, false, KM, VM><<<grid, dim3(64 * FX_NW), 0, st>>>(a, nct, kt, vt);
    ++g_fx_launches;
}

void flash_attn_ext_qx(const fa_dev & a, int D, int k_type, int v_type, hipStream_t st) {
    const bool km = k_type == GGML_TYPE_Q4_1 || k_type == GGML_TYPE_Q5_1, vm = v_type == GGML_TYPE_Q4_1 || v_type == GGML_TYPE_Q5_1;
    const bool k_ok = km || k_type == GGML_TYPE_Q8_0 || k_type == GGML_TYPE_Q4_0 || k_type == GGML_TYPE_Q5_0;
    const bool v_ok = vm || v_type == GGML_TYPE_Q8_0 || v_type == GGML_TYPE_Q4_0 || v_type == GGML_TYPE_Q5_0 || v_type == GGML_TYPE_F16;
    if ((D != 64 && D != 128) || !k_ok || !v_ok) { fprintf(stderr, "[mi355x] flash_attn: no mixed-type cache kernel for head size %d, K type %d, V type %d\n", D, k_type, v_type); abort(); }
#define FX_GO(DD) do { if (km) { if (vm) fx_go<DD, true, true>(a, k_type, v_type, st); else fx_go<DD, true, false>(a, k_type, v_type, st); } \
                       else    { if (vm) fx_go<DD, false, true>(a, k_type, v_type, st); else fx_go<DD, false, false>(a, k_type, v_type, st); } } while (0)
    if (D == 128) FX_GO(128); else FX_GO(64);
#undef FX_GO
}

} // namespace mi
