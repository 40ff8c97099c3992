// fattn_q.hip -- FLASH_ATTN_EXT on the matrix cores over a QUANTISED KV cache: Q8_0 or Q4_0 K / V (alike), head size 64 or 128, f32 Q, one kernel for decode
// and prefill.  What fa_q_plan (fattn.hip) refuses -- ALiBi, a mask per head, other head sizes, BF16 / F32 caches -- stays on k_fattn_any.
//
// Arithmetic restates what the head of fattn_any.hip restates (ggml_compute_forward_flash_attn_ext_f16, ops.cpp:7912-8148), on the matrix cores:
//   q -> Q8_0 blocks INSIDE the kernel (quantize_row_q8_0: per 32 elements d = amax / 127 rounded to f16 and back, qs = rintf(x * (127 / amax)), as k_fattn_any).
//     A lane owns one query column and one K half hb (elements 16 hb .. 16 hb + 15 of every block): the block's amax is the maximum of its 16 values and those
//     of lane ^ 32.
//   scores: ONE __builtin_amdgcn_mfma_i32_32x32x32_i8 per 32-element block is the reference's sumi (ggml_vec_dot_q8_0_q8_0 / _q4_0_q8_0) for 32 cache rows x 32
//     query columns -- the MFMA's K extent is exactly one block; operand layout of mmq_id.hip's stepped body (half hb holds elements 16 hb .. 16 hb + 15).  Q8_0
//     K bytes as they are, Q4_0 nibbles unpacked to n - 8 as int8 while the tile is staged (q40_dec's bit trick).  Then s += (float) sumi * (d_k * d_q) in f32,
//     block by block: the f32 accumulator is never handed to the MFMA.  Computed transposed (S^T = K . Q^T) as in fattn_wide.hip: a lane owns one query column
//     and its 16 accumulator registers are 16 cache rows.
//   soft-max as k_fattn_wide: f32, online, base-2 exponentials; scale [-> softcap * tanh] + mask; sinks folded at the end, then 1 / S.
//   P . V in F32 on __builtin_amdgcn_mfma_f32_32x32x2f32 (as gemm_any.hip): the reference accumulates a quantised V in f32, and the bar of these nodes is NMSE
//     1e-9 against it -- P rounded to f16 gives ~1e-7.  O^T = V^T . P^T in 16 steps per 32-dim block of O^T: step j contracts the two cache rows that register j
//     of the hb = 0 and hb = 1 lanes of the S^T accumulator hold, so the soft-max output registers ARE the B operand (no LDS round trip for P).  The A operand
//     is V de-quantised, d_v * (float) q, exact in f32 for both types.  An eighth of the f16 MFMA rate, accepted: decode is bound by the cache traffic and
//     prefill is still far ahead of a wave per row.  The split-P f16 form (hi + lo) was NOT tried.
//   A block scale that is inf / NaN (an uninitialised cell behind the mask) is staged as 0: the reference skips masked cells, a 0 * NaN must not leak in.
//
// Tiling: fattn_wide.hip's.  A column tile is 32 (token, head) pairs that share one KV head (gq < 32: 32 / gq tokens x gq heads, idle columns when gq does not
// divide 32; gq >= 32: 32 heads of one token).  A workgroup is four waves on four consecutive column tiles of one KV head and sequence; waves past the last
// column tile only help staging.  Each 32-row K tile and V tile is staged ONCE per workgroup in LDS by the 256 threads -- thread c takes the 16 quants of
// (row c / (2 NB), block (c / 2) % NB, half c % 2), NB = D / 32; the half-0 thread also writes the block scale -- as int8 rows of pitch D + 16 bytes plus f32
// scales [32][NB].  K and V tiles have the same layout: V is read row-major, one byte per lane and step.  The global loads are register-staged and overlap
// the other operand's matrix work: V(t) in flight under K(t) . Q, K(t + 1) under P . V(t).  Per live tile two barriers, single-buffered LDS.
// LDS: 2 x (32 x (D + 16) + 32 x NB x 4) + 512 (bitmap) = 10 752 bytes (128), 6 144 bytes (64): no attribute, several workgroups per CU.
// LDS banks (bank = dword address mod 64; ds_read_b128 goes in four 16-lane groups, a group conflict-free iff its 16-byte slots differ mod 16).  K fragment:
//   lane (lq, hb) reads the 16 bytes at row lq, block b, half hb: slot lq * (D + 16) / 16 + 2 b + hb; (D + 16) / 16 = 9 (128) or 5 (64) is odd, so the 16 rows
//   of a group take 16 different slots.  V bytes: lanes lq = 0 .. 31 of half hb read 32 consecutive bytes (8 dwords) of row r + 4 hb; the halves lie
//   4 x (D + 16) / 4 = 144 or 80 dwords = 16 mod 64 apart: disjoint banks.  Scales: a wave reads two addresses (one per half): broadcast.  The staging writes
//   are 16-byte writes to consecutive slots of a row.  Derived from the bank rule, not counted: no counter run was made.
// Alignment: Q8_0 / Q4_0 rows are 34- / 18-byte blocks, so rows, head strides and the base are only 2-byte aligned (the plan refuses odd ones); every load
//   stays inside one block at whatever alignment it has (a 2-byte-aligned 16-byte load of the quants, a 2-byte load of d), as mmq_id.hip's decoders.
// Bounds: rows past n_kv and columns past the last (token, head) pair are CLAMPED to a valid index before any address is formed; such a row is staged as
//   zeros, its probability is zero (mask word 0xfc00) and such a column's output is not stored.
// Registers (-Rpass-analysis=kernel-resource-usage, gfx950; VGPR / AGPR, plain and soft-cap instance; scratch 0 in every instance, no spill to memory):
//   128 q8_0: 256 / 92, 256 / 92    128 q4_0: 256 / 92, 256 / 92    64 q8_0: 166 / 64, 168 / 64    64 q4_0: 167 / 64, 168 / 64
//   (one wave per SIMD at 128 -- the unrolled P . V keeps its 64 V bytes and scales in flight --, two at 64).  Built with -packed-fp32-ops off (Makefile): no
//   packed-f32 instruction beside the MFMAs, the concern -fno-slp-vectorize answers for fattn_wide.o.
// Mask, live-tile bitmap and KV slices: as fattn_wide.hip (a.part [column][slice][D + 2], natural-log M; k_fattn_merge<64 / 128> folds).
#include "fattn_dev.hpp"

namespace mi {

typedef float fq_f16a __attribute__((ext_vector_type(16)));
typedef int   fq_i16a __attribute__((ext_vector_type(16)));
typedef int   fq_i4   __attribute__((ext_vector_type(4)));
typedef u32x4 __attribute__((aligned(2))) fq_u32x4a2;   // (blocks and rows of the f16-header formats are 2-byte aligned)

constexpr int   FQ_KT = 32;                      // KV rows per tile
constexpr int   FQ_NW = 4;                       // waves per workgroup = column tiles per workgroup
constexpr int   FQ_MAXT = 4096;                  // live-tile bitmap capacity: n_kv <= 131072
constexpr float FQ_LOG2E = 1.4426950408889634f;

template <int D, int T, bool CAP>
__global__ void __launch_bounds__(64 * FQ_NW) k_fattn_q(const fa_dev a, const int nct) {
    static_assert(D == 64 || D == 128, "head size");
    static_assert(T == GGML_TYPE_Q8_0 || T == GGML_TYPE_Q4_0, "cache type");
    constexpr int NB  = D / 32;                  // blocks per row = MFMA steps of the scores = 32-dim blocks of O^T
    constexpr int BB  = T == GGML_TYPE_Q8_0 ? 34 : 18;   // bytes per block
    constexpr int LD  = D + 16;                  // tile row pitch in bytes ((D + 16) / 16 odd)
    constexpr int NT  = 64 * FQ_NW;
    constexpr int NCH = FQ_KT * NB * 2;          // 16-quant chunks per tile: 256 (128) or 128 (64) -- at most one per thread
    static_assert(NCH <= NT, "one chunk per thread");
    __shared__ __attribute__((aligned(16))) int8_t Kq[FQ_KT * LD];
    __shared__ __attribute__((aligned(16))) int8_t Vq[FQ_KT * LD];
    __shared__ __attribute__((aligned(16))) float  Kd[FQ_KT * NB];
    __shared__ __attribute__((aligned(16))) float  Vd[FQ_KT * NB];
    __shared__ uint32_t live[FQ_MAXT / 32];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lq = lane & 31, hb = lane >> 5;
    int b = (int) blockIdx.x;
    const int ncg = (nct + FQ_NW - 1) / FQ_NW;
    const int sp  = b % a.nsplit; b /= a.nsplit;
    const int cg  = b % ncg;      b /= ncg;
    const int ikv = b % a.nhkv;   const int is3 = b / a.nhkv;
    const int ct  = cg * FQ_NW + wave;
    const bool active = ct < nct;                         // (wave-uniform)
    int tok, hh; bool row_ok;
    if (a.gq >= 32) { const int tpt = (a.gq + 31) / 32; tok = ct / tpt; hh = (ct % tpt) * 32 + lq; row_ok = active && hh < a.gq && tok < a.nq; }
    else            { tok = ct * a.qpw + lq / a.gq; hh = lq % a.gq; row_ok = active && lq < a.qpw * a.gq && tok < a.nq; }
    const int q = row_ok ? tok : 0;
    const int h = ikv * a.gq + (row_ok ? hh : 0);

    const int ntile = (a.nkv + FQ_KT - 1) / FQ_KT;
    const int tps  = (ntile + a.nsplit - 1) / a.nsplit;
    const int t_lo = sp * tps < ntile ? sp * tps : ntile;
    const int t_hi = (sp + 1) * tps < ntile ? (sp + 1) * tps : ntile;

    const float c2 = CAP ? a.scale * 2.0f * FQ_LOG2E : a.scale * FQ_LOG2E;      // CAP: 2 x log2(e) x the score before the cap, for tanh below
    const float cap2 = a.logit_softcap * FQ_LOG2E;
    const uint16_t * mrow = a.mask ? (const uint16_t *) (a.mask + q * a.mnb1 + (is3 % (int) a.mne3) * a.mnb3) : nullptr;   // (plan: mask ne2 == 1)
    const bool mask_vec = a.mask && a.mnb1 % 8 == 0 && a.mnb3 % 8 == 0 && ((uintptr_t) a.mask) % 8 == 0;     // (uniform: every column's row is 8-byte aligned)

    // mask words of this lane's column in tile t: word pair g = cells t*32 + 4*hb + 8*g + {0..3}; cells past n_kv read as -inf
    auto load_mask = [&](const int t, u32x2 (&mw)[4]) {
        if (t * FQ_KT + FQ_KT <= a.nkv && (!mrow || mask_vec)) {             // (uniform) a whole tile, vector loads
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                if (mrow) mw[g] = *(const u32x2 *) (mrow + t * FQ_KT + 4 * hb + 8 * g); else { mw[g][0] = 0u; mw[g][1] = 0u; }
            }
        } else {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int kvb = t * FQ_KT + 4 * hb + 8 * g;
                uint32_t hv[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) { const int kc = kvb + i < a.nkv ? kvb + i : a.nkv - 1; hv[i] = mrow ? (uint32_t) mrow[kc] : 0u; if (kvb + i >= a.nkv) hv[i] = 0xfc00u; }
                mw[g][0] = hv[0] | (hv[1] << 16); mw[g][1] = hv[2] | (hv[3] << 16);
            }
        }
    };

    // ---- live-tile bitmap of this slice (bit t - t_lo)
    for (int i = tid; i < FQ_MAXT / 32; i += NT) live[i] = a.mask ? 0u : 0xffffffffu;
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

    // ---- staging: this thread's chunk (row, block, half) of a tile: the 16 quants as int8 and, in the half-0 thread, the block scale
    const int  srow = tid / (2 * NB), sblk = (tid >> 1) % NB, shb = tid & 1;
    const bool stager = NCH == NT || tid < NCH;
    const char * kbase = a.k + ikv * a.knb2 + is3 * a.knb3 + sblk * BB;
    const char * vbase = a.v + ikv * a.vnb2 + is3 * a.vnb3 + sblk * BB;
    struct chunk { u32x4 q; uint32_t d; };
    auto load_chunk = [&](const char * base, const int64_t nb1, const int t) {
        chunk c = { u32x4{ 0u, 0u, 0u, 0u }, 0u };
        if (!stager) return c;
        const int  kv = t * FQ_KT + srow;
        const bool ok = kv < a.nkv;
        const char * bp = base + (int64_t) (ok ? kv : a.nkv - 1) * nb1;
        c.q = *(const fq_u32x4a2 *) (bp + 2 + (T == GGML_TYPE_Q8_0 ? 16 * shb : 0));
        c.d = (uint32_t) *(const uint16_t *) bp;
        if (!ok) { c.q = u32x4{ 0u, 0u, 0u, 0u }; c.d = 0u; }
        return c;
    };
    auto store_chunk = [&](int8_t * qs, float * ds, const chunk & c) {
        if (!stager) return;
        u32x4 w = c.q;
        if (T == GGML_TYPE_Q4_0) {                          // nibble - 8 as int8: with y = n ^ 8, y with its bit 3 copied into bits 4..7 (mmq_id.hip q40_dec)
#pragma unroll
            for (int e = 0; e < 4; ++e) { const uint32_t y = ((c.q[e] >> (4 * shb)) & 0x0f0f0f0fu) ^ 0x08080808u; w[e] = y | ((y & 0x08080808u) * 30u); }
        }
        *(u32x4 *) (qs + srow * LD + sblk * 32 + shb * 16) = w;
        if (shb == 0) ds[srow * NB + sblk] = (c.d & 0x7c00u) == 0x7c00u ? 0.0f : h2f((uint16_t) c.d);
    };

    int t = next_live(t_lo);
    chunk kc = { u32x4{ 0u, 0u, 0u, 0u }, 0u }, vc;
    if (t < t_hi) kc = load_chunk(kbase, a.knb1, t);       // in flight under the Q loads

    // ---- Q fragment: B operand, lane (column lq, half hb) holds elements 32 b + 16 hb + {0..15} of its query row as Q8_0 quants, and the blocks' d
    fq_i4 qf[NB]; float qd[NB];
#pragma unroll
    for (int bk = 0; bk < NB; ++bk) { qf[bk] = fq_i4{ 0, 0, 0, 0 }; qd[bk] = 0.0f; }
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
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                uint32_t w = 0u;
#pragma unroll
                for (int i = 0; i < 4; ++i) w |= ((uint32_t) (int) rintf(x[g][i] * id) & 0xffu) << (8 * i);
                qf[bk][g] = (int) w;
            }
        }
    }

    fq_f16a acc_o[NB];
#pragma unroll
    for (int db = 0; db < NB; ++db)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc_o[db][e] = 0.0f;
    float M = -INFINITY, S = 0.0f;

    while (t < t_hi) {
        store_chunk(Kq, Kd, kc);
        vc = load_chunk(vbase, a.vnb1, t);                 // in flight under the score product
        u32x2 mw[4];
        if (active) load_mask(t, mw);
        __syncthreads();                                   // K(t) visible; every wave is past P.V(t - 1): the V tile may be overwritten below
        float alpha = 1.0f;
        fq_f16a sc;
#pragma unroll
        for (int e = 0; e < 16; ++e) sc[e] = 0.0f;
        if (active) {
            // ---- S^T = K . Q^T: the integer sum of every block, then its two scales; sc[e] is cell (e & 3) + 8 * (e >> 2) + 4 * hb of the tile
#pragma unroll
            for (int bk = 0; bk < NB; ++bk) {
                const u32x4 kw = *(const u32x4 *) (Kq + lq * LD + bk * 32 + hb * 16);
                const fq_i4 kf = fq_i4{ (int) kw[0], (int) kw[1], (int) kw[2], (int) kw[3] };
                fq_i16a z;
#pragma unroll
                for (int e = 0; e < 16; ++e) z[e] = 0;
                const fq_i16a sumi = __builtin_amdgcn_mfma_i32_32x32x32_i8(kf, qf[bk], z, 0, 0, 0);
#pragma unroll
                for (int e = 0; e < 16; ++e) sc[e] += (float) sumi[e] * (Kd[((e & 3) + 8 * (e >> 2) + 4 * hb) * NB + bk] * qd[bk]);
            }
            // ---- scale / softcap / mask, base-2 online soft-max
            float tmax = -INFINITY;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const uint32_t w = mw[e >> 2][(e >> 1) & 1];
                const uint16_t hbits = (uint16_t) ((e & 1) ? (w >> 16) : (w & 0xffffu));
                float v = sc[e] * c2;
                if (CAP) v = cap2 - 2.0f * cap2 * __builtin_amdgcn_rcpf(__builtin_amdgcn_exp2f(v) + 1.0f);     // cap * tanh(x) = cap * (1 - 2 / (e^2x + 1)), branch-free; +-cap at +-inf
                v = (hbits == 0xfc00u || !row_ok) ? -INFINITY : v + FQ_LOG2E * h2f(hbits);
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
        store_chunk(Vq, Vd, vc);
        const int tn = next_live(t + 1);
        if (tn < t_hi) kc = load_chunk(kbase, a.knb1, tn); // in flight under P.V
        __syncthreads();                                   // V(t) visible; every wave is past K(t).Q: the K tile may be overwritten at the top
        if (active) {
            if (!__all(alpha == 1.0f)) {
#pragma unroll
                for (int db = 0; db < NB; ++db)
#pragma unroll
                    for (int e = 0; e < 16; ++e) acc_o[db][e] *= alpha;
            }
            // ---- O^T += V^T . P^T in f32: step j contracts cache rows (j & 3) + 8 * (j >> 2) (k = 0: the hb = 0 lanes) and + 4 (k = 1: the hb = 1 lanes);
            //      A: lane (dim lq of block db, hb) supplies d_v * q of its row, B: register j of P^T
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int r = (j & 3) + 8 * (j >> 2) + 4 * hb;
#pragma unroll
                for (int db = 0; db < NB; ++db) {
                    const float va = Vd[r * NB + db] * (float) (int) Vq[r * LD + db * 32 + lq];
                    acc_o[db] = __builtin_amdgcn_mfma_f32_32x32x2f32(va, sc[j], acc_o[db], 0, 0, 0);
                }
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
        const float sk = a.sinks[h] * FQ_LOG2E;
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

static long g_fq_launches = 0;
long fattn_q_launches() { return g_fq_launches; }
int  fattn_q_max_tiles() { return FQ_MAXT; }

template <int D, int T>
static void fq_go(const fa_dev & a0, hipStream_t st) {
    fa_dev a = a0;
    a.qpw = a.gq < 32 ? 32 / a.gq : 1;                                         // tokens per column tile
    const int nct = a.gq >= 32 ? a.nq * ((a.gq + 31) / 32) : (a.nq + a.qpw - 1) / a.qpw;
    const int ncg = (nct + FQ_NW - 1) / FQ_NW;                                 // workgroups per (KV head, sequence, slice)
    const dim3 grid((unsigned) ((int64_t) a.nsplit * ncg * a.nhkv * a.ns));
    if (a.logit_softcap != 0.0f) k_fattn_q<D, T, true><<<grid, dim3(64 * FQ_NW), 0, st>>>(a, nct);
    else                         k_fattn_q<D, T, false><<<grid, dim3(64 * FQ_NW), 0, st>>>(a, nct);
    ++g_fq_launches;
}

void flash_attn_ext_q(const fa_dev & a, int D, int kv_type, hipStream_t st) {
    if (D == 128 && kv_type == GGML_TYPE_Q8_0) fq_go<128, GGML_TYPE_Q8_0>(a, st);
    else if (D == 128 && kv_type == GGML_TYPE_Q4_0) fq_go<128, GGML_TYPE_Q4_0>(a, st);
    else if (D == 64 && kv_type == GGML_TYPE_Q8_0) fq_go<64, GGML_TYPE_Q8_0>(a, st);
    else if (D == 64 && kv_type == GGML_TYPE_Q4_0) fq_go<64, GGML_TYPE_Q4_0>(a, st);
    else { fprintf(stderr, "[mi355x] flash_attn: no quantised-cache kernel for head size %d, type %d\n", D, kv_type); abort(); }
}

} // namespace mi
