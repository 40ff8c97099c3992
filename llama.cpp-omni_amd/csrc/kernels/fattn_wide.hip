// fattn_wide.hip -- FLASH_ATTN_EXT on the matrix cores for the head sizes beside 64 / 128: (DK, DV) = (256, 256) (Gemma 2 / 3), (576, 512) (DeepSeek MLA
// after the absorption: one KV head, K rows 576 wide, V rows 512 wide), and the sizes that are no multiple of the MFMA extents: (40, 40), (72, 72) (SigLip-class
// towers), (80, 80) (Phi-2, StableLM-3B), (96, 96) (Phi-3-mini), (112, 112) and (192, 128) (DeepSeek V2 / V3 before the absorption).  F16 K / V, f32 Q, one
// kernel for decode and prefill.
//
// Arithmetic is fattn_mma.hip's (which restates ops.cpp:7912-8148): Q rounded to f16, s = K.q * scale [-> softcap * tanh] + mask, online
// soft-max in f32 with base-2 exponentials, P rounded to f16 for the second product, O in f32, sinks folded at the end, then 1 / S.
// Both products are v_mfma_f32_32x32x16_f16, computed transposed (S^T = K . Q^T, O^T = V^T . P^T) so that a lane owns one query column and
// the S^T accumulator registers, rounded to f16, are the B operand of the second product (see the head of fattn_mma.hip).
//
// Tiling.  A column tile is 32 (token, head) pairs that share one KV head, as in k_fattn_gqa: with gq = heads per KV head < 32 it is
// 32 / gq tokens x gq heads (gq that does not divide 32 leaves idle columns), with gq >= 32 it is 32 heads of one token.  A workgroup is
// four waves on consecutive column tiles of the same KV head and sequence.  Each 32-row K tile ([32][DK + 8] halfs) and V tile
// (transposed, [DV][34] halfs) is staged ONCE per workgroup in LDS by all 256 threads and read by the four waves.  Waves past the last
// column tile only help staging.
//   256 / 256: a wave owns one column tile: its whole Q fragment (64 registers) and all of O^T (128); four column tiles per workgroup.
//   576 / 512: O^T of 32 columns is 256 registers per lane and the Q fragment 144; with the staging registers that spilled at one wave
//     per SIMD.  So TWO waves share a column tile (NDH = 2; two column tiles per workgroup): wave dh computes the partial scores over
//     its half of DK, the pair exchanges the partial S^T through LDS and adds them in the same order (both hold the same bits), each
//     runs the same soft-max, and wave dh owns O^T for its half of DV (128 registers).  No matrix work is done twice.  The wave's Q
//     fragment (72 registers' worth) lives in lane-private LDS slots: with it in registers the compiler still spilled 140 - 160 bytes.
//     LDS: K 37376 + V^T 34816 + exchange 16384 + Q 73728 + 512 (bitmap) = 162816 of 163840 bytes: one workgroup per CU.
//     MLA decode (128 heads = 4 column tiles) reads a cache row twice per token -- once per workgroup -- not 128 times.
//   40 ... 112 and 192 / 128: as 256 / 256 (NDH = 1, four column tiles per workgroup) on PADDED extents: DKP = DK rounded up to 16 (40 -> 48, 72 -> 80), DVP = DV
//     rounded up to 32 (40 -> 64, 72 / 80 -> 96, 112 -> 128).  The K tile's columns DK .. DKP - 1 (they enter every score) and the V^T tile's rows DV .. DVP - 1
//     are zeros the kernel writes once, before the bitmap barriers: the staging stores never reach them.  DK % 8 == 0, so the 8 elements a lane holds of the
//     Q fragment's last step are inside the row or past it as a whole: past it they are zeros and no address is formed there.  The staging loops' last round
//     is guarded where 256 threads do not divide the chunks (DK = 80: 320 K chunks; DV = 80: 160 V chunk pairs); where they do, the guard is a constant and
//     the 256 and 576 instances keep their loops.  Only d < DV is stored (DV % 4 == 0: a quad is inside the row or in the padding), to dst and to a.part.
//     LDS: K 3 584 (40) ... 12 800 (192) + V^T 4 352 (40) ... 8 704 (112, 128) + 512 bytes (bitmap): no attribute, several workgroups per CU.
// LDS banks (ds_read_b128: bank = dword address mod 64, four 16-lane groups, within a group lq takes 16 values distinct mod 16).  K fragment: lane (lq, hb) reads 16
//   bytes at row lq: 16-byte slot (lq * KLD / 8 + const) mod 16, so the read is conflict-free iff KLD / 8 is odd.  DKP is a multiple of 16, KLD = DKP + 8 makes
//   KLD / 8 odd at every size (7, 11, 11, 13, 15, 25; 33 and 73 as before); DK + 8 would be even at 40 and 72 (2-way).  V^T fragment: b32 reads (banks mod 32, the two
//   32-lane halves apart) of words (row lq) * 17 + const: 17 is odd, 32 rows on 32 banks, conflict-free whatever DV.  The transposing V^T writes are not: thread c
//   writes row 8 * (c % (DV / 8)) + .., word c / (DV / 8), bank (8 * o + p) mod 32 -- 8-way at DV = 256 (32 chunks per row, p constant over 32 lanes), 2- to 4-way at
//   the small sizes where a 32-lane half spans several p.  Derived from the bank rule, not counted: no counter run was made.
// Registers (-Rpass-analysis=kernel-resource-usage, gfx950, VGPR / AGPR, plain and soft-cap instance; scratch 0 in every instance, no spill to memory):
//   40: 128 / 48, 130 / 48    72: 174 / 64, 176 / 64    80: 174 / 64, 176 / 64    96: 178 / 64, 180 / 64    112: 198 / 80, 200 / 80    192 / 128: 214 / 80, 216 / 80
//   256: 256 / 194, 256 / 196    576 / 512: 256 / 221, 256 / 226 (as before the small sizes were added; two waves per SIMD at 40 ... 96, one above)
// Per live KV tile, two barriers (three with the exchange) and single-buffered LDS; the global loads are register-staged and overlap the
// matrix work of the other operand: V(t) is in flight under K(t).Q, K(t + 1) under P.V(t).
//
// Mask (f16, shared by all heads).  Before the loop every wave marks, in an LDS bitmap, the KV tiles of the slice in which any of its
// columns has a visible cell; tiles no wave marked are skipped without K / V traffic or barriers.  A column whose cells of a live tile
// are all masked keeps M = -inf: the exponent base is then 0, not M, so that exp2(-inf - 0) = 0 and nothing turns into NaN.
// Bounds: rows past n_kv and columns past the last (token, head) pair are CLAMPED to a valid index before any address is formed; their
// probability is zero and their output is not stored.
//
// KV slices: grid = slices x column-tile groups x KV heads x sequences.  One slice: the workgroup finishes its rows (sinks, 1 / S, store).
// More: one partial (O, M, S) row per column goes to a.part ([column][slice][DV + 2], natural-log M) and k_fattn_merge<DV> (fattn.hip)
// folds them, applies the sinks and normalises.
#include "fattn_dev.hpp"

namespace mi {

typedef _Float16 fw_h8v  __attribute__((ext_vector_type(8)));
typedef _Float16 fw_h2v  __attribute__((ext_vector_type(2)));
typedef float    fw_f16a __attribute__((ext_vector_type(16)));
typedef float    fw_f32x2 __attribute__((ext_vector_type(2)));

constexpr int   FW_KT = 32;                      // KV rows per tile
constexpr int   FW_NW = 4;                       // waves per workgroup
constexpr int   FW_MAXT = 4096;                  // live-tile bitmap capacity: n_kv <= 131072
constexpr float FW_LOG2E = 1.4426950408889634f;

template <int DK, int DV> struct fw_cfg {
    static constexpr int DKP  = (DK + 15) / 16 * 16;   // DK rounded up to whole MFMA steps: the K tile's columns DK .. DKP - 1 are zeros
    static constexpr int DVP  = (DV + 31) / 32 * 32;   // DV rounded up to whole 32-dim blocks of O^T: the V^T tile's rows DV .. DVP - 1 are zeros
    static constexpr int KLD  = DKP + 8;         // K tile row pitch in halfs (16-byte aligned rows; KLD / 8 is odd: conflict-free b128 reads)
    static constexpr int VLDW = 17;              // V^T row pitch in 32-bit words (odd: spreads the transposing writes)
    static constexpr int KB   = FW_KT * KLD * 2; // bytes of the K tile
    static constexpr int VB   = DVP * VLDW * 4;  // bytes of the V^T tile
    static constexpr int NDH  = DV > 256 ? 2 : 1;                  // waves that share a column tile (halves of DK for the scores, of DV for O^T)
    static constexpr int XB   = NDH > 1 ? FW_NW * 16 * 64 * 4 : 0; // bytes of the partial-score exchange
    static constexpr int QB   = NDH > 1 ? FW_NW * (DKP / 16 / NDH) * 64 * 16 : 0;   // bytes of the waves' Q fragments kept in LDS (576: the registers go to O^T and the staging)
};

extern __shared__ __attribute__((aligned(16))) char fw_lds[];

template <int DK, int DV, bool CAP>
__global__ void __launch_bounds__(64 * FW_NW) k_fattn_wide(const fa_dev a, const int nct) {
    constexpr int KLD = fw_cfg<DK, DV>::KLD, VLDW = fw_cfg<DK, DV>::VLDW;
    constexpr int NDH = fw_cfg<DK, DV>::NDH, CTW = FW_NW / NDH;   // column tiles per workgroup
    constexpr int DKP = fw_cfg<DK, DV>::DKP, DVP = fw_cfg<DK, DV>::DVP;
    constexpr int NKS = DKP / 16 / NDH, NDB = DVP / 32 / NDH;     // this wave's MFMA steps over DK, its 32-dim blocks of O^T
    constexpr int NT  = 64 * FW_NW;
    constexpr int KTOT = FW_KT * (DK / 8), VTOT = (FW_KT / 2) * (DV / 8);   // 16-byte K chunks, 16-byte chunk PAIRS (rows 2p, 2p + 1) of V per tile
    constexpr int KCH = (KTOT + NT - 1) / NT, VCH = (VTOT + NT - 1) / NT;   // ... per thread
    constexpr bool KRAG = KTOT % NT != 0, VRAG = VTOT % NT != 0;            // the last round has idle threads (false: the guards below fold away)
    static_assert(DK % 8 == 0 && DV % 8 == 0, "16-byte chunks of K and V rows");
    static_assert(NDH == 1 || (DKP == DK && DVP == DV && DK % (16 * NDH) == 0 && DV % (32 * NDH) == 0), "the shared column tile splits whole steps");
    _Float16 * Ks = (_Float16 *) fw_lds;
    uint32_t * Vt = (uint32_t *) (fw_lds + fw_cfg<DK, DV>::KB);
    float    * Xs = (float *) (fw_lds + fw_cfg<DK, DV>::KB + fw_cfg<DK, DV>::VB);                 // [wave][16][64] partial scores (NDH == 2)
    fw_h8v   * Ql = (fw_h8v *) (fw_lds + fw_cfg<DK, DV>::KB + fw_cfg<DK, DV>::VB + fw_cfg<DK, DV>::XB) + (threadIdx.x >> 6) * (NKS * 64) + (threadIdx.x & 63);   // this lane's Q fragments, 64 apart (NDH == 2)
    __shared__ uint32_t live[FW_MAXT / 32];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lq = lane & 31, hb = lane >> 5;
    int b = (int) blockIdx.x;
    const int ncg = (nct + CTW - 1) / CTW;
    const int sp  = b % a.nsplit; b /= a.nsplit;
    const int cg  = b % ncg;      b /= ncg;
    const int ikv = b % a.nhkv;   const int is3 = b / a.nhkv;
    const int ct  = cg * CTW + wave / NDH, dh = wave % NDH;
    const bool active = ct < nct;                         // (wave-uniform)
    int tok, hh; bool row_ok;
    if (a.gq >= 32) { const int tpt = (a.gq + 31) / 32; tok = ct / tpt; hh = (ct % tpt) * 32 + lq; row_ok = active && hh < a.gq && tok < a.nq; }
    else            { tok = ct * a.qpw + lq / a.gq; hh = lq % a.gq; row_ok = active && lq < a.qpw * a.gq && tok < a.nq; }
    const int q = row_ok ? tok : 0;
    const int h = ikv * a.gq + (row_ok ? hh : 0);

    const int ntile = (a.nkv + FW_KT - 1) / FW_KT;
    const int tps  = (ntile + a.nsplit - 1) / a.nsplit;
    const int t_lo = sp * tps < ntile ? sp * tps : ntile;
    const int t_hi = (sp + 1) * tps < ntile ? (sp + 1) * tps : ntile;

    const float c2 = CAP ? a.scale * 2.0f * FW_LOG2E : a.scale * FW_LOG2E;      // CAP: 2 x log2(e) x the score before the cap, for tanh below
    const float cap2 = a.logit_softcap * FW_LOG2E;
    const uint16_t * mrow = a.mask ? (const uint16_t *) (a.mask + q * a.mnb1 + (is3 % (int) a.mne3) * a.mnb3) : nullptr;   // (plan: mask ne2 == 1)
    const bool mask_vec = a.mask && a.mnb1 % 8 == 0 && a.mnb3 % 8 == 0 && ((uintptr_t) a.mask) % 8 == 0;     // (uniform: every column's row is 8-byte aligned)

    // mask words of this lane's column in tile t: word pair g = cells t*32 + 4*hb + 8*g + {0..3}; cells past n_kv read as -inf
    auto load_mask = [&](const int t, u32x2 (&mw)[4]) {
        if (t * FW_KT + FW_KT <= a.nkv && (!mrow || mask_vec)) {             // (uniform) a whole tile, vector loads
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                if (mrow) mw[g] = *(const u32x2 *) (mrow + t * FW_KT + 4 * hb + 8 * g); else { mw[g][0] = 0u; mw[g][1] = 0u; }
            }
        } else {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int kvb = t * FW_KT + 4 * hb + 8 * g;
                uint32_t hv[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) { const int kc = kvb + i < a.nkv ? kvb + i : a.nkv - 1; hv[i] = mrow ? (uint32_t) mrow[kc] : 0u; if (kvb + i >= a.nkv) hv[i] = 0xfc00u; }
                mw[g][0] = hv[0] | (hv[1] << 16); mw[g][1] = hv[2] | (hv[3] << 16);
            }
        }
    };

    // ---- the padding the matrix cores read: zeros written HERE, once (store_k / store_v never touch it; the barriers below publish it)
    if constexpr (DKP != DK) {                            // K columns DK .. DKP - 1: one 16-byte chunk per row
        static_assert(DKP - DK == 8, "DK % 8 == 0");
        if (tid < FW_KT) *(u32x4 *) (Ks + tid * KLD + DK) = u32x4{ 0u, 0u, 0u, 0u };
    }
    if constexpr (DVP != DV) {                            // V^T rows DV .. DVP - 1, the 16 words the fragments read
        for (int i = tid; i < (DVP - DV) * 16; i += NT) Vt[(DV + (i >> 4)) * VLDW + (i & 15)] = 0u;
    }

    // ---- live-tile bitmap of this slice (bit t - t_lo)
    for (int i = tid; i < FW_MAXT / 32; i += NT) live[i] = a.mask ? 0u : 0xffffffffu;
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

    const char * kbase = a.k + ikv * a.knb2 + is3 * a.knb3;
    const char * vbase = a.v + ikv * a.vnb2 + is3 * a.vnb3;
    u32x4 kreg[KCH], vreg[VCH][2];
    auto load_k = [&](const int t) {
#pragma unroll
        for (int i = 0; i < KCH; ++i) {
            const int c = tid + i * NT, row = c / (DK / 8), o = c % (DK / 8);
            if (KRAG && c >= KTOT) continue;
            const int kv = t * FW_KT + row;
            const bool ok = kv < a.nkv;
            kreg[i] = *(const u32x4 *) (kbase + (int64_t) (ok ? kv : a.nkv - 1) * a.knb1 + o * 16);
            if (!ok) kreg[i] = u32x4{ 0u, 0u, 0u, 0u };
        }
    };
    auto store_k = [&]() {
#pragma unroll
        for (int i = 0; i < KCH; ++i) {
            const int c = tid + i * NT, row = c / (DK / 8), o = c % (DK / 8);
            if (KRAG && c >= KTOT) continue;
            *(u32x4 *) (Ks + row * KLD + o * 8) = kreg[i];
        }
    };
    auto load_v = [&](const int t) {
#pragma unroll
        for (int i = 0; i < VCH; ++i) {
            const int c = tid + i * NT, o = c % (DV / 8), p = c / (DV / 8);
            if (VRAG && c >= VTOT) continue;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int kv = t * FW_KT + 2 * p + j;
                const bool ok = kv < a.nkv;
                vreg[i][j] = *(const u32x4 *) (vbase + (int64_t) (ok ? kv : a.nkv - 1) * a.vnb1 + o * 16);
                if (!ok) vreg[i][j] = u32x4{ 0u, 0u, 0u, 0u };
            }
        }
    };
    auto store_v = [&]() {                                 // transposed: word p of V^T row d holds rows (2p, 2p + 1) of dim d
#pragma unroll
        for (int i = 0; i < VCH; ++i) {
            const int c = tid + i * NT, o = c % (DV / 8), p = c / (DV / 8);
            if (VRAG && c >= VTOT) continue;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                Vt[(8 * o + 2 * e)     * VLDW + p] = (vreg[i][0][e] & 0xffffu) | (vreg[i][1][e] << 16);
                Vt[(8 * o + 2 * e + 1) * VLDW + p] = (vreg[i][0][e] >> 16)     | (vreg[i][1][e] & 0xffff0000u);
            }
        }
    };

    int t = next_live(t_lo);
    if (t < t_hi) load_k(t);                               // in flight under the Q loads

    // ---- Q fragment: B operand, lane (column lq, half hb) holds d = 16*ks + 8*hb + {0..7}, rounded to f16 (q_to_vec_dot, ops.cpp:8040)
    constexpr bool QLDS = NDH > 1;
    fw_h8v qf[QLDS ? 1 : NKS];
    {
        const char * qr = a.q + q * a.qnb1 + h * a.qnb2 + is3 * a.qnb3 + dh * (DK / NDH) * 4;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            const int  d0  = ks * 16 + hb * 8;
            const bool qin = DKP == DK || d0 < DK;         // (DK % 8 == 0: the lane's 8 elements are inside the row or past it as a whole; past it: zeros, and no address there)
            const int  d0c = qin ? d0 : 0;
            const f32x4 v0 = *(const f32x4 *) (qr + d0c * 4);
            const f32x4 v1 = *(const f32x4 *) (qr + (d0c + 4) * 4);
            fw_h8v x;
#pragma unroll
            for (int e = 0; e < 4; ++e) { x[e] = qin ? (_Float16) v0[e] : (_Float16) 0.0f; x[4 + e] = qin ? (_Float16) v1[e] : (_Float16) 0.0f; }
            if (QLDS) Ql[ks * 64] = x; else qf[QLDS ? 0 : ks] = x;
        }
    }

    fw_f16a acc_o[NDB];
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc_o[db][e] = 0.0f;
    float M = -INFINITY, S = 0.0f;

    while (t < t_hi) {
        store_k();
        load_v(t);                                         // in flight under the score product
        u32x2 mw[4];
        if (active) load_mask(t, mw);
        __syncthreads();                                   // K(t) visible; every wave is past P.V(t - 1): the V tile may be overwritten below
        float alpha = 1.0f;
        union { fw_h2v h2[4]; fw_h8v v; } pf[2];
        fw_f16a sc;
#pragma unroll
        for (int e = 0; e < 16; ++e) sc[e] = 0.0f;
        if (active) {
            // ---- S^T = K . Q^T over this wave's part of DK
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) {
                const fw_h8v kf = *(const fw_h8v *) (Ks + lq * KLD + dh * (DK / NDH) + ks * 16 + hb * 8);
                const fw_h8v qv = QLDS ? Ql[ks * 64] : qf[QLDS ? 0 : ks];
                sc = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qv, sc, 0, 0, 0);
            }
        }
        if (NDH > 1) {                                     // the pair's partial scores, added in the same order by both: dh 0 + dh 1
#pragma unroll
            for (int e = 0; e < 16; ++e) Xs[(wave * 16 + e) * 64 + lane] = sc[e];
            __syncthreads();
#pragma unroll
            for (int e = 0; e < 16; ++e) { const float o = Xs[((wave ^ 1) * 16 + e) * 64 + lane]; sc[e] = dh == 0 ? sc[e] + o : o + sc[e]; }
        }
        if (active) {
            // ---- scale / softcap / mask, base-2 online soft-max; sc[e] is cell (e & 3) + 8 * (e >> 2) + 4 * hb of the tile
            float tmax = -INFINITY;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const uint32_t w = mw[e >> 2][(e >> 1) & 1];
                const uint16_t hbits = (uint16_t) ((e & 1) ? (w >> 16) : (w & 0xffffu));
                float v = sc[e] * c2;
                if (CAP) v = cap2 - 2.0f * cap2 * __builtin_amdgcn_rcpf(__builtin_amdgcn_exp2f(v) + 1.0f);     // cap * tanh(x) = cap * (1 - 2 / (e^2x + 1)), branch-free; +-cap at +-inf
                v = (hbits == 0xfc00u || !row_ok) ? -INFINITY : v + FW_LOG2E * h2f(hbits);
                sc[e] = v;
                tmax = fmaxf(tmax, v);
            }
            tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
            const float Mn = fmaxf(M, tmax);
            const float Mu = Mn == -INFINITY ? 0.0f : Mn;  // a column with nothing visible so far: exp2(-inf - 0) = 0, never -inf - -inf
            alpha = __builtin_amdgcn_exp2f(M - Mu);
            float psum = 0.0f;
#pragma unroll
            for (int e = 0; e < 16; e += 2) {
                const float p0 = __builtin_amdgcn_exp2f(sc[e] - Mu), p1 = __builtin_amdgcn_exp2f(sc[e + 1] - Mu);
                psum += p0 + p1;
                const fw_f32x2 pp = { p0, p1 };
                pf[e >> 3].h2[(e & 7) >> 1] = __builtin_convertvector(pp, fw_h2v);
            }
            S = S * alpha + psum;
            M = Mn;
        }
        store_v();
        const int tn = next_live(t + 1);
        if (tn < t_hi) load_k(tn);                         // in flight under P.V
        __syncthreads();                                   // V(t) visible; every wave is past K(t).Q: the K tile may be overwritten at the top
        if (active) {
            if (!__all(alpha == 1.0f)) {
#pragma unroll
                for (int db = 0; db < NDB; ++db)
#pragma unroll
                    for (int e = 0; e < 16; ++e) acc_o[db][e] *= alpha;
            }
            // ---- O^T += V^T . P^T
#pragma unroll
            for (int db = 0; db < NDB; ++db) {
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    const uint32_t * vr = &Vt[(dh * (DV / NDH) + db * 32 + lq) * VLDW + 8 * s2 + 2 * hb];
                    union { uint32_t u[4]; fw_h8v v; } vf;
                    vf.u[0] = vr[0]; vf.u[1] = vr[1]; vf.u[2] = vr[4]; vf.u[3] = vr[5];
                    acc_o[db] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf.v, pf[s2].v, acc_o[db], 0, 0, 0);
                }
            }
        }
        t = tn;
    }

    if (!row_ok) return;                                   // (no barrier below)
    S += __shfl_xor(S, 32, 64);                            // (row_ok is the same in both lane halves)
    if (a.nsplit > 1) {                                    // partial state of this slice, natural-log convention (k_fattn_merge)
        float * pr = a.part + ((((int64_t) is3 * a.nq + q) * a.nh + h) * a.nsplit + sp) * (DV + 2);
#pragma unroll
        for (int db = 0; db < NDB; ++db)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4 o4;
#pragma unroll
                for (int i = 0; i < 4; ++i) o4[i] = acc_o[db][4 * g + i];
                const int d = dh * (DV / NDH) + db * 32 + 8 * g + 4 * hb;
                if (DVP == DV || d < DV) *(f32x4 *) (pr + d) = o4;      // (DV % 4 == 0: a quad is inside the row or in the padding as a whole)
            }
        if (hb == 0 && dh == 0) { pr[DV] = M * 0.6931471805599453f; pr[DV + 1] = S; }
        return;
    }
    // ---- one slice: finish here -- sinks (ops.cpp:8116-8130), normalise, store permuted
    float osc = 1.0f;
    if (a.sinks) {
        const float sk = a.sinks[h] * FW_LOG2E;
        if (sk > M) { const float f = __builtin_amdgcn_exp2f(M - sk); S = S * f + 1.0f; osc = f; }
        else S += __builtin_amdgcn_exp2f(sk - M);
    }
    const float inv = S == 0.0f ? 0.0f : osc / S;
    char * out = a.dst + h * a.dnb1 + q * a.dnb2 + is3 * a.dnb3;
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f32x4 o4;
#pragma unroll
            for (int i = 0; i < 4; ++i) o4[i] = acc_o[db][4 * g + i] * inv;
            const int d = dh * (DV / NDH) + db * 32 + 8 * g + 4 * hb;
            if (DVP == DV || d < DV) *(f32x4 *) (out + d * 4) = o4;
        }
}

static long g_fw_launches = 0;
long fattn_wide_launches() { return g_fw_launches; }

bool fattn_wide_dims(int64_t DK, int64_t DV) {
    if (DK == DV) return DK == 40 || DK == 72 || DK == 80 || DK == 96 || DK == 112 || DK == 256;
    return (DK == 192 && DV == 128) || (DK == 576 && DV == 512);
}
int  fattn_wide_max_tiles() { return FW_MAXT; }

template <int DK, int DV>
static void fw_go(const fa_dev & a0, hipStream_t st) {
    fa_dev a = a0;
    a.qpw = a.gq < 32 ? 32 / a.gq : 1;                                         // tokens per column tile
    const int nct = a.gq >= 32 ? a.nq * ((a.gq + 31) / 32) : (a.nq + a.qpw - 1) / a.qpw;
    const int ctw = FW_NW / fw_cfg<DK, DV>::NDH, ncg = (nct + ctw - 1) / ctw;                  // column tiles per workgroup, workgroups per (KV head, sequence, slice)
    const size_t lds = (size_t) fw_cfg<DK, DV>::KB + fw_cfg<DK, DV>::VB + fw_cfg<DK, DV>::XB + fw_cfg<DK, DV>::QB;
    const dim3 grid((unsigned) ((int64_t) a.nsplit * ncg * a.nhkv * a.ns));
#define FW_GO(CC) do {                                                                                                                             \
        static bool attr = false;                                                                                                                  \
        if (!attr && lds > 64 * 1024) { HIP_CHECK(hipFuncSetAttribute((const void *) k_fattn_wide<DK, DV, CC>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds)); attr = true; } \
        k_fattn_wide<DK, DV, CC><<<grid, dim3(64 * FW_NW), lds, st>>>(a, nct);                                                                    \
    } while (0)
    if (a.logit_softcap != 0.0f) FW_GO(true); else FW_GO(false);
#undef FW_GO
    ++g_fw_launches;
}

void flash_attn_ext_wide(const fa_dev & a, int DK, int DV, hipStream_t st) {
    if (DK == 256 && DV == 256) fw_go<256, 256>(a, st);
    else if (DK == 576 && DV == 512) fw_go<576, 512>(a, st);
    else if (DK == 96  && DV == 96)  fw_go<96, 96>(a, st);
    else if (DK == 192 && DV == 128) fw_go<192, 128>(a, st);
    else if (DK == 80  && DV == 80)  fw_go<80, 80>(a, st);
    else if (DK == 112 && DV == 112) fw_go<112, 112>(a, st);
    else if (DK == 72  && DV == 72)  fw_go<72, 72>(a, st);
    else if (DK == 40  && DV == 40)  fw_go<40, 40>(a, st);
    else { fprintf(stderr, "[mi355x] flash_attn: no wide kernel for head size %d / %d\n", DK, DV); abort(); }
}

} // namespace mi
