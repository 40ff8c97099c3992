// wkv7_chunk.hip -- RWKV_WKV7 for prompts: the recurrence of wkv.hip's k_wkv7 over CHUNKS of L tokens on the f32 matrix cores (gfx950 / wave64), beside wkv_chunk.hip.
//
// What it takes (wkv7_chunk_takes): head size 64 or 128, 16-byte aligned operands, option "wkv_chunk" not 0, and at the default option at least wkv7_chunk_min_tokens()
// tokens per sequence (64; MI355X_WKV_CHUNK_MIN_TOKENS raises it) and a grid of at most 512 workgroups (heads x sequences <= 256 at S = 64, <= 128 at S = 128), both
// measured (WKV7_CHUNK_* below).  Everything else stays on k_wkv7 / k_wkv7_any.  wkv7_f32 (wkv.hip) routes; a node is one launch either way.
//
// The mathematics (ggml_compute_forward_rwkv_wkv7_f32 restated; layouts as in wkv.hip's header), per (sequence, head): state s[i][j], i the v index, j the k index.
//     sa_t = S_{t-1} a_t        S_t = S_{t-1} diag(w_t) + v_t k_t^T + sa_t b_t^T        out_t = S_t r_t
// Read sa_t as an unknown pseudo-value: S is a decayed linear attention with two rank-one inputs per token, (v_t, k_t) and (sa_t, b_t).  Over a chunk that starts at token
// 0 with state S_0, with D(x, y][j] = prod_{x < u <= y} w_u[j], four token x token score matrices (the first two strictly lower, the last two with an undecayed diagonal):
//     A_ak[t][s] = sum_j a_t[j] k_s[j] D(s, t-1][j]    A_ab likewise with b_s   (s < t)          A_rk[t][s] = sum_j r_t[j] k_s[j] D(s, t][j]    A_rb likewise   (s <= t)
//     SA  = (I - A_ab)^-1 (A0 + A_ak V)          A0[t] = (a_t o D(-1, t-1]) S_0^T        (rows of SA: the sa_t; every column i of V, SA, Out is independent of the others)
//     Out = R0 + A_rk V + A_rb SA                R0[t] = (r_t o D(-1, t]) S_0^T
//     S_n = S_0 diag(D(-1, n-1]) + V^T (K o Dend) + SA^T (B o Dend)                      Dend[s] = D(s, n-1]
// D(s, t] = D(s, t-1] w_t: with rw_t = r_t o w_t (the operand itself, sign and zero included) the off-diagonal entries of all four matrices share the decay D(s, t-1]: the
// stacked queries [a ; rw] against the stacked keys [k ; b] cost ONE exponential per (pair, channel).
// Decays as in wkv_chunk.hip: w travels as l = max(logf(|w|), -128) and a sign, sub-chunks of 16 tokens, and NO POSITIVE EXPONENT of a (0, 1] decay is ever formed:
//     at_t = a_t o D(c0-1, t-1], rt_t = rw_t o D(c0-1, t-1]     queries decayed FROM the start c0 of their sub-chunk        (tiles At, Rt)
//     kh_s = k_s o D(s, e], bh_s = b_s o D(s, e]                keys decayed TO the end e of their sub-chunk               (tiles Kh, Bh)
//     G[c1][c2] = the product of the whole sub-chunks c1 <= c < c2, per channel                                          (table Gt; G[c][c] = 1)
//   off-diagonal block (query sub-chunk 1, key sub-chunk 0; L <= 32, so the two are adjacent and G[1][1] = 1):  {At, Rt} {Kh, Bh}^T, MFMA products over the S channels
//   the S_0 terms of sub-chunk c: ({At, Rt} o G[0][c]) S_0^T, MFMA over the channels;  state: S^T = diag(G[0][NSC]) S^T + (Kh o G[kb+1][NSC])^T V + (Bh o G..)^T SA, MFMA over tokens
//   diagonal blocks: sum_j q_t[j] k_s[j] exp(p_{t-1}[j] - p_s[j]) for s < t element by element on the VALU, p the prefix sum of l INSIDE the sub-chunk, operands times their
//     sign prefixes (tiles As, Rs, Ks, Bs, Pl); the diagonal of A_rk / A_rb is sum_j r_t k_t / r_t b_t with no decay (tile Rq = r times the sign prefix through t, so that
//     Rq Ks = r k); zeros above.  Zero decays are factors exp(-128) = 0 in f32 and rw = 0 exactly; negative decays live in the sign products.
//
// The solve: the FIRST form, per sub-chunk on the slice -- SA_c = (I - N_c)^-1 (A0_c + sum_{c' < c} (A_ak[c][c'] V_c' + A_ab[c][c'] SA_c') + A_ak[c][c] V_c), N_c the strictly
// lower diagonal block of A_ab -- and the inverse is never formed: the right-hand side goes through LDS, and 32 lanes (one per column i of the slice) run the 16 steps of the
// forward substitution sa_t = rhs_t + sum_{s < t} N[t][s] sa_s in registers (120 fmaf; the rows of N are broadcast reads).  Why: a full T = (I - A_ab)^-1 costs the same
// substitution on 16 columns per block PLUS the block products of T and 4 MFMAs per tile, all before the first SA exists, and is a less accurate order (inverse, then product)
// than the plain triangular solve the formulation was checked with; the slice form costs two barriers per sub-chunk (right-hand side written, SA written), 2 NSC <= 4 a chunk.
//
// Grid: one 4-wave workgroup per (32-row slice of i, head, sequence) -- x = S / 32, y = H, z = n_seqs -- that walks the sequence's chunks in order: one launch, no scratch, no
// reduction across workgroups; the score matrices are recomputed per slice.  L = 32 tokens at S = 64, 16 at S = 128 (ten S-wide tiles: 87 KB / 84 KB; L = 32 at S = 128
// would need 169 KB for them alone).  NSC = L / 16 sub-chunks.  The state slice is held TRANSPOSED, St[j][i] (S x 32), so that it is the B operand of the S_0 terms and its
// update contracts over tokens, as in k_wkv6_chunk: it lives in accumulator registers for the whole sequence and goes through LDS once per chunk.
// All products on __builtin_amdgcn_mfma_f32_16x16x4f32: lane (lm = lane % 16, lk = lane / 16) supplies A[lm][k = lk] and B[k = lk][lm]; accumulator r holds row 4 lk + r, column lm.
// Per chunk:
//   1. stage r, w, k, a, b [L][S] and the v slice [L][32] from the registers the previous chunk ran under (the NEXT chunk's 16-byte loads are requested right after); rows
//      past n_t are staged as r = k = v = a = b = 0, w = 1: no second code path, sa = 0 there and the state update stays exact.
//   2. scan (after barrier 1): thread = (sub-chunk, channel), NSC * S = 128 threads, walks its 16 tokens: l, the sign, the prefixes; As, Rs, Ks, Bs, Pl IN PLACE of a, r, k, b,
//      w (the thread re-reads only its own elements), Rq, At, Rt, Kh, Bh and the sub-chunk's totals.
//   3. (after barrier 2) the table G; the diagonal blocks of the four matrices: 4 / NSC waves per block, lane = (t = lm; 2 or 1 key tokens), 16-byte reads along the channels,
//      one __expf and six fmaf per (pair, channel).
//   4. (after barrier 3) NSC = 2: the off-diagonal block of matrix m on wave m (16 MFMAs); the S_0 terms A0 / R0 of the wave's tile (sub-chunk c, column half nh).
//   5. (after barrier 4) for c = 0 .. NSC - 1: the right-hand side of tile (c, nh) -> LDS; barrier; the substitution in place (wave 0, lanes 0 .. 31); barrier.
//   6. Out tile = R0 + sum_{kb <= c} (A_rk V + A_rb SA), stored for t < n_t, 64 contiguous bytes per 16 lanes; the state update, written to LDS for the next chunk.  Barrier.
//   Tiles: NSC = 2: wave w owns (c = w / 2, nh = w % 2), its right-hand side and its output.  NSC = 1: waves 0 / 1 own the right-hand sides, waves 2 / 3 the outputs.
// Start: s_in slice (32 rows of S, contiguous) -> LDS transposed -> accumulators.  End: LDS -> s_out.
//
// LDS (floats; pitches PB = S + 4 for the ten S-wide tiles, PS = PV = 36 for the state, v and SA slices, PA = L + 4 for the four score matrices):
//   10 L PB + S PS + 2 L PV + 4 L PA + (NSC + 1)^2 S + 2 NSC S = 127 232 bytes at S = 64, 115 712 at S = 128: one workgroup per CU, under the 152 KiB rule (asserted at the launch).
// LDS banks, conflict-free by wkv_chunk.hip's derivation for the same pitches: the 16-byte reads along a row of an S-wide tile or of a score matrix (PB / 4 = 17 / 33 and
//   PA / 4 = 9 / 5 odd: a quarter wave's 16 rows take the 64 banks once); the reads across rows of Ss, Vs, SAs, Kh, Bh (4 P = 16 mod 64 for P = 68 / 132 / 36); the accumulator
//   stores to Ss / SAs and to a score matrix at L = 32 (4 PA = 16 mod 64; at L = 16, 4 PA = 80: two-way); the scan's and the substitution's column accesses (consecutive lanes,
//   consecutive dwords; the rows of N are broadcasts).  NOT conflict-free: the transposing state load and store (four-way, once per sequence).
// Registers (-Rpass-analysis=kernel-resource-usage, gfx950; VGPR / AGPR, scratch 0 and no VGPR spill in both instances): <64> 256 / 34 (the allocator parks values in
//   AGPRs, and 24 SGPRs in VGPR lanes; nothing reaches memory), <128> 248 / 16.  The LDS is dynamic (the remark shows 0): the sizes are the ones above.  One workgroup
//   per CU by its LDS, so one wave per SIMD.  Built with -packed-fp32-ops off (Makefile): the accumulators are scaled between MFMA runs.
// Measured (tools/wkv_bench.py --legs prompt7, profiles/wkv7_chunk_bench.txt; one sequence): 64 heads of 64 at 512 tokens 214 us against k_wkv7's 401, 13.3 us per
//   32-token chunk; 32 heads of 128 at 512 tokens 370 us against 792, 11.5 us per 16-token chunk.  Not done: the scan on all 256 threads (half idle now), work for the
//   three waves that wait on the substitution (the K part of the state update does not need SA), more than one wave per SIMD.
#include "../kernels.hpp"
#include <type_traits>

namespace mi {

typedef float w7_f4a __attribute__((ext_vector_type(4)));

struct wkv7_chunk_args {
    const float * r, * w, * k, * v, * a, * b;        // {S, H, T}
    const float * s_in;                              // previous states, sequence q at q * S * S * H
    float * out, * s_out;                            // {S * H, T} outputs; new states
    int H, n_t;                                      // heads; tokens per sequence
};

template <int S> struct w7_cfg {
    static constexpr int L = S == 64 ? 32 : 16, NSC = L / 16, NG = NSC + 1;      // tokens per chunk, sub-chunks, rows / columns of the table G
    static constexpr int PB = S + 4, PS = 36, PV = 36, PA = L + 4, T = L * PB;
    static constexpr int oA = 0, oR = T, oK = 2 * T, oB = 3 * T, oP = 4 * T, oQ = 5 * T, oAt = 6 * T, oRt = 7 * T, oKh = 8 * T, oBh = 9 * T, oS = 10 * T, oV = oS + S * PS,
                         oSA = oV + L * PV, oM = oSA + L * PV, oG = oM + 4 * L * PA, oT = oG + NG * NG * S, oSg = oT + NSC * S;
    static constexpr int floats = oSg + NSC * S;
};

static __device__ __forceinline__ w7_f4a w7_mma(float a, float b, w7_f4a c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

static __device__ __forceinline__ float4 w7_ld4(const float * p, bool in, float fill) {      // a row of the chunk, or the filler past the sequence's end (by value: see wc_ld4)
    float4 v = make_float4(fill, fill, fill, fill);
    if (in) v = *(const float4 *) p;
    return v;
}

// acc += M[16 qa + .][16 kb + .] X[16 kb + .][16 nh + .]: a 16 x 16 block of a score matrix against 16 tokens of a 36-pitch slice
static __device__ __forceinline__ w7_f4a w7_blk(const float * mrow, const float * x, w7_f4a acc) {
    const float4 a4 = *(const float4 *) mrow;
    acc = w7_mma(a4.x, x[0], acc); acc = w7_mma(a4.y, x[36], acc); acc = w7_mma(a4.z, x[72], acc); acc = w7_mma(a4.w, x[108], acc);
    return acc;
}

extern __shared__ float4 w7_lds4[];

template <int S>
__global__ void __launch_bounds__(256) k_wkv7_chunk(const wkv7_chunk_args a) {
    using K = w7_cfg<S>;
    constexpr int L = K::L, NSC = K::NSC, NG = K::NG, PB = K::PB, PS = K::PS, PV = K::PV, PA = K::PA;
    constexpr int NF = L * S / 1024, NS4 = S / 32;           // float4s per thread: a chunk of one operand, the state slice
    constexpr int NWD = 4 / NSC, PPL = 4 / NWD;              // waves per diagonal block, key tokens per lane in it
    constexpr int IPW = S / 64;                              // state row blocks of 16 channels per wave (two tiles each)
    static_assert(NSC <= 2 && PS == 36 && PV == 36, "adjacent sub-chunks only (no G between them); w7_blk's pitch");
    float * lds = (float *) w7_lds4;
    float * As = lds + K::oA, * Rs = lds + K::oR, * Ks = lds + K::oK, * Bs = lds + K::oB, * Pl = lds + K::oP, * Rq = lds + K::oQ, * At = lds + K::oAt, * Rt = lds + K::oRt;
    float * Kh = lds + K::oKh, * Bh = lds + K::oBh, * Ss = lds + K::oS, * Vs = lds + K::oV, * SAs = lds + K::oSA, * Mx = lds + K::oM;
    float * Gt = lds + K::oG, * Tot = lds + K::oT, * Sg = lds + K::oSg;
    constexpr int MS = L * PA;                               // one score matrix: Mx + 0 MS = A_ak, 1 = A_ab, 2 = A_rk, 3 = A_rb

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lm = lane & 15, lk = lane >> 4;
    const int i0 = blockIdx.x * 32, h = blockIdx.y, seq = blockIdx.z;
    const size_t C = (size_t) a.H * S, so = (((size_t) seq * a.H + h) * S + i0) * S;      // the slice: 32 rows of S, contiguous
    const size_t base = (size_t) seq * a.n_t * C + (size_t) h * S;       // token 0 of the sequence, this head
    const float * rp = a.r + base, * wp = a.w + base, * kp = a.k + base, * ap = a.a + base, * bp = a.b + base, * vp = a.v + base + i0;
    float * op = a.out + base + i0;
    const int nh = w & 1, tc = NSC == 2 ? w >> 1 : 0;        // this wave's tile: column half, sub-chunk
    const bool do_sa = NSC == 2 || w < 2, do_out = NSC == 2 || w >= 2;

    // the chunk at t0 .. t0 + L - 1, requested into registers one chunk ahead
    float4 gr[NF], gw[NF], gk[NF], ga[NF], gb[NF], gv;
    auto fetch = [&](int t0) {
#pragma unroll
        for (int u = 0; u < NF; ++u) {
            const int e = tid + 256 * u, t = t0 + e / (S / 4), c4 = e % (S / 4);
            const bool in = t < a.n_t;
            const size_t o = (size_t) t * C + 4 * c4;
            gr[u] = w7_ld4(rp + o, in, 0.0f); gw[u] = w7_ld4(wp + o, in, 1.0f); gk[u] = w7_ld4(kp + o, in, 0.0f); ga[u] = w7_ld4(ap + o, in, 0.0f); gb[u] = w7_ld4(bp + o, in, 0.0f);
        }
        const int t = t0 + (tid >> 3);
        gv = w7_ld4(vp + (size_t) t * C + 4 * (tid & 7), tid < 8 * L && t < a.n_t, 0.0f);
    };

    // the state slice: s_in -> LDS, transposed -> this wave's tiles
#pragma unroll
    for (int u = 0; u < NS4; ++u) {
        const int e = tid + 256 * u, i = e / (S / 4), j = 4 * (e % (S / 4));
        const float4 x = *(const float4 *) (a.s_in + so + (size_t) i * S + j);
        Ss[j * PS + i] = x.x; Ss[(j + 1) * PS + i] = x.y; Ss[(j + 2) * PS + i] = x.z; Ss[(j + 3) * PS + i] = x.w;
    }
    fetch(0);
    __syncthreads();
    w7_f4a acc[IPW][2];
#pragma unroll
    for (int x = 0; x < IPW; ++x) {
#pragma unroll
        for (int n = 0; n < 2; ++n) {
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[x][n][r] = Ss[(16 * (w * IPW + x) + 4 * lk + r) * PS + 16 * n + lm];
        }
    }

    for (int t0 = 0; t0 < a.n_t; t0 += L) {
        // 1. stage
#pragma unroll
        for (int u = 0; u < NF; ++u) {
            const int e = tid + 256 * u, o = (e / (S / 4)) * PB + 4 * (e % (S / 4));
            *(float4 *) (Rs + o) = gr[u]; *(float4 *) (Pl + o) = gw[u]; *(float4 *) (Ks + o) = gk[u]; *(float4 *) (As + o) = ga[u]; *(float4 *) (Bs + o) = gb[u];
        }
        if (tid < 8 * L) *(float4 *) (Vs + (tid >> 3) * PV + 4 * (tid & 7)) = gv;
        if (t0 + L < a.n_t) fetch(t0 + L);
        __syncthreads();                                     // 1: the chunk is staged

        // 2. scan: 16 tokens of one channel
        if (tid < NSC * S) {
            const int sc = tid / S, si = tid % S;
            float p = 0.0f, sg = 1.0f, pl[16], ks[16], bs[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int o = (16 * sc + u) * PB + si;
                const float wv = Pl[o], r = Rs[o];
                const float l = fmaxf(logf(fabsf(wv)), -128.0f);
                const float ex = expf(p), se = sg;           // the decays before token t
                p += l; sg = wv < 0.0f ? -sg : sg;
                const float as = As[o] * se, rs = r * wv * se;
                ks[u] = Ks[o] * sg; bs[u] = Bs[o] * sg; pl[u] = p;
                As[o] = as; Rs[o] = rs; At[o] = as * ex; Rt[o] = rs * ex; Rq[o] = r * sg; Ks[o] = ks[u]; Bs[o] = bs[u]; Pl[o] = p;
            }
#pragma unroll
            for (int u = 0; u < 16; ++u) {                   // (ks / bs carry the signs up to s, sg up to the end: their product is the signs after s)
                const int o = (16 * sc + u) * PB + si;
                const float f = sg * expf(p - pl[u]);
                Kh[o] = ks[u] * f; Bh[o] = bs[u] * f;
            }
            Tot[sc * S + si] = p; Sg[sc * S + si] = sg;
        }
        __syncthreads();                                     // 2: the ten tiles and the totals

        // 3. the table G; the diagonal blocks
        for (int e = tid; e < NG * NG * S; e += 256) {
            const int pr = e / S, i = e % S, c1 = pr / NG, c2 = pr % NG;
            float sum = 0.0f, sgn = 1.0f;
#pragma unroll
            for (int c = 0; c < NSC; ++c) {
                if (c >= c1 && c < c2) { sum += Tot[c * S + i]; sgn *= Sg[c * S + i]; }
            }
            Gt[e] = sgn * expf(sum);
        }
        {
            const int c = w / NWD, t = 16 * c + lm, sl = 4 * lk + PPL * (w % NWD), s0 = 16 * c + sl;      // query token; first key token, in the sub-chunk and in the chunk
            const float * arow = As + t * PB, * rrow = Rs + t * PB, * qrow = Rq + t * PB, * erow = Pl + (lm > 0 ? t - 1 : t) * PB;      // (lm = 0 has no pair below the diagonal)
            float dak[PPL], dab[PPL], drk[PPL], drb[PPL], dqk[PPL], dqb[PPL];
#pragma unroll
            for (int u = 0; u < PPL; ++u) dak[u] = dab[u] = drk[u] = drb[u] = dqk[u] = dqb[u] = 0.0f;
#pragma unroll 2
            for (int i = 0; i < S; i += 4) {
                const float4 a4 = *(const float4 *) (arow + i), r4 = *(const float4 *) (rrow + i), q4 = *(const float4 *) (qrow + i), e4 = *(const float4 *) (erow + i);
#pragma unroll
                for (int u = 0; u < PPL; ++u) {
                    const float4 k4 = *(const float4 *) (Ks + (s0 + u) * PB + i), b4 = *(const float4 *) (Bs + (s0 + u) * PB + i), p4 = *(const float4 *) (Pl + (s0 + u) * PB + i);
#define W7_PAIR(x) { const float ex = __expf(e4.x - p4.x), ke = k4.x * ex, be = b4.x * ex;                                                              \
                     dak[u] = fmaf(a4.x, ke, dak[u]); dab[u] = fmaf(a4.x, be, dab[u]); drk[u] = fmaf(r4.x, ke, drk[u]); drb[u] = fmaf(r4.x, be, drb[u]); \
                     dqk[u] = fmaf(q4.x, k4.x, dqk[u]); dqb[u] = fmaf(q4.x, b4.x, dqb[u]); }
                    W7_PAIR(x) W7_PAIR(y) W7_PAIR(z) W7_PAIR(w)
#undef W7_PAIR
                }
            }
#pragma unroll
            for (int u = 0; u < PPL; ++u) {                  // (a pair on or above the diagonal may hold inf or nan in its decayed sums: selected away, never multiplied)
                const int s = sl + u;
                float * m = Mx + t * PA + s0 + u;
                m[0] = s < lm ? dak[u] : 0.0f; m[MS] = s < lm ? dab[u] : 0.0f;
                m[2 * MS] = s < lm ? drk[u] : s == lm ? dqk[u] : 0.0f; m[3 * MS] = s < lm ? drb[u] : s == lm ? dqb[u] : 0.0f;
            }
        }
        __syncthreads();                                     // 3: G, the diagonal blocks

        // 4. the off-diagonal block (query sub-chunk 1, key sub-chunk 0) of matrix w; the S_0 terms of this wave's tile
        if constexpr (NSC == 2) {
            const float * ar = ((w & 2) ? Rt : At) + (16 + lm) * PB + 4 * lk, * br = ((w & 1) ? Bh : Kh) + lm * PB + 4 * lk;
            w7_f4a sa = { 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll 4
            for (int j = 0; j < S; j += 16) {
                const float4 a4 = *(const float4 *) (ar + j), b4 = *(const float4 *) (br + j);
                sa = w7_mma(a4.x, b4.x, sa); sa = w7_mma(a4.y, b4.y, sa); sa = w7_mma(a4.z, b4.z, sa); sa = w7_mma(a4.w, b4.w, sa);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) Mx[w * MS + (16 + 4 * lk + r) * PA + lm] = sa[r];
        }
        w7_f4a a0 = { 0.0f, 0.0f, 0.0f, 0.0f }, oa = { 0.0f, 0.0f, 0.0f, 0.0f };
        {
            const float * ar = At + (16 * tc + lm) * PB + 4 * lk, * rr = Rt + (16 * tc + lm) * PB + 4 * lk, * gp = Gt + tc * S + 4 * lk, * bs = Ss + 4 * lk * PS + 16 * nh + lm;
#pragma unroll 4
            for (int j = 0; j < S; j += 16) {
                const float4 g4 = *(const float4 *) (gp + j);
                const float b0 = bs[j * PS], b1 = bs[(j + 1) * PS], b2 = bs[(j + 2) * PS], b3 = bs[(j + 3) * PS];
                if (do_sa) {
                    const float4 a4 = *(const float4 *) (ar + j);
                    a0 = w7_mma(a4.x * g4.x, b0, a0); a0 = w7_mma(a4.y * g4.y, b1, a0); a0 = w7_mma(a4.z * g4.z, b2, a0); a0 = w7_mma(a4.w * g4.w, b3, a0);
                }
                if (do_out) {
                    const float4 r4 = *(const float4 *) (rr + j);
                    oa = w7_mma(r4.x * g4.x, b0, oa); oa = w7_mma(r4.y * g4.y, b1, oa); oa = w7_mma(r4.z * g4.z, b2, oa); oa = w7_mma(r4.w * g4.w, b3, oa);
                }
            }
        }
        __syncthreads();                                     // 4: the score matrices are whole, the old state slice is read

        // 5. SA, sub-chunk by sub-chunk: the right-hand side of tile (c, nh), then the forward substitution down its 16 tokens
        const float * mq = Mx + (16 * tc + lm) * PA + 4 * lk, * xv = Vs + 4 * lk * PV + 16 * nh + lm, * xs = SAs + 4 * lk * PV + 16 * nh + lm;
#pragma unroll
        for (int c = 0; c < NSC; ++c) {
            if (do_sa && tc == c) {
                for (int kb = 0; kb <= c; ++kb) a0 = w7_blk(mq + 16 * kb, xv + 16 * kb * PV, a0);                 // A_ak V (its diagonal block is strictly lower)
                for (int kb = 0; kb < c; ++kb) a0 = w7_blk(mq + MS + 16 * kb, xs + 16 * kb * PV, a0);            // A_ab SA of the sub-chunks before
#pragma unroll
                for (int r = 0; r < 4; ++r) SAs[(16 * c + 4 * lk + r) * PV + 16 * nh + lm] = a0[r];
            }
            __syncthreads();                                 // the right-hand side of sub-chunk c
            if (tid < 32) {                                  // lane = column i of the slice
                const float * n = Mx + MS + 16 * c * PA + 16 * c;
                float x[16];
#pragma unroll
                for (int t = 0; t < 16; ++t) x[t] = SAs[(16 * c + t) * PV + tid];
#pragma unroll
                for (int t = 1; t < 16; ++t) {
#pragma unroll
                    for (int s4 = 0; s4 < t; s4 += 4) {
                        const float4 n4 = *(const float4 *) (n + t * PA + s4);
                        x[t] = fmaf(n4.x, x[s4], x[t]);
                        if (s4 + 1 < t) x[t] = fmaf(n4.y, x[s4 + 1], x[t]);
                        if (s4 + 2 < t) x[t] = fmaf(n4.z, x[s4 + 2], x[t]);
                        if (s4 + 3 < t) x[t] = fmaf(n4.w, x[s4 + 3], x[t]);
                    }
                }
#pragma unroll
                for (int t = 1; t < 16; ++t) SAs[(16 * c + t) * PV + tid] = x[t];
            }
            __syncthreads();                                 // SA of sub-chunk c
        }

        // 6. out = R0 + A_rk V + A_rb SA; the state
        if (do_out) {
            for (int kb = 0; kb <= tc; ++kb) {
                oa = w7_blk(mq + 2 * MS + 16 * kb, xv + 16 * kb * PV, oa);
                oa = w7_blk(mq + 3 * MS + 16 * kb, xs + 16 * kb * PV, oa);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int t = t0 + 16 * tc + 4 * lk + r;
                if (t < a.n_t) op[(size_t) t * C + 16 * nh + lm] = oa[r];
            }
        }
#pragma unroll
        for (int x = 0; x < IPW; ++x) {
            const int j0 = 16 * (w * IPW + x);
            const float4 g0 = *(const float4 *) (Gt + NSC * S + j0 + 4 * lk);      // G[0][NSC] of this lane's four channels
            acc[x][0][0] *= g0.x; acc[x][0][1] *= g0.y; acc[x][0][2] *= g0.z; acc[x][0][3] *= g0.w;
            acc[x][1][0] *= g0.x; acc[x][1][1] *= g0.y; acc[x][1][2] *= g0.z; acc[x][1][3] *= g0.w;
#pragma unroll
            for (int kb = 0; kb < NSC; ++kb) {
                const float g = Gt[((kb + 1) * NG + NSC) * S + j0 + lm];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int s = 16 * kb + 4 * lk + e;
                    const float kv = Kh[s * PB + j0 + lm] * g, bv = Bh[s * PB + j0 + lm] * g;
                    acc[x][0] = w7_mma(kv, Vs[s * PV + lm], acc[x][0]); acc[x][1] = w7_mma(kv, Vs[s * PV + 16 + lm], acc[x][1]);
                    acc[x][0] = w7_mma(bv, SAs[s * PV + lm], acc[x][0]); acc[x][1] = w7_mma(bv, SAs[s * PV + 16 + lm], acc[x][1]);
                }
            }
#pragma unroll
            for (int n = 0; n < 2; ++n) {
#pragma unroll
                for (int r = 0; r < 4; ++r) Ss[(j0 + 4 * lk + r) * PS + 16 * n + lm] = acc[x][n][r];
            }
        }
        __syncthreads();                                     // the new state slice is written; every read of the staged chunk is done
    }

    // the final slice (the last barrier made it visible)
#pragma unroll
    for (int u = 0; u < NS4; ++u) {
        const int e = tid + 256 * u, i = e / (S / 4), j = 4 * (e % (S / 4));
        *(float4 *) (a.s_out + so + (size_t) i * S + j) = make_float4(Ss[j * PS + i], Ss[(j + 1) * PS + i], Ss[(j + 2) * PS + i], Ss[(j + 3) * PS + i]);
    }
}

// The defaults, measured (tools/wkv_bench.py --legs prompt7, profiles/wkv7_chunk_bench.txt).  One sequence (128 workgroups) wins from 32 tokens at both head
// sizes (16 loses at S = 64), but one chunk + 1 is the floor and 48 tokens were measured at one sequence only; at four sequences (512 workgroups: two rounds of the 256 CUs)
// it wins at 64 / 128 / 512 tokens, at eight (1024) it loses at every token count, as k_wkv6_chunk does: further sequences come free to the latency-bound serial kernel.
#define WKV7_CHUNK_MIN_TOKENS 64             // tokens per sequence: the smallest count measured at every grid within the bound, and a win at all of them
#define WKV7_CHUNK_MAX_WGS 512               // workgroups (heads x sequences x S / 32): 256 (head, sequence) pairs at S = 64, 128 at S = 128

static long g_wkv7_chunk_launches = 0;
long wkv7_chunk_launches() { return g_wkv7_chunk_launches; }

int wkv7_chunk_min_tokens() {                // MI355X_WKV_CHUNK_MIN_TOKENS raises it, as it raises WKV6's
    static const int v = [] {
        const char * e = getenv("MI355X_WKV_CHUNK_MIN_TOKENS");
        const long n = e ? atol(e) : WKV7_CHUNK_MIN_TOKENS;
        return (int) (n < WKV7_CHUNK_MIN_TOKENS ? WKV7_CHUNK_MIN_TOKENS : n > INT32_MAX ? INT32_MAX : n);
    }();
    return v;
}

bool wkv7_chunk_takes(int64_t S, int64_t tokens_per_seq, bool aligned, int64_t head_seqs) {
    const int mode = wkv_chunk_mode();
    if (mode == 0 || (S != 64 && S != 128) || !aligned) return false;
    if (mode == 2) return tokens_per_seq >= 1;
    return tokens_per_seq >= wkv7_chunk_min_tokens() && head_seqs * (S / 32) <= WKV7_CHUNK_MAX_WGS;
}

// the caller (wkv7_f32) has passed wkv_ok and wkv7_chunk_takes
void wkv7_chunk_f32(const float * r, const float * w, const float * k, const float * v, const float * av, const float * b, const float * s_in, float * out, float * s_out,
                    int64_t S, int64_t H, int64_t n_t, int64_t n_seqs, hipStream_t st) {
    const wkv7_chunk_args a = { r, w, k, v, av, b, s_in, out, s_out, (int) H, (int) n_t };
    const dim3 grid((unsigned) (S / 32), (unsigned) H, (unsigned) n_seqs);
    auto go = [&](auto hs) {
        constexpr int HS = decltype(hs)::value;
        constexpr size_t lds = (size_t) w7_cfg<HS>::floats * 4;
        static_assert(lds <= 152 * 1024, "the chunk's LDS");
        HIP_CHECK(hipFuncSetAttribute((const void *) k_wkv7_chunk<HS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds));
        k_wkv7_chunk<HS><<<grid, dim3(256), lds, st>>>(a);
    };
    if (S == 64) go(std::integral_constant<int, 64>()); else go(std::integral_constant<int, 128>());
    ++g_wkv7_chunk_launches;
}

} // namespace mi
