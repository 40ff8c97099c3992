// wkv_chunk.hip -- RWKV_WKV6 and GATED_LINEAR_ATTN for prompts: the recurrences of wkv.hip's k_wkv6 over CHUNKS of L tokens on the f32 matrix cores (gfx950 / wave64).
//
// What it takes (wkv_chunk_takes): head size 64 or 128, 16-byte aligned operands, at least wkv_chunk_min_tokens() tokens per sequence (64; MI355X_WKV_CHUNK_MIN_TOKENS
// raises it), and a grid of at most 512 workgroups at S = 64 (heads x sequences <= 256) resp. 256 at S = 128 (<= 64): beyond that the latency-bound serial kernel, to
// which further sequences come free, is the faster one (measured).  Everything else -- other head sizes, unaligned operands, shorter ubatches and decode, many
// sequences, option "wkv_chunk" = 0 -- stays on the serial kernels of wkv.hip.  wkv6_go (wkv.hip) routes; a node is one launch either way.  RWKV_WKV7 has a chunked
// kernel of its own, wkv7_chunk.hip, under the same option.
//
// The mathematics (ggml_compute_forward_rwkv_wkv6_f32 / _gla_f32 restated; layouts as in wkv.hip's header), per (sequence, head): state s[i][j], i the k index, j the v
// index, decay d_t[i] per CHANNEL and token (td / g).  A decay travels as l = max(logf(|d|), -128) and sg = sign(d) (+1 for 0); products of decays are sums of l and
// products of sg.  exp(-128) is 0 in f32, so a zero decay is a factor that is exactly 0; negative decays live in the sign products; nothing depends on a model's (0, 1].
// With D(x, y] = prod_{x < u <= y} d_u and o_t = t - 1 (WKV6: the output reads the state BEFORE token t's update) or t (GLA: after it), over a chunk that starts at 0:
//     out_t = sum_{s <= o_t} (sum_i r_t[i] k_s[i] D(s, o_t][i]) v_s  +  (r_t o D(-1, o_t]) . s_in      (+ WKV6: (sum_i r_t[i] tf[i] k_t[i]) v_t; GLA: r = q * scale)
//     s_out = diag(D(-1, L-1]) s_in  +  sum_s (k_s o D(s, L-1]) (x) v_s
// D of one channel spans many orders of magnitude, so the score matrix A[t][s] does not factor as (r o e^c)(k o e^-c)^T without overflow.  NO POSITIVE EXPONENT of a
// (0, 1] decay is ever formed: the chunk is cut into sub-chunks of 16 tokens, and every D is split at sub-chunk boundaries into three factors that are each <= 1:
//     rt_t = r_t o D(a-1, o_t]     r decayed FROM the start a of its sub-chunk               (tile Rt)
//     kh_s = k_s o D(s, e]         k decayed TO the end e of its sub-chunk                   (tile Kh)
//     G[c1][c2] = the product of the whole sub-chunks c1 <= c < c2, per channel              (table Gt, (NSC + 1)^2 rows; G[c][c] = 1)
//   off-diagonal block (query sub-chunk qa, key sub-chunk kb < qa):  A = Rt (Kh o G[kb+1][qa])^T                    an MFMA product over the S channels
//   the s_in term of sub-chunk qa:                                   (Rt o G[0][qa]) s_in                           an MFMA product over the S channels
//   state:                                                           s = diag(G[0][NSC]) s + (Kh o G[kb+1][NSC])^T V an MFMA product over the L tokens
//   diagonal block (both tokens in one sub-chunk):  A[t][s] = sum_i rs_t[i] ks_s[i] exp(e_t[i] - p_s[i]) for s <= o_t, element by element on the VALU, with p the
//     prefix sum of l INSIDE the sub-chunk, e_t = p_{o_t}, and rs / ks the operands times their sign prefixes (tiles Rs, Ks, Pl); 0 above the diagonal; the WKV6 diagonal is
//     u_t = sum_i r_t tf k_t, reduced over the wave's lanes while the sub-chunk is scanned.  Prefix sums never leave a sub-chunk, so their magnitudes stay small.
// Decays above 1 give positive exponents only where the serial recurrence's own state grows by the same factor.
//
// Grid: one 4-wave workgroup per (32-column slice of v and of the state, head, sequence) -- x = S / 32, y = H, z = n_seqs -- that walks the sequence's chunks in order: one
// launch, no scratch, no reduction across workgroups; A is recomputed per slice (2 x / 4 x the workgroups of a head: 128 at one 7B sequence).  L = 64 tokens at S = 64,
// 32 at S = 128 (the five S-wide tiles: 87 KB either way; L = 64 at S = 128 would need 169 KB for them alone).  NSC = L / 16 sub-chunks.
// All products on __builtin_amdgcn_mfma_f32_16x16x4f32, f32 operands: lane (lm = lane % 16, lk = lane / 16) supplies A[lm][k = lk] and B[k = lk][lm]; accumulator r holds
// row 4 lk + r, column lm.  Sixteen-token sub-chunks make 16 x 16 the natural tile, and every wave gets the same number of them.
// Per chunk:
//   1. stage: k, r, d [L][S] and the v slice [L][32] from the registers the previous chunk's products ran under, 16-byte writes (the NEXT chunk's 16-byte global loads
//      are requested right after, before barrier 1); rows past n_t are staged as k = r = v = 0, d = 1: no second code path, and the state update stays exact.
//   2. scan (after barrier 1): thread = (sub-chunk, channel) -- NSC * S = 256 at both head sizes -- walks its 16 tokens: l, sg, the prefixes, then Rs, Ks, Pl IN PLACE
//      (the thread re-reads and overwrites only its own elements), Rt, Kh, the sub-chunk's totals, and u_t (WKV6) by xor-shuffles.
//   3. (after barrier 2) the table G from the totals; the diagonal blocks: 4 / NSC waves per block, lane = (t = lm; 4 or 2 key tokens), 16-byte reads along the channels,
//      one fast exponential (__expf: |argument| <= 16 tokens of l where the term matters) per (pair, channel).  Written to At with zeros above the diagonal.
//   4. (after barrier 3) the off-diagonal blocks -> At; the s_in term of this wave's output tiles (needs no At).
//   5. (after barrier 4) out tile += At V over the key sub-chunks kb <= qa only (nothing above the diagonal is multiplied), stored for t < n_t, 64 contiguous bytes per
//      16 lanes; the state update.  The state slice lives in ACCUMULATOR registers for the whole sequence (S / 64 x 2 tiles per wave); it is written to LDS once per
//      chunk, the B operand of the next chunk's s_in term, and goes to s_out from there at the end.  Barrier 5 ends the chunk.
//   Output tiles (L / 16 x 2): wave w the column half w % 2 and, at L = 64, the sub-chunks w / 2 and 3 - w / 2: 5 key blocks of At V for every wave.
// Start: s_in slice -> LDS (16-byte loads) -> accumulators.  End: LDS -> s_out (16-byte stores).
//
// LDS (floats; pitches PB = S + 4 for the five S-wide tiles, PS = PV = 36 for the state and v slices, PA = L + 4 for At):
//   5 L PB + S PS + L PV + L PA + (NSC + 1)^2 S + 2 NSC S + 2 L = 131 840 bytes at S = 64, 119 040 at S = 128: one workgroup per CU, under the 152 KiB rule.  Dynamic.
// LDS banks (bank = dword address mod 64; a 16-byte access is served a quarter wave at a time), the argument of ssm_chunk.hip for these pitches:
//   along a row (contraction over channels: Rt, Kh, Gt; over key tokens: At): lane (lm, lk) reads the four dwords 16 j + 4 lk .. + 3 of row lm, one ds_read_b128 for four
//     MFMAs.  A quarter wave is 16 rows at one column: banks 4 (P / 4) lm' + 0 .. 3 with P / 4 = 17 / 33 (PB), 17 / 9 (PA) odd: the 16 lanes take the 64 banks once.  A
//     row of Gt is the same for all lm: a broadcast.
//   across rows (contraction over channels: the state slice; over tokens: Kh, v): MFMA e of a group reads row 4 lk + e at column lm: the four lk lie 4 rows apart, and
//     4 PB = 4 PS = 4 PV = 16 mod 64 (PB = 68 / 132, 36): four runs of 16 consecutive dwords at banks 0 / 16 / 32 / 48: the 64 lanes take the 64 banks once.
//   accumulator -> LDS (At blocks, the state slice): the same pattern, rows 4 lk + r, 4 PA = 16 mod 64 as well.  The scan reads and writes columns: consecutive lanes,
//     consecutive dwords.  The diagonal blocks read row lm (the query) as above and 4 distinct key rows per wave (broadcasts).  Derived from the bank rule, not counted.
// Registers (-Rpass-analysis=kernel-resource-usage, gfx950; VGPR / AGPR, scratch 0 in every instance, no spill): <64, WKV6> 248 / 12, <64, GLA> 221 / 12,
//   <128, WKV6> 229 / 16, <128, GLA> 218 / 16.  The chunk's loads go through a by-value helper (wc_ld4): `in ? *p : zero` on float4s became a select of POINTERS and put
//   the fetch registers into 272 bytes of scratch.  The LDS is dynamic (the remark shows 0): the sizes are the ones above, asserted against 152 KiB where the kernel is
//   launched.  One workgroup per CU by its LDS, so one wave per SIMD.  Built with -packed-fp32-ops off (Makefile): the accumulators are scaled between MFMA runs.
// Measured (tools/wkv_bench.py, profiles/wkv_chunk_bench.txt; 64 heads of 64, one sequence): 512 tokens WKV6 123 us against k_wkv6's 307, GLA 119 against 269; 15 us per
//   64-token chunk, about eight times the issue time of a wave's 140 MFMAs (1.9 us at 2.4 GHz): with one wave per SIMD nothing hides the scan's logf / expf chains, the
//   256 exponentials per lane of the diagonal block, the LDS round trips and the five barriers.  32 heads of 128 gain least (WKV6 232 against 278: twice the chunks, and
//   u_t costs 96 shuffles in each).  Not done: more than one wave per SIMD (a smaller chunk footprint), a shuffle tree for u_t, the diagonal block on half the pairs.
#include "../kernels.hpp"
#include <type_traits>

namespace mi {

typedef float wc_f4a __attribute__((ext_vector_type(4)));

struct wkv_chunk_args {
    const float * k, * v, * r, * tf, * d;    // {S, H, T}; tf {S, H} (WKV6); d = td / g; r = q for GLA
    const float * s_in;                      // previous states, sequence q at q * S * S * H
    float * out, * s_out;                    // {S * H, T} outputs; new states
    float scale;                             // GLA
    int H, n_t;                              // heads; tokens per sequence
};

template <int S> struct wc_cfg {
    static constexpr int L = S == 64 ? 64 : 32, NSC = L / 16, NG = NSC + 1;      // tokens per chunk, sub-chunks, rows / columns of the table G
    static constexpr int PB = S + 4, PS = 36, PV = 36, PA = L + 4;
    static constexpr int oR = 0, oK = oR + L * PB, oP = oK + L * PB, oRt = oP + L * PB, oKh = oRt + L * PB, oS = oKh + L * PB, oV = oS + S * PS, oA = oV + L * PV,
                         oG = oA + L * PA, oT = oG + NG * NG * S, oSg = oT + NSC * S, oU = oSg + NSC * S;
    static constexpr int floats = oU + 2 * L;
};

static __device__ __forceinline__ wc_f4a wc_mma(float a, float b, wc_f4a c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

static __device__ __forceinline__ float4 wc_ld4(const float * p, bool in, float fill) {      // a row of the chunk, or the filler past the sequence's end
    float4 v = make_float4(fill, fill, fill, fill);
    if (in) v = *(const float4 *) p;
    return v;
}

extern __shared__ float4 wc_lds4[];

template <int S, bool GLA>
__global__ void __launch_bounds__(256) k_wkv6_chunk(const wkv_chunk_args a) {
    using K = wc_cfg<S>;
    constexpr int L = K::L, NSC = K::NSC, NG = K::NG, PB = K::PB, PS = K::PS, PV = K::PV, PA = K::PA;
    constexpr int NV4 = L / 32, NS4 = S / 32;                // float4s per thread: a chunk of the v slice, the state slice (k, r, d: 4 at both head sizes)
    constexpr int NWD = 4 / NSC, PPL = 4 / NWD;              // waves per diagonal block, key tokens per lane in it
    constexpr int NOFF = NSC * (NSC - 1) / 2;                // off-diagonal blocks
    constexpr int NOT = L / 32, IPW = S / 64;                // output tiles per wave; state row blocks of 16 per wave (two tiles each)
    static_assert(L * S == 4096 && NSC * S == 256, "the thread maps of the staging and of the scan");
    float * lds = (float *) wc_lds4;
    float * Rs = lds + K::oR, * Ks = lds + K::oK, * Pl = lds + K::oP, * Rt = lds + K::oRt, * Kh = lds + K::oKh, * Ss = lds + K::oS, * Vs = lds + K::oV, * At = lds + K::oA;
    float * Gt = lds + K::oG, * Tot = lds + K::oT, * Sg = lds + K::oSg, * Ud = lds + K::oU;

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lm = lane & 15, lk = lane >> 4;
    const int j0 = blockIdx.x * 32, h = blockIdx.y, seq = blockIdx.z;
    const size_t C = (size_t) a.H * S, so = ((size_t) seq * a.H + h) * S * S + j0;
    const size_t base = (size_t) seq * a.n_t * C + (size_t) h * S;       // token 0 of the sequence, this head
    const float * kp = a.k + base, * rp = a.r + base, * dp = a.d + base, * vp = a.v + base + j0;
    float * op = a.out + base + j0;
    const int sc = tid / S, si = tid % S;                    // the scan: this thread's sub-chunk and channel
    const float tfi = GLA ? 0.0f : a.tf[(size_t) h * S + si];
    const int nh = w & 1;                                    // the column half of this wave's output tiles

    // the chunk at t0 .. t0 + L - 1, requested into registers one chunk ahead
    float4 gk[4], gr[4], gd[4], gv[NV4];
    auto fetch = [&](int t0) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = tid + 256 * u, t = t0 + e / (S / 4), c4 = e % (S / 4);
            const bool in = t < a.n_t;
            const size_t o = (size_t) t * C + 4 * c4;
            gk[u] = wc_ld4(kp + o, in, 0.0f); gr[u] = wc_ld4(rp + o, in, 0.0f); gd[u] = wc_ld4(dp + o, in, 1.0f);
        }
#pragma unroll
        for (int u = 0; u < NV4; ++u) {
            const int e = tid + 256 * u, t = t0 + (e >> 3), c4 = e & 7;
            gv[u] = wc_ld4(vp + (size_t) t * C + 4 * c4, t < a.n_t, 0.0f);
        }
    };

    // the state slice: s_in -> LDS -> this wave's tiles
#pragma unroll
    for (int u = 0; u < NS4; ++u) {
        const int e = tid + 256 * u, row = e >> 3, c4 = e & 7;
        *(float4 *) (Ss + row * PS + 4 * c4) = *(const float4 *) (a.s_in + so + (size_t) row * S + 4 * c4);
    }
    fetch(0);
    __syncthreads();
    wc_f4a acc[IPW][2];
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
        for (int u = 0; u < 4; ++u) {
            const int e = tid + 256 * u, o = (e / (S / 4)) * PB + 4 * (e % (S / 4));
            *(float4 *) (Ks + o) = gk[u]; *(float4 *) (Rs + o) = gr[u]; *(float4 *) (Pl + o) = gd[u];
        }
#pragma unroll
        for (int u = 0; u < NV4; ++u) {
            const int e = tid + 256 * u;
            *(float4 *) (Vs + (e >> 3) * PV + 4 * (e & 7)) = gv[u];
        }
        if (t0 + L < a.n_t) fetch(t0 + L);
        __syncthreads();                                     // 1: the chunk is staged

        // 2. scan: 16 tokens of one channel
        {
            float p = 0.0f, sg = 1.0f, pl[16], ks[16], ud[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int o = (16 * sc + u) * PB + si;
                const float d = Pl[o], k = Ks[o];
                const float r = GLA ? Rs[o] * a.scale : Rs[o];
                const float l = fmaxf(logf(fabsf(d)), -128.0f);
                float e = p, se = sg;                        // WKV6: the decays before token t
                p += l; sg = d < 0.0f ? -sg : sg;
                if (GLA) { e = p; se = sg; }                 // GLA: token t's included
                const float rs = r * se;
                ks[u] = k * sg; pl[u] = p;
                Rs[o] = rs; Rt[o] = rs * expf(e); Ks[o] = ks[u]; Pl[o] = p;
                ud[u] = GLA ? 0.0f : r * tfi * k;
            }
#pragma unroll
            for (int u = 0; u < 16; ++u) Kh[(16 * sc + u) * PB + si] = ks[u] * sg * expf(p - pl[u]);      // (ks carries the signs up to s, sg up to the end: their product is the signs after s)
            Tot[sc * S + si] = p; Sg[sc * S + si] = sg;
            if (!GLA) {
#pragma unroll
                for (int u = 0; u < 16; ++u) {
#pragma unroll
                    for (int m = 1; m < 64; m <<= 1) ud[u] += __shfl_xor(ud[u], m, 64);
                }
                if (lane == 0) {                             // (S = 128: a wave holds half of the channels, the reader adds the halves)
#pragma unroll
                    for (int u = 0; u < 16; ++u) Ud[(S == 128 ? (w & 1) : 0) * L + 16 * sc + u] = ud[u];
                }
            }
        }
        __syncthreads();                                     // 2: the five tiles and the totals

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
            const bool he = GLA || lm > 0;                   // WKV6's e of a sub-chunk's first token is 0
            const float * rrow = Rs + t * PB, * erow = Pl + (GLA ? t : (lm > 0 ? t - 1 : t)) * PB;
            float da[PPL];
#pragma unroll
            for (int u = 0; u < PPL; ++u) da[u] = 0.0f;
#pragma unroll 2
            for (int i = 0; i < S; i += 4) {
                const float4 r4 = *(const float4 *) (rrow + i);
                float4 e4 = *(const float4 *) (erow + i);
                if (!he) e4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
                for (int u = 0; u < PPL; ++u) {
                    const float4 k4 = *(const float4 *) (Ks + (s0 + u) * PB + i), p4 = *(const float4 *) (Pl + (s0 + u) * PB + i);
                    da[u] += r4.x * k4.x * __expf(e4.x - p4.x); da[u] += r4.y * k4.y * __expf(e4.y - p4.y);
                    da[u] += r4.z * k4.z * __expf(e4.z - p4.z); da[u] += r4.w * k4.w * __expf(e4.w - p4.w);
                }
            }
            const float ut = GLA ? 0.0f : Ud[t] + (S == 128 ? Ud[L + t] : 0.0f);
#pragma unroll
            for (int u = 0; u < PPL; ++u) {                  // (a pair above the diagonal may hold inf or nan: selected away, never multiplied)
                const int s = sl + u;
                da[u] = GLA ? (s <= lm ? da[u] : 0.0f) : (s < lm ? da[u] : s == lm ? ut : 0.0f);
            }
            if constexpr (PPL == 4) *(float4 *) (At + t * PA + s0) = make_float4(da[0], da[1], da[2], da[3]);
            else                    *(float2 *) (At + t * PA + s0) = make_float2(da[0], da[1]);
        }
        __syncthreads();                                     // 3: G

        // 4. the off-diagonal blocks; the s_in term of this wave's output tiles
        for (int b = 3 - w; b < NOFF; b += 4) {
            int qa = 1, kb = b;
            while (kb >= qa) { kb -= qa; ++qa; }
            const float * ar = Rt + (16 * qa + lm) * PB + 4 * lk, * br = Kh + (16 * kb + lm) * PB + 4 * lk, * gp = Gt + ((kb + 1) * NG + qa) * S + 4 * lk;
            wc_f4a sa = { 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll 4
            for (int j = 0; j < S; j += 16) {
                const float4 a4 = *(const float4 *) (ar + j), b4 = *(const float4 *) (br + j), g4 = *(const float4 *) (gp + j);
                sa = wc_mma(a4.x, b4.x * g4.x, sa); sa = wc_mma(a4.y, b4.y * g4.y, sa); sa = wc_mma(a4.z, b4.z * g4.z, sa); sa = wc_mma(a4.w, b4.w * g4.w, sa);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) At[(16 * qa + 4 * lk + r) * PA + 16 * kb + lm] = sa[r];
        }
        wc_f4a oa[NOT];
#pragma unroll
        for (int q = 0; q < NOT; ++q) {
            const int qa = NOT == 2 ? (q == 0 ? w >> 1 : 3 - (w >> 1)) : w >> 1;
            const float * ar = Rt + (16 * qa + lm) * PB + 4 * lk, * gp = Gt + qa * S + 4 * lk, * bs = Ss + 4 * lk * PS + 16 * nh + lm;
            oa[q] = wc_f4a{ 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll 4
            for (int j = 0; j < S; j += 16) {
                const float4 a4 = *(const float4 *) (ar + j), g4 = *(const float4 *) (gp + j);
                oa[q] = wc_mma(a4.x * g4.x, bs[(j + 0) * PS], oa[q]); oa[q] = wc_mma(a4.y * g4.y, bs[(j + 1) * PS], oa[q]);
                oa[q] = wc_mma(a4.z * g4.z, bs[(j + 2) * PS], oa[q]); oa[q] = wc_mma(a4.w * g4.w, bs[(j + 3) * PS], oa[q]);
            }
        }
        __syncthreads();                                     // 4: At is whole, the old state slice is read

        // 5. out = At V + the s_in term; the state
#pragma unroll
        for (int q = 0; q < NOT; ++q) {
            const int qa = NOT == 2 ? (q == 0 ? w >> 1 : 3 - (w >> 1)) : w >> 1;
            const float * ar = At + (16 * qa + lm) * PA + 4 * lk, * bv = Vs + 4 * lk * PV + 16 * nh + lm;
            for (int kb = 0; kb <= qa; ++kb) {
                const float4 a4 = *(const float4 *) (ar + 16 * kb);
                const float * b = bv + 16 * kb * PV;
                oa[q] = wc_mma(a4.x, b[0], oa[q]); oa[q] = wc_mma(a4.y, b[PV], oa[q]); oa[q] = wc_mma(a4.z, b[2 * PV], oa[q]); oa[q] = wc_mma(a4.w, b[3 * PV], oa[q]);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int t = t0 + 16 * qa + 4 * lk + r;
                if (t < a.n_t) op[(size_t) t * C + 16 * nh + lm] = oa[q][r];
            }
        }
#pragma unroll
        for (int x = 0; x < IPW; ++x) {
            const int i0 = 16 * (w * IPW + x);
            const float4 g0 = *(const float4 *) (Gt + NSC * S + i0 + 4 * lk);      // G[0][NSC] of this lane's four rows
            acc[x][0][0] *= g0.x; acc[x][0][1] *= g0.y; acc[x][0][2] *= g0.z; acc[x][0][3] *= g0.w;
            acc[x][1][0] *= g0.x; acc[x][1][1] *= g0.y; acc[x][1][2] *= g0.z; acc[x][1][3] *= g0.w;
#pragma unroll
            for (int kb = 0; kb < NSC; ++kb) {
                const float g = Gt[((kb + 1) * NG + NSC) * S + i0 + lm];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int s = 16 * kb + 4 * lk + e;
                    const float av = Kh[s * PB + i0 + lm] * g;
                    acc[x][0] = wc_mma(av, Vs[s * PV + lm], acc[x][0]); acc[x][1] = wc_mma(av, Vs[s * PV + 16 + lm], acc[x][1]);
                }
            }
#pragma unroll
            for (int n = 0; n < 2; ++n) {
#pragma unroll
                for (int r = 0; r < 4; ++r) Ss[(i0 + 4 * lk + r) * PS + 16 * n + lm] = acc[x][n][r];
            }
        }
        __syncthreads();                                     // 5: the new state slice is written; every read of the staged chunk is done
    }

    // the final slice (barrier 5 of the last chunk made it visible)
#pragma unroll
    for (int u = 0; u < NS4; ++u) {
        const int e = tid + 256 * u, row = e >> 3, c4 = e & 7;
        *(float4 *) (a.s_out + so + (size_t) row * S + 4 * c4) = *(const float4 *) (Ss + row * PS + 4 * c4);
    }
}

#define WKV_CHUNK_MIN_TOKENS 64              // the default threshold (where it was measured)
#define WKV_CHUNK_CUS 256                    // compute units of an MI355X: one workgroup each

static long g_wkv6_chunk_launches = 0, g_gla_chunk_launches = 0;
long wkv6_chunk_launches() { return g_wkv6_chunk_launches; }
long gla_chunk_launches() { return g_gla_chunk_launches; }
static int g_wkv_chunk_mode = -1;
void wkv_chunk_set_mode(int m) { g_wkv_chunk_mode = m; }

int wkv_chunk_min_tokens() {
    static const int v = [] {
        const char * e = getenv("MI355X_WKV_CHUNK_MIN_TOKENS");
        const long n = e ? atol(e) : WKV_CHUNK_MIN_TOKENS;
        return (int) (n < WKV_CHUNK_MIN_TOKENS ? WKV_CHUNK_MIN_TOKENS : n > INT32_MAX ? INT32_MAX : n);
    }();
    return v;
}

int wkv_chunk_mode() {                       // the option and MI355X_WKV_CHUNK folded: 0 off, 1 by threshold, 2 every token count and grid
    static const bool env_on = [] { const char * e = getenv("MI355X_WKV_CHUNK"); return !e || atoi(e) != 0; }();
    return g_wkv_chunk_mode == 0 || (g_wkv_chunk_mode < 0 && !env_on) ? 0 : g_wkv_chunk_mode == 2 ? 2 : 1;
}

bool wkv_chunk_takes(int64_t S, int64_t tokens_per_seq, bool aligned, int64_t head_seqs) {
    const int mode = wkv_chunk_mode();
    if (mode == 0 || (S != 64 && S != 128) || !aligned) return false;
    if (mode == 2) return tokens_per_seq >= 1;       // 2: every token count and grid (tools/wkv_bench.py locates the crossovers with it)
    // the serial kernel is latency-bound: further sequences cost it nothing until the machine is full, while this kernel's time multiplies with every round of 256
    // workgroups.  Measured (profiles/wkv_chunk_bench.txt): two rounds still win at S = 64, at S = 128 only one does.
    return tokens_per_seq >= wkv_chunk_min_tokens() && head_seqs * (S / 32) <= (S == 64 ? 2 : 1) * WKV_CHUNK_CUS;
}

// the caller (wkv6_go) has passed wkv_ok and wkv_chunk_takes
void wkv6_chunk_f32(bool gla, const float * k, const float * v, const float * r, const float * tf, const float * d, const float * s_in, float * out, float * s_out, float scale,
                    int64_t S, int64_t H, int64_t n_t, int64_t n_seqs, hipStream_t st) {
    const wkv_chunk_args a = { k, v, r, tf, d, s_in, out, s_out, scale, (int) H, (int) n_t };
    const dim3 grid((unsigned) (S / 32), (unsigned) H, (unsigned) n_seqs);
    auto go = [&](auto hs, auto g) {
        constexpr int HS = decltype(hs)::value;
        constexpr bool G = decltype(g)::value;
        constexpr size_t lds = (size_t) wc_cfg<HS>::floats * 4;
        static_assert(lds <= 152 * 1024, "the chunk's LDS");
        HIP_CHECK(hipFuncSetAttribute((const void *) k_wkv6_chunk<HS, G>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds));
        k_wkv6_chunk<HS, G><<<grid, dim3(256), lds, st>>>(a);
    };
    if (S == 64) { if (gla) go(std::integral_constant<int, 64>(), std::true_type());  else go(std::integral_constant<int, 64>(), std::false_type()); }
    else         { if (gla) go(std::integral_constant<int, 128>(), std::true_type()); else go(std::integral_constant<int, 128>(), std::false_type()); }
    ++(gla ? g_gla_chunk_launches : g_wkv6_chunk_launches);
}

} // namespace mi
