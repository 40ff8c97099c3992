// ssm_chunk.hip -- SSM_SCAN for Mamba-2 prompts: the recurrence of ssm.hip's k_ssm_scan over CHUNKS of Q tokens on the f32 matrix cores (gfx950 / wave64).
//
// What it takes (ssm_chunk_takes): one decay per head and token (A {1, n_head}), head_dim a multiple of 32, d_state 64 / 128 / 256, at least
// ssm_chunk_min_tokens() tokens (128; MI355X_SSM_CHUNK_MIN_TOKENS raises it).  Everything else -- Mamba-1 (A {d_state, n_head}), other head_dims, d_state 16 / 32,
// shorter ubatches, option "ssm_chunk" = 0 -- stays on k_ssm_scan.  ssm_scan_f32 (ssm.hip) routes; a node is one launch either way.
//
// The mathematics (ggml_compute_forward_ssm_scan_f32 restated), per (sequence, head h, group g): dt'_t = softplus(dt_t[h]), a_t = dt'_t A[h], x~_t = x_t dt'_t, state
// S[p][n].  Over a chunk of Q tokens with c_j = sum_{i <= j} a_i:
//     y_j   = exp(c_j) (S_in C_j)  +  sum_{i <= j} exp(c_j - c_i) (C_j . B_i) x~_i
//     S_out = exp(c_{Q-1}) S_in    +  sum_i exp(c_{Q-1} - c_i) x~_i (x) B_i
// Only exp(c_j) and exp(c_j - c_i) with i <= j are formed (<= 1 for A < 0), never exp(-c_i).  The prefix sum runs in f64 on one wave and is rounded to f32 once.
//
// Grid: one 4-wave workgroup per (sequence, head, 32-row slice of head_dim) -- x = n_head * head_dim / 32, y = n_s -- that walks the sequence's chunks in order: one
// launch, no scratch, no reduction across workgroups; G below is recomputed per slice.  Q = 64 tokens; 32 at d_state 256 (LDS).  lane = (lq = lane % 32, hb = lane / 32).
// Per chunk, all products on __builtin_amdgcn_mfma_f32_32x32x2f32 (lane (lq, hb) supplies A[lq][k = hb], B[k = hb][lq]; accumulator r holds row 8 (r / 4) + 4 hb + r % 4,
// column lq), f32 operands throughout:
//   1. stage: B [Q][d_state], C [Q][d_state], x~ [Q][32] from the registers the previous chunk's products ran under (the NEXT chunk's global loads are requested right
//      after, before barrier A); rows past n_t are staged as zeros with a = 0.  Wave 0, lane = token: a, the prefix sum c, e = exp(c), w = exp(c_{Q-1} - c).
//   2. G = C B^T.  Q = 64: one 32 x 32 quadrant per wave over the whole d_state, the quadrant above the diagonal skipped (wave 3 goes straight to 3a).  Q = 32: one
//      quadrant, its contraction cut in four, the partials folded by wave 0 through the fold area in wave order (one more barrier, this instance only).  Each element is
//      multiplied by exp(c_j - c_i) where i <= j, else 0, and M = L o G is written TRANSPOSED, Mt[i][j], as four 16-byte writes per lane.
//   3. Y = M X~ + diag(e) (C S_in^T), waves as (row half, contraction part): 2 x 2 at Q = 64, 1 x 4 at Q = 32.  3a, C S_in^T over the wave's part of d_state, needs no M and
//      runs before barrier B; 3b, M X~ over the wave's part of the tokens (the part above the diagonal skipped), after it.  The parts > 0 write to the fold area; after
//      barrier C part 0 adds them in part order and stores y for t < n_t, 128 contiguous bytes per half wave.
//   4. S = e_{Q-1} S + X~^T (w o B): the state slice lives in ACCUMULATOR registers for the whole sequence, wave w the columns [w d_state / 4, (w + 1) d_state / 4) (one
//      tile at 128, two at 256; at 64 there are two tiles and waves 2, 3 have none).  w_i multiplies the B operand as it is read.  The slice is written to LDS once per
//      chunk (after barrier B: 3a has read the old one), the B operand of the next chunk's 3a.
//   Barriers per chunk: A (staged), B (Mt), C (fold area, new S): 3, 4 at Q = 32.
// Start: the slice of row ids[seq] of s (ids is read on the device: it changes between graph replays) -> LDS -> accumulators.  End: LDS -> dst behind y.  Both, and the
// chunk loads, are 16-byte accesses where bases and strides allow (al), 4-byte otherwise; x, B, C, dt go through their strides (views of one xBC tensor).
//
// LDS (floats; pitches PB = d_state + 4 for B, C, S; PX = 36 for x~; PM = Q + 4 for Mt; PY = 40 for the fold area): 2 Q PB + 32 PB + Q PX + Q PM + (4 / (Q / 32) - 1) Q PY + 3 Q
//   = 81 152 bytes at 64, 122 112 at 128, 124 800 at 256: one workgroup per CU, under the 152 KiB rule.  Dynamic, with the attribute.
// LDS banks (bank = dword address mod 64; a 16-byte access is served a quarter wave at a time).  Two read forms, one per contraction direction:
//   along a row (G, 3a: contraction over d_state; rows of C, B, S): lane (lq, hb) reads the four dwords 8 s + 4 hb .. + 3 of row lq, one ds_read_b128 for four MFMAs.  A
//     quarter wave is 16 rows at one column: banks 4 (PB / 4) lq' + 0 .. 3, and PB / 4 = 17 / 33 / 65 is odd, so the 16 lanes take the 64 banks once.
//   across rows (3b, 4: contraction over tokens; rows of Mt, x~, B): step s reads token 16 (s / 8) + 8 hb + s % 8 at column lq: the halves lie 8 rows apart,
//     8 PB = 8 PX = 8 PM = 32 mod 64 (PB = 4 mod 64, PX = 36, PM = 68 / 36), 32 consecutive dwords each: the 64 lanes take the 64 banks once.
//   Writes: staging and Mt are 16-byte writes to consecutive slots of a row (PM / 4 odd, as above).  The accumulator -> LDS writes of S and of the fold area put the
//     halves 4 rows apart: 4 PY = 32 mod 64 is conflict-free for the fold area, 4 PB = 16 mod 64 is a two-way conflict for S -- 16 writes per tile and chunk, left as it
//     is: PB cannot serve this and the 16-byte row reads at once.  Derived from the bank rule, not counted: no counter run was made.
// Registers (-Rpass-analysis=kernel-resource-usage, gfx950; VGPR / AGPR, scratch 0 in every instance, no spill): d_state 64: 170 / 48, 128: 216 / 32, 256: 245 / 48.  The
//   LDS is dynamic (the remark shows 0): the sizes are the ones above, asserted against 152 KiB where the kernel is launched.  One workgroup per CU by its LDS, so one
//   wave per SIMD.  Built with -packed-fp32-ops off (Makefile): no packed-f32 instruction in the object.
// Measured (tools/ssm_bench.py, profiles/ssm_bench.txt; 80 heads of 64, d_state 128, one sequence): 512 tokens 89 us against k_ssm_scan's 445; 128 tokens 25.7 against 115.
//   Not balanced yet: at Q = 64 wave 3 has no G quadrant, and 160 workgroups leave 96 of the 256 CUs idle at one sequence.
#include "../kernels.hpp"
#include <type_traits>

namespace mi {

typedef float sc_f16a __attribute__((ext_vector_type(16)));

struct ssm_chunk_args {
    const char * s; size_t s_nb3;                            // states {d_state, head_dim, n_head, n_rows}, contiguous
    const char * x; size_t x_nb2, x_nb3;                     // {head_dim, n_head, n_t, n_s}, dense up to a head row
    const char * dt; size_t dt_nb1, dt_nb2;                  // {n_head, n_t, n_s}
    const char * A; size_t A_nb1;                            // {1, n_head}
    const char * B; const char * C; size_t b_nb1, b_nb2, b_nb3, c_nb1, c_nb2, c_nb3;      // {d_state, n_group, n_t, n_s}
    const int * ids;                                         // {n_s}
    float * y; char * s_out;                                 // y dense {head_dim, n_head, n_t, n_s}; final states, sequence i3 at i3 * s_nb3
    int head_dim, n_head, heads_per_group, n_t;
    bool al;                                                 // every 16-byte global access is aligned
};

template <int DS> struct sc_cfg {
    static constexpr int Q = DS == 256 ? 32 : 64;            // tokens per chunk
    static constexpr int PB = DS + 4, PX = 36, PM = Q + 4, PY = 40;
    static constexpr int RH = Q / 32, KS = 4 / RH;           // row halves of Y, contraction parts
    static constexpr int NT = DS / 32, TPW = NT >= 4 ? NT / 4 : 1;      // state tiles of 32 columns, tiles per wave
    static constexpr int oB = 0, oC = oB + Q * PB, oS = oC + Q * PB, oX = oS + 32 * PB, oM = oX + Q * PX, oY = oM + Q * PM, oV = oY + (KS - 1) * Q * PY;
    static constexpr int floats = oV + 3 * Q;                // c, e, w
};

static __device__ __forceinline__ float sc_softplus(float v) { return v > 20.0f ? v : logf(1.0f + expf(v)); }      // ggml_softplus (ggml-impl.h:105), as ssm.hip
static __device__ __forceinline__ float4 sc_ld4(const float * p, bool al) {
    if (al) return *(const float4 *) p;
    return make_float4(p[0], p[1], p[2], p[3]);
}
static __device__ __forceinline__ void sc_st4(float * p, float4 v, bool al) {
    if (al) { *(float4 *) p = v; return; }
    p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
}
static __device__ __forceinline__ sc_f16a sc_mma(float a, float b, sc_f16a c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
static __device__ __forceinline__ int sc_row(int r, int hb) { return 8 * (r >> 2) + 4 * hb + (r & 3); }      // the tile row of accumulator element r

// acc += A B^T over LEN contraction elements that lie ALONG the rows of both operands: ap / bp = the lane's row + 4 hb + the first element
template <int LEN>
static __device__ __forceinline__ sc_f16a sc_along(const float * ap, const float * bp, sc_f16a acc) {
#pragma unroll 4
    for (int k = 0; k < LEN; k += 8) {
        const float4 av = *(const float4 *) (ap + k), bv = *(const float4 *) (bp + k);
        acc = sc_mma(av.x, bv.x, acc); acc = sc_mma(av.y, bv.y, acc); acc = sc_mma(av.z, bv.z, acc); acc = sc_mma(av.w, bv.w, acc);
    }
    return acc;
}
// acc += A^T B over the tokens of steps s0 .. s0 + CNT - 1, the contraction ACROSS rows (pitches PA, PB_): ap / bp / sc = row 8 hb, the lane's column; SCALE: b times sc[token]
template <int CNT, int PA, int PB_, bool SCALE>
static __device__ __forceinline__ sc_f16a sc_across(const float * ap, const float * bp, const float * sc, int s0, sc_f16a acc) {
#pragma unroll 8
    for (int s = 0; s < CNT; ++s) {
        const int i = 16 * ((s0 + s) >> 3) + ((s0 + s) & 7);
        float b = bp[i * PB_];
        if (SCALE) b *= sc[i];
        acc = sc_mma(ap[i * PA], b, acc);
    }
    return acc;
}

extern __shared__ float4 sc_lds4[];

template <int DS>
__global__ void __launch_bounds__(256) k_ssm_scan_chunk(const ssm_chunk_args a) {
    using K = sc_cfg<DS>;
    constexpr int Q = K::Q, PB = K::PB, PX = K::PX, PM = K::PM, PY = K::PY, KS = K::KS, NT = K::NT, TPW = K::TPW;
    constexpr int NB4 = Q * DS / 1024, NX4 = Q / 32, NS4 = DS / 32;        // float4s per thread: a chunk of B (of C), of x, the state slice
    float * lds = (float *) sc_lds4;
    float * Bs = lds + K::oB, * Cs = lds + K::oC, * Ss = lds + K::oS, * Xs = lds + K::oX, * Mt = lds + K::oM, * Yf = lds + K::oY;
    float * cs = lds + K::oV, * es = cs + Q, * ws = es + Q;

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lq = lane & 31, hb = lane >> 5;
    const int seq = blockIdx.y, sph = a.head_dim >> 5, h = blockIdx.x / sph, p0 = (blockIdx.x - h * sph) * 32, g = h / a.heads_per_group;
    const int rh = w / KS, kh = w % KS;                      // step 3: this wave's row half and contraction part
    const size_t row0 = (size_t) h * a.head_dim + p0;        // flat row of (h, p0): y / x element, state row
    const float Ah = *(const float *) (a.A + (size_t) h * a.A_nb1);
    const char * bp = a.B + (size_t) seq * a.b_nb3 + (size_t) g * a.b_nb1;
    const char * cp = a.C + (size_t) seq * a.c_nb3 + (size_t) g * a.c_nb1;
    const char * xp = a.x + (size_t) seq * a.x_nb3 + row0 * 4;
    const char * dp = a.dt + (size_t) seq * a.dt_nb2 + (size_t) h * 4;
    float * yp = a.y + ((size_t) seq * a.n_t * a.n_head * a.head_dim + row0);
    const size_t y_ts = (size_t) a.n_head * a.head_dim;

    // the chunk at t0 .. t0 + Q - 1, requested into registers one chunk ahead
    float4 rB[NB4], rC[NB4], rX[NX4]; float rdt[NX4], sdt = 0.0f;
    auto fetch = [&](int t0) {
        const float4 z4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
        for (int u = 0; u < NB4; ++u) {
            const int e = tid + 256 * u, t = t0 + e / (DS / 4), c4 = e % (DS / 4);
            const bool in = t < a.n_t;
            rB[u] = in ? sc_ld4((const float *) (bp + (size_t) t * a.b_nb2) + 4 * c4, a.al) : z4;
            rC[u] = in ? sc_ld4((const float *) (cp + (size_t) t * a.c_nb2) + 4 * c4, a.al) : z4;
        }
#pragma unroll
        for (int u = 0; u < NX4; ++u) {
            const int e = tid + 256 * u, t = t0 + (e >> 3), c4 = e & 7;
            const bool in = t < a.n_t;
            rX[u] = in ? sc_ld4((const float *) (xp + (size_t) t * a.x_nb2) + 4 * c4, a.al) : z4;
            rdt[u] = in ? *(const float *) (dp + (size_t) t * a.dt_nb1) : 0.0f;
        }
        sdt = w == 0 && lane < Q && t0 + lane < a.n_t ? *(const float *) (dp + (size_t) (t0 + lane) * a.dt_nb1) : 0.0f;
    };
    auto stage = [&](int t0) {
#pragma unroll
        for (int u = 0; u < NB4; ++u) {
            const int e = tid + 256 * u, o = (e / (DS / 4)) * PB + 4 * (e % (DS / 4));
            *(float4 *) (Bs + o) = rB[u]; *(float4 *) (Cs + o) = rC[u];
        }
#pragma unroll
        for (int u = 0; u < NX4; ++u) {
            const int e = tid + 256 * u;
            const float dsp = sc_softplus(rdt[u]);
            *(float4 *) (Xs + (e >> 3) * PX + 4 * (e & 7)) = make_float4(rX[u].x * dsp, rX[u].y * dsp, rX[u].z * dsp, rX[u].w * dsp);
        }
        if (w == 0) {                                        // lane = token: a, its prefix sum, the three exponentials
            const bool in = lane < Q && t0 + lane < a.n_t;
            double c = in ? (double) (sc_softplus(sdt) * Ah) : 0.0;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) { const double o = __shfl_up(c, d, 64); if (lane >= d) c += o; }
            const float cf = (float) c, cl = __shfl(cf, Q - 1, 64);
            if (lane < Q) { cs[lane] = cf; es[lane] = expf(cf); ws[lane] = expf(cl - cf); }
        }
    };

    // the state slice: row ids[seq] of s -> LDS -> this wave's tiles
    {
        const float * s0 = (const float *) (a.s + (size_t) a.ids[seq] * a.s_nb3) + row0 * DS;
#pragma unroll
        for (int u = 0; u < NS4; ++u) {
            const int e = tid + 256 * u, r = e / (DS / 4), c4 = e % (DS / 4);
            *(float4 *) (Ss + r * PB + 4 * c4) = sc_ld4(s0 + (size_t) r * DS + 4 * c4, a.al);
        }
    }
    fetch(0);
    __syncthreads();
    sc_f16a acc[TPW];
#pragma unroll
    for (int k = 0; k < TPW; ++k) {
        const int tl = w * TPW + k;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[k][r] = tl < NT ? Ss[sc_row(r, hb) * PB + 32 * tl + lq] : 0.0f;
    }

    for (int t0 = 0; t0 < a.n_t; t0 += Q) {
        stage(t0);
        if (t0 + Q < a.n_t) fetch(t0 + Q);
        __syncthreads();                                     // A: the chunk is staged

        // 2. M = L o (C B^T), written transposed
        sc_f16a gacc;
#pragma unroll
        for (int r = 0; r < 16; ++r) gacc[r] = 0.0f;
        int jq = 0, iq = 0;
        bool masks = false;                                  // this wave turns a G quadrant into Mt
        if constexpr (Q == 64) {
            jq = w > 0; iq = w > 1; masks = w < 3;
            if (masks) gacc = sc_along<DS>(Cs + (32 * jq + lq) * PB + 4 * hb, Bs + (32 * iq + lq) * PB + 4 * hb, gacc);
        } else {
            masks = w == 0;
            gacc = sc_along<DS / 4>(Cs + lq * PB + 4 * hb + w * (DS / 4), Bs + lq * PB + 4 * hb + w * (DS / 4), gacc);
            if (w > 0) {
#pragma unroll
                for (int r = 0; r < 16; ++r) Yf[((w - 1) * 32 + sc_row(r, hb)) * PY + lq] = gacc[r];
            }
            __syncthreads();
            if (w == 0) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) gacc[r] += Yf[(k * 32 + sc_row(r, hb)) * PY + lq];
                }
            }
        }
        if (masks) {
            const int i = 32 * iq + lq;
            const float ci = cs[i];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float m[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int j = 32 * jq + 8 * q + 4 * hb + e;
                    m[e] = i <= j ? gacc[4 * q + e] * expf(cs[j] - ci) : 0.0f;
                }
                *(float4 *) (Mt + i * PM + 32 * jq + 8 * q + 4 * hb) = make_float4(m[0], m[1], m[2], m[3]);
            }
        }
        // 3a. C S_in^T over this wave's part of d_state
        sc_f16a ycs;
#pragma unroll
        for (int r = 0; r < 16; ++r) ycs[r] = 0.0f;
        ycs = sc_along<DS / KS>(Cs + (32 * rh + lq) * PB + 4 * hb + kh * (DS / KS), Ss + lq * PB + 4 * hb + kh * (DS / KS), ycs);
        __syncthreads();                                     // B: Mt is written, the old S is read

        // 3b. M X~ over this wave's part of the tokens, plus diag(e) times 3a
        sc_f16a v;
#pragma unroll
        for (int r = 0; r < 16; ++r) v[r] = 0.0f;
        if (!(Q == 64 && rh == 0 && kh == 1))                // (rows 0 .. 31 against tokens 32 .. 63: above the diagonal)
            v = sc_across<Q / 2 / KS, PM, PX, false>(Mt + 8 * hb * PM + 32 * rh + lq, Xs + 8 * hb * PX + lq, nullptr, kh * (Q / 2 / KS), v);
#pragma unroll
        for (int r = 0; r < 16; ++r) v[r] = fmaf(es[32 * rh + sc_row(r, hb)], ycs[r], v[r]);
        if (kh > 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) Yf[((kh - 1) * Q + 32 * rh + sc_row(r, hb)) * PY + lq] = v[r];
        }
        // 4. S = e_{Q-1} S + X~^T (w o B), then the slice to LDS for the next chunk's 3a
        const float el = es[Q - 1];
#pragma unroll
        for (int k = 0; k < TPW; ++k) {
            const int tl = w * TPW + k;
            if (tl < NT) {
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[k][r] *= el;
                acc[k] = sc_across<Q / 2, PX, PB, true>(Xs + 8 * hb * PX + lq, Bs + 8 * hb * PB + 32 * tl + lq, ws + 8 * hb, 0, acc[k]);
#pragma unroll
                for (int r = 0; r < 16; ++r) Ss[sc_row(r, hb) * PB + 32 * tl + lq] = acc[k][r];
            }
        }
        __syncthreads();                                     // C: the fold area and the new S are written; every read of the staged chunk is done

        if (kh == 0) {
#pragma unroll
            for (int k = 1; k < KS; ++k) {
#pragma unroll
                for (int r = 0; r < 16; ++r) v[r] += Yf[((k - 1) * Q + 32 * rh + sc_row(r, hb)) * PY + lq];
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int t = t0 + 32 * rh + sc_row(r, hb);
                if (t < a.n_t) yp[(size_t) t * y_ts + lq] = v[r];
            }
        }
    }

    // the final slice (barrier C of the last chunk, or the one after the state load, made it visible)
    float * so = (float *) (a.s_out + (size_t) seq * a.s_nb3) + row0 * DS;
#pragma unroll
    for (int u = 0; u < NS4; ++u) {
        const int e = tid + 256 * u, r = e / (DS / 4), c4 = e % (DS / 4);
        sc_st4(so + (size_t) r * DS + 4 * c4, *(const float4 *) (Ss + r * PB + 4 * c4), a.al);
    }
}

static long g_ssm_chunk_launches = 0;
long ssm_scan_chunk_launches() { return g_ssm_chunk_launches; }
static int g_ssm_chunk_mode = -1;
void ssm_chunk_set_mode(int m) { g_ssm_chunk_mode = m; }

int ssm_chunk_min_tokens() {
    static const int v = [] { const char * e = getenv("MI355X_SSM_CHUNK_MIN_TOKENS"); const long n = e ? atol(e) : 128; return (int) (n < 128 ? 128 : n > INT32_MAX ? INT32_MAX : n); }();
    return v;
}

bool ssm_chunk_takes(int64_t A_ne0, int64_t d_state, int64_t head_dim, int64_t n_t) {
    static const bool env_on = [] { const char * e = getenv("MI355X_SSM_CHUNK"); return !e || atoi(e) != 0; }();
    if (g_ssm_chunk_mode == 0 || (g_ssm_chunk_mode < 0 && !env_on)) return false;
    if (A_ne0 != 1 || head_dim % 32 != 0 || (d_state != 64 && d_state != 128 && d_state != 256)) return false;
    return g_ssm_chunk_mode == 2 ? n_t >= 1 : n_t >= ssm_chunk_min_tokens();      // 2: every token count (tools/ssm_bench.py locates the crossover with it)
}

// the caller (ssm_scan_f32) has passed ssm_scan_ok and ssm_chunk_takes
void ssm_scan_chunk_f32(const tdesc & s, const tdesc & x, const tdesc & dt, const tdesc & A, const tdesc & B, const tdesc & C, const int * ids, float * dst, hipStream_t st) {
    const int64_t d_state = s.ne[0], head_dim = x.ne[0], n_head = x.ne[1], n_t = x.ne[2], n_s = x.ne[3], n_group = B.ne[1];
    ssm_chunk_args a;
    a.s = (const char *) s.p; a.s_nb3 = s.nb[3];
    a.x = (const char *) x.p; a.x_nb2 = x.nb[2]; a.x_nb3 = x.nb[3];
    a.dt = (const char *) dt.p; a.dt_nb1 = dt.nb[1]; a.dt_nb2 = dt.nb[2];
    a.A = (const char *) A.p; a.A_nb1 = A.nb[1];
    a.B = (const char *) B.p; a.C = (const char *) C.p;
    a.b_nb1 = B.nb[1]; a.b_nb2 = B.nb[2]; a.b_nb3 = B.nb[3]; a.c_nb1 = C.nb[1]; a.c_nb2 = C.nb[2]; a.c_nb3 = C.nb[3];
    a.ids = ids;
    a.y = dst; a.s_out = (char *) dst + (size_t) (head_dim * n_head * n_t * n_s) * 4;
    a.head_dim = (int) head_dim; a.n_head = (int) n_head; a.heads_per_group = (int) (n_head / n_group); a.n_t = (int) n_t;
    a.al = (((uintptr_t) a.s | a.s_nb3 | (uintptr_t) a.s_out | (uintptr_t) a.B | (uintptr_t) a.C | a.b_nb1 | a.b_nb2 | a.b_nb3 | a.c_nb1 | a.c_nb2 | a.c_nb3 |
             (uintptr_t) a.x | a.x_nb2 | a.x_nb3) & 15) == 0;
    const dim3 grid((unsigned) (n_head * (head_dim / 32)), (unsigned) n_s);
    auto go = [&](auto ds) {
        constexpr int DS = decltype(ds)::value;
        constexpr size_t lds = (size_t) sc_cfg<DS>::floats * 4;
        static_assert(lds <= 152 * 1024, "the chunk's LDS");
        HIP_CHECK(hipFuncSetAttribute((const void *) k_ssm_scan_chunk<DS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds));
        k_ssm_scan_chunk<DS><<<grid, dim3(256), lds, st>>>(a);
    };
    switch (d_state) {
        case 64:  go(std::integral_constant<int, 64>());  break;
        case 128: go(std::integral_constant<int, 128>()); break;
        default:  go(std::integral_constant<int, 256>()); break;
    }
    ++g_ssm_chunk_launches;
}

} // namespace mi
