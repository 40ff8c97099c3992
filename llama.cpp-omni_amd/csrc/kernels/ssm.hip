// ssm.hip -- SSM_CONV and SSM_SCAN, the two ops every Mamba / Mamba-2 layer is built from (gfx950 / wave64).
//
// What is computed (reference: ggml_compute_forward_ssm_conv_f32 / ggml_compute_forward_ssm_scan_f32, ggml-cpu/ops.cpp:8505-8786):
//
//   SSM_CONV   x {d_conv - 1 + n_t, d_inner, n_s} (time contiguous), w {d_conv, d_inner} -> y {d_inner, n_t, n_s} (channels contiguous),
//              y[r, t, s] = sum_{i < d_conv} x[t + i, r, s] * w[i, r], the sum in index order.
//              Up to SSM_CONV_TOK_MAX tokens (decode): k_ssm_conv_tok, a lane owns a channel of one (token, sequence); at one token and d_conv == 4 its window is one
//              16-byte load, consecutive lanes read consecutive windows.  More tokens: k_ssm_conv_tile stages a (64 channels x 64 + d_conv - 1 times) tile through LDS --
//              lanes along TIME on the way in (a channel's times are contiguous in x), lanes along CHANNELS on the way out (contiguous in y); the LDS row stride is odd,
//              so the 32 channels of a ds_read_b32 group fall on 32 banks.
//
//   SSM_SCAN   per (sequence, head h, row i1 of head_dim) a state vector of d_state floats that starts from row ids[seq] of s; per token
//                  dt' = softplus(dt[h]);  state = state * exp(dt' * A) + B[g] * (x * dt');  y = sum(state * C[g]);  g = h / (n_head / n_group)
//              y {head_dim, n_head, n_t, n_s} at the start of dst, the final states behind it (byte nelements(x) * 4, sequence i3 at i3 * s->nb[3]).
//              k_ssm_scan: lanes lie along d_state -- a sub-group of d_state / 4 lanes owns a row, a float4 of it per lane, 64 / (d_state / 4) sub-groups per wave.  A
//              sub-group register-blocks R rows of ONE head (R = 4 from head_dim 4 on, else 1), so one load of B[g], C[g] and dt[h] serves them; a head's rows are cut
//              into ceil(head_dim / R) such groups and the ragged last one is predicated.  The state is read once, stays in registers across the token loop and is
//              written once; the next token's B, C, dt and x are in flight while the current one is computed.  y is reduced inside the sub-group with DPP moves
//              (quad_perm, row_half_mirror, row_mirror) and, beyond a 16-lane row, one or two cross-lane swaps.  The decay is a template form: one exp per head
//              and token (A {1, n_head}, Mamba-2) or one per state element and token (A {d_state, n_head}, Mamba-1; the four A values of a lane are loaded once).
//              ids is read on the device: an input tensor that changes between replays of a captured graph.
#include "../kernels.hpp"
#include <type_traits>

namespace mi {

// ------------------------------------------------------------------------------------------------ SSM_CONV
#define SSM_CONV_TOK_MAX 4          // tokens per sequence up to which a lane owns a channel of one token
#define SSM_CONV_TC 64              // tile: channels
#define SSM_CONV_TT 64              // tile: times

template <int DC>
__global__ void __launch_bounds__(256) k_ssm_conv_tok(const char * __restrict__ x, size_t x_nb1, size_t x_nb2, const char * __restrict__ w, size_t w_nb1,
                                                      char * __restrict__ y, size_t y_nb1, size_t y_nb2, int d_inner, int n_t, bool vec) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= d_inner) return;
    const int t = blockIdx.y, s = blockIdx.z;
    const float * xp = (const float *) (x + (size_t) s * x_nb2 + (size_t) r * x_nb1) + t;
    const float * wp = (const float *) (w + (size_t) r * w_nb1);
    float xv[DC], wv[DC];
    bool loaded = false;
    if constexpr (DC == 4) {
        if (vec) {                                           // (one token, 16-byte aligned windows and weight rows)
            const float4 a = *(const float4 *) xp, b = *(const float4 *) wp;
            xv[0] = a.x; xv[1] = a.y; xv[2] = a.z; xv[3] = a.w; wv[0] = b.x; wv[1] = b.y; wv[2] = b.z; wv[3] = b.w;
            loaded = true;
        }
    }
    if (!loaded) {
#pragma unroll
        for (int i = 0; i < DC; ++i) { xv[i] = xp[i]; wv[i] = wp[i]; }
    }
    float sum = 0.0f;
#pragma unroll
    for (int i = 0; i < DC; ++i) sum += xv[i] * wv[i];
    *((float *) (y + (size_t) s * y_nb2 + (size_t) t * y_nb1) + r) = sum;
}

template <int DC>
__global__ void __launch_bounds__(256) k_ssm_conv_tile(const char * __restrict__ x, size_t x_nb1, size_t x_nb2, const char * __restrict__ w, size_t w_nb1,
                                                       char * __restrict__ y, size_t y_nb1, size_t y_nb2, int d_inner, int n_t) {
    constexpr int TW = SSM_CONV_TT + DC - 1;                 // times a tile reads
    constexpr int LS = TW | 1;                               // LDS row stride in floats: odd
    __shared__ float tile[SSM_CONV_TC * LS];
    const int c0 = blockIdx.x * SSM_CONV_TC, t0 = blockIdx.y * SSM_CONV_TT, s = blockIdx.z;
    const int nc = min(SSM_CONV_TC, d_inner - c0), nw = min(TW, n_t + DC - 1 - t0);
    const char * xs = x + (size_t) s * x_nb2;
    for (int e = threadIdx.x; e < SSM_CONV_TC * TW; e += blockDim.x) {           // lanes along time
        const int c = e / TW, j = e - c * TW;
        if (c < nc && j < nw) tile[c * LS + j] = ((const float *) (xs + (size_t) (c0 + c) * x_nb1))[t0 + j];
    }
    __syncthreads();
    const int c = threadIdx.x & (SSM_CONV_TC - 1);           // lanes along channels
    if (c >= nc) return;
    float wv[DC];
    const float * wp = (const float *) (w + (size_t) (c0 + c) * w_nb1);
#pragma unroll
    for (int i = 0; i < DC; ++i) wv[i] = wp[i];
    const int nt = min(SSM_CONV_TT, n_t - t0);
    for (int t = threadIdx.x / SSM_CONV_TC; t < nt; t += 256 / SSM_CONV_TC) {
        float sum = 0.0f;
#pragma unroll
        for (int i = 0; i < DC; ++i) sum += tile[c * LS + t + i] * wv[i];
        *((float *) (y + (size_t) s * y_nb2 + (size_t) (t0 + t) * y_nb1) + c0 + c) = sum;
    }
}

static long g_ssm_conv_launches = 0, g_ssm_scan_launches = 0;
long ssm_conv_launches() { return g_ssm_conv_launches; }
long ssm_scan_launches() { return g_ssm_scan_launches; }

bool ssm_conv_ok(int64_t d_conv, int64_t d_inner, int64_t n_t, int64_t n_s) {      // the kernels' template range and the launch grid (y: tokens or time tiles, z: sequences)
    return d_conv >= 2 && d_conv <= 8 && d_inner >= 1 && d_inner <= INT32_MAX && n_t >= 1 && n_t <= INT32_MAX - 8 && n_s >= 1 && n_s <= 65535 &&
           (n_t <= SSM_CONV_TOK_MAX || (n_t + SSM_CONV_TT - 1) / SSM_CONV_TT <= 65535);
}

template <int DC>
static void ssm_conv_go(const tdesc & x, const tdesc & w, const tdesc & y, hipStream_t st) {
    const int d_inner = (int) w.ne[1], n_t = (int) y.ne[1], n_s = (int) y.ne[2];
    if (n_t <= SSM_CONV_TOK_MAX) {
        const bool vec = DC == 4 && n_t == 1 && (((uintptr_t) x.p | x.nb[1] | x.nb[2] | (uintptr_t) w.p | w.nb[1]) & 15) == 0;
        k_ssm_conv_tok<DC><<<dim3((d_inner + 255) / 256, n_t, n_s), dim3(256), 0, st>>>((const char *) x.p, x.nb[1], x.nb[2], (const char *) w.p, w.nb[1], (char *) y.p, y.nb[1], y.nb[2], d_inner, n_t, vec);
    } else
        k_ssm_conv_tile<DC><<<dim3((d_inner + SSM_CONV_TC - 1) / SSM_CONV_TC, (n_t + SSM_CONV_TT - 1) / SSM_CONV_TT, n_s), dim3(256), 0, st>>>(
            (const char *) x.p, x.nb[1], x.nb[2], (const char *) w.p, w.nb[1], (char *) y.p, y.nb[1], y.nb[2], d_inner, n_t);
}

void ssm_conv_f32(const tdesc & x, const tdesc & w, const tdesc & y, hipStream_t st) {
    const int64_t d_conv = w.ne[0];
    if (y.ne[0] == 0 || y.ne[1] == 0 || y.ne[2] == 0) return;
    if (!ssm_conv_ok(d_conv, w.ne[1], y.ne[1], y.ne[2]) || x.ne[0] != d_conv - 1 + y.ne[1] || x.ne[1] != w.ne[1] || y.ne[0] != w.ne[1]) {
        fprintf(stderr, "[mi355x] ssm_conv_f32: d_conv %lld, %lld channels, %lld tokens, %lld sequences have no kernel\n", (long long) d_conv, (long long) w.ne[1], (long long) y.ne[1], (long long) y.ne[2]); abort();
    }
    switch (d_conv) {
        case 2: ssm_conv_go<2>(x, w, y, st); break;
        case 3: ssm_conv_go<3>(x, w, y, st); break;
        case 4: ssm_conv_go<4>(x, w, y, st); break;
        case 5: ssm_conv_go<5>(x, w, y, st); break;
        case 6: ssm_conv_go<6>(x, w, y, st); break;
        case 7: ssm_conv_go<7>(x, w, y, st); break;
        default: ssm_conv_go<8>(x, w, y, st); break;
    }
    ++g_ssm_conv_launches;
}

// ------------------------------------------------------------------------------------------------ SSM_SCAN
#define SSM_SCAN_THREADS 128

template <int CTRL> static __device__ __forceinline__ float ssm_dpp(float v) { return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), CTRL, 0xf, 0xf, false)); }
// the sum over the L lanes of a sub-group (L a power of two, sub-groups aligned to L), in every one of its lanes
template <int L> static __device__ __forceinline__ float ssm_group_sum(float v) {
    if (L >= 2)  v += ssm_dpp<0xB1>(v);                      // quad_perm [1,0,3,2]
    if (L >= 4)  v += ssm_dpp<0x4E>(v);                      // quad_perm [2,3,0,1]
    if (L >= 8)  v += ssm_dpp<0x141>(v);                     // row_half_mirror
    if (L >= 16) v += ssm_dpp<0x140>(v);                     // row_mirror
    if (L >= 32) v += __shfl_xor(v, 16, 64);
    if (L >= 64) v += __shfl_xor(v, 32, 64);
    return v;
}
static __device__ __forceinline__ float ssm_softplus(float v) { return v > 20.0f ? v : logf(1.0f + expf(v)); }      // ggml_softplus (ggml-impl.h:105)
static __device__ __forceinline__ float4 ssm_ld4(const float * p, bool al) {
    if (al) return *(const float4 *) p;
    return make_float4(p[0], p[1], p[2], p[3]);
}
static __device__ __forceinline__ void ssm_st4(float * p, float4 v, bool al) {
    if (al) { *(float4 *) p = v; return; }
    p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
}

struct ssm_scan_args {
    const char * s; size_t s_nb3;                            // states {d_state, head_dim, n_head, n_rows}, contiguous
    const char * x; size_t x_nb2, x_nb3;                     // {head_dim, n_head, n_t, n_s}, dense up to a head row
    const char * dt; size_t dt_nb1, dt_nb2;                  // {n_head, n_t, n_s}
    const char * A; size_t A_nb1;                            // {1 | d_state, n_head}
    const char * B; const char * C; size_t b_nb1, b_nb2, b_nb3, c_nb1, c_nb2, c_nb3;      // {d_state, n_group, n_t, n_s}
    const int * ids;                                         // {n_s}
    float * y; char * s_out;                                 // y dense {head_dim, n_head, n_t, n_s}; final states, sequence i3 at i3 * s_nb3
    int head_dim, n_head, heads_per_group, n_t, groups_per_head;      // groups_per_head = ceil(head_dim / R)
    long long n_groups;                                      // n_head * groups_per_head
    bool al;                                                 // every 16-byte access is aligned
};

// DS = d_state, AV: one decay per state element (A {d_state, n_head}), R rows per sub-group
template <int DS, bool AV, int R>
__global__ void __launch_bounds__(SSM_SCAN_THREADS) k_ssm_scan(const ssm_scan_args a) {
    constexpr int L = DS / 4, SG = 64 / L;                   // lanes per row, sub-groups per wave
    const int lane = threadIdx.x & 63, sub = lane / L, l4 = (lane % L) * 4;
    const long long q = ((long long) blockIdx.x * (SSM_SCAN_THREADS / 64) + (threadIdx.x >> 6)) * SG + sub;      // this sub-group's row group
    const int seq = blockIdx.y;
    // a sub-group past the last row group runs on row group 0 with nothing live (its lanes still take part in the DPP moves of their 16-lane row)
    const bool live = q < a.n_groups;
    const long long qq = live ? q : 0;
    const int h = (int) (qq / a.groups_per_head), i0 = (int) (qq - (long long) h * a.groups_per_head) * R, g = h / a.heads_per_group;
    bool on[R];
#pragma unroll
    for (int k = 0; k < R; ++k) on[k] = live && i0 + k < a.head_dim;
    const size_t row0 = (size_t) h * a.head_dim + i0;        // flat row of (h, i0): y / x element, state row
    float4 st[R];
    {
        const float * s0 = (const float *) (a.s + (size_t) a.ids[seq] * a.s_nb3) + row0 * DS + l4;
#pragma unroll
        for (int k = 0; k < R; ++k) st[k] = on[k] ? ssm_ld4(s0 + (size_t) k * DS, a.al) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    float4 Av = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (AV) Av = ssm_ld4((const float *) (a.A + (size_t) h * a.A_nb1) + l4, a.al);
    else    Av.x = *(const float *) (a.A + (size_t) h * a.A_nb1);
    const char * xp = a.x + (size_t) seq * a.x_nb3 + row0 * 4;
    const char * dp = a.dt + (size_t) seq * a.dt_nb2 + (size_t) h * 4;
    const char * bp = a.B + (size_t) seq * a.b_nb3 + (size_t) g * a.b_nb1 + (size_t) l4 * 4;
    const char * cp = a.C + (size_t) seq * a.c_nb3 + (size_t) g * a.c_nb1 + (size_t) l4 * 4;
    float * yp = a.y + ((size_t) seq * a.n_t * a.n_head * a.head_dim + row0);
    const size_t y_ts = (size_t) a.n_head * a.head_dim;
    // token t's operands are loaded while token t - 1 is computed
    float4 nB = make_float4(0.0f, 0.0f, 0.0f, 0.0f), nC = nB; float ndt = 0.0f, nx[R];
    auto fetch = [&](int t) {
        nB = ssm_ld4((const float *) (bp + (size_t) t * a.b_nb2), a.al);
        nC = ssm_ld4((const float *) (cp + (size_t) t * a.c_nb2), a.al);
        ndt = *(const float *) (dp + (size_t) t * a.dt_nb1);
#pragma unroll
        for (int k = 0; k < R; ++k) nx[k] = on[k] ? ((const float *) (xp + (size_t) t * a.x_nb2))[k] : 0.0f;
    };
    if (a.n_t > 0) fetch(0);
    for (int t = 0; t < a.n_t; ++t) {
        const float4 Bv = nB, Cv = nC; const float dtv = ndt;
        float xv[R];
#pragma unroll
        for (int k = 0; k < R; ++k) xv[k] = nx[k];
        if (t + 1 < a.n_t) fetch(t + 1);
        const float dsp = ssm_softplus(dtv);
        float4 dA;
        if (AV) dA = make_float4(expf(dsp * Av.x), expf(dsp * Av.y), expf(dsp * Av.z), expf(dsp * Av.w));
        else  { const float e = expf(dsp * Av.x); dA = make_float4(e, e, e, e); }
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const float x_dt = xv[k] * dsp;
            st[k].x = st[k].x * dA.x + Bv.x * x_dt; st[k].y = st[k].y * dA.y + Bv.y * x_dt;
            st[k].z = st[k].z * dA.z + Bv.z * x_dt; st[k].w = st[k].w * dA.w + Bv.w * x_dt;
            float sum = st[k].x * Cv.x;
            sum += st[k].y * Cv.y; sum += st[k].z * Cv.z; sum += st[k].w * Cv.w;
            sum = ssm_group_sum<L>(sum);
            if (on[k] && l4 == 0) yp[(size_t) t * y_ts + k] = sum;
        }
    }
    float * so = (float *) (a.s_out + (size_t) seq * a.s_nb3) + row0 * DS + l4;
#pragma unroll
    for (int k = 0; k < R; ++k) if (on[k]) ssm_st4(so + (size_t) k * DS, st[k], a.al);
}

bool ssm_scan_ok(int64_t d_state, int64_t head_dim, int64_t n_head, int64_t n_group, int64_t n_t, int64_t n_s) {
    if (d_state != 16 && d_state != 32 && d_state != 64 && d_state != 128 && d_state != 256) return false;
    if (head_dim < 1 || n_head < 1 || n_group < 1 || n_head % n_group != 0 || n_t < 0 || n_t > INT32_MAX || n_s < 1) return false;
    if (head_dim > INT32_MAX || n_head > INT32_MAX || n_s > 65535) return false;                                // grid y
    const int64_t sg = 64 / (d_state / 4), wpb = SSM_SCAN_THREADS / 64;
    const int64_t groups = n_head * (head_dim >= 4 ? (head_dim + 3) / 4 : head_dim);                            // row groups of R = 4 / 1 rows
    if (head_dim * n_head > INT32_MAX) return false;
    return (groups + sg * wpb - 1) / (sg * wpb) <= INT32_MAX;                                                   // grid x
}

template <int DS, bool AV>
static void ssm_scan_go(ssm_scan_args & a, int n_s, hipStream_t st) {
    const int R = a.head_dim >= 4 ? 4 : 1;
    a.groups_per_head = (a.head_dim + R - 1) / R;
    a.n_groups = (long long) a.n_head * a.groups_per_head;
    const long long per_block = (64 / (DS / 4)) * (SSM_SCAN_THREADS / 64);
    const dim3 grid((unsigned) ((a.n_groups + per_block - 1) / per_block), (unsigned) n_s);
    if (R == 4) k_ssm_scan<DS, AV, 4><<<grid, dim3(SSM_SCAN_THREADS), 0, st>>>(a);
    else        k_ssm_scan<DS, AV, 1><<<grid, dim3(SSM_SCAN_THREADS), 0, st>>>(a);
}

void ssm_scan_f32(const tdesc & s, const tdesc & x, const tdesc & dt, const tdesc & A, const tdesc & B, const tdesc & C, const int * ids, float * dst, hipStream_t st) {
    const int64_t d_state = s.ne[0], head_dim = x.ne[0], n_head = x.ne[1], n_t = x.ne[2], n_s = x.ne[3], n_group = B.ne[1];
    if (n_s == 0 || head_dim == 0 || n_head == 0) return;
    const bool av = A.ne[0] != 1;
    if (!ssm_scan_ok(d_state, head_dim, n_head, n_group, n_t, n_s) || (av && A.ne[0] != d_state)) {
        fprintf(stderr, "[mi355x] ssm_scan_f32: d_state %lld, head_dim %lld, %lld heads, %lld groups, A->ne[0] %lld have no kernel\n", (long long) d_state, (long long) head_dim, (long long) n_head, (long long) n_group, (long long) A.ne[0]); abort();
    }
    ssm_scan_args a;
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
             (av ? ((uintptr_t) a.A | a.A_nb1) : 0)) & 15) == 0;
    auto go = [&](auto ds) {
        constexpr int DS = decltype(ds)::value;
        if (av) ssm_scan_go<DS, true>(a, (int) n_s, st); else ssm_scan_go<DS, false>(a, (int) n_s, st);
    };
    switch (d_state) {
        case 16:  go(std::integral_constant<int, 16>());  break;
        case 32:  go(std::integral_constant<int, 32>());  break;
        case 64:  go(std::integral_constant<int, 64>());  break;
        case 128: go(std::integral_constant<int, 128>()); break;
        default:  go(std::integral_constant<int, 256>()); break;
    }
    ++g_ssm_scan_launches;
}

} // namespace mi
