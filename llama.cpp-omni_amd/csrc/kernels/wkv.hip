// wkv.hip -- RWKV_WKV6, GATED_LINEAR_ATTN, RWKV_WKV7 and L2_NORM, the four ops the recurrent layers of rwkv6 / rwkv6qwen2 / rwkv7 / arwkv7 add to a graph (gfx950 / wave64), f32.
//
// What is computed (reference: ggml_compute_forward_rwkv_wkv6_f32 ggml-cpu/ops.cpp:9177, ggml_compute_forward_gla_f32 :9393, ggml_compute_forward_rwkv_wkv7_f32 :9598,
// ggml_compute_forward_l2_norm_f32 :3858; the constructors ggml.c:3018 and :5369-5499).  S = head size, H = heads, C = S * H, T = tokens of all sequences, n_seqs sequences of
// T / n_seqs consecutive tokens each.  dst {C, T + S * n_seqs}: the C * T outputs, then n_seqs new states of S * S * H floats; sequence q's previous state lies at the same
// offset q * S * S * H of the (contiguous, any shape) state source.  A sequence's first token reads the source, later ones the state being built.
//
//   RWKV_WKV6          s[h][i][j], i the k index, j the v index:   out[t,h,j] = sum_i r[i] * (tf[h,i] * k[i] * v[j] + s[i][j]);   s[i][j] = s[i][j] * td[t,h,i] + k[i] * v[j]
//   GATED_LINEAR_ATTN  the same layout:                            tmp = s[i][j] * g[i] + k[i] * v[j];   out[j] = sum_i (q[i] * scale) * tmp;   s[i][j] = tmp
//   RWKV_WKV7          s[h][i][j], i the V index, j the k index:   sa_i = sum_j a[j] * s[i][j];   s[i][j] = s[i][j] * w[j] + v[i] * k[j] + sa_i * b[j];   out[i] = sum_j s[i][j] * r[j]
//   L2_NORM            per row y = x * (1 / max(sqrt(sum x^2), eps)), the sum in double as the reference has it; rows through nb1..nb3
//
// The recurrences split without any reduction across workgroups: the columns j of WKV6 / GLA are independent, and so are the rows i of WKV7 (sa_i needs row i only).
//
//   k_wkv6<S, CW, GLA>   S = 64 / 128.  One wave owns CW = 16 (or 8) columns of one head of one sequence: CW / 4 lanes across the columns, a float4 each, 64 / (CW / 4) lane
//                        groups down the rows, S / groups consecutive rows per lane.  A state load covers 64-byte (32-byte) row segments of 16 (32) rows; the slice stays in
//                        registers over the sequence's tokens (8 .. 32 floats per lane), is read once and written once.  out's sum over i: the lane's rows in order, then
//                        xor-shuffles across the lane groups.  The next token's k, v, r, td are in flight while the current one is computed.  CW = 8 when 16 would leave
//                        fewer than 512 waves (7B decode, H = 64: 512 waves; H = 32: 256).
//   k_wkv7<S, RW>        one wave owns RW = 8 rows of one head: S / 4 lanes along a row, a float4 each -- every state access is a whole 256 / 512-byte row, no transposing
//                        stage -- 64 / (S / 4) rows per pass, 2 / 4 passes.  sa_i and out[i] are reduced over the row's lanes with xor-shuffles (16 / 32 lanes).
//                        H = 64, S = 64: 512 waves per sequence.
//   k_wkv6_any / k_wkv7_any   every other S from 1 to 128 (the loader probes with S = 123), or operands that are not 16-byte aligned: one workgroup per (head, sequence),
//                        thread j owns column j (WKV6 / GLA: coalesced) or row i (WKV7) and keeps the state in dst between tokens -- the same thread writes and re-reads
//                        an element.  Correct, not fast.
#include "../kernels.hpp"
#include <algorithm>

namespace mi {

#define WKV_ANY_THREADS 128          // S <= 128

static long g_wkv6_launches = 0, g_gla_launches = 0, g_wkv7_launches = 0, g_l2_norm_launches = 0;
long wkv6_launches() { return g_wkv6_launches; }
long gla_launches() { return g_gla_launches; }
long wkv7_launches() { return g_wkv7_launches; }
long l2_norm_launches() { return g_l2_norm_launches; }

struct wkv_args {
    const float * p[6];              // WKV6: k v r tf td -;  GLA: k v q - g -;  WKV7: r w k v a b
    const float * s_in;              // previous states, sequence q at q * S * S * H
    float * out, * s_out;            // {C, T} outputs; new states
    float scale;                     // GLA
    int H, n_t;                      // heads; tokens per sequence
};

// ------------------------------------------------------------------------------------------------ RWKV_WKV6 / GATED_LINEAR_ATTN
template <int S, int CW, bool GLA>
__global__ void __launch_bounds__(64) k_wkv6(const wkv_args a) {
    constexpr int LW = CW / 4, RG = 64 / LW, NR = S / RG;            // lanes across the columns, lane groups down the rows, rows per lane
    const int lane = threadIdx.x, c = lane % LW, i0 = (lane / LW) * NR;
    const int j0 = blockIdx.x * CW + c * 4, h = blockIdx.y, seq = blockIdx.z;
    const size_t C = (size_t) a.H * S, so = ((size_t) seq * a.H + h) * S * S;
    const float * kp = a.p[0], * vp = a.p[1], * rp = a.p[2], * dp = a.p[4];
    float4 st[NR];
#pragma unroll
    for (int m = 0; m < NR; ++m) st[m] = *(const float4 *) (a.s_in + so + (size_t) (i0 + m) * S + j0);
    float tf[NR];
#pragma unroll
    for (int m = 0; m < NR; ++m) tf[m] = GLA ? 0.0f : a.p[3][(size_t) h * S + i0 + m];
    size_t off = (size_t) seq * a.n_t * C + (size_t) h * S;          // token 0 of the sequence, this head
    float nk[NR], nr[NR], nd[NR]; float4 nv;
    auto fetch = [&](size_t o) {
#pragma unroll
        for (int m = 0; m < NR; ++m) { nk[m] = kp[o + i0 + m]; nr[m] = rp[o + i0 + m]; nd[m] = dp[o + i0 + m]; }
        nv = *(const float4 *) (vp + o + j0);
    };
    if (a.n_t > 0) fetch(off);
    for (int t = 0; t < a.n_t; ++t, off += C) {
        float kk[NR], rr[NR], dd[NR]; const float4 v = nv;
#pragma unroll
        for (int m = 0; m < NR; ++m) { kk[m] = nk[m]; rr[m] = nr[m]; dd[m] = nd[m]; }
        if (t + 1 < a.n_t) fetch(off + C);
        float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
        for (int m = 0; m < NR; ++m) {
            const float4 kv = make_float4(v.x * kk[m], v.y * kk[m], v.z * kk[m], v.w * kk[m]);
            if (GLA) {
                const float q = rr[m] * a.scale;
                st[m].x = st[m].x * dd[m] + kv.x; st[m].y = st[m].y * dd[m] + kv.y; st[m].z = st[m].z * dd[m] + kv.z; st[m].w = st[m].w * dd[m] + kv.w;
                o.x += st[m].x * q; o.y += st[m].y * q; o.z += st[m].z * q; o.w += st[m].w * q;
            } else {
                o.x += (kv.x * tf[m] + st[m].x) * rr[m]; o.y += (kv.y * tf[m] + st[m].y) * rr[m];
                o.z += (kv.z * tf[m] + st[m].z) * rr[m]; o.w += (kv.w * tf[m] + st[m].w) * rr[m];
                st[m].x = st[m].x * dd[m] + kv.x; st[m].y = st[m].y * dd[m] + kv.y; st[m].z = st[m].z * dd[m] + kv.z; st[m].w = st[m].w * dd[m] + kv.w;
            }
        }
#pragma unroll
        for (int d = LW; d < 64; d <<= 1) {                          // across the lane groups
            o.x += __shfl_xor(o.x, d, 64); o.y += __shfl_xor(o.y, d, 64); o.z += __shfl_xor(o.z, d, 64); o.w += __shfl_xor(o.w, d, 64);
        }
        if (lane < LW) *(float4 *) (a.out + off + j0) = o;
    }
#pragma unroll
    for (int m = 0; m < NR; ++m) *(float4 *) (a.s_out + so + (size_t) (i0 + m) * S + j0) = st[m];
}

// any S <= WKV_ANY_THREADS: thread j owns column j; the state lives in dst between tokens
template <bool GLA>
__global__ void __launch_bounds__(WKV_ANY_THREADS) k_wkv6_any(const wkv_args a, const int S) {
    const int j = threadIdx.x, h = blockIdx.x, seq = blockIdx.y;
    if (j >= S) return;
    const size_t C = (size_t) a.H * S, so = ((size_t) seq * a.H + h) * S * S;
    const float * kp = a.p[0], * vp = a.p[1], * rp = a.p[2], * dp = a.p[4];
    const float * sp = a.s_in + so;                                  // the first token reads the source
    float * sc = a.s_out + so;
    size_t off = (size_t) seq * a.n_t * C + (size_t) h * S;
    for (int t = 0; t < a.n_t; ++t, off += C) {
        const float v = vp[off + j];
        float o = 0.0f;
        for (int i = 0; i < S; ++i) {
            const float k = kp[off + i], r = rp[off + i], d = dp[off + i], kv = v * k, p = sp[(size_t) i * S + j];
            if (GLA) {
                const float tmp = p * d + kv;
                o += tmp * (r * a.scale);
                sc[(size_t) i * S + j] = tmp;
            } else {
                o += (kv * a.p[3][(size_t) h * S + i] + p) * r;
                sc[(size_t) i * S + j] = p * d + kv;
            }
        }
        a.out[off + j] = o;
        sp = sc;
    }
}

// ------------------------------------------------------------------------------------------------ RWKV_WKV7
template <int S, int RW>
__global__ void __launch_bounds__(64) k_wkv7(const wkv_args a) {
    constexpr int L = S / 4, RP = 64 / L, NP = RW / RP;              // lanes per row, rows per pass, passes
    const int lane = threadIdx.x, j0 = (lane % L) * 4, rp = lane / L;
    const int i0 = blockIdx.x * RW + rp, h = blockIdx.y, seq = blockIdx.z;      // the lane's rows: i0 + p * RP
    const size_t C = (size_t) a.H * S, so = ((size_t) seq * a.H + h) * S * S;
    float4 st[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) st[p] = *(const float4 *) (a.s_in + so + (size_t) (i0 + p * RP) * S + j0);
    size_t off = (size_t) seq * a.n_t * C + (size_t) h * S;
    float4 nr, nw, nk, na, nb; float nv[NP];
    auto fetch = [&](size_t o) {
        nr = *(const float4 *) (a.p[0] + o + j0); nw = *(const float4 *) (a.p[1] + o + j0); nk = *(const float4 *) (a.p[2] + o + j0);
        na = *(const float4 *) (a.p[4] + o + j0); nb = *(const float4 *) (a.p[5] + o + j0);
#pragma unroll
        for (int p = 0; p < NP; ++p) nv[p] = a.p[3][o + i0 + p * RP];
    };
    if (a.n_t > 0) fetch(off);
    for (int t = 0; t < a.n_t; ++t, off += C) {
        const float4 r = nr, w = nw, k = nk, av = na, b = nb; float v[NP];
#pragma unroll
        for (int p = 0; p < NP; ++p) v[p] = nv[p];
        if (t + 1 < a.n_t) fetch(off + C);
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            float sa = av.x * st[p].x;
            sa += av.y * st[p].y; sa += av.z * st[p].z; sa += av.w * st[p].w;
#pragma unroll
            for (int d = 1; d < L; d <<= 1) sa += __shfl_xor(sa, d, 64);
            st[p].x = st[p].x * w.x + v[p] * k.x + sa * b.x; st[p].y = st[p].y * w.y + v[p] * k.y + sa * b.y;
            st[p].z = st[p].z * w.z + v[p] * k.z + sa * b.z; st[p].w = st[p].w * w.w + v[p] * k.w + sa * b.w;
            float o = st[p].x * r.x;
            o += st[p].y * r.y; o += st[p].z * r.z; o += st[p].w * r.w;
#pragma unroll
            for (int d = 1; d < L; d <<= 1) o += __shfl_xor(o, d, 64);
            if (j0 == 0) a.out[off + i0 + p * RP] = o;
        }
    }
#pragma unroll
    for (int p = 0; p < NP; ++p) *(float4 *) (a.s_out + so + (size_t) (i0 + p * RP) * S + j0) = st[p];
}

// any S <= WKV_ANY_THREADS: thread i owns row i
__global__ void __launch_bounds__(WKV_ANY_THREADS) k_wkv7_any(const wkv_args a, const int S) {
    const int i = threadIdx.x, h = blockIdx.x, seq = blockIdx.y;
    if (i >= S) return;
    const size_t C = (size_t) a.H * S, so = ((size_t) seq * a.H + h) * S * S + (size_t) i * S;
    const float * sp = a.s_in + so;
    float * sc = a.s_out + so;
    size_t off = (size_t) seq * a.n_t * C + (size_t) h * S;
    for (int t = 0; t < a.n_t; ++t, off += C) {
        const float v = a.p[3][off + i];
        float sa = 0.0f, o = 0.0f;
        for (int j = 0; j < S; ++j) sa += a.p[4][off + j] * sp[j];
        for (int j = 0; j < S; ++j) {
            const float n = sp[j] * a.p[1][off + j] + v * a.p[2][off + j] + sa * a.p[5][off + j];
            sc[j] = n;
            o += n * a.p[0][off + j];
        }
        a.out[off + i] = o;
        sp = sc;
    }
}

bool wkv_ok(int64_t S, int64_t H, int64_t T, int64_t n_seqs) {       // head sizes with a kernel and the launch grid (y: heads or sequences, z: sequences)
    return S >= 1 && S <= WKV_ANY_THREADS && H >= 1 && H <= 65535 && n_seqs >= 1 && n_seqs <= 65535 && T >= 1 && T <= INT32_MAX && T % n_seqs == 0;
}

static bool wkv_aligned(const wkv_args & a) {
    uintptr_t m = (uintptr_t) a.s_in | (uintptr_t) a.out | (uintptr_t) a.s_out;
    for (int i = 0; i < 6; ++i) m |= (uintptr_t) a.p[i];
    return (m & 15) == 0;
}

static void wkv_check(const char * what, int64_t S, int64_t H, int64_t T, int64_t n_seqs) {
    if (wkv_ok(S, H, T, n_seqs)) return;
    fprintf(stderr, "[mi355x] %s: head size %lld, %lld heads, %lld tokens, %lld sequences have no kernel\n", what, (long long) S, (long long) H, (long long) T, (long long) n_seqs); abort();
}

template <bool GLA>
static void wkv6_go(wkv_args & a, int64_t S, int64_t H, int64_t T, int64_t n_seqs, hipStream_t st) {
    if ((S == 64 || S == 128) && wkv_aligned(a)) {
        const bool narrow = H * n_seqs * (S / 16) < 512;             // 8 columns per wave while 16 leave fewer than 512 waves
        const dim3 grid((unsigned) (S / (narrow ? 8 : 16)), (unsigned) H, (unsigned) n_seqs);
        if (S == 64) { if (narrow) k_wkv6<64, 8, GLA><<<grid, dim3(64), 0, st>>>(a);  else k_wkv6<64, 16, GLA><<<grid, dim3(64), 0, st>>>(a); }
        else         { if (narrow) k_wkv6<128, 8, GLA><<<grid, dim3(64), 0, st>>>(a); else k_wkv6<128, 16, GLA><<<grid, dim3(64), 0, st>>>(a); }
    } else
        k_wkv6_any<GLA><<<dim3((unsigned) H, (unsigned) n_seqs), dim3(WKV_ANY_THREADS), 0, st>>>(a, (int) S);
}

void wkv6_f32(const float * k, const float * v, const float * r, const float * tf, const float * td, const float * state, float * dst, int64_t S, int64_t H, int64_t T, int64_t n_seqs, hipStream_t st) {
    wkv_check("wkv6_f32", S, H, T, n_seqs);
    wkv_args a = { { k, v, r, tf, td, k }, state, dst, dst + (size_t) S * H * T, 0.0f, (int) H, (int) (T / n_seqs) };
    wkv6_go<false>(a, S, H, T, n_seqs, st);
    ++g_wkv6_launches;
}

void gla_f32(const float * k, const float * v, const float * q, const float * g, const float * state, float scale, float * dst, int64_t S, int64_t H, int64_t T, int64_t n_seqs, hipStream_t st) {
    wkv_check("gla_f32", S, H, T, n_seqs);
    wkv_args a = { { k, v, q, k, g, k }, state, dst, dst + (size_t) S * H * T, scale, (int) H, (int) (T / n_seqs) };
    wkv6_go<true>(a, S, H, T, n_seqs, st);
    ++g_gla_launches;
}

void wkv7_f32(const float * r, const float * w, const float * k, const float * v, const float * av, const float * b, const float * state, float * dst, int64_t S, int64_t H, int64_t T, int64_t n_seqs, hipStream_t st) {
    wkv_check("wkv7_f32", S, H, T, n_seqs);
    wkv_args a = { { r, w, k, v, av, b }, state, dst, dst + (size_t) S * H * T, 0.0f, (int) H, (int) (T / n_seqs) };
    if ((S == 64 || S == 128) && wkv_aligned(a)) {
        const dim3 grid((unsigned) (S / 8), (unsigned) H, (unsigned) n_seqs);
        if (S == 64) k_wkv7<64, 8><<<grid, dim3(64), 0, st>>>(a); else k_wkv7<128, 8><<<grid, dim3(64), 0, st>>>(a);
    } else
        k_wkv7_any<<<dim3((unsigned) H, (unsigned) n_seqs), dim3(WKV_ANY_THREADS), 0, st>>>(a, (int) S);
    ++g_wkv7_launches;
}

// ------------------------------------------------------------------------------------------------ L2_NORM
#define L2_NORM_THREADS 256

// TEAM threads per row (a wave, or the workgroup for long rows); rows grid-strided
template <int TEAM>
__global__ void __launch_bounds__(L2_NORM_THREADS) k_l2_norm(const char * x, size_t x_nb1, size_t x_nb2, size_t x_nb3, char * y, size_t y_nb1, size_t y_nb2, size_t y_nb3,
                                                             int ne0, int64_t ne1, int64_t ne2, int64_t n_rows, float eps) {
    constexpr int TPB = L2_NORM_THREADS / TEAM;                      // rows per workgroup and step
    __shared__ double part[L2_NORM_THREADS / 64];
    const int l = threadIdx.x % TEAM;
    for (int64_t row0 = (int64_t) blockIdx.x * TPB; row0 < n_rows; row0 += (int64_t) gridDim.x * TPB) {      // (trip count uniform over the workgroup: the barriers below)
        const int64_t row = row0 + threadIdx.x / TEAM;
        const bool on = row < n_rows;
        const int64_t rr = on ? row : 0, i1 = rr % ne1, i2 = (rr / ne1) % ne2, i3 = rr / (ne1 * ne2);
        const float * xp = (const float *) (x + (size_t) i1 * x_nb1 + (size_t) i2 * x_nb2 + (size_t) i3 * x_nb3);
        float * yp = (float *) (y + (size_t) i1 * y_nb1 + (size_t) i2 * y_nb2 + (size_t) i3 * y_nb3);
        double sum = 0.0;
        for (int i = l; i < ne0; i += TEAM) { const float v = xp[i]; sum += (double) (v * v); }
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) sum += __shfl_xor(sum, d, 64);
        if (TEAM > 64) {
            if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = sum;
            __syncthreads();
            sum = 0.0;
#pragma unroll
            for (int k = 0; k < L2_NORM_THREADS / 64; ++k) sum += part[k];
            __syncthreads();
        }
        const float scale = 1.0f / fmaxf(sqrtf((float) sum), eps);
        if (on) for (int i = l; i < ne0; i += TEAM) yp[i] = xp[i] * scale;
    }
}

bool l2_norm_ok(int64_t ne0, int64_t n_rows) { return ne0 >= 1 && ne0 <= INT32_MAX && n_rows >= 1; }

void l2_norm_f32(const tdesc & x, const tdesc & y, float eps, hipStream_t st) {
    const int64_t n_rows = x.ne[1] * x.ne[2] * x.ne[3];
    if (x.ne[0] == 0 || n_rows == 0) return;
    if (!l2_norm_ok(x.ne[0], n_rows)) { fprintf(stderr, "[mi355x] l2_norm_f32: rows of %lld elements have no kernel\n", (long long) x.ne[0]); abort(); }
    if (x.ne[0] <= 1024) {
        const int64_t nb = (n_rows + 3) / 4;
        k_l2_norm<64><<<dim3((unsigned) std::min<int64_t>(nb, 65535)), dim3(L2_NORM_THREADS), 0, st>>>((const char *) x.p, x.nb[1], x.nb[2], x.nb[3], (char *) y.p, y.nb[1], y.nb[2], y.nb[3],
                                                                                                      (int) x.ne[0], x.ne[1], x.ne[2], n_rows, eps);
    } else
        k_l2_norm<L2_NORM_THREADS><<<dim3((unsigned) std::min<int64_t>(n_rows, 65535)), dim3(L2_NORM_THREADS), 0, st>>>((const char *) x.p, x.nb[1], x.nb[2], x.nb[3], (char *) y.p, y.nb[1], y.nb[2], y.nb[3],
                                                                                                                        (int) x.ne[0], x.ne[1], x.ne[2], n_rows, eps);
    ++g_l2_norm_launches;
}

} // namespace mi
