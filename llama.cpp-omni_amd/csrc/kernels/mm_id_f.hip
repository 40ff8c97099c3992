// mm_id_f.hip -- MUL_MAT_ID on UNQUANTISED experts (gfx950, wave64): BF16 (what mixture-of-experts checkpoints are published in) and F32.
//     dst[:, i, t] = as[:, :, ids[i, t]] . b[:, i % b_ne1, t]          (ggml_compute_forward_mul_mat_id, ggml-cpu/ggml-cpu.c:1484 ff.)
// vec_dot_type BF16: b's columns are first rounded to bf16 (ggml_compute_fp32_to_bf16: round to nearest even, a NaN kept quiet), every product of two bf16 values is
// exact in f32, the sum is f32.  vec_dot_type F32: no rounding at all.  Only the order of the f32 additions differs from the reference.
//
//   k_f32_to_bf16_rows   the ACT_BF16 image: one bf16 row of 2 K bytes per column of b, padded with ZEROS to 16 bytes (the mat-vec's ragged last chunk reads the pad).
//   k_mmv_id_f<Dec, VEC> the per-pair mat-vec: decode, every ubatch under the grouped threshold, F32 experts at every token count.  Grid (row workgroups, slot i,
//                        token t) as k_mmv_id (mmvk.hip); the id is read on the device and clamped into [0, n_expert) before it becomes an address.  The workgroup
//                        stages its ONE column into LDS once (the bf16 image / the f32 column where it lies), then every wave takes groups of ROWS = 4 rows: the lanes
//                        walk K in 16-byte chunks (8 bf16 / 4 f32; chunk lane + 64 j at step j), the four rows' chunks of the NEXT step are requested before the current
//                        four are consumed.  A lane adds its chunks in step order, the elements of a chunk in order, then the wave folds over DPP (wave_sum_f32): the
//                        f32 summation order of a row is a function of K alone.  VEC: one 16-byte load per chunk -- base, row stride and expert stride 16-byte aligned
//                        and K a whole number of chunks.  Otherwise the chunk is gathered element by element (index clamped, a value past K zeroed): any K >= 1, any
//                        element-aligned stride.
//   k_mm_id_16<Dec, KS>  BF16 experts from mm_id_bf16_min_tokens() tokens on: the pairs grouped by expert on the device (mmq_id.hip k_moe_group: pair list, tile table,
//                        tile count -- unchanged), one workgroup per (expert, 32-row tile, <= 32-column slice), grid y = the host's bound on the tile count (a workgroup
//                        past the device-side count returns at once: nothing is data-dependent on the host).  v_mfma_f32_32x32x16_bf16 with the operand roles of
//                        k_mmq_id: the lane's COLUMN (lane & 31 of the slice, K half lane >> 5: 8 consecutive bf16 of its image, found through the pair list) against
//                        the lane's weight ROW (row lane & 31 of the tile, the same K half: 8 consecutive bf16 straight from global memory -- a weight is used once per
//                        tile, no LDS sits under it).  Register 4 g + i of the accumulator = column 8 g + 4 hb + i of the lane's row, as mmq_id_finish stores it.
//                        A lane past the slice's columns reads the slice's first column; its results are never stored.  A fetch step is STEP = 4 MFMA steps (64 weights
//                        of K: with its K-half partner a lane pair reads 128 consecutive bytes of the row); two register sets, the next fetch step requested before
//                        the current one's MFMAs issue.  The KS waves take the fetch steps wave, wave + KS, ... and fold through LDS in wave order (mmq_fold).
//                        KS comes from K, the row tiles and the grid bound only -- never from the ids -- so a column's result is bit-reproducible and independent of
//                        the pairs that share its tile.
//                        ONE instance over the column groups (NT = 4): a 32x32x16 MFMA multiplies all 32 columns whatever the slice holds, so a narrower body saves no
//                        MFMA; it would narrow the fold only, and the store is guarded per column already.
// Both matrix kernels are templated on an element decoder; bf16_dec (and, for the mat-vec, f32_dec) are the only instances.
#include "mmq_dev.hpp"

namespace mi {

extern __shared__ __attribute__((aligned(16))) char mf_lds[];

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float  f32x16 __attribute__((ext_vector_type(16)));

// ggml_compute_fp32_to_bf16 (ggml-impl.h), as gemm_any.hip / fattn_any.hip restate it
static __device__ __forceinline__ uint16_t f32_to_bf16(float f) {
    const uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t) ((u >> 16) | 64);          // NaN: quiet, payload kept
    return (uint16_t) ((u + (0x7fffu + ((u >> 16) & 1u))) >> 16);
}

// ------------------------------------------------------------------------------------------------ element decoders
// EPC elements per 16-byte chunk;  dot(w, x, acc): acc + the chunk's products, in element order;  gather(): the element-wise form of a chunk load
struct bf16_dec {
    typedef uint16_t elem;
    static constexpr int EPC = 8;
    static __device__ __forceinline__ float dot(const u32x4 w, const u32x4 x, float acc) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {                                                  // bf16 -> f32 is a shift
            acc = fmaf(__uint_as_float(w[e] << 16), __uint_as_float(x[e] << 16), acc);
            acc = fmaf(__uint_as_float(w[e] & 0xffff0000u), __uint_as_float(x[e] & 0xffff0000u), acc);
        }
        return acc;
    }
    static __device__ __forceinline__ f32x16 mfma(const u32x4 col, const u32x4 row, const f32x16 acc) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, col), __builtin_bit_cast(bf16x8, row), acc, 0, 0, 0);
    }
};
struct f32_dec {
    typedef float elem;
    static constexpr int EPC = 4;
    static __device__ __forceinline__ float dot(const u32x4 w, const u32x4 x, float acc) {
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = fmaf(__uint_as_float(w[e]), __uint_as_float(x[e]), acc);
        return acc;
    }
};
// chunk c of a row of K elements, element by element: indices clamped for the loads, a value past K zero
template <class Dec>
static __device__ __forceinline__ u32x4 mf_gather(const char * row, const int c, const int K) {
    typedef typename Dec::elem elem;
    u32x4 v = { 0u, 0u, 0u, 0u };
#pragma unroll
    for (int e = 0; e < Dec::EPC; ++e) {
        const int k = c * Dec::EPC + e;
        uint32_t bits = 0;
        const elem x = *(const elem *) (row + (size_t) (k < K ? k : K - 1) * sizeof(elem));
        __builtin_memcpy(&bits, &x, sizeof(elem));
        if (k >= K) bits = 0;
        if (sizeof(elem) == 2) v[e >> 1] |= bits << (16 * (e & 1)); else v[e] = bits;
    }
    return v;
}

// ------------------------------------------------------------------------------------------------ the ACT_BF16 image
// row r = (i1, i2) of b (i1 fastest) -> image r: K bf16, then zeros up to the image's 16-byte multiple
__global__ void __launch_bounds__(256) k_f32_to_bf16_rows(const char * __restrict__ x, size_t nb1, size_t nb2, int n1, char * __restrict__ y, size_t ys, int K) {
    const int64_t r = blockIdx.x;
    const float * xr = (const float *) (x + (size_t) (r % n1) * nb1 + (size_t) (r / n1) * nb2);
    uint16_t *    yr = (uint16_t *) (y + (size_t) r * ys);
    const int kp = (int) (ys >> 1);
    for (int k = threadIdx.x; k < kp; k += 256) yr[k] = k < K ? f32_to_bf16(xr[k]) : (uint16_t) 0;
}
void convert_f32_bf16_rows(const float * x, size_t nb1, size_t nb2, int64_t n1, int64_t n2, uint16_t * y, size_t ys, int64_t K, hipStream_t st) {
    if (K == 0 || n1 * n2 == 0) return;
    if (K > INT32_MAX || n1 > INT32_MAX || n1 * n2 > INT32_MAX || ys < (size_t) K * 2 || ys % 16 != 0) { fprintf(stderr, "[mi355x] convert_f32_bf16_rows: shape out of range\n"); abort(); }
    k_f32_to_bf16_rows<<<dim3((unsigned) (n1 * n2)), dim3(256), 0, st>>>((const char *) x, nb1, nb2, (int) n1, (char *) y, ys, (int) K);
}

// ------------------------------------------------------------------------------------------------ the per-pair mat-vec
struct mf_id_dev {
    const char * as; size_t as_nb1, as_nb2; int n_expert;
    const char * ids; size_t ids_nb0, ids_nb1;
    const char * b; size_t b_nb1, b_nb2; int b_ne1;      // column (i1, t) at b + i1 * b_nb1 + t * b_nb2: the bf16 images (b_nb2 = b_ne1 * b_nb1), or b's f32 columns in place
    char * dst; size_t dst_nb1, dst_nb2;
    int K, nrows;
};
static constexpr int MF_ROWS = 4;                                                      // rows per wave at a time

template <class Dec, bool VEC>
__global__ void __launch_bounds__(256) k_mmv_id_f(const mf_id_dev a) {
    typedef typename Dec::elem elem;
    const int i = blockIdx.y, t = blockIdx.z;
    int id = *(const int *) (a.ids + (size_t) i * a.ids_nb0 + (size_t) t * a.ids_nb1);
    id = id < 0 ? 0 : (id >= a.n_expert ? a.n_expert - 1 : id);
    id = __builtin_amdgcn_readfirstlane(id);
    const char * W   = a.as + (size_t) id * a.as_nb2;
    const char * col = a.b + (size_t) (i % a.b_ne1) * a.b_nb1 + (size_t) t * a.b_nb2;
    char * dst       = a.dst + (size_t) i * a.dst_nb1 + (size_t) t * a.dst_nb2;

    const int lane = threadIdx.x & 63;
    const int K = a.K, nrows = a.nrows;
    const int nch = (K + Dec::EPC - 1) / Dec::EPC;                                      // 16-byte chunks of a row (VEC: K / EPC)
    const int nit = (nch + 63) >> 6;
    const int wave   = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    const int nwaves = gridDim.x * 4;
    const int ngrp   = (nrows + MF_ROWS - 1) / MF_ROWS;

    u32x4 q[MF_ROWS];
    auto issue = [&](int grp, int it) {
        int c = it * 64 + lane; c = c < nch ? c : nch - 1;                             // clamped, not branched around: its contribution is dropped when consumed
#pragma unroll
        for (int r = 0; r < MF_ROWS; ++r) {
            int row = grp * MF_ROWS + r; row = row < nrows ? row : nrows - 1;
            const char * rp = W + (size_t) row * a.as_nb1;
            q[r] = VEC ? *(const u32x4 *) (rp + (size_t) c * 16) : mf_gather<Dec>(rp, c, K);
        }
    };
    // the first rows are requested before the column is staged; every wave reaches the barrier before any returns
    int grp = wave, it = 0;
    if (grp < ngrp) issue(grp, 0);
    for (int c = threadIdx.x; c < nch; c += 256)
        ((u32x4 *) mf_lds)[c] = (VEC || sizeof(elem) == 2) ? *(const u32x4 *) (col + (size_t) c * 16) : mf_gather<Dec>(col, c, K);      // (the bf16 image is 16-byte aligned and zero-padded)
    __syncthreads();
    if (grp >= ngrp) return;

    float acc[MF_ROWS];
#pragma unroll
    for (int r = 0; r < MF_ROWS; ++r) acc[r] = 0.0f;
    while (true) {
        u32x4 cq[MF_ROWS];
#pragma unroll
        for (int r = 0; r < MF_ROWS; ++r) cq[r] = q[r];
        const int cgrp = grp, cit = it;
        ++it;
        if (it == nit) { it = 0; grp += nwaves; }
        const bool more = grp < ngrp;
        if (more) issue(grp, it);

        const int  c     = cit * 64 + lane;
        const bool valid = c < nch;
        const u32x4 x = ((const u32x4 *) mf_lds)[valid ? c : nch - 1];
#pragma unroll
        for (int r = 0; r < MF_ROWS; ++r) { const float s = Dec::dot(cq[r], x, acc[r]); acc[r] = valid ? s : acc[r]; }
        if (cit == nit - 1) {
#pragma unroll
            for (int r = 0; r < MF_ROWS; ++r) {
                const int row = cgrp * MF_ROWS + r;
                const float s = wave_sum_f32(acc[r]);
                if (lane == 0 && row < nrows) *(float *) (dst + (size_t) row * 4) = s;
                acc[r] = 0.0f;
            }
        }
        if (!more) break;
    }
}

static long g_mmv_id_f_launches = 0;
long mmv_id_f_launches() { return g_mmv_id_f_launches; }

void mmv_id_f(const mmv_id_args & a, hipStream_t st) {
    if (a.nrows == 0 || a.n_ids == 0 || a.n_tokens == 0) return;
    const bool bf = a.type == GGML_TYPE_BF16;
    const size_t es = bf ? 2 : 4, lds = ((size_t) a.K * es + 15) & ~(size_t) 15;
    if ((!bf && a.type != GGML_TYPE_F32) || a.K < 1 || a.K > INT32_MAX || lds > (size_t) 152 * 1024 || a.n_ids > 65535 || a.n_tokens > 65535 || a.n_expert < 1 || a.b_ne1 < 1 ||
        a.nrows > INT32_MAX || a.as_nb1 < (size_t) a.K * es || a.as_nb1 % es != 0 || a.as_nb2 % es != 0 || (!bf && (a.b_nb1 % 4 != 0 || a.b_nb2 % 4 != 0))) {
        fprintf(stderr, "[mi355x] mmv_id_f: shape / type / stride out of range (type %d, K=%lld, ids %lld x %lld)\n", a.type, (long long) a.K, (long long) a.n_ids, (long long) a.n_tokens); abort();
    }
    // grid.x as mmv_id_mxfp4: every row group of one pair resident at once; with many pairs it shrinks so that the whole launch stays near 4 resident rounds of 1024
    // workgroups -- each workgroup then grid-strides over the pair's row groups and stages the pair's column once
    static const int cap = [] { const char * e = getenv("MI355X_MMV_WGS"); const int c = e ? atoi(e) : 1024; return c < 1 ? 1024 : c; }();
    const int64_t pairs = a.n_ids * a.n_tokens;
    int64_t gx = ((a.nrows + MF_ROWS - 1) / MF_ROWS + 3) / 4;
    const int64_t budget = (int64_t) cap * 4 / pairs;
    if (gx > budget) gx = budget;
    if (gx < 1) gx = 1;
    mf_id_dev d;
    d.as = (const char *) a.as; d.as_nb1 = a.as_nb1; d.as_nb2 = a.as_nb2; d.n_expert = (int) a.n_expert;
    d.ids = (const char *) a.ids; d.ids_nb0 = a.ids_nb0; d.ids_nb1 = a.ids_nb1;
    d.b = (const char *) a.act; d.b_ne1 = (int) a.b_ne1;
    if (bf) { d.b_nb1 = lds; d.b_nb2 = lds * (size_t) a.b_ne1; } else { d.b_nb1 = a.b_nb1; d.b_nb2 = a.b_nb2; }
    d.dst = (char *) a.dst; d.dst_nb1 = a.dst_nb1; d.dst_nb2 = a.dst_nb2;
    d.K = (int) a.K; d.nrows = (int) a.nrows;
    const bool vec = a.K % (16 / es) == 0 && (((uintptr_t) a.as | a.as_nb1 | a.as_nb2) & 15) == 0 && (bf || (((uintptr_t) a.act | a.b_nb1 | a.b_nb2) & 15) == 0);
    const dim3 grid((unsigned) gx, (unsigned) a.n_ids, (unsigned) a.n_tokens);
    auto go = [&](auto kern) {
        if (lds > 64 * 1024) HIP_CHECK(hipFuncSetAttribute((const void *) kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds));
        kern<<<grid, dim3(256), lds, st>>>(d);
    };
    if (bf) { if (vec) go(k_mmv_id_f<bf16_dec, true>); else go(k_mmv_id_f<bf16_dec, false>); }
    else    { if (vec) go(k_mmv_id_f<f32_dec, true>);  else go(k_mmv_id_f<f32_dec, false>); }
    ++g_mmv_id_f_launches;
}

// ------------------------------------------------------------------------------------------------ the grouped bf16-MFMA kernel
struct mm_id16_dev {
    const char * as; size_t as_nb1, as_nb2;
    const int * count; const moe_tile * tiles; const int * list;
    const char * act; size_t img; int b_ne1, n_ids;
    char * dst; size_t dst_nb1, dst_nb2;
    int K, nrows;
};
static constexpr int MM16_STEP = 4;                                                    // MFMA steps (16 weights of K each) per fetch step

template <class Dec, int KS>      // KS: waves per workgroup splitting K
__global__ void __launch_bounds__(64 * KS) __attribute__((amdgpu_waves_per_eu(2))) k_mm_id_16(const mm_id16_dev a) {
    if ((int) blockIdx.y >= *a.count) return;                            // (workgroup-uniform: the grid is the host's bound on the tile count)
    const moe_tile tl = a.tiles[blockIdx.y];
    size_t * dcol = (size_t *) mf_lds;                                   // [32] dst offset of every column of the slice
    float *  red  = (float *) (dcol + 32);                               // [KS - 1][64][16] fold area

    const int lane = threadIdx.x & 63, lq = lane & 31, hb = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int row = (int) blockIdx.x * 32 + lq;
    const bool row_ok = row < a.nrows;
    const char * wrow = a.as + (size_t) tl.expert * a.as_nb2 + (size_t) (row_ok ? row : a.nrows - 1) * a.as_nb1 + 16 * hb;      // (the tile table names clamped experts only)

    // ---- this lane's column: pair p = t * n_ids + i of the list -> image t * b_ne1 + i % b_ne1 (a lane past the slice carries its first column)
    const bool tok_ok = lq < tl.ncols;
    const int p = a.list[tl.first + (tok_ok ? lq : 0)];
    const int t = p / a.n_ids, i = p - t * a.n_ids;
    const char * acol = a.act + (size_t) (t * a.b_ne1 + i % a.b_ne1) * a.img + 16 * hb;
    if (threadIdx.x < 32 && tok_ok) dcol[lq] = (size_t) i * a.dst_nb1 + (size_t) t * a.dst_nb2;

    const int nmf = a.K >> 4, nstep = (nmf + MM16_STEP - 1) / MM16_STEP;
    struct stp { u32x4 w[MM16_STEP], x[MM16_STEP]; };                     // one fetch step of this lane's row, and of its column
    auto fetch = [&](int s, stp & G) {
#pragma unroll
        for (int u = 0; u < MM16_STEP; ++u) {
            int m = s * MM16_STEP + u; m = m < nmf ? m : nmf - 1;        // clamped, not branched around: an MFMA step past the row re-reads the last one
            G.w[u] = *(const u32x4 *) (wrow + (size_t) m * 32);
            G.x[u] = *(const u32x4 *) (acol + (size_t) m * 32);
        }
    };
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
    // this wave's fetch steps: wave, wave + KS, ...; the next one in flight while the current one's MFMAs run
    const int ns_w = wave < nstep ? (nstep - wave + KS - 1) / KS : 0;
    stp R[2];
    if (ns_w > 0) fetch(wave, R[0]);
    for (int i0 = 0; i0 < ns_w; i0 += 2) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int j = i0 + u;
            if (j < ns_w) {
                if (j + 1 < ns_w) fetch(wave + (j + 1) * KS, R[u ^ 1]);
                const int s = wave + j * KS;
#pragma unroll
                for (int v = 0; v < MM16_STEP; ++v)
                    if (s * MM16_STEP + v < nmf) acc = Dec::mfma(R[u].x[v], R[u].w[v], acc);      // (wave-uniform)
            }
        }
    }
    float out[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) out[e] = acc[e];
    if (KS == 1) __syncthreads();                                        // publishes dcol (KS > 1: the fold's barrier does)
    if (!mmq_fold<4, KS>(red, out, wave, lane)) return;
    if (!row_ok) return;
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = 8 * g + 4 * hb + e;
            if (c < tl.ncols) *(float *) (a.dst + dcol[c] + (size_t) row * 4) = out[4 * g + e];
        }
}

static mmq_id_stat g_mm_id_bf16_stat = { 0, 0 };
mmq_id_stat mm_id_bf16_stats() { return g_mm_id_bf16_stat; }
size_t mm_id_bf16_lds_bytes() { return 32 * sizeof(size_t) + (size_t) 7 * 64 * 16 * 4; }      // the slice's dst offsets + the widest fold (KS = 8)

void mm_id_bf16(const mmq_id_args & a, hipStream_t st) {
    const mmv_id_args & m = a.m;
    if (m.nrows == 0 || m.n_ids == 0 || m.n_tokens == 0) return;
    const int64_t n_pairs = m.n_ids * m.n_tokens;
    if (m.type != GGML_TYPE_BF16 || m.K < 16 || m.K % 16 != 0 || m.K > INT32_MAX || mm_id_bf16_lds_bytes() > MMQ_ID_LDS_MAX || n_pairs > MMQ_ID_MAX_PAIRS || m.n_expert < 1 ||
        m.n_expert > MMQ_ID_MAX_EXPERTS || m.b_ne1 < 1 || m.nrows > INT32_MAX || m.as_nb1 < (size_t) m.K * 2 || (((uintptr_t) m.as | m.as_nb1 | m.as_nb2) & 15) != 0 ||
        ((uintptr_t) m.act & 15) != 0 || a.scratch_bytes < moe_group_bytes(n_pairs, m.n_expert)) {
        fprintf(stderr, "[mi355x] mm_id_bf16: shape / type / alignment / scratch out of range (type %d, K=%lld, ids %lld x %lld, %lld experts)\n", m.type, (long long) m.K,
                (long long) m.n_ids, (long long) m.n_tokens, (long long) m.n_expert); abort();
    }
    const int64_t bound = moe_tile_bound(n_pairs, m.n_expert);                          // <= 4096 + 2^15: inside grid y
    const moe_group_out g = moe_group_launch(m, a.scratch, st);

    mm_id16_dev d;
    d.as = (const char *) m.as; d.as_nb1 = m.as_nb1; d.as_nb2 = m.as_nb2;
    d.count = g.count; d.tiles = g.tiles; d.list = g.list;
    d.act = (const char *) m.act; d.img = (size_t) m.K * 2; d.b_ne1 = (int) m.b_ne1; d.n_ids = (int) m.n_ids;      // (K % 16 == 0: the image has no pad)
    d.dst = (char *) m.dst; d.dst_nb1 = m.dst_nb1; d.dst_nb2 = m.dst_nb2;
    d.K = (int) m.K; d.nrows = (int) m.nrows;
    const int64_t row_tiles = (m.nrows + 31) / 32;
    const int units = (int) ((m.K / 16 + MM16_STEP - 1) / MM16_STEP);
    // waves per tile: mmq_id's rule on the grid BOUND -- towards the chip's 2048 wave slots in one round, at least 4 fetch steps per wave.  Host-known quantities only.
    int ks = 1;
    while (ks < 8 && row_tiles * bound * ks * 2 <= 3072 && ks * 4 <= units) ks *= 2;
    const dim3 grid((unsigned) row_tiles, (unsigned) bound);
    const size_t lds = 32 * sizeof(size_t) + (size_t) (ks - 1) * 64 * 16 * 4;
    if (ks == 8)      k_mm_id_16<bf16_dec, 8><<<grid, dim3(512), lds, st>>>(d);
    else if (ks == 4) k_mm_id_16<bf16_dec, 4><<<grid, dim3(256), lds, st>>>(d);
    else if (ks == 2) k_mm_id_16<bf16_dec, 2><<<grid, dim3(128), lds, st>>>(d);
    else              k_mm_id_16<bf16_dec, 1><<<grid, dim3(64), lds, st>>>(d);
    ++g_mm_id_bf16_stat.launches;
    g_mm_id_bf16_stat.ks = ks;
}

} // namespace mi
