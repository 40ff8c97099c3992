// mmq_id_blocks.hip -- MUL_MAT_ID on Q8_0 / Q4_0 / Q5_0 / IQ4_NL experts against MANY tokens (a prefill ubatch) on the int8 matrix cores of gfx950:
//     dst[:, i, t] = as[:, :, ids[i, t]] . b[:, i % b_ne1, t]          (ggml_compute_forward_mul_mat_id, ggml-cpu/ggml-cpu.c:1484 ff.)
// The four formats have the arithmetic shape of MXFP4: a block of 32 weights with one scale and no min term, against the Q8_0 images (common.hpp q80_image_bytes:
// qs[K] | f32 d[K / 32]) --
//     sumi    = sum_j w[j] * y.qs[j]            w: the block's 32 weights as int8
//     out[c] += (float) sumi * (d_y[ib][c] * d_x)
// which is ggml_vec_dot_q8_0_q8_0 / _q4_0_q8_0 / _q5_0_q8_0 / _iq4_nl_q8_0 (ggml-cpu/quants.c:305, :115, :219, :1108) and what the per-pair Forms of mmvq.hip compute.
// So the kernel is mmq_id_mxfp4.hip's with the block decoder as a parameter: the pairs grouped by expert on the device (mmq_id.hip k_moe_group: moe_group_launch), every
// (expert, 32-row tile, <= 32-column slice) one workgroup, ONE __builtin_amdgcn_mfma_i32_32x32x32_i8 per block.  One wave = 32 weight rows (lane & 31) x the slice's
// columns; hb = lane >> 5 is the K half of the MFMA: weights 16 hb .. 16 hb + 15 of the block against the activation bytes 32 ib + 16 hb of the lane's column.
// Register 4 g + i = column 8 g + 4 hb + i of the lane's row (the layout of mmq_dev.hpp).
//
// A Dec supplies what differs between the formats:
//   BYTES                 bytes per block (34 / 18 / 22 / 18; blocks and rows are 2-byte aligned -- the route's condition)
//   blk, load(bp, hb)     what a lane holds of one block of its row, and the loads that fill it (all inside the block)
//   weights(blk, hb)      the 16 int8 weights of half hb, four per dword, in the order of the activation bytes
//   scale(blk)            d_x, from the f16 header
// A lane fetches STEP = 8 consecutive blocks of its row at a time, the next step's weights and activations requested before the current one is consumed.  A ragged
// last step: block indices are clamped for the loads, and a block past the row (the index is wave-uniform) contributes nothing.  The KS waves of a workgroup take the
// steps wave, wave + KS, ...; the fold goes through LDS in wave order (mmq_fold).  KS is chosen from K, the row tiles and the grid bound only -- never from the ids --
// so a column's f32 summation order depends on the shape alone: results are bit-reproducible and independent of the other pairs in the tile.  Nothing on the host
// depends on the ids: a captured graph follows the ids of every replay.
#include "mmq_dev.hpp"
#include "blocks_dev.hpp"

namespace mi {

struct mmq_id_bl_dev {
    const char * as; size_t as_nb1, as_nb2;
    const int * count; const moe_tile * tiles; const int * list;
    const char * act; int b_ne1, n_ids;
    char * dst; size_t dst_nb1, dst_nb2;
    int K, nrows;
};

static constexpr int BL_STEP = 8;                                         // blocks per fetch step
typedef u32x4 __attribute__((aligned(2))) u32x4a2;

// Q8_0 {f16 d, int8 qs[32]}: half hb is qs[16 hb .. 16 hb + 15] as they are
struct q80_dec {
    static constexpr int BYTES = 34;
    struct blk { u32x4 q; uint32_t dw; };
    static __device__ __forceinline__ blk load(const char * bp, int hb) { return { *(const u32x4a2 *) (bp + 2 + 16 * hb), (uint32_t) *(const uint16_t *) bp }; }
    static __device__ __forceinline__ i32x4 weights(const blk & x, int) { return i32x4{ (int) x.q[0], (int) x.q[1], (int) x.q[2], (int) x.q[3] }; }
    static __device__ __forceinline__ float scale(const blk & x) { return h2f((uint16_t) x.dw); }
};
// the nibble formats: weight j of a block is the low nibble of qs[j], weight j + 16 the high one, so half hb takes the low (0) or high (1) nibbles of all 16 bytes.
// Q4_0 {f16 d, qs[16]}: nibble - 8.  With y = n ^ 8, n - 8 as int8 is y with its bit 3 copied into bits 4..7: y | (y & 8) * 30 (8 * 30 = 0xF0: nothing crosses a byte)
struct q40_dec {
    static constexpr int BYTES = 18;
    struct blk { u32x4 q; uint32_t dw; };
    static __device__ __forceinline__ blk load(const char * bp, int) { return { *(const u32x4a2 *) (bp + 2), (uint32_t) *(const uint16_t *) bp }; }
    static __device__ __forceinline__ i32x4 weights(const blk & x, int hb) {
        i32x4 w;
#pragma unroll
        for (int e = 0; e < 4; ++e) { const uint32_t y = ((x.q[e] >> (4 * hb)) & 0x0f0f0f0fu) ^ 0x08080808u; w[e] = (int) (y | ((y & 0x08080808u) * 30u)); }
        return w;
    }
    static __device__ __forceinline__ float scale(const blk & x) { return h2f((uint16_t) x.dw); }
};
// Q5_0 {f16 d, u32 qh, qs[16]}: (nibble | fifth bit << 4) - 16, bit j of qh the fifth bit of weight j.  With y = v ^ 16, v - 16 as int8 is y with its bit 4 copied
// into bits 5..7: y | (y & 16) * 14 (16 * 14 = 0xE0)
struct q50_dec {
    static constexpr int BYTES = 22;
    struct blk { u32x4 q; uint32_t dw; };                               // dw: d | the half's 16 fifth bits << 16 -- one register per block in flight
    static __device__ __forceinline__ blk load(const char * bp, int hb) {
        return { *(const u32x4a2 *) (bp + 6), (uint32_t) *(const uint16_t *) bp | ((uint32_t) *(const uint16_t *) (bp + 2 + 2 * hb) << 16) };
    }
    static __device__ __forceinline__ i32x4 weights(const blk & x, int hb) {
        i32x4 w;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t y = (((x.q[e] >> (4 * hb)) & 0x0f0f0f0fu) | spread5((x.dw >> (16 + 4 * e)) & 0xfu)) ^ 0x10101010u;
            w[e] = (int) (y | ((y & 0x10101010u) * 14u));
        }
        return w;
    }
    static __device__ __forceinline__ float scale(const blk & x) { return h2f((uint16_t) x.dw); }
};
// IQ4_NL {f16 d, qs[16]}: kvalues_iq4nl[nibble] (iq4nl_lut4)
struct iq4nl_dec {
    static constexpr int BYTES = 18;
    struct blk { u32x4 q; uint32_t dw; };
    static __device__ __forceinline__ blk load(const char * bp, int) { return { *(const u32x4a2 *) (bp + 2), (uint32_t) *(const uint16_t *) bp }; }
    static __device__ __forceinline__ i32x4 weights(const blk & x, int hb) {
        i32x4 w;
#pragma unroll
        for (int e = 0; e < 4; ++e) w[e] = (int) iq4nl_lut4((x.q[e] >> (4 * hb)) & 0x0f0f0f0fu);
        return w;
    }
    static __device__ __forceinline__ float scale(const blk & x) { return h2f((uint16_t) x.dw); }
};

// one (expert, 32-row tile, column slice) at NT column groups
template <class Dec, int NT, int KS, typename Stage>
static __device__ __forceinline__ void mmq_id_bl_tile(const mmq_id_bl_dev & a, const char * wrow, const char * acol, const int row, const bool row_ok, const int ncols,
                                                      const float * yd, float * red, const size_t * dcol, Stage stage_scales) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), hb = lane >> 5;
    const int nblk = a.K >> 5, nstep = (nblk + BL_STEP - 1) / BL_STEP;
    const char * arow = acol + 16 * hb;
    float out[NT * 4];
#pragma unroll
    for (int i = 0; i < NT * 4; ++i) out[i] = 0.0f;

    struct stp { typename Dec::blk w[BL_STEP]; u32x4 av[BL_STEP]; };      // one step of this lane's row, and of its column (its 16 bytes of every block)
    auto fetch = [&](int s, stp & G) {
#pragma unroll
        for (int u = 0; u < BL_STEP; ++u) {
            int ib = s * BL_STEP + u; ib = ib < nblk ? ib : nblk - 1;                // clamped, not branched around: a block past the row re-reads the last one
            G.w[u]  = Dec::load(wrow + (size_t) ib * Dec::BYTES, hb);
            G.av[u] = *(const u32x4 *) (arow + (size_t) ib * 32);
        }
    };
    auto reduce = [&](int s, const stp & G) {
#pragma unroll
        for (int u = 0; u < BL_STEP; ++u) {
            const int ib = s * BL_STEP + u;                                          // (wave-uniform)
            if (ib < nblk) {
                const i32x4 wv = Dec::weights(G.w[u], hb);
                const i32x4 aa = i32x4{ (int) G.av[u][0], (int) G.av[u][1], (int) G.av[u][2], (int) G.av[u][3] };      // (lanes past the slice's columns carry another column's bytes: their outputs are never stored)
                i32x16 z;
#pragma unroll
                for (int e = 0; e < 16; ++e) z[e] = 0;
                const i32x16 sj = __builtin_amdgcn_mfma_i32_32x32x32_i8(aa, wv, z, 0, 0, 0);
                const float dx = Dec::scale(G.w[u]);
#pragma unroll
                for (int g = 0; g < NT; ++g) {
                    const f32x4 y4 = *(const f32x4 *) (yd + ib * 32 + 8 * g + 4 * hb);
#pragma unroll
                    for (int i = 0; i < 4; ++i) out[4 * g + i] += (float) sj[4 * g + i] * (y4[i] * dx);
                }
            }
        }
    };
    // this wave's steps: wave, wave + KS, ...; two register sets, the next step in flight while the current one is reduced
    const int ns_w = wave < nstep ? (nstep - wave + KS - 1) / KS : 0;
    stp R[2];
    if (ns_w > 0) fetch(wave, R[0]);
    stage_scales();
    for (int i0 = 0; i0 < ns_w; i0 += 2) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int i = i0 + u;
            if (i < ns_w) {
                if (i + 1 < ns_w) fetch(wave + (i + 1) * KS, R[u ^ 1]);
                reduce(wave + i * KS, R[u]);
            }
        }
    }
    if (!mmq_fold<NT, KS>(red, out, wave, lane)) return;
    if (!row_ok) return;
#pragma unroll
    for (int g = 0; g < NT; ++g)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = 8 * g + 4 * hb + i;
            if (c < ncols) *(float *) (a.dst + dcol[c] + (size_t) row * 4) = out[4 * g + i];
        }
}

template <class Dec, int KS>     // KS: waves per workgroup splitting K
__global__ void __launch_bounds__(64 * KS) __attribute__((amdgpu_waves_per_eu(2))) k_mmq_id_blocks(const mmq_id_bl_dev a) {
    extern __shared__ __attribute__((aligned(16))) char mmq_bl_lds[];
    if ((int) blockIdx.y >= *a.count) return;                            // (workgroup-uniform: the grid is the host's bound on the tile count)
    const moe_tile tl = a.tiles[blockIdx.y];
    const int nblk = a.K >> 5;
    size_t * dcol = (size_t *) mmq_bl_lds;                               // [32] dst offset of every column of the slice
    float * yd  = (float *) (dcol + 32);                                 // [nblk][32] column scales of every block (transposed)
    float * red = yd + nblk * 32;                                        // [KS - 1][64][16] fold area

    const int lane = threadIdx.x & 63, lq = lane & 31;
    const int row = (int) blockIdx.x * 32 + lq;
    const bool row_ok = row < a.nrows;
    const char * wrow = a.as + (size_t) tl.expert * a.as_nb2 + (size_t) (row_ok ? row : a.nrows - 1) * a.as_nb1;      // (the tile table names clamped experts only)

    // ---- this lane's column: pair p = t * n_ids + i of the list -> image t * b_ne1 + i % b_ne1 (lanes past the slice carry its first column's bytes)
    const bool tok_ok = lq < tl.ncols;
    const int p = a.list[tl.first + (tok_ok ? lq : 0)];
    const int t = p / a.n_ids, i = p - t * a.n_ids;
    const char * acol = a.act + (size_t) (t * a.b_ne1 + i % a.b_ne1) * q80_image_bytes(a.K);
    if (threadIdx.x < 32 && tok_ok) dcol[lq] = (size_t) i * a.dst_nb1 + (size_t) t * a.dst_nb2;

    // ---- column scales of all blocks -> LDS, transposed: yd[b][c]; the stride is a multiple of 32, so every thread stages its own column lq.  The barrier also
    //      publishes dcol.  (called after the first step's loads are in flight)
    const int K = a.K;
    auto stage_scales = [&]() {
        for (int j = threadIdx.x; j < nblk * 32; j += 64 * KS) yd[j] = tok_ok ? *(const float *) (acol + K + 4 * (j >> 5)) : 0.0f;
        __syncthreads();
    };
    const int nt = (tl.ncols + 7) >> 3;
    if (nt == 1)      mmq_id_bl_tile<Dec, 1, KS>(a, wrow, acol, row, row_ok, tl.ncols, yd, red, dcol, stage_scales);
    else if (nt == 2) mmq_id_bl_tile<Dec, 2, KS>(a, wrow, acol, row, row_ok, tl.ncols, yd, red, dcol, stage_scales);
    else if (nt == 3) mmq_id_bl_tile<Dec, 3, KS>(a, wrow, acol, row, row_ok, tl.ncols, yd, red, dcol, stage_scales);
    else              mmq_id_bl_tile<Dec, 4, KS>(a, wrow, acol, row, row_ok, tl.ncols, yd, red, dcol, stage_scales);
}

static long g_mmq_id_blocks_launches = 0;
long mmq_id_blocks_launches() { return g_mmq_id_blocks_launches; }
static int g_mmq_id_blocks_ks = 0;                                                       // KS of the most recent launch (0: none yet)
int mmq_id_blocks_last_ks() { return g_mmq_id_blocks_ks; }

bool mmq_id_blocks_takes(int type) { return type == GGML_TYPE_Q8_0 || type == GGML_TYPE_Q4_0 || type == GGML_TYPE_Q5_0 || type == GGML_TYPE_IQ4_NL; }
size_t mmq_id_blocks_lds_bytes(int64_t K) { return 32 * sizeof(size_t) + (size_t) (K >> 5) * 32 * 4 + (size_t) 7 * 64 * 16 * 4; }      // at the widest fold (KS = 8)

template <class Dec>
static void mmq_id_blocks_go(const mmq_id_bl_dev & d, const dim3 grid, const int ks, const size_t lds, hipStream_t st) {
    if (ks == 8)      k_mmq_id_blocks<Dec, 8><<<grid, dim3(512), lds, st>>>(d);
    else if (ks == 4) k_mmq_id_blocks<Dec, 4><<<grid, dim3(256), lds, st>>>(d);
    else if (ks == 2) k_mmq_id_blocks<Dec, 2><<<grid, dim3(128), lds, st>>>(d);
    else              k_mmq_id_blocks<Dec, 1><<<grid, dim3(64), lds, st>>>(d);
}

void mmq_id_blocks(const mmq_id_args & a, hipStream_t st) {
    const mmv_id_args & m = a.m;
    if (m.nrows == 0 || m.n_ids == 0 || m.n_tokens == 0) return;
    const int64_t n_pairs = m.n_ids * m.n_tokens;
    const size_t bytes = m.type == GGML_TYPE_Q8_0 ? q80_dec::BYTES : m.type == GGML_TYPE_Q5_0 ? q50_dec::BYTES : q40_dec::BYTES;
    if (!mmq_id_blocks_takes(m.type) || m.K < 32 || m.K % 32 != 0 || m.K > INT32_MAX || mmq_id_blocks_lds_bytes(m.K) > MMQ_ID_LDS_MAX || n_pairs > MMQ_ID_MAX_PAIRS || m.n_expert < 1 ||
        m.n_expert > MMQ_ID_MAX_EXPERTS || m.b_ne1 < 1 || m.nrows > INT32_MAX || m.as_nb1 < (size_t) (m.K / 32) * bytes || m.as_nb1 % 2 != 0 || m.as_nb2 % 2 != 0 ||
        ((uintptr_t) m.as & 1) != 0 || a.scratch_bytes < moe_group_bytes(n_pairs, m.n_expert)) {
        fprintf(stderr, "[mi355x] mmq_id_blocks: shape / type / alignment / scratch out of range (type %d, K=%lld, ids %lld x %lld, %lld experts)\n", m.type, (long long) m.K,
                (long long) m.n_ids, (long long) m.n_tokens, (long long) m.n_expert); abort();
    }
    const int64_t bound = moe_tile_bound(n_pairs, m.n_expert);                          // <= 4096 + 2^15: inside grid y
    const moe_group_out g = moe_group_launch(m, a.scratch, st);

    mmq_id_bl_dev d;
    d.as = (const char *) m.as; d.as_nb1 = m.as_nb1; d.as_nb2 = m.as_nb2;
    d.count = g.count; d.tiles = g.tiles; d.list = g.list;
    d.act = (const char *) m.act; d.b_ne1 = (int) m.b_ne1; d.n_ids = (int) m.n_ids;
    d.dst = (char *) m.dst; d.dst_nb1 = m.dst_nb1; d.dst_nb2 = m.dst_nb2;
    d.K = (int) m.K; d.nrows = (int) m.nrows;
    const int64_t row_tiles = (m.nrows + 31) / 32;
    const int nblk = (int) (m.K >> 5), nstep = (nblk + BL_STEP - 1) / BL_STEP;
    // waves per tile: mmq_id_mxfp4's rule on the grid BOUND -- towards the chip's 2048 wave slots in one round, at least 4 steps per wave.  Host-known quantities only.
    int ks = 1;
    while (ks < 8 && row_tiles * bound * ks * 2 <= 3072 && ks * 4 <= nstep) ks *= 2;
    const dim3 grid((unsigned) row_tiles, (unsigned) bound);
    const size_t lds = 32 * sizeof(size_t) + (size_t) nblk * 32 * 4 + (size_t) (ks - 1) * 64 * 16 * 4;
    switch (m.type) {
        case GGML_TYPE_Q8_0: mmq_id_blocks_go<q80_dec>(d, grid, ks, lds, st); break;
        case GGML_TYPE_Q4_0: mmq_id_blocks_go<q40_dec>(d, grid, ks, lds, st); break;
        case GGML_TYPE_Q5_0: mmq_id_blocks_go<q50_dec>(d, grid, ks, lds, st); break;
        default:             mmq_id_blocks_go<iq4nl_dec>(d, grid, ks, lds, st); break;
    }
    ++g_mmq_id_blocks_launches;
    g_mmq_id_blocks_ks = ks;
}

} // namespace mi
