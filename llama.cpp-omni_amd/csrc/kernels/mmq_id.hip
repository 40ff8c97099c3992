// mmq_id.hip -- MUL_MAT_ID against MANY tokens (a prefill ubatch) on the int8 matrix cores of gfx950, for K-quant (Q4_K / Q5_K / Q6_K), MXFP4 (gpt-oss) and
// Q8_0 / Q4_0 / Q5_0 / IQ4_NL experts:
//     dst[:, i, t] = as[:, :, ids[i, t]] . b[:, i % b_ne1, t]          (ggml_compute_forward_mul_mat_id, ggml-cpu/ggml-cpu.c:1484 ff.)
// The per-pair mat-vecs (mmvk.hip k_mmv_id, mmv_mxfp4.hip, mmvq.hip k_mmv_blocks_id) stream one expert matrix per (slot, token) pair: right for decode, but a 512-token
// ubatch of 8 used experts reads 4096 matrices where 128 distinct ones exist (gpt-oss-20b: 2048 where 32 exist).  Here the pairs are grouped by expert ON THE DEVICE and
// every (expert, 32-row tile, <= 32-column slice) is one workgroup: a weight block read once per 32 columns instead of once per column.
//
// Two launches per node, nothing data-dependent on the host (a captured graph follows the ids of every replay):
//   k_moe_group  one workgroup: LDS histogram of the (clamped) ids, scan, placement.  Writes into the node's scratch (moe_group_bytes):
//                  [0]      the tile count
//                  tiles[]  one entry per non-empty (expert, <= 32-column slice): expert, first position in the pair list, column count
//                  list[]   the pair indices p = t * n_ids + i, ordered by expert (inside an expert in arrival order of the LDS atomics: NOT stable -- no result
//                           depends on it, a column's sum is a function of its own weights, image and the launch's KS alone)
//   k_mmq_id     grid = 32-row tiles x the host-side BOUND on the tile count, min(n_pairs, n_expert) + n_pairs / 32 (every non-empty expert has at most one ragged slice);
//                a workgroup whose slot is past the device-side count returns at once.  Columns are read and results stored through the pair list.
// KS (waves splitting K) is chosen from K, the row tiles and the grid bound only -- never from the ids -- so a column's f32 summation order depends on the shape alone:
// results are bit-reproducible and independent of the other pairs in the tile.  The column-group count NT (1..4 groups of 8) is known on the device only: the workgroup
// branches uniformly into the templated bodies.
//
// k_mmq_id<Body, KS, NT4> is ONE frame -- count check, tile look-up, LDS carve-up, row and column set-up, the columns' block scales into LDS, the NT branch and, in
// mmq_id_finish, the KS fold (mmq_dev.hpp mmq_fold) and the store through the slice's dst offsets -- around a Body, which supplies
//   SB_SHIFT              log2 of the weights per scale block of the activation image (8: Q8_K images, 5: Q8_0 images)
//   scales(acol, K)       where the f32 block scales sit in a column's image;  image_bytes(K): the image size per column
//   tile<NT, KS>(...)     the K blocks of this wave into its own out[] -- register 4 g + i = column 8 g + 4 hb + i of the lane's row (hb = lane >> 5, the K half of the
//                         MFMA), the wave index kept the way the body wants it (in a scalar register or not) -- handed to mmq_id_finish
// Two bodies:
//   mmq_id_kquant_body    mmq.hip's blocks (mmq_dev.hpp mmq_blocks): the vec_dot_q*_K_q8_K integers against the Q8_K images.  MI355X_MMQ_ID_NT4=1 keeps every tile of
//                         this body on the four-group instance (NT4: the measurement switch of tools/moe_mmq_bench.py)
//   mmq_id_stepped_body   a block of 32 weights with one scale and no min term against the Q8_0 images (common.hpp q80_image_bytes: qs[K] | f32 d[K / 32]) --
//                             sumi    = sum_j w[j] * y.qs[j]            w: the block's 32 weights as int8
//                             out[c] += (float) sumi * (d_y[ib][c] * d_x)
//                         ONE __builtin_amdgcn_mfma_i32_32x32x32_i8 per block is the reference's sumi for 32 rows x 32 columns: weights 16 hb .. 16 hb + 15 of the block
//                         against the activation bytes 32 ib + 16 hb of the lane's column.  The float epilogue per block is NT * 4 registers wide: it, not the MFMA, is
//                         what a block costs.  A Dec supplies what differs between the formats:
//                           BYTES                 bytes per block (17 / 34 / 18 / 22 / 18)
//                           load(bp, hb)          what a lane holds of one block of its row (mmq_id_blk), by loads that stay inside the block
//                           weights(blk, hb)      the 16 int8 weights of half hb, four per dword, in the order of the activation bytes
//                           scale(blk)            d_x, from the block's header
//                         A lane fetches STEP = 8 consecutive blocks of its row at a time (the 256 weights of a K-quant block), the next step's weights and activations
//                         requested before the current one is consumed.  A ragged last step (gpt-oss rows are 90 blocks): block indices are clamped for the loads, and
//                         a block past the row (the index is wave-uniform) contributes nothing.  The KS waves of a workgroup take the steps wave, wave + KS, ...
#include "mmq_dev.hpp"
#include "mxfp4_dev.hpp"
#include "blocks_dev.hpp"

namespace mi {

// (moe_tile, one entry of the tile table, and moe_group_out, where a grouping lies in the scratch: kernels.hpp)
static constexpr size_t MOE_HDR = 16;                                                  // the tile count, padded so that the table behind it is 16-byte aligned

int64_t moe_tile_bound(int64_t n_pairs, int64_t n_expert) { return (n_pairs < n_expert ? n_pairs : n_expert) + n_pairs / 32; }
size_t  moe_group_bytes(int64_t n_pairs, int64_t n_expert) { return MOE_HDR + (size_t) moe_tile_bound(n_pairs, n_expert) * sizeof(moe_tile) + (size_t) n_pairs * 4; }

struct moe_group_dev {
    const char * ids; size_t ids_nb0, ids_nb1;
    int n_ids, n_pairs, n_expert;
    int * count; moe_tile * tiles; int * list;
};

static constexpr int GROUP_THREADS = 1024;
// LDS: cnt[n_expert] (histogram, then the placement cursors), tile0[n_expert] (first tile of every expert), part[2][GROUP_THREADS] (the scan over the threads' chunks)
__global__ void __launch_bounds__(GROUP_THREADS) k_moe_group(const moe_group_dev a) {
    extern __shared__ __attribute__((aligned(16))) char grp_lds[];
    int * cnt = (int *) grp_lds, * tile0 = cnt + a.n_expert, * part_p = tile0 + a.n_expert, * part_t = part_p + GROUP_THREADS;
    const int tid = threadIdx.x;
    auto expert_of = [&](int p) {
        const int t = p / a.n_ids, i = p - t * a.n_ids;
        const int id = *(const int *) (a.ids + (size_t) i * a.ids_nb0 + (size_t) t * a.ids_nb1);
        return id < 0 ? 0 : (id >= a.n_expert ? a.n_expert - 1 : id);                 // clamped before it becomes an index, as k_mmv_id
    };
    for (int e = tid; e < a.n_expert; e += GROUP_THREADS) cnt[e] = 0;
    __syncthreads();
    for (int p = tid; p < a.n_pairs; p += GROUP_THREADS) atomicAdd(&cnt[expert_of(p)], 1);
    __syncthreads();
    // ---- exclusive scan of (pairs, tiles) over the experts: every thread a chunk of consecutive experts, Hillis-Steele over the chunk sums
    const int ch = (a.n_expert + GROUP_THREADS - 1) / GROUP_THREADS;
    const int e0 = tid * ch < a.n_expert ? tid * ch : a.n_expert, e1 = e0 + ch < a.n_expert ? e0 + ch : a.n_expert;
    int sp = 0, stl = 0;
    for (int e = e0; e < e1; ++e) { sp += cnt[e]; stl += (cnt[e] + 31) >> 5; }
    part_p[tid] = sp; part_t[tid] = stl;
    __syncthreads();
    for (int d = 1; d < GROUP_THREADS; d <<= 1) {
        const int vp = tid >= d ? part_p[tid - d] : 0, vt = tid >= d ? part_t[tid - d] : 0;
        __syncthreads();
        part_p[tid] += vp; part_t[tid] += vt;
        __syncthreads();
    }
    int pos = part_p[tid] - sp, tl = part_t[tid] - stl;                                 // exclusive prefix of this thread's chunk
    if (tid == GROUP_THREADS - 1) *a.count = part_t[tid];
    for (int e = e0; e < e1; ++e) {
        const int c = cnt[e];
        for (int k = 0; k * 32 < c; ++k) a.tiles[tl + k] = { e, pos + 32 * k, c - 32 * k < 32 ? c - 32 * k : 32 };
        cnt[e] = pos;                                                                   // from here on: the expert's placement cursor
        pos += c; tl += (c + 31) >> 5;
    }
    __syncthreads();
    for (int p = tid; p < a.n_pairs; p += GROUP_THREADS) a.list[atomicAdd(&cnt[expert_of(p)], 1)] = p;
}

struct mmq_id_dev {
    const char * as; size_t as_nb1, as_nb2;
    const int * count; const moe_tile * tiles; const int * list;
    const char * act; int b_ne1, n_ids;
    char * dst; size_t dst_nb1, dst_nb2;
    int K, nrows, type;
};

// ------------------------------------------------------------------------------------------------ the frame
// the end of one (expert, 32-row tile, column slice) at NT column groups: the KS fold, the store through the slice's dst offsets.  (The bodies call this with their
// accumulators, not the other way round: accumulators handed INTO a body's loop by reference change how the compiler vectorises the loop's f32 epilogue -- 8 more
// VGPRs in every stepped instance, profiles/mmq_id_frame_ab.txt B)
template <int NT, int KS>
static __device__ __forceinline__ void mmq_id_finish(const mmq_id_dev & a, float * red, float (&out)[NT * 4], const int wave, const int lane, const int hb, const int row,
                                                     const bool row_ok, const int ncols, const size_t * dcol) {
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

// ------------------------------------------------------------------------------------------------ the bodies
// (the K-quant tile is a free function, as it always was: as a member of its body the compiler lays the NT branch out differently)
template <int NT, int KS, typename Stage>
static __device__ __forceinline__ void mmq_id_kquant_tile(const mmq_id_dev & a, const char * wrow, const char * acol, const int row, const bool row_ok, const int ncols,
                                                          const float * yd, float * red, const size_t * dcol, Stage stage_scales) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hb = lane >> 5;
    float out[NT * 4];
#pragma unroll
    for (int i = 0; i < NT * 4; ++i) out[i] = 0.0f;
    mmq_blocks<NT, KS>(a.type, wrow, acol, a.K >> 8, wave, hb, yd, out, stage_scales);
    mmq_id_finish<NT, KS>(a, red, out, wave, lane, hb, row, row_ok, ncols, dcol);
}
struct mmq_id_kquant_body {
    static constexpr int SB_SHIFT = 8;
    static __device__ __forceinline__ const char * scales(const char * acol, int K) { return acol + K + (K >> 3); }
    static __device__ __forceinline__ size_t image_bytes(int K) { return q8k_image_bytes(K); }
    template <int NT, int KS, typename Stage>
    static __device__ __forceinline__ void tile(const mmq_id_dev & a, const char * wrow, const char * acol, const int row, const bool row_ok, const int ncols,
                                                const float * yd, float * red, const size_t * dcol, Stage stage_scales) {
        mmq_id_kquant_tile<NT, KS>(a, wrow, acol, row, row_ok, ncols, yd, red, dcol, stage_scales);
    }
};

struct mmq_id_blk { u32x4 q; uint32_t dw; };                              // what a lane holds of one 32-weight block: 16 quant bytes and a header word
typedef u32x4 __attribute__((aligned(1))) u32x4a1;
typedef u32x4 __attribute__((aligned(2))) u32x4a2;                        // (blocks and rows of the f16-header formats are 2-byte aligned -- the route's condition)

// MXFP4 {uint8 e; uint8 qs[16]}: ggml_vec_dot_mxfp4_q8_0 (ggml-cpu/quants.c:188-215), in the product order of the per-pair kernel:
//     sumi    = sum_j y.qs[j] * kv[x.qs[j] & 0xF] + y.qs[j + 16] * kv[x.qs[j] >> 4]
//     out[c] += (float) sumi * (d_y[ib][c] * e8m0_half(x.e))
// weight j of a block is the low nibble of qs[j], weight j + 16 the high one, so half hb takes the low (0) or high (1) nibbles of all 16 quant bytes -- four mxfp4_lut4.
// The 16 quant bytes sit at row + 17 ib + 1, at any alignment: one 1-byte-aligned 16-byte load that never leaves the block (as mmv_mxfp4.hip's 8-byte one).  dw: e
struct mxfp4_dec {
    static constexpr int BYTES = 17;
    static __device__ __forceinline__ mmq_id_blk load(const char * bp, int) { return { *(const u32x4a1 *) (bp + 1), (uint32_t) *(const uint8_t *) bp }; }
    static __device__ __forceinline__ i32x4 weights(const mmq_id_blk & x, int hb) {
        i32x4 w;
#pragma unroll
        for (int e = 0; e < 4; ++e) w[e] = (int) mxfp4_lut4((x.q[e] >> (4 * hb)) & 0x0f0f0f0fu);
        return w;
    }
    static __device__ __forceinline__ float scale(const mmq_id_blk & x) { return e8m0_half(x.dw); }
};
// The f16-header formats: ggml_vec_dot_q8_0_q8_0 / _q4_0_q8_0 / _q5_0_q8_0 / _iq4_nl_q8_0 (ggml-cpu/quants.c:305, :115, :219, :1108), what the per-pair Forms of mmvq.hip
// compute.  dw: d (Q5_0: and the half's fifth bits)
// Q8_0 {f16 d, int8 qs[32]}: half hb is qs[16 hb .. 16 hb + 15] as they are
struct q80_dec {
    static constexpr int BYTES = 34;
    static __device__ __forceinline__ mmq_id_blk load(const char * bp, int hb) { return { *(const u32x4a2 *) (bp + 2 + 16 * hb), (uint32_t) *(const uint16_t *) bp }; }
    static __device__ __forceinline__ i32x4 weights(const mmq_id_blk & x, int) { return i32x4{ (int) x.q[0], (int) x.q[1], (int) x.q[2], (int) x.q[3] }; }
    static __device__ __forceinline__ float scale(const mmq_id_blk & x) { return h2f((uint16_t) x.dw); }
};
// the nibble formats: weight j of a block is the low nibble of qs[j], weight j + 16 the high one, so half hb takes the low (0) or high (1) nibbles of all 16 bytes.
// Q4_0 {f16 d, qs[16]}: nibble - 8.  With y = n ^ 8, n - 8 as int8 is y with its bit 3 copied into bits 4..7: y | (y & 8) * 30 (8 * 30 = 0xF0: nothing crosses a byte)
struct q40_dec {
    static constexpr int BYTES = 18;
    static __device__ __forceinline__ mmq_id_blk load(const char * bp, int) { return { *(const u32x4a2 *) (bp + 2), (uint32_t) *(const uint16_t *) bp }; }
    static __device__ __forceinline__ i32x4 weights(const mmq_id_blk & x, int hb) {
        i32x4 w;
#pragma unroll
        for (int e = 0; e < 4; ++e) { const uint32_t y = ((x.q[e] >> (4 * hb)) & 0x0f0f0f0fu) ^ 0x08080808u; w[e] = (int) (y | ((y & 0x08080808u) * 30u)); }
        return w;
    }
    static __device__ __forceinline__ float scale(const mmq_id_blk & x) { return h2f((uint16_t) x.dw); }
};
// Q5_0 {f16 d, u32 qh, qs[16]}: (nibble | fifth bit << 4) - 16, bit j of qh the fifth bit of weight j.  With y = v ^ 16, v - 16 as int8 is y with its bit 4 copied
// into bits 5..7: y | (y & 16) * 14 (16 * 14 = 0xE0).  dw: d | the half's 16 fifth bits << 16 -- one register per block in flight
struct q50_dec {
    static constexpr int BYTES = 22;
    static __device__ __forceinline__ mmq_id_blk load(const char * bp, int hb) {
        return { *(const u32x4a2 *) (bp + 6), (uint32_t) *(const uint16_t *) bp | ((uint32_t) *(const uint16_t *) (bp + 2 + 2 * hb) << 16) };
    }
    static __device__ __forceinline__ i32x4 weights(const mmq_id_blk & x, int hb) {
        i32x4 w;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t y = (((x.q[e] >> (4 * hb)) & 0x0f0f0f0fu) | spread5((x.dw >> (16 + 4 * e)) & 0xfu)) ^ 0x10101010u;
            w[e] = (int) (y | ((y & 0x10101010u) * 14u));
        }
        return w;
    }
    static __device__ __forceinline__ float scale(const mmq_id_blk & x) { return h2f((uint16_t) x.dw); }
};
// IQ4_NL {f16 d, qs[16]}: kvalues_iq4nl[nibble] (iq4nl_lut4)
struct iq4nl_dec {
    static constexpr int BYTES = 18;
    static __device__ __forceinline__ mmq_id_blk load(const char * bp, int) { return { *(const u32x4a2 *) (bp + 2), (uint32_t) *(const uint16_t *) bp }; }
    static __device__ __forceinline__ i32x4 weights(const mmq_id_blk & x, int hb) {
        i32x4 w;
#pragma unroll
        for (int e = 0; e < 4; ++e) w[e] = (int) iq4nl_lut4((x.q[e] >> (4 * hb)) & 0x0f0f0f0fu);
        return w;
    }
    static __device__ __forceinline__ float scale(const mmq_id_blk & x) { return h2f((uint16_t) x.dw); }
};

static constexpr int MMQ_ID_STEP = 8;                                     // blocks per fetch step

template <class Dec>
struct mmq_id_stepped_body {
    static constexpr int SB_SHIFT = 5;
    static __device__ __forceinline__ const char * scales(const char * acol, int K) { return acol + K; }
    static __device__ __forceinline__ size_t image_bytes(int K) { return q80_image_bytes(K); }
    template <int NT, int KS, typename Stage>
    static __device__ __forceinline__ void tile(const mmq_id_dev & a, const char * wrow, const char * acol, const int row, const bool row_ok, const int ncols,
                                                const float * yd, float * red, const size_t * dcol, Stage stage_scales) {
        const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), hb = lane >> 5;
        const int nblk = a.K >> 5, nstep = (nblk + MMQ_ID_STEP - 1) / MMQ_ID_STEP;
        const char * arow = acol + 16 * hb;
        float out[NT * 4];
#pragma unroll
        for (int i = 0; i < NT * 4; ++i) out[i] = 0.0f;
        struct stp { mmq_id_blk w[MMQ_ID_STEP]; u32x4 av[MMQ_ID_STEP]; };    // one step of this lane's row, and of its column (its 16 bytes of every block)
        auto fetch = [&](int s, stp & G) {
#pragma unroll
            for (int u = 0; u < MMQ_ID_STEP; ++u) {
                int ib = s * MMQ_ID_STEP + u; ib = ib < nblk ? ib : nblk - 1;        // clamped, not branched around: a block past the row re-reads the last one
                G.w[u]  = Dec::load(wrow + (size_t) ib * Dec::BYTES, hb);
                G.av[u] = *(const u32x4 *) (arow + (size_t) ib * 32);
            }
        };
        auto reduce = [&](int s, const stp & G) {
#pragma unroll
            for (int u = 0; u < MMQ_ID_STEP; ++u) {
                const int ib = s * MMQ_ID_STEP + u;                                  // (wave-uniform)
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
        mmq_id_finish<NT, KS>(a, red, out, wave, lane, hb, row, row_ok, ncols, dcol);
    }
};

template <class Body, int KS, bool NT4>      // KS: waves per workgroup splitting K; NT4: every tile on the four-group body
__global__ void __launch_bounds__(64 * KS) __attribute__((amdgpu_waves_per_eu(2))) k_mmq_id(const mmq_id_dev a) {
    extern __shared__ __attribute__((aligned(16))) char mmq_lds[];
    if ((int) blockIdx.y >= *a.count) return;                            // (workgroup-uniform: the grid is the host's bound on the tile count)
    const moe_tile tl = a.tiles[blockIdx.y];
    const int nblk = a.K >> Body::SB_SHIFT;
    size_t * dcol = (size_t *) mmq_lds;                                  // [32] dst offset of every column of the slice
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
    const char * acol = a.act + (size_t) (t * a.b_ne1 + i % a.b_ne1) * Body::image_bytes(a.K);
    if (threadIdx.x < 32 && tok_ok) dcol[lq] = (size_t) i * a.dst_nb1 + (size_t) t * a.dst_nb2;

    // ---- column scales of all blocks -> LDS, transposed: yd[b][c]; the stride is a multiple of 32, so every thread stages its own column lq.  The barrier also
    //      publishes dcol.  (called after the body's first loads are in flight)
    const int K = a.K;
    auto stage_scales = [&]() {
        for (int j = threadIdx.x; j < nblk * 32; j += 64 * KS) yd[j] = tok_ok ? *(const float *) (Body::scales(acol, K) + 4 * (j >> 5)) : 0.0f;
        __syncthreads();
    };
    const int nt = NT4 ? 4 : (tl.ncols + 7) >> 3;
    if (nt == 1)      Body::template tile<1, KS>(a, wrow, acol, row, row_ok, tl.ncols, yd, red, dcol, stage_scales);
    else if (nt == 2) Body::template tile<2, KS>(a, wrow, acol, row, row_ok, tl.ncols, yd, red, dcol, stage_scales);
    else if (nt == 3) Body::template tile<3, KS>(a, wrow, acol, row, row_ok, tl.ncols, yd, red, dcol, stage_scales);
    else              Body::template tile<4, KS>(a, wrow, acol, row, row_ok, tl.ncols, yd, red, dcol, stage_scales);
}

// ------------------------------------------------------------------------------------------------ host
// the grouping of one node into its scratch (moe_group_bytes; the caller has checked the pair and expert counts against MMQ_ID_MAX_* and the scratch size)
moe_group_out moe_group_launch(const mmv_id_args & m, void * scratch, hipStream_t st) {
    const int64_t n_pairs = m.n_ids * m.n_tokens, bound = moe_tile_bound(n_pairs, m.n_expert);
    moe_group_dev g;
    g.ids = (const char *) m.ids; g.ids_nb0 = m.ids_nb0; g.ids_nb1 = m.ids_nb1;
    g.n_ids = (int) m.n_ids; g.n_pairs = (int) n_pairs; g.n_expert = (int) m.n_expert;
    g.count = (int *) scratch; g.tiles = (moe_tile *) ((char *) scratch + MOE_HDR); g.list = (int *) ((char *) scratch + MOE_HDR + (size_t) bound * sizeof(moe_tile));
    k_moe_group<<<dim3(1), dim3(GROUP_THREADS), ((size_t) m.n_expert * 2 + GROUP_THREADS * 2) * 4, st>>>(g);
    return { g.count, g.tiles, g.list };
}

// what the launcher knows of a family.  K is a multiple of `gran` weights (one scale block of the activation image) and at least kmin; the KS rule counts units of `step`
// scale blocks (a 256-weight K-quant block; a fetch step of 8 blocks for the rest); rows, experts and the base are `align`-byte aligned
struct mmq_id_fam_desc { const char * name; int64_t gran, kmin; int step; size_t align; };
static const mmq_id_fam_desc MMQ_ID_FAMS[MMQ_ID_FAMILIES] = {
    { "mmq_id_kquant", 256,  0, 1,           1 },       // (the MFMA body's 16-byte row alignment is mmq_ok's: the route's condition)
    { "mmq_id_mxfp4",   32, 32, MMQ_ID_STEP, 1 },
    { "mmq_id_blocks",  32, 32, MMQ_ID_STEP, 2 },
};
int mmq_id_family(int type) {
    switch (type) {
        case GGML_TYPE_Q4_K: case GGML_TYPE_Q5_K: case GGML_TYPE_Q6_K: return MMQ_ID_KQUANT;
        case GGML_TYPE_MXFP4: return MMQ_ID_MXFP4;
        case GGML_TYPE_Q8_0: case GGML_TYPE_Q4_0: case GGML_TYPE_Q5_0: case GGML_TYPE_IQ4_NL: return MMQ_ID_BLOCKS;
        default: return -1;
    }
}
// bytes of a 32-weight block of the stepped body's types: the least row stride is K / 32 of them (K-quant rows: the route's condition)
static size_t mmq_id_block_bytes(int type) {
    switch (type) {
        case GGML_TYPE_MXFP4: return mxfp4_dec::BYTES;
        case GGML_TYPE_Q8_0:  return q80_dec::BYTES;
        case GGML_TYPE_Q4_0:  return q40_dec::BYTES;
        case GGML_TYPE_Q5_0:  return q50_dec::BYTES;
        case GGML_TYPE_IQ4_NL: return iq4nl_dec::BYTES;
        default: return 0;
    }
}

static mmq_id_stat g_mmq_id_stat[MMQ_ID_FAMILIES];                                     // launches so far, KS of the most recent one (0: none yet)
mmq_id_stat mmq_id_stats(int family) { return g_mmq_id_stat[family]; }

static size_t mmq_id_lds(int64_t nblk, int ks) { return 32 * sizeof(size_t) + (size_t) nblk * 32 * 4 + (size_t) (ks - 1) * 64 * 16 * 4; }
size_t mmq_id_lds_bytes(int type, int64_t K) { return mmq_id_lds(K / MMQ_ID_FAMS[mmq_id_family(type)].gran, 8); }      // at the widest fold (KS = 8)

template <class Body, bool NT4 = false>
static void mmq_id_go(const mmq_id_dev & d, const dim3 grid, const int ks, const size_t lds, hipStream_t st) {
    if (ks == 8)      k_mmq_id<Body, 8, NT4><<<grid, dim3(512), lds, st>>>(d);
    else if (ks == 4) k_mmq_id<Body, 4, NT4><<<grid, dim3(256), lds, st>>>(d);
    else if (ks == 2) k_mmq_id<Body, 2, NT4><<<grid, dim3(128), lds, st>>>(d);
    else              k_mmq_id<Body, 1, NT4><<<grid, dim3(64), lds, st>>>(d);
}

void mmq_id(const mmq_id_args & a, hipStream_t st) {
    const mmv_id_args & m = a.m;
    if (m.nrows == 0 || m.n_ids == 0 || m.n_tokens == 0) return;
    const int64_t n_pairs = m.n_ids * m.n_tokens;
    const int fam = mmq_id_family(m.type);
    const mmq_id_fam_desc & f = MMQ_ID_FAMS[fam < 0 ? 0 : fam];
    if (fam < 0 || m.K < f.kmin ||m.K % f.gran != 0 || m.K > INT32_MAX || mmq_id_lds_bytes(m.type, m.K) > MMQ_ID_LDS_MAX || n_pairs > MMQ_ID_MAX_PAIRS || m.n_expert < 1 ||
        m.n_expert > MMQ_ID_MAX_EXPERTS || m.b_ne1 < 1 || m.nrows > INT32_MAX || m.as_nb1 < (size_t) (m.K / 32) * mmq_id_block_bytes(m.type) || m.as_nb1 % f.align != 0 ||
        m.as_nb2 % f.align != 0 || ((uintptr_t) m.as & (f.align - 1)) != 0 || a.scratch_bytes < moe_group_bytes(n_pairs, m.n_expert)) {
        fprintf(stderr, "[mi355x] %s: shape / type / alignment / scratch out of range (type %d, K=%lld, ids %lld x %lld, %lld experts)\n", f.name, m.type, (long long) m.K,
                (long long) m.n_ids, (long long) m.n_tokens, (long long) m.n_expert); abort();
    }
    const int64_t bound = moe_tile_bound(n_pairs, m.n_expert);                          // <= 4096 + 2^15: inside grid y
    const moe_group_out g = moe_group_launch(m, a.scratch, st);

    mmq_id_dev d;
    d.as = (const char *) m.as; d.as_nb1 = m.as_nb1; d.as_nb2 = m.as_nb2;
    d.count = g.count; d.tiles = g.tiles; d.list = g.list;
    d.act = (const char *) m.act; d.b_ne1 = (int) m.b_ne1; d.n_ids = (int) m.n_ids;
    d.dst = (char *) m.dst; d.dst_nb1 = m.dst_nb1; d.dst_nb2 = m.dst_nb2;
    d.K = (int) m.K; d.nrows = (int) m.nrows; d.type = m.type;
    const int64_t row_tiles = (m.nrows + 31) / 32;
    const int nblk = (int) (m.K / f.gran), units = (nblk + f.step - 1) / f.step;
    // waves per tile: mmq_kquant's rule on the grid BOUND -- towards the chip's 2048 wave slots in one round, at least 4 units (K-quant blocks; fetch steps of 256
    // weights) per wave.  Host-known quantities only.
    int ks = 1;
    while (ks < 8 && row_tiles * bound * ks * 2 <= 3072 && ks * 4 <= units) ks *= 2;
    static const bool nt4 = getenv("MI355X_MMQ_ID_NT4") && atoi(getenv("MI355X_MMQ_ID_NT4")) != 0;
    const dim3 grid((unsigned) row_tiles, (unsigned) bound);
    const size_t lds = mmq_id_lds(nblk, ks);
    switch (m.type) {
        case GGML_TYPE_MXFP4:  mmq_id_go<mmq_id_stepped_body<mxfp4_dec>>(d, grid, ks, lds, st); break;
        case GGML_TYPE_Q8_0:   mmq_id_go<mmq_id_stepped_body<q80_dec>>(d, grid, ks, lds, st); break;
        case GGML_TYPE_Q4_0:   mmq_id_go<mmq_id_stepped_body<q40_dec>>(d, grid, ks, lds, st); break;
        case GGML_TYPE_Q5_0:   mmq_id_go<mmq_id_stepped_body<q50_dec>>(d, grid, ks, lds, st); break;
        case GGML_TYPE_IQ4_NL: mmq_id_go<mmq_id_stepped_body<iq4nl_dec>>(d, grid, ks, lds, st); break;
        default:               if (nt4) mmq_id_go<mmq_id_kquant_body, true>(d, grid, ks, lds, st); else mmq_id_go<mmq_id_kquant_body>(d, grid, ks, lds, st); break;
    }
    ++g_mmq_id_stat[fam].launches;
    g_mmq_id_stat[fam].ks = ks;
}

} // namespace mi
