// mmq_id_mxfp4.hip -- MUL_MAT_ID on MXFP4 experts (gpt-oss) against MANY tokens (a prefill ubatch) on the int8 matrix cores of gfx950:
//     dst[:, i, t] = as[:, :, ids[i, t]] . b[:, i % b_ne1, t]          (ggml_compute_forward_mul_mat_id, ggml-cpu/ggml-cpu.c:1484 ff.)
// The per-pair mat-vec (mmv_mxfp4.hip) streams one expert matrix per (slot, token) pair: a 512-token ubatch of gpt-oss-20b reads 2048 matrices where 32 distinct ones
// exist.  Here the pairs are grouped by expert on the device (mmq_id.hip k_moe_group, the launch the K-quant experts use: moe_group_launch) and every (expert, 32-row
// tile, <= 32-column slice) is one workgroup, as k_mmq_id -- with a body for 17-byte blocks of 32 weights {uint8 e; uint8 qs[16]} against the Q8_0 images
// (common.hpp q80_image_bytes: qs[K] | f32 d[K / 32]).
//
// Arithmetic: ggml_vec_dot_mxfp4_q8_0 (ggml-cpu/quants.c:188-215), in the product order of the per-pair kernel:
//     sumi    = sum_j y.qs[j] * kv[x.qs[j] & 0xF] + y.qs[j + 16] * kv[x.qs[j] >> 4]
//     out[c] += (float) sumi * (d_y[ib][c] * e8m0_half(x.e))
// One wave = 32 weight rows (lane & 31) x the slice's columns.  hb = lane >> 5 is the K half of __builtin_amdgcn_mfma_i32_32x32x32_i8: weight j of a block is the low
// nibble of qs[j], weight j + 16 the high one, so half hb takes the low (0) or high (1) nibbles of all 16 quant bytes -- four mxfp4_lut4 -- against the 16 activation
// bytes 32 ib + 16 hb of the lane's column.  ONE MFMA per block is the reference's sumi for 32 rows x 32 columns; register 4 g + i = column 8 g + 4 hb + i of the
// lane's row (the layout of mmq_dev.hpp).  The float epilogue per block is NT * 4 registers wide (NT = 1..4 column groups of 8 in use, known on the device only: the
// workgroup branches uniformly into the templated bodies): it, not the MFMA, is what a block costs.
//
// A lane fetches STEP = 8 consecutive blocks of its row at a time (136 contiguous bytes: the 256 weights of a K-quant block), the next step's weights and activations
// requested before the current one is consumed.  The 16 quant bytes of a block sit at row + 17 ib + 1, at any alignment: one 1-byte-aligned 16-byte load that never
// leaves the block (as mmv_mxfp4.hip's 8-byte one).  gpt-oss rows are 90 blocks: the last step is ragged -- block indices are clamped for the loads, and a block past
// the row (the index is wave-uniform) contributes nothing.  The KS waves of a workgroup take the steps wave, wave + KS, ...; the fold goes through LDS in wave order
// (mmq_fold).  KS is chosen from K, the row tiles and the grid bound only -- never from the ids -- so a column's f32 summation order depends on the shape alone: results
// are bit-reproducible and independent of the other pairs in the tile.  Nothing on the host depends on the ids: a captured graph follows the ids of every replay.
#include "mmq_dev.hpp"
#include "mxfp4_dev.hpp"

namespace mi {

struct mmq_id_mx_dev {
    const char * as; size_t as_nb1, as_nb2;
    const int * count; const moe_tile * tiles; const int * list;
    const char * act; int b_ne1, n_ids;
    char * dst; size_t dst_nb1, dst_nb2;
    int K, nrows;
};

static constexpr int MX_STEP = 8, MX_BYTES = 17;                          // blocks per fetch step, bytes per block

// one (expert, 32-row tile, column slice) at NT column groups
template <int NT, int KS, typename Stage>
static __device__ __forceinline__ void mmq_id_mx_tile(const mmq_id_mx_dev & a, const char * wrow, const char * acol, const int row, const bool row_ok, const int ncols,
                                                      const float * yd, float * red, const size_t * dcol, Stage stage_scales) {
    typedef u32x4 __attribute__((aligned(1))) u32x4a1;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), hb = lane >> 5;
    const int nblk = a.K >> 5, nstep = (nblk + MX_STEP - 1) / MX_STEP;
    const int sh = 4 * hb;
    const char * arow = acol + 16 * hb;
    float out[NT * 4];
#pragma unroll
    for (int i = 0; i < NT * 4; ++i) out[i] = 0.0f;

    struct stp { u32x4 q[MX_STEP]; uint32_t e[MX_STEP]; u32x4 av[MX_STEP]; };      // one step of this lane's row, and of its column (its 16 bytes of every block)
    auto fetch = [&](int s, stp & G) {
#pragma unroll
        for (int u = 0; u < MX_STEP; ++u) {
            int ib = s * MX_STEP + u; ib = ib < nblk ? ib : nblk - 1;                // clamped, not branched around: a block past the row re-reads the last one
            const char * bp = wrow + (size_t) ib * MX_BYTES;
            G.e[u]  = *(const uint8_t *) bp;
            G.q[u]  = *(const u32x4a1 *) (bp + 1);
            G.av[u] = *(const u32x4 *) (arow + (size_t) ib * 32);
        }
    };
    auto reduce = [&](int s, const stp & G) {
#pragma unroll
        for (int u = 0; u < MX_STEP; ++u) {
            const int ib = s * MX_STEP + u;                                          // (wave-uniform)
            if (ib < nblk) {
                i32x4 wv, aa;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    wv[e] = (int) mxfp4_lut4((G.q[u][e] >> sh) & 0x0f0f0f0fu);
                    aa[e] = (int) G.av[u][e];                          // (lanes past the slice's columns carry another column's bytes: their outputs are never stored)
                }
                i32x16 z;
#pragma unroll
                for (int e = 0; e < 16; ++e) z[e] = 0;
                const i32x16 sj = __builtin_amdgcn_mfma_i32_32x32x32_i8(aa, wv, z, 0, 0, 0);
                const float eh = e8m0_half(G.e[u]);
#pragma unroll
                for (int g = 0; g < NT; ++g) {
                    const f32x4 y4 = *(const f32x4 *) (yd + ib * 32 + 8 * g + 4 * hb);
#pragma unroll
                    for (int i = 0; i < 4; ++i) out[4 * g + i] += (float) sj[4 * g + i] * (y4[i] * eh);
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

template <int KS>                // KS: waves per workgroup splitting K
__global__ void __launch_bounds__(64 * KS) __attribute__((amdgpu_waves_per_eu(2))) k_mmq_id_mxfp4(const mmq_id_mx_dev a) {
    extern __shared__ __attribute__((aligned(16))) char mmq_mx_lds[];
    if ((int) blockIdx.y >= *a.count) return;                            // (workgroup-uniform: the grid is the host's bound on the tile count)
    const moe_tile tl = a.tiles[blockIdx.y];
    const int nblk = a.K >> 5;
    size_t * dcol = (size_t *) mmq_mx_lds;                               // [32] dst offset of every column of the slice
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
    if (nt == 1)      mmq_id_mx_tile<1, KS>(a, wrow, acol, row, row_ok, tl.ncols, yd, red, dcol, stage_scales);
    else if (nt == 2) mmq_id_mx_tile<2, KS>(a, wrow, acol, row, row_ok, tl.ncols, yd, red, dcol, stage_scales);
    else if (nt == 3) mmq_id_mx_tile<3, KS>(a, wrow, acol, row, row_ok, tl.ncols, yd, red, dcol, stage_scales);
    else              mmq_id_mx_tile<4, KS>(a, wrow, acol, row, row_ok, tl.ncols, yd, red, dcol, stage_scales);
}

static long g_mmq_id_mxfp4_launches = 0;
long mmq_id_mxfp4_launches() { return g_mmq_id_mxfp4_launches; }
static int g_mmq_id_mxfp4_ks = 0;                                                      // KS of the most recent launch (0: none yet)
int mmq_id_mxfp4_last_ks() { return g_mmq_id_mxfp4_ks; }

size_t mmq_id_mxfp4_lds_bytes(int64_t K) { return 32 * sizeof(size_t) + (size_t) (K >> 5) * 32 * 4 + (size_t) 7 * 64 * 16 * 4; }      // at the widest fold (KS = 8)

void mmq_id_mxfp4(const mmq_id_args & a, hipStream_t st) {
    const mmv_id_args & m = a.m;
    if (m.nrows == 0 || m.n_ids == 0 || m.n_tokens == 0) return;
    const int64_t n_pairs = m.n_ids * m.n_tokens;
    if (m.type != GGML_TYPE_MXFP4 || m.K < 32 || m.K % 32 != 0 || m.K > INT32_MAX || mmq_id_mxfp4_lds_bytes(m.K) > MMQ_ID_LDS_MAX || n_pairs > MMQ_ID_MAX_PAIRS || m.n_expert < 1 ||
        m.n_expert > MMQ_ID_MAX_EXPERTS || m.b_ne1 < 1 || m.nrows > INT32_MAX || m.as_nb1 < (size_t) (m.K / 32) * 17 || a.scratch_bytes < moe_group_bytes(n_pairs, m.n_expert)) {
        fprintf(stderr, "[mi355x] mmq_id_mxfp4: shape / type / scratch out of range (type %d, K=%lld, ids %lld x %lld, %lld experts)\n", m.type, (long long) m.K, (long long) m.n_ids,
                (long long) m.n_tokens, (long long) m.n_expert); abort();
    }
    const int64_t bound = moe_tile_bound(n_pairs, m.n_expert);                          // <= 4096 + 2^15: inside grid y
    const moe_group_out g = moe_group_launch(m, a.scratch, st);

    mmq_id_mx_dev d;
    d.as = (const char *) m.as; d.as_nb1 = m.as_nb1; d.as_nb2 = m.as_nb2;
    d.count = g.count; d.tiles = g.tiles; d.list = g.list;
    d.act = (const char *) m.act; d.b_ne1 = (int) m.b_ne1; d.n_ids = (int) m.n_ids;
    d.dst = (char *) m.dst; d.dst_nb1 = m.dst_nb1; d.dst_nb2 = m.dst_nb2;
    d.K = (int) m.K; d.nrows = (int) m.nrows;
    const int64_t row_tiles = (m.nrows + 31) / 32;
    const int nblk = (int) (m.K >> 5), nstep = (nblk + MX_STEP - 1) / MX_STEP;
    // waves per tile: mmq_id_kquant's rule on the grid BOUND, a fetch step (256 weights) for a K-quant block -- towards the chip's 2048 wave slots in one round, at
    // least 4 steps per wave.  Host-known quantities only.
    int ks = 1;
    while (ks < 8 && row_tiles * bound * ks * 2 <= 3072 && ks * 4 <= nstep) ks *= 2;
    const dim3 grid((unsigned) row_tiles, (unsigned) bound);
    const size_t lds = 32 * sizeof(size_t) + (size_t) nblk * 32 * 4 + (size_t) (ks - 1) * 64 * 16 * 4;
    if (ks == 8)      k_mmq_id_mxfp4<8><<<grid, dim3(512), lds, st>>>(d);
    else if (ks == 4) k_mmq_id_mxfp4<4><<<grid, dim3(256), lds, st>>>(d);
    else if (ks == 2) k_mmq_id_mxfp4<2><<<grid, dim3(128), lds, st>>>(d);
    else              k_mmq_id_mxfp4<1><<<grid, dim3(64), lds, st>>>(d);
    ++g_mmq_id_mxfp4_launches;
    g_mmq_id_mxfp4_ks = ks;
}

} // namespace mi
