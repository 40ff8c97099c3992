// mmq_id.hip -- MUL_MAT_ID on K-quant experts against MANY tokens (a prefill ubatch) on the int8 matrix cores of gfx950:
//     dst[:, i, t] = as[:, :, ids[i, t]] . b[:, i % b_ne1, t]          (ggml_compute_forward_mul_mat_id, ggml-cpu/ggml-cpu.c:1484 ff.)
// The per-pair mat-vec (mmvk.hip k_mmv_id) streams one expert matrix per (slot, token) pair: right for decode, but a 512-token ubatch of 8 used experts reads 4096
// matrices where 128 distinct ones exist.  Here the pairs are grouped by expert ON THE DEVICE and every (expert, 32-row tile, <= 32-column slice) is one workgroup of
// mmq.hip's body (mmq_dev.hpp): the same vec_dot_q*_K_q8_K integers, a weight block read once per 32 columns instead of once per column.
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
// branches uniformly into the templated bodies (MI355X_MMQ_ID_NT4=1 keeps every tile on the four-group body: the measurement switch of tools/moe_mmq_bench.py).
#include "mmq_dev.hpp"

namespace mi {

// (moe_tile, one entry of the tile table, and moe_group_out, where a grouping lies in the scratch: kernels.hpp -- mmq_id_mxfp4.hip reads the same tables)
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

// one (expert, 32-row tile, column slice) at NT column groups: mmq_dev.hpp's blocks and fold, the store through the slice's dst offsets
template <int NT, int KS, typename Stage>
static __device__ __forceinline__ void mmq_id_tile(const mmq_id_dev & a, const char * wrow, const char * acol, const int row, const bool row_ok, const int ncols,
                                                   const float * yd, float * red, const size_t * dcol, Stage stage_scales) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hb = lane >> 5;
    float out[NT * 4];
#pragma unroll
    for (int i = 0; i < NT * 4; ++i) out[i] = 0.0f;
    mmq_blocks<NT, KS>(a.type, wrow, acol, a.K >> 8, wave, hb, yd, out, stage_scales);
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

template <int KS, bool NT4>      // KS: waves per workgroup splitting K; NT4: every tile on the four-group body
__global__ void __launch_bounds__(64 * KS) __attribute__((amdgpu_waves_per_eu(2))) k_mmq_id(const mmq_id_dev a) {
    extern __shared__ __attribute__((aligned(16))) char mmq_lds[];
    if ((int) blockIdx.y >= *a.count) return;                            // (workgroup-uniform: the grid is the host's bound on the tile count)
    const moe_tile tl = a.tiles[blockIdx.y];
    const int nblk = a.K >> 8;
    size_t * dcol = (size_t *) mmq_lds;                                  // [32] dst offset of every column of the slice
    float * yd  = (float *) (dcol + 32);                                 // [nblk][32] column scales of every block (transposed)
    float * red = yd + nblk * 32;                                        // [KS - 1][64][16] fold area

    const int lane = threadIdx.x & 63, lq = lane & 31;
    const int row = (int) blockIdx.x * 32 + lq;
    const bool row_ok = row < a.nrows;
    const char * wrow = a.as + (size_t) tl.expert * a.as_nb2 + (size_t) (row_ok ? row : a.nrows - 1) * a.as_nb1;

    // ---- this lane's column: pair p = t * n_ids + i of the list -> image t * b_ne1 + i % b_ne1 (lanes past the slice carry its first column's bytes)
    const bool tok_ok = lq < tl.ncols;
    const int p = a.list[tl.first + (tok_ok ? lq : 0)];
    const int t = p / a.n_ids, i = p - t * a.n_ids;
    const char * acol = a.act + (size_t) (t * a.b_ne1 + i % a.b_ne1) * q8k_image_bytes(a.K);
    if (threadIdx.x < 32 && tok_ok) dcol[lq] = (size_t) i * a.dst_nb1 + (size_t) t * a.dst_nb2;

    // ---- column scales of all blocks -> LDS, transposed: yd[b][c]; the stride is a multiple of 32, so every thread stages its own column lq.  The barrier also
    //      publishes dcol.  (called after the first block's loads are in flight)
    const int K = a.K;
    auto stage_scales = [&]() {
        for (int j = threadIdx.x; j < nblk * 32; j += 64 * KS) yd[j] = tok_ok ? *(const float *) (acol + K + (K >> 3) + 4 * (j >> 5)) : 0.0f;
        __syncthreads();
    };
    const int nt = NT4 ? 4 : (tl.ncols + 7) >> 3;
    if (nt == 1)      mmq_id_tile<1, KS>(a, wrow, acol, row, row_ok, tl.ncols, yd, red, dcol, stage_scales);
    else if (nt == 2) mmq_id_tile<2, KS>(a, wrow, acol, row, row_ok, tl.ncols, yd, red, dcol, stage_scales);
    else if (nt == 3) mmq_id_tile<3, KS>(a, wrow, acol, row, row_ok, tl.ncols, yd, red, dcol, stage_scales);
    else              mmq_id_tile<4, KS>(a, wrow, acol, row, row_ok, tl.ncols, yd, red, dcol, stage_scales);
}

static long g_mmq_id_launches = 0;
long mmq_id_launches() { return g_mmq_id_launches; }
static int g_mmq_id_ks = 0;                                                            // KS of the most recent launch (0: none yet)
int mmq_id_last_ks() { return g_mmq_id_ks; }

size_t mmq_id_lds_bytes(int64_t K) { return 32 * sizeof(size_t) + (size_t) (K >> 8) * 32 * 4 + (size_t) 7 * 64 * 16 * 4; }      // at the widest fold (KS = 8)

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

void mmq_id_kquant(const mmq_id_args & a, hipStream_t st) {
    const mmv_id_args & m = a.m;
    if (m.nrows == 0 || m.n_ids == 0 || m.n_tokens == 0) return;
    const int64_t n_pairs = m.n_ids * m.n_tokens;
    if (m.K % 256 != 0 || m.K > INT32_MAX || mmq_id_lds_bytes(m.K) > MMQ_ID_LDS_MAX || n_pairs > MMQ_ID_MAX_PAIRS || m.n_expert < 1 || m.n_expert > MMQ_ID_MAX_EXPERTS || m.b_ne1 < 1 ||
        m.nrows > INT32_MAX || (m.type != GGML_TYPE_Q4_K && m.type != GGML_TYPE_Q5_K && m.type != GGML_TYPE_Q6_K) || a.scratch_bytes < moe_group_bytes(n_pairs, m.n_expert)) {
        fprintf(stderr, "[mi355x] mmq_id_kquant: shape / type / scratch out of range (type %d, K=%lld, ids %lld x %lld, %lld experts)\n", m.type, (long long) m.K, (long long) m.n_ids,
                (long long) m.n_tokens, (long long) m.n_expert); abort();
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
    const int nblk = (int) (m.K >> 8);
    // waves per tile: mmq_kquant's rule on the grid BOUND -- towards the chip's 2048 wave slots in one round, at least 4 K blocks per wave.  Host-known quantities only.
    int ks = 1;
    while (ks < 8 && row_tiles * bound * ks * 2 <= 3072 && ks * 4 <= nblk) ks *= 2;
    static const bool nt4 = getenv("MI355X_MMQ_ID_NT4") && atoi(getenv("MI355X_MMQ_ID_NT4")) != 0;
    const dim3 grid((unsigned) row_tiles, (unsigned) bound);
    const size_t lds = 32 * sizeof(size_t) + (size_t) nblk * 32 * 4 + (size_t) (ks - 1) * 64 * 16 * 4;
#define MMQ_ID_GO(KSS) do { if (nt4) k_mmq_id<KSS, true><<<grid, dim3(64 * KSS), lds, st>>>(d); else k_mmq_id<KSS, false><<<grid, dim3(64 * KSS), lds, st>>>(d); } while (0)
    if (ks == 8) MMQ_ID_GO(8); else if (ks == 4) MMQ_ID_GO(4); else if (ks == 2) MMQ_ID_GO(2); else MMQ_ID_GO(1);
#undef MMQ_ID_GO
    ++g_mmq_id_launches;
    g_mmq_id_ks = ks;
}

} // namespace mi
