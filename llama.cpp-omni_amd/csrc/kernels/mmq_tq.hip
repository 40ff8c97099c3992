// mmq_tq.hip -- MUL_MAT of ternary weights (TQ1_0 / TQ2_0: BitNet-b1.58, TriLM, Falcon-E files) against 9 .. 64 activation columns on the int8 matrix cores of gfx950.
//
// reference arithmetic: ggml_vec_dot_tq1_0_q8_K / ggml_vec_dot_tq2_0_q8_K (ggml-cpu/quants.c:335 / :387) on activations quantised by quantize_row_q8_K --
// per 256-weight block ONE integer sum and ONE float multiply:
//     sumi  = sum_e (x_e - 1) * y.qs[e]              x_e: the block's base-3 digit (TQ1_0, 0 .. 2) or 2-bit field (TQ2_0, 0 .. 3; 3 is the weight + 2)
//     out  += (float) sumi * (d_x * d_y)
// so the eight __builtin_amdgcn_mfma_i32_32x32x32_i8 of a block chain through ONE i32 accumulator (|sumi| <= 256 * 127 * 2) and the float epilogue -- what a block
// costs in the kernels of mmq_id.hip, where it runs once per 32 weights -- runs once per 256.  The integers are the reference's; only the f32 additions across blocks
// are re-associated.
//
// Work split.  One workgroup = one 32-row tile x one slice of at most 32 columns (grid x: row tiles, grid y: column slices); its KS waves take the K blocks
// wave, wave + KS, ... of the same rows and fold through LDS in wave order (mmq_dev.hpp mmq_fold).  KS comes from K and the row-tile count alone, never from the
// column count: a column's f32 summation order depends on the shape only, whatever stands in the other columns.
//
// Data movement.  Lane = (row lane & 31, K half hb = lane >> 5).  In the MFMA the activations are the A operand (lane & 31 = column of the slice), the weights the B
// operand (lane & 31 = row), and both carry, in MFMA k of a block, the sixteen K values 32 k + 16 hb .. + 15 of the block: the A operand is the sixteen image bytes at
// 256 ib + 32 k + 16 hb as they lie (from L2 at use), and the packing hands the lane exactly those weights out of 16-byte loads that stay inside its own row's block:
//     TQ2_0 {qs[64], d}         plane l (bits 2l, 2l + 1) of qs bytes 32 j + 16 hb .. + 15 is weights 128 j + 32 l + 16 hb .. + 15: MFMA k = 4 j + l.
//     TQ1_0 {qs[48], qh[4], d}  digit n of qs[16 hb .. + 15] is weights 32 n + 16 hb .. + 15: MFMA k = n (0 .. 4).  Digit n of qs[32 .. 47] is weights 160 + 16 n .. + 15:
//                               hb 0 takes digits 0, 2, 4 and hb 1 digits 1, 3 of those bytes in MFMAs 5, 6, 7; the last half operand (hb 1 of MFMA 7, weights 240 .. 255)
//                               is the four digits of the qh dword, one per operand dword.
// The block goes straight into VGPRs, the wave's next block requested before the current one is decoded; the - 1 is a bytewise subtract on the decoded digits.  LDS
// holds the columns' block scales d_y[ib][c] (as in k_mmq_id) and the fold area, nothing per column beyond that.
//
// Edges.  Rows past M: the load address is clamped, the store masked.  Columns past the slice: the lane reads the slice's first column, its scale is staged as 0 and the
// store masked.  K blocks uneven over KS: a wave simply has fewer (or no) blocks; every wave reaches the two barriers.
#include "mmq_dev.hpp"
#include "blocks_dev.hpp"

namespace mi {

typedef u32x4    __attribute__((aligned(2))) tq_u32x4a2;                  // (blocks are 54 / 66 bytes: rows and fields are 2-byte aligned, never better)
typedef uint32_t __attribute__((aligned(2))) tq_u32a2;

// x - 1 in every byte, x in 0 .. 3: the add cannot carry out of a byte (0x7f + 3 < 0x100), the xor turns 0x7f .. 0x82 into 0xff, 0x00, 0x01, 0x02
static __device__ __forceinline__ int tq_minus1(uint32_t x) { return (int) ((x + 0x7f7f7f7fu) ^ 0x80808080u); }

struct tq2_dec {
    static constexpr int BYTES = 66;
    struct blk { u32x4 q[2]; uint32_t dw; };
    static __device__ __forceinline__ blk load(const char * bp, int hb) {
        return { { *(const tq_u32x4a2 *) (bp + 16 * hb), *(const tq_u32x4a2 *) (bp + 32 + 16 * hb) }, (uint32_t) *(const uint16_t *) (bp + 64) };
    }
    static __device__ __forceinline__ void weights(const blk & x, int, i32x4 (&w)[8]) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int l = 0; l < 4; ++l)
#pragma unroll
                for (int e = 0; e < 4; ++e) w[4 * j + l][e] = tq_minus1((x.q[j][e] >> (2 * l)) & 0x03030303u);
    }
    static __device__ __forceinline__ float scale(const blk & x) { return h2f((uint16_t) x.dw); }
};

struct tq1_dec {
    static constexpr int BYTES = 54;
    struct blk { u32x4 q, t; uint32_t qh, dw; };                           // qs[16 hb .. + 15], qs[32 .. 47], qh, d
    static __device__ __forceinline__ blk load(const char * bp, int hb) {
        return { *(const tq_u32x4a2 *) (bp + 16 * hb), *(const tq_u32x4a2 *) (bp + 32), *(const tq_u32a2 *) (bp + 48), (uint32_t) *(const uint16_t *) (bp + 52) };
    }
    static __device__ __forceinline__ void weights(const blk & x, int hb, i32x4 (&w)[8]) {
        uint32_t pw = 1;
#pragma unroll
        for (int n = 0; n < 5; ++n) {
#pragma unroll
            for (int e = 0; e < 4; ++e) w[n][e] = tq_minus1(tq1_digits(x.q[e], pw));
            pw *= 3;
        }
        const uint32_t m5 = hb ? 3u : 1u, m6 = hb ? 27u : 9u;              // digits 0 / 1 and 2 / 3 of qs[32 .. 47]
        pw = 1;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            w[5][e] = tq_minus1(tq1_digits(x.t[e], m5));
            w[6][e] = tq_minus1(tq1_digits(x.t[e], m6));
            w[7][e] = tq_minus1(tq1_digits(hb ? x.qh : x.t[e], hb ? pw : 81u));      // digit 4 of qs[32 .. 47] / digit e of qh
            pw *= 3;
        }
    }
    static __device__ __forceinline__ float scale(const blk & x) { return h2f((uint16_t) x.dw); }
};

struct mmq_tq_dev {
    const char * W; size_t w_rs;
    const char * act; size_t act_cs;          // Q8_K images (q8k_image_bytes(K) each): [K int8][K/16 int16][K/256 f32]
    char * dst; size_t dst_cs;
    int K, nrows, ncols;
};

template <class Dec, int KS>      // KS: waves per workgroup splitting K
__global__ void __launch_bounds__(64 * KS) __attribute__((amdgpu_waves_per_eu(2))) k_mmq_tq(const mmq_tq_dev a) {
    extern __shared__ __attribute__((aligned(16))) char mmq_lds[];
    const int nblk = a.K >> 8;
    float * yd  = (float *) mmq_lds;                                     // [nblk][32] column scales of every block (transposed)
    float * red = yd + nblk * 32;                                        // [KS - 1][64][16] fold area

    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lq = lane & 31, hb = lane >> 5;
    const int row = (int) blockIdx.x * 32 + lq;
    const bool row_ok = row < a.nrows;
    const char * wrow = a.W + (size_t) (row_ok ? row : a.nrows - 1) * a.w_rs;
    const int c0 = (int) blockIdx.y * 32;
    const int ncols = a.ncols - c0 < 32 ? a.ncols - c0 : 32;             // (>= 1: grid y is the slice count)
    const char * acol = a.act + (size_t) (c0 + (lq < ncols ? lq : 0)) * a.act_cs + 16 * hb;

    float out[16];                                                       // register 4 g + i = column 8 g + 4 hb + i of this lane's row
#pragma unroll
    for (int i = 0; i < 16; ++i) out[i] = 0.0f;

    auto block = [&](int ib, const typename Dec::blk & G) {
        const char * ab = acol + (size_t) ib * 256;
        u32x4 av[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) av[k] = *(const u32x4 *) (ab + 32 * k);
        i32x4 w[8];
        Dec::weights(G, hb, w);
        i32x16 acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const i32x4 aa = i32x4{ (int) av[k][0], (int) av[k][1], (int) av[k][2], (int) av[k][3] };
            acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(aa, w[k], acc, 0, 0, 0);
        }
        const float dx = Dec::scale(G);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 y4 = *(const f32x4 *) (yd + ib * 32 + 8 * g + 4 * hb);
#pragma unroll
            for (int i = 0; i < 4; ++i) out[4 * g + i] += (float) acc[4 * g + i] * (dx * y4[i]);
        }
    };

    // this wave's blocks: wave, wave + KS, ...; two register sets, the next block in flight while the current one is decoded and multiplied
    const int nb_w = wave < nblk ? (nblk - wave + KS - 1) / KS : 0;
    typename Dec::blk R[2];
    if (nb_w > 0) R[0] = Dec::load(wrow + (size_t) wave * Dec::BYTES, hb);
    // column scales of all blocks -> LDS, transposed: yd[b][c], behind the first block's loads
    for (int i = threadIdx.x; i < nblk * 32; i += 64 * KS) {
        const int b = i >> 5, c = i & 31;
        yd[i] = c < ncols ? *(const float *) (a.act + (size_t) (c0 + c) * a.act_cs + a.K + (a.K >> 3) + 4 * b) : 0.0f;
    }
    __syncthreads();
    for (int i0 = 0; i0 < nb_w; i0 += 2) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int i = i0 + u;
            if (i < nb_w) {
                if (i + 1 < nb_w) R[u ^ 1] = Dec::load(wrow + (size_t) (wave + (i + 1) * KS) * Dec::BYTES, hb);
                block(wave + i * KS, R[u]);
            }
        }
    }

    if (!mmq_fold<4, KS>(red, out, wave, lane)) return;
    if (!row_ok) return;
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = 8 * g + 4 * hb + i;
            if (c < ncols) *(float *) (a.dst + (size_t) (c0 + c) * a.dst_cs + (size_t) row * 4) = out[4 * g + i];
        }
}

// ------------------------------------------------------------------------------------------------ host
static const size_t MMQ_TQ_LDS_MAX = 64 * 1024;                          // no launch attribute needed
static size_t mmq_tq_lds(int64_t nblk, int ks) { return (size_t) nblk * 32 * 4 + (size_t) (ks - 1) * 64 * 16 * 4; }
static int mmq_tq_block_bytes(int type) { return type == GGML_TYPE_TQ1_0 ? tq1_dec::BYTES : type == GGML_TYPE_TQ2_0 ? tq2_dec::BYTES : 0; }

bool mmq_tq_ok(int type, int64_t K, int64_t nrows, const void * W, size_t w_rs) {
    const int bs = mmq_tq_block_bytes(type);
    return bs && K >= 256 && K % 256 == 0 && K <= INT32_MAX && nrows >= 1 && nrows <= INT32_MAX && w_rs % 2 == 0 && ((uintptr_t) W & 1) == 0 &&
           w_rs >= (size_t) (K / 256) * bs && mmq_tq_lds(K / 256, 8) <= MMQ_TQ_LDS_MAX;
}

static mmq_tq_stat g_mmq_tq_stat;
mmq_tq_stat mmq_tq_stats() { return g_mmq_tq_stat; }

template <class Dec>
static void mmq_tq_go(const mmq_tq_dev & d, const dim3 grid, const int ks, const size_t lds, hipStream_t st) {
    if (ks == 8)      k_mmq_tq<Dec, 8><<<grid, dim3(512), lds, st>>>(d);
    else if (ks == 4) k_mmq_tq<Dec, 4><<<grid, dim3(256), lds, st>>>(d);
    else if (ks == 2) k_mmq_tq<Dec, 2><<<grid, dim3(128), lds, st>>>(d);
    else              k_mmq_tq<Dec, 1><<<grid, dim3(64), lds, st>>>(d);
}

void mmq_tq(const mmq_tq_args & a, hipStream_t st) {
    if (a.nrows == 0 || a.ncols == 0) return;
    if (!mmq_tq_ok(a.type, a.K, a.nrows, a.W, a.w_rs) || a.ncols < 1 || (a.ncols + 31) / 32 > 65535) {
        fprintf(stderr, "[mi355x] mmq_tq: shape / type / alignment out of range (type %d, K=%lld, %lld rows, %d columns)\n", a.type, (long long) a.K, (long long) a.nrows, a.ncols); abort();
    }
    mmq_tq_dev d;
    d.W = (const char *) a.W; d.w_rs = a.w_rs; d.act = (const char *) a.act; d.act_cs = a.act_cs; d.dst = (char *) a.dst; d.dst_cs = a.dst_cs;
    d.K = (int) a.K; d.nrows = (int) a.nrows; d.ncols = a.ncols;
    const int64_t row_tiles = (a.nrows + 31) / 32;
    const int nblk = (int) (a.K >> 8);
    // waves per tile: mmq_kquant's rule -- towards the chip's 2048 wave slots in one round, at least 2 blocks per wave.  From K and the row tiles only, never the
    // column count (a second column slice doubles the workgroups, not KS).
    int ks = 1;
    while (ks < 8 && row_tiles * ks * 2 <= 3072 && ks * 4 <= nblk) ks *= 2;
    const dim3 grid((unsigned) row_tiles, (unsigned) ((a.ncols + 31) / 32));
    const size_t lds = mmq_tq_lds(nblk, ks);
    if (a.type == GGML_TYPE_TQ1_0) mmq_tq_go<tq1_dec>(d, grid, ks, lds, st); else mmq_tq_go<tq2_dec>(d, grid, ks, lds, st);
    ++g_mmq_tq_stat.launches;
    g_mmq_tq_stat.ks = ks;
}

} // namespace mi
