// mmq.hip -- MUL_MAT of K-quant weights against a FEW activation columns (2 .. 64 tokens: several sequences decoded together,
// speculative drafts, small ubatches) on the int8 matrix cores of gfx950.
//
// reference arithmetic: ggml_vec_dot_q4_K_q8_K / ggml_vec_dot_q6_K_q8_K (ggml-cpu/quants.c:550-623, 705-758) on activations quantised by
// quantize_row_q8_K (ggml-quants.c:2555-2592): per 256-block
//     Q4_K:  d*yd * sum_j sc_j * (q4 . q8)_j  -  dmin*yd * sum_j m_j * bsum_j          (8 sub-blocks of 32)
//     Q6_K:  d*yd * sum_s sc_s * ((q6 - 32) . q8)_s                                    (16 sub-blocks of 16)
// The integer sums are exact (the same integers as the reference); only the f32 accumulation across blocks is re-associated, exactly as
// in the mat-vec kernels (mmvk.hip).  The dot4 mat-vec spends one VALU op per 4 weights PER COLUMN, so at 8+ columns it is
// compute-bound long before HBM; here the sub-block dot products of 32 weight rows x 32 tokens are ONE MFMA:
//     tokens are the M side (A operand, int8 activations from the Q8_K image), weight rows the N side (B operand, unpacked nibbles),
//     so a lane owns ONE weight row (lane % 32) and 16 tokens (its accumulator registers): the per-(row, sub-block) scale is a
//     lane-uniform multiplier (v_mad_i32_i24 on the int32 tile) and the per-(token, block) scale is applied once per block.
//     Q4_K mins:  sum_j m_j * bsum_j == sum_k m_{j(k)} * q8_k  -- a second MFMA per sub-block whose B operand is m_j replicated,
//                 accumulated over the block by the matrix core itself (no bsums needed).
//     Q6_K -32 :  sum_s sc_s * 32 * sum_{k in s} q8_k          -- likewise an MFMA with B = sc_s replicated; the weights go in unsigned.
// One wave = 32 weight rows x the token tile; the KS waves of a workgroup split the K blocks of the SAME rows and fold through LDS, so
// that small matrices (wk: 1024 rows) still put thousands of waves on the chip.  Weights stream straight from HBM into registers, one
// block ahead; activations (a few hundred KB, L2-resident) are read per sub-block.
// The block bodies (fetch / reduce per K block, the KS fold) live in mmq_dev.hpp: the expert-grouped MUL_MAT_ID kernel (mmq_id.hip) runs the same ones.
#include "mmq_dev.hpp"

namespace mi {

struct mmq_mat_dev { const char * W; size_t w_rs; float * dst; size_t dst_cs; const char * resid; size_t resid_cs; int nrows; int type; int tile_end; };
struct mmq_dev {
    mmq_mat_dev m[3]; int nmat;
    const char * act; size_t act_cs;          // Q8_K images (q8k_image_bytes(K) each): [K int8][K/16 int16][K/256 f32]
    int K, ncols;
};

template <int NT, int KS>      // NT: token groups of 8 in use (1..4), KS: waves per workgroup splitting K
__global__ void __launch_bounds__(64 * KS) __attribute__((amdgpu_waves_per_eu(2))) k_mmq_kquant(const mmq_dev a) {
    extern __shared__ __attribute__((aligned(16))) char mmq_lds[];
    const int nblk = a.K >> 8;
    float * yd  = (float *) mmq_lds;                       // [nblk][32] token scales of every block (transposed)
    float * red = yd + nblk * 32;                          // [KS - 1][64][NT * 4] fold area

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lq = lane & 31, hb = lane >> 5;
    // ---- which matrix / which 32-row tile
    int tile = (int) blockIdx.x, mi = 0;
#pragma unroll
    for (int i = 0; i < 2; ++i) if (i + 1 < a.nmat && (int) blockIdx.x >= a.m[i].tile_end) { mi = i + 1; tile = (int) blockIdx.x - a.m[i].tile_end; }
    const mmq_mat_dev M = mi == 0 ? a.m[0] : (mi == 1 ? a.m[1] : a.m[2]);
    const int row = tile * 32 + lq;
    const bool row_ok = row < M.nrows;
    const char * wrow = M.W + (size_t) (row_ok ? row : M.nrows - 1) * M.w_rs;

    // ---- token scales of all blocks -> LDS, transposed: yd[b][t]  (called after the first block's loads are in flight)
    auto stage_scales = [&]() {
        for (int i = threadIdx.x; i < nblk * 32; i += 64 * KS) {
            const int b = i >> 5, t = i & 31;
            yd[i] = t < a.ncols ? *(const float *) (a.act + (size_t) t * a.act_cs + a.K + (a.K >> 3) + 4 * b) : 0.0f;
        }
        __syncthreads();
    };

    const bool tok_ok = lq < a.ncols;                                    // A-operand role: lane = token lq  (lanes past ncols carry token 0's bytes)
    const char * acol = a.act + (size_t) (tok_ok ? lq : 0) * a.act_cs;

    float out[NT * 4];
#pragma unroll
    for (int i = 0; i < NT * 4; ++i) out[i] = 0.0f;

    mmq_blocks<NT, KS>(M.type, wrow, acol, nblk, wave, hb, yd, out, stage_scales);

    // ---- fold the KS waves' partial sums (same lane layout), store: lane = row, registers = tokens (reg&3) + 8*(reg>>2) + 4*hb
    if (!mmq_fold<NT, KS>(red, out, wave, lane)) return;
    if (!row_ok) return;
#pragma unroll
    for (int g = 0; g < NT; ++g)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int t = 8 * g + 4 * hb + i;
            if (t >= a.ncols) continue;
            float v = out[4 * g + i];
            if (M.resid) v += *(const float *) (M.resid + (size_t) t * M.resid_cs + (size_t) row * 4);        // residual ADD epilogue
            *(float *) ((char *) M.dst + (size_t) t * M.dst_cs + (size_t) row * 4) = v;
        }
}

bool mmq_ok(int type, int64_t K, const void * W, size_t w_rs) {
    if (type == GGML_TYPE_Q4_K || type == GGML_TYPE_Q5_K) return K % 256 == 0 && w_rs % 16 == 0 && ((uintptr_t) W & 15) == 0;
    if (type == GGML_TYPE_Q6_K) return K % 256 == 0 && w_rs % 2 == 0 && ((uintptr_t) W & 1) == 0;
    return false;
}

template <int NT, int KS>
static void mmq_launch(const mmq_dev & d, int ntiles, hipStream_t st) {
    const size_t lds = (size_t) (d.K >> 8) * 32 * 4 + (size_t) (KS > 1 ? (KS - 1) * 64 * NT * 4 * 4 : 0);
    k_mmq_kquant<NT, KS><<<dim3((unsigned) ntiles), dim3(64 * KS), lds, st>>>(d);
}

// up to 3 matrices sharing the activation images, at most 32 columns per call (the caller walks wider batches in chunks)
void mmq_kquant(const mmq_args & a, hipStream_t st) {
    if (a.ncols < 1 || a.ncols > 32 || a.nmat < 1 || a.nmat > 3) { fprintf(stderr, "[mi355x] mmq_kquant: bad shape\n"); abort(); }
    mmq_dev d;
    d.nmat = a.nmat; d.act = (const char *) a.act; d.act_cs = a.act_cs; d.K = (int) a.K; d.ncols = a.ncols;
    int acc = 0;
    for (int i = 0; i < 3; ++i) {
        const mmq_mat & s = a.m[i < a.nmat ? i : 0];
        d.m[i] = { (const char *) s.W, s.w_rs, s.dst, s.dst_cs, (const char *) s.resid, s.resid_cs, (int) s.nrows, s.type, 0 };
        if (i < a.nmat) acc += (int) ((s.nrows + 31) / 32);
        d.m[i].tile_end = acc;
    }
    const int nblk = (int) (a.K >> 8);
    // waves per 32-row tile: towards the chip's 2048 wave slots (two per SIMD) in one round, at least 4 K blocks per wave
    int ks = 1;
    while (ks < 8 && acc * ks * 2 <= 3072 && ks * 4 <= nblk) ks *= 2;
    const int nt = (a.ncols + 7) / 8;
#define MMQ_GO(NTT) do { if (ks == 8) mmq_launch<NTT, 8>(d, acc, st); else if (ks == 4) mmq_launch<NTT, 4>(d, acc, st); else if (ks == 2) mmq_launch<NTT, 2>(d, acc, st); else mmq_launch<NTT, 1>(d, acc, st); } while (0)
    switch (nt) { case 1: MMQ_GO(1); break; case 2: MMQ_GO(2); break; case 3: MMQ_GO(3); break; default: MMQ_GO(4); break; }
#undef MMQ_GO
}

} // namespace mi
