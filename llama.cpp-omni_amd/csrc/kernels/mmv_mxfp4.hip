// mmv_mxfp4.hip -- MUL_MAT_ID on MXFP4 experts (gpt-oss): dst[:, i, t] = as[:, :, ids[i, t]] . b[:, i % b_ne1, t]   (gfx950, wave64)
//
// reference: ggml_compute_forward_mul_mat_id (ggml-cpu/ggml-cpu.c:1484 ff.) with ggml_vec_dot_mxfp4_q8_0 (ggml-cpu/quants.c:188-215; x86 arch/x86/quants.c:760 ff.):
//     sumi  = sum_j y.qs[j] * kv[x.qs[j] & 0xF] + y.qs[j + 16] * kv[x.qs[j] >> 4]        kv = kvalues_mxfp4 (ggml-common.h:1094)
//     sumf += sumi * (d_y * e8m0_half(x.e))                                                e8m0_half = ggml_e8m0_to_fp32_half (ggml-impl.h:471-489)
// An MXFP4 block is {uint8 e; uint8 qs[16]}: 32 weights in 17 bytes, aligned to nothing -- an IQ4_NL block with another 16-entry int8 table and a power-of-two
// scale, against the same Q8_0 activation image (common.hpp q80_image_bytes: qs[K] | f32 d[K / 32]).
//
// The launch has the shape of k_mmv_id (mmvk.hip): grid x = row workgroups, y = slot i, z = token t.  Every workgroup reads its ONE id from device memory (a
// captured graph follows the ids of each replay), clamps it into [0, n_expert) before it becomes an address (the reference asserts), stages that column's
// image in LDS and streams the expert's rows.  The row loop is the frame of the 32-weight nibble forms (mmvq.hip k_mmv_blocks at one column, two rows per
// wave): two lanes per block, lane half hf owns qs bytes 8hf .. 8hf+7 = weights 8hf..8hf+7 (low nibbles) and 16+8hf..23+8hf (high); 32 blocks per wave step,
// U steps per stage, the next stage requested before the current one is consumed; block index and row are clamped instead of branching around a load, the
// contribution of an out-of-range lane is zeroed when it is consumed.
//
// The lane's 8 quant bytes sit at row + 17 ib + 1 + 8 hf: every alignment 0..7 occurs.  They are read with ONE 1-byte-aligned 8-byte load (gfx950 takes
// unaligned global loads in hardware: global_load_dwordx2 ... offset:1, no byte ladder); the load never leaves the block, so nothing is read outside the tensor.
#include "mxfp4_dev.hpp"

namespace mi {

extern __shared__ __attribute__((aligned(16))) char mx_lds[];

// (mxfp4_lut4, the table look-up of four nibbles, and e8m0_half, half the block scale: mxfp4_dev.hpp -- shared with the grouped kernel, mmq_id.hip)

struct mx_id_dev {
    const char * as; size_t as_nb1, as_nb2; int n_expert;
    const char * ids; size_t ids_nb0, ids_nb1;
    const char * act; int b_ne1;
    char * dst; size_t dst_nb1, dst_nb2;
    int K, nrows;
};

template <int U>
__global__ void __launch_bounds__(256) k_mmv_id_mxfp4(const mx_id_dev a) {
    constexpr int ROWS = 2, BPS = 32, BYTES = 17;                          // rows per wave, blocks per wave step, bytes per block
    typedef u32x2 __attribute__((aligned(1))) u32x2a1;
    const int i = blockIdx.y, t = blockIdx.z;
    int id = *(const int *) (a.ids + (size_t) i * a.ids_nb0 + (size_t) t * a.ids_nb1);
    id = id < 0 ? 0 : (id >= a.n_expert ? a.n_expert - 1 : id);
    id = __builtin_amdgcn_readfirstlane(id);
    const char * W   = a.as + (size_t) id * a.as_nb2;
    const size_t img = q80_image_bytes(a.K);
    const char * act = a.act + (size_t) (t * a.b_ne1 + i % a.b_ne1) * img;
    char * dst       = a.dst + (size_t) i * a.dst_nb1 + (size_t) t * a.dst_nb2;

    const int lane = threadIdx.x & 63;
    const int g = lane >> 1, hf = lane & 1;
    const int K = a.K, nrows = a.nrows;
    const int nb  = K >> 5;
    const int nit = (nb + BPS * U - 1) / (BPS * U);
    const int wave   = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    const int nwaves = gridDim.x * 4;
    const int ngrp   = (nrows + ROWS - 1) / ROWS;

    struct regs { u32x2 q; uint32_t e; };
    regs q[U][ROWS];
    auto issue = [&](int grp, int it) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int ib = (it * U + u) * BPS + g; ib = ib < nb ? ib : nb - 1;
#pragma unroll
            for (int r = 0; r < ROWS; ++r) {
                int row = grp * ROWS + r; row = row < nrows ? row : nrows - 1;
                const char * bp = W + (size_t) row * a.as_nb1 + (size_t) ib * BYTES;
                q[u][r].e = *(const uint8_t *) bp;
                q[u][r].q = *(const u32x2a1 *) (bp + 1 + 8 * hf);
            }
        }
    };
    // the first stage is requested before the activation image is staged; every wave reaches the barrier before any returns
    int grp = wave, it = 0;
    if (grp < ngrp) issue(grp, 0);
    {
        const int n16 = (int) (img >> 4);
        const u32x4 * s = (const u32x4 *) act;
        u32x4 *       d = (u32x4 *) mx_lds;
        for (int k = threadIdx.x; k < n16; k += 256) d[k] = s[k];
    }
    __syncthreads();
    if (grp >= ngrp) return;

    float acc[ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) acc[r] = 0.0f;
    while (true) {
        regs cq[U][ROWS];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int r = 0; r < ROWS; ++r) cq[u][r] = q[u][r];
        const int cgrp = grp, cit = it;
        ++it;
        if (it == nit) { it = 0; grp += nwaves; }
        const bool more = grp < ngrp;
        if (more) issue(grp, it);

#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int  ib    = (cit * U + u) * BPS + g;
            const bool valid = ib < nb;
            const int  ibc   = valid ? ib : nb - 1;
            const u32x2 a0 = *(const u32x2 *) (mx_lds + ibc * 32 + 8 * hf);              // the activations under the lane's low and high nibbles
            const u32x2 a1 = *(const u32x2 *) (mx_lds + ibc * 32 + 16 + 8 * hf);
            const float yd = *(const float *) (mx_lds + K + ibc * 4);
#pragma unroll
            for (int r = 0; r < ROWS; ++r) {
                const u32x2 x = cq[u][r].q;
                const uint32_t l0 = mxfp4_lut4(x[0] & 0x0f0f0f0fu), l1 = mxfp4_lut4(x[1] & 0x0f0f0f0fu);
                const uint32_t h0 = mxfp4_lut4((x[0] >> 4) & 0x0f0f0f0fu), h1 = mxfp4_lut4((x[1] >> 4) & 0x0f0f0f0fu);
                const int sumi = dot4(l0, a0[0], dot4(l1, a0[1], dot4(h0, a1[0], dot4(h1, a1[1], 0))));
                const float tm = (float) sumi * (yd * e8m0_half(cq[u][r].e));
                const bool rv = valid && (cgrp * ROWS + r) < nrows;
                acc[r] += rv ? tm : 0.0f;
            }
        }
        if (cit == nit - 1) {
#pragma unroll
            for (int r = 0; r < ROWS; ++r) {
                const int row = cgrp * ROWS + r;
                const float s = wave_sum(acc[r]);
                if (lane == 0 && row < nrows) *(float *) (dst + (size_t) row * 4) = s;
                acc[r] = 0.0f;
            }
        }
        if (!more) break;
    }
}

static long g_mmv_id_mxfp4_launches = 0;
long mmv_id_mxfp4_launches() { return g_mmv_id_mxfp4_launches; }

void mmv_id_mxfp4(const mmv_id_args & a, hipStream_t st) {
    if (a.nrows == 0 || a.n_ids == 0 || a.n_tokens == 0) return;
    const size_t lds = q80_image_bytes(a.K);
    if (a.type != GGML_TYPE_MXFP4 || a.K < 32 || a.K % 32 != 0 || a.K > INT32_MAX || lds > (size_t) 152 * 1024 || a.n_ids > 65535 || a.n_tokens > 65535 || a.n_expert < 1 || a.b_ne1 < 1 ||
        a.nrows > INT32_MAX || a.as_nb1 < (size_t) (a.K / 32) * 17) {
        fprintf(stderr, "[mi355x] mmv_id_mxfp4: shape / type out of range (type %d, K=%lld, ids %lld x %lld)\n", a.type, (long long) a.K, (long long) a.n_ids, (long long) a.n_tokens); abort();
    }
    // grid.x as mmv_id_kquant (mmvk.hip): every row group of one pair resident at once; with many pairs it shrinks so that the whole launch stays near 4 resident
    // rounds of 1024 workgroups -- each workgroup then grid-strides over the pair's row groups and stages the pair's image once
    static const int cap = [] { const char * e = getenv("MI355X_MMV_WGS"); const int c = e ? atoi(e) : 1024; return c < 1 ? 1024 : c; }();
    const int64_t pairs = a.n_ids * a.n_tokens;
    int64_t gx = ((a.nrows + 1) / 2 + 3) / 4;
    const int64_t budget = (int64_t) cap * 4 / pairs;
    if (gx > budget) gx = budget;
    if (gx < 1) gx = 1;
    mx_id_dev d;
    d.as = (const char *) a.as; d.as_nb1 = a.as_nb1; d.as_nb2 = a.as_nb2; d.n_expert = (int) a.n_expert;
    d.ids = (const char *) a.ids; d.ids_nb0 = a.ids_nb0; d.ids_nb1 = a.ids_nb1;
    d.act = (const char *) a.act; d.b_ne1 = (int) a.b_ne1;
    d.dst = (char *) a.dst; d.dst_nb1 = a.dst_nb1; d.dst_nb2 = a.dst_nb2;
    d.K = (int) a.K; d.nrows = (int) a.nrows;
    const dim3 grid((unsigned) gx, (unsigned) a.n_ids, (unsigned) a.n_tokens);
    // steps per stage: two (64 blocks, as the dense nibble forms at one column) unless one wastes fewer lane slots on the row's ragged end -- gpt-oss rows are
    // 90 blocks: three steps of 32 cover them with 6 idle slots, two stages of 64 with 38.  MI355X_MXFP4_U = 1 / 2 overrides for tuning.
    static const int u_env = getenv("MI355X_MXFP4_U") ? atoi(getenv("MI355X_MXFP4_U")) : 0;
    const int64_t nb = a.K / 32;
    const bool u2 = u_env ? u_env == 2 : ((nb + 63) / 64 * 64 - nb <= (nb + 31) / 32 * 32 - nb);
    auto go = [&](auto kern) {
        if (lds > 64 * 1024) HIP_CHECK(hipFuncSetAttribute((const void *) kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds));
        kern<<<grid, dim3(256), lds, st>>>(d);
    };
    if (u2) go(k_mmv_id_mxfp4<2>); else go(k_mmv_id_mxfp4<1>);
    ++g_mmv_id_mxfp4_launches;
}

} // namespace mi
