// mmvq.hip -- weight-streaming mat-vec kernels for Q8_0 / Q4_0 / Q5_0 / Q4_1 / Q5_1 / Q2_K / Q3_K / IQ4_NL / IQ4_XS / F16 / F32 weights (gfx950, wave64); Q4_K / Q5_K / Q6_K live in mmvk.hip.
//
// Computes what the reference CPU backend computes in ggml_compute_forward_mul_mat
// (ggml-cpu/ggml-cpu.c:1210-1402) for ne11 <= 8: every output is one `vec_dot` of a quantised weight
// row with the activation row quantised to the weight type's vec_dot_type:
//     Q4_K x Q8_K : ggml_vec_dot_q4_K_q8_K  (ggml-cpu/quants.c:550-623)
//     Q6_K x Q8_K : ggml_vec_dot_q6_K_q8_K  (ggml-cpu/quants.c:705-758)
//     Q8_0 x Q8_0 : ggml_vec_dot_q8_0_q8_0  (ggml-cpu/quants.c:305-333)
//     F16  x F16  : ggml_vec_dot_f16        (ggml-cpu/vec.cpp)
// Integer sub-block sums are exact and identical to the oracle; only the order of the f32 additions
// across blocks differs (64-lane tree instead of an 8-lane SIMD accumulator).
//
// Design (HBM-bound, 8 TB/s): the weight matrix is read exactly once with 16-B non-temporal loads
// straight into VGPRs (no LDS round trip for single-use data); the small activation image is staged once
// per workgroup in LDS; the next step's weight loads are issued before the current step is consumed so
// every wave keeps >= 2*ROWS KiB in flight; 4-way int8 dot products (v_dot4_i32_i8); wave64 butterfly at
// the end of each row group.  No bounds branches around loads: addresses are clamped and the contribution
// of out-of-range lanes is zeroed, so the compiler keeps all loads of a step in one clause.
#include "blocks_dev.hpp"

namespace mi {

extern __shared__ __attribute__((aligned(16))) char mmv_lds[];

// stage `ncols` activation images (each `bytes`, multiple of 16) into LDS
static __device__ __forceinline__ void stage_act(const char * act, size_t act_cs, int ncols, size_t bytes) {
    const int n16 = (int) (bytes >> 4);
    for (int c = 0; c < ncols; ++c) {
        const u32x4 * s = (const u32x4 *) (act + c * act_cs);
        u32x4 *       d = (u32x4 *) (mmv_lds + c * bytes);
        for (int i = threadIdx.x; i < n16; i += blockDim.x) d[i] = s[i];
    }
}

// =================================================================================================
// The block formats share one kernel frame, k_mmv_blocks<Form, NCOLS, ROWS>.  A wave walks the row groups wave, wave + nwaves, ... of ROWS
// rows each; in one step its 64 lanes cover 64 / Form::LANES blocks of every row of the group (lane = block g, part `part` of that block),
// U steps make a stage.  The frame owns the bookkeeping, the clamps that keep every load in bounds, the barrier, the stage pipeline, the
// masking of out-of-range lanes and rows, and the reduction and store at the end of a row group.  A Form supplies what differs:
//   LANES, BYTES, LOG2W, ID    lanes per block, bytes per block, log2 of the weights per block, slot of the launch counter
//   U(ncols)                   steps per stage
//   image_bytes(K)             size of one activation image (Q8_0 / Q8_1 / Q8_K)
//   regs,  load(bp, part)      what a lane holds in flight for one row of one step, and the loads of block `bp` that fill it
//   row,   decode(regs, part)  the weights as the dot products take them: once per (step, row), not per column
//   col,   read(im, ib, part, K, nb)   the lane's part of block ib of one image: once per (step, column), not per row
//   term(row, col, part)       the f32 contribution of the block part to the output; the frame masks and adds it
//   reduce(v)                  the wave sum.  wave_sum (six shuffles, a butterfly) and wave_sum_f32 (DPP rows, then row broadcasts) add in
//                              different orders, so their f32 results differ in the last bit: each form keeps the one it was written with.
// =================================================================================================
template <class Form, int NCOLS, int ROWS>
__global__ void __launch_bounds__(256) k_mmv_blocks(const char * __restrict__ W, size_t w_rs, const char * __restrict__ act, size_t act_cs,
                                                   char * __restrict__ dst, size_t dst_cs, int K, int nrows) {
    constexpr int U = Form::U(NCOLS), BPS = 64 / Form::LANES;                 // blocks per wave step
    const int lane = threadIdx.x & 63;
    const int g = lane / Form::LANES, part = lane % Form::LANES;
    const int nb  = K >> Form::LOG2W;
    const int nit = (nb + BPS * U - 1) / (BPS * U);
    const size_t img = Form::image_bytes(K);
    const int wave   = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int nwaves = gridDim.x * 4;
    const int ngrp   = (nrows + ROWS - 1) / ROWS;

    // no bounds branch around a load: block index and row are clamped, the contribution is zeroed when it is consumed
    typename Form::regs q[U][ROWS];
    auto issue = [&](int grp, int it) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int ib = (it * U + u) * BPS + g; ib = ib < nb ? ib : nb - 1;
#pragma unroll
            for (int r = 0; r < ROWS; ++r) {
                int row = grp * ROWS + r; row = row < nrows ? row : nrows - 1;
                q[u][r] = Form::load(W + (size_t) row * w_rs + (size_t) ib * Form::BYTES, part);
            }
        }
    };
    // the first stage is requested before the activation images are staged; every wave reaches the barrier before any returns
    int grp = wave, it = 0;
    if (grp < ngrp) issue(grp, 0);
    stage_act(act, act_cs, NCOLS, img);
    __syncthreads();
    if (grp >= ngrp) return;

    float acc[ROWS][NCOLS];
#pragma unroll
    for (int r = 0; r < ROWS; ++r)
#pragma unroll
        for (int c = 0; c < NCOLS; ++c) acc[r][c] = 0.0f;
    while (true) {
        // the registers in flight are copied, then the next stage (of this row group or of the wave's next one) is requested
        typename Form::regs cq[U][ROWS];
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
            typename Form::row w[ROWS];
#pragma unroll
            for (int r = 0; r < ROWS; ++r) w[r] = Form::decode(cq[u][r], part);
#pragma unroll
            for (int c = 0; c < NCOLS; ++c) {
                const typename Form::col y = Form::read(mmv_lds + c * img, ibc, part, K, nb);
#pragma unroll
                for (int r = 0; r < ROWS; ++r) {
                    const bool rv = valid && (cgrp * ROWS + r) < nrows;
                    const float t = Form::term(w[r], y, part);
                    acc[r][c] += rv ? t : 0.0f;
                }
            }
        }
        if (cit == nit - 1) {
#pragma unroll
            for (int r = 0; r < ROWS; ++r) {
                const int row = cgrp * ROWS + r;
#pragma unroll
                for (int c = 0; c < NCOLS; ++c) {
                    const float s = Form::reduce(acc[r][c]);
                    if (lane == 0 && row < nrows) *(float *) (dst + c * dst_cs + (size_t) row * 4) = s;
                    acc[r][c] = 0.0f;
                }
            }
        }
        if (!more) break;
    }
}

// MUL_MAT_ID (mixture-of-experts) on experts of the block formats: dst[:, i, t] = as[:, :, ids[i, t]] . b[:, i % b_ne1, t], as k_mmv_id (mmvk.hip) for the K-quants.
// Grid x = row workgroups, y = slot i, z = token t: every workgroup reads its ONE id from device memory (a captured graph follows the ids of each replay), clamps it
// into [0, n_expert) before it becomes an address, picks the expert's matrix and the pair's image, and runs the frame above at ONE column: the same stages, clamps and
// masks, the Forms unchanged -- so the same vec_dot integers and the same f32 summation order as a MUL_MAT of that expert's matrix with that column.  (The frame is
// written out a second time rather than shared as a device function: shared, the dense kernels' code would no longer be the instructions they were measured with.)
struct mmv_blocks_id_dev {
    const char * as; size_t as_nb1, as_nb2; int n_expert;
    const char * ids; size_t ids_nb0, ids_nb1;
    const char * act; int b_ne1;
    char * dst; size_t dst_nb1, dst_nb2;
    int K, nrows;
};
template <class Form, int ROWS>
__global__ void __launch_bounds__(256) k_mmv_blocks_id(const mmv_blocks_id_dev a) {
    constexpr int U = Form::U(1), BPS = 64 / Form::LANES;
    const int i = blockIdx.y, t = blockIdx.z;
    int id = *(const int *) (a.ids + (size_t) i * a.ids_nb0 + (size_t) t * a.ids_nb1);
    id = id < 0 ? 0 : (id >= a.n_expert ? a.n_expert - 1 : id);
    id = __builtin_amdgcn_readfirstlane(id);
    const int K = a.K, nrows = a.nrows;
    const size_t w_rs = a.as_nb1;
    const char * __restrict__ W   = a.as + (size_t) id * a.as_nb2;
    const char * __restrict__ act = a.act + (size_t) (t * a.b_ne1 + i % a.b_ne1) * Form::image_bytes(K);
    char * __restrict__ dst       = a.dst + (size_t) i * a.dst_nb1 + (size_t) t * a.dst_nb2;

    const int lane = threadIdx.x & 63;
    const int g = lane / Form::LANES, part = lane % Form::LANES;
    const int nb  = K >> Form::LOG2W;
    const int nit = (nb + BPS * U - 1) / (BPS * U);
    const int wave   = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int nwaves = gridDim.x * 4;
    const int ngrp   = (nrows + ROWS - 1) / ROWS;

    // no bounds branch around a load: block index and row are clamped, the contribution is zeroed when it is consumed
    typename Form::regs q[U][ROWS];
    auto issue = [&](int grp, int it) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int ib = (it * U + u) * BPS + g; ib = ib < nb ? ib : nb - 1;
#pragma unroll
            for (int r = 0; r < ROWS; ++r) {
                int row = grp * ROWS + r; row = row < nrows ? row : nrows - 1;
                q[u][r] = Form::load(W + (size_t) row * w_rs + (size_t) ib * Form::BYTES, part);
            }
        }
    };
    // the first stage is requested before the pair's image is staged; every wave reaches the barrier before any returns
    int grp = wave, it = 0;
    if (grp < ngrp) issue(grp, 0);
    stage_act(act, 0, 1, Form::image_bytes(K));
    __syncthreads();
    if (grp >= ngrp) return;

    float acc[ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) acc[r] = 0.0f;
    while (true) {
        typename Form::regs cq[U][ROWS];
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
            const typename Form::col y = Form::read(mmv_lds, valid ? ib : nb - 1, part, K, nb);
#pragma unroll
            for (int r = 0; r < ROWS; ++r) {
                const bool rv = valid && (cgrp * ROWS + r) < nrows;
                const float tm = Form::term(Form::decode(cq[u][r], part), y, part);
                acc[r] += rv ? tm : 0.0f;
            }
        }
        if (cit == nit - 1) {
#pragma unroll
            for (int r = 0; r < ROWS; ++r) {
                const int row = cgrp * ROWS + r;
                const float s = Form::reduce(acc[r]);
                if (lane == 0 && row < nrows) *(float *) (dst + (size_t) row * 4) = s;
                acc[r] = 0.0f;
            }
        }
        if (!more) break;
    }
}

// =================================================================================================
// Q8_0 : 34-B block {f16 d, int8 qs[32]} (ggml-common.h:219-224).  Activation image: qs[K] int8 + per-32 f32 scale.
//   sumf += sumi * (d_x * d_y)   (ggml-cpu/quants.c:318-327)
// Four lanes per 34-byte block (8 quants = one hardware-unaligned 8-byte load each; blocks are only 2-byte aligned), 16 blocks per
// wave step, U steps per stage.
// =================================================================================================
struct q80_form {
    static constexpr int LANES = 4, BYTES = 34, LOG2W = 5, ID = MMV_FORM_Q8_0;
    static constexpr int U(int ncols) { return ncols <= 2 ? 4 : 2; }
    MI_HD static size_t image_bytes(int64_t K) { return q80_image_bytes(K); }
    typedef u32x2 __attribute__((aligned(2))) u32x2a2;
    struct regs { u32x2 q; uint32_t dw; };
    struct row  { u32x2 q; float dx; };
    struct col  { u32x2 a; float yd; };
    static __device__ __forceinline__ regs load(const char * bp, int lp) {
        regs x;
        x.dw = *(const uint16_t *) bp;
        x.q  = *(const u32x2a2 *) (bp + 2 + 8 * lp);
        return x;
    }
    static __device__ __forceinline__ row decode(const regs & x, int) { return { x.q, h2f((uint16_t) x.dw) }; }
    static __device__ __forceinline__ col read(const char * im, int ib, int lp, int K, int) {
        col y;
        y.a  = *(const u32x2 *) (im + ib * 32 + 8 * lp);
        y.yd = *(const float *) (im + K + ib * 4);
        return y;
    }
    static __device__ __forceinline__ float term(const row & w, const col & y, int) { return (float) dot4(w.q[0], y.a[0], dot4(w.q[1], y.a[1], 0)) * (w.dx * y.yd); }
    static __device__ __forceinline__ float reduce(float v) { return wave_sum(v); }
};

// ---- shared by the five nibble forms of 32-weight blocks (Q4_0 / Q5_0 / IQ4_NL / Q4_1 / Q5_1).  Two lanes per block: lane half hf owns nibble
// bytes 8hf .. 8hf+7 = weights 8hf..8hf+7 (low nibbles) and 16+8hf..23+8hf (high); 32 blocks per wave step, U steps per stage.
template <bool Q5> struct qh_word { uint32_t qh; };            // the fifth bits of a Q5_0 / Q5_1 block: a member of `regs` only where the format has them
template <> struct qh_word<false> {};
// (spread5, the fifth bits of 4 consecutive weights into bit 4 of the four bytes of a word: blocks_dev.hpp)
struct nib_quants { uint32_t lo[2], hi[2]; };                   // the lane's 16 quants, one per byte
template <bool Q5>
static __device__ __forceinline__ nib_quants nib_unpack(u32x2 q, uint32_t qh, int hf) {
    nib_quants n;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        n.lo[k] = q[k] & 0x0f0f0f0fu; n.hi[k] = (q[k] >> 4) & 0x0f0f0f0fu;
        if (Q5) { n.lo[k] |= spread5((qh >> (8 * hf + 4 * k)) & 0xfu); n.hi[k] |= spread5((qh >> (16 + 8 * hf + 4 * k)) & 0xfu); }
    }
    return n;
}
struct nib_act { u32x2 a0, a1; float yd; };                     // the activations under the lane's low and high nibbles, and the block's scale
static __device__ __forceinline__ nib_act nib_read(const char * im, int ib, int hf, int K) {
    nib_act y;
    y.a0 = *(const u32x2 *) (im + ib * 32 + 8 * hf);
    y.a1 = *(const u32x2 *) (im + ib * 32 + 16 + 8 * hf);
    y.yd = *(const float *) (im + K + ib * 4);
    return y;
}
static __device__ __forceinline__ int nib_dot(const nib_quants & n, const nib_act & y) {
    return dot4(n.lo[0], y.a0[0], dot4(n.lo[1], y.a0[1], dot4(n.hi[0], y.a1[0], dot4(n.hi[1], y.a1[1], 0))));
}

// =================================================================================================
// Q4_0 / Q5_0 weights x Q8_0 activations.  reference: ggml_vec_dot_q4_0_q8_0 / _q5_0_q8_0 (ggml-cpu/quants.c:115-149, 219-262):
//   sumi = sum_j ((x.qs[j] & 0xF) [| fifth bit] - OFF) * y.qs[j] + ((x.qs[j] >> 4) [| fifth bit] - OFF) * y.qs[j + 16],  OFF = 8 / 16
//   sumf += sumi * d_x * d_y
// Blocks are 18 B {f16 d, qs[16]} / 22 B {f16 d, u32 qh, qs[16]}, 2-byte aligned.  Two lanes per block (see above); the offset is taken out of
// the dot products (sum q*y - OFF * sum y), all in exact integers.
// =================================================================================================
template <bool Q5>
struct q40_form {
    static constexpr int LANES = 2, BYTES = Q5 ? 22 : 18, LOG2W = 5, ID = Q5 ? MMV_FORM_Q5_0 : MMV_FORM_Q4_0;
    static constexpr int QOFF = Q5 ? 6 : 2, OFF = Q5 ? 16 : 8;
    static constexpr int U(int ncols) { return ncols <= 2 ? 2 : 1; }
    MI_HD static size_t image_bytes(int64_t K) { return q80_image_bytes(K); }
    typedef u32x2 __attribute__((aligned(2))) u32x2a2;
    typedef uint32_t __attribute__((aligned(2))) u32a2;
    struct regs : qh_word<Q5> { u32x2 q; uint32_t dw; };
    struct row  { nib_quants n; float dx; };
    struct col  { nib_act y; int ysum; };
    static __device__ __forceinline__ regs load(const char * bp, int hf) {
        regs x;
        x.dw = *(const uint16_t *) bp;
        x.q  = *(const u32x2a2 *) (bp + QOFF + 8 * hf);
        if constexpr (Q5) x.qh = *(const u32a2 *) (bp + 2);
        return x;
    }
    static __device__ __forceinline__ row decode(const regs & x, int hf) {
        uint32_t qh = 0;
        if constexpr (Q5) qh = x.qh;
        return { nib_unpack<Q5>(x.q, qh, hf), h2f((uint16_t) x.dw) };
    }
    static __device__ __forceinline__ col read(const char * im, int ib, int hf, int K, int) {
        col c;
        c.y    = nib_read(im, ib, hf, K);
        c.ysum = dot4(0x01010101u, c.y.a0[0], dot4(0x01010101u, c.y.a0[1], dot4(0x01010101u, c.y.a1[0], dot4(0x01010101u, c.y.a1[1], 0))));
        return c;
    }
    static __device__ __forceinline__ float term(const row & w, const col & c, int) {
        const int isum = nib_dot(w.n, c.y) - OFF * c.ysum;
        return (float) isum * (w.dx * c.y.yd);
    }
    static __device__ __forceinline__ float reduce(float v) { return wave_sum(v); }
};

// =================================================================================================
// IQ4_NL / IQ4_XS: 4-bit indices into the 16-entry int8 table kvalues_iq4nl (ggml-common.h:1088-1090), no min term.
//   IQ4_NL x Q8_0 : ggml_vec_dot_iq4_nl_q8_0 (ggml-cpu/arch/x86/quants.c:3631; generic ggml-cpu/quants.c:1108-1131)
//                   sumi = sum_j y.qs[j] * kv[x.qs[j] & 0xF] + y.qs[j + 16] * kv[x.qs[j] >> 4];  sumf += sumi * (d_x * d_y)
//   IQ4_XS x Q8_K : ggml_vec_dot_iq4_xs_q8_K (x86 :3715; generic :1133-1170) -- the x86 form scales every 32-weight sub-block sum by
//                   (ls - 32) in integers and converts once per 256-weight super-block: sumi = sum_ib (ls_ib - 32) * sumi_ib;  sumf += sumi * (d_x * d_y)
// Four indices become four int8 values through iq4nl_lut4 (blocks_dev.hpp: the table in four dwords of registers, two byte permutes and a per-byte select), then go
// straight into v_dot4_i32_i8.
// =================================================================================================

// IQ4_NL: 18-B block {f16 d, qs[16]} (2-byte aligned).  Two lanes per block as Q4_0: lane half hf owns qs bytes 8hf .. 8hf+7 = weights
// 8hf..8hf+7 (low nibbles) and 16+8hf..23+8hf (high); 32 blocks per wave step, U steps per stage.
struct iq4nl_form {
    static constexpr int LANES = 2, BYTES = 18, LOG2W = 5, ID = MMV_FORM_IQ4_NL;
    static constexpr int U(int ncols) { return ncols <= 2 ? 2 : 1; }
    MI_HD static size_t image_bytes(int64_t K) { return q80_image_bytes(K); }
    typedef u32x2 __attribute__((aligned(2))) u32x2a2;
    struct regs { u32x2 q; uint32_t dw; };
    struct row  { nib_quants n; float dx; };
    typedef nib_act col;
    static __device__ __forceinline__ regs load(const char * bp, int hf) {
        regs x;
        x.dw = *(const uint16_t *) bp;
        x.q  = *(const u32x2a2 *) (bp + 2 + 8 * hf);
        return x;
    }
    static __device__ __forceinline__ row decode(const regs & x, int) {
        row w;
        w.dx = h2f((uint16_t) x.dw);
#pragma unroll
        for (int k = 0; k < 2; ++k) { w.n.lo[k] = iq4nl_lut4(x.q[k] & 0x0f0f0f0fu); w.n.hi[k] = iq4nl_lut4((x.q[k] >> 4) & 0x0f0f0f0fu); }
        return w;
    }
    static __device__ __forceinline__ col read(const char * im, int ib, int hf, int K, int) { return nib_read(im, ib, hf, K); }
    static __device__ __forceinline__ float term(const row & w, const col & y, int) { return (float) nib_dot(w.n, y) * (w.dx * y.yd); }
    static __device__ __forceinline__ float reduce(float v) { return wave_sum(v); }
};

// IQ4_XS: 136-B super-block {f16 d, u16 scales_h, u8 scales_l[4], qs[128]} (2-byte aligned rows), Q8_K image (qs[K] | bsums | d[K/256]).
// Four lanes per super-block: lane quarter qq owns the 32-weight sub-blocks 2qq and 2qq+1 (qs bytes 32qq .. 32qq+31, two 16-byte loads) and
// reads the 8-byte header beside them; 16 super-blocks per wave step (K = 4096: one step per row), the next row group's loads issued before
// the current one is consumed.  ls = scales_l nibble | two bits of scales_h << 4 (dequantize_row_iq4_xs, ggml-quants.c:2530-2550).
struct iq4xs_form {
    static constexpr int LANES = 4, BYTES = 136, LOG2W = 8, ID = MMV_FORM_IQ4_XS;
    static constexpr int U(int) { return 1; }
    MI_HD static size_t image_bytes(int64_t K) { return q8k_image_bytes(K); }
    typedef u32x2 __attribute__((aligned(2))) u32x2a2;
    typedef u32x4 __attribute__((aligned(2))) u32x4a2;
    struct regs { u32x2 h; u32x4 q[2]; };
    struct row  { uint32_t lo[2][4], hi[2][4]; int ls[2]; float dx; };
    struct col  { u32x4 a[2][2]; float yd; };
    static __device__ __forceinline__ regs load(const char * bp, int qq) {
        regs x;
        x.h    = *(const u32x2a2 *) bp;
        x.q[0] = *(const u32x4a2 *) (bp + 8 + 32 * qq);
        x.q[1] = *(const u32x4a2 *) (bp + 24 + 32 * qq);
        return x;
    }
    static __device__ __forceinline__ row decode(const regs & x, int qq) {
        row w;
        w.dx = h2f((uint16_t) (x.h[0] & 0xffffu));
        const uint32_t sh = (x.h[0] >> 16) >> (4 * qq), sl = (x.h[1] >> (8 * qq)) & 0xffu;
        w.ls[0] = (int) ((sl & 0xfu) | ((sh & 3u) << 4)) - 32;
        w.ls[1] = (int) ((sl >> 4) | (((sh >> 2) & 3u) << 4)) - 32;
#pragma unroll
        for (int sb = 0; sb < 2; ++sb)
#pragma unroll
            for (int k = 0; k < 4; ++k) { w.lo[sb][k] = iq4nl_lut4(x.q[sb][k] & 0x0f0f0f0fu); w.hi[sb][k] = iq4nl_lut4((x.q[sb][k] >> 4) & 0x0f0f0f0fu); }
        return w;
    }
    static __device__ __forceinline__ col read(const char * im, int ib, int qq, int K, int) {
        col y;
        const char * p = im + (size_t) ib * 256 + 64 * qq;
#pragma unroll
        for (int sb = 0; sb < 2; ++sb) { y.a[sb][0] = *(const u32x4 *) (p + 32 * sb); y.a[sb][1] = *(const u32x4 *) (p + 32 * sb + 16); }
        y.yd = *(const float *) (im + K + K / 8 + ib * 4);
        return y;
    }
    static __device__ __forceinline__ float term(const row & w, const col & y, int) {
        int isum = 0;
#pragma unroll
        for (int sb = 0; sb < 2; ++sb) {
            int s = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) s = dot4(w.lo[sb][k], y.a[sb][0][k], dot4(w.hi[sb][k], y.a[sb][1][k], s));
            isum += w.ls[sb] * s;
        }
        return (float) isum * (w.dx * y.yd);
    }
    static __device__ __forceinline__ float reduce(float v) { return wave_sum(v); }
};

// =================================================================================================
// Q4_1 / Q5_1 weights x Q8_1 activations.  reference: ggml_vec_dot_q4_1_q8_1 / _q5_1_q8_1 (ggml-cpu/arch/x86/quants.c:701-758, :925):
//   sumi = sum_j (x.qs[j] & 0xF [| fifth bit]) * y.qs[j] + (x.qs[j] >> 4 [| fifth bit]) * y.qs[j + 16]      (quants unsigned: 0..15 / 0..31)
//   sumf += (d_x * d_y) * sumi + m_x * s_y,      s_y = f16(d_y * sum(y.qs)) from the Q8_1 image (qs[K] | d[K/32] | s[K/32])
// Blocks are 20 B {f16 d, f16 m, qs[16]} / 24 B {f16 d, f16 m, u32 qh, qs[16]}: rows and blocks are 4-byte aligned only, so every load is
// a dword or a dword pair.  Two lanes per block as Q4_0: lane half hf owns qs bytes 8hf .. 8hf+7 = weights 8hf..8hf+7 (low nibbles)
// and 16+8hf..23+8hf (high) and reads the header dword(s) beside them; half 0 adds the block's m_x * s_y.  32 blocks per wave step, U steps
// per stage.
// =================================================================================================
template <bool Q5>
struct q41_form {
    static constexpr int LANES = 2, BYTES = Q5 ? 24 : 20, LOG2W = 5, ID = Q5 ? MMV_FORM_Q5_1 : MMV_FORM_Q4_1;
    static constexpr int QOFF = Q5 ? 8 : 4;
    static constexpr int U(int ncols) { return ncols <= 2 ? 2 : 1; }
    MI_HD static size_t image_bytes(int64_t K) { return q81_image_bytes(K); }
    typedef u32x2 __attribute__((aligned(4))) u32x2a4;
    struct regs : qh_word<Q5> { u32x2 q; uint32_t dm; };
    struct row  { nib_quants n; float dx, mx; };
    struct col  { nib_act y; float ys; };
    static __device__ __forceinline__ regs load(const char * bp, int hf) {
        regs x;
        x.dm = *(const uint32_t *) bp;
        x.q  = *(const u32x2a4 *) (bp + QOFF + 8 * hf);
        if constexpr (Q5) x.qh = *(const uint32_t *) (bp + 4);
        return x;
    }
    static __device__ __forceinline__ row decode(const regs & x, int hf) {
        uint32_t qh = 0;
        if constexpr (Q5) qh = x.qh;
        return { nib_unpack<Q5>(x.q, qh, hf), h2f((uint16_t) (x.dm & 0xffffu)), hf == 0 ? h2f((uint16_t) (x.dm >> 16)) : 0.0f };
    }
    static __device__ __forceinline__ col read(const char * im, int ib, int hf, int K, int nb) {
        col c;
        c.y  = nib_read(im, ib, hf, K);
        c.ys = *(const float *) (im + K + (nb + ib) * 4);
        return c;
    }
    static __device__ __forceinline__ float term(const row & w, const col & c, int hf) {
        return (float) nib_dot(w.n, c.y) * (w.dx * c.y.yd) + (hf == 0 ? w.mx * c.ys : 0.0f);
    }
    static __device__ __forceinline__ float reduce(float v) { return wave_sum_f32(v); }
};

// =================================================================================================
// Q2_K / Q3_K weights x Q8_K activations (image: qs[K] | bsums[K/16] int16 | d[K/256]).  Both formats cut a 256-weight super-block into sixteen
// 16-weight groups: group k = 8n + 2j + sub covers weights 128n + 32j + 16sub .. +15, whose 2-bit quants are bits 2j, 2j+1 of qs bytes
// 32n + 16sub .. +15 (dequantize_row_q2_K / _q3_K, ggml-quants.c:784 / :1128) -- bsums[k] of the image is the sum of exactly those activations.
// Four lanes per super-block: lane quarter qq = 2n + sub owns those 16 qs bytes (one 16-byte load), i.e. the four groups j = 0..3 of its (n, sub);
// 16 super-blocks per wave step (K = 4096: one step per row), the next row group's loads issued before the current one is consumed.
//   Q2_K x Q8_K : ggml_vec_dot_q2_K_q8_K (ggml-cpu/arch/x86/quants.c:1277-1353)
//                 sumf += (d_y * d_x) * sum_k sc_k * sum(q2 * q8) - (d_y * dmin_x) * sum_k m_k * bsums[k],   scales[k] = sc_k | m_k << 4
//   Q3_K x Q8_K : ggml_vec_dot_q3_K_q8_K (:1469-1587)
//                 sumf += (d_y * d_x) * sum_k (sc_k - 32) * sum(q3 * q8),   q3 = 2 low bits | hmask bit << 2, minus 4  (the 4 taken out: - 4 * bsums[k])
// All sums are exact integers; the four lanes of a super-block each convert their quarter, which the reference converts in eight SIMD lanes.
// =================================================================================================
struct k16_act { u32x4 a[4]; int bsum[4]; float yd; };           // the activations of the lane's four groups, their sums, the super-block's scale
static __device__ __forceinline__ k16_act k16_read(const char * im, int ib, int qq, int K) {
    const int n = qq >> 1, sub = qq & 1;
    k16_act y;
#pragma unroll
    for (int j = 0; j < 4; ++j) y.a[j] = *(const u32x4 *) (im + (size_t) ib * 256 + 128 * n + 32 * j + 16 * sub);
    const u32x4 bs = *(const u32x4 *) (im + K + ib * 32 + 16 * n);          // bsums[8n .. 8n+7]: group j of this lane is element 2j + sub
    y.yd = *(const float *) (im + K + K / 8 + ib * 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) y.bsum[j] = ((int) (bs[j] << (16 - 16 * sub))) >> 16;
    return y;
}

// Q2_K: 84-B block {scales[16], qs[64], f16 d, f16 dmin}, 4-byte aligned: the lane reads its 16 qs bytes, the 8 scale bytes of its half n
// (its own four are bytes 2j + sub of them) and the d / dmin dword.
struct q2k_form {
    static constexpr int LANES = 4, BYTES = 84, LOG2W = 8, ID = MMV_FORM_Q2_K;
    static constexpr int U(int) { return 1; }
    MI_HD static size_t image_bytes(int64_t K) { return q8k_image_bytes(K); }
    typedef u32x2 __attribute__((aligned(4))) u32x2a4;
    typedef u32x4 __attribute__((aligned(4))) u32x4a4;
    struct regs { u32x4 q; u32x2 sc; uint32_t dd; };
    struct row  { uint32_t q2[4][4]; int scl[4], mn[4]; float dx, dmin; };
    typedef k16_act col;
    static __device__ __forceinline__ regs load(const char * bp, int qq) {
        regs x;
        x.sc = *(const u32x2a4 *) (bp + 8 * (qq >> 1));
        x.q  = *(const u32x4a4 *) (bp + 16 + 16 * qq);
        x.dd = *(const uint32_t *) (bp + 80);
        return x;
    }
    static __device__ __forceinline__ row decode(const regs & x, int qq) {
        const int sub = qq & 1;
        row w;
        w.dx = h2f((uint16_t) (x.dd & 0xffffu)); w.dmin = h2f((uint16_t) (x.dd >> 16));
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t sb = (x.sc[j >> 1] >> (8 * (2 * (j & 1) + sub))) & 0xffu;
            w.scl[j] = (int) (sb & 0xfu); w.mn[j] = (int) (sb >> 4);
#pragma unroll
            for (int k = 0; k < 4; ++k) w.q2[j][k] = (x.q[k] >> (2 * j)) & 0x03030303u;
        }
        return w;
    }
    static __device__ __forceinline__ col read(const char * im, int ib, int qq, int K, int) { return k16_read(im, ib, qq, K); }
    static __device__ __forceinline__ float term(const row & w, const col & y, int) {
        int isum = 0, msum = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int s = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) s = dot4(w.q2[j][k], y.a[j][k], s);
            isum += w.scl[j] * s;
            msum += w.mn[j] * y.bsum[j];
        }
        return (y.yd * w.dx) * (float) isum - (y.yd * w.dmin) * (float) msum;
    }
    static __device__ __forceinline__ float reduce(float v) { return wave_sum_f32(v); }
};

// Q3_K: 110-B block {hmask[32], qs[64], scales[12], f16 d}, 2-byte aligned only (110 = 2 * 55): no field of a block has a fixed dword phase, so
// the lane mapping is built on three 16-byte loads that the hardware takes at any 2-byte address and that all stay inside the block --
//   hmask bytes 16sub .. +15 (bit 4n + j of byte l is the high bit of group j's weight l), qs bytes 16qq .. +15, and bytes 94 .. 109:
//   the last two qs bytes (unused), the 12 scale bytes and d -- a 16-byte load at 96 would run two bytes past the tensor's last block.
// The 6-bit scales are unpacked as the reference does (kmask1 / kmask2 on three dwords): scale k is byte k & 3 of word k >> 2.
struct q3k_form {
    static constexpr int LANES = 4, BYTES = 110, LOG2W = 8, ID = MMV_FORM_Q3_K;
    static constexpr int U(int) { return 1; }
    MI_HD static size_t image_bytes(int64_t K) { return q8k_image_bytes(K); }
    typedef u32x4 __attribute__((aligned(2))) u32x4a2;
    struct regs { u32x4 hm, q, hd; };
    struct row  { uint32_t q3[4][4]; int scl[4]; float dx; };
    typedef k16_act col;
    static __device__ __forceinline__ regs load(const char * bp, int qq) {
        regs x;
        x.hm = *(const u32x4a2 *) (bp + 16 * (qq & 1));
        x.q  = *(const u32x4a2 *) (bp + 32 + 16 * qq);
        x.hd = *(const u32x4a2 *) (bp + 94);
        return x;
    }
    static __device__ __forceinline__ row decode(const regs & x, int qq) {
        const int n = qq >> 1, sub = qq & 1;
        row w;
        const uint32_t aux0 = (x.hd[0] >> 16) | (x.hd[1] << 16), aux1 = (x.hd[1] >> 16) | (x.hd[2] << 16), aux2 = (x.hd[2] >> 16) | (x.hd[3] << 16);
        w.dx = h2f((uint16_t) (x.hd[3] >> 16));
        // words 2n and 2n + 1 of the reference's scales128: scales 8n .. 8n+3 and 8n+4 .. 8n+7
        const uint32_t sa = ((aux0 >> (4 * n)) & 0x0f0f0f0fu) | (((aux2 >> (4 * n)) & 0x03030303u) << 4);
        const uint32_t sb = ((aux1 >> (4 * n)) & 0x0f0f0f0fu) | (((aux2 >> (4 * n + 2)) & 0x03030303u) << 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            w.scl[j] = (int) (((j < 2 ? sa : sb) >> (8 * (2 * (j & 1) + sub))) & 0xffu) - 32;
#pragma unroll
            for (int k = 0; k < 4; ++k) w.q3[j][k] = ((x.q[k] >> (2 * j)) & 0x03030303u) | (((x.hm[k] >> (4 * n + j)) & 0x01010101u) << 2);
        }
        return w;
    }
    static __device__ __forceinline__ col read(const char * im, int ib, int qq, int K, int) { return k16_read(im, ib, qq, K); }
    static __device__ __forceinline__ float term(const row & w, const col & y, int) {
        int isum = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int s = -4 * y.bsum[j];
#pragma unroll
            for (int k = 0; k < 4; ++k) s = dot4(w.q3[j][k], y.a[j][k], s);
            isum += w.scl[j] * s;
        }
        return (y.yd * w.dx) * (float) isum;
    }
    static __device__ __forceinline__ float reduce(float v) { return wave_sum_f32(v); }
};

// =================================================================================================
// F16 / F32 weights: each lane consumes 16 B (8 halfs / 4 floats) per step; activations (f16 rows for F16
// weights, as the reference rounds src1 to the F16 vec_dot_type; f32 rows for F32 weights) live in LDS.
// =================================================================================================
// blockIdx.y walks the broadcast batch (attention without FLASH_ATTN_EXT: one K / V^T matrix per KV head, one activation per query
// head): batch b = i13 * ne12 + i12 reads W + (i12 / r2) * w_nb2 + (i13 / r3) * w_nb3 -- one launch instead of one per head.
struct mmv_batch { int ne12, r2, r3; size_t w_nb2, w_nb3, act_bs, dst_nb2, dst_nb3; };

template <int NCOLS, int ROWS, bool WF16>
__global__ void __launch_bounds__(256) k_mmv_f(const char * __restrict__ W, size_t w_rs, const char * __restrict__ act, size_t act_cs,
                                              char * __restrict__ dst, size_t dst_cs, int K, int nrows, const mmv_batch bt) {
    {
        const int b = blockIdx.y, i12 = b % bt.ne12, i13 = b / bt.ne12;
        W   += (size_t) (i12 / bt.r2) * bt.w_nb2 + (size_t) (i13 / bt.r3) * bt.w_nb3;
        act += (size_t) b * bt.act_bs;
        dst += (size_t) i12 * bt.dst_nb2 + (size_t) i13 * bt.dst_nb3;
    }
    constexpr int EPL = WF16 ? 8 : 4;                 // elements per lane per step
    const int lane = threadIdx.x & 63;
    const int nstep = (K + 64 * EPL - 1) / (64 * EPL);
    const size_t arow = ((size_t) K * (WF16 ? 2 : 4) + 15) & ~(size_t) 15;
    const int wave   = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int nwaves = gridDim.x * 4;
    const int ngrp   = (nrows + ROWS - 1) / ROWS;

    // stage activations (row bytes may be unaligned to 16: copy by 2/4-byte elements)
    for (int c = 0; c < NCOLS; ++c) {
        if (WF16) {
            const uint16_t * s = (const uint16_t *) (act + c * act_cs); uint16_t * d = (uint16_t *) (mmv_lds + c * arow);
            for (int i = threadIdx.x; i < K; i += blockDim.x) d[i] = s[i];
        } else {
            const float * s = (const float *) (act + c * act_cs); float * d = (float *) (mmv_lds + c * arow);
            for (int i = threadIdx.x; i < K; i += blockDim.x) d[i] = s[i];
        }
    }
    __syncthreads();

    const bool vec_ok = (K % EPL == 0) && (w_rs % 16 == 0) && (((uintptr_t) W & 15) == 0);
    if (vec_ok && K % (64 * EPL) == 0) {
        // whole 16-byte steps only (every model matrix): U steps per stage, the next stage's loads issued before the current one is
        // multiplied, activations read from LDS as one 16-byte vector per step.  Same multiply-add order as the general loop below.
        constexpr int U = NCOLS <= 2 ? 4 : 2;
        const int nstage = (nstep + U - 1) / U;
        u32x4 v[U][ROWS];
        auto issue = [&](int grp, int st) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                int sidx = st * U + u; sidx = sidx < nstep ? sidx : nstep - 1;
#pragma unroll
                for (int r = 0; r < ROWS; ++r) {
                    int row = grp * ROWS + r; row = row < nrows ? row : nrows - 1;
                    v[u][r] = ld_nt16(W + (size_t) row * w_rs + ((size_t) sidx * 64 + lane) * 16);
                }
            }
        };
        int grp = wave, st = 0;
        if (grp >= ngrp) return;
        issue(grp, 0);
        float acc[ROWS][NCOLS];
#pragma unroll
        for (int r = 0; r < ROWS; ++r)
#pragma unroll
            for (int c = 0; c < NCOLS; ++c) acc[r][c] = 0.0f;
        while (true) {
            u32x4 cv[U][ROWS];
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int r = 0; r < ROWS; ++r) cv[u][r] = v[u][r];
            const int cgrp = grp, cst = st;
            ++st;
            if (st == nstage) { st = 0; grp += nwaves; }
            const bool more = grp < ngrp;
            if (more) issue(grp, st);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int sidx = cst * U + u;
                if (sidx >= nstep) continue;
                float w[ROWS][EPL];
#pragma unroll
                for (int r = 0; r < ROWS; ++r) {
                    if (WF16) {
#pragma unroll
                        for (int k = 0; k < 4; ++k) { w[r][2 * k] = h2f((uint16_t) (cv[u][r][k] & 0xffff)); w[r][2 * k + 1] = h2f((uint16_t) (cv[u][r][k] >> 16)); }
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; ++k) { const uint32_t bits = cv[u][r][k]; w[r][k] = __uint_as_float(bits); }
                    }
                }
#pragma unroll
                for (int c = 0; c < NCOLS; ++c) {
                    const u32x4 xv = *(const u32x4 *) (mmv_lds + c * arow + ((size_t) sidx * 64 + lane) * 16);
                    float x[EPL];
                    if (WF16) {
#pragma unroll
                        for (int k = 0; k < 4; ++k) { x[2 * k] = h2f((uint16_t) (xv[k] & 0xffff)); x[2 * k + 1] = h2f((uint16_t) (xv[k] >> 16)); }
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; ++k) { const uint32_t bits = xv[k]; x[k] = __uint_as_float(bits); }
                    }
#pragma unroll
                    for (int r = 0; r < ROWS; ++r)
#pragma unroll
                        for (int k = 0; k < EPL; ++k) acc[r][c] = fmaf(w[r][k], x[k], acc[r][c]);
                }
            }
            if (cst == nstage - 1) {
#pragma unroll
                for (int r = 0; r < ROWS; ++r) {
                    const int row = cgrp * ROWS + r;
#pragma unroll
                    for (int c = 0; c < NCOLS; ++c) {
                        const float sum = wave_sum(acc[r][c]);
                        if (lane == 0 && row < nrows) *(float *) (dst + c * dst_cs + (size_t) row * 4) = sum;
                        acc[r][c] = 0.0f;
                    }
                }
            }
            if (!more) break;
        }
        return;
    }
    for (int grp = wave; grp < ngrp; grp += nwaves) {
        float acc[ROWS][NCOLS];
#pragma unroll
        for (int r = 0; r < ROWS; ++r)
#pragma unroll
            for (int c = 0; c < NCOLS; ++c) acc[r][c] = 0.0f;
        for (int s = 0; s < nstep; ++s) {
            const int e0 = (s * 64 + lane) * EPL;
            float w[ROWS][EPL];
#pragma unroll
            for (int r = 0; r < ROWS; ++r) {
                int row = grp * ROWS + r; row = row < nrows ? row : nrows - 1;
                const char * rp = W + (size_t) row * w_rs;
                if (vec_ok && e0 + EPL <= K) {
                    const u32x4 v = ld_nt16(rp + (size_t) e0 * (WF16 ? 2 : 4));
                    if (WF16) {
#pragma unroll
                        for (int k = 0; k < 4; ++k) { w[r][2 * k] = h2f((uint16_t) (v[k] & 0xffff)); w[r][2 * k + 1] = h2f((uint16_t) (v[k] >> 16)); }
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; ++k) { const uint32_t bits = v[k]; w[r][k] = __uint_as_float(bits); }   // (bit_cast on a vector element mis-selects element 0)
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < EPL; ++k) {
                        const int e = e0 + k;
                        w[r][k] = e < K ? (WF16 ? h2f(((const uint16_t *) rp)[e]) : ((const float *) rp)[e]) : 0.0f;
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < NCOLS; ++c) {
                float x[EPL];
#pragma unroll
                for (int k = 0; k < EPL; ++k) {
                    const int e = e0 + k;
                    x[k] = e < K ? (WF16 ? h2f(((const uint16_t *) (mmv_lds + c * arow))[e]) : ((const float *) (mmv_lds + c * arow))[e]) : 0.0f;
                }
#pragma unroll
                for (int r = 0; r < ROWS; ++r)
#pragma unroll
                    for (int k = 0; k < EPL; ++k) acc[r][c] = fmaf(w[r][k], x[k], acc[r][c]);
            }
        }
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            const int row = grp * ROWS + r;
#pragma unroll
            for (int c = 0; c < NCOLS; ++c) {
                const float s = wave_sum(acc[r][c]);
                if (lane == 0 && row < nrows) *(float *) (dst + c * dst_cs + (size_t) row * 4) = s;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ launch
static int grid_for(int64_t nrows, int rows_per_wave) {
    const int64_t ngrp = (nrows + rows_per_wave - 1) / rows_per_wave;
    int64_t g = (ngrp + 3) / 4;
    const int64_t cap = 256 * 8;          // 256 CUs x up to 8 resident workgroups
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (int) g;
}

// LDS budget: a workgroup may own up to 160 KiB; split the columns when the images would not fit.
static const size_t MMV_LDS_MAX = 152 * 1024;

template <typename F>
static void split_cols(const mmv_args & a, size_t bytes_per_col, F && launch) {
    int maxc = (int) (MMV_LDS_MAX / bytes_per_col);
    if (maxc < 1) { fprintf(stderr, "[mi355x] mmv: K=%lld too large for LDS staging\n", (long long) a.K); abort(); }
    if (maxc > MI_MMVQ_MAX_COLS) maxc = MI_MMVQ_MAX_COLS;
    for (int c0 = 0; c0 < a.ncols; c0 += maxc) {
        mmv_args s = a;
        s.ncols = a.ncols - c0 < maxc ? a.ncols - c0 : maxc;
        s.act   = (const char *) a.act + (size_t) c0 * a.act_cs;
        s.dst   = (float *) ((char *) a.dst + (size_t) c0 * a.dst_cs);
        launch(s);
    }
}

typedef void (*mmv_kernel_t)(const char *, size_t, const char *, size_t, char *, size_t, int, int);

static void launch_mmv(mmv_kernel_t k, int rows_per_wave, size_t lds, const mmv_args & a, hipStream_t st) {
    if (lds > 64 * 1024) HIP_CHECK(hipFuncSetAttribute((const void *) k, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds));
    k<<<dim3(grid_for(a.nrows, rows_per_wave)), dim3(256), lds, st>>>((const char *) a.W, a.w_rs, (const char *) a.act, a.act_cs,
                                                                     (char *) a.dst, a.dst_cs, (int) a.K, (int) a.nrows);
}

// tuning knob (decode, ncols == 1): MI355X_MMV_CFG = "<rows><u>" e.g. "22" (default), "12", "21", "41"
static void mmv_kquant_single(int type, const mmv_args & a0, hipStream_t st) {
    if (a0.nrows == 0 || a0.ncols == 0) return;
    split_cols(a0, q8k_image_bytes(a0.K), [&](const mmv_args & a) {
        mmv_multi_args m;
        m.nmat = 1; m.act = a.act; m.act_cs = a.act_cs; m.K = a.K; m.ncols = a.ncols;
        m.m[0] = { a.W, a.w_rs, a.dst, a.dst_cs, nullptr, 0, a.nrows, type };
        mmv_kquant_multi(m, st);
    });
}
void mmv_q4_K(const mmv_args & a, hipStream_t st) { mmv_kquant_single(GGML_TYPE_Q4_K, a, st); }
void mmv_q6_K(const mmv_args & a, hipStream_t st) { mmv_kquant_single(GGML_TYPE_Q6_K, a, st); }
void mmv_q5_K(const mmv_args & a, hipStream_t st) { mmv_kquant_single(GGML_TYPE_Q5_K, a, st); }

// the block formats: one launch per call of up to 8 columns (1 - 4 columns: two rows per wave, 5 - 8: one), counted per form
static long g_blocks_launches[MMV_FORM_COUNT];
long mmv_blocks_launches(int form) { return form >= 0 && form < MMV_FORM_COUNT ? g_blocks_launches[form] : 0; }
template <class Form>
static void mmv_blocks_launch(const mmv_args & a0, hipStream_t st) {
    if (a0.nrows == 0 || a0.ncols == 0) return;
    const size_t ib = Form::image_bytes(a0.K);
    split_cols(a0, ib, [&](const mmv_args & a) {
        mmv_kernel_t k = nullptr; int rows = 2;
        switch (a.ncols) {
            case 1: k = k_mmv_blocks<Form, 1, 2>; break;
            case 2: k = k_mmv_blocks<Form, 2, 2>; break;
            case 3: k = k_mmv_blocks<Form, 3, 2>; break;
            case 4: k = k_mmv_blocks<Form, 4, 2>; break;
            case 5: k = k_mmv_blocks<Form, 5, 1>; rows = 1; break;
            case 6: k = k_mmv_blocks<Form, 6, 1>; rows = 1; break;
            case 7: k = k_mmv_blocks<Form, 7, 1>; rows = 1; break;
            case 8: k = k_mmv_blocks<Form, 8, 1>; rows = 1; break;
            default: abort();
        }
        launch_mmv(k, rows, ib * a.ncols, a, st);
        ++g_blocks_launches[Form::ID];
    });
}
void mmv_q8_0(const mmv_args & a, hipStream_t st)   { mmv_blocks_launch<q80_form>(a, st); }
void mmv_q4_0(const mmv_args & a, hipStream_t st)   { mmv_blocks_launch<q40_form<false>>(a, st); }
void mmv_q5_0(const mmv_args & a, hipStream_t st)   { mmv_blocks_launch<q40_form<true>>(a, st); }
void mmv_iq4_nl(const mmv_args & a, hipStream_t st) { mmv_blocks_launch<iq4nl_form>(a, st); }
void mmv_iq4_xs(const mmv_args & a, hipStream_t st) { mmv_blocks_launch<iq4xs_form>(a, st); }
void mmv_q4_1(const mmv_args & a, hipStream_t st)   { mmv_blocks_launch<q41_form<false>>(a, st); }
void mmv_q5_1(const mmv_args & a, hipStream_t st)   { mmv_blocks_launch<q41_form<true>>(a, st); }
void mmv_q2_K(const mmv_args & a, hipStream_t st)   { mmv_blocks_launch<q2k_form>(a, st); }
void mmv_q3_K(const mmv_args & a, hipStream_t st)   { mmv_blocks_launch<q3k_form>(a, st); }

// ---- MUL_MAT_ID on experts of the nine block formats (k_mmv_blocks_id): one launch per node, grid sized as mmv_id_kquant (mmvk.hip)
static long g_mmv_id_blocks_launches = 0;
long mmv_id_blocks_launches() { return g_mmv_id_blocks_launches; }
template <class Form>
static void mmv_id_blocks_launch(const mmv_id_args & a, hipStream_t st) {
    const size_t lds = Form::image_bytes(a.K);
    if (a.K < (1 << Form::LOG2W) || a.K % (1 << Form::LOG2W) != 0 || a.K > INT32_MAX || lds > MMV_LDS_MAX || a.n_ids > 65535 || a.n_tokens > 65535 || a.n_expert < 1 || a.b_ne1 < 1 ||
        a.nrows > INT32_MAX || a.as_nb1 < (size_t) (a.K >> Form::LOG2W) * Form::BYTES) {
        fprintf(stderr, "[mi355x] mmv_id_blocks: shape out of range (type %d, K=%lld, ids %lld x %lld)\n", a.type, (long long) a.K, (long long) a.n_ids, (long long) a.n_tokens); abort();
    }
    // grid.x: every row group of one pair resident at once; with many pairs it shrinks so that the whole launch stays near 4 resident rounds of 1024 workgroups --
    // each workgroup then grid-strides over the pair's row groups and stages the pair's image once
    static const int cap = [] { const char * e = getenv("MI355X_MMV_WGS"); const int c = e ? atoi(e) : 1024; return c < 1 ? 1024 : c; }();
    const int64_t pairs = a.n_ids * a.n_tokens;
    int64_t gx = ((a.nrows + 1) / 2 + 3) / 4;
    const int64_t budget = (int64_t) cap * 4 / pairs;
    if (gx > budget) gx = budget;
    if (gx < 1) gx = 1;
    mmv_blocks_id_dev d;
    d.as = (const char *) a.as; d.as_nb1 = a.as_nb1; d.as_nb2 = a.as_nb2; d.n_expert = (int) a.n_expert;
    d.ids = (const char *) a.ids; d.ids_nb0 = a.ids_nb0; d.ids_nb1 = a.ids_nb1;
    d.act = (const char *) a.act; d.b_ne1 = (int) a.b_ne1;
    d.dst = (char *) a.dst; d.dst_nb1 = a.dst_nb1; d.dst_nb2 = a.dst_nb2;
    d.K = (int) a.K; d.nrows = (int) a.nrows;
    if (lds > 64 * 1024) HIP_CHECK(hipFuncSetAttribute((const void *) k_mmv_blocks_id<Form, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds));
    k_mmv_blocks_id<Form, 2><<<dim3((unsigned) gx, (unsigned) a.n_ids, (unsigned) a.n_tokens), dim3(256), lds, st>>>(d);
    ++g_mmv_id_blocks_launches;
}
void mmv_id_blocks(const mmv_id_args & a, hipStream_t st) {
    if (a.nrows == 0 || a.n_ids == 0 || a.n_tokens == 0) return;
    switch (a.type) {
        case GGML_TYPE_Q8_0:   mmv_id_blocks_launch<q80_form>(a, st); break;
        case GGML_TYPE_Q4_0:   mmv_id_blocks_launch<q40_form<false>>(a, st); break;
        case GGML_TYPE_Q5_0:   mmv_id_blocks_launch<q40_form<true>>(a, st); break;
        case GGML_TYPE_IQ4_NL: mmv_id_blocks_launch<iq4nl_form>(a, st); break;
        case GGML_TYPE_IQ4_XS: mmv_id_blocks_launch<iq4xs_form>(a, st); break;
        case GGML_TYPE_Q4_1:   mmv_id_blocks_launch<q41_form<false>>(a, st); break;
        case GGML_TYPE_Q5_1:   mmv_id_blocks_launch<q41_form<true>>(a, st); break;
        case GGML_TYPE_Q2_K:   mmv_id_blocks_launch<q2k_form>(a, st); break;
        case GGML_TYPE_Q3_K:   mmv_id_blocks_launch<q3k_form>(a, st); break;
        default: fprintf(stderr, "[mi355x] mmv_id_blocks: type %d is none of the nine block formats\n", a.type); abort();
    }
}

#define MMVF_LAUNCH(NC, ROWS, WF16)                                                                                    \
    do {                                                                                                               \
        const size_t ldsb = arow * (NC);                                                                               \
        if (ldsb > 64 * 1024) HIP_CHECK(hipFuncSetAttribute((const void *) k_mmv_f<NC, ROWS, WF16>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) ldsb));                              \
        k_mmv_f<NC, ROWS, WF16><<<dim3(grid_for(a.nrows, ROWS), (unsigned) a.nbatch), dim3(256), ldsb, st>>>(          \
            (const char *) a.W, a.w_rs, (const char *) a.act, a.act_cs, (char *) a.dst, a.dst_cs, (int) a.K, (int) a.nrows, bt); \
    } while (0)

template <bool WF16>
static void mmv_float(const mmv_args & a0, hipStream_t st) {
    if (a0.nrows == 0 || a0.ncols == 0) return;
    const size_t arow = ((size_t) a0.K * (WF16 ? 2 : 4) + 15) & ~(size_t) 15;
    const mmv_batch bt = { a0.nbatch > 1 ? a0.ne12 : 1, a0.nbatch > 1 ? a0.r2 : 1, a0.nbatch > 1 ? a0.r3 : 1, a0.w_nb2, a0.w_nb3, a0.act_bs, a0.dst_nb2, a0.dst_nb3 };
    split_cols(a0, arow, [&](const mmv_args & a) {
        switch (a.ncols) {
            case 1: MMVF_LAUNCH(1, 2, WF16); break;
            case 2: MMVF_LAUNCH(2, 2, WF16); break;
            case 3: MMVF_LAUNCH(3, 1, WF16); break;
            case 4: MMVF_LAUNCH(4, 1, WF16); break;
            case 5: MMVF_LAUNCH(5, 1, WF16); break;
            case 6: MMVF_LAUNCH(6, 1, WF16); break;
            case 7: MMVF_LAUNCH(7, 1, WF16); break;
            case 8: MMVF_LAUNCH(8, 1, WF16); break;
            default: abort();
        }
    });
}
void mmv_f16(const mmv_args & a, hipStream_t st) { mmv_float<true>(a, st); }
void mmv_f32(const mmv_args & a, hipStream_t st) { mmv_float<false>(a, st); }

} // namespace mi
