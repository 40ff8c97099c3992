// mxfp4_dev.hpp -- what the two MXFP4 kernels share (mmv_mxfp4.hip: the per-pair mat-vec, mmq_id.hip: the expert-grouped int8-MFMA kernel): the 16-entry
// int8 table look-up of kvalues_mxfp4 (ggml-common.h:1094) and half the E8M0 block scale (ggml_e8m0_to_fp32_half, ggml-impl.h:471-489).
#pragma once
#include "../kernels.hpp"

namespace mi {

// four 4-bit indices (one in the low nibble of each byte, upper nibbles zero) -> four int8 values of kvalues_mxfp4: two byte permutes over the low and the
// high 8-byte half of the table and a per-byte select on index bit 3, as iq4nl_lut4 (mmvq.hip) with the other four table dwords
static __device__ __forceinline__ uint32_t mxfp4_lut4(uint32_t n) {
    const uint32_t T0 = 0x03020100u, T1 = 0x0C080604u, T2 = 0xFDFEFF00u, T3 = 0xF4F8FAFCu;   // 0 1 2 3 | 4 6 8 12 | 0 -1 -2 -3 | -4 -6 -8 -12
    const uint32_t i  = n & 0x07070707u;
    const uint32_t lo = __builtin_amdgcn_perm(T1, T0, i);                 // selector byte k < 4: byte k of T0, 4..7: byte k - 4 of T1
    const uint32_t hi = __builtin_amdgcn_perm(T3, T2, i);
    uint32_t m = (n >> 3) & 0x01010101u;
    m = (m << 8) - m;                                                     // 0xFF in every byte whose index is >= 8 (no borrow crosses a byte)
    return (hi & m) | (lo & ~m);
}
// half the E8M0 scale, built in integers as the reference does: e < 2 is an f32 denormal (2^-128, 2^-127) and is kept (f32 denormals are on in every kernel here)
static __device__ __forceinline__ float e8m0_half(uint32_t e) {
    const uint32_t bits = e < 2 ? 0x00200000u << e : (e - 1) << 23;
    return __uint_as_float(bits);
}

} // namespace mi
