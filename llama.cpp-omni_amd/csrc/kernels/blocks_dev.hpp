// blocks_dev.hpp -- what the mat-vec Forms of the 32-weight block formats (mmvq.hip) and the expert-grouped int8-MFMA kernel on the same blocks (mmq_id.hip)
// share: the fifth-bit spread of Q5_0 / Q5_1 and the IQ4_NL table look-up.
#pragma once
#include "../kernels.hpp"

namespace mi {

// fifth bits of 4 consecutive weights (bits b .. b+3 of qh) spread into bit 4 of the four bytes of a word
static __device__ __forceinline__ uint32_t spread5(uint32_t bits) { return ((bits & 1u) | ((bits & 2u) << 7) | ((bits & 4u) << 14) | ((bits & 8u) << 21)) << 4; }

// IQ4_NL / IQ4_XS: 4-bit indices into the 16-entry int8 table kvalues_iq4nl (ggml-common.h:1088-1090).  The table lives in four dwords of registers; four indices
// become four int8 values through two byte permutes (v_perm_b32 over the low and the high 8-byte half of the table) and a per-byte select on the index's bit 3
// (v_bfi_b32), then go straight into v_dot4_i32_i8 or an int8 MFMA.
static __device__ __forceinline__ uint32_t iq4nl_lut4(uint32_t n) {      // n: four indices, one in the low nibble of each byte (upper nibbles zero)
    const uint32_t T0 = 0xBFAD9881u, T1 = 0xF6EADDCFu, T2 = 0x26190D01u, T3 = 0x71594535u;   // -127 -104 -83 -65 | -49 -35 -22 -10 | 1 13 25 38 | 53 69 89 113
    const uint32_t i  = n & 0x07070707u;
    const uint32_t lo = __builtin_amdgcn_perm(T1, T0, i);                 // selector byte k < 4: byte k of T0, 4..7: byte k - 4 of T1
    const uint32_t hi = __builtin_amdgcn_perm(T3, T2, i);
    uint32_t m = (n >> 3) & 0x01010101u;
    m = (m << 8) - m;                                                     // 0xFF in every byte whose index is >= 8 (no borrow crosses a byte)
    return (hi & m) | (lo & ~m);
}

} // namespace mi
