// Quantizer::quantize + to_symbols for one coefficient on the device, shared by the forward temporal kernel
// (transform.hip) and the rate prediction's fold (rate.hip), so both map a value to the same symbol.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace alice {

__device__ __forceinline__ uint32_t sat_sub_u32(uint32_t a, uint32_t b) { return __builtin_elementwise_sub_sat(a, b); }

// Quantizer::quantize (src/quant.rs:89-97, dead zone = step) followed by to_symbols (:555-560); hdz = step / 2,
// magic = ceil(2^32 / step) (see quant_sym4 in transform.hip for the derivation).
template <bool STEP1>
__device__ __forceinline__ uint32_t quant_sym1(int val, uint32_t hdz, uint32_t magic) {
    const uint32_t mag = (uint32_t)max(val, -val);
    const uint32_t adj = sat_sub_u32(mag, hdz);
    const uint32_t q = STEP1 ? adj : __umulhi(adj, magic);
    return sat_sub_u32((q << 1) + ((uint32_t)val >> 31), 1u) & 0xFFu;
}

// The wide symbol of .alc v3: quant_sym1 without its `& 0xFF`, clamped at 65535 -- the untruncated
// zigzag z.  Derived from quant_sym4_wide in transform.hip (the map the wide forward pass stores), one value at a time: the
// same operations in the same order, so the fold of the rate prediction (rate.hip) and the encoder cannot disagree.
template <bool STEP1>
__device__ __forceinline__ uint32_t quant_sym1_wide(int val, uint32_t hdz, uint32_t magic) {
    const uint32_t mag = (uint32_t)max(val, -val);
    const uint32_t adj = sat_sub_u32(mag, hdz);
    const uint32_t q = STEP1 ? adj : __umulhi(adj, magic);
    return min(sat_sub_u32((q << 1) + ((uint32_t)val >> 31), 1u), 65535u);
}

}  // namespace alice
