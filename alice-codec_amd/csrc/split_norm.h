// Rule 10.2 of the split-stream format as one device function, shared by the table kernel that
// encodes (split.hip) and the cost kernel that predicts (rate.hip): the predicted table is the encoded one by construction.
#pragma once

#include "common.h"

namespace alice {

// max over the 256 threads of a block; red: 4 u32 of LDS
__device__ __forceinline__ uint32_t block_max_256(uint32_t v, uint32_t* red) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const uint32_t a = red[0] > red[1] ? red[0] : red[1], b = red[2] > red[3] ? red[2] : red[3];
    return a > b ? a : b;
}

__device__ __forceinline__ unsigned long long block_sum_256(unsigned long long v, unsigned long long* red) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// Normalisation: freq = max(1, floor(count * 4096 / total)) for a present symbol, 0 for an absent one;
// a short sum gives the whole deficit to the largest frequency (lowest symbol on ties); a sum that is over takes one at
// a time from the currently largest frequency (lowest symbol on ties).  The excess is at most the number of symbols the
// floor of 1 lifted, so the loop runs at most 255 rounds.  Called by all 256 threads of a workgroup, thread s with the
// count of symbol s; returns the symbol's frequency and the histogram's total.  red64 / red32: 4 entries of LDS each.
__device__ __forceinline__ uint32_t split_normalize_256(uint32_t count, unsigned long long* red64, uint32_t* red32,
                                                        unsigned long long& total) {
    const int s = threadIdx.x;
    total = block_sum_256(count, red64);
    uint32_t f = 0u;
    if (count) {
        f = (uint32_t)(((unsigned long long)count << kProbBits) / total);
        if (f < 1u) f = 1u;
    }
    if (total) {
        uint32_t sum = (uint32_t)block_sum_256(f, red64);
        // key: larger frequency first, then the lower symbol
        uint32_t top = block_max_256((f << 8) | (255u - (uint32_t)s), red32);
        if (sum < kProbScale) {
            if (255u - (top & 255u) == (uint32_t)s) f += kProbScale - sum;
        } else {
            while (sum > kProbScale) {   // uniform across the block
                if (255u - (top & 255u) == (uint32_t)s) f -= 1u;
                sum -= 1u;
                top = block_max_256((f << 8) | (255u - (uint32_t)s), red32);
            }
        }
    }
    return f;
}

}  // namespace alice
