// FrequencyTable::from_histogram on the device (src/rans.rs:102-189), shared by the rANS table kernel (rans.hip) and the
// rate prediction's cost kernel (rate.hip), so the prediction classifies exactly the table the encoder builds.
#pragma once

#include "common.h"

namespace alice {

// Computes the reference table for a histogram of n_sym <= 256 bins (FrequencyTable::from_histogram takes any slice,
// src/rans.rs:102-104; the pipeline always passes 256).  Must be called by the first 256 threads of a block (all of
// them), s = threadIdx.x; scratch: 256+ u32 in LDS; count = 0 for s >= n_sym.
// Returns freq/cum as the reference stores them (u16 truncated); symbols s >= n_sym do not exist: freq = cum = 0.
__device__ inline void freq_table_256(uint32_t count, uint32_t n_sym, uint32_t* scratch, uint32_t& freq16, uint32_t& cum16) {
    const int s = threadIdx.x;
    const bool exists = (uint32_t)s < n_sym;
    const uint32_t last = n_sym - 1u;
    __shared__ unsigned long long total_sh;
    if (s == 0) total_sh = 0ull;
    __syncthreads();
    atomicAdd(&total_sh, (unsigned long long)count);
    __syncthreads();
    const unsigned long long total = total_sh;
    uint32_t freq;
    if (!exists) {
        freq = 0u;
    } else if (total == 0ull) {
        freq = (kProbScale / n_sym) & 0xFFFFu;  // uniform(n): src/rans.rs:159-166
    } else {
        if (count == 0u) freq = 1u;  // src/rans.rs:117-118
        else {
            unsigned long long f = ((unsigned long long)count * kProbScale) / total;  // :120
            freq = (uint32_t)(f < 1ull ? 1ull : f);
        }
    }
    // exclusive scan of freq over 256 symbols
    scratch[s] = freq;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        uint32_t v = (s >= off) ? scratch[s - off] : 0u;
        __syncthreads();
        scratch[s] += v;
        __syncthreads();
    }
    const uint32_t incl = scratch[s];
    const uint32_t nt = scratch[255];
    __syncthreads();
    uint32_t cum = incl - freq;
    if (total == 0ull) {
        // uniform: last.freq = 4096 - last.cum (src/rans.rs:169-172)
        if ((uint32_t)s == last) freq = (kProbScale - cum) & 0xFFFFu;
    } else if ((uint32_t)s == last && nt != kProbScale) {
        // src/rans.rs:128-132: wrapping cast to u16
        int32_t diff = (int32_t)kProbScale - (int32_t)nt;
        freq = (uint32_t)((int32_t)freq + diff) & 0xFFFFu;
    }
    freq16 = exists ? freq & 0xFFFFu : 0u;
    cum16 = exists ? cum & 0xFFFFu : 0u;
}

}  // namespace alice
