// Rate prediction for gfx950: the size of a chunk's .alc at every quality, before any rANS chain runs.
//
// Only the dead-zone quantiser depends on the quality; the transform does not.  For 8-bit RGB every coefficient lies in
// [-2048, 2048) (transform.hip, kQLutR), so one 4096-bin histogram of the UNQUANTISED coefficients per channel
// (fwd_t_bins_kernel on the tile path, coef_hist_kernel on the generic path) determines the symbol histogram of every
// step: fold_kernel relabels the bins through the encoder's own value -> symbol map (quant_sym1).  cost_kernel then
// builds the reference table of each folded histogram (freq_table_256, the code the encoder's table kernel runs),
// classifies it and brackets the stream length.  split_cost_kernel does the same for the split-stream container, with that
// format's normalisation rule and per-lane overheads, and wide_cost_kernel for the wide container (.alc v3) over the
// histograms of fold_kernel<true>: the coded symbol min(z, 255), with the 12-bit residual of every escape priced in.
//
// The bracket (per channel; n = number of symbols, f = a symbol's table frequency, encoder of src/rans.rs:244-308):
//   The state starts at x0 = 2^23.  Before a symbol it is renormalised (x >>= 8, one byte out, while x >= f * 2^19) and
//   then x' = floor(x / f) * 4096 + x mod f + cum.  A table is BOUNDED when every present symbol has 1 <= f <= 4096; let
//   e = max(0, cum + f - 4096) over the present symbols (the reference's freq-1 floor for empty bins lets the cums run past
//   4096: e > 0 for most tables of real chunks, so the bracket must cover it).  Then:
//   * every state a symbol starts from is >= 2^23 (induction: x' >= 4096 * floor(x / f) >= 2^23 when x >= f * 2^11), so
//     x >= min(2^23, f * 2^11) = f * 2^11 whenever it is divided, and x' < 2^31 + e < 2^32;
//   * with x = q f + r (r < f): x' >= 4096 q > (4096 / f)(x - f) and x' <= 4096 q + 4095 + e < (4096 / f)(x + f) + e, so
//     one symbol multiplies the state by (4096 / f)(1 + d) with -2^-11 < d < 2^-11 + e 2^-23 (f / x <= 2^-11, e f / (4096 x)
//     <= e 2^-23);
//   * a byte out divides the state by 256 and drops at most 255 / x <= 255 / 2^19 < 2^-11 of it (x >= f * 2^19 there):
//     log2 loss in [8, 8 - log2(1 - 2^-11)];
//   * finish() writes the final state, in [2^23, 2^31 + e), as 4 bytes.
//   With M = sum over symbols of log2(4096 / f), E bytes emitted and x_end the final state:
//     log2(x_end) - 23 = growth - loss, 0 <= log2(x_end) - 23 < 8 (< 9 when e > 0), so
//     8 E <= loss <= M + n u                      ->  bytes <= (M + n u) / 8 + 4,   u = log2(1 + 2^-11 + e 2^-23)
//     (8 - log2(1 - 2^-11)) E >= loss > M + n log2(1 - 2^-11) - 8 (- 9 when e > 0)
//                                                 ->  bytes >= (M + n log2(1 - 2^-11) - 8) / (8 - log2(1 - 2^-11)) + 4
//   All of it in integers: M is summed in 2^-24 bit units from a per-frequency table of log2(4096 / f) rounded down (lower
//   bound) and up (upper bound); the log2(1 +- 2^-11) terms are rounded away from the bound they feed, and for e > 0,
//   u <= (2^-11 + e 2^-23) / ln 2 < (8192 + 2 e) * 1.4427 units of 2^-24.  12 bits per symbol x 2^32 symbols x 2^24 stays
//   below 2^60.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "freq_table.h"
#include "kernels.h"
#include "split_norm.h"
#include "symbols.h"

namespace alice {

// Generic path: bins of one channel's i32 coefficient volume (same range and out-of-range counter as fwd_t_bins_kernel).
__global__ __launch_bounds__(256) void coef_hist_kernel(const int32_t* __restrict__ v, uint64_t n, uint32_t qr,
                                                        uint32_t* __restrict__ bins, uint32_t* __restrict__ oor) {
    __shared__ uint32_t lb[4096];
    for (uint32_t i = threadIdx.x; i < 2u * qr; i += 256u) lb[i] = 0u;
    __syncthreads();
    uint32_t out = 0u;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) {
        const uint32_t u = (uint32_t)v[i] + qr;
        if (u < 2u * qr) atomicAdd(&lb[u], 1u);
        else ++out;
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < 2u * qr; i += 256u)
        if (lb[i]) atomicAdd(&bins[i], lb[i]);
    if (out) atomicAdd(oor, out);
}

void launch_coef_hist(const int32_t* d_vol, uint64_t n, uint32_t* d_bins, uint32_t* d_oor, hipStream_t st) {
    const uint64_t blocks = std::min<uint64_t>((n + 255) / 256, 1024);
    hipLaunchKernelGGL(coef_hist_kernel, dim3((unsigned)std::max<uint64_t>(blocks, 1)), dim3(256), 0, st, d_vol, n,
                       (uint32_t)value_table_radius(), d_bins, d_oor);
}

// One workgroup per (chunk, channel, step - 1): step_hist[((chunk * 64 + step - 1) * 3 + ch) * 256 + symbol].  Chunks with
// out-of-range coefficients are skipped (the host fills their histograms from real forward passes).
// WIDE: the coded symbol of .alc v3, min(z, 255) with z the untruncated zigzag (quant_sym1_wide); bin 255 counts the escapes.
template <bool WIDE>
__global__ __launch_bounds__(256) void fold_kernel(const uint32_t* __restrict__ bins, const uint32_t* __restrict__ oor,
                                                   uint32_t qr, uint32_t* __restrict__ step_hist) {
    __shared__ uint32_t sh[256];
    const uint32_t chunk = blockIdx.x / 192u, ch = (blockIdx.x / 64u) % 3u, step = blockIdx.x % 64u + 1u;
    if (oor[chunk]) return;
    const uint32_t tid = threadIdx.x;
    sh[tid] = 0u;
    __syncthreads();
    const uint32_t hdz = step / 2u;
    const uint32_t magic = step == 1u ? 0u : (uint32_t)(((1ull << 32) + step - 1u) / step);
    const uint32_t* b = bins + ((size_t)chunk * 3 + ch) * 4096;
    for (uint32_t i = tid; i < 2u * qr; i += 256u) {
        const uint32_t c = b[i];
        if (!c) continue;
        const int val = (int)i - (int)qr;
        uint32_t s;
        if (WIDE) s = min(step == 1u ? quant_sym1_wide<true>(val, hdz, magic) : quant_sym1_wide<false>(val, hdz, magic), 255u);
        else s = step == 1u ? quant_sym1<true>(val, hdz, magic) : quant_sym1<false>(val, hdz, magic);
        atomicAdd(&sh[s], c);
    }
    __syncthreads();
    step_hist[(((size_t)chunk * 64 + step - 1u) * 3 + ch) * 256 + tid] = sh[tid];
}

// One workgroup per (chunk, channel, step - 1): the reference table of the step's histogram, its class and the bracket.
__global__ __launch_bounds__(256) void cost_kernel(const uint32_t* __restrict__ step_hist, const uint32_t* __restrict__ log_lo,
                                                   const uint32_t* __restrict__ log_hi, uint32_t g_up, uint32_t g_dn,
                                                   RateChannel* __restrict__ out) {
    __shared__ uint32_t scratch[768];
    __shared__ unsigned long long sum[3];
    __shared__ uint32_t cls, excess;
    const uint32_t s = threadIdx.x;
    const uint32_t count = step_hist[(size_t)blockIdx.x * 256 + s];
    if (s == 0) { sum[0] = sum[1] = sum[2] = 0ull; cls = kRateBounded; excess = 0u; }
    uint32_t f, c;
    freq_table_256(count, 256u, scratch, f, c);   // (its barriers order the initialisation above)
    if (count) {
        if (f == 0u) atomicMax(&cls, (uint32_t)kRateDiverges);
        else if (f > kProbScale) atomicMax(&cls, (uint32_t)kRateUnbounded);
        else {
            if (c + f > kProbScale) atomicMax(&excess, c + f - kProbScale);
            atomicAdd(&sum[0], (unsigned long long)count * log_lo[f]);
            atomicAdd(&sum[1], (unsigned long long)count * log_hi[f]);
        }
        atomicAdd(&sum[2], (unsigned long long)count);
    }
    __syncthreads();
    if (s == 0) {
        RateChannel r{};
        r.status = cls;
        if (cls == kRateBounded) {
            const unsigned long long n = sum[2], one = 1ull << kRateFracBits;
            const unsigned long long up = excess ? ((8192ull + 2ull * excess) * 14427ull + 9999ull) / 10000ull : g_up;
            r.hi = (sum[1] + n * up) / (8ull * one) + 4ull;
            const unsigned long long sub = n * g_dn + (excess ? 9ull : 8ull) * one;
            r.lo = (sum[0] > sub ? (sum[0] - sub + 8ull * one + g_dn - 1ull) / (8ull * one + g_dn) : 0ull) + 4ull;
        }
        out[blockIdx.x] = r;
    }
}

// The same for the split-stream container (.alc v2): one workgroup per (chunk, channel, step - 1).  The table
// is the one split_table_kernel stores (split_normalize_256): it sums to exactly 4096, so every lane of the payload is a chain
// of the argument above with e = 0, starting at 2^23 and ending in four state bytes.  With n symbols in B blocks of 64 * L,
// K lanes that own a symbol, M / u / g as above, the lane bounds add up to
//   sum of lane bytes <= (M + n u) / 8 + 4 K        sum of lane bytes > (M - n g - 8 K) / (8 + g) + 4 K
// and the payload adds 4 bytes of block length and a 128-byte lane directory per block.  No table is unbounded: a present
// symbol has 1 <= f <= 4096.  K <= n <= 2^32: 8 K 2^24 and n g stay below 2^60.
__global__ __launch_bounds__(256) void split_cost_kernel(const uint32_t* __restrict__ step_hist, const uint32_t* __restrict__ log_lo,
                                                         const uint32_t* __restrict__ log_hi, uint32_t g_up, uint32_t g_dn,
                                                         uint32_t lane_symbols, RateChannel* __restrict__ out) {
    __shared__ unsigned long long red64[4];
    __shared__ uint32_t red32[4];
    const uint32_t count = step_hist[(size_t)blockIdx.x * 256 + threadIdx.x];
    unsigned long long n;
    const uint32_t f = split_normalize_256(count, red64, red32, n);
    const unsigned long long s_lo = block_sum_256(count ? (unsigned long long)count * log_lo[f] : 0ull, red64);
    const unsigned long long s_hi = block_sum_256(count ? (unsigned long long)count * log_hi[f] : 0ull, red64);
    if (threadIdx.x == 0) {
        RateChannel r{};
        r.status = kRateBounded;
        if (n) {
            const unsigned long long one = 1ull << kRateFracBits, per_block = 64ull * lane_symbols;
            const unsigned long long blocks = (n + per_block - 1ull) / per_block;
            const unsigned long long last = n - (blocks - 1ull) * per_block;   // symbols of the last block, >= 1
            const unsigned long long lanes = 64ull * (blocks - 1ull) + (last < 64ull ? last : 64ull);
            const unsigned long long fixed = 132ull * blocks + 4ull * lanes;
            r.hi = fixed + (s_hi + n * g_up) / (8ull * one);
            const unsigned long long sub = n * g_dn + 8ull * lanes * one;
            r.lo = fixed + (s_lo > sub ? (s_lo - sub + 8ull * one + g_dn - 1ull) / (8ull * one + g_dn) : 0ull);
        }
        out[blockIdx.x] = r;
    }
}

// The same for the wide container (.alc v3): one workgroup per (chunk, channel, step - 1) over the histogram
// of the coded symbol min(z, 255).  E = hist[255] is the number of escapes, and each escape is followed in its lane chain by
// the residual step: an ordinary step with frequency 1 and cum r (cum + f <= 4096, so e = 0) that renormalises against
// 1 * 2^19 and then sets x' = 4096 x + r with 2^11 <= x < 2^19 (11.1) -- the per-step argument at the top of this file
// with f = 1: growth (4096 / 1)(1 + d), 0 <= d < 2^-11, a byte out drops less than 2^-11 of the state.  A lane is a chain
// of n_lane + E_lane steps with e = 0, and a residual costs exactly log2(4096 / 1) = 12 bits in both table sums:
//   steps = n + E      T_lo = S_lo + 12 one E      T_hi = S_hi + 12 one E
// in split_cost_kernel's formula with steps for n in the g terms.  With E = 0 it is that kernel's bracket integer for
// integer.  Every table is bounded (1 <= f <= 4096), so there is no status array.  n <= 2^32 and E <= n give steps <= 2^33:
// T <= 12 * 2^24 * 2^33 < 2^61, steps * g < 2^33 * 2^14 and 8 K 2^24 <= 2^59, so every product and sum stays below 2^62.
__global__ __launch_bounds__(256) void wide_cost_kernel(const uint32_t* __restrict__ step_hist, const uint32_t* __restrict__ log_lo,
                                                        const uint32_t* __restrict__ log_hi, uint32_t g_up, uint32_t g_dn,
                                                        uint32_t lane_symbols, RateChannel* __restrict__ out) {
    __shared__ unsigned long long red64[4];
    __shared__ uint32_t red32[4];
    __shared__ uint32_t escapes;
    const uint32_t count = step_hist[(size_t)blockIdx.x * 256 + threadIdx.x];
    if (threadIdx.x == 255u) escapes = count;   // (the barriers of the normalisation order it before thread 0 reads)
    unsigned long long n;
    const uint32_t f = split_normalize_256(count, red64, red32, n);
    const unsigned long long s_lo = block_sum_256(count ? (unsigned long long)count * log_lo[f] : 0ull, red64);
    const unsigned long long s_hi = block_sum_256(count ? (unsigned long long)count * log_hi[f] : 0ull, red64);
    if (threadIdx.x == 0) {
        RateChannel r{};
        r.status = kRateBounded;
        if (n) {
            const unsigned long long one = 1ull << kRateFracBits, per_block = 64ull * lane_symbols;
            const unsigned long long blocks = (n + per_block - 1ull) / per_block;
            const unsigned long long last = n - (blocks - 1ull) * per_block;   // symbols of the last block, >= 1
            const unsigned long long lanes = 64ull * (blocks - 1ull) + (last < 64ull ? last : 64ull);
            const unsigned long long fixed = 132ull * blocks + 4ull * lanes;
            const unsigned long long e = escapes, steps = n + e;
            const unsigned long long t_lo = s_lo + 12ull * one * e, t_hi = s_hi + 12ull * one * e;
            r.hi = fixed + (t_hi + steps * g_up) / (8ull * one);
            const unsigned long long sub = steps * g_dn + 8ull * lanes * one;
            r.lo = fixed + (t_lo > sub ? (t_lo - sub + 8ull * one + g_dn - 1ull) / (8ull * one + g_dn) : 0ull);
        }
        out[blockIdx.x] = r;
    }
}

void launch_rate_fold(const uint32_t* d_bins, const uint32_t* d_oor, uint32_t n_chunks, uint32_t* d_step_hist, hipStream_t st) {
    hipLaunchKernelGGL(fold_kernel<false>, dim3(n_chunks * 192u), dim3(256), 0, st, d_bins, d_oor, (uint32_t)value_table_radius(), d_step_hist);
}

void launch_rate_fold_wide(const uint32_t* d_bins, const uint32_t* d_oor, uint32_t n_chunks, uint32_t* d_step_hist, hipStream_t st) {
    hipLaunchKernelGGL(fold_kernel<true>, dim3(n_chunks * 192u), dim3(256), 0, st, d_bins, d_oor, (uint32_t)value_table_radius(), d_step_hist);
}

void launch_rate_cost(const uint32_t* d_step_hist, const uint32_t* d_log, uint32_t n_chunks, RateChannel* d_out, hipStream_t st) {
    const RateLogTable& t = rate_log_table();
    hipLaunchKernelGGL(cost_kernel, dim3(n_chunks * 192u), dim3(256), 0, st, d_step_hist, d_log, d_log + (kProbScale + 1),
                       t.g_up, t.g_dn, d_out);
}

void launch_split_rate_cost(const uint32_t* d_step_hist, const uint32_t* d_log, uint32_t n_chunks, uint32_t lane_symbols,
                            RateChannel* d_out, hipStream_t st) {
    const RateLogTable& t = rate_log_table();
    hipLaunchKernelGGL(split_cost_kernel, dim3(n_chunks * 192u), dim3(256), 0, st, d_step_hist, d_log, d_log + (kProbScale + 1),
                       t.g_up, t.g_dn, lane_symbols, d_out);
}

void launch_wide_rate_cost(const uint32_t* d_step_hist, const uint32_t* d_log, uint32_t n_chunks, uint32_t lane_symbols,
                           RateChannel* d_out, hipStream_t st) {
    const RateLogTable& t = rate_log_table();
    hipLaunchKernelGGL(wide_cost_kernel, dim3(n_chunks * 192u), dim3(256), 0, st, d_step_hist, d_log, d_log + (kProbScale + 1),
                       t.g_up, t.g_dn, lane_symbols, d_out);
}

// floor / ceil of log2(4096 / f) * 2^24 for f = 0 .. 4096 (entry 0 unused), and the two log2(1 +- 2^-11) terms rounded
// up.  log2l carries 64 mantissa bits; the values are below 2^28 and irrational unless f is a power of two (then exact),
// so the rounding direction is decided with 30+ bits to spare (the suite checks every entry at 50 digits).
const RateLogTable& rate_log_table() {
    static const RateLogTable t = [] {
        RateLogTable r{};
        const long double one = (long double)(1u << kRateFracBits);
        for (uint32_t f = 1; f <= kProbScale; ++f) {
            if ((f & (f - 1u)) == 0u) {
                r.lo[f] = r.hi[f] = (uint32_t)(kProbBits - (31 - __builtin_clz(f))) << kRateFracBits;
            } else {
                const long double v = log2l((long double)kProbScale / (long double)f) * one;
                r.lo[f] = (uint32_t)floorl(v);
                r.hi[f] = r.lo[f] + 1u;
            }
        }
        r.g_up = (uint32_t)ceill(log2l(1.0L + ldexpl(1.0L, -11)) * one);
        r.g_dn = (uint32_t)ceill(-log2l(1.0L - ldexpl(1.0L, -11)) * one);
        return r;
    }();
    return t;
}

}  // namespace alice
