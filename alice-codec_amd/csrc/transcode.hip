// Transcode of .alc v2-v4 symbols to a coarser quantiser step: the map of one symbol, and the two
// bandwidth kernels around it.  Nothing here touches pixels or coefficients: a symbol is a function of the quantised
// coefficient alone, so a coarser chunk is made from the decoded symbols.
//
// The map, with source step s1 and target step s2 > s1:
//   q1 = what the container's decoder makes of the symbol (|q1| = (z + 1) >> 1, negative for an even z > 0)
//   m  = 0 for q1 = 0, else sign(q1) * (|q1| * s1 + s1 / 2 + s1 / 2): the centre of the interval the encoder's quantiser
//        (q = (|v| - s1 / 2) / s1) maps to q1, not the decoder's q1 * s1, which is the interval's lower end less s1 / 2
//   q2 = the encoder's own quantiser of m at s2 (quant_sym1 / quant_sym1_wide: the same operations in the same order)
// |q2| <= |q1|, so no symbol leaves the range of the one it replaces.  s2 <= s1 is the identity.
#include <algorithm>
#include <type_traits>

#include "common.h"
#include "kernels.h"
#include "symbols.h"

namespace alice {

struct RequantMap {
    uint32_t s1, off;      // source step, s1 / 2 + s1 / 2
    uint32_t hdz, magic;   // of the target step: s2 / 2, ceil(2^32 / s2); magic == 0: the identity (target not coarser)
};

static RequantMap requant_map(int32_t step_from, int32_t step_to) {
    RequantMap p{};
    p.s1 = (uint32_t)step_from; p.off = 2u * ((uint32_t)step_from / 2u);
    if (step_to > step_from) {   // step_to >= 2: the reciprocal fits 32 bits
        p.hdz = (uint32_t)step_to / 2u;
        p.magic = (uint32_t)(((1ull << 32) + (uint32_t)step_to - 1u) / (uint32_t)step_to);
    }
    return p;
}

// |m| of a symbol: at most 32768 * 64 + 64 < 2^22 for any u16, far inside the range where umulhi(adj, magic) is adj / s2
__device__ __forceinline__ uint32_t symbol_centre(uint32_t z, uint32_t s1, uint32_t off) {
    const uint32_t a = (z + 1u) >> 1;
    return a ? a * s1 + off : 0u;
}

template <bool WIDE>
__device__ __forceinline__ uint32_t requant_sym1(uint32_t z, const RequantMap& p) {
    if (p.magic == 0u) return z;
    const uint32_t m = symbol_centre(z, p.s1, p.off);
    const uint32_t neg = (z & 1u) ^ 1u;                     // an even z is a negative coefficient (z = 0: m = 0 below)
    const uint32_t q = __umulhi(sat_sub_u32(m, p.hdz), p.magic);
    const uint32_t t = sat_sub_u32((q << 1) + neg, 1u);     // quant_sym1's last line with the sign bit of m
    return WIDE ? min(t, 65535u) : (t & 0xFFu);
}

// How n elements of E bytes at src (and dst) split into an element run up to the first 16-byte boundary of dst, 16-byte
// vectors, and an element run at the end.  Vectors need src and dst to share their offset inside 16 bytes; otherwise every
// element takes the element path.
struct VecSplit { unsigned long long head, nvec, tail0; };
template <int E>
__device__ __forceinline__ VecSplit vec_split(const void* src, const void* dst, unsigned long long n) {
    const uintptr_t sa = (uintptr_t)src, da = (uintptr_t)dst;
    VecSplit s;
    s.head = n;
    if (((sa ^ da) & 15u) == 0u) s.head = min((unsigned long long)(((16u - (unsigned)(da & 15u)) & 15u) / E), n);
    s.nvec = (n - s.head) / (16 / E);
    s.tail0 = s.head + s.nvec * (16 / E);
    return s;
}

constexpr int kRequantReplicas = 8;   // copies of the 256 counters: word = symbol * 8 + (lane & 7), as in fwd_t_kernel

// n symbols (u8, WIDE: u16) from src to dst -- the same address, or buffers that do not overlap -- through the map, and the
// 256-bin histogram of the coded symbol (WIDE: min(z, 255)) added to hist (may be null).  Any base alignment of the element
// type.  Version 2 maps through a 256-entry table the workgroup builds from the map itself; wide symbols take the
// arithmetic (65536 entries do not fit, and 8 KB for the symbols below the escape would cost the histogram its replicas:
// fwd_t_wide_kernel made the same choice).  Zero, the dominant symbol, is counted in a register.
template <bool WIDE>
__global__ __launch_bounds__(256) void requant_symbols_kernel(const uint8_t* src, uint8_t* dst, unsigned long long n, RequantMap p,
                                                              uint32_t* __restrict__ hist) {
    using T = typename std::conditional<WIDE, uint16_t, uint8_t>::type;
    constexpr int E = (int)sizeof(T);
    __shared__ uint32_t lh[kRequantReplicas * 256];
    __shared__ uint8_t lut[256];
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < kRequantReplicas * 256u; i += 256u) lh[i] = 0u;
    if (!WIDE) lut[tid] = (uint8_t)requant_sym1<false>(tid, p);
    __syncthreads();
    const uint32_t rep = tid & (kRequantReplicas - 1);
    uint32_t zeros = 0u;
    auto one = [&](uint32_t z) -> uint32_t {
        const uint32_t t = WIDE ? requant_sym1<true>(z, p) : (uint32_t)lut[z];
        const uint32_t c = WIDE ? min(t, 255u) : t;
        if (c) atomicAdd(&lh[c * kRequantReplicas + rep], 1u); else ++zeros;
        return t;
    };
    const VecSplit s = vec_split<E>(src, dst, n);
    const unsigned long long g = (unsigned long long)blockIdx.x * 256u + tid, stride = (unsigned long long)gridDim.x * 256u;
    const uint4* sv = (const uint4*)(src + s.head * E);
    uint4* dv = (uint4*)(dst + s.head * E);
    for (unsigned long long v = g; v < s.nvec; v += stride) {
        const uint4 q = sv[v];
        uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (WIDE) {
                const uint32_t lo = one(w[k] & 0xFFFFu), hi = one(w[k] >> 16);
                w[k] = lo | (hi << 16);
            } else {
                uint32_t r = 0u;
#pragma unroll
                for (int b = 0; b < 4; ++b) r |= one((w[k] >> (8 * b)) & 0xFFu) << (8 * b);
                w[k] = r;
            }
        }
        dv[v] = make_uint4(w[0], w[1], w[2], w[3]);
    }
    // the elements before the first and behind the last vector
    const unsigned long long n_edge = s.head + (n - s.tail0);
    for (unsigned long long e = g; e < n_edge; e += stride) {
        const unsigned long long i = e < s.head ? e : s.tail0 + (e - s.head);
        ((T*)dst)[i] = (T)one(((const T*)src)[i]);
    }
    if (zeros) atomicAdd(&lh[rep], zeros);
    __syncthreads();
    if (!hist) return;
    uint32_t cnt = 0u;
#pragma unroll
    for (int r = 0; r < kRequantReplicas; ++r) cnt += lh[tid * kRequantReplicas + ((r + tid) & (kRequantReplicas - 1))];
    if (cnt) atomicAdd(&hist[tid], cnt);
}

// Workgroups of the two kernels: one per 256 vectors up to the cap of the histogram launches; further trips stride
static unsigned symbol_grid(uint64_t n, int elem_bytes) {
    return std::min(generic_grid_for(n / (16 / elem_bytes) + 32), 2048u);
}

void launch_requant_symbols(const void* d_src, void* d_dst, uint64_t n, bool wide, int32_t step_from, int32_t step_to,
                            uint32_t* d_hist, hipStream_t st) {
    if (!n) return;
    const RequantMap p = requant_map(step_from, step_to);
    if (wide) hipLaunchKernelGGL(requant_symbols_kernel<true>, dim3(symbol_grid(n, 2)), dim3(256), 0, st, (const uint8_t*)d_src,
                                 (uint8_t*)d_dst, (unsigned long long)n, p, d_hist);
    else hipLaunchKernelGGL(requant_symbols_kernel<false>, dim3(symbol_grid(n, 1)), dim3(256), 0, st, (const uint8_t*)d_src,
                            (uint8_t*)d_dst, (unsigned long long)n, p, d_hist);
}

// The twin of coef_hist_kernel for the size prediction of a transcode: the bins of m (the value the map quantises) of one
// channel's symbols, bins[m + qr] for m in [-qr, qr), everything else in *oor.  No stores of symbols.
template <bool WIDE>
__global__ __launch_bounds__(256) void symbol_bins_kernel(const uint8_t* __restrict__ sym, unsigned long long n, uint32_t s1, uint32_t off,
                                                          uint32_t qr, uint32_t* __restrict__ bins, uint32_t* __restrict__ oor) {
    using T = typename std::conditional<WIDE, uint16_t, uint8_t>::type;
    constexpr int E = (int)sizeof(T);
    __shared__ uint32_t lb[4096];
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < 2u * qr; i += 256u) lb[i] = 0u;
    __syncthreads();
    uint32_t out = 0u, zeros = 0u;
    auto one = [&](uint32_t z) {
        if (!z) { ++zeros; return; }
        const uint32_t m = symbol_centre(z, s1, off);
        const uint32_t u = ((z & 1u) ? m : 0u - m) + qr;
        if (u < 2u * qr) atomicAdd(&lb[u], 1u); else ++out;
    };
    const VecSplit s = vec_split<E>(sym, sym, n);
    const unsigned long long g = (unsigned long long)blockIdx.x * 256u + tid, stride = (unsigned long long)gridDim.x * 256u;
    const uint4* sv = (const uint4*)(sym + s.head * E);
    for (unsigned long long v = g; v < s.nvec; v += stride) {
        const uint4 q = sv[v];
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (WIDE) { one(w[k] & 0xFFFFu); one(w[k] >> 16); }
            else {
#pragma unroll
                for (int b = 0; b < 4; ++b) one((w[k] >> (8 * b)) & 0xFFu);
            }
        }
    }
    const unsigned long long n_edge = s.head + (n - s.tail0);
    for (unsigned long long e = g; e < n_edge; e += stride) one(((const T*)sym)[e < s.head ? e : s.tail0 + (e - s.head)]);
    if (zeros) atomicAdd(&lb[qr], zeros);
    __syncthreads();
    for (uint32_t i = tid; i < 2u * qr; i += 256u)
        if (lb[i]) atomicAdd(&bins[i], lb[i]);
    if (out) atomicAdd(oor, out);
}

void launch_symbol_bins(const void* d_sym, uint64_t n, bool wide, int32_t step_from, uint32_t* d_bins, uint32_t* d_oor, hipStream_t st) {
    if (!n) return;
    const RequantMap p = requant_map(step_from, step_from);
    const uint32_t qr = (uint32_t)value_table_radius();
    if (wide) hipLaunchKernelGGL(symbol_bins_kernel<true>, dim3(std::min(symbol_grid(n, 2), 1024u)), dim3(256), 0, st, (const uint8_t*)d_sym,
                                 (unsigned long long)n, p.s1, p.off, qr, d_bins, d_oor);
    else hipLaunchKernelGGL(symbol_bins_kernel<false>, dim3(std::min(symbol_grid(n, 1), 1024u)), dim3(256), 0, st, (const uint8_t*)d_sym,
                            (unsigned long long)n, p.s1, p.off, qr, d_bins, d_oor);
}

// The rows of a chunk's step histograms at which a channel would be left untouched (step <= its source step): the source's
// own coded histogram instead of the fold's.  One workgroup per (step - 1, channel) of step_hist[step - 1][channel][256].
struct KeptRows { int32_t s1[3]; };
__global__ __launch_bounds__(256) void kept_rows_kernel(const uint32_t* __restrict__ src_hist, KeptRows k, uint32_t* __restrict__ step_hist) {
    const uint32_t step = blockIdx.x / 3u + 1u, ch = blockIdx.x % 3u;
    if ((int32_t)step > k.s1[ch]) return;
    step_hist[(size_t)blockIdx.x * 256 + threadIdx.x] = src_hist[ch * 256 + threadIdx.x];
}

void launch_kept_rows(const uint32_t* d_src_hist, const int32_t step_from[3], uint32_t* d_step_hist, hipStream_t st) {
    const KeptRows k{{step_from[0], step_from[1], step_from[2]}};
    hipLaunchKernelGGL(kept_rows_kernel, dim3(192), dim3(256), 0, st, d_src_hist, k, d_step_hist);
}

}  // namespace alice
