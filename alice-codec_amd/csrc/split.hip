// Split-stream entropy stage (.alc v2 to v4; DESIGN.md sections 10, 11, 14, 15, 16) for gfx950.
//
// A channel's symbols are cut into blocks of 64 * L consecutive symbols; inside a block lane j owns symbols j, j + 64,
// j + 128, ... and codes them as an independent rANS chain with the reference coder's parameters (32-bit state, lower
// bound 2^23, byte renormalisation, 12-bit scale; src/rans.rs:269-308, 351-371 in the reference).  One wavefront per
// block, one lane per chain: the opposite operating point to the v1 chain kernels of rans.hip -- tens of thousands of
// short chains, several wavefronts per SIMD, latency hidden by occupancy instead of by a stripped dependency chain.
//
// The chain stands once per direction: lane_encode<WIDE, kWrite> and lane_decode<WIDE>(..., store).  WIDE is the u16
// symbol with the escape step of .alc v3.  The kernels are faces of the two: a kernel chooses the block its wavefront
// takes and, when decoding, what happens to symbol i once it is known.  (split_frames_decode_kernel carries its own
// copy of the decode chain: see there.)
//   split_table_kernel    histogram -> normalised frequencies (sum exactly 4096) and their running sum
//   split_encode_kernel / split_wide_encode_kernel   <false> counts every lane's stream length, <true> writes directory
//                         and streams in place
//   split_scan_kernel     block lengths -> block offsets (encode: from the count pass; decode: from the stream, validated)
//   split_decode_kernel / split_wide_decode_kernel   every block; symbol i at the lane's own position
//   split_frames_decode_kernel<WIDE>    the blocks a frame range needs, stored as a compact volume
//   split_box_decode_kernel<WIDE, XY_HIGH>   the blocks a preview or a spatial rectangle needs: the kept runs of three axes
//   split_header_kernel / split_version_kernel   the 1630-byte container header of whole chunks
// The output is sized by counting first and writing second: the chain arithmetic runs twice, but nothing is staged in
// worst-case slots (2 bytes per symbol) and no compaction pass moves the payload again.
//
// Every store to memory is a vector store; the scalar unit only reads.
#include "common.h"
#include "kernels.h"
#include "split_norm.h"

#include <type_traits>

namespace alice {

namespace {

template <bool WIDE> using SplitSym = std::conditional_t<WIDE, uint16_t, uint8_t>;

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}

// Block b of a job (b < n_blocks): its first symbol, its symbol count, and how many of them lane `lane` owns.
struct LaneGeometry {
    unsigned long long base;
    uint32_t in_block, k;
    __device__ __forceinline__ LaneGeometry(const SplitJob& job, unsigned long long b, int lane) {
        base = b * 64ull * job.lane_symbols;
        const unsigned long long left = job.n - base;
        in_block = left < 64ull * job.lane_symbols ? (uint32_t)left : 64u * job.lane_symbols;
        k = (uint32_t)lane < in_block ? (in_block - (uint32_t)lane + 63u) / 64u : 0u;
    }
};

// The decoders' LDS tables, loaded by the 256 threads of a workgroup: the slot -> symbol map (4096 x u8) and
// freq | cum << 16 per symbol.
__device__ __forceinline__ void load_decode_tables(const RansTable* table, uint32_t* c2s_sh, uint32_t* symtab) {
    const uint32_t* src = (const uint32_t*)table->dec.c2s;
#pragma unroll
    for (int t = 0; t < 4; ++t) c2s_sh[threadIdx.x + 256 * t] = src[threadIdx.x + 256 * t];
    symtab[threadIdx.x] = table->dec.symtab[threadIdx.x];
    __syncthreads();
}

}  // namespace

// ----------------------------------------------------------------------------------
// Normalisation (the rule itself is split_normalize_256 of split_norm.h, which the size prediction of
// rate.hip calls too) and the running sum of the frequencies.  One 256-thread workgroup per table.
// ----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void split_table_kernel(const uint32_t* __restrict__ hist, uint16_t* __restrict__ freq,
                                                          uint16_t* __restrict__ cum) {
    __shared__ unsigned long long red64[4];
    __shared__ uint32_t red32[4];
    __shared__ uint32_t scan[256];
    const int s = threadIdx.x;
    const size_t t = blockIdx.x;
    unsigned long long total;
    const uint32_t f = split_normalize_256(hist[t * 256 + s], red64, red32, total);
    scan[s] = f;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const uint32_t o = s >= d ? scan[s - d] : 0u;
        __syncthreads();
        scan[s] += o;
        __syncthreads();
    }
    freq[t * 256 + s] = (uint16_t)f;
    cum[t * 256 + s] = (uint16_t)(scan[s] - f);
}

// ----------------------------------------------------------------------------------
// Encoder.  A workgroup is four wavefronts = four blocks of job blockIdx.y.  The table rows sit in LDS, 16 bytes each
// (one ds_read_b128 per symbol): xmax = freq << 19, the exact reciprocal, cum bias, and 4096 - freq with the shift.
// The chain walks a lane's symbols last to first and writes its bytes back to front, so the finished stream reads
// forward: four state bytes, most significant first, then the renormalisation bytes in the order the decoder wants them.
//
// The escape rule of the wide coder (.alc v3; u16 symbols, 128 consecutive bytes per wavefront
// step): the coded symbol is s = min(z, 255); s = 255 is an escape followed in the same chain by the residual r = z - 255
// as one uniform 12-bit step (frequency 1, cum r: xmax = 2^19, x = (x << 12) + r).  The encoder walks last to first, so
// it codes the residual BEFORE the step of symbol 255; the decoder meets them the other way round.  A residual above 4095
// cannot be coded: the count pass records it in *job.flags (kSplitWideResidual) and the host refuses the call before the
// write pass runs; the write pass masks r so that its byte count stays the counted one.
// ----------------------------------------------------------------------------------
template <bool WIDE, bool kWrite>
__device__ __forceinline__ void lane_encode(const SplitJob* jobs, uint4* rows) {
    const SplitJob job = jobs[blockIdx.y];
    {
        const RansEncEntry e = job.table->enc[threadIdx.x];
        rows[threadIdx.x] = make_uint4(e.xmax, e.rcp, e.cbias, (uint32_t)e.g | (e.rsh << 16));
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const unsigned long long b = (unsigned long long)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (b >= job.n_blocks) return;
    const LaneGeometry g(job, b, lane);
    const uint32_t k = g.k, kmax = (g.in_block + 63u) / 64u;   // kmax: lane 0's count
    const SplitSym<WIDE>* __restrict__ sym = (const SplitSym<WIDE>*)job.sym + g.base + lane;

    uint32_t len = 0u;              // bytes of this lane's stream
    uint8_t* out = nullptr;         // kWrite: one past the lane's last byte
    uint32_t acc = 0u, nacc = 0u;   // kWrite: bytes collected for the dword in progress (lowest address in the low byte)
    bool wide_bad = false;          // WIDE count pass: a residual above 4095
    if (kWrite) {
        len = job.lane_len[b * 64u + lane];
        const uint32_t incl = wave_incl_scan(len, lane);
        uint8_t* blk = job.stream + job.blk_off[b];
        blk[2 * lane] = (uint8_t)len;
        blk[2 * lane + 1] = (uint8_t)(len >> 8);
        if (lane < 4) job.stream[4ull * b + lane] = (uint8_t)(job.blk_len[b] >> (8 * lane));
        out = blk + 128u + incl;
    }
    auto put = [&](uint32_t byte) {
        if (kWrite) {
            --out;
            acc = (acc << 8) | byte;
            ++nacc;
            if (((uintptr_t)out & 3u) == 0u) {
                if (nacc == 4u) *(uint32_t*)out = acc;
                else for (uint32_t t = 0; t < nacc; ++t) out[t] = (uint8_t)(acc >> (8u * t));
                nacc = 0u;
            }
        } else {
            ++len;
        }
    };
    uint32_t x = kRansL;
    // eight symbols are loaded ahead of the chain that consumes them
    for (uint32_t hi = kmax; hi > 0u; hi = hi > 8u ? hi - 8u : 0u) {
        uint32_t s[8];
#pragma unroll
        for (uint32_t u = 0; u < 8u; ++u) {
            const uint32_t i = hi - 1u - u;   // wraps past 0: then i >= k
            s[u] = i < k ? sym[(size_t)i * 64u] : 0u;
        }
#pragma unroll
        for (uint32_t u = 0; u < 8u; ++u) {
            const uint32_t i = hi - 1u - u;
            if (i < k) {
                const uint32_t z = s[u];
                if (WIDE && z >= 255u) {
                    const uint32_t r = z - 255u;
                    if (r > kSplitWideMaxResidual) wide_bad = true;
                    if (x >= (1u << 19)) { put(x & 255u); x >>= 8; }
                    if (x >= (1u << 19)) { put(x & 255u); x >>= 8; }
                    x = (x << 12) + (r & kSplitWideMaxResidual);
                }
                const uint4 row = rows[WIDE && z >= 255u ? 255u : z];
                if (x >= row.x) { put(x & 255u); x >>= 8; }
                if (x >= row.x) { put(x & 255u); x >>= 8; }
                const uint32_t q = __umulhi(x, row.y) >> (row.w >> 16);
                x = x + q * (row.w & 0xFFFFu) + row.z;
            }
        }
    }
    if (k) {
        put(x & 255u); put((x >> 8) & 255u); put((x >> 16) & 255u); put(x >> 24);
    }
    if (kWrite) {
        for (uint32_t t = 0; t < nacc; ++t) out[t] = (uint8_t)(acc >> (8u * t));
    } else {
        job.lane_len[b * 64u + lane] = (uint16_t)len;
        const uint32_t incl = wave_incl_scan(len, lane);
        if (lane == 63) job.blk_len[b] = 128u + incl;
        if (WIDE && wide_bad) *job.flags = kSplitWideResidual;
    }
}

template <bool kWrite>
__global__ __launch_bounds__(256) void split_encode_kernel(const SplitJob* __restrict__ jobs) {
    __shared__ uint4 rows[256];
    lane_encode<false, kWrite>(jobs, rows);
}
template <bool kWrite>
__global__ __launch_bounds__(256) void split_wide_encode_kernel(const SplitJob* __restrict__ jobs) {
    __shared__ uint4 rows[256];
    lane_encode<true, kWrite>(jobs, rows);
}

// ----------------------------------------------------------------------------------
// Block offsets: blk_off[b] = 4 * n_blocks + sum of the lengths of the blocks before b; blk_off[n_blocks] = the payload's
// length.  One workgroup per job.  kFromStream: the lengths are the u32 table at the head of the payload (any alignment),
// and the scan is the directory check of the decoder: a table that does not fit, a block shorter than its lane directory
// or a sum that is not the payload's length sets kSplitBadDirectory, and offsets are clamped so that no block reaches
// outside the payload.
// ----------------------------------------------------------------------------------
template <bool kFromStream>
__global__ __launch_bounds__(256) void split_scan_kernel(const SplitJob* __restrict__ jobs, unsigned long long* __restrict__ totals) {
    __shared__ unsigned long long sc[256];
    __shared__ uint32_t bad_sh;
    const SplitJob job = jobs[blockIdx.x];
    const int s = threadIdx.x;
    if (s == 0) bad_sh = 0u;
    __syncthreads();
    const unsigned long long head = 4ull * job.n_blocks;
    const bool table_fits = !kFromStream || head <= job.len;
    unsigned long long carry = head;
    for (unsigned long long b0 = 0; b0 < job.n_blocks; b0 += 256u) {
        const unsigned long long b = b0 + s;
        unsigned long long v = 0;
        if (b < job.n_blocks) {
            if (kFromStream) {
                if (table_fits) {
                    const uint8_t* p = job.stream + 4ull * b;
                    v = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
                    job.blk_len[b] = (uint32_t)v;
                }
            } else {
                v = job.blk_len[b];
            }
        }
        sc[s] = v;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const unsigned long long o = s >= d ? sc[s - d] : 0ull;
            __syncthreads();
            sc[s] += o;
            __syncthreads();
        }
        if (b < job.n_blocks) {
            const unsigned long long off = carry + sc[s] - v;
            if (kFromStream && (v < 128u || off + v > job.len)) {
                bad_sh = 1u;
                job.blk_len[b] = 0u;   // the decoders skip the block
                job.blk_off[b] = 0ull;
            } else {
                job.blk_off[b] = off;
            }
        }
        carry += sc[255];
        __syncthreads();
    }
    if (s == 0) {
        job.blk_off[job.n_blocks] = carry;
        if (totals) totals[blockIdx.x] = carry;
        if (kFromStream && (bad_sh || !table_fits || carry != job.len)) *job.flags = kSplitBadDirectory;
    }
}

// ----------------------------------------------------------------------------------
// Decoder: the geometry of the encoder.  lane_decode runs lane `lane` of block b (k symbols, tables in LDS) and hands
// symbol i to store(i, s), once per symbol and in order; WIDE adds the escape step (see the encoder).
// A lane reads its stream four bytes at a time; a read never leaves [lane start, lane end): past the end the window
// is zero-filled and the cursor keeps counting, so a damaged stream ends in a failed end check (state back at 2^23,
// cursor at the end of the stream) and never in an access outside the payload.  A damaged wide stream can give any
// residual in 0..4095, so any z up to 4350; it is handed to store like every other symbol.
// ----------------------------------------------------------------------------------
template <bool WIDE, typename Store>
__device__ __forceinline__ void lane_decode(const SplitJob& job, unsigned long long b, int lane, uint32_t k, const uint8_t* c2s,
                                            const uint32_t* symtab, Store store) {
    const uint32_t blen = job.blk_len[b];
    const unsigned long long boff = job.blk_off[b];
    // (the scan left 0 for a block it refused; checked again here so that the bounds do not rest on another kernel)
    if (blen < 128u || boff + blen > job.len) { if (lane == 0) *job.flags = kSplitBadDirectory; return; }
    const uint8_t* blk = job.stream + boff;
    const uint32_t len = (uint32_t)blk[2 * lane] | ((uint32_t)blk[2 * lane + 1] << 8);
    const uint32_t incl = wave_incl_scan(len, lane);
    const uint32_t all = __shfl(incl, 63, 64);
    if (all + 128u != blen) { if (lane == 0) *job.flags = kSplitBadDirectory; return; }
    const uint8_t* __restrict__ src = blk + 128u + (incl - len);   // [src, src + len) lies inside the block

    uint32_t win = 0u, nwin = 0u, fpos = 0u, pos = 0u;
    auto take = [&]() -> uint32_t {
        if (nwin == 0u) {
            uint32_t w = 0u;
            if (fpos + 4u <= len) {
                uint32_t t;
                __builtin_memcpy(&t, src + fpos, 4);
                w = __builtin_bswap32(t);
            } else {
#pragma unroll
                for (uint32_t t = 0; t < 4u; ++t) w = (w << 8) | (fpos + t < len ? (uint32_t)src[fpos + t] : 0u);
            }
            fpos += 4u;
            win = w;
            nwin = 4u;
        }
        const uint32_t byte = win >> 24;
        win <<= 8;
        --nwin;
        ++pos;
        return byte;
    };
    bool ok = true;
    if (k == 0u) {
        ok = len == 0u;
    } else {
        uint32_t x = take() << 24;
        x |= take() << 16;
        x |= take() << 8;
        x |= take();
        for (uint32_t i = 0; i < k; ++i) {
            const uint32_t slot = x & (kProbScale - 1u);
            uint32_t s = c2s[slot];
            const uint32_t fc = symtab[s];
            x = (fc & 0xFFFFu) * (x >> kProbBits) + slot - (fc >> 16);
            if (x < kRansL) x = (x << 8) | take();
            if (x < kRansL) x = (x << 8) | take();
            if (WIDE && s == 255u) {
                s += x & kSplitWideMaxResidual;
                x >>= 12;
                if (x < kRansL) x = (x << 8) | take();
                if (x < kRansL) x = (x << 8) | take();
            }
            store(i, s);
        }
        ok = x == kRansL && pos == len;
    }
    if (!ok) *job.flags = kSplitBadLane;
}

// Every block of job blockIdx.y, four per workgroup.  Symbol i of the lane goes to its own position inside the block:
// base + lane + 64 i < base + in_block.
template <bool WIDE>
__device__ __forceinline__ void decode_every_block(const SplitJob* jobs, uint32_t* c2s_sh, uint32_t* symtab) {
    const SplitJob job = jobs[blockIdx.y];
    load_decode_tables(job.table, c2s_sh, symtab);
    const int lane = threadIdx.x & 63;
    const unsigned long long b = (unsigned long long)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (b >= job.n_blocks) return;
    const LaneGeometry g(job, b, lane);
    SplitSym<WIDE>* __restrict__ sym = (SplitSym<WIDE>*)job.sym + g.base + lane;
    lane_decode<WIDE>(job, b, lane, g.k, (const uint8_t*)c2s_sh, symtab,
                      [&](uint32_t i, uint32_t s) { sym[(size_t)i * 64u] = (SplitSym<WIDE>)s; });
}

__global__ __launch_bounds__(256) void split_decode_kernel(const SplitJob* __restrict__ jobs) {
    __shared__ uint32_t c2s_sh[kProbScale / 4];
    __shared__ uint32_t symtab[256];
    decode_every_block<false>(jobs, c2s_sh, symtab);
}
__global__ __launch_bounds__(256) void split_wide_decode_kernel(const SplitJob* __restrict__ jobs) {
    __shared__ uint32_t c2s_sh[kProbScale / 4];
    __shared__ uint32_t symtab[256];
    decode_every_block<true>(jobs, c2s_sh, symtab);
}

// ----------------------------------------------------------------------------------
// Lane decode of a block subset (frame ranges): the one or two runs of blocks a SplitFramesJob
// names.  A block that straddles an edge of a symbol range still runs its 64 chains to their end checks (a chain is
// serial, and its end check is the integrity check), but stores only the symbols inside the ranges, relocated into the
// compact volume at job.j.sym: range 0 first, range 1 behind it.  The two symbol ranges become two per-lane iteration
// ranges before the chain loop, so the loop itself carries two 32-bit compares.  End checks cover the decoded blocks only.
// This kernel alone keeps a copy of lane_decode's checks, window and chain: with the range store passed as a callback the
// WIDE instance measured 0.6 to 1.1 % slower (the two stores fold into one behind a selected address), outside the
// run-to-run spread.  A change to lane_decode is repeated below.
// ----------------------------------------------------------------------------------
template <bool WIDE>
__global__ __launch_bounds__(256) void split_frames_decode_kernel(const SplitFramesJob* __restrict__ jobs) {
    using SymT = SplitSym<WIDE>;
    __shared__ uint32_t c2s_sh[kProbScale / 4];
    __shared__ uint32_t symtab[256];
    const SplitFramesJob fj = jobs[blockIdx.y];
    const SplitJob& job = fj.j;
    load_decode_tables(job.table, c2s_sh, symtab);
    const uint8_t* c2s = (const uint8_t*)c2s_sh;
    const int lane = threadIdx.x & 63;
    const unsigned long long slot = (unsigned long long)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (slot >= (unsigned long long)fj.blk_count[0] + fj.blk_count[1]) return;
    const unsigned long long b = slot < fj.blk_count[0] ? fj.blk_first[0] + slot : fj.blk_first[1] + (slot - fj.blk_count[0]);
    if (b >= job.n_blocks) return;   // (the host plans inside the channel; the bounds below do not rest on it)
    const LaneGeometry g(job, b, lane);
    const uint32_t k = g.k;

    // Range r keeps the lane's symbols i in [lo[r], hi[r]): position base + lane + 64 i inside [sym_lo[r], sym_hi[r]).
    // Symbol i of range r goes to out[off[r] + 64 i]; off[r] + 64 i is the position inside the compact volume, so it
    // lies inside range r's part of it for every kept i.  (An inverted range keeps nothing.)
    uint32_t lo[2], hi[2];
    long long off[2];
    const unsigned long long p0 = g.base + (unsigned)lane;
    unsigned long long before = 0;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const unsigned long long s0 = fj.sym_lo[r], s1 = fj.sym_hi[r];
        const unsigned long long a = s0 > p0 ? (s0 - p0 + 63u) / 64u : 0ull;
        const unsigned long long e = s1 > p0 ? (s1 - p0 + 63u) / 64u : 0ull;
        lo[r] = (uint32_t)(a < k ? a : k);
        hi[r] = (uint32_t)(e < k ? e : k);
        if (hi[r] < lo[r]) hi[r] = lo[r];
        off[r] = (long long)before + (long long)p0 - (long long)s0;
        before += s1 > s0 ? s1 - s0 : 0ull;
    }
    SymT* __restrict__ out = (SymT*)job.sym;

    const uint32_t blen = job.blk_len[b];
    const unsigned long long boff = job.blk_off[b];
    if (blen < 128u || boff + blen > job.len) { if (lane == 0) *job.flags = kSplitBadDirectory; return; }
    const uint8_t* blk = job.stream + boff;
    const uint32_t len = (uint32_t)blk[2 * lane] | ((uint32_t)blk[2 * lane + 1] << 8);
    const uint32_t incl = wave_incl_scan(len, lane);
    const uint32_t all = __shfl(incl, 63, 64);
    if (all + 128u != blen) { if (lane == 0) *job.flags = kSplitBadDirectory; return; }
    const uint8_t* __restrict__ src = blk + 128u + (incl - len);   // [src, src + len) lies inside the block

    uint32_t win = 0u, nwin = 0u, fpos = 0u, pos = 0u;
    auto take = [&]() -> uint32_t {
        if (nwin == 0u) {
            uint32_t w = 0u;
            if (fpos + 4u <= len) {
                uint32_t t;
                __builtin_memcpy(&t, src + fpos, 4);
                w = __builtin_bswap32(t);
            } else {
#pragma unroll
                for (uint32_t t = 0; t < 4u; ++t) w = (w << 8) | (fpos + t < len ? (uint32_t)src[fpos + t] : 0u);
            }
            fpos += 4u;
            win = w;
            nwin = 4u;
        }
        const uint32_t byte = win >> 24;
        win <<= 8;
        --nwin;
        ++pos;
        return byte;
    };
    bool ok = true;
    if (k == 0u) {
        ok = len == 0u;
    } else {
        uint32_t x = take() << 24;
        x |= take() << 16;
        x |= take() << 8;
        x |= take();
        for (uint32_t i = 0; i < k; ++i) {
            const uint32_t slot12 = x & (kProbScale - 1u);
            uint32_t s = c2s[slot12];
            const uint32_t fc = symtab[s];
            x = (fc & 0xFFFFu) * (x >> kProbBits) + slot12 - (fc >> 16);
            if (x < kRansL) x = (x << 8) | take();
            if (x < kRansL) x = (x << 8) | take();
            if (WIDE && s == 255u) {
                s += x & kSplitWideMaxResidual;
                x >>= 12;
                if (x < kRansL) x = (x << 8) | take();
                if (x < kRansL) x = (x << 8) | take();
            }
            if (i - lo[0] < hi[0] - lo[0]) out[off[0] + (long long)i * 64] = (SymT)s;
            else if (i - lo[1] < hi[1] - lo[1]) out[off[1] + (long long)i * 64] = (SymT)s;
        }
        ok = x == kRansL && pos == len;
    }
    if (!ok) *job.flags = kSplitBadLane;
}

// ----------------------------------------------------------------------------------
// Lane decode of a box (half-resolution preview and spatial rectangle, DESIGN.md sections 15 and 16): the blocks a
// SplitBoxJob lists (slot -> block through the list).  Every chain runs to its end check; a symbol is stored only when each
// of (x, y, t') lies in the low or the high run of its axis, relocated into the compact volume at job.j.sym.  A lane's
// positions advance by 64 = dP * P + dy * pw + dx (dy * pw + dx < P), so (x, y, t') are carried with three adds and at most
// one wrap each -- also for pw = 2 and P < 64 (then dP >= 1).  The 64-bit divisions happen once per lane, before the chain
// loop; the box is wave-uniform, the coordinates and the destination (two multiplies) do not depend on the chain's state, so
// the serial dependency is lane_decode's own.
// XY_HIGH = false is the instance for jobs that keep the low run alone on x and y (n_hi[0] = n_hi[1] = 0, the preview): the
// two high-run compares and selects are not compiled in.  A partial call runs about one wavefront per SIMD, so every
// instruction of the store rule is paid in full: with the compares left in, the preview's launches measured 337.4 -> 344.8
// us (u8) and 540.8 -> 550.5 us (u16), +2.2 and +1.8 % against a spread of 1.1 and 0.7 % (six rounds, one 1920x1080x64
// chunk); carrying the destination additively instead of multiplying measured +1.0 to +8.6 % in all four roles.  On this
// form the preview's launches are level or faster than the kernel they replace (326.3 and 538.4 us) and the rectangle's level
// (profiles/r21_box_kernel_trace_vs_parent.json).
// ----------------------------------------------------------------------------------
template <bool WIDE, bool XY_HIGH>
__global__ __launch_bounds__(256) void split_box_decode_kernel(const SplitBoxJob* __restrict__ jobs) {
    using SymT = SplitSym<WIDE>;
    __shared__ uint32_t c2s_sh[kProbScale / 4];
    __shared__ uint32_t symtab[256];
    const SplitBoxJob bj = jobs[blockIdx.y];
    const SplitJob& job = bj.j;
    load_decode_tables(job.table, c2s_sh, symtab);
    const int lane = threadIdx.x & 63;
    const unsigned long long slot = (unsigned long long)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (slot >= bj.n_planned) return;
    const unsigned long long b = bj.blocks[slot];
    if (b >= job.n_blocks || !bj.pw || !bj.ph) return;   // (the host plans inside the channel; the bounds of lane_decode do not rest on it)
    const LaneGeometry g(job, b, lane);

    // where the lane's first symbol lies, and what 64 positions further means
    const uint32_t pw = bj.pw, ph = bj.ph;
    const unsigned long long P = (unsigned long long)pw * ph;
    const unsigned long long p0 = g.base + (unsigned)lane;
    const unsigned long long rem0 = p0 % P, step_rem = 64ull % P;
    uint32_t tp = (uint32_t)(p0 / P), y = (uint32_t)(rem0 / pw), x = (uint32_t)(rem0 % pw);
    const uint32_t dP = (uint32_t)(64ull / P), dy = (uint32_t)(step_rem / pw), dx = (uint32_t)(step_rem % pw);   // dy, dx < 64
    const uint32_t x_lo = bj.lo[0], y_lo = bj.lo[1], t_lo = bj.lo[2];
    const uint32_t x_hi = bj.half[0] + x_lo, y_hi = bj.half[1] + y_lo, t_hi = bj.half[2] + t_lo;
    const uint32_t lx = bj.n_lo[0], ly = bj.n_lo[1], lt = bj.n_lo[2], hx = bj.n_hi[0], hy = bj.n_hi[1], ht = bj.n_hi[2];
    const unsigned long long row = (unsigned long long)lx + hx, pitch = bj.pitch;
    const unsigned long long limit = ((unsigned long long)lt + ht) * pitch;   // symbols of the channel's compact volume
    SymT* __restrict__ out = (SymT*)job.sym;
    lane_decode<WIDE>(job, b, lane, g.k, (const uint8_t*)c2s_sh, symtab, [&](uint32_t, uint32_t s) {
        // a kept coordinate c of an axis has c - lo < n_lo (place c - lo) or c - hi < n_hi (place n_lo + c - hi): vx < row,
        // vy < n_lo[1] + n_hi[1] and vt < n_lo[2] + n_hi[2], so with the job's pitch the index lies inside the channel's
        // volume; the compare with `limit` keeps the store there whatever the job and the carried coordinates hold
        const uint32_t x0 = x - x_lo, x1 = x - x_hi, y0 = y - y_lo, y1 = y - y_hi, t0 = tp - t_lo, t1 = tp - t_hi;
        if ((x0 < lx || (XY_HIGH && x1 < hx)) && (y0 < ly || (XY_HIGH && y1 < hy)) && (t0 < lt || t1 < ht)) {
            const uint32_t vx = !XY_HIGH || x0 < lx ? x0 : lx + x1, vy = !XY_HIGH || y0 < ly ? y0 : ly + y1, vt = t0 < lt ? t0 : lt + t1;
            const unsigned long long at = vt * pitch + vy * row + vx;
            if (at < limit) out[at] = (SymT)s;
        }
        x += dx;
        if (x >= pw) { x -= pw; ++y; }
        y += dy;
        if (y >= ph) { y -= ph; ++tp; }
        tp += dP;
    });
}

// ----------------------------------------------------------------------------------
// Container header of whole chunks, one workgroup per chunk.
// ----------------------------------------------------------------------------------
__device__ __forceinline__ void put_le(uint8_t* p, unsigned long long v, int bytes) {
    for (int i = 0; i < bytes; ++i) p[i] = (uint8_t)(v >> (8 * i));
}

__global__ __launch_bounds__(256) void split_header_kernel(const SplitHeaderDesc* __restrict__ descs) {
    const SplitHeaderDesc h = descs[blockIdx.x];
    uint8_t* p = h.out;
    const int s = threadIdx.x;
    if (s == 0) {
        p[0] = 'A'; p[1] = 'L'; p[2] = 'C'; p[3] = 'C'; p[4] = 2; p[5] = h.wavelet;
        put_le(p + 6, h.width, 4); put_le(p + 10, h.height, 4); put_le(p + 14, h.frames, 4);
        put_le(p + 18, h.lane_symbols, 4);
    }
    for (int c = 0; c < 3; ++c) {
        uint8_t* q = p + kSplitFixedHeaderBytes + c * kSplitChannelHeaderBytes;
        if (s == 0) {
            put_le(q, (uint32_t)h.step[c], 4); put_le(q + 4, (uint32_t)h.dead_zone[c], 4);
            put_le(q + 8, h.num_symbols, 4); put_le(q + 12, h.n_blocks, 4);
            put_le(q + 16, h.payload_len[c], 8);
        }
        const uint16_t f = h.freq[c * 256 + s];
        q[24 + 2 * s] = (uint8_t)f;
        q[25 + 2 * s] = (uint8_t)(f >> 8);
    }
}

// The version byte of containers whose headers split_header_kernel has written (.alc v3 differs from v2 in that byte).
__global__ __launch_bounds__(64) void split_version_kernel(const SplitHeaderDesc* __restrict__ descs, int n, uint32_t version) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i < n) descs[i].out[4] = (uint8_t)version;
}

// ----------------------------------------------------------------------------------
// launchers
// ----------------------------------------------------------------------------------
void launch_split_table(const uint32_t* d_hist, uint16_t* d_freq, uint16_t* d_cum, int n_tables, hipStream_t st) {
    if (n_tables > 0) hipLaunchKernelGGL(split_table_kernel, dim3(n_tables), dim3(256), 0, st, d_hist, d_freq, d_cum);
}

// one lane kernel over n_jobs jobs of at most max_blocks blocks: four blocks per workgroup
template <typename Job>
static void launch_lanes(void (*narrow)(const Job*), void (*wide_k)(const Job*), bool wide, const Job* d_jobs, int n_jobs,
                         uint32_t max_blocks, hipStream_t st) {
    if (n_jobs <= 0 || !max_blocks) return;
    hipLaunchKernelGGL(wide ? wide_k : narrow, dim3((max_blocks + 3u) / 4u, (unsigned)n_jobs), dim3(256), 0, st, d_jobs);
}

void launch_split_count(const SplitJob* d_jobs, int n_jobs, uint32_t max_blocks, bool wide, hipStream_t st) {
    launch_lanes(split_encode_kernel<false>, split_wide_encode_kernel<false>, wide, d_jobs, n_jobs, max_blocks, st);
}
void launch_split_write(const SplitJob* d_jobs, int n_jobs, uint32_t max_blocks, bool wide, hipStream_t st) {
    launch_lanes(split_encode_kernel<true>, split_wide_encode_kernel<true>, wide, d_jobs, n_jobs, max_blocks, st);
}
void launch_split_scan(const SplitJob* d_jobs, int n_jobs, bool from_stream, unsigned long long* d_totals, hipStream_t st) {
    if (n_jobs <= 0) return;
    if (from_stream) hipLaunchKernelGGL(split_scan_kernel<true>, dim3(n_jobs), dim3(256), 0, st, d_jobs, d_totals);
    else hipLaunchKernelGGL(split_scan_kernel<false>, dim3(n_jobs), dim3(256), 0, st, d_jobs, d_totals);
}
void launch_split_decode(const SplitJob* d_jobs, int n_jobs, uint32_t max_blocks, bool wide, hipStream_t st) {
    launch_lanes(split_decode_kernel, split_wide_decode_kernel, wide, d_jobs, n_jobs, max_blocks, st);
}
void launch_split_frames_decode(const SplitFramesJob* d_jobs, int n_jobs, uint32_t max_blocks, bool wide, hipStream_t st) {
    launch_lanes(split_frames_decode_kernel<false>, split_frames_decode_kernel<true>, wide, d_jobs, n_jobs, max_blocks, st);
}
void launch_split_box_decode(const SplitBoxJob* d_jobs, int n_jobs, uint32_t max_planned, bool wide, bool xy_high, hipStream_t st) {
    if (xy_high) launch_lanes(split_box_decode_kernel<false, true>, split_box_decode_kernel<true, true>, wide, d_jobs, n_jobs, max_planned, st);
    else launch_lanes(split_box_decode_kernel<false, false>, split_box_decode_kernel<true, false>, wide, d_jobs, n_jobs, max_planned, st);
}
void launch_split_headers(const SplitHeaderDesc* d_descs, int n_chunks, hipStream_t st) {
    if (n_chunks > 0) hipLaunchKernelGGL(split_header_kernel, dim3(n_chunks), dim3(256), 0, st, d_descs);
}
void launch_split_header_version(const SplitHeaderDesc* d_descs, int n_chunks, uint8_t version, hipStream_t st) {
    if (n_chunks > 0) hipLaunchKernelGGL(split_version_kernel, dim3((n_chunks + 63) / 64), dim3(64), 0, st, d_descs, n_chunks, (uint32_t)version);
}

}  // namespace alice
