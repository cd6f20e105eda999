// Banded entropy stage (.alc v5) for gfx950: one frequency table per wavelet subband.
//
// A channel's [t'][yy][xx] symbol volume is the eight octants of the one-level 3-D lifting.  Band k = 4 bt + 2 by + bx is the
// box t' in [bt ht, (bt + 1) ht), yy in [by hh, (by + 1) hh), xx in [bx hw, (bx + 1) hw); its symbols in band order are the
// raster [t''][y''][x''] of the box.  A band is coded exactly as a channel of .alc v2 to v4 is (blocks of 64 L symbols, 64
// lanes per block, lane directory, block-length table, end checks, the escape step of the wide symbol; split.hip), with the
// band's own table: a job is one (chunk, channel, band), so a workgroup still holds one table in LDS.  What differs from
// split.hip is where symbol i of lane j of block B lives: band-order index idx = 64 L B + j + 64 i is the symbol at
// sym + (t'' ph + y'') pw + x'', sym the band's origin inside the channel volume.  A lane carries (x'', y'', t'') and steps
// them by 64 = dP hw hh + dy hw + dx (dy hw + dx < hw hh) with at most one wrap per axis -- also for hw hh < 64, where one
// step crosses rows and frames.  The divisions that split idx and 64 happen once per lane, in 32 bits (a band has at most
// 2^29 symbols), before the chain loop; the address does not depend on the chain's state.
//
// The chains below are copies of lane_encode / lane_decode of split.hip, kept here so that no instance of that file is
// compiled differently (the encoder needs its symbols through the carried coordinates, which lane_encode does not offer).
// A change to either chain is repeated here.
//   band_hist_kernel<WIDE>            symbols [3][pf][ph][pw] -> u32 [3][8][256], min(z, 255) when WIDE
//   band_encode_kernel<WIDE, kWrite>  <false> counts every lane's stream length, <true> writes directory and streams
//   band_decode_kernel<WIDE>          every block of a band; symbol i at its place in the channel volume
//   band_range_decode_kernel<WIDE>    a block run of a band; the symbols of a plane range alone, into a compact volume
//   band_header_kernel                the 12 636-byte container header
// Tables, block offsets and the decoder's directory check are split_table_kernel, rans_tables_from_arrays_kernel and
// split_scan_kernel, unchanged.
//
// Every store to memory is a vector store; the scalar unit only reads.
#include "common.h"
#include "kernels.h"

#include <algorithm>
#include <type_traits>

namespace alice {

namespace {

template <bool WIDE> using BandSym = std::conditional_t<WIDE, uint16_t, uint8_t>;

__device__ __forceinline__ uint32_t band_wave_incl_scan(uint32_t v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}

// Block b of a band job (b < n_blocks): its first band-order index, its symbol count, and how many of them lane `lane` owns.
struct BandLaneGeometry {
    uint32_t base, in_block, k;
    __device__ __forceinline__ BandLaneGeometry(const SplitJob& job, uint32_t b, int lane) {
        const unsigned long long first = (unsigned long long)b * 64ull * job.lane_symbols;   // b < n_blocks: below n < 2^29
        base = (uint32_t)first;
        const unsigned long long left = job.n - first;
        in_block = left < 64ull * job.lane_symbols ? (uint32_t)left : 64u * job.lane_symbols;
        k = (uint32_t)lane < in_block ? (in_block - (uint32_t)lane + 63u) / 64u : 0u;
    }
};

// Where a band-order index lies inside its box, and the step of 64 indices, forwards or backwards.  x < hw and y < hh hold
// before and after every step; t counts on (past the box for indices at or above n, which are never loaded or stored).
struct BandWalk {
    uint32_t x, y, hw, hh, dx, dy;
    int32_t t, dP;
    __device__ __forceinline__ BandWalk(uint32_t hw_, uint32_t hh_, uint32_t idx) {   // (band_range_decode_kernel's)
        hw = hw_; hh = hh_;
        const uint32_t P = hw * hh;
        const uint32_t rem = idx % P, srem = 64u % P;
        t = (int32_t)(idx / P); y = rem / hw; x = rem % hw;
        dP = (int32_t)(64u / P); dy = srem / hw; dx = srem % hw;
    }
    __device__ __forceinline__ BandWalk(const SplitBandJob& bj, uint32_t idx) {
        hw = bj.hw; hh = bj.hh;
        const uint32_t P = hw * hh;        // hw hh ht = n < 2^29
        const uint32_t rem = idx % P, srem = 64u % P;
        t = (int32_t)(idx / P); y = rem / hw; x = rem % hw;
        dP = (int32_t)(64u / P); dy = srem / hw; dx = srem % hw;
    }
    // offset of the symbol inside the channel volume, relative to the band's origin
    __device__ __forceinline__ size_t at(const SplitBandJob& bj) const { return ((size_t)(uint32_t)t * bj.ph + y) * bj.pw + x; }
    __device__ __forceinline__ void forward() {
        x += dx;
        if (x >= hw) { x -= hw; ++y; }
        y += dy;
        if (y >= hh) { y -= hh; ++t; }
        t += dP;
    }
    __device__ __forceinline__ void back() {
        uint32_t borrow = 0u;
        if (x < dx) { x += hw; borrow = 1u; }
        x -= dx;
        const uint32_t sub = dy + borrow;   // at most hh
        if (y < sub) { y += hh; --t; }
        y -= sub;
        t -= dP;
    }
};

__device__ __forceinline__ bool band_job_ok(const SplitBandJob& bj) {
    // (the host plans the box; nothing below divides by zero or leaves 32 bits whatever the job holds)
    return bj.hw && bj.hh && (unsigned long long)bj.hw * bj.hh <= bj.j.n && bj.j.n < (1ull << 30);
}
__device__ __forceinline__ bool band_range_job_ok(const SplitBandRangeJob& rj) {
    return rj.hw && rj.hh && (unsigned long long)rj.hw * rj.hh <= rj.j.n && rj.j.n < (1ull << 30) && rj.idx_lo <= rj.idx_hi &&
           rj.idx_hi <= rj.j.n;
}

}  // namespace

// ----------------------------------------------------------------------------------
// Band histograms of one chunk.  A virtual block is rows_per_vb whole rows (a row shorter than 4096 symbols) or one
// 4096-symbol segment of a row; a thread takes 16 consecutive symbols of one row in pieces of `align` bytes, the largest
// power of two up to 16 that divides the address of the volume and the bytes of a row (so every row start is that aligned
// and no piece straddles a row's end).  A row lies in two bands (bx = 0, 1), chosen per symbol: a wavefront's span may
// straddle hw.  Each wavefront bins into its own copy of the channel's [8][256] counters in LDS; the copies are folded and
// added to memory with vector atomics when the channel changes and at the end of the grid-stride loop.  Virtual blocks
// never straddle a channel.
// ----------------------------------------------------------------------------------
struct BandHistArgs {
    const uint8_t* sym;
    uint32_t pw, ph, pf, hw;
    uint32_t units_per_row;    // ceil(pw / 16)
    uint32_t rows_per_vb;      // >= 1; above 1 only when units_per_row * rows_per_vb <= 256
    uint32_t segs;             // ceil(units_per_row / 256)
    uint32_t align;            // 1 (u8 only), 2, 4, 8 or 16 bytes
    unsigned long long vbs_per_channel, rows_per_channel;
    uint32_t* hist;            // [3][8][256], zeroed by the caller
};

template <bool WIDE>
__global__ __launch_bounds__(256) void band_hist_kernel(const BandHistArgs a) {
    __shared__ uint32_t bins[4][8 * 256];
    constexpr uint32_t SB = WIDE ? 2u : 1u;
    const int wave = threadIdx.x >> 6;
    auto clear = [&]() {
        for (int i = threadIdx.x; i < 4 * 8 * 256; i += 256) (&bins[0][0])[i] = 0u;
        __syncthreads();
    };
    auto flush = [&](uint32_t c) {
        __syncthreads();
        for (int i = threadIdx.x; i < 8 * 256; i += 256) {
            const uint32_t v = bins[0][i] + bins[1][i] + bins[2][i] + bins[3][i];
            if (v) atomicAdd(a.hist + (size_t)c * 8 * 256 + i, v);
        }
        __syncthreads();
    };
    clear();
    const unsigned long long total = 3ull * a.vbs_per_channel;
    uint32_t cur = 0xFFFFFFFFu;
    for (unsigned long long vb = blockIdx.x; vb < total; vb += gridDim.x) {
        const uint32_t c = (uint32_t)(vb / a.vbs_per_channel);
        const unsigned long long v = vb % a.vbs_per_channel;
        if (c != cur) {
            if (cur != 0xFFFFFFFFu) { flush(cur); clear(); }
            cur = c;
        }
        unsigned long long row;
        uint32_t unit;
        bool active;
        if (a.segs == 1u) {
            const uint32_t r = threadIdx.x / a.units_per_row;
            unit = threadIdx.x % a.units_per_row;
            row = v * a.rows_per_vb + r;
            active = r < a.rows_per_vb && row < a.rows_per_channel;
        } else {
            row = v / a.segs;
            unit = (uint32_t)(v % a.segs) * 256u + threadIdx.x;
            active = unit < a.units_per_row;
        }
        if (!active) continue;
        const uint32_t tp = (uint32_t)(row / a.ph), y = (uint32_t)(row % a.ph);
        const uint32_t band_ty = ((tp >= a.pf / 2u ? 4u : 0u) | (y >= a.ph / 2u ? 2u : 0u)) << 8;
        const uint32_t x0 = unit * 16u;
        const uint32_t n = a.pw - x0 < 16u ? a.pw - x0 : 16u;     // symbols of this thread, x0 < pw
        const uint8_t* p = a.sym + (((size_t)c * a.rows_per_channel + row) * a.pw + x0) * SB;
        // the thread's bytes, in registers: pieces at or past the row's end are not read
        uint32_t w[4 * SB] = {};
        const uint32_t nbytes = n * SB;
        if (a.align >= 16u) {
#pragma unroll
            for (uint32_t q = 0; q < SB; ++q)
                if (16u * q < nbytes) {
                    const uint4 t = *(const uint4*)(p + 16u * q);
                    w[4 * q] = t.x; w[4 * q + 1] = t.y; w[4 * q + 2] = t.z; w[4 * q + 3] = t.w;
                }
        } else if (a.align == 8u) {
#pragma unroll
            for (uint32_t q = 0; q < 2u * SB; ++q)
                if (8u * q < nbytes) {
                    const uint2 t = *(const uint2*)(p + 8u * q);
                    w[2 * q] = t.x; w[2 * q + 1] = t.y;
                }
        } else if (a.align == 4u) {
#pragma unroll
            for (uint32_t q = 0; q < 4u * SB; ++q)
                if (4u * q < nbytes) w[q] = *(const uint32_t*)(p + 4u * q);
        } else if (a.align == 2u) {
#pragma unroll
            for (uint32_t q = 0; q < 8u * SB; ++q)
                if (2u * q < nbytes) w[q >> 1] |= (uint32_t)(*(const uint16_t*)(p + 2u * q)) << (16u * (q & 1u));
        } else {
#pragma unroll
            for (uint32_t q = 0; q < 16u * SB; ++q)
                if (q < nbytes) w[q >> 2] |= (uint32_t)p[q] << (8u * (q & 3u));
        }
        // runs of equal bins cost one LDS atomic (the high bands pile up at 0)
        uint32_t run_bin = 0xFFFFFFFFu, run = 0u;
#pragma unroll
        for (uint32_t i = 0; i < 16u; ++i) {
            if (i < n) {
                uint32_t z = WIDE ? (w[i >> 1] >> (16u * (i & 1u))) & 0xFFFFu : (w[i >> 2] >> (8u * (i & 3u))) & 0xFFu;
                if (WIDE && z > 255u) z = 255u;
                const uint32_t bin = band_ty | (x0 + i >= a.hw ? 256u : 0u) | z;
                if (bin == run_bin) {
                    ++run;
                } else {
                    if (run) atomicAdd(&bins[wave][run_bin], run);
                    run_bin = bin; run = 1u;
                }
            }
        }
        if (run) atomicAdd(&bins[wave][run_bin], run);
    }
    if (cur != 0xFFFFFFFFu) flush(cur);
}

// ----------------------------------------------------------------------------------
// Encoder: lane_encode of split.hip with the symbols read through the lane's walk.  The chain walks a lane's symbols last
// to first, eight loaded ahead of the chain that consumes them; the walk steps back once per symbol.
// ----------------------------------------------------------------------------------
template <bool WIDE, bool kWrite>
__global__ __launch_bounds__(256) void band_encode_kernel(const SplitBandJob* __restrict__ jobs) {
    __shared__ uint4 rows[256];
    const SplitBandJob bj = jobs[blockIdx.y];
    const SplitJob& job = bj.j;
    {
        const RansEncEntry e = job.table->enc[threadIdx.x];
        rows[threadIdx.x] = make_uint4(e.xmax, e.rcp, e.cbias, (uint32_t)e.g | (e.rsh << 16));
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const unsigned long long b64 = (unsigned long long)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (b64 >= job.n_blocks || !band_job_ok(bj)) return;
    const uint32_t b = (uint32_t)b64;
    const BandLaneGeometry g(job, b, lane);
    const uint32_t k = g.k, kmax = (g.in_block + 63u) / 64u;   // kmax: lane 0's count, >= 1
    const BandSym<WIDE>* __restrict__ sym = (const BandSym<WIDE>*)job.sym;
    BandWalk walk(bj, g.base + (uint32_t)lane + 64u * (kmax - 1u));   // below n + 64 L + 64 < 2^31

    uint32_t len = 0u;              // bytes of this lane's stream
    uint8_t* out = nullptr;         // kWrite: one past the lane's last byte
    uint32_t acc = 0u, nacc = 0u;   // kWrite: bytes collected for the dword in progress (lowest address in the low byte)
    bool wide_bad = false;          // WIDE count pass: a residual above 4095
    if (kWrite) {
        len = job.lane_len[(size_t)b * 64u + lane];
        const uint32_t incl = band_wave_incl_scan(len, lane);
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
    for (uint32_t hi = kmax; hi > 0u; hi = hi > 8u ? hi - 8u : 0u) {
        uint32_t s[8];
#pragma unroll
        for (uint32_t u = 0; u < 8u; ++u) {
            const uint32_t i = hi - 1u - u;   // wraps past 0: then i >= k
            s[u] = i < k ? sym[walk.at(bj)] : 0u;   // i < k: index below n, inside the box
            walk.back();
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
        job.lane_len[(size_t)b * 64u + lane] = (uint16_t)len;
        const uint32_t incl = band_wave_incl_scan(len, lane);
        if (lane == 63) job.blk_len[b] = 128u + incl;
        if (WIDE && wide_bad) *job.flags = kSplitWideResidual;
    }
}

// ----------------------------------------------------------------------------------
// Decoder: lane_decode of split.hip; symbol i goes to the place the lane's walk names.  A lane reads its stream four bytes
// at a time; a read never leaves [lane start, lane end): past the end the window is zero-filled and the cursor keeps
// counting, so a damaged stream ends in a failed end check and never in an access outside the payload.  Stores happen
// for i < k only, band-order indices below n: inside the box.
// ----------------------------------------------------------------------------------
template <bool WIDE>
__global__ __launch_bounds__(256) void band_decode_kernel(const SplitBandJob* __restrict__ jobs) {
    __shared__ uint32_t c2s_sh[kProbScale / 4];
    __shared__ uint32_t symtab[256];
    const SplitBandJob bj = jobs[blockIdx.y];
    const SplitJob& job = bj.j;
    {
        const uint32_t* src = (const uint32_t*)job.table->dec.c2s;
#pragma unroll
        for (int t = 0; t < 4; ++t) c2s_sh[threadIdx.x + 256 * t] = src[threadIdx.x + 256 * t];
        symtab[threadIdx.x] = job.table->dec.symtab[threadIdx.x];
        __syncthreads();
    }
    const uint8_t* c2s = (const uint8_t*)c2s_sh;
    const int lane = threadIdx.x & 63;
    const unsigned long long b64 = (unsigned long long)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (b64 >= job.n_blocks || !band_job_ok(bj)) return;
    const uint32_t b = (uint32_t)b64;
    const BandLaneGeometry g(job, b, lane);
    const uint32_t k = g.k;
    BandSym<WIDE>* __restrict__ sym = (BandSym<WIDE>*)job.sym;
    BandWalk walk(bj, g.base + (uint32_t)lane);

    const uint32_t blen = job.blk_len[b];
    const unsigned long long boff = job.blk_off[b];
    // (the scan left 0 for a block it refused; checked again here so that the bounds do not rest on another kernel)
    if (blen < 128u || boff + blen > job.len) { if (lane == 0) *job.flags = kSplitBadDirectory; return; }
    const uint8_t* blk = job.stream + boff;
    const uint32_t len = (uint32_t)blk[2 * lane] | ((uint32_t)blk[2 * lane + 1] << 8);
    const uint32_t incl = band_wave_incl_scan(len, lane);
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
            sym[walk.at(bj)] = (BandSym<WIDE>)s;
            walk.forward();
        }
        ok = x == kRansL && pos == len;
    }
    if (!ok) *job.flags = kSplitBadLane;
}

// ----------------------------------------------------------------------------------
// Lane decode of a plane range of a band (frame ranges and previews of a banded chunk): the blocks
// [blk_first, blk_first + blk_count) of a SplitBandRangeJob, four consecutive ones per workgroup.  A block that straddles an
// edge of [idx_lo, idx_hi) still runs its 64 chains to their end checks (a chain is serial, and its end check is the
// integrity check) but stores only the symbols inside, at (t'' - idx_lo / (hw hh)) plane_pitch + y'' row_pitch + x'' of the
// destination.  The index range becomes a per-lane iteration range before the chain loop (as in
// split_frames_decode_kernel), so the loop carries one 32-bit compare and BandWalk's three adds, also for hw hh < 64.  For a
// kept symbol idx >= idx_lo, so t'' - idx_lo / (hw hh) >= 0.  End checks cover the decoded blocks only.  The chain is a copy
// of band_decode_kernel's, kept apart so that no existing instance is compiled differently; a change to either is repeated.
// ----------------------------------------------------------------------------------
template <bool WIDE>
__global__ __launch_bounds__(256) void band_range_decode_kernel(const SplitBandRangeJob* __restrict__ jobs) {
    __shared__ uint32_t c2s_sh[kProbScale / 4];
    __shared__ uint32_t symtab[256];
    const SplitBandRangeJob rj = jobs[blockIdx.y];
    const SplitJob& job = rj.j;
    {
        const uint32_t* src = (const uint32_t*)job.table->dec.c2s;
#pragma unroll
        for (int t = 0; t < 4; ++t) c2s_sh[threadIdx.x + 256 * t] = src[threadIdx.x + 256 * t];
        symtab[threadIdx.x] = job.table->dec.symtab[threadIdx.x];
        __syncthreads();
    }
    const uint8_t* c2s = (const uint8_t*)c2s_sh;
    const int lane = threadIdx.x & 63;
    const unsigned long long slot = (unsigned long long)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (slot >= rj.blk_count || !band_range_job_ok(rj)) return;
    const unsigned long long b64 = (unsigned long long)rj.blk_first + slot;
    if (b64 >= job.n_blocks) return;   // (the host plans inside the band; the bounds below do not rest on it)
    const uint32_t b = (uint32_t)b64;
    const BandLaneGeometry g(job, b, lane);
    const uint32_t k = g.k;
    BandSym<WIDE>* __restrict__ sym = (BandSym<WIDE>*)job.sym;
    const uint32_t p0 = g.base + (uint32_t)lane;   // below n + 64 < 2^31
    BandWalk walk(rj.hw, rj.hh, p0);
    // the lane's symbols i in [i_lo, i_hi) have their index p0 + 64 i inside [idx_lo, idx_hi)
    uint32_t i_lo = rj.idx_lo > p0 ? (rj.idx_lo - p0 + 63u) / 64u : 0u;
    uint32_t i_hi = rj.idx_hi > p0 ? (rj.idx_hi - p0 + 63u) / 64u : 0u;
    if (i_lo > k) i_lo = k;
    if (i_hi > k) i_hi = k;
    if (i_hi < i_lo) i_hi = i_lo;
    const uint32_t kept = i_hi - i_lo;
    const int32_t t_lo = (int32_t)(rj.idx_lo / (rj.hw * rj.hh));

    const uint32_t blen = job.blk_len[b];
    const unsigned long long boff = job.blk_off[b];
    // (the scan left 0 for a block it refused; checked again here so that the bounds do not rest on another kernel)
    if (blen < 128u || boff + blen > job.len) { if (lane == 0) *job.flags = kSplitBadDirectory; return; }
    const uint8_t* blk = job.stream + boff;
    const uint32_t len = (uint32_t)blk[2 * lane] | ((uint32_t)blk[2 * lane + 1] << 8);
    const uint32_t incl = band_wave_incl_scan(len, lane);
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
            if (i - i_lo < kept)
                sym[(size_t)(uint32_t)(walk.t - t_lo) * rj.plane_pitch + (size_t)walk.y * rj.row_pitch + walk.x] = (BandSym<WIDE>)s;
            walk.forward();
        }
        ok = x == kRansL && pos == len;
    }
    if (!ok) *job.flags = kSplitBadLane;
}

// ----------------------------------------------------------------------------------
// Container header, one workgroup per chunk; any alignment, byte stores.
// ----------------------------------------------------------------------------------
namespace {
__device__ __forceinline__ void band_put_le(uint8_t* p, unsigned long long v, int bytes) {
    for (int i = 0; i < bytes; ++i) p[i] = (uint8_t)(v >> (8 * i));
}
}  // namespace

__global__ __launch_bounds__(256) void band_header_kernel(const BandHeaderDesc* __restrict__ descs) {
    const BandHeaderDesc& h = descs[blockIdx.x];
    uint8_t* p = h.out;
    const int s = threadIdx.x;
    if (s == 0) {
        p[0] = 'A'; p[1] = 'L'; p[2] = 'C'; p[3] = 'C'; p[4] = 5; p[5] = h.wavelet;
        band_put_le(p + 6, h.width, 4); band_put_le(p + 10, h.height, 4); band_put_le(p + 14, h.frames, 4);
        band_put_le(p + 18, h.lane_symbols, 4);
        p[22] = h.base; p[23] = 0;
    }
    if (s < 3) {
        uint8_t* q = p + kBandFixedHeaderBytes + s * kBandChannelHeaderBytes;
        band_put_le(q, (uint32_t)h.step[s], 4); band_put_le(q + 4, (uint32_t)h.dead_zone[s], 4);
        band_put_le(q + 8, h.num_symbols, 4);
    }
    if (s < 24) {
        uint8_t* q = p + kBandFixedHeaderBytes + (s / 8) * kBandChannelHeaderBytes + 12 + (s % 8) * kBandBandHeaderBytes;
        band_put_le(q, h.n_blocks, 4);
        band_put_le(q + 4, h.payload_len[s], 8);
    }
    for (int j = 0; j < 24; ++j) {
        uint8_t* q = p + kBandFixedHeaderBytes + (j / 8) * kBandChannelHeaderBytes + 12 + (j % 8) * kBandBandHeaderBytes + 12;
        const uint16_t f = h.freq[j * 256 + s];
        q[2 * s] = (uint8_t)f;
        q[2 * s + 1] = (uint8_t)(f >> 8);
    }
}

// ----------------------------------------------------------------------------------
// launchers
// ----------------------------------------------------------------------------------
void launch_band_hist(const void* d_sym, const ChunkDims& d, bool wide, uint32_t* d_hist, hipStream_t st) {
    if (!d.padded) return;
    BandHistArgs a{};
    a.sym = (const uint8_t*)d_sym;
    a.pw = (uint32_t)d.pw; a.ph = (uint32_t)d.ph; a.pf = (uint32_t)d.pf; a.hw = a.pw / 2u;
    a.units_per_row = (a.pw + 15u) / 16u;
    a.segs = (a.units_per_row + 255u) / 256u;
    a.rows_per_vb = a.segs == 1u ? 256u / a.units_per_row : 1u;
    a.rows_per_channel = (unsigned long long)a.pf * a.ph;
    a.vbs_per_channel = a.segs == 1u ? (a.rows_per_channel + a.rows_per_vb - 1u) / a.rows_per_vb : a.rows_per_channel * a.segs;
    const unsigned long long row_bytes = (unsigned long long)a.pw * (wide ? 2u : 1u);
    const unsigned long long bits = (unsigned long long)(uintptr_t)d_sym | row_bytes | 16ull;
    a.align = (uint32_t)(bits & (~bits + 1ull));   // lowest set bit: 1 .. 16
    a.hist = d_hist;
    const unsigned grid = std::min(generic_grid_for(3ull * a.vbs_per_channel * 256ull), 2048u);
    if (wide) hipLaunchKernelGGL(band_hist_kernel<true>, dim3(grid), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(band_hist_kernel<false>, dim3(grid), dim3(256), 0, st, a);
}

namespace {
void launch_band_lanes(void (*narrow)(const SplitBandJob*), void (*wide_k)(const SplitBandJob*), bool wide, const SplitBandJob* d_jobs,
                       int n_jobs, uint32_t max_blocks, hipStream_t st) {
    if (n_jobs <= 0 || !max_blocks) return;
    hipLaunchKernelGGL(wide ? wide_k : narrow, dim3((max_blocks + 3u) / 4u, (unsigned)n_jobs), dim3(256), 0, st, d_jobs);
}
}  // namespace

void launch_band_count(const SplitBandJob* d_jobs, int n_jobs, uint32_t max_blocks, bool wide, hipStream_t st) {
    launch_band_lanes(band_encode_kernel<false, false>, band_encode_kernel<true, false>, wide, d_jobs, n_jobs, max_blocks, st);
}
void launch_band_write(const SplitBandJob* d_jobs, int n_jobs, uint32_t max_blocks, bool wide, hipStream_t st) {
    launch_band_lanes(band_encode_kernel<false, true>, band_encode_kernel<true, true>, wide, d_jobs, n_jobs, max_blocks, st);
}
void launch_band_decode(const SplitBandJob* d_jobs, int n_jobs, uint32_t max_blocks, bool wide, hipStream_t st) {
    launch_band_lanes(band_decode_kernel<false>, band_decode_kernel<true>, wide, d_jobs, n_jobs, max_blocks, st);
}
void launch_band_range_decode(const SplitBandRangeJob* d_jobs, int n_jobs, uint32_t max_blocks, bool wide, hipStream_t st) {
    if (n_jobs <= 0 || !max_blocks) return;
    const dim3 grid((max_blocks + 3u) / 4u, (unsigned)n_jobs);
    if (wide) hipLaunchKernelGGL(band_range_decode_kernel<true>, grid, dim3(256), 0, st, d_jobs);
    else hipLaunchKernelGGL(band_range_decode_kernel<false>, grid, dim3(256), 0, st, d_jobs);
}
void launch_band_headers(const BandHeaderDesc* d_descs, int n_chunks, hipStream_t st) {
    if (n_chunks > 0) hipLaunchKernelGGL(band_header_kernel, dim3(n_chunks), dim3(256), 0, st, d_descs);
}

}  // namespace alice
