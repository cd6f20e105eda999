// Person segmentation (reference src/segment.rs) on the device: motion and chroma-key masks, the
// dilate-then-erode cleanup, bounding box and count, the mask's run-length code and the compaction of
// the person's pixels.  Bit-exact to the reference; the C ABI and its validation live in codec.hip.
//
//   segment_by_motion     src/segment.rs:172-230     dilate_mask_separable  :313-373
//   segment_by_chroma     :234-265                   erode_mask_separable   :378-390
//   compute_bbox_fast     :400-441                   rle_encode_mask        :131-154
//   extract_person_rgb    :107-125
//
// Masks are bit-packed between stages: row-major words of 64 pixels, ceil(w/64) words per row, bits beyond
// the frame width always 0.  Dilation of radius r is a box maximum over the (2r+1)^2 window clipped to the
// frame (what the reference's two distance scans per axis compute), so it is done as two 1-D passes whose
// cost does not depend on r:
//   * along a row, a pixel is set iff the nearest set pixel lies at most r away: per word, the last set bit
//     to its left and the first set bit to its right come from a max/min scan over the row's words
//     (clz/ctz per word), and the word's own bits are smeared by min(r, 63);
//   * along a column, van Herk/Gil-Werman: OR prefixes (G) and suffixes (H) within blocks of B = 2r+1 rows,
//     and the window [y-r, y+r] clipped to the frame is H[lo] | G[hi] (one of them when lo and hi share a
//     block).  B is clamped to the height: with one block the clipped window always touches a frame edge.
// Erosion is complement, dilate, complement (:378-390), so pixels outside the frame count as foreground.
//
// Launch sequence of one call (any radii, any number of frames): fill of the stats, a row kernel
// (threshold + ballot-pack + horizontal dilation), a column kernel, a row kernel (vertical combine +
// complement + horizontal dilation for the erosion), a column kernel, a final row kernel (combine, u8 mask,
// bbox/count partials) and a finalize kernel.  A radius of 0 drops its two kernels (:213-218).
#include "common.h"
#include "kernels.h"

namespace alice {

namespace {

constexpr long long kNoPos = -1;                    // "no set pixel to the left"
constexpr long long kFarPos = 0x7FFFFFFFFFFFFFFFll;  // "no set pixel to the right"

__device__ __forceinline__ uint64_t tail_bits(uint64_t k, uint64_t W64, uint64_t w) {
    if (k + 1 < W64) return ~0ull;
    const unsigned rem = (unsigned)(w & 63);
    return rem ? ((1ull << rem) - 1) : ~0ull;
}

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
    for (int d = 32; d >= 1; d >>= 1) v = min(v, (uint32_t)__shfl_xor(v, d));
    return v;
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
    for (int d = 32; d >= 1; d >>= 1) v = max(v, (uint32_t)__shfl_xor(v, d));
    return v;
}

// pixel predicate of the first stage: motion (:204-208), planar Cg (:245-249), or Cg of interleaved RGB computed
// as alice_codec_rgb_to_ycocg_r does (src/color.rs:225-228)
template <int SRC>
__device__ __forceinline__ bool pixel_on(const SegSource& s, uint64_t frame, uint64_t pix, uint64_t wh) {
    if (SRC == kSegMotion) {
        const unsigned c = s.cur[frame * wh + pix], r = s.ref[frame * s.ref_stride + pix];
        const unsigned d = c > r ? c - r : r - c;
        return d > s.motion_threshold;
    } else if (SRC == kSegCg) {
        return s.cg[frame * wh + pix] <= s.green_threshold;
    } else {
        const uint8_t* p = s.rgb + 3 * (frame * wh + pix);
        const int r = p[0], g = p[1], b = p[2];
        const int co = r - b;
        const int t = b + (co >> 1);
        return (int16_t)(g - t) <= s.green_threshold;
    }
}

// Horizontal dilation of one word: P = last set position left of the word (kNoPos), N = first set position right of
// it (kFarPos), r >= 1.
__device__ __forceinline__ uint64_t dilate_word(uint64_t x, uint64_t k, long long P, long long N, uint64_t r) {
    const long long base = (long long)(k * 64);
    uint64_t out = 0;
    if (P != kNoPos) {
        const long long t = P + (long long)r - base;   // bits 0..t are within r of P
        if (t >= 63) out = ~0ull;
        else if (t >= 0) out |= (2ull << t) - 1;
    }
    if (N != kFarPos) {
        const long long s = N - (long long)r - base;   // bits s..63 are within r of N
        if (s <= 0) out = ~0ull;
        else if (s <= 63) out |= ~0ull << s;
    }
    if (x) {
        if (r >= 63) {
            out = ~0ull;
        } else {
            uint64_t a = x, b = x;                      // a = OR of x << d, b = OR of x >> d, d = 0..done
            unsigned done = 0;
            while (done < (unsigned)r) {
                const unsigned s = min(done + 1, (unsigned)r - done);
                a |= a << s;
                b |= b >> s;
                done += s;
            }
            out |= a | b;
        }
    }
    return out;
}

// block index of row y0 + lane for blocks of B rows (B >= 1); y0 is wave-uniform
__device__ __forceinline__ uint64_t block_of(uint64_t y0, unsigned lane, uint64_t B) {
    const uint64_t blk0 = y0 / B, t = y0 % B + lane;
    return blk0 + (B >= 64 ? (uint64_t)(t >= B) : (uint64_t)((uint32_t)t / (uint32_t)B));
}

struct SegRowArgs {
    SegSource px;
    const uint64_t* G;       // SRC == kSegPacked: vertical combine of these block prefixes / suffixes
    const uint64_t* H;
    uint64_t vr, vB;         // radius and (clamped) block length of that vertical pass
    uint64_t w, h, n_frames, W64;
    uint32_t invert;         // complement (within the frame) after the source
    uint64_t hr;             // horizontal dilation radius, 0 = none
    uint64_t* dst;           // packed output (not final)
    long long* ncarry;       // rows of more than 64 words: first set position right of each 64-word chunk
    uint32_t final_;         // final stage: u8 mask + stats
    uint8_t* mask;           // may be null
    uint32_t* stats;         // n_frames x {~min_x, ~min_y, max_x, max_y, count} accumulators
};

// One wave per row, four rows of one frame per workgroup.  Lane j holds word 64c + j of chunk c.
template <int SRC>
__global__ __launch_bounds__(256) void segment_row_kernel(SegRowArgs a) {
    __shared__ uint32_t red[4][5];
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t w = a.w, h = a.h, wh = w * h, W64 = a.W64, nch = (W64 + 63) / 64;
    const uint64_t bpf = (h + 3) / 4, nblocks = bpf * a.n_frames;
    for (uint64_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
        const uint64_t f = blk / bpf, y = (blk % bpf) * 4 + wave;
        uint32_t cnt = 0, minx = 0xFFFFFFFFu, maxx = 0, rowany = 0;
        if (y < h) {
            const uint64_t row = f * h + y;
            // vertical combine for this row (wave-uniform choice)
            uint64_t lo = 0, hi = 0;
            int pick = 0;   // 0: H[lo] | G[hi], 1: G[hi], 2: H[lo]
            if (SRC == kSegPacked) {
                lo = y > a.vr ? y - a.vr : 0;
                hi = (h - 1 - y) > a.vr ? y + a.vr : h - 1;
                if (lo / a.vB == hi / a.vB) pick = (lo % a.vB == 0) ? 1 : 2;
            }
            auto source = [&](uint64_t c) -> uint64_t {
                const uint64_t k0 = c * 64, nw = min((uint64_t)64, W64 - k0);
                uint64_t mine = 0;
                if (SRC == kSegPacked) {
                    if (lane < nw) {
                        const uint64_t k = k0 + lane, fb = f * h * W64 + k;
                        if (pick == 1) mine = a.G[fb + hi * W64];
                        else if (pick == 2) mine = a.H[fb + lo * W64];
                        else mine = a.H[fb + lo * W64] | a.G[fb + hi * W64];
                    }
                } else {
                    for (uint64_t i = 0; i < nw; ++i) {
                        const uint64_t x = (k0 + i) * 64 + lane;
                        const bool on = x < w && pixel_on<SRC>(a.px, f, y * w + x, wh);
                        const uint64_t b = __ballot(on);
                        if (lane == i) mine = b;
                    }
                }
                if (a.invert) mine = ~mine;
                return lane < nw ? (mine & tail_bits(k0 + lane, W64, w)) : 0;
            };
            auto emit = [&](uint64_t c, uint64_t x) {
                const uint64_t k0 = c * 64, nw = min((uint64_t)64, W64 - k0);
                if (!a.final_) {
                    if (lane < nw) a.dst[row * W64 + k0 + lane] = x;
                    return;
                }
                if (x) {   // compute_bbox_fast, :407-432
                    const uint64_t p = (k0 + lane) * 64;
                    cnt += (uint32_t)__popcll(x);
                    minx = min(minx, (uint32_t)(p + __builtin_ctzll(x)));
                    maxx = max(maxx, (uint32_t)(p + 63 - __builtin_clzll(x)));
                    rowany = 1;
                }
                if (a.mask) {
                    uint8_t* m = a.mask + f * wh + y * w;
                    for (uint64_t i = 0; i < nw; ++i) {
                        const uint64_t word = __shfl(x, (int)i);
                        const uint64_t px = (k0 + i) * 64 + lane;
                        if (px < w) m[px] = (uint8_t)((word >> lane) & 1u);
                    }
                }
            };
            // exclusive scans over the chunk: last set position left of each word, first set position right of it
            auto scan = [&](uint64_t c, uint64_t x, long long Pin, long long Nin, long long* P, long long* N,
                            long long* Pout, long long* Nout) {
                const long long p = (long long)((c * 64 + lane) * 64);
                long long last = x ? p + 63 - __builtin_clzll(x) : kNoPos;
                long long first = x ? p + __builtin_ctzll(x) : kFarPos;
                for (int d = 1; d < 64; d <<= 1) {
                    const long long ol = __shfl_up(last, d);
                    const long long of = __shfl_down(first, d);
                    if ((int)lane >= d && ol > last) last = ol;
                    if ((int)lane + d < 64 && of < first) first = of;
                }
                // (every lane takes part in the shuffles: a source lane that is switched off reads as 0)
                const long long ul = __shfl_up(last, 1), df = __shfl_down(first, 1);
                const long long el = lane == 0 ? kNoPos : ul;
                const long long ef = lane == 63 ? kFarPos : df;
                const long long l63 = __shfl(last, 63), f0 = __shfl(first, 0);
                *P = el > Pin ? el : Pin;
                *N = ef < Nin ? ef : Nin;
                *Pout = l63 > Pin ? l63 : Pin;
                *Nout = f0 < Nin ? f0 : Nin;
            };
            if (a.hr == 0) {
                for (uint64_t c = 0; c < nch; ++c) emit(c, source(c));
            } else if (nch == 1) {
                const uint64_t x = source(0);
                long long P, N, Po, No;
                scan(0, x, kNoPos, kFarPos, &P, &N, &Po, &No);
                emit(0, dilate_word(x, lane, P, N, a.hr) & tail_bits(lane, W64, w) & (lane < W64 ? ~0ull : 0ull));
            } else {
                // right to left: source words into dst, the first set position right of every chunk into ncarry
                long long Nc = kFarPos;
                long long* nc = a.ncarry + row * nch;
                for (uint64_t c = nch; c-- > 0;) {
                    const uint64_t x = source(c);
                    const uint64_t k = c * 64 + lane;
                    if (k < W64) a.dst[row * W64 + k] = x;
                    if (lane == 0) nc[c] = Nc;
                    long long P, N, Po, No;
                    scan(c, x, kNoPos, Nc, &P, &N, &Po, &No);
                    Nc = No;
                }
                __threadfence_block();
                long long Pc = kNoPos;
                for (uint64_t c = 0; c < nch; ++c) {
                    const uint64_t k = c * 64 + lane;
                    const uint64_t x = k < W64 ? a.dst[row * W64 + k] : 0;
                    long long P, N, Po, No;
                    scan(c, x, Pc, nc[c], &P, &N, &Po, &No);
                    Pc = Po;
                    emit(c, k < W64 ? dilate_word(x, k, P, N, a.hr) & tail_bits(k, W64, w) : 0);
                }
            }
        }
        if (a.final_) {
            cnt = wave_sum_u32(cnt);
            minx = wave_min_u32(minx);
            maxx = wave_max_u32(maxx);
            rowany = wave_max_u32(rowany);
            if (lane == 0) {
                red[wave][0] = minx; red[wave][1] = rowany ? (uint32_t)y : 0xFFFFFFFFu;
                red[wave][2] = maxx; red[wave][3] = rowany ? (uint32_t)y : 0u; red[wave][4] = cnt;
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                uint32_t r0 = red[0][0], r1 = red[0][1], r2 = red[0][2], r3 = red[0][3], r4 = red[0][4];
                for (int q = 1; q < 4; ++q) {
                    r0 = min(r0, red[q][0]); r1 = min(r1, red[q][1]);
                    r2 = max(r2, red[q][2]); r3 = max(r3, red[q][3]); r4 += red[q][4];
                }
                if (r4) {
                    uint32_t* s = a.stats + (blk / bpf) * 5;
                    atomicMax(s + 0, ~r0);
                    atomicMax(s + 1, ~r1);
                    atomicMax(s + 2, r2);
                    atomicMax(s + 3, r3);
                    atomicAdd(s + 4, r4);
                }
            }
            __syncthreads();
        }
    }
}

// One wave per column of words: OR prefixes (G) and suffixes (H) within blocks of B rows, 64 rows per step.
__global__ __launch_bounds__(256) void segment_column_kernel(const uint64_t* __restrict__ A, uint64_t* __restrict__ G,
                                                             uint64_t* __restrict__ H, uint64_t h, uint64_t W64,
                                                             uint64_t n_frames, uint64_t B) {
    const unsigned lane = threadIdx.x & 63;
    const uint64_t ncols = n_frames * W64, nck = (h + 63) / 64;
    for (uint64_t col = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); col < ncols; col += (uint64_t)gridDim.x * 4) {
        const uint64_t base = (col / W64) * h * W64 + col % W64;
        uint64_t carry = 0, cblk = ~0ull;
        for (uint64_t c = 0; c < nck; ++c) {
            const uint64_t y = c * 64 + lane;
            uint64_t v = y < h ? A[base + y * W64] : 0;
            const uint64_t b = block_of(c * 64, lane, B);
            for (int d = 1; d < 64; d <<= 1) {
                const uint64_t o = __shfl_up(v, d), ob = __shfl_up(b, d);
                if ((int)lane >= d && ob == b) v |= o;
            }
            if (b == cblk) v |= carry;
            if (y < h) G[base + y * W64] = v;
            carry = __shfl(v, 63);
            cblk = __shfl(b, 63);
        }
        carry = 0; cblk = ~0ull;
        for (uint64_t c = nck; c-- > 0;) {
            const uint64_t y = c * 64 + lane;
            uint64_t v = y < h ? A[base + y * W64] : 0;
            const uint64_t b = block_of(c * 64, lane, B);
            for (int d = 1; d < 64; d <<= 1) {
                const uint64_t o = __shfl_down(v, d), ob = __shfl_down(b, d);
                if ((int)lane + d < 64 && ob == b) v |= o;
            }
            if (b == cblk) v |= carry;
            if (y < h) H[base + y * W64] = v;
            carry = __shfl(v, 0);
            cblk = __shfl(b, 0);
        }
    }
}

// accumulators -> {x, y, w, h, count}; an empty mask gives [0,0,0,0] and 0 (:434-440)
__global__ __launch_bounds__(256) void segment_finalize_kernel(uint32_t* stats, uint64_t n_frames) {
    for (uint64_t f = (uint64_t)blockIdx.x * 256 + threadIdx.x; f < n_frames; f += (uint64_t)gridDim.x * 256) {
        uint32_t* s = stats + f * 5;
        const uint32_t c = s[4];
        if (!c) { s[0] = s[1] = s[2] = s[3] = 0; continue; }
        const uint32_t x = ~s[0], y = ~s[1];
        s[2] = s[2] - x + 1;
        s[3] = s[3] - y + 1;
        s[0] = x;
        s[1] = y;
    }
}

unsigned grid_cap(uint64_t blocks) { return (unsigned)(blocks < (1u << 20) ? (blocks ? blocks : 1) : (1u << 20)); }

// ---- stream compaction: count per item, exclusive scan, emit at the scanned offset (shared by the RLE and
// extract_person_rgb) ----------------------------------------------------------------------------------------

constexpr unsigned kCompactItems = 16;
constexpr uint64_t kCompactTile = 256 * kCompactItems;

__device__ __forceinline__ unsigned long long wave_incl_scan(unsigned long long v, unsigned lane) {
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long o = __shfl_up(v, d);
        if ((int)lane >= d) v += o;
    }
    return v;
}

template <class Op>
__global__ __launch_bounds__(256) void compact_count_kernel(Op op, uint64_t n, unsigned long long* tile_sums) {
    __shared__ unsigned long long part[4];
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t ntiles = (n + kCompactTile - 1) / kCompactTile;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t i0 = t * kCompactTile + (uint64_t)threadIdx.x * kCompactItems;
        unsigned long long s = 0;
        for (unsigned j = 0; j < kCompactItems; ++j)
            if (i0 + j < n) s += op.count(i0 + j);
        for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
        if (lane == 0) part[wave] = s;
        __syncthreads();
        if (threadIdx.x == 0) tile_sums[t] = part[0] + part[1] + part[2] + part[3];
        __syncthreads();
    }
}

// one workgroup: exclusive scan of the tile sums in place, the total into *total
__global__ __launch_bounds__(256) void compact_scan_kernel(unsigned long long* sums, uint64_t ntiles, unsigned long long* total) {
    __shared__ unsigned long long wsum[4];
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long carry = 0;
    for (uint64_t b = 0; b < ntiles; b += 256) {
        const uint64_t i = b + threadIdx.x;
        const unsigned long long v = i < ntiles ? sums[i] : 0;
        const unsigned long long incl = wave_incl_scan(v, lane);
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        unsigned long long woff = 0, all = 0;
        for (unsigned q = 0; q < 4; ++q) { if (q < wave) woff += wsum[q]; all += wsum[q]; }
        if (i < ntiles) sums[i] = carry + woff + incl - v;
        carry += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

template <class Op>
__global__ __launch_bounds__(256) void compact_emit_kernel(Op op, uint64_t n, const unsigned long long* __restrict__ tile_offsets) {
    __shared__ unsigned long long wsum[4];
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t ntiles = (n + kCompactTile - 1) / kCompactTile;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t i0 = t * kCompactTile + (uint64_t)threadIdx.x * kCompactItems;
        unsigned long long s = 0;
        for (unsigned j = 0; j < kCompactItems; ++j)
            if (i0 + j < n) s += op.count(i0 + j);
        const unsigned long long incl = wave_incl_scan(s, lane);
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        unsigned long long off = tile_offsets[t] + incl - s;
        for (unsigned q = 0; q < wave; ++q) off += wsum[q];
        for (unsigned j = 0; j < kCompactItems; ++j) {
            if (i0 + j >= n) break;
            const unsigned long long c = op.count(i0 + j);
            if (c) { op.emit(i0 + j, off, c); off += c; }
        }
        __syncthreads();
    }
}

// starts of maximal runs of (m[i] & 1) (:139-145)
struct RleStartOp {
    const uint8_t* m;
    unsigned long long* starts;
    __device__ unsigned long long count(uint64_t i) const { return i == 0 || ((m[i] ^ m[i - 1]) & 1u); }
    __device__ void emit(uint64_t i, unsigned long long off, unsigned long long) const { starts[off] = i; }
};

// a maximal run of L elements is ceil(L / 65535) triples [len u16 LE, value] (:143-151)
struct RlePieceOp {
    const uint8_t* m;
    const unsigned long long* starts;
    const unsigned long long* n_runs;
    uint64_t n;
    uint8_t* out;
    __device__ uint64_t run_len(uint64_t r) const { return (r + 1 < *n_runs ? starts[r + 1] : n) - starts[r]; }
    __device__ unsigned long long count(uint64_t r) const { return r < *n_runs ? (run_len(r) + 65534) / 65535 : 0; }
    __device__ void emit(uint64_t r, unsigned long long off, unsigned long long pieces) const {
        const uint64_t L = run_len(r);
        const uint8_t v = m[starts[r]] & 1u;
        for (unsigned long long p = 0; p < pieces; ++p) {
            const uint64_t len = min((uint64_t)65535, L - p * 65535);
            uint8_t* o = out + (off + p) * 3;
            o[0] = (uint8_t)(len & 0xFF);
            o[1] = (uint8_t)(len >> 8);
            o[2] = v;
        }
    }
};

// row-major walk over the bbox keeping mask bytes == 1 (:111-123); the host has checked that every index fits u32
struct ExtractOp {
    const uint8_t* mask;
    uint64_t mask_len;
    const uint8_t* rgb;
    uint64_t rgb_len;
    uint64_t width, bx, by, bw;
    uint8_t* out;
    __device__ uint64_t index(uint64_t t) const { return (by + t / bw) * width + bx + t % bw; }
    __device__ unsigned long long count(uint64_t t) const {
        const uint64_t mi = index(t);
        return mi < mask_len && mask[mi] == 1 && mi * 3 + 2 < rgb_len;
    }
    __device__ void emit(uint64_t t, unsigned long long off, unsigned long long) const {
        const uint64_t mi = index(t);
        uint8_t* o = out + off * 3;
        o[0] = rgb[mi * 3]; o[1] = rgb[mi * 3 + 1]; o[2] = rgb[mi * 3 + 2];
    }
};

template <class Op>
void run_compact(const Op& op, uint64_t n, unsigned long long* d_tiles, unsigned long long* d_total, hipStream_t st) {
    const uint64_t ntiles = (n + kCompactTile - 1) / kCompactTile;
    hipLaunchKernelGGL(compact_count_kernel<Op>, dim3(grid_cap(ntiles)), dim3(256), 0, st, op, (uint64_t)n, d_tiles);
    hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(256), 0, st, d_tiles, ntiles, d_total);
    hipLaunchKernelGGL(compact_emit_kernel<Op>, dim3(grid_cap(ntiles)), dim3(256), 0, st, op, (uint64_t)n,
                       (const unsigned long long*)d_tiles);
}

uint64_t compact_tiles(uint64_t n) { return (n + kCompactTile - 1) / kCompactTile; }

}  // namespace

// ---- host side -----------------------------------------------------------------------------------------------

static uint64_t seg_words(uint32_t w, uint32_t h, uint32_t n_frames) {
    return (uint64_t)n_frames * h * (((uint64_t)w + 63) / 64);
}

uint64_t segment_scratch_bytes(uint32_t w, uint32_t h, uint32_t n_frames, uint32_t dilate_radius, uint32_t erode_radius) {
    if (!dilate_radius && !erode_radius) return 0;
    const uint64_t W64 = ((uint64_t)w + 63) / 64, nch = (W64 + 63) / 64;
    const uint64_t carry = nch > 1 ? (uint64_t)n_frames * h * nch * 8 : 0;
    return 3 * seg_words(w, h, n_frames) * 8 + carry;
}

static void row_stage(int src, SegRowArgs a, hipStream_t st) {
    const uint64_t blocks = ((a.h + 3) / 4) * a.n_frames;
    const dim3 g(grid_cap(blocks)), b(256);
    switch (src) {
    case kSegMotion: hipLaunchKernelGGL(segment_row_kernel<kSegMotion>, g, b, 0, st, a); break;
    case kSegCg: hipLaunchKernelGGL(segment_row_kernel<kSegCg>, g, b, 0, st, a); break;
    case kSegRgb: hipLaunchKernelGGL(segment_row_kernel<kSegRgb>, g, b, 0, st, a); break;
    default: hipLaunchKernelGGL(segment_row_kernel<kSegPacked>, g, b, 0, st, a); break;
    }
}

void launch_segment(const SegSource& src, uint32_t w, uint32_t h, uint32_t n_frames, uint32_t dilate_radius,
                    uint32_t erode_radius, void* d_scratch, uint8_t* d_mask, uint32_t* d_stats, hipStream_t st) {
    (void)hipMemsetAsync(d_stats, 0, (size_t)n_frames * 5 * sizeof(uint32_t), st);
    const uint64_t W64 = ((uint64_t)w + 63) / 64, words = seg_words(w, h, n_frames);
    uint64_t* A = (uint64_t*)d_scratch;
    uint64_t* G = A + words;
    uint64_t* H = G + words;
    long long* carry = (long long*)(H + words);
    SegRowArgs a{};
    a.px = src; a.w = w; a.h = h; a.n_frames = n_frames; a.W64 = W64; a.ncarry = carry; a.mask = d_mask; a.stats = d_stats;
    const unsigned col_grid = grid_cap(((uint64_t)n_frames * W64 + 3) / 4);
    // B = 2r+1 in 64 bits (2^33 - 1 for r = 2^32 - 1), clamped to the height
    auto block_len = [&](uint64_t r) { const uint64_t B = 2 * r + 1; return B < h ? B : (uint64_t)h; };
    auto column = [&](uint64_t r) {
        hipLaunchKernelGGL(segment_column_kernel, dim3(col_grid), dim3(256), 0, st, (const uint64_t*)A, G, H, (uint64_t)h,
                           W64, (uint64_t)n_frames, block_len(r));
    };
    auto from_columns = [&](uint64_t r) { a.G = G; a.H = H; a.vr = r; a.vB = block_len(r); };
    int first = src.kind;
    if (dilate_radius) {
        a.hr = dilate_radius; a.dst = A;
        row_stage(first, a, st);
        column(dilate_radius);
        from_columns(dilate_radius);
        first = kSegPacked;
    }
    if (erode_radius) {
        a.invert = 1; a.hr = erode_radius; a.dst = A;
        row_stage(first, a, st);
        column(erode_radius);
        from_columns(erode_radius);
        first = kSegPacked;
    } else {
        a.invert = 0;
    }
    // final stage: the last vertical combine (complemented after an erosion), or the threshold itself
    a.hr = 0; a.dst = nullptr; a.final_ = 1;
    row_stage(first, a, st);
    hipLaunchKernelGGL(segment_finalize_kernel, dim3(grid_cap(((uint64_t)n_frames + 255) / 256)), dim3(256), 0, st,
                       d_stats, (uint64_t)n_frames);
}

uint64_t compact_scratch_bytes(uint64_t n_items) { return (compact_tiles(n_items) + 2) * 8; }

uint64_t rle_scratch_bytes(uint64_t n) { return n * 8 + compact_scratch_bytes(n) + 8; }

void launch_rle(const uint8_t* d_mask, uint64_t n, uint8_t* d_out, void* d_scratch, unsigned long long* d_pieces,
                hipStream_t st) {
    unsigned long long* starts = (unsigned long long*)d_scratch;
    unsigned long long* n_runs = starts + n;
    unsigned long long* tiles = n_runs + 1;
    run_compact(RleStartOp{d_mask, starts}, n, tiles, n_runs, st);
    run_compact(RlePieceOp{d_mask, starts, n_runs, n, d_out}, n, tiles, d_pieces, st);
}

void launch_extract_person(const uint8_t* d_mask, uint64_t mask_len, const uint8_t* d_rgb, uint64_t rgb_len, uint32_t width,
                           const uint32_t bbox[4], uint8_t* d_out, void* d_scratch, unsigned long long* d_count,
                           hipStream_t st) {
    const uint64_t n = (uint64_t)bbox[2] * bbox[3];
    ExtractOp op{d_mask, mask_len, d_rgb, rgb_len, width, bbox[0], bbox[1], bbox[2], d_out};
    run_compact(op, n, (unsigned long long*)d_scratch, d_count, st);
}

}  // namespace alice
