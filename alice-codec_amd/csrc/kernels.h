// Kernel launch interface (host side) for the gfx950 ALICE-Codec path.
#pragma once

#include <vector>

#include "common.h"

namespace alice {

constexpr uint32_t kRansOverflow = 4u;   // output region too small (host retries with 2N+4)
constexpr uint32_t kRansInternal = 8u;   // invariant violated (never expected)

struct RansResult {
    unsigned long long len;   // encode: stream bytes; decode: stream bytes consumed
    uint32_t flags;
    uint32_t final_state;
    uint32_t fast_tiles;      // decode: tiles taken by the scalar fast path / by the exact lane loop
    uint32_t slow_tiles;      // encode: tiles taken by the one-compare clean path / block by block
    // diagnostics (ALICE_CODEC_DEBUG): shader cycles and 100 MHz ticks the chain took (kibi-units), where it ran
    uint32_t cycles_k, ticks_k;
    uint32_t hw_id;           // HW_REG_HW_ID: wave [3:0], SIMD [5:4], pipe [7:6], CU [11:8], SH [12], SE [15:13]
    uint32_t xcc_id;          // HW_REG_XCC_ID [3:0]
    uint32_t paths;           // which branches of the tile loop ran (decode: kDecPath*, encode: kEncPath*), for the test-suite's coverage check
    uint32_t comp_blocks;     // encode: 64-symbol blocks of clean tiles that took the complement step (ripple64_comp_run)
};

constexpr uint32_t kDecPathDry = 1u;          // stream exhausted: no-window tile
constexpr uint32_t kDecPathWhole = 2u;        // fast tile on a window that lies wholly inside the stream
constexpr uint32_t kDecPathSpecKept = 4u;     // fast tile on a zero-padded window, no padding consumed
constexpr uint32_t kDecPathSpecDropped = 8u;  // ... padding consumed: result dropped, exact loop redid the tile
constexpr uint32_t kDecPathPendingFed = 16u;  // renormalisation owed by an exact-loop symbol settled before a fast tile
constexpr uint32_t kDecPathExact = 32u;       // exact scalar-lane loop
constexpr uint32_t kDecPathStarved = 64u;     // exact loop stopped at the end of its window with bytes still owed
constexpr uint32_t kDecPathTail = 128u;       // last tile of fewer than 4096 symbols
constexpr uint32_t kDecPathUnaligned = 256u;  // output not dword aligned
constexpr uint32_t kDecPathBelowL = 512u;     // fast tile refused: state below 2^23 with no renormalisation owed
constexpr uint32_t kDecPathStillStarved = 1024u;  // fast tile refused: the owed renormalisation could not reach 2^23

constexpr uint32_t kEncPathClean = 1u;         // full tile through the one-compare step (ripple64_clean)
constexpr uint32_t kEncPathCapRefused = 2u;    // full tile of a clean chain block by block: no room for a tile's worst case
constexpr uint32_t kEncPathNotClean = 4u;      // full tile block by block: table not verified clean, or a start state other than 2^23
constexpr uint32_t kEncPathTail = 8u;          // first tile of fewer than 1024 symbols (the chain runs back to front)
constexpr uint32_t kEncPathExact = 16u;        // exact serial block: a frequency of 0 or above 4096 in use
constexpr uint32_t kEncPathNoRoom = 32u;       // a block's bytes or the four state bytes refused for lack of room
constexpr uint32_t kEncPathFunnel = 64u;       // symbols not dword aligned: five-dword funnel shift
constexpr uint32_t kEncPathBytewiseEnd = 128u; // ... within 20 bytes of the end of the symbols: byte loads
constexpr uint32_t kEncPathBytewiseHead = 256u;  // lane's 16 bytes start before symbol 0 (tail tile): byte loads

struct RansDecodeDesc {
    const uint8_t* in;        // channel stream
    unsigned long long in_len;
    uint8_t* out;             // n symbols
    unsigned long long n;
    const RansTable* table;   // built by rans_table_kernel from the stored channel histogram
    // a RansDecoder object that has decoded before continues from where it stopped (src/rans.rs:351-381): state and
    // position of the next stream byte instead of the four head bytes
    uint32_t resume, x0;
    unsigned long long pos0;
    // where the chain's result goes; null: results[chain] of the launch.  (Chains of several callers merged into one
    // launch -- codec.hip, ChainHub -- report into their callers' own buffers.)
    RansResult* result;
};

// One encode chain of a merged launch (launch_rans_encode_descs): what launch_rans_encode derives from a base, strides and
// the chain number, spelled out per chain.
struct RansEncodeDesc {
    const uint8_t* sym;       // n symbols
    unsigned long long n;
    const RansTable* table;
    uint8_t* region;          // the stream is written back to front into [region, region + cap)
    unsigned long long cap;
    RansResult* result;
    uint32_t x_init;          // kRansL for a fresh encoder; a RansEncoder object between calls brings its state
    uint32_t keep_open;       // 1: leave the four state bytes of finish() unwritten (the object lives on)
};

// ---- rans.hip ----
// n_symbols <= 256: length of the histogram slice (FrequencyTable::from_histogram(&[u32]), src/rans.rs:102-104); bins from
// n_symbols on are ignored and the symbols do not exist in the table (freq 0)
// d_used (256 counts per chain, or null = d_hist): the histogram of the symbols the encoder will really see.  The table is
// d_hist's; the flags that let the encode chain skip its per-block table check (kTableVerified and its two companions)
// are d_used's.  For a histogram that is the caller's word, not a count of the data.
void launch_rans_table(const uint32_t* d_hist, RansTable* d_tables, int n_chains, hipStream_t st, uint32_t n_symbols = 256,
                       const uint32_t* d_used = nullptr);
void launch_rans_table_from_arrays(const uint16_t* d_cum, const uint16_t* d_freq, RansTable* d_table,
                                   hipStream_t st);
// n tables in one launch: cum and freq are [n][256], table i comes out byte for byte what the call above writes for row i
void launch_rans_tables_from_arrays(const uint16_t* d_cum, const uint16_t* d_freq, RansTable* d_tables, int n,
                                    hipStream_t st);
// chain c reads sym + c*sym_stride (n symbols) and writes its stream back-to-front into a cap-sized region;
// the stream is the last results[c].len bytes of that region.  group_stride == 0: region c starts at
// out + c*cap.  Otherwise chains 3g, 3g+1, 3g+2 write into chunk g's .alc buffer: region start =
// out + g*group_stride + group_head + (c % 3)*cap.  Chains c >= n_split encode n - 1 symbols.
// cap_co / cap_cg (grouped mode only, 0 = same as cap): the second and third chain of a group get regions of their own
// sizes, laid out back to back behind the first (Y streams are about twice as long as Co / Cg streams).
void launch_rans_encode(const uint8_t* d_sym, uint64_t sym_stride, uint64_t n, const RansTable* d_tables,
                        uint8_t* d_out, uint64_t cap, RansResult* d_results, int n_chains, hipStream_t st,
                        uint64_t group_stride = 0, uint64_t group_head = 0, unsigned n_split = 0xFFFFFFFFu,
                        uint64_t cap_co = 0, uint64_t cap_cg = 0, uint32_t x_init = kRansL, bool keep_open = false);
// x_init / keep_open: a RansEncoder object between calls (src/rans.rs:269-294): the chain starts from the object's state
// and leaves the four state bytes of finish() unwritten (results[c].final_state carries the state on)
// out_j[k] = in[4k + j] for the four sub-sequences of an interleaved stream (out_j = out + j*stride)
void launch_split4(const uint8_t* d_in, uint64_t n, uint8_t* d_out, uint64_t stride, hipStream_t st);
// InterleavedRansDecoder::decode_n order (src/rans.rs:501-519): symbol k of stream j lands at
// sum_i min(count_i, k) + #{i < j : count_i > k}; positions >= n_out are dropped.  have[j] symbols of stream j
// are present in d_in (the ones that land below n_out), count[j] is the header's count.
void launch_merge4(const uint8_t* d_in, uint64_t stride, const uint64_t have[4], const uint64_t count[4], uint8_t* d_out,
                   uint64_t n_out, hipStream_t st);
void launch_rans_decode(const RansDecodeDesc* d_descs, RansResult* d_results, int n_chains, hipStream_t st);
// chains described one by one; every desc names its result, its start state and whether the stream is finished
void launch_rans_encode_descs(const RansEncodeDesc* d_descs, int n_chains, hipStream_t st);
// what the runtime reports for the one-chain-per-SIMD instances: out[0..2] = encoder registers per lane (VGPR + AGPR),
// static LDS bytes, workgroups per CU it would co-schedule; out[3..5] = decoder.  False when a query failed.
bool chain_kernel_occupancy(uint32_t out[6]);

// Where a chunk's interleaved RGB pixels live: pixel x of row y of frame t at base + t * frame_pitch + y * row_pitch + 3 * x,
// for x < w, y < h, t < f of the chunk.  A chunk stored on its own is packed (row_pitch 3w, frame_pitch 3wh); a region of
// larger frames points base at its origin pixel and keeps the frames' pitches.  All offsets are 64-bit.
struct RgbLayout {
    uint8_t* base;
    uint64_t row_pitch, frame_pitch;
};
inline RgbLayout packed_rgb(const void* p, const ChunkDims& d) { return RgbLayout{(uint8_t*)p, 3ull * d.w, 3ull * d.w * d.h}; }
inline bool rgb_is_packed(const RgbLayout& l, const ChunkDims& d) { return l.row_pitch == 3ull * d.w && l.frame_pitch == 3ull * d.w * d.h; }
// the tile kernels' dword loads / stores: every row start 4-byte aligned (a 16-pixel segment starts at a multiple of 48
// bytes into its row), and a region of 4-aligned width-W frames qualifies when W % 4 == 0 and x0 % 4 == 0
inline bool rgb_dword_aligned(const RgbLayout& l) { return (((uintptr_t)l.base) & 3u) == 0 && l.row_pitch % 4 == 0 && l.frame_pitch % 4 == 0; }

// ---- transform.hip (pipeline-specialised: RGB <-> u8 symbols) ----
// A chunk is processed in BANDS of whole tile rows so that a band's intermediate (i16 after the spatial pass, i16 / i32
// after the inverse temporal pass) stays in the Infinity Cache between the two passes, and every launch runs the
// temporal role of one band beside the tile role of its neighbour (transform.hip, "Band-ordered, role-fused launches").
struct BandPlan {
    int tile_h, tiles_y;   // tile height of the tile pass, tile rows of the frame
    int tpb, n_bands;      // tile rows per band, bands (1 = the frame is not cut)
    size_t slot_bytes;     // scratch the launches of one chunk need
};
// false: the shape needs the generic path -- a padded width or height below 6 (the tile kernels read their halo
// through one reflection), a frame of more than 2^30 samples (32-bit offsets inside a frame), or more tiles than a
// 1-D grid holds.
bool transform_tiles_eligible(const ChunkDims& d);
// scratch (one band slot) the forward / inverse launches of a chunk of this shape need; the caller owns the buffer
size_t forward_scratch_bytes(const ChunkDims& d);
size_t inverse_scratch_bytes(const ChunkDims& d, bool mid16);
bool inverse_cuts_chunk(const ChunkDims& d);   // the inverse launches of this shape work band by band (see launch_inverse_transform)
// measurement only (alice_codec_test_transform_ms): the calling thread's next launches of the CDF 9/7 instances run their
// probe twins: 0 off, 1 loads and stores replaced by register moves (the VALU floor), 2 loads only, 3 stores only
void set_transform_probe(int mode);
// target size of a band slot in KiB (0 = never cut; negative = keep).  Process-wide; meant for tests and probes.
void set_transform_tuning(long band_kb);
// radius of the forward temporal kernel's value -> symbol table (clamped to 1 .. 2048, the default).  Process-wide; tests only.
void set_value_table_radius(int r);
int value_table_radius();
// Launches of one chunk on `st`, band after band (tile pass then temporal pass; the inverse the other way round).
// hist: uint32 [3][256], zeroed by the caller.  Returns false (nothing launched) when the shape needs the generic path.
bool launch_forward_transform(const RgbLayout& rgb, const ChunkDims& d, int wavelet, int32_t step,
                              void* d_scratch, uint8_t* d_sym, uint32_t* d_hist, hipStream_t st);
// The same band loop for the rate prediction: the temporal pass counts the unquantised coefficients of each channel into
// bins[c * 4096 + value + r] (r = value_table_radius(); zeroed by the caller) and values outside [-r, r) into *oor.
// Returns false (nothing launched) when the shape needs the generic path.
bool launch_forward_coef_hist(const RgbLayout& rgb, const ChunkDims& d, int wavelet, void* d_scratch, uint32_t* d_bins,
                              uint32_t* d_oor, hipStream_t st);
// steps per channel come from the chunk header.  exact = 64-bit lifting products.  mid16 = the intermediate after the
// temporal pass provably fits i16 (halves its traffic); lds16 = so does everything after the column pass (packed tile).
// When the chunk is cut into bands the pixels of the first band are written while the symbols of later bands are still
// unread: the pixels must not overlap d_sym then (an uncut chunk may decode over its own symbols).  Only the w x h x f
// pixels of `rgb` are written: no byte between or beside the rows of a region.
// The instance the flags select: 0 exact (wrapping i32 sums, 64-bit products), 1 fast i32 (24-bit multiply-adds, i32 band
// slot), 2 fast with an i16 band slot and the lane-exchange tile, 3 fast with an i16 band slot and the packed i16 LDS tile.
inline int inverse_variant(bool exact, bool mid16, bool lds16) { return exact ? 0 : (mid16 ? (lds16 ? 3 : 2) : 1); }
bool launch_inverse_transform(const uint8_t* d_sym, const ChunkDims& d, int wavelet, const int32_t step[3],
                              bool exact, bool mid16, bool lds16, void* d_scratch, const RgbLayout& rgb, hipStream_t st);
// The wide twins (.alc v3): the temporal passes write / read untruncated u16 symbols z (0, 2q - 1, -2q) and the histogram
// bins min(z, 255); the tile passes, band plans and scratch sizes are those above.
bool launch_forward_transform_wide(const RgbLayout& rgb, const ChunkDims& d, int wavelet, int32_t step,
                                   void* d_scratch, uint16_t* d_sym, uint32_t* d_hist, hipStream_t st);
bool launch_inverse_transform_wide(const uint16_t* d_sym, const ChunkDims& d, int wavelet, const int32_t step[3],
                                   bool exact, bool mid16, bool lds16, void* d_scratch, const RgbLayout& rgb, hipStream_t st);
// The reversible twin (.alc v4): the wide launcher with the mirrored instances of both roles -- every
// lifting step subtracts the forward's own delta.  Same symbols, bands, scratch and instance flags.
bool launch_inverse_transform_reversible(const uint16_t* d_sym, const ChunkDims& d, int wavelet, const int32_t step[3],
                                         bool exact, bool mid16, bool lds16, void* d_scratch, const RgbLayout& rgb, hipStream_t st);
// Frame ranges: d_sym is the symbol volume of a virtual chunk dv (u8 for format 0 = .alc v2, u16 for
// 1 = v3 and 2 = v4, mirrored); its inverse runs with the instance flags the full chunk takes, and only frames
// [win.lo, win.hi) of it reach the spatial pass and `rgb` (a layout of win.hi - win.lo frames).  The scratch is
// inverse_scratch_bytes(make_dims(w, h, win.hi - win.lo), mid16): the slot holds the frames that are kept.
struct FrameWindow { uint32_t lo, hi; };
bool launch_inverse_transform_window(const void* d_sym, const ChunkDims& dv, const FrameWindow& win, int format, int wavelet,
                                     const int32_t step[3], bool exact, bool mid16, bool lds16, void* d_scratch, const RgbLayout& rgb,
                                     hipStream_t st);
// Half-resolution preview: d_sym is the compact volume [3][planes][pitch] of the low-low quadrants of a
// virtual chunk's planes (u8 for format 0, u16 for 1 and 2; pitch a multiple of 4, q = qw * qh <= pitch quadrant pixels per
// plane).  One fused launch: symbols -> dequantise -> inverse temporal lifting of the three channels in lock step -> DC
// normalisation -> `as i16` -> colour; frames [win.lo, win.hi) of the virtual chunk go to d_rgb as (hi - lo) * q * 3 packed
// bytes.  No tile geometry: every shape takes this path.  False (nothing launched): arguments that are no such volume.
constexpr int kPreviewGainOne = 65536;    // CDF 5/3, Haar: the low band's DC gain is exactly 1
constexpr int kPreviewGain97 = 47484;     // CDF 9/7: round(65536 / g^2), g = 1.17480326 per spatial axis
bool launch_preview_inverse(const void* d_sym, uint64_t pitch, uint64_t q, uint32_t planes, const FrameWindow& win, int format,
                            int wavelet, const int32_t step[3], bool exact, uint8_t* d_rgb, hipStream_t st);
// The same finish over many volumes in one queue (the batched preview).  preview_records_plan checks
// every item as launch_preview_inverse checks its arguments, groups the items by instance class (format x lifting steps x
// exact: at most 12), writes their device records, class after class, to h_records (n * preview_record_bytes() bytes) and
// names one launch per class present; false: an item is no such volume, nothing was written that matters.  After the
// records have been copied to d_records, launch_preview_inverse_many runs one class: a flattened work list, so the grid is
// the sum of the items' own workgroups whatever their sizes.
struct PreviewFinish {
    const void* d_sym;
    uint64_t pitch, q;
    uint32_t planes;
    FrameWindow win;
    int format, wavelet;
    int32_t step[3];
    bool exact;
    uint8_t* d_rgb;
};
struct PreviewFinishLaunch { int cls; uint32_t first, count, grid; };   // records [first, first + count), `grid` workgroups
size_t preview_record_bytes();
bool preview_records_plan(const PreviewFinish* items, uint32_t n, void* h_records, std::vector<PreviewFinishLaunch>& launches);
void launch_preview_inverse_many(const void* d_records, const PreviewFinishLaunch& l, hipStream_t st);
// The window inverse over many virtual chunks in one queue (batched frame ranges and rectangles).  An
// item is what launch_inverse_transform_window takes, with a band slot of its own (d_slot: inverse_scratch_bytes of the kept
// frames' chunk).  rects_finish_batchable: the tile kernels take dv and the kept frames' inverse is one band; every other
// item runs through launch_inverse_transform_window (or the generic path) on its own.  rects_records_plan checks every item
// as the single launcher checks its arguments, derives the two roles' arguments with the single launcher's code, groups the
// items by instance class with a stable sort -- temporal role: lifting steps x {exact i32, fast i32, i16} x {u8, wide, wide
// mirrored}, 18; tile role: lifting steps x inverse_variant x mirrored, 16 -- writes the records of each role, class after
// class, to h_t_records / h_xy_records (n * rects_record_bytes(role) bytes each) and names the launches: every temporal
// launch, then every tile launch.  false: an item is no such volume.  launch_rects_inverse_many runs one of them over the
// records' device copies: a flattened work list whose grid is the sum of the items' own workgroups (tile role: padded to a
// multiple of 8, the XCD order over the whole list).
struct RectFinish {
    const void* d_sym;
    ChunkDims dv;
    FrameWindow win;
    int format, wavelet;
    int32_t step[3];
    bool exact, mid16, lds16;
    void* d_slot;
    RgbLayout rgb;               // win.hi - win.lo frames of dv.w x dv.h
};
struct RectFinishLaunch { int role, cls; uint32_t first, count, grid; };   // role 0 temporal, 1 tile; records [first, first + count)
size_t rects_record_bytes(int role);
bool rects_finish_batchable(const ChunkDims& dv, uint32_t frames_kept, bool exact, bool mid16);
bool rects_records_plan(const RectFinish* items, uint32_t n, void* h_t_records, void* h_xy_records, std::vector<RectFinishLaunch>& launches);
void launch_rects_inverse_many(const void* d_t_records, const void* d_xy_records, const RectFinishLaunch& l, hipStream_t st);

// ---- transform.hip, stage level: Wavelet2D / Wavelet3D of caller-shaped i32 data on the tile kernels' exact instances ----
// eligible: even width and height >= 6, even depth (or depth 1); otherwise the caller uses launch_wavelet_axis.
bool stage_tiles_eligible(uint64_t w, uint64_t h, uint64_t depth, int ndim);
// in place for the caller (result in d_data); d_tmp: same size.  ndim 2: `depth` independent planes.
void launch_stage_wavelet(int32_t* d_data, int32_t* d_tmp, uint64_t w, uint64_t h, uint64_t depth, int ndim, int wavelet,
                          bool inverse, hipStream_t st);

// ---- generic.hip (stage-level API on arbitrary i32 data; exact reference arithmetic) ----
// 1-D transform of n_lines lines: element k of line (a, b) is at data[a*stride_a + b*stride_b + k*stride_k],
// a in [0, n_a), b in [0, n_b).  tmp: same size as data.
// Cap on the workgroups of the launches sized per item (grid_for in generic.hip); 0 restores the default, 65535 * 4.  The
// launches that clamp further (to 2048) still do.  Process-wide; tests only.
void set_generic_grid_cap(uint32_t max_blocks);
// grid_for for the launches outside generic.hip that are sized per item and obey the same cap (quality.hip)
unsigned generic_grid_for(unsigned long long items);
void launch_wavelet_axis(int32_t* d_data, int32_t* d_tmp, uint64_t n, uint64_t stride_k, uint64_t n_a,
                         uint64_t stride_a, uint64_t n_b, uint64_t stride_b, int wavelet, bool inverse,
                         hipStream_t st, bool mirror = false);   // mirror (inverse only): the mirrored inverse of .alc v4
void launch_rgb_to_ycocg(const uint8_t* d_rgb, uint64_t n_pixels, int16_t* y, int16_t* co, int16_t* cg, hipStream_t st);
void launch_ycocg_to_rgb(const int16_t* y, const int16_t* co, const int16_t* cg, uint64_t n_pixels, uint8_t* d_rgb, hipStream_t st);
// the same for the w x h x f pixels of a chunk at any layout (planes packed [f][h][w]; a packed layout takes the calls above)
void launch_rgb_to_ycocg(const RgbLayout& rgb, const ChunkDims& d, int16_t* y, int16_t* co, int16_t* cg, hipStream_t st);
void launch_ycocg_to_rgb(const int16_t* y, const int16_t* co, const int16_t* cg, const ChunkDims& d, const RgbLayout& rgb, hipStream_t st);
// Rectangle paste: the w x h pixels at (x, y) of each of n_frames frames of `src` go to pixels
// (0, 0) .. of the frames of `dst`; nothing else of dst is written and nothing else of src is read.  Any alignment.
void launch_rgb_rect_paste(const RgbLayout& src, uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint32_t n_frames, const RgbLayout& dst,
                           hipStream_t st);
// Many such pastes in one queue (batched rectangles).  rect_paste_records_plan groups the items by the
// piece width the single launcher would pick (16, 4 or 1 bytes: the same alignment test on both sides) with a stable sort,
// writes their device records, widest group first, to h_records (n * rect_paste_record_bytes() bytes) and names one launch
// per width present; an item's workgroups are what the single launcher's grid would be.  false: an empty rectangle.
struct RectPaste {
    RgbLayout src;
    uint32_t x, y, w, h, n_frames;
    RgbLayout dst;
};
struct RectPasteLaunch { int piece; uint32_t first, count, grid; };   // records [first, first + count), `grid` workgroups
size_t rect_paste_record_bytes();
bool rect_paste_records_plan(const RectPaste* items, uint32_t n, void* h_records, std::vector<RectPasteLaunch>& launches);
void launch_rgb_rect_paste_many(const void* d_records, const RectPasteLaunch& l, hipStream_t st);
void launch_pad_channel(const int16_t* ch, const ChunkDims& d, int32_t* out, hipStream_t st);
void launch_strip_channel(const int32_t* in, const ChunkDims& d, int16_t* ch, hipStream_t st);
void launch_quantize(const int32_t* in, int32_t* out, uint64_t n, int32_t step, int32_t dead_zone, hipStream_t st);
void launch_fast_quantize(const int32_t* in, int32_t* out, uint64_t n, uint64_t reciprocal, uint32_t shift,
                          int32_t dead_zone, hipStream_t st);
void launch_dequantize(const int32_t* in, int32_t* out, uint64_t n, int32_t step, hipStream_t st);
void launch_to_symbols(const int32_t* in, uint8_t* out, uint64_t n, hipStream_t st);
void launch_from_symbols(const uint8_t* in, int32_t* out, uint64_t n, hipStream_t st);
void launch_histogram(const uint8_t* sym, uint64_t n, uint32_t* hist /*zeroed*/, hipStream_t st);
// wide twins: z untruncated as u16 (the caller guarantees |q| <= 32767); the histogram bins min(z, 255)
void launch_to_symbols_wide(const int32_t* in, uint16_t* out, uint64_t n, hipStream_t st);
void launch_from_symbols_wide(const uint16_t* in, int32_t* out, uint64_t n, hipStream_t st);
void launch_histogram_wide(const uint16_t* sym, uint64_t n, uint32_t* hist /*zeroed*/, hipStream_t st);
// ssim (src/ssim.rs): per-8x8-block values in raster order; f64 fold in element order; 2x2 truncating mean
void launch_ssim_blocks(const uint8_t* d_a, const uint8_t* d_b, uint64_t width, uint64_t bw, uint64_t nblocks, double* d_out, hipStream_t st);
void launch_ordered_sum_f64(const double* d_v, uint64_t n, double* d_out, hipStream_t st);
void launch_downsample2(const uint8_t* d_in, uint64_t width, uint64_t height, uint8_t* d_out, hipStream_t st);
// AnalyticalRDO::estimate_variance pieces: exact i64 sum; f64 sum of (x - mean)^2 in element order
void launch_sum_i32(const int32_t* d_x, uint64_t n, unsigned long long* d_sum /*zeroed*/, hipStream_t st);
void launch_ordered_sqdev_sum(const int32_t* d_x, uint64_t n, double mean, double* d_out, hipStream_t st);
void launch_sq_diff_sum(const uint8_t* a, const uint8_t* b, uint64_t n, unsigned long long* d_sum /*zeroed*/, hipStream_t st);
// Each chunk's .alc buffer holds, behind `head` bytes, three cap-sized regions with a stream at the tail of
// each; moves the streams, in place, to directly behind the 3138-byte header slot.
constexpr uint64_t kStreamHead = 3328;   // >= kAlcHeaderBytes, multiple of 256
void launch_compact_streams(uint8_t* d_alc, uint64_t alc_stride, uint64_t head, const uint64_t cap[3],
                            const RansResult* d_results, int n_chunks, hipStream_t st);
// fills the 3138-byte headers on the device (magic, dims, per-channel fields, histograms)
void launch_write_headers(uint8_t* d_alc, uint64_t alc_stride, const ChunkDims& d, int wavelet, int32_t step,
                          const uint32_t* d_hist, const RansResult* d_results, unsigned long long* d_sizes,
                          int n_chunks, hipStream_t st);

// ---- segment.hip: person segmentation (reference src/segment.rs) ----
enum SegSourceKind : int { kSegMotion = 0, kSegCg = 1, kSegRgb = 2, kSegPacked = 3 };
// the first stage's pixels: frames [f][h][w] back to back
struct SegSource {
    int kind;                 // kSegMotion, kSegCg (planar i16 Cg) or kSegRgb (interleaved RGB, Cg computed on load)
    const uint8_t* cur;       // motion: current frames
    const uint8_t* ref;       // motion: reference frame(s); frame f at ref + f * ref_stride
    uint64_t ref_stride;
    uint8_t motion_threshold;
    const int16_t* cg;
    const uint8_t* rgb;
    int16_t green_threshold;
};
// device scratch launch_segment needs (0 when both radii are 0)
uint64_t segment_scratch_bytes(uint32_t w, uint32_t h, uint32_t n_frames, uint32_t dilate_radius, uint32_t erode_radius);
// threshold, dilate, erode, then d_mask (u8, may be null) and d_stats (n_frames x {x, y, w, h, count}); w*h > 0
void launch_segment(const SegSource& src, uint32_t w, uint32_t h, uint32_t n_frames, uint32_t dilate_radius,
                    uint32_t erode_radius, void* d_scratch, uint8_t* d_mask, uint32_t* d_stats, hipStream_t st);
// rle_encode_mask of n > 0 bytes into d_out (>= 3n bytes); *d_pieces = number of 3-byte triples written
uint64_t rle_scratch_bytes(uint64_t n);
void launch_rle(const uint8_t* d_mask, uint64_t n, uint8_t* d_out, void* d_scratch, unsigned long long* d_pieces, hipStream_t st);
// extract_person_rgb over bbox = {x, y, w, h} with w*h > 0 into d_out (>= 3*w*h bytes); *d_count = pixels written.
// Every mask index (y+h-1)*width + x+w-1 must fit u32 (checked by the caller).
uint64_t compact_scratch_bytes(uint64_t n_items);
void launch_extract_person(const uint8_t* d_mask, uint64_t mask_len, const uint8_t* d_rgb, uint64_t rgb_len, uint32_t width,
                           const uint32_t bbox[4], uint8_t* d_out, void* d_scratch, unsigned long long* d_count,
                           hipStream_t st);

// ---- rate.hip: size prediction (see the derivation at the top of rate.hip) ----
enum RateStatus : uint32_t { kRateBounded = 0, kRateUnbounded = 1, kRateDiverges = 2 };
constexpr int kRateFracBits = 24;
struct RateChannel {          // one (chunk, step, channel): stream bytes lo <= len <= hi when status == kRateBounded
    unsigned long long lo, hi;
    uint32_t status, pad_;
};
struct RateLogTable {
    uint32_t lo[kProbScale + 1], hi[kProbScale + 1];   // floor / ceil of log2(4096 / f) * 2^24
    uint32_t g_up, g_dn;                               // ceil(log2(1 + 2^-11) * 2^24), ceil(-log2(1 - 2^-11) * 2^24)
};
const RateLogTable& rate_log_table();
// generic path: bins of one channel's coefficient volume (n values), same layout and counter as launch_forward_coef_hist
void launch_coef_hist(const int32_t* d_vol, uint64_t n, uint32_t* d_bins, uint32_t* d_oor, hipStream_t st);
// step_hist: [chunk][step - 1][channel][256]; chunks with a non-zero out-of-range counter are left alone
void launch_rate_fold(const uint32_t* d_bins, const uint32_t* d_oor, uint32_t n_chunks, uint32_t* d_step_hist, hipStream_t st);
// the same over the coded symbol of the wide container, min(z, 255): bin 255 is the number of escapes
void launch_rate_fold_wide(const uint32_t* d_bins, const uint32_t* d_oor, uint32_t n_chunks, uint32_t* d_step_hist, hipStream_t st);
// d_log: the lo and hi arrays of rate_log_table() back to back on the device; out: [chunk][step - 1][channel]
void launch_rate_cost(const uint32_t* d_step_hist, const uint32_t* d_log, uint32_t n_chunks, RateChannel* d_out, hipStream_t st);
// the same for the channel payloads of the split-stream container at `lane_symbols` (status is always kRateBounded; a
// histogram without symbols gives 0 / 0)
void launch_split_rate_cost(const uint32_t* d_step_hist, const uint32_t* d_log, uint32_t n_chunks, uint32_t lane_symbols,
                            RateChannel* d_out, hipStream_t st);
// the same for the channel payloads of the wide container (.alc v3) over the histograms of launch_rate_fold_wide
void launch_wide_rate_cost(const uint32_t* d_step_hist, const uint32_t* d_log, uint32_t n_chunks, uint32_t lane_symbols,
                           RateChannel* d_out, hipStream_t st);

// ---- split.hip: the split-stream entropy stage of .alc v2 ----
constexpr uint32_t kSplitFixedHeaderBytes = 22;      // magic, version, wavelet, width, height, frames, lane_symbols
constexpr uint32_t kSplitChannelHeaderBytes = 536;   // step, dead zone, num_symbols, n_blocks, payload_len u64, 256 x u16
constexpr uint32_t kSplitHeaderBytes = kSplitFixedHeaderBytes + 3 * kSplitChannelHeaderBytes;   // 1630
constexpr uint32_t kSplitMinLane = 64, kSplitMaxLane = 16384, kSplitDefaultLane = 512;
constexpr uint32_t kSplitBadDirectory = 1u;   // block table or lane directory does not add up to the payload
constexpr uint32_t kSplitBadLane = 2u;        // a lane failed its end check
// .alc v3: u16 symbols, coded symbol min(z, 255), escape 255 + a uniform 12-bit residual
constexpr uint32_t kSplitWideMaxLane = 8192;          // 4 L + 4 bytes per lane stream must fit the u16 directory
constexpr uint32_t kSplitWideMaxResidual = 4095u;     // z <= 255 + 4095
constexpr uint32_t kSplitWideResidual = 4u;           // count pass: a symbol whose residual does not fit 12 bits
constexpr int kWideMaxQ = 2175;                       // |q| of z = 4350, the largest symbol a (damaged) v3 stream decodes to
// One channel: n symbols in blocks of 64 * lane_symbols, payload at `stream`.
struct SplitJob {
    const uint8_t* sym;        // encode: the symbols; decode: where they go (written).  The wide kernels: n x u16
    unsigned long long n;
    const RansTable* table;
    uint8_t* stream;           // the channel's payload: u32 block lengths, then the blocks
    unsigned long long len;    // decode: length of the payload
    uint32_t n_blocks, lane_symbols;
    uint32_t* blk_len;         // scratch, n_blocks
    unsigned long long* blk_off;   // scratch, n_blocks + 1
    uint16_t* lane_len;        // scratch, 64 * n_blocks (encode)
    uint32_t* flags;           // decode: kSplitBad*, zeroed by the caller
};
// Frame ranges: the blocks [blk_first[r], blk_first[r] + blk_count[r]) of channel `j` are decoded,
// and the symbols at positions [sym_lo[r], sym_hi[r]) of the channel are stored at j.sym, range 0 first and range 1
// directly behind it (sym_hi[0] - sym_lo[0] + sym_hi[1] - sym_lo[1] symbols; an unused range is empty, count 0).
struct SplitFramesJob {
    SplitJob j;
    uint32_t blk_first[2], blk_count[2];
    unsigned long long sym_lo[2], sym_hi[2];
};
// A box of a channel's [t'][ph][pw] symbol volume (preview and rectangle, DESIGN.md sections 15 and 16): the n_planned
// blocks blocks[0 .. n_planned) of channel `j` (ascending, no duplicates) are decoded.  Axis k (0 = x, 1 = y, 2 = t') keeps the
// coordinates [lo[k], lo[k] + n_lo[k]) (low run, place c - lo[k]) and [half[k] + lo[k], half[k] + lo[k] + n_hi[k]) (high run,
// place n_lo[k] + ...); n_hi[k] is n_lo[k] when both bands are kept and 0 when only the low band is.  A symbol at channel
// position (t' * ph + y) * pw + x is stored only when all three coordinates are kept: at j.sym[vt * pitch + vy * (n_lo[0] +
// n_hi[0]) + vx], v* the places.  pitch >= the rows times the row extent; the channel's compact volume is (n_lo[2] + n_hi[2]) *
// pitch symbols.  The rectangle keeps both runs of every axis, pitch = rows * row extent (the virtual chunk); the preview keeps
// both runs of t' only, lo = 0 on x and y, and pitch = qw * qh rounded up to 4.
struct SplitBoxJob {
    SplitJob j;
    const uint32_t* blocks;
    uint32_t n_planned;
    uint32_t pw, ph;
    uint32_t lo[3], half[3], n_lo[3], n_hi[3];
    unsigned long long pitch;
};
// One band of a channel (.alc v5): `j` is a channel job whose n symbols are the band's, in band order
// (the raster of an hw x hh x (n / (hw hh)) box), and j.sym is the band's origin inside the channel's [t'][ph][pw] volume:
// band-order index idx lives at j.sym[((idx / (hw hh)) * ph + (idx / hw) % hh) * pw + idx % hw].
struct SplitBandJob {
    SplitJob j;
    uint32_t pw, ph, hw, hh;
};
// A plane range of one band (frame ranges and previews of .alc v5): `j` is the band's job as in
// SplitBandJob, but the blocks [blk_first, blk_first + blk_count) alone are decoded, and the symbol of band-order index idx =
// (t'' hh + y'') hw + x'' is stored only for idx in [idx_lo, idx_hi), at j.sym[(t'' - idx_lo / (hw hh)) * plane_pitch +
// y'' * row_pitch + x'']: j.sym is where the symbol of index idx_lo goes (idx_lo a multiple of hw hh).
struct SplitBandRangeJob {
    SplitJob j;
    uint32_t hw, hh;
    unsigned long long row_pitch, plane_pitch;   // of the destination, in symbols
    uint32_t blk_first, blk_count;
    uint32_t idx_lo, idx_hi;
};
struct SplitHeaderDesc {
    uint8_t* out;
    uint32_t width, height, frames, lane_symbols, num_symbols, n_blocks;
    int32_t step[3], dead_zone[3];
    unsigned long long payload_len[3];
    const uint16_t* freq;      // device, 3 x 256
    uint8_t wavelet;
};
// hist [n_tables][256] -> freq, cum [n_tables][256]
void launch_split_table(const uint32_t* d_hist, uint16_t* d_freq, uint16_t* d_cum, int n_tables, hipStream_t st);
// max_blocks: the largest n_blocks among the jobs.  count fills lane_len and blk_len; scan(from_stream = false) turns
// blk_len into blk_off and the payload lengths d_totals[job]; write then needs `stream` to hold that many bytes.
// wide: the same passes on u16 symbols with the escape step (.alc v3); the count pass then sets kSplitWideResidual in
// *flags (zeroed by the caller) when a symbol exceeds 255 + kSplitWideMaxResidual
void launch_split_count(const SplitJob* d_jobs, int n_jobs, uint32_t max_blocks, bool wide, hipStream_t st);
void launch_split_write(const SplitJob* d_jobs, int n_jobs, uint32_t max_blocks, bool wide, hipStream_t st);
void launch_split_scan(const SplitJob* d_jobs, int n_jobs, bool from_stream, unsigned long long* d_totals, hipStream_t st);
// after scan(from_stream = true); *flags != 0 afterwards: the payload is not a valid stream
void launch_split_decode(const SplitJob* d_jobs, int n_jobs, uint32_t max_blocks, bool wide, hipStream_t st);
void launch_split_headers(const SplitHeaderDesc* d_descs, int n_chunks, hipStream_t st);
// after scan(from_stream = true) over the same channels; max_blocks: the largest blk_count[0] + blk_count[1] among the jobs
void launch_split_frames_decode(const SplitFramesJob* d_jobs, int n_jobs, uint32_t max_blocks, bool wide, hipStream_t st);
// after scan(from_stream = true) over the same channels; max_planned: the largest n_planned among the jobs; xy_high: a job
// has a high run on x or y (false: the instance without them, which stores nothing of such runs)
void launch_split_box_decode(const SplitBoxJob* d_jobs, int n_jobs, uint32_t max_planned, bool wide, bool xy_high, hipStream_t st);
// overwrites the version byte of the headers launch_split_headers wrote (same stream, after it)
void launch_split_header_version(const SplitHeaderDesc* d_descs, int n_chunks, uint8_t version, hipStream_t st);

// ---- band.hip: the banded entropy stage of .alc v5 ----
constexpr uint32_t kBandFixedHeaderBytes = 24;       // the fixed fields of version 2, then base and a reserved byte
constexpr uint32_t kBandBandHeaderBytes = 524;       // n_blocks, payload_len u64, 256 x u16
constexpr uint32_t kBandChannelHeaderBytes = 12 + 8 * kBandBandHeaderBytes;   // step, dead zone, num_symbols, eight bands: 4204
constexpr uint32_t kBandHeaderBytes = kBandFixedHeaderBytes + 3 * kBandChannelHeaderBytes;   // 12636
struct BandHeaderDesc {
    uint8_t* out;
    uint32_t width, height, frames, lane_symbols, num_symbols, n_blocks;   // n_blocks: of every band
    int32_t step[3], dead_zone[3];
    unsigned long long payload_len[24];   // channel-major, band ascending
    const uint16_t* freq;      // device, 24 x 256
    uint8_t wavelet, base;
};
// symbols [3][pf][ph][pw] of one chunk (u8; wide: u16 at an even address) -> d_hist u32 [3][8][256], ADDED (the caller
// zeroes); wide bins min(z, 255).  One read pass; the grid obeys generic_grid_for's cap.
void launch_band_hist(const void* d_sym, const ChunkDims& d, bool wide, uint32_t* d_hist, hipStream_t st);
// the passes of launch_split_count / _write / _decode over band jobs; the scan between them is launch_split_scan over the
// same jobs' SplitJob parts
void launch_band_count(const SplitBandJob* d_jobs, int n_jobs, uint32_t max_blocks, bool wide, hipStream_t st);
void launch_band_write(const SplitBandJob* d_jobs, int n_jobs, uint32_t max_blocks, bool wide, hipStream_t st);
void launch_band_decode(const SplitBandJob* d_jobs, int n_jobs, uint32_t max_blocks, bool wide, hipStream_t st);
void launch_band_headers(const BandHeaderDesc* d_descs, int n_chunks, hipStream_t st);
// after scan(from_stream = true) over the same bands' SplitJob parts; max_blocks: the largest blk_count among the jobs
void launch_band_range_decode(const SplitBandRangeJob* d_jobs, int n_jobs, uint32_t max_blocks, bool wide, hipStream_t st);

// ---- quality.hip: exact squared error of two RGB volumes ----
constexpr uint32_t kSseBlock = 256;               // lanes of a workgroup
constexpr uint32_t kSseVectorsPerLane = 8;        // 16-byte windows a lane takes per virtual block (256 * 8 windows = 32 KiB a side)
// 16-byte windows a lane may hold in its u32 sums before it folds them into its u64: each byte adds at most 255^2 = 65 025
// to a sum, and 4128 * 16 * 65 025 = 4 294 771 200 < 2^32, while the next multiple of kSseVectorsPerLane (4136 windows) would not.  A
// multiple of kSseVectorsPerLane.
constexpr uint32_t kSseLaneFlushVectors = 4128;
constexpr uint32_t kSseMaxBlocks = 2048;          // workgroups of a launch at most (256 CUs x 8), below grid_for's cap
static_assert(kSseLaneFlushVectors % kSseVectorsPerLane == 0, "the fold is checked once per virtual block");
static_assert(16ull * 65025ull * kSseLaneFlushVectors < (1ull << 32), "a lane's u32 sums must hold kSseLaneFlushVectors windows");
static_assert(16ull * 65025ull * (kSseLaneFlushVectors + kSseVectorsPerLane) >= (1ull << 32), "the limit is the last that fits: the tests rely on it");
// one run of 3wh bytes per frame (both sides keep their rows back to back, or there is one row) instead of h runs of 3w
bool rgb_sse_flat(const RgbLayout& a, const RgbLayout& b, uint64_t w, uint64_t h);
// d_frame_sse[k] = sum over the w x h pixels of frame k of (a - b)^2, all three colours; zeroed here.  Bases of any byte
// alignment, pitches >= the bytes they span (the caller checks); reads exactly the w x h x n_frames pixels of each side.
// Returns the status of zeroing and launching; on an error nothing was launched.
hipError_t launch_rgb_sse(const RgbLayout& a, const RgbLayout& b, uint64_t w, uint64_t h, uint64_t n_frames,
                          unsigned long long* d_frame_sse, hipStream_t st);

// ---- transcode.hip: symbols of .alc v2-v4 to a coarser quantiser step ----
// n symbols (u8; wide: u16 at an even address) from d_src to d_dst -- the same address, or buffers that do not overlap --
// through the map of steps (step_from, step_to), both in 1..64; step_to <= step_from is the identity.  d_hist (256 u32, or
// null): the histogram of the coded symbols written (wide: min(z, 255)) is ADDED to it.
void launch_requant_symbols(const void* d_src, void* d_dst, uint64_t n, bool wide, int32_t step_from, int32_t step_to,
                            uint32_t* d_hist, hipStream_t st);
// the bins of the value the map quantises, layout and counter of launch_coef_hist (d_bins: 4096 u32 of one channel, zeroed
// by the caller): what launch_rate_fold / launch_rate_fold_wide turn into the histogram of every target step
void launch_symbol_bins(const void* d_sym, uint64_t n, bool wide, int32_t step_from, uint32_t* d_bins, uint32_t* d_oor, hipStream_t st);
// rows (step - 1, channel) of one chunk's step_hist [64][3][256] with step <= step_from[channel]: d_src_hist [3][256], the
// coded histogram of the channel's own symbols (a transcode leaves the channel untouched there)
void launch_kept_rows(const uint32_t* d_src_hist, const int32_t step_from[3], uint32_t* d_step_hist, hipStream_t st);

}  // namespace alice
