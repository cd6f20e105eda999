/* TEST AND MEASUREMENT HOOKS of libalice_codec.so.  Not part of the API: nothing here is needed by a caller, nothing
 * here is mirrored by the language bindings, and include/alice_codec.h does not include this file.  The test-suite and
 * the developer probes under scripts/ bind these symbols directly. */
#ifndef ALICE_CODEC_TEST_H
#define ALICE_CODEC_TEST_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The next encodes OF THE CALLING THREAD size their stream regions with this capacity instead of the histogram-derived
 * one (0 = off), so that the suite can drive the overflow-and-retry path.  Thread-local: encodes on other threads are
 * not affected, and a test that dies before resetting it leaves no process-wide state behind. */
void alice_codec_test_force_first_cap(uint64_t cap);

/* The last alice_codec_rans_decode / alice_codec_dev_rans_decode of the calling thread: tiles taken by the fast path,
 * tiles taken by the exact loop, the mask of tile-loop branches that ran (kDecPath* in csrc/kernels.h), stream bytes
 * consumed. */
void alice_codec_test_last_decode_stats(uint32_t out[4]);

/* ONE launch of n_chains decode chains on device buffers (csrc/rans.hip, launch_rans_decode), each with a table of its own
 * given as arrays: chain c decodes n symbols from d_streams[c] (lens[c] bytes, any byte alignment) with
 * cum_freq[256 c ..] / freq[256 c ..] into d_symbols[c].  out[4 c ..] = stream bytes consumed (RansResult.len, saturated
 * to 32 bits), final state, mask of tile-loop branches (kDecPath*), tiles taken by the fast path. */
int alice_codec_test_decode_chains(uint32_t n_chains, const void *const *d_streams, const uint64_t *lens,
                                   const uint16_t *cum_freq, const uint16_t *freq, void *const *d_symbols, uint64_t n,
                                   uint32_t *out, void *hip_stream);

/* The same launch with a symbol count per chain: chain c decodes ns[c] symbols. */
int alice_codec_test_decode_chains_n(uint32_t n_chains, const void *const *d_streams, const uint64_t *lens,
                                     const uint16_t *cum_freq, const uint16_t *freq, void *const *d_symbols,
                                     const uint64_t *ns, uint32_t *out, void *hip_stream);

/* ONE launch_rans_decode of n_chains descriptors spelled out per chain, the way the chain hub and the stateful decoder
 * objects fill them (up to 1024 chains run the one-chain-per-SIMD instance of the kernel, more run the plain one).  Chain c
 * decodes ns[c] symbols (0 is allowed: nothing is written, the chain still reports) from d_streams[c] (lens[c] bytes) into
 * d_symbols[c], both at any byte alignment.
 * Tables: hists gives 256 counts per chain and the table the kernel builds from a histogram (the production path, with its
 * kTableDec* flags); cum_freq[256 c ..] / freq[256 c ..] are taken as they are, all of them built in one launch.  One of the
 * two may be NULL.  With both given, from_arrays[c] != 0 picks chain c's arrays and 0 its histogram (every row of both is
 * built, so every row must be a table); from_arrays == NULL picks the histograms when they are given.
 * resume / x0 / pos0 (NULL: a fresh decoder for every chain): resume[c] != 0 starts chain c from state x0[c] at stream
 * position pos0[c] (at most lens[c]) instead of from the four head bytes.
 * own_result (NULL: 0 for every chain): own_result[c] != 0 gives chain c a RansResult of its own through its descriptor, 0
 * leaves it results[c] of the launch; a chain that writes the one it was not given is an error.
 * hipGetLastError() is checked behind the launch.  out[6 c ..] = stream bytes consumed (RansResult.len, saturated to 32
 * bits), final state, mask of tile-loop branches (kDecPath*), tiles taken by the fast path, tiles taken by the exact loop,
 * RansResult.flags. */
int alice_codec_test_decode_chains_ex(uint32_t n_chains, const void *const *d_streams, const uint64_t *lens,
                                      void *const *d_symbols, const uint64_t *ns, const uint32_t *hists,
                                      const uint16_t *cum_freq, const uint16_t *freq, const uint32_t *from_arrays,
                                      const uint32_t *resume, const uint32_t *x0, const uint64_t *pos0,
                                      const uint32_t *own_result, uint32_t *out, void *hip_stream);

/* ONE launch of n_chains encode chains on device buffers (csrc/rans.hip, launch_rans_encode_descs: up to 1024 chains run
 * the one-chain-per-SIMD instance of the kernel, more run the plain one).  Chain c encodes the ns[c] symbols at d_symbols[c]
 * (any byte alignment) back to front into [d_regions[c], d_regions[c] + caps[c]); its stream is the LAST len bytes of that
 * region.  Tables: hists != NULL gives 256 counts per chain and the table the kernel builds from a histogram, flagged as
 * verified against the data (so the counts must be the data's own, or at least cover it); hists == NULL takes
 * cum_freq[256 c ..] / freq[256 c ..] as they are.  x_init / keep_open (NULL: 2^23 / 0 for every chain): the state a
 * RansEncoder object brings along, and whether it stays open (the four state bytes of finish() are not written and do not
 * count in len).  No retry and no error mapping: out[6 c ..] = len (saturated to 32 bits), final state, RansResult.flags
 * (kRansOverflow, kTableDiverges, ...), mask of branches that ran (kEncPath* in csrc/kernels.h), tiles taken by the
 * one-compare clean path, tiles taken block by block. */
int alice_codec_test_encode_chains(uint32_t n_chains, const void *const *d_symbols, const uint64_t *ns, const uint32_t *hists,
                                   const uint16_t *cum_freq, const uint16_t *freq, void *const *d_regions, const uint64_t *caps,
                                   const uint32_t *x_init, const uint32_t *keep_open, uint32_t *out, void *hip_stream);

/* The same launch with one more result per chain: out[7 c ..] = the six values above, then the number of 64-symbol blocks of
 * clean tiles that took the complement step (csrc/rans.hip, ripple64_comp_run: blocks in which every symbol has a table
 * frequency of at least 17). */
int alice_codec_test_encode_chains_blocks(uint32_t n_chains, const void *const *d_symbols, const uint64_t *ns,
                                          const uint32_t *hists, const uint16_t *cum_freq, const uint16_t *freq,
                                          void *const *d_regions, const uint64_t *caps, const uint32_t *x_init,
                                          const uint32_t *keep_open, uint32_t *out, void *hip_stream);

/* Times the transform launches alone (no chains) with HIP events on `hip_stream`: `reps` passes over `n_chunks` chunks
 * of w x h x f pixels, forward (RGB -> symbols + histograms) and inverse (symbols -> RGB), through the same pipes the
 * encode / decode of a batch use.  Device buffers: d_rgb and d_rgb_out hold n_buffers chunks of RGB, d_sym n_buffers
 * chunks of 3 * padded symbols; chunk c uses buffer c mod n_buffers.  out_ms[0] / out_ms[1] = milliseconds per chunk
 * forward / inverse.  probe: 0 = the real kernels; 1 = the VALU-floor probe (same instruction streams, same registers
 * and LDS, global loads and stores replaced by register moves; the outputs are NOT produced); 2 = only the loads
 * replaced; 3 = only the stores replaced (CDF 9/7 with a step > 1 and the i16 lane-exchange inverse only). */
int alice_codec_test_transform_ms(const void *d_rgb, void *d_sym, void *d_rgb_out, uint32_t n_buffers, uint32_t width,
                                  uint32_t height, uint32_t frames, uint8_t wavelet_type, uint8_t quality, uint32_t n_chunks,
                                  uint32_t reps, int probe, float out_ms[2], void *hip_stream);

/* Band plan of the transform launches (csrc/transform.hip, "Bands"), process-wide: target size of a band slot in KiB
 * (0 = never cut a chunk into bands; negative = keep; default 1048576).  The suite uses it to run small shapes through
 * many bands; results never depend on it. */
void alice_codec_test_set_tuning(long band_kb);

/* Radius r of the value -> symbol table of the forward temporal kernel (csrc/transform.hip, kQLutR), process-wide, clamped
 * to 1 .. 2048 (the default): coefficients in [-r, r) are quantised through the table, a wavefront holding any other value
 * through the arithmetic.  8-bit RGB never leaves the default table, so the suite shrinks it to run the arithmetic path
 * and the boundary; results never depend on it. */
void alice_codec_test_set_value_table_radius(int r);

/* Cap on the workgroups of the generic stage kernels' launches (csrc/generic.hip, grid_for), process-wide: the stage calls
 * (wavelets, quantisers, symbol maps, colour, pad / strip, ssim / ms_ssim) and the chunks the tile kernels do not cover
 * launch one workgroup per 256 items up to 262 140 workgroups and cover the rest in further trips of a grid-stride loop.
 * 0 restores 262 140; larger values are clamped to it.  The launches that clamp further to 2048 workgroups (histograms,
 * psnr, the RDO sum) keep doing so on top of it.  Read at launch time on the host; no kernel knows about it.  The suite
 * lowers it so that a few hundred items already take several trips; results never depend on it. */
void alice_codec_test_set_grid_cap(uint32_t max_blocks);

/* The wide twins of the symbol kernels (csrc/generic.hip), which no stage call reaches on data of the caller's choice: n host
 * coefficients through to_symbols_wide, its result through from_symbols_wide and histogram_wide.  out receives
 * 1024 + 6 n bytes: the 256 u32 bins of min(z, 255), then n i32 (the coefficients from_symbols_wide gives back), then n
 * u16 (z; 65535 for a coefficient above 32768 or below -32767). */
int alice_codec_test_wide_symbols(const int32_t *coeffs, uint64_t n, uint8_t *out);

/* Admission budget of the calling thread's device (csrc/codec.hip, ChainHub::admit): whole-chunk host calls state the
 * device memory they are about to allocate and wait while the calls already in flight hold more than the budget allows
 * (a call alone always enters).  Default: 90 % of what is free (device + the library's cache) whenever a call enters an
 * idle hub; 0 restores that.  The suite
 * shrinks it so that a handful of small calls already queue; results never depend on it. */
int alice_codec_test_set_admission_budget(uint64_t bytes);

/* Resident chain kernels: what the runtime reports for the one-chain-per-SIMD instances of the rANS kernels.
 * out[0..2] = encoder: registers per lane (VGPR + AGPR, as allocated), static LDS bytes, workgroups per CU the runtime
 * would co-schedule; out[3..5] = the same for the decoder.  The exclusive instances must report at most 4 workgroups
 * per CU (one wave per SIMD). */
int alice_codec_test_chain_occupancy(uint32_t out[6]);

/* The fixed-point table of the rate prediction (csrc/rate.hip): lo[f] / hi[f] = floor / ceil of log2(4096 / f) * 2^24 for
 * f = 1 .. 4096 (entry 0 unused), g[0] = ceil(log2(1 + 2^-11) * 2^24), g[1] = ceil(-log2(1 - 2^-11) * 2^24).  Any pointer may
 * be NULL.  No device needed. */
void alice_codec_test_rate_log_table(uint32_t lo[4097], uint32_t hi[4097], uint32_t g[2]);

/* The instance of the inverse transform a decode picks for these quantiser steps (csrc/codec.hip, inverse_bounds, through
 * the mapping the launcher itself uses, csrc/kernels.h inverse_variant): 0 = exact (wrapping i32 sums, 64-bit products),
 * 1 = fast i32 (24-bit multiply-adds, i32 band slot), 2 = fast with an i16 band slot and the lane-exchange tile, 3 = fast
 * with an i16 band slot and the packed i16 LDS tile; -1 for an unknown wavelet.  wide != 0: the symbols are those of
 * version 3 (|q| <= 2175), else the u8 symbols of versions 1 and 2 (|q| <= 128).  Shapes the tile kernels do not cover
 * run exact reference arithmetic whatever this says.  No device needed. */
int alice_codec_test_inverse_variant(uint8_t wavelet_type, const int32_t step[3], int wide);

/* The last version 2 or version 3 budget call of the calling thread (alice_codec_encode_split_to_size,
 * alice_codec_dev_encode_split_to_budget, alice_codec_encode_wide_to_size, alice_codec_dev_encode_wide_to_budget),
 * whichever came last: returns its number of chunks and writes the refinement trials (exact sizes
 * computed, at most ALICE_SPLIT_REFINE_TRIALS each) of the first min(that, cap) chunks to per_chunk (may be NULL). */
uint32_t alice_codec_test_last_split_trials(uint32_t *per_chunk, uint32_t cap);

/* The last alice_codec_dev_encode_to_psnr / alice_codec_encode_to_psnr of the calling thread: returns its number of chunks and
 * writes the trials (transform pairs measured, at most ALICE_QUALITY_MAX_TRIALS each) of the first min(that, cap) chunks to
 * per_chunk (may be NULL). */
uint32_t alice_codec_test_last_quality_trials(uint32_t *per_chunk, uint32_t cap);

/* Bytes of the band slot the inverse transform of a width x height x frames chunk needs under the current band target
 * (alice_codec_test_set_tuning) when its intermediate is i16 (mid16 != 0: the steps alice_codec_test_inverse_variant maps to 2
 * or 3) or i32; 0 for a shape the tile kernels do not cover.  The two plans cut a chunk differently, and either slot can be
 * the larger.  No device needed. */
uint64_t alice_codec_test_inverse_scratch_bytes(uint32_t width, uint32_t height, uint32_t frames, int mid16);

/* Bytes of the band slot one decode group allocates for chunks of this shape under the current band target (csrc/codec.hip,
 * group_scratch_bytes): every chunk of the group plans its bands by its own sample width into the one slot, so a group that
 * holds both widths (any16 != 0 and any32 != 0) gets the larger of the two plans' slots, a group of one width exactly
 * alice_codec_test_inverse_scratch_bytes of that width (neither flag: the i16 slot, as for an empty group); 0 for a shape the
 * tile kernels do not cover.  No device needed. */
uint64_t alice_codec_test_group_scratch_bytes(uint32_t width, uint32_t height, uint32_t frames, int any16, int any32);

/* Cap on the chunks a call works on at a time, process-wide: the groups of the device-resident calls of versions 2-4
 * (csrc/codec.hip, split_group: 4 GiB of symbols) and the passes of the version 1 host calls (chunks_that_fit) hold at most
 * max_chunks chunks; never fewer than 1, never more than they compute themselves.  0 restores the default.  Read at call time
 * on the host; no kernel knows about it.  The suite lowers it so that a call of seven small chunks already takes several
 * groups with a ragged last one; results never depend on it. */
void alice_codec_test_set_group_chunks(uint32_t max_chunks);

/* The group size a device-resident call of this shape in this format (2, 3 or 4) would use under the current cap; 0 for
 * another format or a shape no call accepts.  No device needed. */
uint32_t alice_codec_test_group_chunks(uint32_t width, uint32_t height, uint32_t frames, int format);

/* The byte-at-a-time squared-error kernel behind alice_codec_psnr (csrc/generic.hip, sq_diff_sum_kernel) on two device
 * buffers of n bytes: *sse (host) = the sum.  For the probes that time it beside alice_codec_dev_rgb_sse. */
int alice_codec_test_sq_diff_sum(const void *d_a, const void *d_b, uint64_t n, uint64_t *sse, void *hip_stream);

/* The last alice_codec_decode_frames / alice_codec_dev_decode_frames of the calling thread that reached the device:
 * out = {a, b of the window, blocks decoded over the three channels, payload bytes the host call uploaded (the planned
 * blocks; 0 for the device call), frames given to the spatial pass}. */
void alice_codec_test_last_frames_stats(uint64_t out[5]);

/* The last alice_codec_decode_preview / alice_codec_dev_decode_preview of the calling thread that reached the device:
 * out = {a, b of the window, blocks decoded over the three channels, payload bytes the host call uploaded (the planned
 * blocks; 0 for the device call), frames written, symbols stored over the three channels (3 (b - a) qw qh)}. */
void alice_codec_test_last_preview_stats(uint64_t out[6]);

/* The last alice_codec_decode_previews / alice_codec_dev_decode_previews of the calling thread that ran to its end (a
 * refused call leaves it alone; the single-item calls above never touch it): out = {items, distinct containers, table
 * launches, lane launches, finish launches, stream drains, blocks decoded over all items and channels, payload bytes the
 * host call uploaded (the union of the planned blocks per distinct container; 0 for the device call), symbols stored over
 * all items and channels}. */
void alice_codec_test_last_previews_stats(uint64_t out[9]);

/* The last alice_codec_decode_rect / alice_codec_dev_decode_rect of the calling thread that reached the device:
 * out = {ta, tb, xa, xb, ya, yb of the three windows, blocks decoded over the three channels, payload bytes the host call
 * uploaded (the planned blocks; 0 for the device call), frames written, symbols stored over the three channels
 * (3 (tb - ta) (yb - ya) (xb - xa))}. */
void alice_codec_test_last_rect_stats(uint64_t out[10]);

/* The last alice_codec_decode_rects / alice_codec_dev_decode_rects of the calling thread that ran to its end (a refused call
 * leaves it alone; the single calls and the previews never touch it, nor it their hooks): out = {items, distinct
 * containers, table launches, lane launches, batched finish launches (temporal, tile and paste work lists), items finished
 * through the per-item path, stream drains, blocks decoded over all items and channels, payload bytes the host call
 * uploaded (the union of the planned blocks per distinct container; 0 for the device call), symbols stored over all items
 * and channels, frames written over all items}. */
void alice_codec_test_last_rects_stats(uint64_t out[11]);

/* The disjointness rule of alice_codec_dev_decode_rects alone, on items with explicit w, h and count (alc, len, first, x, y
 * are not looked at; rgb_out is only compared); no device needed.  0: no two outputs conflict.  ALICE_ERR_INVALID_DIMENSIONS
 * with *bad_item the later item of the first conflicting pair; an item without w, h or count, or with bad pitches, is
 * refused with its index too. */
int alice_codec_test_rects_outputs_disjoint(const alice_codec_rect_item *items, uint32_t n_items, uint32_t *bad_item);

/* The bins kernel of the transcode's size prediction (csrc/transcode.hip, symbol_bins_kernel), which no public call reaches
 * on data of the caller's choice: n device symbols (u8; wide != 0: u16 at an even address) of a channel whose step is
 * step_from (1..64) -> the value m the map quantises is counted into d_bins[m + r] (4096 u32 on the device,
 * ADDED to) for m in [-r, r), r the value table's radius, and every other symbol into *d_oor (one u32, added to).
 * Finished on return.  The budget transcodes report their trials through alice_codec_test_last_split_trials. */
int alice_codec_test_symbol_bins(const void *d_symbols, uint64_t n, int wide, int32_t step_from, void *d_bins, void *d_oor,
                                 void *hip_stream);

/* The last alice_codec_decode_banded_frames / alice_codec_dev_decode_banded_frames (and the same for the preview) of the
 * calling thread that ran to its end: out = {a, b of the window, blocks decoded summed over the three channels and the kept
 * bands (8 for frames, 2 for a preview), payload bytes the host call uploaded (the planned blocks of the kept bands; 0 for
 * the device call), frames written, symbols stored over the three channels (3 (b - a) pw ph, preview: 3 (b - a) hw hh)}. */
void alice_codec_test_last_banded_frames_stats(uint64_t out[6]);
void alice_codec_test_last_banded_preview_stats(uint64_t out[6]);

#ifdef __cplusplus
}
#endif
#endif
