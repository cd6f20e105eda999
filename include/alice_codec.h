/*
 * alice_codec.h -- C ABI of libalice_codec.so, the MI355X (gfx950) encode/decode path.
 *
 * PART 1 is the drop-in boundary: the 20 functions the reference `cdylib` exports from
 * src/ffi.rs (C statement of the ABI: bindings/ue5/AliceCodec.h:14-68 in the reference),
 * with the same names, signatures, ownership and failure conventions (NULL / -1.0 / 0,
 * `*out_len` written only on success).  Every call runs on the GPU; there is no CPU
 * fallback -- without a usable HIP device the calls fail (NULL) and
 * alice_codec_last_error() reports ALICE_ERR_DEVICE.
 *
 * PART 2 are extension entry points the reference ABI cannot express: wavelet selection
 * (the reference FFI can only create CDF 5/3 encoders, src/ffi.rs:92-94), 64-bit lengths
 * (src/ffi.rs:119 carries u32), device-resident batches of chunks (many rANS chains in
 * flight is the only parallelism the single-stream format offers), and stage-level calls
 * for the Rust API surface named by the task (Wavelet2D/3D, Quantizer/FastQuantizer,
 * to_symbols/from_symbols/build_histogram, FrequencyTable, RansEncoder/RansDecoder, colour).
 *
 * Handles are opaque and immutable after creation; encode/decode may be called from many
 * threads on the same handle (reference: Send + Sync, src/pipeline.rs:635-644).  Concurrent
 * encode / decode calls scale: the serial entropy chains of all calls in flight leave in merged
 * kernel launches (chain hub), so a thread pool over chunks keeps as many
 * chunks' chains running as the device holds, not one per hardware queue.
 */
#ifndef ALICE_CODEC_H
#define ALICE_CODEC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct Wavelet1D Wavelet1D;
typedef struct FrameEncoder FrameEncoder;
typedef struct EncodedChunk EncodedChunk;

/* ===================== PART 1: reference ABI (src/ffi.rs) ===================== */

Wavelet1D *alice_codec_wavelet1d_haar(void);                 /* src/ffi.rs:16  */
Wavelet1D *alice_codec_wavelet1d_cdf53(void);                /* src/ffi.rs:22  */
Wavelet1D *alice_codec_wavelet1d_cdf97(void);                /* src/ffi.rs:28  */
void alice_codec_wavelet1d_destroy(Wavelet1D *ptr);          /* src/ffi.rs:38  null-ok */
/* no-op if wavelet/data is NULL or len < 2 */
void alice_codec_wavelet1d_forward(const Wavelet1D *wavelet, int32_t *data, uint32_t len); /* src/ffi.rs:52 */
void alice_codec_wavelet1d_inverse(const Wavelet1D *wavelet, int32_t *data, uint32_t len); /* src/ffi.rs:73 */

FrameEncoder *alice_codec_encoder_create(uint8_t quality);   /* src/ffi.rs:92  always CDF 5/3 */
void alice_codec_encoder_destroy(FrameEncoder *ptr);         /* src/ffi.rs:102 null-ok */
/* NULL on any error or NULL argument */
EncodedChunk *alice_codec_encode(const FrameEncoder *encoder, const uint8_t *rgb, uint32_t rgb_len,
                                 uint32_t width, uint32_t height, uint32_t frames); /* src/ffi.rs:116 */
/* NULL on error; caller frees with alice_codec_data_free(ptr, *out_len) */
uint8_t *alice_codec_decode(const EncodedChunk *chunk, uint32_t *out_len);          /* src/ffi.rs:145 */

void alice_codec_chunk_destroy(EncodedChunk *ptr);                                  /* src/ffi.rs:171 */
uint8_t *alice_codec_chunk_to_bytes(const EncodedChunk *chunk, uint32_t *out_len);  /* src/ffi.rs:185 */
EncodedChunk *alice_codec_chunk_from_bytes(const uint8_t *data, uint32_t len);      /* src/ffi.rs:207 */
uint32_t alice_codec_chunk_width(const EncodedChunk *chunk);                        /* src/ffi.rs:226 */
uint32_t alice_codec_chunk_height(const EncodedChunk *chunk);                       /* src/ffi.rs:240 */
uint32_t alice_codec_chunk_frames(const EncodedChunk *chunk);                       /* src/ffi.rs:254 */

/* -1.0 on NULL; +inf when identical or empty */
double alice_codec_psnr(const uint8_t *a, const uint8_t *b, uint32_t len);          /* src/ffi.rs:270 */

void alice_codec_data_free(uint8_t *ptr, uint32_t len);                             /* src/ffi.rs:288 */
void alice_codec_string_free(char *s);                                              /* src/ffi.rs:302 */
char *alice_codec_version(void);                                                    /* src/ffi.rs:311 */

/* ===================== PART 2: extensions ===================== */

/* CodecError (src/error.rs:12-23) as integers, plus library-side conditions */
enum {
    ALICE_OK = 0,
    ALICE_ERR_INVALID_BUFFER_SIZE = 1,
    ALICE_ERR_INVALID_DIMENSIONS = 2,
    ALICE_ERR_DIMENSION_OVERFLOW = 3,
    ALICE_ERR_INVALID_BITSTREAM = 4,
    ALICE_ERR_INVALID_QUANT_STEP = 5,
    ALICE_ERR_REFERENCE_DIVERGES = 6, /* the reference would hang/divide by zero (src/rans.rs:275-283) */
    ALICE_ERR_OUT_OF_MEMORY = 7,
    ALICE_ERR_DEVICE = 8,
    ALICE_ERR_NULL_ARGUMENT = 9,
    ALICE_ERR_INTERNAL = 10
};
/* WaveletType (src/pipeline.rs:34-41) */
enum { ALICE_WAVELET_CDF53 = 0, ALICE_WAVELET_CDF97 = 1, ALICE_WAVELET_HAAR = 2 };

int alice_codec_last_error(void);                 /* code of the last failing call on this thread */
const char *alice_codec_last_error_message(void); /* thread-local, valid until the next call */
int alice_codec_device_count(void);
int alice_codec_set_device(int device);           /* device used by this thread's later calls */
void alice_codec_trim(void);                      /* release cached device memory */
/* (test and measurement hooks live in alice_codec_test.h, which this header does not include) */

/* FrameEncoder::with_wavelet (src/pipeline.rs:356) */
FrameEncoder *alice_codec_encoder_create_ex(uint8_t quality, uint8_t wavelet_type);
uint8_t alice_codec_encoder_quality(const FrameEncoder *encoder);
uint8_t alice_codec_encoder_wavelet(const FrameEncoder *encoder);
/* EncodedChunk public fields / compressed_size (src/pipeline.rs:172-192) */
uint8_t alice_codec_chunk_wavelet(const EncodedChunk *chunk);
uint64_t alice_codec_chunk_compressed_size(const EncodedChunk *chunk);

/* 64-bit length variants of #9, #10, #12, #13, #18 */
EncodedChunk *alice_codec_encode64(const FrameEncoder *encoder, const uint8_t *rgb, uint64_t rgb_len,
                                   uint32_t width, uint32_t height, uint32_t frames);
uint8_t *alice_codec_decode64(const EncodedChunk *chunk, uint64_t *out_len);
uint8_t *alice_codec_chunk_to_bytes64(const EncodedChunk *chunk, uint64_t *out_len);
EncodedChunk *alice_codec_chunk_from_bytes64(const uint8_t *data, uint64_t len);
void alice_codec_data_free64(uint8_t *ptr, uint64_t len);

/* ---- rate control: the size of a chunk at every quality before it is encoded, and encodes to a byte budget ----
 * From one forward transform per chunk the library derives, for every quality q = 0..100, the exact symbol histograms the
 * encoder would write and from them a guaranteed bracket lo[q] <= length of the .alc (to_bytes) <= hi[q], before any rANS
 * chain runs (derivation: csrc/rate.hip).  status[q]: ALICE_RATE_BOUNDED when every channel's table is one the bracket
 * covers (every present symbol has a frequency in 1..4096).  NOTE, a deliberate choice: a table whose cum + freq runs
 * past 4096 -- the reference's freq-1 floor for empty bins makes that most tables of real chunks -- is BOUNDED here, the
 * excess carried into the bracket; classing it UNBOUNDED would leave almost no quality of real content predictable.
 * ALICE_RATE_UNBOUNDED when a present symbol's frequency is above 4096 (lo = 0, hi = UINT64_MAX); ALICE_RATE_DIVERGES when a present symbol's frequency wrapped to 0 (an encode at that quality
 * fails with ALICE_ERR_REFERENCE_DIVERGES; lo = 0, hi = UINT64_MAX).  A chunk without pixels is its 3138-byte header at
 * every quality.  Validation is that of alice_codec_encode64 (dimensions, then the buffer size); wavelet_type > 2 is
 * ALICE_ERR_INVALID_BITSTREAM.  Budget calls: qualities above 100 act as 100, and min_q > max_q (after that) is
 * ALICE_ERR_INVALID_DIMENSIONS.  The chosen quality is the largest q in [min_q, max_q] with status BOUNDED and
 * hi[q] <= budget (every q is looked at; size need not fall with quality); when none fits, min_q with *fits = 0. */
enum { ALICE_RATE_BOUNDED = 0, ALICE_RATE_UNBOUNDED = 1, ALICE_RATE_DIVERGES = 2 };
/* one host chunk: lo / hi / status at the 101 qualities */
int alice_codec_predict_sizes(uint8_t wavelet_type, const uint8_t *rgb, uint64_t rgb_len, uint32_t width,
                              uint32_t height, uint32_t frames, uint64_t lo[101], uint64_t hi[101], uint8_t status[101]);
/* FrameEncoder::with_wavelet(q, wavelet_type).encode(...) at the chosen q for the budget max_bytes (whole .alc bytes);
 * *chosen_q and *fits out.  NULL on error (alice_codec_last_error). */
EncodedChunk *alice_codec_encode_to_size(uint8_t wavelet_type, const uint8_t *rgb, uint64_t rgb_len, uint32_t width,
                                         uint32_t height, uint32_t frames, uint64_t max_bytes, uint8_t min_q,
                                         uint8_t max_q, uint8_t *chosen_q, uint8_t *fits);
/* n_chunks equal-shaped packed chunks on the device, back to back: lo / hi / status of n_chunks * 101 entries, index
 * chunk * 101 + quality.  Like every device call, a chunk without pixels is ALICE_ERR_INVALID_DIMENSIONS here (the host
 * calls above answer it with its header size).  d_step_hist: device, n_chunks * 64 * 3 * 256 u32 (index [chunk][step - 1][channel][symbol]:
 * the channel histograms the .alc header would hold at that quantiser step), or NULL.  Launches on hip_stream; finished
 * on return. */
int alice_codec_dev_predict_sizes(const void *d_rgb, uint32_t width, uint32_t height, uint32_t frames, uint32_t n_chunks,
                                  uint8_t wavelet_type, uint64_t *lo, uint64_t *hi, uint8_t *status, void *d_step_hist,
                                  void *hip_stream);
/* (the same for a device batch: alice_codec_batch_predict_sizes / _set_qualities / _encode_to_budget, below) */

/* ---- many equal-shaped chunks from host memory in one call (what a 64-frame chunk driver wants: the serial
 * entropy chains of all chunks run side by side).  rgb = n_chunks chunks back to back; out_chunks[n_chunks] receives
 * handles to free with alice_codec_chunk_destroy.  Same results as n_chunks calls of alice_codec_encode64. ---- */
int alice_codec_encode_many(const FrameEncoder *encoder, const uint8_t *rgb, uint64_t rgb_len, uint32_t width,
                            uint32_t height, uint32_t frames, uint32_t n_chunks, EncodedChunk **out_chunks);
int alice_codec_decode_many(const EncodedChunk *const *chunks, uint32_t n_chunks, uint8_t *rgb_out, uint64_t rgb_out_len);
/* (Both take as many chunks at a time as the device's memory holds and loop over the rest.)
 *
 * The same over several GPUs of the node, for hosts that are not Python (the chunk driver of src/pipeline.rs:461-497:
 * 64-frame chunks are independent bitstreams).  Chunk k runs on devices[k mod n_devices]; the library starts one host
 * thread per entry of the list, every device copies its own chunks in and its own results out (its
 * own PCIe link; nothing is staged on another GPU), and results arrive in chunk order.  A device may be listed more than
 * once (two host threads sharing it).  Byte-identical to alice_codec_encode_many / decode_many for every device list.
 * alice_codec_many_devices_plan fills device_of_chunk[n_chunks] with that assignment (no device is touched). */
int alice_codec_many_devices_plan(uint32_t n_chunks, const int *devices, uint32_t n_devices, int *device_of_chunk);
int alice_codec_encode_many_devices(const FrameEncoder *encoder, const uint8_t *rgb, uint64_t rgb_len, uint32_t width,
                                    uint32_t height, uint32_t frames, uint32_t n_chunks, const int *devices,
                                    uint32_t n_devices, EncodedChunk **out_chunks);
int alice_codec_decode_many_devices(const EncodedChunk *const *chunks, uint32_t n_chunks, const int *devices,
                                    uint32_t n_devices, uint8_t *rgb_out, uint64_t rgb_out_len);

/* ---- device-resident batches: n_chunks equal-shaped chunks, inputs and outputs in HBM ---- */
typedef struct AliceBatch AliceBatch;
AliceBatch *alice_codec_batch_create(uint32_t width, uint32_t height, uint32_t frames, uint32_t n_chunks,
                                     uint8_t quality, uint8_t wavelet_type);
void alice_codec_batch_destroy(AliceBatch *batch);
/* Rate control of a batch (the rules of the rate-control calls above).  predict_sizes: lo / hi / status of
 * n_chunks * 101 entries for the chunks at d_rgb (as for alice_codec_batch_encode); finished on return. */
int alice_codec_batch_predict_sizes(AliceBatch *batch, const void *d_rgb, uint64_t *lo, uint64_t *hi, uint8_t *status,
                                    void *hip_stream);
/* qualities: n_chunks entries, copied; the batch's next encodes (alice_codec_batch_encode, _encode_regions) encode chunk i
 * at qualities[i], each header carrying its own step.  NULL: every chunk at the batch's quality again. */
int alice_codec_batch_set_qualities(AliceBatch *batch, const uint8_t *qualities);
/* budgets: n_chunks whole-.alc byte budgets.  Predicts, chooses each chunk's quality (chosen[n_chunks], fits[n_chunks]
 * out), sets those qualities and queues the encode: finish with alice_codec_batch_encode_finish. */
int alice_codec_batch_encode_to_budget(AliceBatch *batch, const void *d_rgb, const uint64_t *budgets, uint8_t min_q,
                                       uint8_t max_q, uint8_t *chosen, uint8_t *fits, void *hip_stream);
/* d_rgb: device pointer to n_chunks * width*height*frames*3 bytes.  hip_stream: hipStream_t (NULL = default).
 * Runs the transforms, waits for them once to size the stream regions from the histograms, then queues the
 * entropy coding and the .alc assembly asynchronously; the .alc buffers stay on the device.
 * d_rgb must stay valid until alice_codec_batch_encode_finish. Returns an ALICE_* code. */
int alice_codec_batch_encode(AliceBatch *batch, const void *d_rgb, void *hip_stream);
/* waits for the encode, checks per-chain flags, writes the .alc size of each chunk */
int alice_codec_batch_encode_finish(AliceBatch *batch, uint64_t *sizes /* n_chunks */);
const void *alice_codec_batch_alc_ptr(const AliceBatch *batch, uint32_t chunk); /* device pointer */
uint64_t alice_codec_batch_alc_stride(const AliceBatch *batch); /* valid after alice_codec_batch_encode */
/* copies the n_chunks finished .alc buffers back to back into d_dst (device), in chunk order:
 * the contiguous byte blob a rank contributes to the multi-GPU gather. Asynchronous. */
int alice_codec_batch_pack_alc(AliceBatch *batch, const uint64_t *sizes, void *d_dst, uint64_t dst_capacity,
                               void *hip_stream);
/* d_alc: device pointer, chunk i at d_alc + i*alc_stride (whole .alc, header first).
 * d_rgb_out: device pointer to n_chunks * width*height*frames*3 bytes, or NULL: the pixels of chunk i are then
 * written into the batch's own storage (over the chunk's symbols, which the decode has consumed by then) and
 * are read at alice_codec_batch_rgb_ptr(batch, i) until the next encode/decode on the batch -- saves one
 * RGB-sized buffer per chunk in flight.  Synchronises once to read headers. */
int alice_codec_batch_decode(AliceBatch *batch, const void *d_alc, uint64_t alc_stride, void *d_rgb_out,
                             void *hip_stream);
/* Region encode / decode (the hybrid flow of src/segment.rs: only the person's box is coded).
 * Chunk i of the batch is frames [i*frames, (i+1)*frames) of d_frames (frame_width x frame_height interleaved RGB,
 * tightly packed), cropped to the batch's width x height at origin (origins[2i], origins[2i+1]) in pixels.  The .alc of
 * chunk i is byte-identical to alice_codec_encode64 of crop_to_bbox of those frames (src/segment.rs:269-281).
 * origins: host array of 2*n_chunks u32, copied before return.  A region not inside the frame is
 * ALICE_ERR_INVALID_DIMENSIONS and nothing is queued (the reference's crop skips such rows instead).
 * The transforms read the rectangles in place; d_frames must stay valid until alice_codec_batch_encode_finish. */
int alice_codec_batch_encode_regions(AliceBatch *batch, const void *d_frames, uint32_t frame_width,
                                     uint32_t frame_height, const uint32_t *origins, void *hip_stream);
/* Decodes chunk i and writes its pixels into that rectangle of d_frames_out (paste_from_bbox, :284-297).
 * Bytes outside the rectangles are not written.  alice_codec_batch_rgb_ptr then gives each rectangle's first pixel. */
int alice_codec_batch_decode_regions(AliceBatch *batch, const void *d_alc, uint64_t alc_stride, void *d_frames_out,
                                     uint32_t frame_width, uint32_t frame_height, const uint32_t *origins,
                                     void *hip_stream);
const void *alice_codec_batch_rgb_ptr(const AliceBatch *batch, uint32_t chunk); /* device pointer, see above */
int alice_codec_batch_decode_finish(AliceBatch *batch);
/* per-stage device times of the last encode+finish / decode+finish, measured with HIP events on the
 * batch's stream: [0] forward transform, [1] table, [2] rANS encode, [3] assemble,
 * [4] rANS decode, [5] inverse transform.  Milliseconds. */
int alice_codec_batch_stage_ms(const AliceBatch *batch, float out[6]);
/* device pointer to the batch's u8 symbols (3 * padded per chunk, channel-major) -- for parity tests */
const void *alice_codec_batch_symbols_ptr(const AliceBatch *batch);
/* Device memory the batch holds per chunk (symbols = decoded pixels, the .alc buffer at its current capacities, tables)
 * and independent of the chunk count (transform scratch): a trial batch of one chunk tells how many chunks the free HBM
 * holds. */
uint64_t alice_codec_batch_bytes_per_chunk(const AliceBatch *batch);
uint64_t alice_codec_batch_fixed_bytes(const AliceBatch *batch);
uint64_t alice_codec_batch_padded_pixels(const AliceBatch *batch);

/* ---- stage level (host pointers; data is staged through the GPU) ---- */
/* Wavelet2D / Wavelet3D forward/inverse (src/wavelet.rs:292-340, 392-484), in place */
int alice_codec_wavelet2d_forward(uint8_t wavelet_type, int32_t *image, uint64_t width, uint64_t height);
int alice_codec_wavelet2d_inverse(uint8_t wavelet_type, int32_t *image, uint64_t width, uint64_t height);
int alice_codec_wavelet3d_forward(uint8_t wavelet_type, int32_t *volume, uint64_t width, uint64_t height, uint64_t depth);
int alice_codec_wavelet3d_inverse(uint8_t wavelet_type, int32_t *volume, uint64_t width, uint64_t height, uint64_t depth);
/* Quantizer::{quantize_buffer,dequantize_buffer} (src/quant.rs:117-146); error if n_out < n_in */
int alice_codec_quantize_buffer(int32_t step, int32_t dead_zone, const int32_t *in, uint64_t n_in, int32_t *out, uint64_t n_out);
int alice_codec_dequantize_buffer(int32_t step, const int32_t *in, uint64_t n_in, int32_t *out, uint64_t n_out);
/* FastQuantizer (src/quant.rs:171-359) */
typedef struct FastQuantizer FastQuantizer;
FastQuantizer *alice_codec_fastquant_new(int32_t step);                              /* NULL if step <= 0 */
FastQuantizer *alice_codec_fastquant_with_dead_zone(int32_t step, int32_t dead_zone);
void alice_codec_fastquant_destroy(FastQuantizer *q);
int32_t alice_codec_fastquant_step(const FastQuantizer *q);
int32_t alice_codec_fastquant_dead_zone(const FastQuantizer *q);
int alice_codec_fastquant_quantize_buffer(const FastQuantizer *q, const int32_t *in, uint64_t n_in, int32_t *out, uint64_t n_out);
int alice_codec_fastquant_dequantize_buffer(const FastQuantizer *q, const int32_t *in, uint64_t n_in, int32_t *out, uint64_t n_out);
/* to_symbols / from_symbols / build_histogram (src/quant.rs:547-600) */
int alice_codec_to_symbols(const int32_t *coeffs, uint64_t n, uint8_t *symbols, uint64_t n_out);
int alice_codec_from_symbols(const uint8_t *symbols, uint64_t n, int32_t *coeffs, uint64_t n_out);
int alice_codec_build_histogram(const uint8_t *symbols, uint64_t n, uint32_t hist[256]);
/* FrequencyTable::from_histogram over 256 bins (src/rans.rs:102-150): writes cum_freq[256], freq[256] */
int alice_codec_freq_table_from_histogram(const uint32_t hist[256], uint16_t cum_freq[256], uint16_t freq[256]);
/* RansEncoder::new().encode_symbols(symbols, table).finish() (src/rans.rs:288-308); table given as arrays.
 * Returns a buffer to free with alice_codec_data_free64, NULL on error. */
uint8_t *alice_codec_rans_encode(const uint8_t *symbols, uint64_t n, const uint16_t cum_freq[256],
                                 const uint16_t freq[256], uint64_t *out_len);
/* RansDecoder::new(bytes).decode_n(n, table) (src/rans.rs:330-381); cum_to_sym is rebuilt from the arrays */
int alice_codec_rans_decode(const uint8_t *bytes, uint64_t len, const uint16_t cum_freq[256],
                            const uint16_t freq[256], uint64_t n, uint8_t *symbols);
/* FrequencyTable::from_histogram(&[u32]) for a slice of n_symbols bins, 1 <= n_symbols <= 256 (src/rans.rs:102-150; an
 * all-zero slice gives FrequencyTable::uniform(n_symbols), :106-109,158-189).  Entries from n_symbols on come back as
 * (0, 0): those symbols do not exist, and encoding one is an error (the reference indexes out of bounds).  n_symbols = 0:
 * ALICE_ERR_REFERENCE_DIVERGES (the reference divides by zero). */
int alice_codec_freq_table_from_histogram_n(const uint32_t *hist, uint32_t n_symbols, uint16_t cum_freq[256], uint16_t freq[256]);
/* RansEncoder as an object that lives across calls (src/rans.rs:238-309): new / with_capacity, encode(&RansSymbol),
 * encode_symbols (any number of calls: each continues the state, so s1 then s2 leaves the stream of one call on
 * s2 || s1), finish (consumes the encoder; buffer to free with alice_codec_data_free64). */
typedef struct AliceRansEncoder AliceRansEncoder;
AliceRansEncoder *alice_codec_rans_encoder_new(void);
void alice_codec_rans_encoder_destroy(AliceRansEncoder *e);
int alice_codec_rans_encoder_encode(AliceRansEncoder *e, uint16_t cum_freq, uint16_t freq);
int alice_codec_rans_encoder_encode_symbols(AliceRansEncoder *e, const uint8_t *symbols, uint64_t n,
                                            const uint16_t cum_freq[256], const uint16_t freq[256]);
uint32_t alice_codec_rans_encoder_state(const AliceRansEncoder *e);
uint8_t *alice_codec_rans_encoder_finish(AliceRansEncoder *e, uint64_t *out_len);
/* RansDecoder as an object (src/rans.rs:321-389): new (copies the input), decode_n (continues from the current state and
 * position; decode() is decode_n(1)), is_empty. */
typedef struct AliceRansDecoder AliceRansDecoder;
AliceRansDecoder *alice_codec_rans_decoder_new(const uint8_t *data, uint64_t len);
void alice_codec_rans_decoder_destroy(AliceRansDecoder *d);
int alice_codec_rans_decoder_decode_n(AliceRansDecoder *d, uint64_t n, const uint16_t cum_freq[256], const uint16_t freq[256],
                                      uint8_t *symbols);
int alice_codec_rans_decoder_is_empty(const AliceRansDecoder *d);
uint32_t alice_codec_rans_decoder_state(const AliceRansDecoder *d);
uint64_t alice_codec_rans_decoder_position(const AliceRansDecoder *d);
/* quantize_subband / dequantize_subband (src/quant.rs:518-545): a sub-band's coefficients through a Quantizer */
int alice_codec_quantize_subband(int32_t step, int32_t dead_zone, const int32_t *coeffs, uint64_t n, int32_t *out, uint64_t n_out);
int alice_codec_dequantize_subband(int32_t step, const int32_t *coeffs, uint64_t n, int32_t *out, uint64_t n_out);
/* ssim / ms_ssim (src/ssim.rs:63-176): mean SSIM over 8x8 blocks of two single-plane images, and the 3-scale
 * variant.  Bit-identical f64 results (block sums are exact, the mean over blocks is folded in raster order).
 * Returns -1.0 on the reference's Err cases (length mismatch), with alice_codec_last_error() set. */
double alice_codec_ssim(const uint8_t *a, uint64_t a_len, const uint8_t *b, uint64_t b_len, uint64_t width, uint64_t height);
double alice_codec_ms_ssim(const uint8_t *a, uint64_t a_len, const uint8_t *b, uint64_t b_len, uint64_t width, uint64_t height);
/* AnalyticalRDO (src/quant.rs:377-505): with_quality's target bits per pixel, and compute_quantizer for one
 * sub-band (0 = LLL .. 7 = HHH, src/lib.rs:115-132) -> step and dead zone of the Quantizer it returns.  The f64
 * sum of squared deviations is accumulated in element order, as the reference does, so the step is identical. */
double alice_codec_rdo_target_bpp(uint8_t quality);
uint8_t alice_codec_subband_quant_strength(uint8_t subband);     /* SubBand3D::quant_strength, src/lib.rs:149-158 */
int alice_codec_rdo_compute_quantizer(double target_bpp, const int32_t *coeffs, uint64_t n, uint8_t subband,
                                      int32_t *step, int32_t *dead_zone);
/* InterleavedRansEncoder::new().encode(symbols, table).finish() (src/rans.rs:393-456): 32-byte header + four
 * independent streams over the sub-sequences i = j mod 4 (an opt-in format, not used by .alc v1).
 * Returns a buffer to free with alice_codec_data_free64, NULL on error. */
uint8_t *alice_codec_rans_encode_interleaved(const uint8_t *symbols, uint64_t n, const uint16_t cum_freq[256],
                                             const uint16_t freq[256], uint64_t *out_len);
/* InterleavedRansDecoder::new(bytes).decode_n(n, table) (src/rans.rs:468-519; SimdRansDecoder, :531-666, reads
 * the same format).  Inputs on which the reference indexes out of bounds or never terminates give an error. */
int alice_codec_rans_decode_interleaved(const uint8_t *bytes, uint64_t len, const uint16_t cum_freq[256],
                                        const uint16_t freq[256], uint64_t n, uint8_t *symbols);
/* rgb_bytes_to_ycocg_r / ycocg_r_to_rgb_bytes (src/color.rs:199-276) */
int alice_codec_rgb_to_ycocg_r(const uint8_t *rgb, uint64_t rgb_len, int16_t *y, int16_t *co, int16_t *cg, uint64_t n_out);
int alice_codec_ycocg_r_to_rgb(const int16_t *y, const int16_t *co, const int16_t *cg, uint64_t n, uint8_t *rgb, uint64_t rgb_len);

/* ---- device-resident stage calls: the pieces of FrameEncoder::encode / FrameDecoder::decode
 * (src/pipeline.rs:429-497, 581-623) on device pointers, for callers that split ONE chunk across GPUs
 * (row slabs) and run the exchanges between the pieces themselves.
 * d_* are device pointers; work runs on hip_stream (hipStream_t, NULL = default) and has finished on return. ---- */
/* colour + pad + Wavelet3D::forward + Quantizer(step(quality), dead zone = step) + to_symbols
 * (src/pipeline.rs:429-470) of a width x height x frames RGB volume -> 3 * padded u8 symbols (Y, Co, Cg; each
 * [pf][ph][pw], low|high halves along every axis).  d_hist: 3*256 u32 or NULL. */
int alice_codec_dev_forward_symbols(const void *d_rgb, uint32_t width, uint32_t height, uint32_t frames,
                                    uint8_t wavelet_type, uint8_t quality, void *d_symbols, void *d_hist,
                                    void *hip_stream);
/* from_symbols + dequantise (steps as stored in the chunk header) + Wavelet3D::inverse + strip + colour
 * (src/pipeline.rs:597-621) */
int alice_codec_dev_inverse_symbols(const void *d_symbols, uint32_t width, uint32_t height, uint32_t frames,
                                    uint8_t wavelet_type, const int32_t step[3], void *d_rgb, void *hip_stream);
/* Wavelet3D::forward / inverse (src/wavelet.rs:392-484) of a device-resident i32 volume [depth][height][width], in place
 * for the caller; d_tmp: scratch of the same size.  Any i32 values (wrapping sums, 64-bit products).  Even width and
 * height >= 6 with an even depth run two tiled passes over the data; other shapes the per-axis kernels. */
int alice_codec_dev_wavelet3d_forward(uint8_t wavelet_type, void *d_volume, void *d_tmp, uint64_t width, uint64_t height,
                                      uint64_t depth, void *hip_stream);
int alice_codec_dev_wavelet3d_inverse(uint8_t wavelet_type, void *d_volume, void *d_tmp, uint64_t width, uint64_t height,
                                      uint64_t depth, void *hip_stream);
/* build_histogram (src/quant.rs:587-600) of n device symbols -> d_hist[256] (u32, device) */
int alice_codec_dev_histogram(const void *d_symbols, uint64_t n, void *d_hist, void *hip_stream);
/* capacity that alice_codec_dev_rans_encode needs for n symbols whose histogram this is (NULL: worst case, right for any
 * symbols and any table): the stream's length plus 64 bytes the encode chain keeps free at the front of the region */
uint64_t alice_codec_rans_stream_bound(const uint32_t hist[256], uint64_t n);
/* FrequencyTable::from_histogram(hist) + RansEncoder over n device symbols (src/pipeline.rs:479-484): the
 * stream is written at the END of [d_out, d_out + cap): bytes [*out_offset, *out_offset + *out_len).  d_symbols and d_out
 * may have any byte alignment.  `hist` need not be the histogram of these symbols: the table is from_histogram(hist)
 * whatever the symbols are, and the call counts the symbols itself (32-bit counts: n < 2^32, or no symbol that occurs an
 * exact multiple of 2^32 times) to learn which table entries they use.  A symbol whose
 * frequency there is above 4096 (the wrapped freq[255] of src/rans.rs:125-131) is encoded exactly as the reference
 * encodes it; one whose frequency is 0 has no encoding (the reference does not terminate): ReferenceDiverges.  A region
 * that is too small returns InvalidBufferSize and leaves every byte outside [d_out, d_out + cap) alone. */
int alice_codec_dev_rans_encode(const void *d_symbols, uint64_t n, const uint32_t hist[256], void *d_out,
                                uint64_t cap, uint64_t *out_offset, uint64_t *out_len, void *hip_stream);
/* RansDecoder::new(stream).decode_n(n, from_histogram(hist)) (src/pipeline.rs:585-594) into device memory */
int alice_codec_dev_rans_decode(const void *d_stream, uint64_t len, const uint32_t hist[256], void *d_symbols,
                                uint64_t n, void *hip_stream);

/* ---- segmentation ----
 * Person segmentation of the reference (src/segment.rs), bit-exact: a motion mask (|current - reference| > threshold,
 * :172-230) or a chroma-key mask (cg <= green_threshold, :234-265), then a box dilation of dilate_radius and a box erosion
 * of erode_radius (a radius of 0 skips its step; pixels outside the frame count as background for the dilation and as
 * foreground for the erosion, :313-390), then the bounding box [x, y, w, h] and the foreground count (:400-441; an empty
 * mask gives [0,0,0,0] and 0).  Radii are any u32.  Where the reference panics or wraps these return an error: a cg
 * shorter than width*height is ALICE_ERR_INVALID_BUFFER_SIZE, width*height past u32 is ALICE_ERR_DIMENSION_OVERFLOW. */
/* segment_by_motion on host buffers; mask_len >= width*height; a short current, then a short reference, is
 * ALICE_ERR_INVALID_BUFFER_SIZE (:180-191) */
int alice_codec_segment_by_motion(const uint8_t *current, uint64_t current_len, const uint8_t *reference, uint64_t reference_len,
                                  uint32_t width, uint32_t height, uint8_t motion_threshold, uint32_t dilate_radius,
                                  uint32_t erode_radius, uint8_t *mask, uint64_t mask_len, uint32_t bbox[4],
                                  uint32_t *foreground_count);
/* segment_by_chroma (dilate 2, erode 1); the reference's y and co planes are accepted and ignored there, so only cg is taken */
int alice_codec_segment_by_chroma(const int16_t *cg, uint64_t cg_len, uint32_t width, uint32_t height, int16_t green_threshold,
                                  uint8_t *mask, uint64_t mask_len, uint32_t bbox[4], uint32_t *foreground_count);
/* SegmentResult::rle_encode_mask (:131-154): runs of (mask[i] & 1) as [len u16 LE, value u8], a run cut after 65535
 * elements.  Buffer freed with alice_codec_data_free64; an empty mask gives *out_len = 0. */
uint8_t *alice_codec_rle_encode_mask(const uint8_t *mask, uint64_t n, uint64_t *out_len);
/* SegmentResult::extract_person_rgb (:107-125): RGB of the bbox pixels whose mask byte is exactly 1, row-major, with the
 * reference's mask_idx < mask_len and rgb_idx + 2 < rgb_len guards.  out_cap >= 3 * bbox[2] * bbox[3]; every index
 * (y+h-1)*width + x+w-1 must fit u32 (ALICE_ERR_DIMENSION_OVERFLOW otherwise). */
int alice_codec_extract_person_rgb(const uint8_t *mask, uint64_t mask_len, uint32_t width, const uint32_t bbox[4],
                                   const uint8_t *rgb, uint64_t rgb_len, uint8_t *out, uint64_t out_cap, uint64_t *out_len);
/* Device-resident, n_frames frames [f][height][width] in one launch sequence.  Frame f's reference is at
 * d_reference + f * reference_stride (0: one shared background, width*height: one per frame).  d_stats receives
 * n_frames x {x, y, w, h, count} u32; d_mask (n_frames * width*height u8) may be NULL: then only the stats are made.
 * Finished on return, like PART 3. */
int alice_codec_dev_segment_motion(const void *d_current, const void *d_reference, uint64_t reference_stride, uint32_t width,
                                   uint32_t height, uint32_t n_frames, uint8_t motion_threshold, uint32_t dilate_radius,
                                   uint32_t erode_radius, void *d_mask, void *d_stats, void *hip_stream);
/* segment_by_chroma of interleaved RGB frames: Cg is computed on load as alice_codec_rgb_to_ycocg_r does */
int alice_codec_dev_segment_chroma_rgb(const void *d_rgb, uint32_t width, uint32_t height, uint32_t n_frames,
                                       int16_t green_threshold, void *d_mask, void *d_stats, void *hip_stream);
/* the most bytes rle_encode_mask writes for n mask bytes: 3n (the capacity alice_codec_dev_rle_encode_mask requires) */
uint64_t alice_codec_rle_bound(uint64_t n);
int alice_codec_dev_rle_encode_mask(const void *d_mask, uint64_t n, void *d_out, uint64_t cap, uint64_t *out_len,
                                    void *hip_stream);
/* extract_person_rgb of one device frame (mask width*height bytes, rgb 3*width*height); cap >= 3 * bbox[2] * bbox[3] */
int alice_codec_dev_extract_person_rgb(const void *d_mask, uint32_t width, uint32_t height, const uint32_t bbox[4],
                                       const void *d_rgb, void *d_out, uint64_t cap, uint64_t *out_len, void *hip_stream);

/* ---- split-stream format (.alc version 2) ----
 * An opt-in second container.  Colour, padding, 3-D lifting, quantiser and symbol map are those of version 1 (the symbols
 * are the ones alice_codec_dev_forward_symbols gives); the entropy stage is replaced: a frequency table that sums to
 * exactly 4096, stored in the header, and one short independent rANS chain per lane -- blocks of 64 * lane_symbols
 * symbols, lane j of a block owning symbols j, j + 64, ... -- so one chunk uses the whole device and
 * decode(encode(x)) is the video the transform and quantiser define.  Version 1 stays the format for byte compatibility
 * with the reference; alice_codec_chunk_from_bytes keeps refusing version 2.  lane_symbols: a power of two in
 * [64, 16384], or 0 for the default (ALICE_SPLIT_DEFAULT_LANE_SYMBOLS).  A lane whose end check fails (state back at 2^23,
 * cursor at the end of its stream) or a directory that does not add up makes a decode ALICE_ERR_INVALID_BITSTREAM. */
enum { ALICE_SPLIT_DEFAULT_LANE_SYMBOLS = 512, ALICE_SPLIT_HEADER_BYTES = 1630 };
typedef struct AliceSplitInfo {
    uint32_t width, height, frames, lane_symbols;
    uint8_t wavelet, reserved[3];
    int32_t quant_step[3], dead_zone[3];
    uint32_t num_symbols[3], n_blocks[3];
    uint64_t payload_len[3];
} AliceSplitInfo;
/* stage level.  The most bytes a channel payload of n symbols takes (0: lane_symbols out of range or n above 2^32 - 1) */
uint64_t alice_codec_split_stream_bound(uint64_t n, uint32_t lane_symbols);
/* the normalised frequencies of a histogram (sum 4096, present >= 1, absent 0; all zero for an all-zero histogram),
 * computed by the table kernel */
int alice_codec_split_normalize(const uint32_t hist[256], uint16_t freq[256]);
/* n device symbols with histogram hist (it must count exactly n symbols) -> the channel payload (block lengths, then per
 * block the lane directory and the lane streams) at d_out[0 .. *out_len).  `hist` need not be the histogram of these
 * symbols: the table is normalize(hist) whatever the symbols are, and the call counts the symbols itself to learn which
 * table entries they use.  A symbol that occurs while hist[s] == 0 has frequency 0 and no encoding:
 * ALICE_ERR_INVALID_BUFFER_SIZE (the message names the first such symbol and how often it occurs), *out_len = 0 and
 * nothing written.  cap below what the stream needs is ALICE_ERR_INVALID_BUFFER_SIZE with nothing written.  Finished on
 * return. */
int alice_codec_dev_split_encode(const void *d_symbols, uint64_t n, const uint32_t hist[256], uint32_t lane_symbols,
                                 void *d_out, uint64_t cap, uint64_t *out_len, void *hip_stream);
/* a channel payload of len bytes at d_stream (any alignment) with the header's frequencies -> n device symbols */
int alice_codec_dev_split_decode(const void *d_stream, uint64_t len, const uint16_t freq[256], uint32_t lane_symbols,
                                 void *d_symbols, uint64_t n, void *hip_stream);
/* whole chunk, host memory.  encode: the handle's wavelet and quality, alice_codec_encode64's validation in its order, then
 * lane_symbols (ALICE_ERR_INVALID_DIMENSIONS); returns the version 2 bytes (free with alice_codec_data_free64), NULL on error.
 * decode: returns width*height*frames*3 RGB bytes.  Header parsing and validation (alice_codec_split_info is only that) are
 * host code and need no device; the checks run in a fixed order: length of the fixed part, magic, version, wavelet byte,
 * lane_symbols, length of the header, then per channel the quantiser step (at least 1) and dead zone (at least 0),
 * num_symbols (the padded volume, in 64 bits), n_blocks, the
 * frequency sum, payload_len against its directories; then the total length; then each channel's block lengths. */
uint8_t *alice_codec_encode_split(const FrameEncoder *encoder, const uint8_t *rgb, uint64_t rgb_len, uint32_t width,
                                  uint32_t height, uint32_t frames, uint32_t lane_symbols, uint64_t *out_len);
uint8_t *alice_codec_decode_split(const uint8_t *data, uint64_t len, uint64_t *out_len);
int alice_codec_split_info(const uint8_t *data, uint64_t len, AliceSplitInfo *info);
/* device-resident, n_chunks equal-shaped packed chunks per call.  Chunk i is encoded at qualities[i] (NULL: all at
 * `quality`) into d_out + i * out_stride; sizes[i] receives its length.  Any number of chunks: the calls work through
 * them in groups whose symbols take at most 4 GiB (ten 1080p x 64 chunks; one chunk already fills the device).  A chunk
 * longer than out_stride is ALICE_ERR_INVALID_BUFFER_SIZE before anything of its group is written (earlier groups are
 * complete; ALICE_SPLIT_HEADER_BYTES + 3 * alice_codec_split_stream_bound always suffices).  Finished on return. */
int alice_codec_dev_encode_split(const void *d_rgb, uint32_t width, uint32_t height, uint32_t frames, uint32_t n_chunks,
                                 uint8_t wavelet_type, uint8_t quality, const uint8_t *qualities, uint32_t lane_symbols,
                                 void *d_out, uint64_t out_stride, uint64_t *sizes, void *hip_stream);
/* chunk i: sizes[i] bytes at d_alc + i * alc_stride -> pixels at d_rgb_out + i * width*height*frames*3 (shape from the
 * headers; all chunks of a call must agree) */
int alice_codec_dev_decode_split(const void *d_alc, uint64_t alc_stride, const uint64_t *sizes, uint32_t n_chunks,
                                 void *d_rgb_out, void *hip_stream);

/* ---- wide format (.alc version 3) ----
 * Version 2 with an untruncated symbol.  Versions 1 and 2 end their symbol map in the reference's `as u8`, so a
 * quantised coefficient q with |q| > 127 wraps: at the top of the quality scale (small quantiser steps; about q > 90)
 * the decoded video is garbage.  Version 3 codes the wide symbol z = 0, 2q - 1 (q > 0), -2q (q < 0) as the coded symbol
 * min(z, 255) and, behind an escape (255), the residual z - 255 as one uniform 12-bit step of the same lane chain.  Choose
 * it for qualities whose step lets z reach 255; below that its pixels are version 2's and its bytes differ only where the
 * symbol 255 occurs.  lane_symbols: a power of two in [64, 8192] (a symbol emits up to 4 bytes and a lane stream must fit
 * its u16 directory entry), 0 for the default.  The version 2 calls refuse version 3 data and these refuse versions 1 and
 * 2 ("unsupported version").  Size prediction, byte budgets and region calls of version 3 are declared at the end of this
 * header, behind their version 2 twins.  Every call validates like its version 2 twin, in the same order. */
/* the most bytes a channel payload of n wide symbols takes (0: lane_symbols out of range or n above 2^32 - 1) */
uint64_t alice_codec_wide_stream_bound(uint64_t n, uint32_t lane_symbols);
/* stage pair on one channel: n device symbols z as u16; hist is over min(z, 255) and must count exactly n.  As for
 * version 2 it need not be the histogram of these symbols: the table is normalize(hist) whatever the symbols are, the call
 * counts the coded symbols min(z, 255) itself, and one that occurs while hist[s] == 0 (255: any z >= 255) is
 * ALICE_ERR_INVALID_BUFFER_SIZE with *out_len = 0 and nothing written.  A symbol above 255 + 4095 has no code:
 * ALICE_ERR_INTERNAL with nothing written (8-bit RGB stays below 4081).  Otherwise as alice_codec_dev_split_encode /
 * _decode. */
int alice_codec_dev_wide_encode(const void *d_symbols, uint64_t n, const uint32_t hist[256], uint32_t lane_symbols,
                                void *d_out, uint64_t cap, uint64_t *out_len, void *hip_stream);
int alice_codec_dev_wide_decode(const void *d_stream, uint64_t len, const uint16_t freq[256], uint32_t lane_symbols,
                                void *d_symbols, uint64_t n, void *hip_stream);
/* whole chunk, host memory: alice_codec_encode_split / _decode_split / _split_info for version 3 */
uint8_t *alice_codec_encode_wide(const FrameEncoder *encoder, const uint8_t *rgb, uint64_t rgb_len, uint32_t width,
                                 uint32_t height, uint32_t frames, uint32_t lane_symbols, uint64_t *out_len);
uint8_t *alice_codec_decode_wide(const uint8_t *data, uint64_t len, uint64_t *out_len);
int alice_codec_wide_info(const uint8_t *data, uint64_t len, AliceSplitInfo *info);
/* device-resident: alice_codec_dev_encode_split / _dev_decode_split for version 3 (groups are sized at 2 bytes per
 * symbol; ALICE_SPLIT_HEADER_BYTES + 3 * alice_codec_wide_stream_bound always suffices as out_stride) */
int alice_codec_dev_encode_wide(const void *d_rgb, uint32_t width, uint32_t height, uint32_t frames, uint32_t n_chunks,
                                uint8_t wavelet_type, uint8_t quality, const uint8_t *qualities, uint32_t lane_symbols,
                                void *d_out, uint64_t out_stride, uint64_t *sizes, void *hip_stream);
int alice_codec_dev_decode_wide(const void *d_alc, uint64_t alc_stride, const uint64_t *sizes, uint32_t n_chunks,
                                void *d_rgb_out, void *hip_stream);
/* alice_codec_dev_forward_symbols with the wide symbol map: 3 * padded u16 symbols z (what alice_codec_encode_wide codes);
 * d_hist (3*256 u32 or NULL) counts min(z, 255) */
int alice_codec_dev_forward_symbols_wide(const void *d_rgb, uint32_t width, uint32_t height, uint32_t frames,
                                         uint8_t wavelet_type, uint8_t quality, void *d_symbols, void *d_hist,
                                         void *hip_stream);

/* ---- version 2: size prediction, byte budgets, regions of device frames ----
 * Validation of every call below is host code and runs in this order before a device is looked for: NULL arguments,
 * dimensions (overflow, empty), buffer size / regions inside the frame, wavelet byte (ALICE_ERR_INVALID_BITSTREAM),
 * lane_symbols (ALICE_ERR_INVALID_DIMENSIONS), then the quality range (min_q > max_q after qualities above 100 became 100:
 * ALICE_ERR_INVALID_DIMENSIONS).  Memory comes from the library's pool; nothing goes through the chain hub. */
enum { ALICE_SPLIT_REFINE_TRIALS = 4 };
/* lo[q] <= length of alice_codec_encode_split at quality q <= hi[q] for q = 0 .. 100, from one forward transform (no
 * entropy coding): the bracket of every channel payload (about one byte per lane wide) plus the 1630-byte header.  Every
 * version 2 table is bounded, so there is no status array.  A chunk without pixels is 1630 / 1630. */
int alice_codec_predict_split_sizes(uint8_t wavelet_type, const uint8_t *rgb, uint64_t rgb_len, uint32_t width, uint32_t height,
                                    uint32_t frames, uint32_t lane_symbols, uint64_t lo[101], uint64_t hi[101]);
/* n_chunks packed device chunks; lo / hi: n_chunks * 101 */
int alice_codec_dev_predict_split_sizes(const void *d_rgb, uint32_t width, uint32_t height, uint32_t frames, uint32_t n_chunks,
                                        uint8_t wavelet_type, uint32_t lane_symbols, uint64_t *lo, uint64_t *hi, void *hip_stream);
/* One chunk as version 2 bytes at the quality the budget rule picks in [min_q, max_q] (qualities above 100 act as 100):
 *  1. q0 = the largest quality whose hi fits max_bytes;
 *  2. the qualities above q0 (all of them without a q0) whose bracket straddles max_bytes are tried from the highest down,
 *     one exact size (forward pass, table, count pass: no byte written) per quantiser step not tried before, at most
 *     ALICE_SPLIT_REFINE_TRIALS in all; the first that fits is chosen;
 *  3. otherwise q0; without one, min_q with *fits = 0 (the chunk is still encoded).
 * The bytes are exactly alice_codec_encode_split's at *chosen_q.  Free with alice_codec_data_free64; NULL on error. */
uint8_t *alice_codec_encode_split_to_size(uint8_t wavelet_type, const uint8_t *rgb, uint64_t rgb_len, uint32_t width,
                                          uint32_t height, uint32_t frames, uint32_t lane_symbols, uint64_t max_bytes,
                                          uint8_t min_q, uint8_t max_q, uint8_t *chosen_q, uint8_t *fits, uint64_t *out_len);
/* Regions of device frames, with the semantics of alice_codec_batch_encode_regions / _decode_regions: chunk i is frames
 * [i * frames, (i + 1) * frames) of the frame_width x frame_height packed RGB frames at d_frames, cropped to width x height
 * at origins[2i], origins[2i + 1] (2 * n_chunks u32, read before return).  A rectangle that does not lie inside the frame
 * is ALICE_ERR_INVALID_DIMENSIONS with nothing queued or written.  The bytes of chunk i are alice_codec_encode_split's of
 * the crop; otherwise as alice_codec_dev_encode_split. */
int alice_codec_dev_encode_split_regions(const void *d_frames, uint32_t frame_width, uint32_t frame_height, const uint32_t *origins,
                                         uint32_t width, uint32_t height, uint32_t frames, uint32_t n_chunks, uint8_t wavelet_type,
                                         uint8_t quality, const uint8_t *qualities, uint32_t lane_symbols, void *d_out,
                                         uint64_t out_stride, uint64_t *sizes, void *hip_stream);
/* alice_codec_dev_decode_split with chunk i pasted into its rectangle of frames [i * frames, (i + 1) * frames) of
 * d_frames_out (shape from the headers): no byte outside the rectangles is written. */
int alice_codec_dev_decode_split_regions(const void *d_alc, uint64_t alc_stride, const uint64_t *sizes, uint32_t n_chunks,
                                         void *d_frames_out, uint32_t frame_width, uint32_t frame_height, const uint32_t *origins,
                                         void *hip_stream);
/* Budget encode of n_chunks device chunks, chunk i under budgets[i] by the rule of alice_codec_encode_split_to_size:
 * chosen[i], fits[i], sizes[i] and the bytes at d_out + i * out_stride.  origins == NULL: packed chunks at d_frames
 * (frame_width / frame_height unused); otherwise regions as above.  On error chosen, fits and sizes are left alone. */
int alice_codec_dev_encode_split_to_budget(const void *d_frames, uint32_t frame_width, uint32_t frame_height, const uint32_t *origins,
                                           uint32_t width, uint32_t height, uint32_t frames, uint32_t n_chunks, uint8_t wavelet_type,
                                           uint32_t lane_symbols, const uint64_t *budgets, uint8_t min_q, uint8_t max_q,
                                           uint8_t *chosen, uint8_t *fits, void *d_out, uint64_t out_stride, uint64_t *sizes,
                                           void *hip_stream);

/* ---- version 3: size prediction, byte budgets, regions of device frames ----
 * The calls above for the wide container: the same bodies with the version as an argument, the same validation in the
 * same order before a device is looked for, with lane_symbols a power of two in [64, 8192] (16384 is refused), the same
 * budget rule and ALICE_SPLIT_REFINE_TRIALS.  The histogram priced is of the coded symbol min(z, 255); its bin 255 is the
 * number of escapes E, and each escape adds one chain step of exactly 12 bits (the residual), so the bracket is version 2's
 * with n + E steps and 12 E more bits.  A trial is the wide forward pass, the table and the wide count pass; the residual
 * guard applies to it as to an encode (ALICE_ERR_INTERNAL before a byte is written). */
/* lo[q] <= length of alice_codec_encode_wide at quality q <= hi[q] for q = 0 .. 100.  A chunk without pixels is 1630 / 1630. */
int alice_codec_predict_wide_sizes(uint8_t wavelet_type, const uint8_t *rgb, uint64_t rgb_len, uint32_t width, uint32_t height,
                                   uint32_t frames, uint32_t lane_symbols, uint64_t lo[101], uint64_t hi[101]);
/* n_chunks packed device chunks; lo / hi: n_chunks * 101.  d_step_hist: NULL, or device memory for n_chunks * 64 * 3 * 256
 * u32 that receives the histograms of the coded symbol behind the prediction, [chunk][step - 1][channel][symbol]. */
int alice_codec_dev_predict_wide_sizes(const void *d_rgb, uint32_t width, uint32_t height, uint32_t frames, uint32_t n_chunks,
                                       uint8_t wavelet_type, uint32_t lane_symbols, uint64_t *lo, uint64_t *hi, void *d_step_hist,
                                       void *hip_stream);
/* alice_codec_encode_split_to_size for version 3: the bytes are exactly alice_codec_encode_wide's at *chosen_q. */
uint8_t *alice_codec_encode_wide_to_size(uint8_t wavelet_type, const uint8_t *rgb, uint64_t rgb_len, uint32_t width,
                                         uint32_t height, uint32_t frames, uint32_t lane_symbols, uint64_t max_bytes,
                                         uint8_t min_q, uint8_t max_q, uint8_t *chosen_q, uint8_t *fits, uint64_t *out_len);
/* alice_codec_dev_encode_split_regions / _dev_decode_split_regions for version 3: the bytes of chunk i are
 * alice_codec_encode_wide's of the crop; a rectangle outside the frame is ALICE_ERR_INVALID_DIMENSIONS with nothing queued
 * or written; a decode writes no byte outside the rectangles. */
int alice_codec_dev_encode_wide_regions(const void *d_frames, uint32_t frame_width, uint32_t frame_height, const uint32_t *origins,
                                        uint32_t width, uint32_t height, uint32_t frames, uint32_t n_chunks, uint8_t wavelet_type,
                                        uint8_t quality, const uint8_t *qualities, uint32_t lane_symbols, void *d_out,
                                        uint64_t out_stride, uint64_t *sizes, void *hip_stream);
int alice_codec_dev_decode_wide_regions(const void *d_alc, uint64_t alc_stride, const uint64_t *sizes, uint32_t n_chunks,
                                        void *d_frames_out, uint32_t frame_width, uint32_t frame_height, const uint32_t *origins,
                                        void *hip_stream);
/* alice_codec_dev_encode_split_to_budget for version 3: packed chunks when origins == NULL, regions otherwise; the trials run
 * chunk by chunk and the final encode in the groups of alice_codec_dev_encode_wide. */
int alice_codec_dev_encode_wide_to_budget(const void *d_frames, uint32_t frame_width, uint32_t frame_height, const uint32_t *origins,
                                          uint32_t width, uint32_t height, uint32_t frames, uint32_t n_chunks, uint8_t wavelet_type,
                                          uint32_t lane_symbols, const uint64_t *budgets, uint8_t min_q, uint8_t max_q,
                                          uint8_t *chosen, uint8_t *fits, void *d_out, uint64_t out_stride, uint64_t *sizes,
                                          void *hip_stream);

/* ---- reversible format (.alc version 4) ----
 * Version 3 with a decoder whose inverse lifting is the forward's mirror: the steps in reverse order, each one
 * target -= delta(neighbours, +c) with the forward's own delta, where the reference's inverse (versions 1 to 3) re-runs the
 * step with the negated coefficient and is off by one wherever (a + b) * c = 4096 (mod 8192).  At quality 100 (quantiser
 * step 1) the decoded pixels ARE the input: choose it for lossless archival or intermediate storage.  Any quality is
 * legal (the header stores the step); below 100 its pixels are no better than version 3's and it is not recommended.
 * The encoder is version 3's: the bytes equal alice_codec_encode_wide's of the same call except byte 4 (the version), so
 * alice_codec_predict_wide_sizes / _dev_predict_wide_sizes are exact for version 4 and alice_codec_wide_stream_bound is
 * its stream bound; there are no byte-budget calls.  These calls refuse versions 1 to 3 and the calls of those versions
 * refuse version 4 ("unsupported version: 3 (expected 4)").  Every call validates like its version 3 twin, in the same
 * order. */
uint8_t *alice_codec_encode_reversible(const FrameEncoder *encoder, const uint8_t *rgb, uint64_t rgb_len, uint32_t width,
                                       uint32_t height, uint32_t frames, uint32_t lane_symbols, uint64_t *out_len);
uint8_t *alice_codec_decode_reversible(const uint8_t *data, uint64_t len, uint64_t *out_len);
int alice_codec_reversible_info(const uint8_t *data, uint64_t len, AliceSplitInfo *info);
/* device-resident: alice_codec_dev_encode_wide / _dev_decode_wide for version 4 */
int alice_codec_dev_encode_reversible(const void *d_rgb, uint32_t width, uint32_t height, uint32_t frames, uint32_t n_chunks,
                                      uint8_t wavelet_type, uint8_t quality, const uint8_t *qualities, uint32_t lane_symbols,
                                      void *d_out, uint64_t out_stride, uint64_t *sizes, void *hip_stream);
int alice_codec_dev_decode_reversible(const void *d_alc, uint64_t alc_stride, const uint64_t *sizes, uint32_t n_chunks,
                                      void *d_rgb_out, void *hip_stream);
/* alice_codec_dev_encode_wide_regions / _dev_decode_wide_regions for version 4 */
int alice_codec_dev_encode_reversible_regions(const void *d_frames, uint32_t frame_width, uint32_t frame_height,
                                              const uint32_t *origins, uint32_t width, uint32_t height, uint32_t frames,
                                              uint32_t n_chunks, uint8_t wavelet_type, uint8_t quality, const uint8_t *qualities,
                                              uint32_t lane_symbols, void *d_out, uint64_t out_stride, uint64_t *sizes,
                                              void *hip_stream);
int alice_codec_dev_decode_reversible_regions(const void *d_alc, uint64_t alc_stride, const uint64_t *sizes, uint32_t n_chunks,
                                              void *d_frames_out, uint32_t frame_width, uint32_t frame_height,
                                              const uint32_t *origins, void *hip_stream);

/* ---- quality control: exact trial distortion and PSNR-floor encodes ----
 * The lane coders of versions 2, 3 and 4 are lossless, so the pixels a decode returns are the format's inverse transform of
 * the format's forward symbols: the distortion of an encode is known from a transform pair and one comparison pass, without
 * a byte of a container.  The container is chosen by its version byte; any other value is ALICE_ERR_INVALID_BITSTREAM.
 * Version 1 has no such calls (its decoder desynchronises on almost all content).  Validation is host code in this order
 * before a device is looked for: null arguments, the format byte, dimensions (overflow, empty), pitches / regions inside
 * the frame, wavelet byte (ALICE_ERR_INVALID_BITSTREAM), lane_symbols (ALICE_ERR_INVALID_DIMENSIONS), the quality range
 * (as in the budget calls), then the target.  Memory comes from the library's pool; nothing goes through the chain hub. */
enum { ALICE_FORMAT_SPLIT = 2, ALICE_FORMAT_WIDE = 3, ALICE_FORMAT_REVERSIBLE = 4 };
enum { ALICE_QUALITY_MAX_TRIALS = 8 };
/* d_frame_sse[k] (n_frames u64 on the device) = the exact sum over frame k of (a - b)^2, all three colours, of two volumes
 * of n_frames frames of width x height interleaved 8-bit RGB on the device.  Pixel x of row y of frame k of a side is at
 * base + k * frame_pitch + y * row_pitch + 3 x; the base may have any byte alignment; a packed volume has pitches 3 * width
 * and 3 * width * height.  A row pitch below 3 * width or a frame pitch below (height - 1) * row_pitch + 3 * width is
 * ALICE_ERR_INVALID_DIMENSIONS.  Only the pixels named are read.  Integer arithmetic throughout.  Finished on return. */
int alice_codec_dev_rgb_sse(const void *d_a, uint64_t a_row_pitch, uint64_t a_frame_pitch, const void *d_b, uint64_t b_row_pitch,
                            uint64_t b_frame_pitch, uint32_t width, uint32_t height, uint64_t n_frames, void *d_frame_sse,
                            void *hip_stream);
/* Trial distortion of n_chunks device chunks (packed when origins == NULL, regions otherwise, as in
 * alice_codec_dev_encode_split_to_budget), chunk i at qualities[i] (NULL: all at `quality`): the format's forward pass to
 * symbols, the format's inverse (the reference's for versions 2 and 3, the mirrored one for version 4) into scratch, and the
 * comparison against the source.  sse[i] (host) = the chunk's total; d_frame_sse: NULL, or device memory for
 * n_chunks * frames u64, [chunk][frame].  No lane coding, no table, no byte of a container; the chunks are worked on in
 * the groups of alice_codec_dev_encode_split / _wide.  CONTRACT: sse[i] equals the squared error between the source and the
 * pixels the format's decode returns for the format's encode at that quality, bit for bit.  On error sse is left alone. */
int alice_codec_dev_trial_sse(uint8_t format, const void *d_frames, uint32_t frame_width, uint32_t frame_height,
                              const uint32_t *origins, uint32_t width, uint32_t height, uint32_t frames, uint32_t n_chunks,
                              uint8_t wavelet_type, uint8_t quality, const uint8_t *qualities, uint64_t *sse, void *d_frame_sse,
                              void *hip_stream);
/* The dB value of a squared error over n_bytes samples, by the expression alice_codec_psnr uses (which calls this):
 * +inf when the mean squared error is 0, else 10 * log10(255^2 / (sse / n_bytes)).  No device, no error state. */
double alice_codec_psnr_from_sse(uint64_t sse, uint64_t n_bytes);
/* PSNR-floor encode: the smallest quality whose trial reaches min_psnr_db, for versions 2 and 3 (version 4 is refused: a
 * lossless encode has no quality to search).  min_psnr_db NaN or negative is ALICE_ERR_INVALID_DIMENSIONS; +inf means exact.
 * The rule, per chunk (N = the unpadded chunk's bytes, T = min_psnr_db):
 *   1. sse_max = floor(65025 * N / 10^(T / 10)) in f64 (0 for T = +inf).  A trial passes iff its integer sse <= sse_max:
 *      integers decide, not the reported dB.
 *   2. The candidates are the distinct quantiser steps of the qualities in [min_q, max_q] after qualities above 100 became
 *      100; the step falls with quality, and each step is tried at the lowest quality that has it.
 *   3. The finest step (max_q's) is tried.  If it fails: chosen = max_q, reached = 0.
 *   4. The coarsest step (min_q's) is tried.  If it passes it is chosen.
 *   5. Otherwise bisection between a passing finer step and a failing coarser one, the midpoint rounded towards the finer,
 *      until they are adjacent; the coarsest passing step found is chosen.  At most ALICE_QUALITY_MAX_TRIALS = 2 + 6 trials
 *      for the 64 steps.
 *   6. chosen = the lowest quality in the range with the chosen step; the bytes are exactly alice_codec_encode_split's /
 *      _wide's at chosen; psnr = alice_codec_psnr_from_sse of the chosen step's trial.
 * Bisection assumes that distortion does not fall as the step grows.  The call PROMISES only: the returned point was
 * measured, `reached` tells the truth about it, and no trial between the finest step and the chosen one was seen to fail.
 * On 64x48x8 smooth-plus-noise content the CPU oracle finds version 3 monotone over all 64 steps for all three wavelets;
 * version 2 is NOT among steps 1 to 3 (q >= 97), where the u8 symbol wraps (step 1 with every wavelet, steps 2 and 3 too
 * with CDF 9/7): there the finest step fails and the call answers max_q with reached = 0.  Callers who want a floor near the top should use version 3, or max_q <= 96 with version 2.
 * Device call: packed chunks when origins == NULL, regions otherwise; chosen / reached / psnr / sizes per chunk and the
 * bytes at d_out + i * out_stride; the trials run chunk by chunk, the final encode in the groups of
 * alice_codec_dev_encode_split / _wide.  On error the outputs are left alone. */
int alice_codec_dev_encode_to_psnr(uint8_t format, const void *d_frames, uint32_t frame_width, uint32_t frame_height,
                                   const uint32_t *origins, uint32_t width, uint32_t height, uint32_t frames, uint32_t n_chunks,
                                   uint8_t wavelet_type, uint32_t lane_symbols, double min_psnr_db, uint8_t min_q, uint8_t max_q,
                                   uint8_t *chosen, uint8_t *reached, double *psnr, void *d_out, uint64_t out_stride,
                                   uint64_t *sizes, void *hip_stream);
/* The same for one chunk in host memory: returns the bytes (free with alice_codec_data_free64), NULL on error.  A chunk
 * without pixels has squared error 0 at every step: min_q, reached, +inf, and the 1630-byte header. */
uint8_t *alice_codec_encode_to_psnr(uint8_t format, uint8_t wavelet_type, const uint8_t *rgb, uint64_t rgb_len, uint32_t width,
                                    uint32_t height, uint32_t frames, uint32_t lane_symbols, double min_psnr_db, uint8_t min_q,
                                    uint8_t max_q, uint8_t *chosen_q, uint8_t *reached, double *psnr, uint64_t *out_len);

/* ---- frame ranges of a version 2, 3 or 4 chunk ----
 * The lane formats cut a channel's symbols, coded in [t'][y][x] order, into blocks of 64 * lane_symbols symbols behind a
 * table of their byte lengths, and the temporal transform is one lifting level: frames [first, first + count) depend on
 * the coefficient planes of the frame pairs inside a window [a, b) only.  With pf the padded frame count (frames rounded up
 * to even; 2 for 1), NS the wavelet's lifting steps (4 for CDF 9/7; 2 for CDF 5/3 and for Haar, whose predict step
 * averages both even neighbours) and t1 = first + count:
 *     a = max(0, (first - NS) & ~1)        b = min(pf, (t1 + NS + 1) & ~1)
 * The planes a/2 .. b/2 of the low band and of the high band are the symbol volume of a chunk of b - a frames whose inverse
 * temporal lifting equals the full chunk's at [first - a, t1 - a), bit for bit.  These calls decode the blocks that
 * intersect those planes, run the temporal pass over them, and the spatial pass over `count` frames.  The pixels are the
 * full decode's, the inverse instance is the full decode's (it depends on the wavelet and the quantiser steps alone).
 * INTEGRITY: the whole block-length tables are checked, so a damaged table is refused wherever the damage is; the lane end
 * checks cover the blocks that are decoded.  Damage inside a lane of any other block is NOT seen: a range may decode from
 * a file whose full decode is refused.  A range that is refused for damage in a decoded block writes nothing to d_rgb_out:
 * the verdict of the end checks is read before the inverse is queued.
 * Validation is host code in this order: null arguments; the fixed fields and the magic; the version byte (1 is
 * ALICE_ERR_INVALID_BITSTREAM, "version 1 has no random access (one serial chain per channel)"; anything but 2, 3, 4 is
 * refused as unsupported); that version's header checks in their order; count >= 1 and first + count <=
 * frames, else ALICE_ERR_INVALID_DIMENSIONS (so a chunk without pixels refuses every range).  Nothing is queued or written
 * on a refusal.  Memory comes from the library's pool; nothing goes through the chain hub. */
/* The window of a range; no device needed.  wavelet_type above 2: ALICE_ERR_INVALID_BITSTREAM; frames = 2^32 - 1 (its
 * padded count does not fit b): ALICE_ERR_DIMENSION_OVERFLOW; count 0 or first + count above frames:
 * ALICE_ERR_INVALID_DIMENSIONS. */
int alice_codec_frames_window(uint8_t wavelet_type, uint32_t frames, uint32_t first, uint32_t count, uint32_t *a, uint32_t *b);
/* One container in host memory -> count * height * width * 3 packed RGB bytes (free with alice_codec_data_free64), NULL on
 * error.  Reads and uploads the 1630-byte header, the three block-length tables and the byte runs of the planned blocks,
 * nothing else of `data` (which may be a mapped file); downloads `count` frames. */
uint8_t *alice_codec_decode_frames(const uint8_t *data, uint64_t len, uint32_t first, uint32_t count, uint64_t *out_len);
/* The same for a container of `len` bytes on the device (any byte alignment) into count packed frames at d_rgb_out, which
 * must not overlap it.  The header is read back first.  Finished on return. */
int alice_codec_dev_decode_frames(const void *d_alc, uint64_t len, uint32_t first, uint32_t count, void *d_rgb_out,
                                  void *hip_stream);

/* ---- Half-resolution preview of a version 2, 3 or 4 chunk from the low band alone ----
 * The spatial transform is one lifting level, so the low-low quadrant of every coefficient plane is a half-size picture of
 * qw x qh = ceil(width / 2) x ceil(height / 2) pixels.  For frames [first, first + count) these calls decode the blocks
 * that intersect the quadrants of the planes inside the frame-range window [a, b) above -- the top half of a plane is one
 * contiguous symbol run; the bottom half is never entropy-decoded -- and finish in one launch: dequantise, the container's
 * inverse temporal lifting, n = (v * K + 32768) >> 16 (64-bit product, arithmetic shift; K = 65536 for CDF 5/3 and Haar,
 * whose low band has DC gain 1, and 47484 = round(65536 / 1.17480326^2) for CDF 9/7), `as i16`, colour.  No spatial inverse
 * runs.  The output is count * qh * qw * 3 packed RGB bytes; it approximates the 2x2 box average of the full decode (it is
 * the wavelet's low-pass, not the box filter).
 * Validation, its order and its codes are alice_codec_decode_frames' (version 1: "no random access").  INTEGRITY as above:
 * the whole block-length tables are checked, the lane end checks cover the decoded blocks only, and a refusal for damage in
 * a decoded block writes nothing to d_rgb_out.  Memory comes from the library's pool; nothing goes through the chain hub. */
/* qw, qh of a width x height picture; no device needed.  width or height 0: ALICE_ERR_INVALID_DIMENSIONS. */
int alice_codec_preview_dims(uint32_t width, uint32_t height, uint32_t *qw, uint32_t *qh);
/* One container in host memory -> count * qh * qw * 3 packed RGB bytes (free with alice_codec_data_free64), NULL on error.
 * Reads and uploads the 1630-byte header, the three block-length tables and the byte runs of consecutive planned blocks,
 * nothing else of `data` (which may be a mapped file). */
uint8_t *alice_codec_decode_preview(const uint8_t *data, uint64_t len, uint32_t first, uint32_t count, uint64_t *out_len);
/* The same for a container of `len` bytes on the device (any byte alignment) into d_rgb_out, which must not overlap it.
 * The header is read back first.  Finished on return. */
int alice_codec_dev_decode_preview(const void *d_alc, uint64_t len, uint32_t first, uint32_t count, void *d_rgb_out,
                                   void *hip_stream);

/* ---- Many previews in one call ----
 * A contact sheet wants one frame of each of N chunks, a scrub bar every k-th frame of one chunk.  These calls take an array
 * of items; every item alone means exactly what alice_codec_dev_decode_preview(alc, len, first, count, rgb_out, stream)
 * means, bit for bit.  Items may mix versions 2, 3 and 4, the wavelets, dimensions and lane sizes, and any number of items
 * may name the same container (the same pointer and the same len): such items share one header fetch, one validation, one
 * set of tables and one directory scan.  One launch builds every table, one covers every directory, one lane launch per
 * symbol width decodes the planned blocks of all items, and the finish runs once per instance class present.
 * ALL OR NOTHING.  Validation: items NULL (ALICE_ERR_NULL_ARGUMENT), n_items 0 or above ALICE_PREVIEWS_MAX_ITEMS
 * (ALICE_ERR_INVALID_DIMENSIONS), a NULL alc -- or, dev call, rgb_out -- in an item (ALICE_ERR_NULL_ARGUMENT), then
 * alice_codec_decode_frames' checks, in its order and with its codes, item after item; the dev call then refuses two items
 * whose output byte ranges overlap (ALICE_ERR_INVALID_DIMENSIONS, the later item of the pair).  The first item that fails
 * decides the code, *bad_item (when not NULL) receives its index and the message starts with "item <index>: "; a refusal
 * that is no item's leaves *bad_item = 0xFFFFFFFF.  A refused call queues nothing and writes nothing.  INTEGRITY: the end
 * checks of all items are read in one copy before anything that writes an output is queued; a directory that does not add
 * up or a failed lane in a planned block of any item is ALICE_ERR_INVALID_BITSTREAM for the whole call with *bad_item the
 * first such item, and no output is written, the clean items' included.  Damage in a block no item plans is not seen.
 * Memory comes from the library's pool; nothing goes through the chain hub. */
typedef struct alice_codec_preview_item {
    const void *alc;       /* the container: device memory for the dev call, host memory for the host call */
    uint64_t    len;
    uint32_t    first, count;
    void       *rgb_out;   /* dev call: count * qh * qw * 3 packed bytes go here; host call: ignored */
} alice_codec_preview_item;

#define ALICE_PREVIEWS_MAX_ITEMS 1024u

/* Containers on the device (any byte alignment), outputs on the device (any byte alignment, disjoint, not overlapping a
 * container).  The stream is drained at most three times: after the header fetches of all distinct containers, at the
 * verdict, and at the end.  Finished on return. */
int alice_codec_dev_decode_previews(const alice_codec_preview_item *items, uint32_t n_items, uint32_t *bad_item, void *hip_stream);
/* Containers in host memory (they may be mapped files) -> one buffer (free with alice_codec_data_free64(ptr,
 * offsets[n_items])), NULL on error; item i is at [offsets[i], offsets[i + 1]), in item order.  Per distinct container the
 * 1630-byte header, the three block-length tables and the byte runs of the union of its items' planned blocks go up, once.
 * offsets (n_items + 1 entries) is left alone on a refusal. */
uint8_t *alice_codec_decode_previews(const alice_codec_preview_item *items, uint32_t n_items, uint64_t *offsets, uint32_t *bad_item);

/* ---- A spatial rectangle of a frame range of a version 2, 3 or 4 chunk ----
 * The spatial transform is one lifting level per axis and every axis of a channel's [t'][y][x] symbol volume is stored as
 * [low | high], so the frame-range rule above holds on x and on y as it holds on t.  With pw, ph the padded width and
 * height, for an axis of padded length pn and the real positions [c0, c1):
 *     a = 0 if c0 - NS <= 0 else (c0 - NS) & ~1        b = min(pn, (c1 + NS + 1) & ~1)
 * gives [ta, tb), [ya, yb) and [xa, xb).  The coefficients whose coordinate lies, on every axis, in [a/2, b/2) or in
 * pn/2 + [a/2, b/2) are, low run then high run, the symbol volume of a chunk of (xb - xa) x (yb - ya) x (tb - ta) whose
 * inverse equals the full chunk's at the rectangle shifted by (xa, ya, ta), bit for bit.  These calls decode the blocks
 * that hold such a coefficient, run the container's inverse over that virtual chunk (the instance is the full decode's) and
 * copy the w x h pixels at (x, y) of frames [first, first + count) out of it; a rectangle that is the whole frame is
 * written directly and costs what a frame range costs.  The pixels are the full decode's.
 * Validation, its order and its codes are alice_codec_decode_frames' (version 1: "no random access"); then w >= 1, h >= 1,
 * x + w <= width and y + h <= height, else ALICE_ERR_INVALID_DIMENSIONS; then the pitches.  INTEGRITY as above: the whole
 * block-length tables are checked, the lane end checks cover the decoded blocks only, and a refusal for damage in a decoded
 * block writes nothing to d_rgb_out.  Nothing is queued or written on a refusal.  Memory comes from the library's pool;
 * nothing goes through the chain hub. */
/* The spatial windows of a rectangle of a width x height frame; no device needed.  wavelet_type above 2:
 * ALICE_ERR_INVALID_BITSTREAM; width or height = 2^32 - 1: ALICE_ERR_DIMENSION_OVERFLOW; a rectangle that is empty or
 * does not lie inside the frame: ALICE_ERR_INVALID_DIMENSIONS. */
int alice_codec_rect_window(uint8_t wavelet_type, uint32_t width, uint32_t height, uint32_t x, uint32_t y, uint32_t w, uint32_t h,
                            uint32_t *xa, uint32_t *xb, uint32_t *ya, uint32_t *yb);
/* One container in host memory -> count * h * w * 3 packed RGB bytes (free with alice_codec_data_free64), NULL on error.
 * Reads and uploads the 1630-byte header, the three block-length tables and the byte runs of consecutive planned blocks,
 * nothing else of `data` (which may be a mapped file); downloads the rectangles. */
uint8_t *alice_codec_decode_rect(const uint8_t *data, uint64_t len, uint32_t first, uint32_t count, uint32_t x, uint32_t y,
                                 uint32_t w, uint32_t h, uint64_t *out_len);
/* The same for a container of `len` bytes on the device (any byte alignment).  Pixel i of row r of frame k of the rectangle
 * goes to d_rgb_out + k * frame_pitch + r * row_pitch + 3 * i (pitches in bytes); row_pitch = frame_pitch = 0 means packed
 * (3 w, 3 w h); one of them 0 takes its packed value from the other.  Non-zero pitches need row_pitch >= 3 w and
 * frame_pitch >= row_pitch * h, else ALICE_ERR_INVALID_DIMENSIONS.  Only the 3 w bytes of each of the h rows of each frame
 * are written, so d_rgb_out may point into full-size frames.  The output must not overlap the container.  The header is
 * read back first.  Finished on return. */
int alice_codec_dev_decode_rect(const void *d_alc, uint64_t len, uint32_t first, uint32_t count, uint32_t x, uint32_t y, uint32_t w,
                                uint32_t h, void *d_rgb_out, uint64_t row_pitch, uint64_t frame_pitch, void *hip_stream);

/* ---- Many frame ranges and rectangles in one call ----
 * A detector wants the same crop of frame k of every chunk, a viewer a mosaic of crops pasted into one surface, a sheet
 * frame 0 of each of N chunks at full resolution.  These calls take an array of items, as the batched preview does; every
 * item alone means exactly what alice_codec_dev_decode_rect(alc, len, first, count, x, y, w, h, rgb_out, row_pitch,
 * frame_pitch, stream) means, bit for bit, and an item with x = y = w = h = 0 is the whole frame: what
 * alice_codec_dev_decode_frames means (its pitches, when given, are those of a rectangle that is the whole frame).  Items
 * may mix versions 2, 3 and 4, the wavelets, dimensions, lane sizes, ranges and rectangles, and any number of items may name
 * the same container (the same pointer and the same len): such items share one header fetch, one validation, one set of
 * tables and one directory scan.  One launch builds every table, one covers every directory, at most four lane launches
 * (whole planes or boxes, u8 or u16 symbols) decode the planned blocks of all items, and the finish -- the window inverse's
 * two roles and the paste -- runs once per instance class present over all items; an item whose virtual chunk the tile
 * kernels do not take, or whose inverse is cut into bands, is finished on its own after those, on the same stream.
 * ALL OR NOTHING.  Validation: items NULL (ALICE_ERR_NULL_ARGUMENT), n_items 0 or above ALICE_RECTS_MAX_ITEMS
 * (ALICE_ERR_INVALID_DIMENSIONS), a NULL alc -- or, dev call, rgb_out -- in an item (ALICE_ERR_NULL_ARGUMENT), all without a
 * device; then, item after item, alice_codec_decode_frames' checks in its order and with its codes (a container's header
 * is checked once), the rectangle's and the pitches' of alice_codec_dev_decode_rect; the dev call then refuses two items
 * whose outputs conflict (ALICE_ERR_INVALID_DIMENSIONS, the later item of the first such pair in item order).  The first
 * item that fails decides the code, *bad_item (when not NULL) receives its index and the message starts with
 * "item <index>: "; a refusal that is no item's leaves *bad_item = 0xFFFFFFFF.  A refused call queues nothing and writes
 * nothing.
 * DISJOINT OUTPUTS.  An item's enclosing byte range is [rgb_out, rgb_out + (count - 1) frame_pitch + (h - 1) row_pitch +
 * 3 w) with its effective pitches.  Two items conflict when these ranges intersect -- unless both have the same effective
 * row_pitch and frame_pitch and are disjoint boxes of that surface: with off the distance of an item's base from the lower
 * of the two bases, t = off / frame_pitch, y = (off % frame_pitch) / row_pitch, x_byte = (off % frame_pitch) % row_pitch,
 * each item stays a box (x_byte + 3 w <= row_pitch, (y + h) row_pitch <= frame_pitch) and the boxes [t, t + count) x [y,
 * y + h) x [x_byte, x_byte + 3 w) are apart on at least one axis.  This is exact for items pasted into a common surface
 * (a mosaic, whose ranges interleave) and conservative elsewhere: interleaved ranges with different pitches, or a row that
 * wraps past row_pitch, are refused although their bytes may be disjoint.
 * INTEGRITY: the end checks of all items are read in one copy before anything that writes an output is queued; a directory
 * that does not add up or a failed lane in a planned block of any item is ALICE_ERR_INVALID_BITSTREAM for the whole call
 * with *bad_item the first such item, and no output is written, the clean items' included.  Damage in a block no item plans
 * is not seen.  Memory comes from the library's pool (every item's volumes are sub-ranges of pooled buffers; a failed
 * allocation is ALICE_ERR_OUT_OF_MEMORY before any output is written); nothing goes through the chain hub. */
typedef struct alice_codec_rect_item {
    const void *alc;       /* the container: device memory for the dev call, host memory for the host call */
    uint64_t    len;
    uint32_t    first, count;              /* frames [first, first + count) */
    uint32_t    x, y, w, h;                /* x = y = w = h = 0: the whole frame (a frame range) */
    void       *rgb_out;                   /* dev call: the rectangle's first byte; host call: ignored */
    uint64_t    row_pitch, frame_pitch;    /* dev call: as alice_codec_dev_decode_rect's, 0, 0 = packed; host call: ignored */
} alice_codec_rect_item;                   /* 64 bytes */

#define ALICE_RECTS_MAX_ITEMS 1024u

/* Containers on the device (any byte alignment), outputs on the device (any byte alignment, disjoint by the rule above, not
 * overlapping a container).  The stream is drained at most three times: after the header fetches of all distinct
 * containers, at the verdict, and at the end.  Finished on return. */
int alice_codec_dev_decode_rects(const alice_codec_rect_item *items, uint32_t n_items, uint32_t *bad_item, void *hip_stream);
/* Containers in host memory (they may be mapped files) -> one buffer (free with alice_codec_data_free64(ptr,
 * offsets[n_items])), NULL on error; item i is count * h * w * 3 packed bytes at [offsets[i], offsets[i + 1]), in item
 * order.  Per distinct container the 1630-byte header, the three block-length tables and the byte runs of the union of its
 * items' planned blocks go up, once.  offsets (n_items + 1 entries) is left alone on a refusal. */
uint8_t *alice_codec_decode_rects(const alice_codec_rect_item *items, uint32_t n_items, uint64_t *offsets, uint32_t *bad_item);

/* ---- Transcode of a version 2, 3 or 4 chunk to a lower quality or a byte budget, without pixels ----
 * The header stores the quantiser step per channel, a symbol is a function of the quantised coefficient alone and the
 * transform does not depend on the quality, so a chunk at a coarser step is made from the symbols: lane decode, a map of
 * every symbol, histogram and table, lane encode.  No transform runs.  Per channel, with s1 the step in the header and
 * s2 = the step of `quality` (64 - quality * 63 / 100, at least 1; qualities above 100 act as 100):
 *   s2 <= s1: the channel is untouched -- its symbols, its step and its dead zone stay.  A transcode never refuses because the
 *             target is not coarser; (90 -> 89), which share a step, and (60 -> 90) give the source's bytes back.
 *   s2 >  s1: q1 = the coefficient the container's decoder makes of the symbol; m = 0 for q1 = 0, else
 *             sign(q1) * (|q1| * s1 + s1 / 2 + s1 / 2) (integer divisions: the centre of the values the encoder's quantiser
 *             sends to q1; the stored dead zone is not consulted); q2 = the encoder's quantiser of m at step and dead zone
 *             s2; the symbol is the container's of q2, and the channel's step and dead zone become s2.
 * |q2| <= |q1|: no escape appears that was not there.  From a step-1 source (quality 100) m is the coefficient itself, so the
 * result is byte for byte the direct encode at `quality`; otherwise it is close to it, not equal.  The
 * output is an ordinary container: the table is the normalised histogram of the new symbols, as every encoder writes it,
 * and the existing decode calls read it.
 * lane_symbols: 0 keeps the source's; otherwise a power of two in the version's range (the chunk is laned again), else
 * ALICE_ERR_INVALID_DIMENSIONS.  out_version: 0 keeps the version; 3 or 4 for a version 3 or 4 source (only the version byte
 * differs, hence which inverse a decoder runs); every other combination is ALICE_ERR_INVALID_DIMENSIONS.
 * Validation, its order and its codes are alice_codec_decode_frames' for the container (version 1: "no random access"),
 * then lane_symbols, out_version, (budget calls) min_q > max_q and a version 4 result -- a byte budget searches the
 * quality, which version 4 does not have: ALICE_ERR_INVALID_BITSTREAM, ask for out_version = 3 -- all on the host, before a
 * device is looked for.  INTEGRITY: every block is decoded, so every lane end check runs; a directory that does not add up
 * or a failed lane is ALICE_ERR_INVALID_BITSTREAM and nothing is written.  Memory comes from the library's pool; nothing
 * goes through the chain hub. */
/* One container in host memory -> the transcoded container (free with alice_codec_data_free64), NULL on error. */
uint8_t *alice_codec_transcode(const uint8_t *data, uint64_t len, uint8_t quality, uint32_t lane_symbols, uint8_t out_version,
                               uint64_t *out_len);
/* The same at the quality the version 2 / 3 budget rule chooses for max_bytes (alice_codec_encode_split_to_size: q0 from
 * the brackets below, at most ALICE_SPLIT_REFINE_TRIALS exact trials; a trial maps the decoded symbols, which stay on the
 * device, into a scratch copy and runs the table and the count pass).  The bytes are exactly alice_codec_transcode's at
 * *chosen_q; *fits = 0: not even min_q fits, the chunk at min_q is returned. */
uint8_t *alice_codec_transcode_to_size(const uint8_t *data, uint64_t len, uint32_t lane_symbols, uint8_t out_version, uint64_t max_bytes,
                                       uint8_t min_q, uint8_t max_q, uint8_t *chosen_q, uint8_t *fits, uint64_t *out_len);
/* lo[q] <= the size of alice_codec_transcode(data, len, q, lane_symbols, 0) <= hi[q] for the 101 qualities, from one decode,
 * one pass over the symbols and the encoders' fold and cost kernels.  At a step that leaves a channel untouched the
 * channel's bracket is that of its own histogram. */
int alice_codec_predict_transcode_sizes(const uint8_t *data, uint64_t len, uint32_t lane_symbols, uint64_t lo[101], uint64_t hi[101]);
/* n_chunks containers on the device, chunk i of sizes[i] bytes at d_alc + i * alc_stride (any byte alignment), that agree
 * in version, wavelet, shape and lane_symbols (else ALICE_ERR_INVALID_DIMENSIONS; a chunk without pixels likewise) -> chunk
 * i at qualities[i] (NULL: `quality` for all) at d_out + i * out_stride, its size in out_sizes[i].  The output must not
 * overlap the input.  The headers are read back first.  The chunks are worked on in groups (at most 4 GiB of symbols); a
 * chunk that needs more than out_stride bytes is ALICE_ERR_INVALID_BUFFER_SIZE before anything of its group is written, and
 * damage likewise.  Finished on return. */
int alice_codec_dev_transcode(const void *d_alc, uint64_t alc_stride, const uint64_t *sizes, uint32_t n_chunks, uint8_t quality,
                              const uint8_t *qualities, uint32_t lane_symbols, uint8_t out_version, void *d_out, uint64_t out_stride,
                              uint64_t *out_sizes, void *hip_stream);
/* The budget form: chunk i under budgets[i] bytes, by the rule of alice_codec_transcode_to_size.  chosen, fits and out_sizes
 * are written only when the call succeeds. */
int alice_codec_dev_transcode_to_budget(const void *d_alc, uint64_t alc_stride, const uint64_t *sizes, uint32_t n_chunks,
                                        uint32_t lane_symbols, uint8_t out_version, const uint64_t *budgets, uint8_t min_q, uint8_t max_q,
                                        uint8_t *chosen, uint8_t *fits, void *d_out, uint64_t out_stride, uint64_t *out_sizes,
                                        void *hip_stream);
/* Stage call: the map alone.  n symbols (u8; wide != 0: u16 at even addresses) from d_src to d_dst on the device -- the same
 * address (in place) or buffers that do not overlap, any alignment of the element type -- through the map of (step_from,
 * step_to), both in 1..64 (else ALICE_ERR_INVALID_QUANT_STEP); step_to <= step_from copies.  d_hist (256 u32 on the device,
 * or NULL): the histogram of the coded symbols written (wide: min(z, 255)) is ADDED to it.  Finished on return. */
int alice_codec_dev_requant_symbols(const void *d_src, void *d_dst, uint64_t n, int wide, int32_t step_from, int32_t step_to,
                                    void *d_hist, void *hip_stream);

/* ---- banded format (.alc version 5) ----
 * Versions 2 to 4 code a channel with one frequency table; version 5 codes each of the channel's eight wavelet subbands (the
 * octants of its [t'][yy][xx] symbol volume) with a table of its own.  A version 5 chunk names a BASE version 2, 3 or 4 and
 * decodes to exactly the pixels of the base chunk made from the same input, wavelet and quality: colour, padding, lifting,
 * quantiser, symbols and inverse are the base's, and so are the lanes, directories, end checks and (base >= 3) the escape
 * step, applied to every band's symbols in band order.  At the sizes people store (160x96x16 and up) the same pixels take
 * 10 to 45 % fewer bytes; the header is 12 636 bytes and every band carries its own directories, so a thumbnail-sized chunk
 * grows instead: the format is for chunks.
 * lane_symbols: a power of two in [64, 16384] (base 2) or [64, 8192] (bases 3 and 4), 0 for the default.
 * Version 5 has no frame-range, preview, rectangle, batched, budget or transcode call: those keep refusing it with
 * "unsupported version: 5".  The way to them is the repack below, back to the base version byte for byte.
 * Validation of a container is host code, every failure ALICE_ERR_INVALID_BITSTREAM, in the order of DESIGN.md 20.3; lane
 * directories and end checks belong to the decode kernel ("stream j", j = 24 * chunk + 8 * channel + band). */
enum { ALICE_BANDED_HEADER_BYTES = 12636 };
typedef struct AliceBandedInfo {
    uint32_t width, height, frames, lane_symbols;
    uint8_t wavelet, base, reserved[2];
    int32_t quant_step[3], dead_zone[3];
    uint32_t num_symbols[3];
    uint32_t n_blocks[24];      /* channel-major, band k = 4 bt + 2 by + bx ascending inside a channel */
    uint64_t payload_len[24];
} AliceBandedInfo;
/* The most bytes a band payload of n_band symbols takes (0: base, lane_symbols or n_band out of range) */
uint64_t alice_codec_banded_stream_bound(uint64_t n_band, uint32_t lane_symbols, uint8_t base);
/* One chunk in host memory (free the result with alice_codec_data_free64), NULL on error.  Validation order of the encode
 * is alice_codec_encode_split's up to lane_symbols, then base (ALICE_ERR_INVALID_DIMENSIONS), then lane_symbols against the
 * base's range. */
uint8_t *alice_codec_encode_banded(const FrameEncoder *encoder, const uint8_t *rgb, uint64_t rgb_len, uint32_t width,
                                   uint32_t height, uint32_t frames, uint32_t lane_symbols, uint8_t base, uint64_t *out_len);
uint8_t *alice_codec_decode_banded(const uint8_t *data, uint64_t len, uint64_t *out_len);
int alice_codec_banded_info(const uint8_t *data, uint64_t len, AliceBandedInfo *info);
/* device-resident: alice_codec_dev_encode_wide / _dev_decode_wide for version 5 of `base`.  Groups hold at most 2730 chunks
 * (24 jobs each); ALICE_BANDED_HEADER_BYTES + 24 * alice_codec_banded_stream_bound always suffices as out_stride.  The
 * chunks of a decode agree in base, wavelet, shape and lane_symbols; d_alc may have any byte alignment. */
int alice_codec_dev_encode_banded(const void *d_rgb, uint32_t width, uint32_t height, uint32_t frames, uint32_t n_chunks,
                                  uint8_t wavelet_type, uint8_t quality, const uint8_t *qualities, uint32_t lane_symbols,
                                  uint8_t base, void *d_out, uint64_t out_stride, uint64_t *sizes, void *hip_stream);
int alice_codec_dev_decode_banded(const void *d_alc, uint64_t alc_stride, const uint64_t *sizes, uint32_t n_chunks,
                                  void *d_rgb_out, void *hip_stream);
/* Repack without pixels: a version 2, 3 or 4 chunk -> the version 5 chunk of that base (lane decode of every block, band
 * histograms, band encode), and back (band decode, a 256-bin count of each channel, the base's encode).  No transform runs.
 * lane_symbols: 0 keeps the source's.  alice_codec_from_banded(alice_codec_to_banded(x)) == x and alice_codec_to_banded of a
 * base encode == alice_codec_encode_banded of the same input, byte for byte.  Every end check of the source runs; damage is
 * ALICE_ERR_INVALID_BITSTREAM and nothing is written. */
uint8_t *alice_codec_to_banded(const uint8_t *data, uint64_t len, uint32_t lane_symbols, uint64_t *out_len);
uint8_t *alice_codec_from_banded(const uint8_t *data, uint64_t len, uint32_t lane_symbols, uint64_t *out_len);
/* The same on the device, shaped as alice_codec_dev_transcode without the quality and version arguments. */
int alice_codec_dev_to_banded(const void *d_alc, uint64_t alc_stride, const uint64_t *sizes, uint32_t n_chunks, uint32_t lane_symbols,
                              void *d_out, uint64_t out_stride, uint64_t *out_sizes, void *hip_stream);
int alice_codec_dev_from_banded(const void *d_alc, uint64_t alc_stride, const uint64_t *sizes, uint32_t n_chunks, uint32_t lane_symbols,
                                void *d_out, uint64_t out_stride, uint64_t *out_sizes, void *hip_stream);
/* Stage call: the symbols [3][pf][ph][pw] of one chunk's padded volume (u8; wide != 0: u16 at an even address) -> d_hist,
 * 3 x 8 x 256 u32 on the device (overwritten): the histogram of every band, wide: of min(z, 255).  Finished on return. */
int alice_codec_dev_band_histograms(const void *d_symbols, uint32_t width, uint32_t height, uint32_t frames, int wide,
                                    void *d_hist, void *hip_stream);
/* Random access into a version 5 chunk: frames [first, first + count) at full size, and their
 * half-size preview, bit for bit what alice_codec_decode_frames / alice_codec_decode_preview give on
 * alice_codec_from_banded(data).  Only the blocks that hold coefficient planes of the window (alice_codec_frames_window) are
 * entropy-decoded: of all eight bands for the frames, of bands 0 and 4 alone for the preview; the host calls upload the
 * header, the 24 block-length tables and those blocks (data may be a mapped file).  Output sizes: width * height * count * 3
 * bytes, and qw * qh * count * 3 bytes with alice_codec_preview_dims' qw and qh.  Validation: null arguments, the header in
 * the order of DESIGN.md 20.3 (another version: "unsupported version: N (expected 5)"), then the range as
 * alice_codec_decode_frames has it; a chunk without pixels refuses every range.  Every block-length table is checked, the end
 * checks cover the decoded blocks ("stream j", j = 8 * channel + band); a refused call writes nothing of its output.  The
 * device calls read the header back first, take d_alc at any byte alignment and return after their work has drained. */
uint8_t *alice_codec_decode_banded_frames(const uint8_t *data, uint64_t len, uint32_t first, uint32_t count, uint64_t *out_len);
int alice_codec_dev_decode_banded_frames(const void *d_alc, uint64_t len, uint32_t first, uint32_t count, void *d_rgb_out,
                                         void *hip_stream);
uint8_t *alice_codec_decode_banded_preview(const uint8_t *data, uint64_t len, uint32_t first, uint32_t count, uint64_t *out_len);
int alice_codec_dev_decode_banded_preview(const void *d_alc, uint64_t len, uint32_t first, uint32_t count, void *d_rgb_out,
                                          void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* ALICE_CODEC_H */
