//! MI355X back end for ALICE-Codec's hot path, as the reference's own Rust API.
//!
//! NOT COMPILED, NOT TESTED: the image this repository is built in has no Rust toolchain (no `cargo`, no `rustc`),
//! and neither has the GPU box.  What is verified is the C ABI underneath (`include/alice_codec.h`, exercised through
//! ctypes by `tests/` and through the C++ mirror `include/alice_codec.hpp` by `tests/cpp/test_cpp_mirror.cpp`).  This
//! file is the binding a maintainer of the reference crate would add -- `src/gpu_backend.rs` behind a cargo feature --
//! and states, type by type, which reference item each wrapper replaces.  Names, argument order, argument meaning and
//! error variants are the reference's:
//!
//!   FrameEncoder::{new, with_wavelet, encode}          src/pipeline.rs:347, 356, 377
//!   FrameDecoder::{new, decode}                        src/pipeline.rs:524, 537
//!   EncodedChunk::{compressed_size, to_bytes, from_bytes}   src/pipeline.rs:190, 200, 235
//!   Wavelet3D::{new, cdf97, cdf53, forward, inverse}   src/wavelet.rs:366, 372, 378, 392, 441
//!   Wavelet2D::{cdf97, cdf53, forward, inverse}        src/wavelet.rs:278, 284, 292, 319
//!   FastQuantizer::{new, with_dead_zone, quantize, dequantize, quantize_buffer, dequantize_buffer,
//!                   quantize_buffer_simd, step, dead_zone}   src/quant.rs:190-347
//!   to_symbols / from_symbols / build_histogram        src/quant.rs:547, 572, 594
//!   FrequencyTable::{from_histogram, uniform, get_symbol, len, is_empty}   src/rans.rs:102, 158, 194, 209, 216 (any n <= 256)
//!   RansEncoder::{new, with_capacity, encode, encode_symbols, finish}       src/rans.rs:249, 258, 269, 288, 298
//!   RansDecoder::{new, decode, decode_n, is_empty}     src/rans.rs:330, 351, 375, 385
//!   quantize_subband / dequantize_subband              src/quant.rs:518, 531
//!   encode_many / decode_many (chunk driver, optionally over several GPUs)   src/pipeline.rs:461-497
//!
//! Every call computes on the GPU; without an MI355X the library returns an error (`CodecError::Device`), it never
//! falls back to the CPU.  Results are byte-identical to the reference's (this repository's parity tests), with one
//! documented divergence: encoding a symbol whose table frequency wrapped to 0 returns `CodecError::ReferenceDiverges`
//! where the reference never returns (src/rans.rs:275-283).
#![allow(dead_code)]

use std::os::raw::{c_char, c_int};

// ---------------------------------------------------------------------------------------------------------------
// the C ABI (include/alice_codec.h); opaque handles
// ---------------------------------------------------------------------------------------------------------------

#[repr(C)] pub struct RawEncoder { _p: [u8; 0] }
#[repr(C)] pub struct RawChunk { _p: [u8; 0] }
#[repr(C)] pub struct RawFastQuantizer { _p: [u8; 0] }
#[repr(C)] pub struct RawRansEncoder { _p: [u8; 0] }
#[repr(C)] pub struct RawRansDecoder { _p: [u8; 0] }

#[link(name = "alice_codec")]
extern "C" {
    fn alice_codec_last_error() -> c_int;
    fn alice_codec_last_error_message() -> *const c_char;

    fn alice_codec_encoder_create_ex(quality: u8, wavelet_type: u8) -> *mut RawEncoder;
    fn alice_codec_encoder_destroy(p: *mut RawEncoder);
    fn alice_codec_encode64(e: *const RawEncoder, rgb: *const u8, rgb_len: u64, w: u32, h: u32, f: u32) -> *mut RawChunk;
    fn alice_codec_decode64(c: *const RawChunk, out_len: *mut u64) -> *mut u8;
    fn alice_codec_chunk_destroy(c: *mut RawChunk);
    fn alice_codec_chunk_to_bytes64(c: *const RawChunk, out_len: *mut u64) -> *mut u8;
    fn alice_codec_chunk_from_bytes64(data: *const u8, len: u64) -> *mut RawChunk;
    fn alice_codec_chunk_width(c: *const RawChunk) -> u32;
    fn alice_codec_chunk_height(c: *const RawChunk) -> u32;
    fn alice_codec_chunk_frames(c: *const RawChunk) -> u32;
    fn alice_codec_chunk_wavelet(c: *const RawChunk) -> u8;
    fn alice_codec_chunk_compressed_size(c: *const RawChunk) -> u64;
    fn alice_codec_data_free64(p: *mut u8, len: u64);

    fn alice_codec_wavelet2d_forward(wavelet: u8, image: *mut i32, w: u64, h: u64) -> c_int;
    fn alice_codec_wavelet2d_inverse(wavelet: u8, image: *mut i32, w: u64, h: u64) -> c_int;
    fn alice_codec_wavelet3d_forward(wavelet: u8, volume: *mut i32, w: u64, h: u64, d: u64) -> c_int;
    fn alice_codec_wavelet3d_inverse(wavelet: u8, volume: *mut i32, w: u64, h: u64, d: u64) -> c_int;

    fn alice_codec_fastquant_new(step: i32) -> *mut RawFastQuantizer;
    fn alice_codec_fastquant_with_dead_zone(step: i32, dead_zone: i32) -> *mut RawFastQuantizer;
    fn alice_codec_fastquant_destroy(q: *mut RawFastQuantizer);
    fn alice_codec_fastquant_quantize_buffer(q: *const RawFastQuantizer, input: *const i32, n_in: u64, out: *mut i32, n_out: u64) -> c_int;
    fn alice_codec_fastquant_dequantize_buffer(q: *const RawFastQuantizer, input: *const i32, n_in: u64, out: *mut i32, n_out: u64) -> c_int;

    fn alice_codec_to_symbols(coeffs: *const i32, n: u64, symbols: *mut u8, n_out: u64) -> c_int;
    fn alice_codec_from_symbols(symbols: *const u8, n: u64, coeffs: *mut i32, n_out: u64) -> c_int;
    fn alice_codec_build_histogram(symbols: *const u8, n: u64, hist: *mut u32) -> c_int;
    fn alice_codec_freq_table_from_histogram(hist: *const u32, cum_freq: *mut u16, freq: *mut u16) -> c_int;
    fn alice_codec_freq_table_from_histogram_n(hist: *const u32, n_symbols: u32, cum_freq: *mut u16, freq: *mut u16) -> c_int;
    fn alice_codec_rans_encode(symbols: *const u8, n: u64, cum_freq: *const u16, freq: *const u16, out_len: *mut u64) -> *mut u8;
    fn alice_codec_rans_decode(bytes: *const u8, len: u64, cum_freq: *const u16, freq: *const u16, n: u64, symbols: *mut u8) -> c_int;
    fn alice_codec_rans_encoder_new() -> *mut RawRansEncoder;
    fn alice_codec_rans_encoder_destroy(e: *mut RawRansEncoder);
    fn alice_codec_rans_encoder_encode(e: *mut RawRansEncoder, cum_freq: u16, freq: u16) -> c_int;
    fn alice_codec_rans_encoder_encode_symbols(e: *mut RawRansEncoder, symbols: *const u8, n: u64, cum_freq: *const u16, freq: *const u16) -> c_int;
    fn alice_codec_rans_encoder_finish(e: *mut RawRansEncoder, out_len: *mut u64) -> *mut u8;
    fn alice_codec_rans_decoder_new(data: *const u8, len: u64) -> *mut RawRansDecoder;
    fn alice_codec_rans_decoder_destroy(d: *mut RawRansDecoder);
    fn alice_codec_rans_decoder_decode_n(d: *mut RawRansDecoder, n: u64, cum_freq: *const u16, freq: *const u16, symbols: *mut u8) -> c_int;
    fn alice_codec_rans_decoder_is_empty(d: *const RawRansDecoder) -> c_int;
    fn alice_codec_quantize_subband(step: i32, dead_zone: i32, coeffs: *const i32, n: u64, out: *mut i32, n_out: u64) -> c_int;
    fn alice_codec_dequantize_subband(step: i32, coeffs: *const i32, n: u64, out: *mut i32, n_out: u64) -> c_int;
    fn alice_codec_encode_many(e: *const RawEncoder, rgb: *const u8, rgb_len: u64, w: u32, h: u32, f: u32, n_chunks: u32, out: *mut *mut RawChunk) -> c_int;
    fn alice_codec_decode_many(chunks: *const *const RawChunk, n_chunks: u32, rgb_out: *mut u8, rgb_out_len: u64) -> c_int;
    fn alice_codec_encode_many_devices(e: *const RawEncoder, rgb: *const u8, rgb_len: u64, w: u32, h: u32, f: u32, n_chunks: u32,
                                       devices: *const c_int, n_devices: u32, out: *mut *mut RawChunk) -> c_int;
    fn alice_codec_decode_many_devices(chunks: *const *const RawChunk, n_chunks: u32, devices: *const c_int, n_devices: u32,
                                       rgb_out: *mut u8, rgb_out_len: u64) -> c_int;
    fn alice_codec_predict_sizes(wavelet: u8, rgb: *const u8, rgb_len: u64, w: u32, h: u32, f: u32, lo: *mut u64, hi: *mut u64,
                                 status: *mut u8) -> c_int;
    fn alice_codec_encode_to_size(wavelet: u8, rgb: *const u8, rgb_len: u64, w: u32, h: u32, f: u32, max_bytes: u64, min_q: u8,
                                  max_q: u8, chosen_q: *mut u8, fits: *mut u8) -> *mut RawChunk;
}

// ---------------------------------------------------------------------------------------------------------------
// errors: CodecError (src/error.rs:12-23) + the library-side conditions
// ---------------------------------------------------------------------------------------------------------------

#[derive(Debug, Clone, PartialEq, Eq)]
pub enum CodecError {
    InvalidBufferSize { expected: usize, got: usize },
    InvalidDimensions { width: u32, height: u32 },
    DimensionOverflow,
    InvalidBitstream(String),
    InvalidQuantStep(i32),
    /// the reference would spin forever / divide by zero on this input (src/rans.rs:275-283)
    ReferenceDiverges,
    /// no usable MI355X, out of device memory, or a HIP runtime failure; the message is the library's
    Device(String),
}

fn last_error(expected: usize, got: usize, width: u32, height: u32, step: i32) -> CodecError {
    // ALICE_ERR_* (include/alice_codec.h): 1..=5 are the reference's variants in declaration order
    let msg = unsafe {
        let p = alice_codec_last_error_message();
        if p.is_null() { String::new() } else { std::ffi::CStr::from_ptr(p).to_string_lossy().into_owned() }
    };
    match unsafe { alice_codec_last_error() } {
        1 => CodecError::InvalidBufferSize { expected, got },
        2 => CodecError::InvalidDimensions { width, height },
        3 => CodecError::DimensionOverflow,
        4 => CodecError::InvalidBitstream(msg),
        5 => CodecError::InvalidQuantStep(step),
        6 => CodecError::ReferenceDiverges,
        _ => CodecError::Device(msg),
    }
}

/// 0 -> Ok, anything else -> the calling thread's last error (expected / got fill InvalidBufferSize)
fn check(rc: c_int, expected: usize, got: usize) -> Result<(), CodecError> {
    if rc == 0 { Ok(()) } else { Err(last_error(expected, got, 0, 0, 0)) }
}

unsafe fn take(p: *mut u8, n: u64) -> Vec<u8> {
    let v = std::slice::from_raw_parts(p, n as usize).to_vec();
    alice_codec_data_free64(p, n);
    v
}

// ---------------------------------------------------------------------------------------------------------------
// pipeline: src/pipeline.rs
// ---------------------------------------------------------------------------------------------------------------

/// src/pipeline.rs:34-41 (the discriminants are the `.alc` wavelet byte, :46-62)
#[derive(Debug, Clone, Copy, PartialEq, Eq)]
#[repr(u8)]
pub enum WaveletType { Cdf53 = 0, Cdf97 = 1, Haar = 2 }

/// src/pipeline.rs:172-185.  Owns the library's chunk handle; `to_bytes` is the `.alc` serialisation.
pub struct EncodedChunk { raw: *mut RawChunk }
unsafe impl Send for EncodedChunk {}
unsafe impl Sync for EncodedChunk {}   // immutable after creation, as src/pipeline.rs:635-644 asserts

impl EncodedChunk {
    pub fn width(&self) -> u32 { unsafe { alice_codec_chunk_width(self.raw) } }
    pub fn height(&self) -> u32 { unsafe { alice_codec_chunk_height(self.raw) } }
    pub fn frames(&self) -> u32 { unsafe { alice_codec_chunk_frames(self.raw) } }
    pub fn wavelet_type(&self) -> WaveletType {
        match unsafe { alice_codec_chunk_wavelet(self.raw) } { 1 => WaveletType::Cdf97, 2 => WaveletType::Haar, _ => WaveletType::Cdf53 }
    }
    /// src/pipeline.rs:190
    pub fn compressed_size(&self) -> usize { unsafe { alice_codec_chunk_compressed_size(self.raw) as usize } }
    /// src/pipeline.rs:200
    pub fn to_bytes(&self) -> Vec<u8> {
        let mut n = 0u64;
        unsafe { let p = alice_codec_chunk_to_bytes64(self.raw, &mut n); if p.is_null() { Vec::new() } else { take(p, n) } }
    }
    /// src/pipeline.rs:235 (validation and messages: codec.hip parse_alc_header / chunk_from_bytes)
    pub fn from_bytes(data: &[u8]) -> Result<Self, CodecError> {
        let raw = unsafe { alice_codec_chunk_from_bytes64(data.as_ptr(), data.len() as u64) };
        if raw.is_null() { Err(last_error(0, data.len(), 0, 0, 0)) } else { Ok(Self { raw }) }
    }
}
impl Drop for EncodedChunk { fn drop(&mut self) { unsafe { alice_codec_chunk_destroy(self.raw) } } }

// ---------------------------------------------------------------------------------------------------------------
// rate control on the GPU (an extension: the reference's own RateController / estimate_quality stay the reference's)
// ---------------------------------------------------------------------------------------------------------------

/// status of a quality's prediction (ALICE_RATE_*)
pub const RATE_BOUNDED: u8 = 0;
pub const RATE_UNBOUNDED: u8 = 1;
pub const RATE_DIVERGES: u8 = 2;

/// The guaranteed .alc length bracket `lo[q] <= len <= hi[q]` of a chunk at every quality q = 0..=100 (where
/// `status[q] == RATE_BOUNDED`), from one forward transform on the GPU.
pub struct SizePrediction { pub lo: [u64; 101], pub hi: [u64; 101], pub status: [u8; 101] }

pub fn predict_sizes(rgb_frames: &[u8], width: u32, height: u32, frames: u32, wavelet_type: WaveletType)
    -> Result<SizePrediction, CodecError> {
    let mut p = SizePrediction { lo: [0; 101], hi: [0; 101], status: [0; 101] };
    let rc = unsafe {
        alice_codec_predict_sizes(wavelet_type as u8, rgb_frames.as_ptr(), rgb_frames.len() as u64, width, height, frames,
                                  p.lo.as_mut_ptr(), p.hi.as_mut_ptr(), p.status.as_mut_ptr())
    };
    let expected = (width as usize).saturating_mul(height as usize).saturating_mul(frames as usize).saturating_mul(3);
    check(rc, expected, rgb_frames.len()).map(|_| p)
}

/// Encodes once, at the highest quality in `min_quality..=max_quality` whose predicted length fits `max_bytes`:
/// (chunk, chosen quality, fits).  When none fits, the chunk is encoded at `min_quality` and `fits` is false.
pub fn encode_to_size(rgb_frames: &[u8], width: u32, height: u32, frames: u32, max_bytes: u64, wavelet_type: WaveletType,
                      min_quality: u8, max_quality: u8) -> Result<(EncodedChunk, u8, bool), CodecError> {
    let (mut q, mut fits) = (0u8, 0u8);
    let raw = unsafe {
        alice_codec_encode_to_size(wavelet_type as u8, rgb_frames.as_ptr(), rgb_frames.len() as u64, width, height, frames, max_bytes,
                                   min_quality, max_quality, &mut q, &mut fits)
    };
    if raw.is_null() {
        let expected = (width as usize).saturating_mul(height as usize).saturating_mul(frames as usize).saturating_mul(3);
        return Err(last_error(expected, rgb_frames.len(), width, height, 0));
    }
    Ok((EncodedChunk { raw }, q, fits != 0))
}

/// src/pipeline.rs:335-340
pub struct FrameEncoder { quality: u8, wavelet_type: WaveletType }

impl FrameEncoder {
    /// src/pipeline.rs:347: CDF 5/3
    pub const fn new(quality: u8) -> Self { Self { quality, wavelet_type: WaveletType::Cdf53 } }
    /// src/pipeline.rs:356
    pub const fn with_wavelet(quality: u8, wavelet_type: WaveletType) -> Self { Self { quality, wavelet_type } }
    /// src/pipeline.rs:377.  `rgb_frames`: interleaved RGB, frame-major, `width * height * frames * 3` bytes.
    pub fn encode(&self, rgb_frames: &[u8], width: u32, height: u32, frames: u32) -> Result<EncodedChunk, CodecError> {
        unsafe {
            let e = alice_codec_encoder_create_ex(self.quality, self.wavelet_type as u8);
            let raw = alice_codec_encode64(e, rgb_frames.as_ptr(), rgb_frames.len() as u64, width, height, frames);
            alice_codec_encoder_destroy(e);
            if raw.is_null() {
                let expected = (width as usize).saturating_mul(height as usize).saturating_mul(frames as usize).saturating_mul(3);
                return Err(last_error(expected, rgb_frames.len(), width, height, 0));
            }
            Ok(EncodedChunk { raw })
        }
    }
}

/// src/pipeline.rs:519
pub struct FrameDecoder;

impl FrameDecoder {
    /// src/pipeline.rs:524
    pub const fn new() -> Self { Self }
    /// src/pipeline.rs:537
    pub fn decode(&self, chunk: &EncodedChunk) -> Result<Vec<u8>, CodecError> {
        let mut n = 0u64;
        unsafe {
            let p = alice_codec_decode64(chunk.raw, &mut n);
            if p.is_null() { Err(last_error(0, 0, chunk.width(), chunk.height(), 0)) } else { Ok(take(p, n)) }
        }
    }
}
impl Default for FrameDecoder { fn default() -> Self { Self::new() } }

// ---------------------------------------------------------------------------------------------------------------
// wavelets: src/wavelet.rs.  The filter is carried as the wavelet byte; the lifting itself runs on the GPU.
// ---------------------------------------------------------------------------------------------------------------

/// src/wavelet.rs:47 -- here only the choice of filter (coefficient lists: csrc/common.h lift_steps)
#[derive(Debug, Clone, Copy, PartialEq, Eq)]
pub struct Wavelet1D { kind: WaveletType }
impl Wavelet1D {
    pub fn cdf97() -> Self { Self { kind: WaveletType::Cdf97 } }   // src/wavelet.rs:66
    pub fn haar() -> Self { Self { kind: WaveletType::Haar } }     // :96
    pub fn cdf53() -> Self { Self { kind: WaveletType::Cdf53 } }   // :113
    /// src/wavelet.rs:133 (no-op below two samples; an odd tail sample is dropped, :225-232)
    pub fn forward(&self, signal: &mut [i32]) { Wavelet3D::new(*self).forward(signal, signal.len(), 1, 1) }
    /// src/wavelet.rs:157
    pub fn inverse(&self, signal: &mut [i32]) { Wavelet3D::new(*self).inverse(signal, signal.len(), 1, 1) }
}

/// src/wavelet.rs:265
pub struct Wavelet2D { wavelet_1d: Wavelet1D }
impl Wavelet2D {
    pub const fn new(wavelet_1d: Wavelet1D) -> Self { Self { wavelet_1d } }       // :272
    pub fn cdf97() -> Self { Self::new(Wavelet1D::cdf97()) }                        // :278
    pub fn cdf53() -> Self { Self::new(Wavelet1D::cdf53()) }                        // :284
    /// src/wavelet.rs:292 (rows, then columns)
    pub fn forward(&self, image: &mut [i32], width: usize, height: usize) {
        assert!(image.len() >= width * height);
        unsafe { alice_codec_wavelet2d_forward(self.wavelet_1d.kind as u8, image.as_mut_ptr(), width as u64, height as u64); }
    }
    /// src/wavelet.rs:319 (columns, then rows)
    pub fn inverse(&self, image: &mut [i32], width: usize, height: usize) {
        assert!(image.len() >= width * height);
        unsafe { alice_codec_wavelet2d_inverse(self.wavelet_1d.kind as u8, image.as_mut_ptr(), width as u64, height as u64); }
    }
}

/// src/wavelet.rs:359
pub struct Wavelet3D { wavelet_1d: Wavelet1D }
impl Wavelet3D {
    pub const fn new(wavelet_1d: Wavelet1D) -> Self { Self { wavelet_1d } }       // :366
    pub fn cdf97() -> Self { Self::new(Wavelet1D::cdf97()) }                        // :372
    pub fn cdf53() -> Self { Self::new(Wavelet1D::cdf53()) }                        // :378
    /// src/wavelet.rs:392: rows and columns of every frame, then the temporal vector of every pixel; one level;
    /// `volume[t * width * height + y * width + x]`, in place, any i32 values (wrapping sums, 64-bit products).
    pub fn forward(&self, volume: &mut [i32], width: usize, height: usize, depth: usize) {
        assert!(volume.len() >= width * height * depth);
        unsafe { alice_codec_wavelet3d_forward(self.wavelet_1d.kind as u8, volume.as_mut_ptr(), width as u64, height as u64, depth as u64); }
    }
    /// src/wavelet.rs:441: temporal, then columns, then rows (negated coefficients, rounding not mirrored, :167-174)
    pub fn inverse(&self, volume: &mut [i32], width: usize, height: usize, depth: usize) {
        assert!(volume.len() >= width * height * depth);
        unsafe { alice_codec_wavelet3d_inverse(self.wavelet_1d.kind as u8, volume.as_mut_ptr(), width as u64, height as u64, depth as u64); }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// quantiser and symbols: src/quant.rs
// ---------------------------------------------------------------------------------------------------------------

/// src/quant.rs:171.  The scalar `quantize` / `dequantize` are the reference's own arithmetic (they are two lines and
/// gain nothing from a device round trip); the buffer forms run on the GPU.
pub struct FastQuantizer { raw: *mut RawFastQuantizer, step: i32, dead_zone: i32, reciprocal: u64, shift: u32 }
unsafe impl Send for FastQuantizer {}
unsafe impl Sync for FastQuantizer {}

impl FastQuantizer {
    /// src/quant.rs:190: `step <= 0` is `InvalidQuantStep`
    pub fn new(step: i32) -> Result<Self, CodecError> { Self::with_dead_zone(step, step) }
    /// src/quant.rs:224
    pub fn with_dead_zone(step: i32, dead_zone: i32) -> Result<Self, CodecError> {
        if step <= 0 { return Err(CodecError::InvalidQuantStep(step)); }
        let raw = unsafe { alice_codec_fastquant_with_dead_zone(step, dead_zone) };
        if raw.is_null() { return Err(last_error(0, 0, 0, 0, step)); }
        // src/quant.rs:200-216: reciprocal = ceil(2^(32 + bits(step)) / step)
        let extra = 32 - (step as u32).leading_zeros();
        let shift = 32 + extra;
        let reciprocal = (((1u128 << shift) + step as u128 - 1) / step as u128) as u64;
        Ok(Self { raw, step, dead_zone, reciprocal, shift })
    }
    /// src/quant.rs:243
    pub const fn quantize(&self, value: i32) -> i32 {
        let abs_val = value.unsigned_abs();
        if abs_val < self.dead_zone as u32 { return 0; }
        let adjusted = abs_val - (self.dead_zone as u32) / 2;
        let q = ((adjusted as u64).wrapping_mul(self.reciprocal) >> self.shift) as i32;   // fast_div, :232-236
        if value < 0 { -q } else { q }
    }
    /// src/quant.rs:269
    pub const fn dequantize(&self, qvalue: i32) -> i32 { qvalue.wrapping_mul(self.step) }
    /// src/quant.rs:282: `output.len() < input.len()` is `InvalidBufferSize`
    pub fn quantize_buffer(&self, input: &[i32], output: &mut [i32]) -> Result<(), CodecError> {
        let rc = unsafe { alice_codec_fastquant_quantize_buffer(self.raw, input.as_ptr(), input.len() as u64, output.as_mut_ptr(), output.len() as u64) };
        if rc == 0 { Ok(()) } else { Err(last_error(input.len(), output.len(), 0, 0, self.step)) }
    }
    /// src/quant.rs:300
    pub fn dequantize_buffer(&self, input: &[i32], output: &mut [i32]) -> Result<(), CodecError> {
        let rc = unsafe { alice_codec_fastquant_dequantize_buffer(self.raw, input.as_ptr(), input.len() as u64, output.as_mut_ptr(), output.len() as u64) };
        if rc == 0 { Ok(()) } else { Err(last_error(input.len(), output.len(), 0, 0, self.step)) }
    }
    /// src/quant.rs:322: the reference's AVX2 entry point; same results as `quantize_buffer`, panics on a short output
    pub fn quantize_buffer_simd(&self, input: &[i32], output: &mut [i32]) {
        self.quantize_buffer(input, output).expect("output buffer too small");
    }
    pub const fn step(&self) -> i32 { self.step }             // src/quant.rs:337
    pub const fn dead_zone(&self) -> i32 { self.dead_zone }   // src/quant.rs:344
}
impl Drop for FastQuantizer { fn drop(&mut self) { unsafe { alice_codec_fastquant_destroy(self.raw) } } }

/// src/quant.rs:547
pub fn to_symbols(coeffs: &[i32], symbols: &mut [u8]) -> Result<(), CodecError> {
    let rc = unsafe { alice_codec_to_symbols(coeffs.as_ptr(), coeffs.len() as u64, symbols.as_mut_ptr(), symbols.len() as u64) };
    if rc == 0 { Ok(()) } else { Err(last_error(coeffs.len(), symbols.len(), 0, 0, 0)) }
}
/// src/quant.rs:572
pub fn from_symbols(symbols: &[u8], coeffs: &mut [i32]) -> Result<(), CodecError> {
    let rc = unsafe { alice_codec_from_symbols(symbols.as_ptr(), symbols.len() as u64, coeffs.as_mut_ptr(), coeffs.len() as u64) };
    if rc == 0 { Ok(()) } else { Err(last_error(symbols.len(), coeffs.len(), 0, 0, 0)) }
}
/// src/quant.rs:594
pub fn build_histogram(symbols: &[u8]) -> [u32; 256] {
    let mut h = [0u32; 256];
    unsafe { alice_codec_build_histogram(symbols.as_ptr(), symbols.len() as u64, h.as_mut_ptr()); }
    h
}

// ---------------------------------------------------------------------------------------------------------------
// entropy coder: src/rans.rs
// ---------------------------------------------------------------------------------------------------------------

/// src/rans.rs:59
#[derive(Debug, Clone, Copy, PartialEq, Eq)]
pub struct RansSymbol { pub cum_freq: u16, pub freq: u16 }
impl RansSymbol { pub const fn new(cum_freq: u16, freq: u16) -> Self { Self { cum_freq, freq } } }   // :69

/// src/rans.rs:85.  n symbols, 1 <= n <= 256 (the coders address symbols as u8); the arrays always hold 256 entries,
/// those from n on are (0, 0).
pub struct FrequencyTable { cum_freq: [u16; 256], freq: [u16; 256], n_symbols: usize }
impl FrequencyTable {
    /// src/rans.rs:102 (freq 1 for unused symbols, wrapping fix on the last symbol, uniform fallback when empty); any
    /// slice length the u8 symbol API can address.  Panics where the reference panics (an empty slice divides by zero in
    /// `uniform(0)`, :159) and for more than 256 symbols, which the GPU path does not carry.
    pub fn from_histogram(histogram: &[u32]) -> Self {
        let mut t = Self { cum_freq: [0; 256], freq: [0; 256], n_symbols: histogram.len() };
        let rc = unsafe { alice_codec_freq_table_from_histogram_n(histogram.as_ptr(), histogram.len() as u32, t.cum_freq.as_mut_ptr(), t.freq.as_mut_ptr()) };
        assert!(rc == 0, "FrequencyTable::from_histogram: {:?}", last_error(0, 0, 0, 0, 0));
        t
    }
    /// src/rans.rs:158
    pub fn uniform(n_symbols: usize) -> Self { Self::from_histogram(&vec![0u32; n_symbols]) }   // total == 0 -> uniform(n) (:106-109)
    pub fn get_symbol(&self, sym: u8) -> RansSymbol {                                             // :194 (panics out of range, as the Vec index does)
        assert!((sym as usize) < self.n_symbols);
        RansSymbol::new(self.cum_freq[sym as usize], self.freq[sym as usize])
    }
    pub const fn len(&self) -> usize { self.n_symbols }          // :209
    pub const fn is_empty(&self) -> bool { self.n_symbols == 0 } // :216
}

/// src/rans.rs:238: an encoder object that lives across calls.  Every call runs one chain on the device from the object's
/// current state (`encode_symbols` s1 then s2 leaves the stream of one call on s2 || s1, :288-294; `encode` takes the
/// (cum_freq, freq) pair itself, :269-285); the bytes a call emits come back to the host, `finish` prepends the state.
/// The methods return Results because of the one documented divergence (a frequency-0 symbol, :275-283: the reference
/// never returns).
pub struct RansEncoder { raw: *mut RawRansEncoder }
impl RansEncoder {
    pub fn new() -> Self { Self { raw: unsafe { alice_codec_rans_encoder_new() } } }             // :249
    pub fn with_capacity(_capacity: usize) -> Self { Self::new() }                               // :258 (a hint there too)
    /// src/rans.rs:269
    pub fn encode(&mut self, sym: &RansSymbol) -> Result<(), CodecError> {
        check(unsafe { alice_codec_rans_encoder_encode(self.raw, sym.cum_freq, sym.freq) }, 0, 0)
    }
    /// src/rans.rs:288
    pub fn encode_symbols(&mut self, symbols: &[u8], table: &FrequencyTable) -> Result<(), CodecError> {
        if symbols.is_empty() { return Ok(()); }
        check(unsafe { alice_codec_rans_encoder_encode_symbols(self.raw, symbols.as_ptr(), symbols.len() as u64, table.cum_freq.as_ptr(), table.freq.as_ptr()) }, 0, 0)
    }
    /// src/rans.rs:298: the stream starts with the final state, big-endian
    pub fn finish(mut self) -> Result<Vec<u8>, CodecError> {
        let mut n = 0u64;
        let raw = std::mem::replace(&mut self.raw, std::ptr::null_mut());
        unsafe {
            let p = alice_codec_rans_encoder_finish(raw, &mut n);   // consumes the handle
            if p.is_null() { Err(last_error(0, 0, 0, 0, 0)) } else { Ok(take(p, n)) }
        }
    }
}
impl Drop for RansEncoder { fn drop(&mut self) { if !self.raw.is_null() { unsafe { alice_codec_rans_encoder_destroy(self.raw) } } } }
impl Default for RansEncoder { fn default() -> Self { Self::new() } }

/// src/rans.rs:321: a decoder object; `decode` / `decode_n` continue from the current state and position (the library
/// keeps a copy of the input, so the lifetime parameter of the reference type only documents the borrow)
pub struct RansDecoder<'a> { raw: *mut RawRansDecoder, _input: std::marker::PhantomData<&'a [u8]> }
impl<'a> RansDecoder<'a> {
    pub fn new(input: &'a [u8]) -> Self {   // :330
        Self { raw: unsafe { alice_codec_rans_decoder_new(input.as_ptr(), input.len() as u64) }, _input: std::marker::PhantomData }
    }
    /// src/rans.rs:351
    pub fn decode(&mut self, table: &FrequencyTable) -> u8 { self.decode_n(1, table)[0] }
    /// src/rans.rs:375, including the behaviour on short, truncated and desynchronised streams (:341-347, 365-368)
    pub fn decode_n(&mut self, n: usize, table: &FrequencyTable) -> Vec<u8> {
        let mut out = vec![0u8; n];
        unsafe { alice_codec_rans_decoder_decode_n(self.raw, n as u64, table.cum_freq.as_ptr(), table.freq.as_ptr(), out.as_mut_ptr()); }
        out
    }
    /// src/rans.rs:385
    pub fn is_empty(&self) -> bool { unsafe { alice_codec_rans_decoder_is_empty(self.raw) != 0 } }
}
impl<'a> Drop for RansDecoder<'a> { fn drop(&mut self) { unsafe { alice_codec_rans_decoder_destroy(self.raw) } } }

/// src/quant.rs:518 / :531: a sub-band's coefficients through a Quantizer (step, dead zone)
pub fn quantize_subband(coeffs: &[i32], step: i32, dead_zone: i32, output: &mut [i32]) -> Result<(), CodecError> {
    check(unsafe { alice_codec_quantize_subband(step, dead_zone, coeffs.as_ptr(), coeffs.len() as u64, output.as_mut_ptr(), output.len() as u64) }, coeffs.len(), output.len())
}
pub fn dequantize_subband(coeffs: &[i32], step: i32, output: &mut [i32]) -> Result<(), CodecError> {
    check(unsafe { alice_codec_dequantize_subband(step, coeffs.as_ptr(), coeffs.len() as u64, output.as_mut_ptr(), output.len() as u64) }, coeffs.len(), output.len())
}

/// The chunk driver over several GPUs of the node (src/pipeline.rs:461-497: 64-frame chunks are independent): chunk k
/// runs on devices[k % devices.len()], one host thread per entry inside the library; an empty list = the calling
/// thread's device.  Byte-identical to `chunks.len()` calls of `FrameEncoder::encode`.
pub fn encode_many(encoder: &FrameEncoder, rgb_chunks: &[u8], width: u32, height: u32, frames: u32, n_chunks: u32, devices: &[i32])
                   -> Result<Vec<EncodedChunk>, CodecError> {
    let raw_enc = unsafe { alice_codec_encoder_create_ex(encoder.quality, encoder.wavelet_type as u8) };
    let mut raw: Vec<*mut RawChunk> = vec![std::ptr::null_mut(); n_chunks as usize];
    let rc = unsafe {
        if devices.is_empty() { alice_codec_encode_many(raw_enc, rgb_chunks.as_ptr(), rgb_chunks.len() as u64, width, height, frames, n_chunks, raw.as_mut_ptr()) }
        else { alice_codec_encode_many_devices(raw_enc, rgb_chunks.as_ptr(), rgb_chunks.len() as u64, width, height, frames, n_chunks,
                                               devices.as_ptr(), devices.len() as u32, raw.as_mut_ptr()) }
    };
    unsafe { alice_codec_encoder_destroy(raw_enc) };
    check(rc, 0, 0)?;
    Ok(raw.into_iter().map(|r| EncodedChunk { raw: r }).collect())
}
pub fn decode_many(chunks: &[EncodedChunk], devices: &[i32]) -> Result<Vec<u8>, CodecError> {
    if chunks.is_empty() { return Ok(Vec::new()); }
    let raw: Vec<*const RawChunk> = chunks.iter().map(|c| c.raw as *const RawChunk).collect();
    let per = chunks[0].width() as usize * chunks[0].height() as usize * chunks[0].frames() as usize * 3;
    let mut out = vec![0u8; per * chunks.len()];
    let rc = unsafe {
        if devices.is_empty() { alice_codec_decode_many(raw.as_ptr(), raw.len() as u32, out.as_mut_ptr(), out.len() as u64) }
        else { alice_codec_decode_many_devices(raw.as_ptr(), raw.len() as u32, devices.as_ptr(), devices.len() as u32, out.as_mut_ptr(), out.len() as u64) }
    };
    check(rc, 0, 0)?;
    Ok(out)
}

// ---------------------------------------------------------------------------------------------------------------
// person segmentation: src/segment.rs (GPU; crop / paste are byte copies on the host)
// ---------------------------------------------------------------------------------------------------------------

#[link(name = "alice_codec")]
extern "C" {
    fn alice_codec_segment_by_motion(current: *const u8, current_len: u64, reference: *const u8, reference_len: u64, width: u32,
                                     height: u32, motion_threshold: u8, dilate_radius: u32, erode_radius: u32, mask: *mut u8,
                                     mask_len: u64, bbox: *mut u32, foreground_count: *mut u32) -> c_int;
    fn alice_codec_segment_by_chroma(cg: *const i16, cg_len: u64, width: u32, height: u32, green_threshold: i16, mask: *mut u8,
                                     mask_len: u64, bbox: *mut u32, foreground_count: *mut u32) -> c_int;
    fn alice_codec_rle_encode_mask(mask: *const u8, n: u64, out_len: *mut u64) -> *mut u8;
    fn alice_codec_extract_person_rgb(mask: *const u8, mask_len: u64, width: u32, bbox: *const u32, rgb: *const u8, rgb_len: u64,
                                      out: *mut u8, out_cap: u64, out_len: *mut u64) -> c_int;
}

/// src/segment.rs:42-63 (`min_region_size` is carried and, as in the reference, unused)
#[derive(Debug, Clone)]
pub struct SegmentConfig { pub motion_threshold: u8, pub min_region_size: u32, pub dilate_radius: u32, pub erode_radius: u32 }
impl Default for SegmentConfig {
    fn default() -> Self { Self { motion_threshold: 25, min_region_size: 100, dilate_radius: 2, erode_radius: 1 } }
}

/// src/segment.rs:78-89
#[derive(Debug, Clone)]
pub struct SegmentResult { pub mask: Vec<u8>, pub bbox: [u32; 4], pub foreground_count: u32, pub width: u32, pub height: u32 }

impl SegmentResult {
    /// src/segment.rs:94-101
    pub fn coverage(&self) -> f32 {
        let total = self.width.wrapping_mul(self.height);
        if total == 0 { return 0.0; }
        let inv_total = 1.0 / total as f32;
        self.foreground_count as f32 * inv_total
    }
    /// src/segment.rs:107-125 (on the GPU)
    pub fn extract_person_rgb(&self, frame_rgb: &[u8]) -> Result<Vec<u8>, CodecError> {
        let [_, _, bw, bh] = self.bbox;
        let mut out = vec![0u8; 3 * bw as usize * bh as usize];
        let mut n = 0u64;
        let rc = unsafe {
            alice_codec_extract_person_rgb(self.mask.as_ptr(), self.mask.len() as u64, self.width, self.bbox.as_ptr(), frame_rgb.as_ptr(),
                                           frame_rgb.len() as u64, out.as_mut_ptr(), out.len() as u64, &mut n)
        };
        check(rc, 0, 0)?;
        out.truncate(n as usize);
        Ok(out)
    }
    /// src/segment.rs:131-154 (on the GPU)
    pub fn rle_encode_mask(&self) -> Result<Vec<u8>, CodecError> {
        let mut n = 0u64;
        unsafe {
            let p = alice_codec_rle_encode_mask(self.mask.as_ptr(), self.mask.len() as u64, &mut n);
            if p.is_null() { Err(last_error(0, 0, 0, 0, 0)) } else { Ok(take(p, n)) }
        }
    }
}

/// src/segment.rs:172-230.  width * height past u32 is `DimensionOverflow` (the reference wraps or panics).
pub fn segment_by_motion(current: &[u8], reference: &[u8], width: u32, height: u32, config: &SegmentConfig)
    -> Result<SegmentResult, CodecError> {
    let total = (width as u64 * height as u64).min(u32::MAX as u64 + 1) as usize;
    let mut r = SegmentResult { mask: vec![0u8; if total > u32::MAX as usize { 0 } else { total }], bbox: [0; 4], foreground_count: 0, width, height };
    let rc = unsafe {
        alice_codec_segment_by_motion(current.as_ptr(), current.len() as u64, reference.as_ptr(), reference.len() as u64, width, height,
                                      config.motion_threshold, config.dilate_radius, config.erode_radius, r.mask.as_mut_ptr(),
                                      r.mask.len() as u64, r.bbox.as_mut_ptr(), &mut r.foreground_count)
    };
    check(rc, total, current.len().min(reference.len()))?;
    Ok(r)
}

/// src/segment.rs:234-265.  Returns a `Result` where the reference panics on a short `cg`.
pub fn segment_by_chroma(_y: &[i16], _co: &[i16], cg: &[i16], width: u32, height: u32, green_threshold: i16)
    -> Result<SegmentResult, CodecError> {
    let total = (width as u64 * height as u64).min(u32::MAX as u64 + 1) as usize;
    let mut r = SegmentResult { mask: vec![0u8; if total > u32::MAX as usize { 0 } else { total }], bbox: [0; 4], foreground_count: 0, width, height };
    let rc = unsafe {
        alice_codec_segment_by_chroma(cg.as_ptr(), cg.len() as u64, width, height, green_threshold, r.mask.as_mut_ptr(),
                                      r.mask.len() as u64, r.bbox.as_mut_ptr(), &mut r.foreground_count)
    };
    check(rc, total, cg.len())?;
    Ok(r)
}

/// u32 `row * frame_width + bx` of crop / paste (src/segment.rs:273-274, :288-289); overflow is `DimensionOverflow`
fn bbox_row_start(row: u32, frame_width: u32, bx: u32) -> Result<usize, CodecError> {
    row.checked_mul(frame_width).and_then(|v| v.checked_add(bx)).map(|v| v as usize).ok_or(CodecError::DimensionOverflow)
}

/// src/segment.rs:269-281 (host): a row whose end falls past the frame is skipped
pub fn crop_to_bbox(frame: &[u8], frame_width: u32, bbox: &[u32; 4]) -> Result<Vec<u8>, CodecError> {
    let [bx, by, bw, bh] = *bbox;
    let mut cropped = Vec::new();
    for row in by..by.checked_add(bh).ok_or(CodecError::DimensionOverflow)? {
        let start = bbox_row_start(row, frame_width, bx)?;
        let end = start + bw as usize;
        if end <= frame.len() { cropped.extend_from_slice(&frame[start..end]); }
    }
    Ok(cropped)
}

/// src/segment.rs:284-298 (host)
pub fn paste_from_bbox(frame: &mut [u8], frame_width: u32, person_data: &[u8], bbox: &[u32; 4]) -> Result<(), CodecError> {
    let [bx, by, bw, bh] = *bbox;
    let mut src = 0usize;
    for row in by..by.checked_add(bh).ok_or(CodecError::DimensionOverflow)? {
        let d0 = bbox_row_start(row, frame_width, bx)?;
        let d1 = d0 + bw as usize;
        if d1 <= frame.len() && src + bw as usize <= person_data.len() { frame[d0..d1].copy_from_slice(&person_data[src..src + bw as usize]); }
        src += bw as usize;
    }
    Ok(())
}

// ---------------------------------------------------------------------------------------------------------------
// split-stream format (.alc version 2).  An extension: version 1 (FrameEncoder::encode,
// EncodedChunk) stays the reference's bitstream byte for byte; version 2 keeps transform, quantiser and symbols and
// codes them as independent lanes with a table that sums to 4096 -- for video that comes back and for the latency of
// one chunk.  EncodedChunk::from_bytes refuses version 2; alc_version tells the two apart.
// ---------------------------------------------------------------------------------------------------------------

#[repr(C)]
#[derive(Default, Clone, Copy)]
struct RawSplitInfo {
    width: u32, height: u32, frames: u32, lane_symbols: u32,
    wavelet: u8, reserved: [u8; 3],
    quant_step: [i32; 3], dead_zone: [i32; 3],
    num_symbols: [u32; 3], n_blocks: [u32; 3],
    payload_len: [u64; 3],
}

#[link(name = "alice_codec")]
extern "C" {
    fn alice_codec_split_stream_bound(n: u64, lane_symbols: u32) -> u64;
    fn alice_codec_split_normalize(hist: *const u32, freq: *mut u16) -> c_int;
    fn alice_codec_split_info(data: *const u8, len: u64, info: *mut RawSplitInfo) -> c_int;
    fn alice_codec_encode_split(e: *const RawEncoder, rgb: *const u8, rgb_len: u64, w: u32, h: u32, f: u32, lane_symbols: u32,
                                out_len: *mut u64) -> *mut u8;
    fn alice_codec_decode_split(data: *const u8, len: u64, out_len: *mut u64) -> *mut u8;
    fn alice_codec_dev_encode_split(d_rgb: *const std::ffi::c_void, w: u32, h: u32, f: u32, n_chunks: u32, wavelet: u8, quality: u8,
                                    qualities: *const u8, lane_symbols: u32, d_out: *mut std::ffi::c_void, out_stride: u64,
                                    sizes: *mut u64, hip_stream: *mut std::ffi::c_void) -> c_int;
    fn alice_codec_dev_decode_split(d_alc: *const std::ffi::c_void, alc_stride: u64, sizes: *const u64, n_chunks: u32,
                                    d_rgb_out: *mut std::ffi::c_void, hip_stream: *mut std::ffi::c_void) -> c_int;
    fn alice_codec_predict_split_sizes(wavelet: u8, rgb: *const u8, rgb_len: u64, w: u32, h: u32, f: u32, lane_symbols: u32,
                                       lo: *mut u64, hi: *mut u64) -> c_int;
    fn alice_codec_encode_split_to_size(wavelet: u8, rgb: *const u8, rgb_len: u64, w: u32, h: u32, f: u32, lane_symbols: u32,
                                        max_bytes: u64, min_q: u8, max_q: u8, chosen_q: *mut u8, fits: *mut u8,
                                        out_len: *mut u64) -> *mut u8;
    fn alice_codec_predict_wide_sizes(wavelet: u8, rgb: *const u8, rgb_len: u64, w: u32, h: u32, f: u32, lane_symbols: u32,
                                      lo: *mut u64, hi: *mut u64) -> c_int;
    fn alice_codec_encode_wide_to_size(wavelet: u8, rgb: *const u8, rgb_len: u64, w: u32, h: u32, f: u32, lane_symbols: u32,
                                       max_bytes: u64, min_q: u8, max_q: u8, chosen_q: *mut u8, fits: *mut u8,
                                       out_len: *mut u64) -> *mut u8;
}

pub const SPLIT_DEFAULT_LANE_SYMBOLS: u32 = 512;
pub const SPLIT_HEADER_BYTES: usize = 1630;

/// The validated header of a version 2 container.
#[derive(Debug, Clone, PartialEq, Eq)]
pub struct SplitInfo {
    pub width: u32, pub height: u32, pub frames: u32, pub lane_symbols: u32,
    pub wavelet_type: WaveletType,
    pub quant_step: [i32; 3], pub dead_zone: [i32; 3],
    pub num_symbols: [u32; 3], pub n_blocks: [u32; 3],
    pub payload_len: [u64; 3],
}

/// Header parsing and validation: host code, no device needed; `InvalidBitstream` on a malformed field.
pub fn split_info(data: &[u8]) -> Result<SplitInfo, CodecError> {
    let mut c = RawSplitInfo::default();
    let rc = unsafe { alice_codec_split_info(data.as_ptr(), data.len() as u64, &mut c) };
    check(rc, 0, data.len())?;
    Ok(SplitInfo {
        width: c.width, height: c.height, frames: c.frames, lane_symbols: c.lane_symbols,
        wavelet_type: match c.wavelet { 1 => WaveletType::Cdf97, 2 => WaveletType::Haar, _ => WaveletType::Cdf53 },
        quant_step: c.quant_step, dead_zone: c.dead_zone, num_symbols: c.num_symbols, n_blocks: c.n_blocks,
        payload_len: c.payload_len,
    })
}

/// The version byte of a container (0 when the data is too short to have one).
pub fn alc_version(data: &[u8]) -> u8 { if data.len() > 4 { data[4] } else { 0 } }

/// One chunk as version 2 bytes, with the encoder's wavelet and quality (`lane_symbols` 0: the default).
pub fn encode_split(encoder: &FrameEncoder, rgb_frames: &[u8], width: u32, height: u32, frames: u32, lane_symbols: u32)
    -> Result<Vec<u8>, CodecError> {
    let mut n = 0u64;
    unsafe {
        let e = alice_codec_encoder_create_ex(encoder.quality, encoder.wavelet_type as u8);
        let p = alice_codec_encode_split(e, rgb_frames.as_ptr(), rgb_frames.len() as u64, width, height, frames, lane_symbols, &mut n);
        alice_codec_encoder_destroy(e);
        if p.is_null() {
            let expected = (width as usize).saturating_mul(height as usize).saturating_mul(frames as usize).saturating_mul(3);
            return Err(last_error(expected, rgb_frames.len(), width, height, 0));
        }
        Ok(take(p, n))
    }
}

/// The RGB bytes of a version 2 container; `InvalidBitstream` when a directory does not add up or a lane fails its end check.
pub fn decode_split(data: &[u8]) -> Result<Vec<u8>, CodecError> {
    let mut n = 0u64;
    unsafe {
        let p = alice_codec_decode_split(data.as_ptr(), data.len() as u64, &mut n);
        if p.is_null() { Err(last_error(0, data.len(), 0, 0, 0)) } else { Ok(take(p, n)) }
    }
}

/// The 256 frequencies a version 2 header stores for this histogram (sum 4096), from the table kernel.
pub fn normalized_frequencies(histogram: &[u32; 256]) -> Result<[u16; 256], CodecError> {
    let mut f = [0u16; 256];
    let rc = unsafe { alice_codec_split_normalize(histogram.as_ptr(), f.as_mut_ptr()) };
    check(rc, 0, 0).map(|_| f)
}

pub fn split_stream_bound(n: u64, lane_symbols: u32) -> u64 { unsafe { alice_codec_split_stream_bound(n, lane_symbols) } }

/// `n_chunks` packed device chunks -> version 2 bytes at `d_out + i * out_stride`; returns the sizes.  `qualities`: one
/// per chunk, or `None` for `quality` everywhere.
///
/// # Safety
/// `d_rgb` and `d_out` must be device pointers to `n_chunks * width*height*frames*3` and `n_chunks * out_stride` bytes.
pub unsafe fn split_encode_device(d_rgb: *const std::ffi::c_void, width: u32, height: u32, frames: u32, n_chunks: u32,
                                  wavelet_type: WaveletType, quality: u8, qualities: Option<&[u8]>, lane_symbols: u32,
                                  d_out: *mut std::ffi::c_void, out_stride: u64, hip_stream: *mut std::ffi::c_void)
    -> Result<Vec<u64>, CodecError> {
    if let Some(q) = qualities {
        if q.len() != n_chunks as usize { return Err(CodecError::InvalidBufferSize { expected: n_chunks as usize, got: q.len() }); }
    }
    let mut sizes = vec![0u64; n_chunks as usize];
    let rc = alice_codec_dev_encode_split(d_rgb, width, height, frames, n_chunks, wavelet_type as u8, quality,
                                          qualities.map_or(std::ptr::null(), |q| q.as_ptr()), lane_symbols, d_out, out_stride,
                                          sizes.as_mut_ptr(), hip_stream);
    check(rc, 0, 0).map(|_| sizes)
}

/// # Safety
/// `d_alc` holds chunk i's `sizes[i]` bytes at `i * alc_stride`; `d_rgb_out` has room for every chunk's pixels.
pub unsafe fn split_decode_device(d_alc: *const std::ffi::c_void, alc_stride: u64, sizes: &[u64], d_rgb_out: *mut std::ffi::c_void,
                                  hip_stream: *mut std::ffi::c_void) -> Result<(), CodecError> {
    check(alice_codec_dev_decode_split(d_alc, alc_stride, sizes.as_ptr(), sizes.len() as u32, d_rgb_out, hip_stream), 0, 0)
}


/// The bracket of `encode_split`'s length at the 101 qualities, from one forward transform on the GPU.  Every version 2
/// table is bounded, so `status` stays 0 throughout.
pub fn predict_split_sizes(rgb_frames: &[u8], width: u32, height: u32, frames: u32, wavelet_type: WaveletType, lane_symbols: u32)
    -> Result<SizePrediction, CodecError> {
    let mut p = SizePrediction { lo: [0; 101], hi: [0; 101], status: [0; 101] };
    let rc = unsafe {
        alice_codec_predict_split_sizes(wavelet_type as u8, rgb_frames.as_ptr(), rgb_frames.len() as u64, width, height, frames,
                                        lane_symbols, p.lo.as_mut_ptr(), p.hi.as_mut_ptr())
    };
    let expected = (width as usize).saturating_mul(height as usize).saturating_mul(frames as usize).saturating_mul(3);
    check(rc, expected, rgb_frames.len()).map(|_| p)
}

/// One chunk as version 2 bytes at the quality the budget rule picks in `[min_quality, max_quality]`: the largest whose
/// predicted upper bound fits `max_bytes`, refined by at most four exact size counts among the qualities whose bracket
/// straddles the budget.  Returns `(bytes, quality, fits)`; `fits` is false when not even `min_quality` is guaranteed to fit.
pub fn encode_split_to_size(rgb_frames: &[u8], width: u32, height: u32, frames: u32, max_bytes: u64, wavelet_type: WaveletType,
                            min_quality: u8, max_quality: u8, lane_symbols: u32) -> Result<(Vec<u8>, u8, bool), CodecError> {
    let (mut q, mut fits, mut n) = (0u8, 0u8, 0u64);
    unsafe {
        let p = alice_codec_encode_split_to_size(wavelet_type as u8, rgb_frames.as_ptr(), rgb_frames.len() as u64, width, height,
                                                 frames, lane_symbols, max_bytes, min_quality, max_quality, &mut q, &mut fits, &mut n);
        if p.is_null() {
            let expected = (width as usize).saturating_mul(height as usize).saturating_mul(frames as usize).saturating_mul(3);
            return Err(last_error(expected, rgb_frames.len(), width, height, 0));
        }
        Ok((take(p, n), q, fits != 0))
    }
}

// ---------------------------------------------------------------------------------------------------------------
// wide format (.alc version 3).  Version 2 with an untruncated symbol: the coded symbol is
// min(z, 255) and 255 is an escape followed by a 12-bit residual in the same lane chain.  The container for the top of
// the quality scale, where versions 1 and 2 wrap large coefficients modulo 256.  `lane_symbols`: a power of two in
// [64, 8192].  The header fields are version 2's (`SplitInfo`); each parser refuses the other versions.
// ---------------------------------------------------------------------------------------------------------------

#[link(name = "alice_codec")]
extern "C" {
    fn alice_codec_wide_stream_bound(n: u64, lane_symbols: u32) -> u64;
    fn alice_codec_wide_info(data: *const u8, len: u64, info: *mut RawSplitInfo) -> c_int;
    fn alice_codec_encode_wide(e: *const RawEncoder, rgb: *const u8, rgb_len: u64, w: u32, h: u32, f: u32, lane_symbols: u32,
                               out_len: *mut u64) -> *mut u8;
    fn alice_codec_decode_wide(data: *const u8, len: u64, out_len: *mut u64) -> *mut u8;
    fn alice_codec_dev_encode_wide(d_rgb: *const std::ffi::c_void, w: u32, h: u32, f: u32, n_chunks: u32, wavelet: u8, quality: u8,
                                   qualities: *const u8, lane_symbols: u32, d_out: *mut std::ffi::c_void, out_stride: u64,
                                   sizes: *mut u64, hip_stream: *mut std::ffi::c_void) -> c_int;
    fn alice_codec_dev_decode_wide(d_alc: *const std::ffi::c_void, alc_stride: u64, sizes: *const u64, n_chunks: u32,
                                   d_rgb_out: *mut std::ffi::c_void, hip_stream: *mut std::ffi::c_void) -> c_int;
}

pub const WIDE_MAX_LANE_SYMBOLS: u32 = 8192;

/// The validated header of a version 3 container (host code, no device needed).
pub fn wide_info(data: &[u8]) -> Result<SplitInfo, CodecError> {
    let mut c = RawSplitInfo::default();
    let rc = unsafe { alice_codec_wide_info(data.as_ptr(), data.len() as u64, &mut c) };
    check(rc, 0, data.len())?;
    Ok(SplitInfo {
        width: c.width, height: c.height, frames: c.frames, lane_symbols: c.lane_symbols,
        wavelet_type: match c.wavelet { 1 => WaveletType::Cdf97, 2 => WaveletType::Haar, _ => WaveletType::Cdf53 },
        quant_step: c.quant_step, dead_zone: c.dead_zone, num_symbols: c.num_symbols, n_blocks: c.n_blocks,
        payload_len: c.payload_len,
    })
}

/// One chunk as version 3 bytes, with the encoder's wavelet and quality (`lane_symbols` 0: the default).
pub fn encode_wide(encoder: &FrameEncoder, rgb_frames: &[u8], width: u32, height: u32, frames: u32, lane_symbols: u32)
    -> Result<Vec<u8>, CodecError> {
    let mut n = 0u64;
    unsafe {
        let e = alice_codec_encoder_create_ex(encoder.quality, encoder.wavelet_type as u8);
        let p = alice_codec_encode_wide(e, rgb_frames.as_ptr(), rgb_frames.len() as u64, width, height, frames, lane_symbols, &mut n);
        alice_codec_encoder_destroy(e);
        if p.is_null() {
            let expected = (width as usize).saturating_mul(height as usize).saturating_mul(frames as usize).saturating_mul(3);
            return Err(last_error(expected, rgb_frames.len(), width, height, 0));
        }
        Ok(take(p, n))
    }
}

/// The RGB bytes of a version 3 container; `InvalidBitstream` when a directory does not add up or a lane fails its end check.
pub fn decode_wide(data: &[u8]) -> Result<Vec<u8>, CodecError> {
    let mut n = 0u64;
    unsafe {
        let p = alice_codec_decode_wide(data.as_ptr(), data.len() as u64, &mut n);
        if p.is_null() { Err(last_error(0, data.len(), 0, 0, 0)) } else { Ok(take(p, n)) }
    }
}

pub fn wide_stream_bound(n: u64, lane_symbols: u32) -> u64 { unsafe { alice_codec_wide_stream_bound(n, lane_symbols) } }

/// The RGB bytes of a container of any version: 1 (`FrameDecoder`), 2 (`decode_split`), 3 (`decode_wide`),
/// 4 (`decode_reversible`) or 5 (`decode_banded`).
pub fn decode_alc(data: &[u8]) -> Result<Vec<u8>, CodecError> {
    match alc_version(data) {
        2 => decode_split(data),
        3 => decode_wide(data),
        4 => decode_reversible(data),
        5 => decode_banded(data),
        _ => FrameDecoder::new().decode(&EncodedChunk::from_bytes(data)?),
    }
}

/// # Safety
/// As `split_encode_device`.
pub unsafe fn wide_encode_device(d_rgb: *const std::ffi::c_void, width: u32, height: u32, frames: u32, n_chunks: u32,
                                 wavelet_type: WaveletType, quality: u8, qualities: Option<&[u8]>, lane_symbols: u32,
                                 d_out: *mut std::ffi::c_void, out_stride: u64, hip_stream: *mut std::ffi::c_void)
    -> Result<Vec<u64>, CodecError> {
    if let Some(q) = qualities {
        if q.len() != n_chunks as usize { return Err(CodecError::InvalidBufferSize { expected: n_chunks as usize, got: q.len() }); }
    }
    let mut sizes = vec![0u64; n_chunks as usize];
    let rc = alice_codec_dev_encode_wide(d_rgb, width, height, frames, n_chunks, wavelet_type as u8, quality,
                                         qualities.map_or(std::ptr::null(), |q| q.as_ptr()), lane_symbols, d_out, out_stride,
                                         sizes.as_mut_ptr(), hip_stream);
    check(rc, 0, 0).map(|_| sizes)
}

/// # Safety
/// As `split_decode_device`.
pub unsafe fn wide_decode_device(d_alc: *const std::ffi::c_void, alc_stride: u64, sizes: &[u64], d_rgb_out: *mut std::ffi::c_void,
                                 hip_stream: *mut std::ffi::c_void) -> Result<(), CodecError> {
    check(alice_codec_dev_decode_wide(d_alc, alc_stride, sizes.as_ptr(), sizes.len() as u32, d_rgb_out, hip_stream), 0, 0)
}


// version 3 rate control: the twins of `predict_split_sizes` / `encode_split_to_size`.

/// The bracket of `encode_wide`'s length at the 101 qualities, from one forward transform on the GPU.  Every version 3
/// table is bounded, so `status` stays 0 throughout.
pub fn predict_wide_sizes(rgb_frames: &[u8], width: u32, height: u32, frames: u32, wavelet_type: WaveletType, lane_symbols: u32)
    -> Result<SizePrediction, CodecError> {
    let mut p = SizePrediction { lo: [0; 101], hi: [0; 101], status: [0; 101] };
    let rc = unsafe {
        alice_codec_predict_wide_sizes(wavelet_type as u8, rgb_frames.as_ptr(), rgb_frames.len() as u64, width, height, frames,
                                        lane_symbols, p.lo.as_mut_ptr(), p.hi.as_mut_ptr())
    };
    let expected = (width as usize).saturating_mul(height as usize).saturating_mul(frames as usize).saturating_mul(3);
    check(rc, expected, rgb_frames.len()).map(|_| p)
}

/// One chunk as version 3 bytes at the quality the budget rule picks in `[min_quality, max_quality]`: the largest whose
/// predicted upper bound fits `max_bytes`, refined by at most four exact size counts among the qualities whose bracket
/// straddles the budget (a trial is the wide forward pass, the table and the wide count pass).  Returns `(bytes, quality, fits)`; `fits` is false when not even `min_quality` is guaranteed to fit.
pub fn encode_wide_to_size(rgb_frames: &[u8], width: u32, height: u32, frames: u32, max_bytes: u64, wavelet_type: WaveletType,
                           min_quality: u8, max_quality: u8, lane_symbols: u32) -> Result<(Vec<u8>, u8, bool), CodecError> {
    let (mut q, mut fits, mut n) = (0u8, 0u8, 0u64);
    unsafe {
        let p = alice_codec_encode_wide_to_size(wavelet_type as u8, rgb_frames.as_ptr(), rgb_frames.len() as u64, width, height,
                                                 frames, lane_symbols, max_bytes, min_quality, max_quality, &mut q, &mut fits, &mut n);
        if p.is_null() {
            let expected = (width as usize).saturating_mul(height as usize).saturating_mul(frames as usize).saturating_mul(3);
            return Err(last_error(expected, rgb_frames.len(), width, height, 0));
        }
        Ok((take(p, n), q, fits != 0))
    }
}

// ---------------------------------------------------------------------------------------------------------------
// reversible format (.alc version 4).  Version 3 whose decoder runs the forward lifting's mirror:
// at quality 100 (quantiser step 1) the pixels come back exactly.  The container for lossless archival and intermediate
// storage; below quality 100 prefer version 3 (or 2).  The encoder is version 3's -- the bytes are `encode_wide`'s except
// byte 4 -- so `predict_wide_sizes` brackets a version 4 length and `wide_stream_bound` is its stream bound; there are no
// byte-budget calls.  Each parser refuses the other versions.
// ---------------------------------------------------------------------------------------------------------------

#[link(name = "alice_codec")]
extern "C" {
    fn alice_codec_reversible_info(data: *const u8, len: u64, info: *mut RawSplitInfo) -> c_int;
    fn alice_codec_encode_reversible(e: *const RawEncoder, rgb: *const u8, rgb_len: u64, w: u32, h: u32, f: u32, lane_symbols: u32,
                                     out_len: *mut u64) -> *mut u8;
    fn alice_codec_decode_reversible(data: *const u8, len: u64, out_len: *mut u64) -> *mut u8;
    fn alice_codec_dev_encode_reversible(d_rgb: *const std::ffi::c_void, w: u32, h: u32, f: u32, n_chunks: u32, wavelet: u8,
                                         quality: u8, qualities: *const u8, lane_symbols: u32, d_out: *mut std::ffi::c_void,
                                         out_stride: u64, sizes: *mut u64, hip_stream: *mut std::ffi::c_void) -> c_int;
    fn alice_codec_dev_decode_reversible(d_alc: *const std::ffi::c_void, alc_stride: u64, sizes: *const u64, n_chunks: u32,
                                         d_rgb_out: *mut std::ffi::c_void, hip_stream: *mut std::ffi::c_void) -> c_int;
    fn alice_codec_dev_encode_reversible_regions(d_frames: *const std::ffi::c_void, frame_width: u32, frame_height: u32,
                                                 origins: *const u32, w: u32, h: u32, f: u32, n_chunks: u32, wavelet: u8,
                                                 quality: u8, qualities: *const u8, lane_symbols: u32,
                                                 d_out: *mut std::ffi::c_void, out_stride: u64, sizes: *mut u64,
                                                 hip_stream: *mut std::ffi::c_void) -> c_int;
    fn alice_codec_dev_decode_reversible_regions(d_alc: *const std::ffi::c_void, alc_stride: u64, sizes: *const u64, n_chunks: u32,
                                                 d_frames_out: *mut std::ffi::c_void, frame_width: u32, frame_height: u32,
                                                 origins: *const u32, hip_stream: *mut std::ffi::c_void) -> c_int;
}

pub const LOSSLESS_QUALITY: u8 = 100;

/// The validated header of a version 4 container (host code, no device needed).
pub fn reversible_info(data: &[u8]) -> Result<SplitInfo, CodecError> {
    let mut c = RawSplitInfo::default();
    let rc = unsafe { alice_codec_reversible_info(data.as_ptr(), data.len() as u64, &mut c) };
    check(rc, 0, data.len())?;
    Ok(SplitInfo {
        width: c.width, height: c.height, frames: c.frames, lane_symbols: c.lane_symbols,
        wavelet_type: match c.wavelet { 1 => WaveletType::Cdf97, 2 => WaveletType::Haar, _ => WaveletType::Cdf53 },
        quant_step: c.quant_step, dead_zone: c.dead_zone, num_symbols: c.num_symbols, n_blocks: c.n_blocks,
        payload_len: c.payload_len,
    })
}

/// One chunk as version 4 bytes, with the encoder's wavelet and quality (`lane_symbols` 0: the default).
pub fn encode_reversible(encoder: &FrameEncoder, rgb_frames: &[u8], width: u32, height: u32, frames: u32, lane_symbols: u32)
    -> Result<Vec<u8>, CodecError> {
    let mut n = 0u64;
    unsafe {
        let e = alice_codec_encoder_create_ex(encoder.quality, encoder.wavelet_type as u8);
        let p = alice_codec_encode_reversible(e, rgb_frames.as_ptr(), rgb_frames.len() as u64, width, height, frames, lane_symbols,
                                              &mut n);
        alice_codec_encoder_destroy(e);
        if p.is_null() {
            let expected = (width as usize).saturating_mul(height as usize).saturating_mul(frames as usize).saturating_mul(3);
            return Err(last_error(expected, rgb_frames.len(), width, height, 0));
        }
        Ok(take(p, n))
    }
}

/// `encode_reversible` at quality 100: `decode_reversible` (or `decode_alc`) returns `rgb_frames` exactly.
pub fn encode_lossless(rgb_frames: &[u8], width: u32, height: u32, frames: u32, wavelet_type: WaveletType, lane_symbols: u32)
    -> Result<Vec<u8>, CodecError> {
    encode_reversible(&FrameEncoder::with_wavelet(LOSSLESS_QUALITY, wavelet_type), rgb_frames, width, height, frames, lane_symbols)
}

/// The RGB bytes of a version 4 container; `InvalidBitstream` when a directory does not add up or a lane fails its end check.
pub fn decode_reversible(data: &[u8]) -> Result<Vec<u8>, CodecError> {
    let mut n = 0u64;
    unsafe {
        let p = alice_codec_decode_reversible(data.as_ptr(), data.len() as u64, &mut n);
        if p.is_null() { Err(last_error(0, data.len(), 0, 0, 0)) } else { Ok(take(p, n)) }
    }
}

/// # Safety
/// As `split_encode_device`.
pub unsafe fn reversible_encode_device(d_rgb: *const std::ffi::c_void, width: u32, height: u32, frames: u32, n_chunks: u32,
                                       wavelet_type: WaveletType, quality: u8, qualities: Option<&[u8]>, lane_symbols: u32,
                                       d_out: *mut std::ffi::c_void, out_stride: u64, hip_stream: *mut std::ffi::c_void)
    -> Result<Vec<u64>, CodecError> {
    if let Some(q) = qualities {
        if q.len() != n_chunks as usize { return Err(CodecError::InvalidBufferSize { expected: n_chunks as usize, got: q.len() }); }
    }
    let mut sizes = vec![0u64; n_chunks as usize];
    let rc = alice_codec_dev_encode_reversible(d_rgb, width, height, frames, n_chunks, wavelet_type as u8, quality,
                                               qualities.map_or(std::ptr::null(), |q| q.as_ptr()), lane_symbols, d_out, out_stride,
                                               sizes.as_mut_ptr(), hip_stream);
    check(rc, 0, 0).map(|_| sizes)
}

/// `reversible_encode_device` at quality 100 for every chunk.
///
/// # Safety
/// As `split_encode_device`.
pub unsafe fn encode_lossless_device(d_rgb: *const std::ffi::c_void, width: u32, height: u32, frames: u32, n_chunks: u32,
                                     wavelet_type: WaveletType, lane_symbols: u32, d_out: *mut std::ffi::c_void, out_stride: u64,
                                     hip_stream: *mut std::ffi::c_void) -> Result<Vec<u64>, CodecError> {
    reversible_encode_device(d_rgb, width, height, frames, n_chunks, wavelet_type, LOSSLESS_QUALITY, None, lane_symbols, d_out,
                             out_stride, hip_stream)
}

/// # Safety
/// As `split_decode_device`.
pub unsafe fn reversible_decode_device(d_alc: *const std::ffi::c_void, alc_stride: u64, sizes: &[u64],
                                       d_rgb_out: *mut std::ffi::c_void, hip_stream: *mut std::ffi::c_void)
    -> Result<(), CodecError> {
    check(alice_codec_dev_decode_reversible(d_alc, alc_stride, sizes.as_ptr(), sizes.len() as u32, d_rgb_out, hip_stream), 0, 0)
}

/// Chunk i is frames `[i * frames, (i + 1) * frames)` of the `frame_width` x `frame_height` device frames, cropped to
/// `width` x `height` at `origins[i]`; the bytes of chunk i are `encode_reversible`'s of the crop.
///
/// # Safety
/// As `split_encode_device`; `d_frames` holds `origins.len() * frames` packed RGB frames.
pub unsafe fn reversible_encode_regions_device(d_frames: *const std::ffi::c_void, frame_width: u32, frame_height: u32,
                                               origins: &[(u32, u32)], width: u32, height: u32, frames: u32,
                                               wavelet_type: WaveletType, quality: u8, qualities: Option<&[u8]>, lane_symbols: u32,
                                               d_out: *mut std::ffi::c_void, out_stride: u64, hip_stream: *mut std::ffi::c_void)
    -> Result<Vec<u64>, CodecError> {
    let n_chunks = origins.len();
    if let Some(q) = qualities {
        if q.len() != n_chunks { return Err(CodecError::InvalidBufferSize { expected: n_chunks, got: q.len() }); }
    }
    let flat: Vec<u32> = origins.iter().flat_map(|&(x, y)| [x, y]).collect();
    let mut sizes = vec![0u64; n_chunks];
    let rc = alice_codec_dev_encode_reversible_regions(d_frames, frame_width, frame_height, flat.as_ptr(), width, height, frames,
                                                       n_chunks as u32, wavelet_type as u8, quality,
                                                       qualities.map_or(std::ptr::null(), |q| q.as_ptr()), lane_symbols, d_out,
                                                       out_stride, sizes.as_mut_ptr(), hip_stream);
    check(rc, 0, 0).map(|_| sizes)
}

/// Chunk i is decoded and pasted into its rectangle of frames `[i * frames, (i + 1) * frames)`; no byte outside the
/// rectangles is written.
///
/// # Safety
/// As `split_decode_device`; `d_frames_out` holds `sizes.len() * frames` packed RGB frames.
pub unsafe fn reversible_decode_regions_device(d_alc: *const std::ffi::c_void, alc_stride: u64, sizes: &[u64],
                                               d_frames_out: *mut std::ffi::c_void, frame_width: u32, frame_height: u32,
                                               origins: &[(u32, u32)], hip_stream: *mut std::ffi::c_void) -> Result<(), CodecError> {
    if origins.len() != sizes.len() { return Err(CodecError::InvalidBufferSize { expected: sizes.len(), got: origins.len() }); }
    let flat: Vec<u32> = origins.iter().flat_map(|&(x, y)| [x, y]).collect();
    check(alice_codec_dev_decode_reversible_regions(d_alc, alc_stride, sizes.as_ptr(), sizes.len() as u32, d_frames_out, frame_width,
                                                    frame_height, flat.as_ptr(), hip_stream), 0, 0)
}

// ---------------------------------------------------------------------------------------------------------------
// quality control: exact trial distortion and PSNR-floor encodes.  The lane coders of versions 2 to 4
// are lossless, so the distortion of an encode is that of a transform pair: a trial runs the format's forward pass and the
// format's inverse on the device and compares the pixels with the source, without a byte of a container.
// ---------------------------------------------------------------------------------------------------------------

#[link(name = "alice_codec")]
extern "C" {
    fn alice_codec_dev_rgb_sse(d_a: *const std::ffi::c_void, a_row_pitch: u64, a_frame_pitch: u64, d_b: *const std::ffi::c_void,
                               b_row_pitch: u64, b_frame_pitch: u64, w: u32, h: u32, n_frames: u64,
                               d_frame_sse: *mut std::ffi::c_void, hip_stream: *mut std::ffi::c_void) -> c_int;
    fn alice_codec_dev_trial_sse(format: u8, d_frames: *const std::ffi::c_void, frame_width: u32, frame_height: u32,
                                 origins: *const u32, w: u32, h: u32, f: u32, n_chunks: u32, wavelet: u8, quality: u8,
                                 qualities: *const u8, sse: *mut u64, d_frame_sse: *mut std::ffi::c_void,
                                 hip_stream: *mut std::ffi::c_void) -> c_int;
    fn alice_codec_psnr_from_sse(sse: u64, n_bytes: u64) -> f64;
    fn alice_codec_dev_encode_to_psnr(format: u8, d_frames: *const std::ffi::c_void, frame_width: u32, frame_height: u32,
                                      origins: *const u32, w: u32, h: u32, f: u32, n_chunks: u32, wavelet: u8, lane_symbols: u32,
                                      min_psnr_db: f64, min_q: u8, max_q: u8, chosen: *mut u8, reached: *mut u8, psnr: *mut f64,
                                      d_out: *mut std::ffi::c_void, out_stride: u64, sizes: *mut u64,
                                      hip_stream: *mut std::ffi::c_void) -> c_int;
    fn alice_codec_encode_to_psnr(format: u8, wavelet: u8, rgb: *const u8, rgb_len: u64, w: u32, h: u32, f: u32, lane_symbols: u32,
                                  min_psnr_db: f64, min_q: u8, max_q: u8, chosen_q: *mut u8, reached: *mut u8, psnr: *mut f64,
                                  out_len: *mut u64) -> *mut u8;
}

/// The container of a quality call, by its version byte.
#[repr(u8)]
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum ContainerFormat { Split = 2, Wide = 3, Reversible = 4 }

pub const QUALITY_MAX_TRIALS: u32 = 8;

/// The dB value of a squared error over `n_bytes` samples, by the expression `psnr` uses: infinite at 0.
pub fn psnr_from_sse(sse: u64, n_bytes: u64) -> f64 { unsafe { alice_codec_psnr_from_sse(sse, n_bytes) } }

/// Exact squared error per frame of two device volumes of `n_frames` frames of `width` x `height` interleaved RGB; the
/// `n_frames` u64 sums land at `d_frame_sse`.  A side's pitches are `(row_pitch, frame_pitch)` in bytes, `None` for packed.
///
/// # Safety
/// `d_a` / `d_b` (any byte alignment) must hold the pixels their pitches name, `d_frame_sse` `n_frames` u64, all on the device.
pub unsafe fn rgb_sse_device(d_a: *const std::ffi::c_void, a_pitches: Option<(u64, u64)>, d_b: *const std::ffi::c_void,
                             b_pitches: Option<(u64, u64)>, width: u32, height: u32, n_frames: u64,
                             d_frame_sse: *mut std::ffi::c_void, hip_stream: *mut std::ffi::c_void) -> Result<(), CodecError> {
    let packed = (3 * width as u64, 3 * width as u64 * height as u64);
    let (a, b) = (a_pitches.unwrap_or(packed), b_pitches.unwrap_or(packed));
    check(alice_codec_dev_rgb_sse(d_a, a.0, a.1, d_b, b.0, b.1, width, height, n_frames, d_frame_sse, hip_stream), 0, 0)
}

/// The squared error, per chunk, between the source and what the format's decode returns for the format's encode (chunk i at
/// `qualities[i]` when given, else all at `quality`).  Packed chunks when `origins` is `None`, else regions of the
/// `frame_width` x `frame_height` frames.  `d_frame_sse`: null, or device memory for `n_chunks * frames` u64.
///
/// # Safety
/// `d_frames` must hold the chunks (or the frames the regions lie in) on the device.
pub unsafe fn trial_sse_device(format: ContainerFormat, d_frames: *const std::ffi::c_void, frame_width: u32, frame_height: u32,
                               origins: Option<&[(u32, u32)]>, width: u32, height: u32, frames: u32, n_chunks: u32,
                               wavelet_type: WaveletType, quality: u8, qualities: Option<&[u8]>,
                               d_frame_sse: *mut std::ffi::c_void, hip_stream: *mut std::ffi::c_void)
    -> Result<Vec<u64>, CodecError> {
    let n = n_chunks as usize;
    if let Some(q) = qualities {
        if q.len() != n { return Err(CodecError::InvalidBufferSize { expected: n, got: q.len() }); }
    }
    if let Some(o) = origins {
        if o.len() != n { return Err(CodecError::InvalidBufferSize { expected: n, got: o.len() }); }
    }
    let flat: Option<Vec<u32>> = origins.map(|o| o.iter().flat_map(|&(x, y)| [x, y]).collect());
    let mut sse = vec![0u64; n.max(1)];
    let rc = alice_codec_dev_trial_sse(format as u8, d_frames, frame_width, frame_height,
                                       flat.as_ref().map_or(std::ptr::null(), |o| o.as_ptr()), width, height, frames, n_chunks,
                                       wavelet_type as u8, quality, qualities.map_or(std::ptr::null(), |q| q.as_ptr()),
                                       sse.as_mut_ptr(), d_frame_sse, hip_stream);
    sse.truncate(n);
    check(rc, 0, 0).map(|_| sse)
}

/// `trial_sse_device` as dB per chunk.
///
/// # Safety
/// As `trial_sse_device`.
pub unsafe fn trial_psnr_device(format: ContainerFormat, d_frames: *const std::ffi::c_void, frame_width: u32, frame_height: u32,
                                origins: Option<&[(u32, u32)]>, width: u32, height: u32, frames: u32, n_chunks: u32,
                                wavelet_type: WaveletType, quality: u8, qualities: Option<&[u8]>,
                                hip_stream: *mut std::ffi::c_void) -> Result<Vec<f64>, CodecError> {
    let n_bytes = 3 * width as u64 * height as u64 * frames as u64;
    trial_sse_device(format, d_frames, frame_width, frame_height, origins, width, height, frames, n_chunks, wavelet_type, quality,
                     qualities, std::ptr::null_mut(), hip_stream)
        .map(|sse| sse.into_iter().map(|s| psnr_from_sse(s, n_bytes)).collect())
}

fn encode_to_psnr(format: ContainerFormat, rgb_frames: &[u8], width: u32, height: u32, frames: u32, min_psnr: f64,
                  wavelet_type: WaveletType, min_quality: u8, max_quality: u8, lane_symbols: u32)
    -> Result<(Vec<u8>, u8, bool, f64), CodecError> {
    let (mut q, mut reached, mut db, mut n) = (0u8, 0u8, 0f64, 0u64);
    unsafe {
        let p = alice_codec_encode_to_psnr(format as u8, wavelet_type as u8, rgb_frames.as_ptr(), rgb_frames.len() as u64, width,
                                           height, frames, lane_symbols, min_psnr, min_quality, max_quality, &mut q, &mut reached,
                                           &mut db, &mut n);
        if p.is_null() {
            let expected = (width as usize).saturating_mul(height as usize).saturating_mul(frames as usize).saturating_mul(3);
            return Err(last_error(expected, rgb_frames.len(), width, height, 0));
        }
        Ok((take(p, n), q, reached != 0, db))
    }
}

/// One chunk as version 2 bytes at the lowest quality in `[min_quality, max_quality]` whose measured PSNR is at least
/// `min_psnr` dB: the finest and the coarsest step of the range, then bisection, at most eight exact trials.  Returns
/// `(bytes, quality, reached, psnr)`; `reached` is false when not even `max_quality` reaches the floor (the chunk is then
/// coded at `max_quality`).  Version 2 wraps at qualities 97 and above: keep `max_quality <= 96` or use `encode_wide_to_psnr`.
pub fn encode_split_to_psnr(rgb_frames: &[u8], width: u32, height: u32, frames: u32, min_psnr: f64, wavelet_type: WaveletType,
                            min_quality: u8, max_quality: u8, lane_symbols: u32) -> Result<(Vec<u8>, u8, bool, f64), CodecError> {
    encode_to_psnr(ContainerFormat::Split, rgb_frames, width, height, frames, min_psnr, wavelet_type, min_quality, max_quality,
                   lane_symbols)
}

/// `encode_split_to_psnr` for version 3: the bytes are `encode_wide`'s at the returned quality.
pub fn encode_wide_to_psnr(rgb_frames: &[u8], width: u32, height: u32, frames: u32, min_psnr: f64, wavelet_type: WaveletType,
                           min_quality: u8, max_quality: u8, lane_symbols: u32) -> Result<(Vec<u8>, u8, bool, f64), CodecError> {
    encode_to_psnr(ContainerFormat::Wide, rgb_frames, width, height, frames, min_psnr, wavelet_type, min_quality, max_quality,
                   lane_symbols)
}

/// What a device PSNR-floor encode chose per chunk.
pub struct PsnrChoices { pub chosen: Vec<u8>, pub reached: Vec<bool>, pub psnr: Vec<f64>, pub sizes: Vec<u64> }

unsafe fn encode_to_psnr_device(format: ContainerFormat, d_frames: *const std::ffi::c_void, frame_width: u32, frame_height: u32,
                                origins: Option<&[(u32, u32)]>, width: u32, height: u32, frames: u32, n_chunks: u32,
                                wavelet_type: WaveletType, lane_symbols: u32, min_psnr: f64, min_quality: u8, max_quality: u8,
                                d_out: *mut std::ffi::c_void, out_stride: u64, hip_stream: *mut std::ffi::c_void)
    -> Result<PsnrChoices, CodecError> {
    let n = n_chunks as usize;
    if let Some(o) = origins {
        if o.len() != n { return Err(CodecError::InvalidBufferSize { expected: n, got: o.len() }); }
    }
    let flat: Option<Vec<u32>> = origins.map(|o| o.iter().flat_map(|&(x, y)| [x, y]).collect());
    let (mut chosen, mut reached, mut psnr, mut sizes) = (vec![0u8; n.max(1)], vec![0u8; n.max(1)], vec![0f64; n.max(1)], vec![0u64; n.max(1)]);
    let rc = alice_codec_dev_encode_to_psnr(format as u8, d_frames, frame_width, frame_height,
                                            flat.as_ref().map_or(std::ptr::null(), |o| o.as_ptr()), width, height, frames, n_chunks,
                                            wavelet_type as u8, lane_symbols, min_psnr, min_quality, max_quality, chosen.as_mut_ptr(),
                                            reached.as_mut_ptr(), psnr.as_mut_ptr(), d_out, out_stride, sizes.as_mut_ptr(), hip_stream);
    chosen.truncate(n); reached.truncate(n); psnr.truncate(n); sizes.truncate(n);
    check(rc, 0, 0).map(|_| PsnrChoices { chosen, reached: reached.into_iter().map(|r| r != 0).collect(), psnr, sizes })
}

/// `n_chunks` device chunks (packed, or regions when `origins` is given), chunk i at the quality `encode_split_to_psnr`'s
/// rule picks for it, the bytes at `d_out + i * out_stride`.
///
/// # Safety
/// As `split_encode_device`.
pub unsafe fn split_encode_to_psnr_device(d_frames: *const std::ffi::c_void, frame_width: u32, frame_height: u32,
                                          origins: Option<&[(u32, u32)]>, width: u32, height: u32, frames: u32, n_chunks: u32,
                                          wavelet_type: WaveletType, lane_symbols: u32, min_psnr: f64, min_quality: u8,
                                          max_quality: u8, d_out: *mut std::ffi::c_void, out_stride: u64,
                                          hip_stream: *mut std::ffi::c_void) -> Result<PsnrChoices, CodecError> {
    encode_to_psnr_device(ContainerFormat::Split, d_frames, frame_width, frame_height, origins, width, height, frames, n_chunks,
                          wavelet_type, lane_symbols, min_psnr, min_quality, max_quality, d_out, out_stride, hip_stream)
}

/// `split_encode_to_psnr_device` for version 3.
///
/// # Safety
/// As `split_encode_device`.
pub unsafe fn wide_encode_to_psnr_device(d_frames: *const std::ffi::c_void, frame_width: u32, frame_height: u32,
                                         origins: Option<&[(u32, u32)]>, width: u32, height: u32, frames: u32, n_chunks: u32,
                                         wavelet_type: WaveletType, lane_symbols: u32, min_psnr: f64, min_quality: u8,
                                         max_quality: u8, d_out: *mut std::ffi::c_void, out_stride: u64,
                                         hip_stream: *mut std::ffi::c_void) -> Result<PsnrChoices, CodecError> {
    encode_to_psnr_device(ContainerFormat::Wide, d_frames, frame_width, frame_height, origins, width, height, frames, n_chunks,
                          wavelet_type, lane_symbols, min_psnr, min_quality, max_quality, d_out, out_stride, hip_stream)
}

// ---- frame ranges of a version 2, 3 or 4 chunk ----

extern "C" {
    fn alice_codec_frames_window(wavelet_type: u8, frames: u32, first: u32, count: u32, a: *mut u32, b: *mut u32) -> c_int;
    fn alice_codec_decode_frames(data: *const u8, len: u64, first: u32, count: u32, out_len: *mut u64) -> *mut u8;
    fn alice_codec_dev_decode_frames(d_alc: *const std::ffi::c_void, len: u64, first: u32, count: u32,
                                     d_rgb_out: *mut std::ffi::c_void, hip_stream: *mut std::ffi::c_void) -> c_int;
}

/// `(a, b)`: frames `[first, first + count)` of a chunk of `frames` frames depend on the coefficient planes of the frame
/// pairs inside `[a, b)` only.  No device needed.
pub fn frames_window(wavelet_type: WaveletType, frames: u32, first: u32, count: u32) -> Result<(u32, u32), CodecError> {
    let (mut a, mut b) = (0u32, 0u32);
    let rc = unsafe { alice_codec_frames_window(wavelet_type as u8, frames, first, count, &mut a, &mut b) };
    check(rc, 0, 0).map(|_| (a, b))
}

/// The RGB bytes of frames `[first, first + count)` of a version 2, 3 or 4 container, from the blocks they need: only the
/// header, the block-length tables and those blocks are read and uploaded.  The end checks cover the blocks that are read;
/// version 1 is `InvalidBitstream` (it has no random access).
pub fn decode_frames(data: &[u8], first: u32, count: u32) -> Result<Vec<u8>, CodecError> {
    let mut n = 0u64;
    unsafe {
        let p = alice_codec_decode_frames(data.as_ptr(), data.len() as u64, first, count, &mut n);
        if p.is_null() { Err(last_error(0, data.len(), 0, 0, 0)) } else { Ok(take(p, n)) }
    }
}

/// `decode_frames` of a device-resident container of `length` bytes into `count` packed frames at `d_rgb_out`.
///
/// # Safety
/// As `split_decode_device`: `d_alc` holds `length` bytes and `d_rgb_out` room for `count` frames on the current device.
pub unsafe fn frames_decode_device(d_alc: *const std::ffi::c_void, length: u64, first: u32, count: u32,
                                   d_rgb_out: *mut std::ffi::c_void, hip_stream: *mut std::ffi::c_void)
    -> Result<(), CodecError> {
    check(alice_codec_dev_decode_frames(d_alc, length, first, count, d_rgb_out, hip_stream), 0, 0)
}

// ---- half-resolution preview of a version 2, 3 or 4 chunk from the low band alone ----

extern "C" {
    fn alice_codec_preview_dims(width: u32, height: u32, qw: *mut u32, qh: *mut u32) -> c_int;
    fn alice_codec_decode_preview(data: *const u8, len: u64, first: u32, count: u32, out_len: *mut u64) -> *mut u8;
    fn alice_codec_dev_decode_preview(d_alc: *const std::ffi::c_void, len: u64, first: u32, count: u32,
                                      d_rgb_out: *mut std::ffi::c_void, hip_stream: *mut std::ffi::c_void) -> c_int;
}

/// `(qw, qh)` = `(ceil(width / 2), ceil(height / 2))`: the size of a preview frame.  No device needed.
pub fn preview_dims(width: u32, height: u32) -> Result<(u32, u32), CodecError> {
    let (mut qw, mut qh) = (0u32, 0u32);
    let rc = unsafe { alice_codec_preview_dims(width, height, &mut qw, &mut qh) };
    check(rc, 0, 0).map(|_| (qw, qh))
}

/// The half-resolution RGB bytes (`count * qh * qw * 3`) of frames `[first, first + count)` of a version 2, 3 or 4
/// container, from the low-low quadrants of the coefficient planes the range needs: the blocks of a plane's bottom half are
/// never read.  The end checks cover the blocks that are read; version 1 is `InvalidBitstream`.
pub fn decode_preview(data: &[u8], first: u32, count: u32) -> Result<Vec<u8>, CodecError> {
    let mut n = 0u64;
    unsafe {
        let p = alice_codec_decode_preview(data.as_ptr(), data.len() as u64, first, count, &mut n);
        if p.is_null() { Err(last_error(0, data.len(), 0, 0, 0)) } else { Ok(take(p, n)) }
    }
}

/// `decode_preview` of a device-resident container of `length` bytes into `count` packed preview frames at `d_rgb_out`.
///
/// # Safety
/// As `split_decode_device`: `d_alc` holds `length` bytes and `d_rgb_out` room for `count * qh * qw * 3` bytes on the
/// current device.
pub unsafe fn preview_decode_device(d_alc: *const std::ffi::c_void, length: u64, first: u32, count: u32,
                                    d_rgb_out: *mut std::ffi::c_void, hip_stream: *mut std::ffi::c_void)
    -> Result<(), CodecError> {
    check(alice_codec_dev_decode_preview(d_alc, length, first, count, d_rgb_out, hip_stream), 0, 0)
}

// ---- many previews in one call ----

/// `alice_codec_preview_item` of include/alice_codec.h
#[repr(C)]
#[derive(Debug, Clone, Copy)]
pub struct PreviewItem {
    pub alc: *const std::ffi::c_void,
    pub len: u64,
    pub first: u32,
    pub count: u32,
    pub rgb_out: *mut std::ffi::c_void,
}

pub const PREVIEWS_MAX_ITEMS: u32 = 1024;

extern "C" {
    fn alice_codec_decode_previews(items: *const PreviewItem, n_items: u32, offsets: *mut u64, bad_item: *mut u32) -> *mut u8;
    fn alice_codec_dev_decode_previews(items: *const PreviewItem, n_items: u32, bad_item: *mut u32,
                                       hip_stream: *mut std::ffi::c_void) -> c_int;
}

/// `decode_preview` of many `(data, first, count)` items in one call, one `Vec` per item in item order.  Items that pass the
/// same slice share its header, tables, directory scan and upload.  All or nothing: the message of the error of a refused
/// or damaged call starts with `item <index>: `.
pub fn decode_previews(items: &[(&[u8], u32, u32)]) -> Result<Vec<Vec<u8>>, CodecError> {
    let raw: Vec<PreviewItem> = items.iter().map(|(d, first, count)| PreviewItem {
        alc: d.as_ptr() as *const std::ffi::c_void, len: d.len() as u64, first: *first, count: *count, rgb_out: std::ptr::null_mut(),
    }).collect();
    let mut offsets = vec![0u64; items.len() + 1];
    let n = u32::try_from(items.len()).unwrap_or(u32::MAX);
    unsafe {
        let p = alice_codec_decode_previews(raw.as_ptr(), n, offsets.as_mut_ptr(), std::ptr::null_mut());
        if p.is_null() { return Err(last_error(0, 0, 0, 0, 0)); }
        let whole = take(p, offsets[items.len()]);
        Ok((0..items.len()).map(|i| whole[offsets[i] as usize..offsets[i + 1] as usize].to_vec()).collect())
    }
}

/// `preview_decode_device` of many items in one call; returns the index of the item that decided a refusal with the error.
///
/// # Safety
/// As `preview_decode_device` for every item; the outputs must not overlap.
pub unsafe fn previews_decode_device(items: &[PreviewItem], hip_stream: *mut std::ffi::c_void) -> Result<(), (CodecError, u32)> {
    let mut bad = u32::MAX;
    let n = u32::try_from(items.len()).unwrap_or(u32::MAX);
    check(alice_codec_dev_decode_previews(items.as_ptr(), n, &mut bad, hip_stream), 0, 0).map_err(|e| (e, bad))
}

// ---- a spatial rectangle of a frame range of a version 2, 3 or 4 chunk ----

extern "C" {
    fn alice_codec_rect_window(wavelet_type: u8, width: u32, height: u32, x: u32, y: u32, w: u32, h: u32, xa: *mut u32,
                               xb: *mut u32, ya: *mut u32, yb: *mut u32) -> c_int;
    fn alice_codec_decode_rect(data: *const u8, len: u64, first: u32, count: u32, x: u32, y: u32, w: u32, h: u32,
                               out_len: *mut u64) -> *mut u8;
    fn alice_codec_dev_decode_rect(d_alc: *const std::ffi::c_void, len: u64, first: u32, count: u32, x: u32, y: u32, w: u32,
                                   h: u32, d_rgb_out: *mut std::ffi::c_void, row_pitch: u64, frame_pitch: u64,
                                   hip_stream: *mut std::ffi::c_void) -> c_int;
}

/// The `w x h` pixels at `(x, y)` of a frame.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct Rect { pub x: u32, pub y: u32, pub w: u32, pub h: u32 }

/// `(xa, xb, ya, yb)`: the rectangle's pixels depend on the coefficient columns inside `[xa, xb)` and rows inside
/// `[ya, yb)` only.  No device needed.
pub fn rect_window(wavelet_type: WaveletType, width: u32, height: u32, r: Rect) -> Result<(u32, u32, u32, u32), CodecError> {
    let (mut xa, mut xb, mut ya, mut yb) = (0u32, 0u32, 0u32, 0u32);
    let rc = unsafe { alice_codec_rect_window(wavelet_type as u8, width, height, r.x, r.y, r.w, r.h, &mut xa, &mut xb, &mut ya, &mut yb) };
    check(rc, 0, 0).map(|_| (xa, xb, ya, yb))
}

/// The RGB bytes (`count * h * w * 3`, packed) of the rectangle of frames `[first, first + count)` of a version 2, 3 or 4
/// container, from the blocks they need: only the header, the block-length tables and those blocks are read and uploaded.
/// The end checks cover the blocks that are read; version 1 is `InvalidBitstream`.
pub fn decode_rect(data: &[u8], first: u32, count: u32, r: Rect) -> Result<Vec<u8>, CodecError> {
    let mut n = 0u64;
    unsafe {
        let p = alice_codec_decode_rect(data.as_ptr(), data.len() as u64, first, count, r.x, r.y, r.w, r.h, &mut n);
        if p.is_null() { Err(last_error(0, data.len(), 0, 0, 0)) } else { Ok(take(p, n)) }
    }
}

/// `decode_rect` of a device-resident container of `length` bytes to `d_rgb_out`: packed when both pitches are 0, else row
/// `r` of frame `k` at `k * frame_pitch + r * row_pitch` bytes, so that the rectangle can be pasted into full-size frames.
///
/// # Safety
/// As `split_decode_device`: `d_alc` holds `length` bytes, and every byte `d_rgb_out + k * frame_pitch + r * row_pitch +
/// [0, 3 w)` for `k < count`, `r < h` is writable on the current device.
pub unsafe fn rect_decode_device(d_alc: *const std::ffi::c_void, length: u64, first: u32, count: u32, r: Rect,
                                 d_rgb_out: *mut std::ffi::c_void, row_pitch: u64, frame_pitch: u64,
                                 hip_stream: *mut std::ffi::c_void) -> Result<(), CodecError> {
    check(alice_codec_dev_decode_rect(d_alc, length, first, count, r.x, r.y, r.w, r.h, d_rgb_out, row_pitch, frame_pitch, hip_stream), 0, 0)
}

// ---- many frame ranges and rectangles in one call ----

/// `alice_codec_rect_item` of include/alice_codec.h (64 bytes); `x = y = w = h = 0` is the whole frame
#[repr(C)]
#[derive(Debug, Clone, Copy)]
pub struct RectItem {
    pub alc: *const std::ffi::c_void,
    pub len: u64,
    pub first: u32,
    pub count: u32,
    pub x: u32,
    pub y: u32,
    pub w: u32,
    pub h: u32,
    pub rgb_out: *mut std::ffi::c_void,
    pub row_pitch: u64,
    pub frame_pitch: u64,
}

pub const RECTS_MAX_ITEMS: u32 = 1024;

extern "C" {
    fn alice_codec_decode_rects(items: *const RectItem, n_items: u32, offsets: *mut u64, bad_item: *mut u32) -> *mut u8;
    fn alice_codec_dev_decode_rects(items: *const RectItem, n_items: u32, bad_item: *mut u32,
                                    hip_stream: *mut std::ffi::c_void) -> c_int;
}

/// `decode_rect` (or, with `None`, `decode_frames`) of many `(data, first, count, rectangle)` items in one call, one `Vec`
/// per item in item order.  Items that pass the same slice share its header, tables, directory scan and upload.  All or
/// nothing: the message of the error of a refused or damaged call starts with `item <index>: `.
pub fn decode_rects(items: &[(&[u8], u32, u32, Option<Rect>)]) -> Result<Vec<Vec<u8>>, CodecError> {
    let raw: Vec<RectItem> = items.iter().map(|(d, first, count, r)| {
        let r = r.unwrap_or(Rect { x: 0, y: 0, w: 0, h: 0 });
        RectItem { alc: d.as_ptr() as *const std::ffi::c_void, len: d.len() as u64, first: *first, count: *count, x: r.x, y: r.y,
                   w: r.w, h: r.h, rgb_out: std::ptr::null_mut(), row_pitch: 0, frame_pitch: 0 }
    }).collect();
    let mut offsets = vec![0u64; items.len() + 1];
    let n = u32::try_from(items.len()).unwrap_or(u32::MAX);
    unsafe {
        let p = alice_codec_decode_rects(raw.as_ptr(), n, offsets.as_mut_ptr(), std::ptr::null_mut());
        if p.is_null() { return Err(last_error(0, 0, 0, 0, 0)); }
        let whole = take(p, offsets[items.len()]);
        Ok((0..items.len()).map(|i| whole[offsets[i] as usize..offsets[i + 1] as usize].to_vec()).collect())
    }
}

/// `rect_decode_device` of many items in one call; returns the index of the item that decided a refusal with the error.
///
/// # Safety
/// As `rect_decode_device` for every item; the outputs must be disjoint (byte ranges apart, or boxes of one pitched surface
/// that are).
pub unsafe fn rects_decode_device(items: &[RectItem], hip_stream: *mut std::ffi::c_void) -> Result<(), (CodecError, u32)> {
    let mut bad = u32::MAX;
    let n = u32::try_from(items.len()).unwrap_or(u32::MAX);
    check(alice_codec_dev_decode_rects(items.as_ptr(), n, &mut bad, hip_stream), 0, 0).map_err(|e| (e, bad))
}

// ---- transcode of a version 2, 3 or 4 chunk to a lower quality or a byte budget, without pixels ----

extern "C" {
    fn alice_codec_transcode(data: *const u8, len: u64, quality: u8, lane_symbols: u32, out_version: u8, out_len: *mut u64) -> *mut u8;
    fn alice_codec_transcode_to_size(data: *const u8, len: u64, lane_symbols: u32, out_version: u8, max_bytes: u64, min_q: u8, max_q: u8,
                                     chosen_q: *mut u8, fits: *mut u8, out_len: *mut u64) -> *mut u8;
    fn alice_codec_predict_transcode_sizes(data: *const u8, len: u64, lane_symbols: u32, lo: *mut u64, hi: *mut u64) -> c_int;
    fn alice_codec_dev_transcode(d_alc: *const std::ffi::c_void, alc_stride: u64, sizes: *const u64, n_chunks: u32, quality: u8,
                                 qualities: *const u8, lane_symbols: u32, out_version: u8, d_out: *mut std::ffi::c_void, out_stride: u64,
                                 out_sizes: *mut u64, hip_stream: *mut std::ffi::c_void) -> c_int;
    fn alice_codec_dev_transcode_to_budget(d_alc: *const std::ffi::c_void, alc_stride: u64, sizes: *const u64, n_chunks: u32,
                                           lane_symbols: u32, out_version: u8, budgets: *const u64, min_q: u8, max_q: u8, chosen: *mut u8,
                                           fits: *mut u8, d_out: *mut std::ffi::c_void, out_stride: u64, out_sizes: *mut u64,
                                           hip_stream: *mut std::ffi::c_void) -> c_int;
    fn alice_codec_dev_requant_symbols(d_src: *const std::ffi::c_void, d_dst: *mut std::ffi::c_void, n: u64, wide: c_int, step_from: i32,
                                       step_to: i32, d_hist: *mut std::ffi::c_void, hip_stream: *mut std::ffi::c_void) -> c_int;
}

/// A version 2, 3 or 4 container at `quality`, made from its symbols alone.  A channel whose quantiser step is already at or
/// above the target's is left as it is, so a quality at or above the source's returns the source's bytes; from a quality-100
/// source the result is byte for byte the direct encode at `quality`.  `lane_symbols` 0 keeps the source's; `out_version` 0
/// keeps the version, 3 and 4 may be exchanged.  Version 1 is `InvalidBitstream`.
pub fn transcode(data: &[u8], quality: u8, lane_symbols: u32, out_version: u8) -> Result<Vec<u8>, CodecError> {
    let mut n = 0u64;
    unsafe {
        let p = alice_codec_transcode(data.as_ptr(), data.len() as u64, quality, lane_symbols, out_version, &mut n);
        if p.is_null() { Err(last_error(0, data.len(), 0, 0, 0)) } else { Ok(take(p, n)) }
    }
}

/// `transcode` at the highest quality in `[min_quality, max_quality]` the byte-budget rule of `encode_split_to_size` finds to
/// fit `max_bytes`: `(bytes, quality, fits)`.  A version 4 result has no budget: pass `out_version` 3.
pub fn transcode_to_size(data: &[u8], max_bytes: u64, min_quality: u8, max_quality: u8, lane_symbols: u32, out_version: u8)
    -> Result<(Vec<u8>, u8, bool), CodecError> {
    let (mut q, mut fits, mut n) = (0u8, 0u8, 0u64);
    unsafe {
        let p = alice_codec_transcode_to_size(data.as_ptr(), data.len() as u64, lane_symbols, out_version, max_bytes, min_quality,
                                              max_quality, &mut q, &mut fits, &mut n);
        if p.is_null() { return Err(last_error(0, data.len(), 0, 0, 0)); }
        Ok((take(p, n), q, fits != 0))
    }
}

/// `(lo, hi)`: `lo[q] <= transcode(data, q, lane_symbols, 0).len() <= hi[q]` for the 101 qualities.
pub fn predict_transcode_sizes(data: &[u8], lane_symbols: u32) -> Result<([u64; 101], [u64; 101]), CodecError> {
    let (mut lo, mut hi) = ([0u64; 101], [0u64; 101]);
    let rc = unsafe { alice_codec_predict_transcode_sizes(data.as_ptr(), data.len() as u64, lane_symbols, lo.as_mut_ptr(), hi.as_mut_ptr()) };
    check(rc, 0, data.len()).map(|_| (lo, hi))
}

/// `sizes.len()` device containers of one version, wavelet, shape and lane_symbols, chunk `i` at `d_alc + i * alc_stride`, to
/// `qualities[i]` (`None`: `quality`) at `d_out + i * out_stride`; returns the sizes.
///
/// # Safety
/// `d_alc` holds the chunks and `d_out` room for `sizes.len() * out_stride` bytes on the current device; they do not overlap.
pub unsafe fn transcode_device(d_alc: *const std::ffi::c_void, alc_stride: u64, sizes: &[u64], quality: u8, qualities: Option<&[u8]>,
                               lane_symbols: u32, out_version: u8, d_out: *mut std::ffi::c_void, out_stride: u64,
                               hip_stream: *mut std::ffi::c_void) -> Result<Vec<u64>, CodecError> {
    if let Some(q) = qualities { if q.len() != sizes.len() { return Err(CodecError::InvalidDimensions { width: 0, height: 0 }); } }
    let mut out = vec![0u64; sizes.len()];
    let n = u32::try_from(sizes.len()).unwrap_or(u32::MAX);
    check(alice_codec_dev_transcode(d_alc, alc_stride, sizes.as_ptr(), n, quality, qualities.map_or(std::ptr::null(), |q| q.as_ptr()),
                                    lane_symbols, out_version, d_out, out_stride, out.as_mut_ptr(), hip_stream), 0, 0).map(|_| out)
}

/// `transcode_device` with chunk `i` under `budgets[i]` bytes: `(chosen, fits, sizes)`.
///
/// # Safety
/// As `transcode_device`.
pub unsafe fn transcode_to_budget_device(d_alc: *const std::ffi::c_void, alc_stride: u64, sizes: &[u64], budgets: &[u64], min_quality: u8,
                                         max_quality: u8, lane_symbols: u32, out_version: u8, d_out: *mut std::ffi::c_void,
                                         out_stride: u64, hip_stream: *mut std::ffi::c_void)
    -> Result<(Vec<u8>, Vec<bool>, Vec<u64>), CodecError> {
    if budgets.len() != sizes.len() { return Err(CodecError::InvalidDimensions { width: 0, height: 0 }); }
    let (mut chosen, mut fits, mut out) = (vec![0u8; sizes.len()], vec![0u8; sizes.len()], vec![0u64; sizes.len()]);
    let n = u32::try_from(sizes.len()).unwrap_or(u32::MAX);
    check(alice_codec_dev_transcode_to_budget(d_alc, alc_stride, sizes.as_ptr(), n, lane_symbols, out_version, budgets.as_ptr(), min_quality,
                                              max_quality, chosen.as_mut_ptr(), fits.as_mut_ptr(), d_out, out_stride, out.as_mut_ptr(),
                                              hip_stream), 0, 0)?;
    Ok((chosen, fits.into_iter().map(|v| v != 0).collect(), out))
}

/// Stage call: the map alone.  `n` device symbols (u8; `wide`: u16) from `d_src` to `d_dst` through the transcode map of the
/// quantiser steps `(step_from, step_to)`; the histogram of the coded symbols is added to the 256 u32 at `d_hist` when not null.
///
/// # Safety
/// `d_src` and `d_dst` hold `n` symbols on the current device and are the same address or do not overlap.
pub unsafe fn requant_symbols_device(d_src: *const std::ffi::c_void, d_dst: *mut std::ffi::c_void, n: u64, wide: bool, step_from: i32,
                                     step_to: i32, d_hist: *mut std::ffi::c_void, hip_stream: *mut std::ffi::c_void)
    -> Result<(), CodecError> {
    check(alice_codec_dev_requant_symbols(d_src, d_dst, n, wide as c_int, step_from, step_to, d_hist, hip_stream), 0, 0)
}

// ---- banded format (.alc version 5): one frequency table per wavelet subband ----
pub const BANDED_HEADER_BYTES: usize = 12636;

#[repr(C)]
#[derive(Clone, Copy)]
struct RawBandedInfo {
    width: u32, height: u32, frames: u32, lane_symbols: u32,
    wavelet: u8, base: u8, reserved: [u8; 2],
    quant_step: [i32; 3], dead_zone: [i32; 3],
    num_symbols: [u32; 3], n_blocks: [u32; 24], payload_len: [u64; 24],
}

extern "C" {
    fn alice_codec_banded_stream_bound(n_band: u64, lane_symbols: u32, base: u8) -> u64;
    fn alice_codec_banded_info(data: *const u8, len: u64, info: *mut RawBandedInfo) -> c_int;
    fn alice_codec_encode_banded(encoder: *const RawEncoder, rgb: *const u8, rgb_len: u64, width: u32, height: u32, frames: u32,
                                 lane_symbols: u32, base: u8, out_len: *mut u64) -> *mut u8;
    fn alice_codec_decode_banded(data: *const u8, len: u64, out_len: *mut u64) -> *mut u8;
    fn alice_codec_to_banded(data: *const u8, len: u64, lane_symbols: u32, out_len: *mut u64) -> *mut u8;
    fn alice_codec_from_banded(data: *const u8, len: u64, lane_symbols: u32, out_len: *mut u64) -> *mut u8;
    fn alice_codec_dev_encode_banded(d_rgb: *const std::ffi::c_void, width: u32, height: u32, frames: u32, n_chunks: u32, wavelet_type: u8,
                                     quality: u8, qualities: *const u8, lane_symbols: u32, base: u8, d_out: *mut std::ffi::c_void,
                                     out_stride: u64, sizes: *mut u64, hip_stream: *mut std::ffi::c_void) -> c_int;
    fn alice_codec_dev_decode_banded(d_alc: *const std::ffi::c_void, alc_stride: u64, sizes: *const u64, n_chunks: u32,
                                     d_rgb_out: *mut std::ffi::c_void, hip_stream: *mut std::ffi::c_void) -> c_int;
    fn alice_codec_dev_to_banded(d_alc: *const std::ffi::c_void, alc_stride: u64, sizes: *const u64, n_chunks: u32, lane_symbols: u32,
                                 d_out: *mut std::ffi::c_void, out_stride: u64, out_sizes: *mut u64, hip_stream: *mut std::ffi::c_void) -> c_int;
    fn alice_codec_dev_from_banded(d_alc: *const std::ffi::c_void, alc_stride: u64, sizes: *const u64, n_chunks: u32, lane_symbols: u32,
                                   d_out: *mut std::ffi::c_void, out_stride: u64, out_sizes: *mut u64, hip_stream: *mut std::ffi::c_void) -> c_int;
    fn alice_codec_dev_band_histograms(d_symbols: *const std::ffi::c_void, width: u32, height: u32, frames: u32, wide: c_int,
                                       d_hist: *mut std::ffi::c_void, hip_stream: *mut std::ffi::c_void) -> c_int;
}

/// The validated header of a version 5 container; `n_blocks` and `payload_len` are channel-major, band ascending.
#[derive(Debug, Clone, PartialEq, Eq)]
pub struct BandedInfo {
    pub width: u32, pub height: u32, pub frames: u32, pub lane_symbols: u32,
    pub wavelet_type: WaveletType, pub base: u8,
    pub quant_step: [i32; 3], pub dead_zone: [i32; 3], pub num_symbols: [u32; 3],
    pub n_blocks: [u32; 24], pub payload_len: [u64; 24],
}

pub fn banded_info(data: &[u8]) -> Result<BandedInfo, CodecError> {
    let mut c = RawBandedInfo { width: 0, height: 0, frames: 0, lane_symbols: 0, wavelet: 0, base: 0, reserved: [0; 2], quant_step: [0; 3],
                                dead_zone: [0; 3], num_symbols: [0; 3], n_blocks: [0; 24], payload_len: [0; 24] };
    let rc = unsafe { alice_codec_banded_info(data.as_ptr(), data.len() as u64, &mut c) };
    check(rc, 0, data.len())?;
    Ok(BandedInfo {
        width: c.width, height: c.height, frames: c.frames, lane_symbols: c.lane_symbols,
        wavelet_type: match c.wavelet { 1 => WaveletType::Cdf97, 2 => WaveletType::Haar, _ => WaveletType::Cdf53 }, base: c.base,
        quant_step: c.quant_step, dead_zone: c.dead_zone, num_symbols: c.num_symbols, n_blocks: c.n_blocks, payload_len: c.payload_len,
    })
}

pub fn banded_stream_bound(n_band: u64, lane_symbols: u32, base: u8) -> u64 { unsafe { alice_codec_banded_stream_bound(n_band, lane_symbols, base) } }

/// One chunk as version 5 bytes of `base` (2, 3 or 4), with the encoder's wavelet and quality (`lane_symbols` 0: the default).
pub fn encode_banded(encoder: &FrameEncoder, rgb_frames: &[u8], width: u32, height: u32, frames: u32, lane_symbols: u32, base: u8)
    -> Result<Vec<u8>, CodecError> {
    let mut n = 0u64;
    unsafe {
        let e = alice_codec_encoder_create_ex(encoder.quality, encoder.wavelet_type as u8);
        let p = alice_codec_encode_banded(e, rgb_frames.as_ptr(), rgb_frames.len() as u64, width, height, frames, lane_symbols, base, &mut n);
        alice_codec_encoder_destroy(e);
        if p.is_null() {
            let expected = (width as usize).saturating_mul(height as usize).saturating_mul(frames as usize).saturating_mul(3);
            return Err(last_error(expected, rgb_frames.len(), width, height, 0));
        }
        Ok(take(p, n))
    }
}

/// The RGB bytes of a version 5 container: the pixels of its base version's chunk.
pub fn decode_banded(data: &[u8]) -> Result<Vec<u8>, CodecError> {
    let mut n = 0u64;
    unsafe {
        let p = alice_codec_decode_banded(data.as_ptr(), data.len() as u64, &mut n);
        if p.is_null() { Err(last_error(0, data.len(), 0, 0, 0)) } else { Ok(take(p, n)) }
    }
}

/// A version 2, 3 or 4 container as the version 5 container of that base, from its symbols alone (`lane_symbols` 0 keeps it).
pub fn to_banded(data: &[u8], lane_symbols: u32) -> Result<Vec<u8>, CodecError> {
    let mut n = 0u64;
    unsafe {
        let p = alice_codec_to_banded(data.as_ptr(), data.len() as u64, lane_symbols, &mut n);
        if p.is_null() { Err(last_error(0, data.len(), 0, 0, 0)) } else { Ok(take(p, n)) }
    }
}

/// A version 5 container as the container of its base version: `from_banded(to_banded(x)) == x`.
pub fn from_banded(data: &[u8], lane_symbols: u32) -> Result<Vec<u8>, CodecError> {
    let mut n = 0u64;
    unsafe {
        let p = alice_codec_from_banded(data.as_ptr(), data.len() as u64, lane_symbols, &mut n);
        if p.is_null() { Err(last_error(0, data.len(), 0, 0, 0)) } else { Ok(take(p, n)) }
    }
}

/// # Safety
/// As `split_encode_device`.
pub unsafe fn banded_encode_device(d_rgb: *const std::ffi::c_void, width: u32, height: u32, frames: u32, n_chunks: u32,
                                   wavelet_type: WaveletType, quality: u8, qualities: Option<&[u8]>, lane_symbols: u32, base: u8,
                                   d_out: *mut std::ffi::c_void, out_stride: u64, hip_stream: *mut std::ffi::c_void)
    -> Result<Vec<u64>, CodecError> {
    if let Some(q) = qualities { if q.len() != n_chunks as usize { return Err(CodecError::InvalidDimensions { width, height }); } }
    let mut sizes = vec![0u64; n_chunks as usize];
    check(alice_codec_dev_encode_banded(d_rgb, width, height, frames, n_chunks, wavelet_type as u8, quality,
                                        qualities.map_or(std::ptr::null(), |q| q.as_ptr()), lane_symbols, base, d_out, out_stride,
                                        sizes.as_mut_ptr(), hip_stream), 0, 0).map(|_| sizes)
}

/// # Safety
/// As `split_decode_device`.
pub unsafe fn banded_decode_device(d_alc: *const std::ffi::c_void, alc_stride: u64, sizes: &[u64], d_rgb_out: *mut std::ffi::c_void,
                                   hip_stream: *mut std::ffi::c_void) -> Result<(), CodecError> {
    let n = u32::try_from(sizes.len()).unwrap_or(u32::MAX);
    check(alice_codec_dev_decode_banded(d_alc, alc_stride, sizes.as_ptr(), n, d_rgb_out, hip_stream), 0, 0)
}

/// # Safety
/// As `transcode_device`.
pub unsafe fn to_banded_device(d_alc: *const std::ffi::c_void, alc_stride: u64, sizes: &[u64], lane_symbols: u32, d_out: *mut std::ffi::c_void,
                               out_stride: u64, hip_stream: *mut std::ffi::c_void) -> Result<Vec<u64>, CodecError> {
    let mut out = vec![0u64; sizes.len()];
    let n = u32::try_from(sizes.len()).unwrap_or(u32::MAX);
    check(alice_codec_dev_to_banded(d_alc, alc_stride, sizes.as_ptr(), n, lane_symbols, d_out, out_stride, out.as_mut_ptr(), hip_stream), 0, 0)
        .map(|_| out)
}

/// # Safety
/// As `transcode_device`.
pub unsafe fn from_banded_device(d_alc: *const std::ffi::c_void, alc_stride: u64, sizes: &[u64], lane_symbols: u32, d_out: *mut std::ffi::c_void,
                                 out_stride: u64, hip_stream: *mut std::ffi::c_void) -> Result<Vec<u64>, CodecError> {
    let mut out = vec![0u64; sizes.len()];
    let n = u32::try_from(sizes.len()).unwrap_or(u32::MAX);
    check(alice_codec_dev_from_banded(d_alc, alc_stride, sizes.as_ptr(), n, lane_symbols, d_out, out_stride, out.as_mut_ptr(), hip_stream), 0, 0)
        .map(|_| out)
}

/// Stage call: the 3 x 8 x 256 u32 band histograms (`wide`: of min(z, 255)) of one chunk's 3 * padded device symbols.
///
/// # Safety
/// `d_symbols` holds the chunk's symbols and `d_hist` room for 6144 u32 on the current device.
pub unsafe fn band_histograms_device(d_symbols: *const std::ffi::c_void, width: u32, height: u32, frames: u32, wide: bool,
                                     d_hist: *mut std::ffi::c_void, hip_stream: *mut std::ffi::c_void) -> Result<(), CodecError> {
    check(alice_codec_dev_band_histograms(d_symbols, width, height, frames, wide as c_int, d_hist, hip_stream), 0, 0)
}

// ---- frame ranges and half-size previews of a version 5 chunk ----

extern "C" {
    fn alice_codec_decode_banded_frames(data: *const u8, len: u64, first: u32, count: u32, out_len: *mut u64) -> *mut u8;
    fn alice_codec_dev_decode_banded_frames(d_alc: *const std::ffi::c_void, len: u64, first: u32, count: u32,
                                            d_rgb_out: *mut std::ffi::c_void, hip_stream: *mut std::ffi::c_void) -> c_int;
    fn alice_codec_decode_banded_preview(data: *const u8, len: u64, first: u32, count: u32, out_len: *mut u64) -> *mut u8;
    fn alice_codec_dev_decode_banded_preview(d_alc: *const std::ffi::c_void, len: u64, first: u32, count: u32,
                                             d_rgb_out: *mut std::ffi::c_void, hip_stream: *mut std::ffi::c_void) -> c_int;
}

/// The RGB bytes of frames `[first, first + count)` of a version 5 container, bit for bit
/// `decode_frames(&from_banded(data, 0)?, first, count)`: of every band only the blocks that hold coefficient planes of the
/// range's window are read.  The end checks cover the blocks that are read.
pub fn decode_banded_frames(data: &[u8], first: u32, count: u32) -> Result<Vec<u8>, CodecError> {
    let mut n = 0u64;
    unsafe {
        let p = alice_codec_decode_banded_frames(data.as_ptr(), data.len() as u64, first, count, &mut n);
        if p.is_null() { Err(last_error(0, data.len(), 0, 0, 0)) } else { Ok(take(p, n)) }
    }
}

/// `decode_banded_frames` of a device-resident container of `length` bytes into `count` packed frames at `d_rgb_out`.
///
/// # Safety
/// As `frames_decode_device`.
pub unsafe fn banded_frames_decode_device(d_alc: *const std::ffi::c_void, length: u64, first: u32, count: u32,
                                          d_rgb_out: *mut std::ffi::c_void, hip_stream: *mut std::ffi::c_void)
    -> Result<(), CodecError> {
    check(alice_codec_dev_decode_banded_frames(d_alc, length, first, count, d_rgb_out, hip_stream), 0, 0)
}

/// The half-resolution RGB bytes (`count * qh * qw * 3`, `preview_dims`) of frames `[first, first + count)` of a version 5
/// container, bit for bit `decode_preview(&from_banded(data, 0)?, first, count)`: bands 0 and 4 are the low-low quadrants,
/// so only their blocks inside the window are read.
pub fn decode_banded_preview(data: &[u8], first: u32, count: u32) -> Result<Vec<u8>, CodecError> {
    let mut n = 0u64;
    unsafe {
        let p = alice_codec_decode_banded_preview(data.as_ptr(), data.len() as u64, first, count, &mut n);
        if p.is_null() { Err(last_error(0, data.len(), 0, 0, 0)) } else { Ok(take(p, n)) }
    }
}

/// `decode_banded_preview` of a device-resident container of `length` bytes into `count` packed preview frames.
///
/// # Safety
/// As `preview_decode_device`.
pub unsafe fn banded_preview_decode_device(d_alc: *const std::ffi::c_void, length: u64, first: u32, count: u32,
                                           d_rgb_out: *mut std::ffi::c_void, hip_stream: *mut std::ffi::c_void)
    -> Result<(), CodecError> {
    check(alice_codec_dev_decode_banded_preview(d_alc, length, first, count, d_rgb_out, hip_stream), 0, 0)
}
