// alice_codec.hpp -- header-only C++17 mirror of the reference's Rust API over the C ABI (alice_codec.h).
//
// The reference is a Rust crate; no Rust toolchain exists in the build image, so the host side above the
// C ABI is C++ with the reference's names, argument meaning and error behaviour (Result<T, CodecError>
// becomes a thrown alice_codec::CodecError carrying the same variant):
//   FrameEncoder::{new_, with_wavelet, encode}      src/pipeline.rs:335-507
//   FrameDecoder::{decode}                          src/pipeline.rs:519-631
//   EncodedChunk::{to_bytes, from_bytes, ...}       src/pipeline.rs:172-313
//   Wavelet1D / Wavelet2D / Wavelet3D               src/wavelet.rs:47-485
//   Quantizer / FastQuantizer                       src/quant.rs:57-359
//   to_symbols / from_symbols / build_histogram     src/quant.rs:547-600
//   FrequencyTable / RansEncoder / RansDecoder      src/rans.rs:85-389
// Everything executes on the GPU through libalice_codec.so; there is no CPU fallback.
#pragma once

#include <algorithm>
#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "alice_codec.h"

namespace alice_codec {

enum class WaveletType : uint8_t { Cdf53 = 0, Cdf97 = 1, Haar = 2 };  // src/pipeline.rs:34-41

// src/error.rs:12-23 (+ library-side conditions)
struct CodecError : std::runtime_error {
    enum Kind { InvalidBufferSize = 1, InvalidDimensions, DimensionOverflow, InvalidBitstream, InvalidQuantStep,
                ReferenceDiverges, OutOfMemory, DeviceError, NullArgument, Internal };
    Kind kind;
    CodecError(int code, const std::string& msg) : std::runtime_error(msg), kind(static_cast<Kind>(code)) {}
};

namespace detail {
[[noreturn]] inline void raise(int fallback = ALICE_ERR_INTERNAL) {
    int code = alice_codec_last_error();
    const char* m = alice_codec_last_error_message();
    throw CodecError(code ? code : fallback, m ? m : "");
}
inline void check(int rc) { if (rc != ALICE_OK) raise(rc); }
inline std::vector<uint8_t> take(uint8_t* p, uint64_t n) {
    std::vector<uint8_t> v(p, p + n);
    alice_codec_data_free64(p, n);
    return v;
}
}  // namespace detail

class EncodedChunk {
public:
    explicit EncodedChunk(::EncodedChunk* h) : h_(h) {}
    EncodedChunk(EncodedChunk&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
    EncodedChunk& operator=(EncodedChunk&& o) noexcept { reset(); h_ = std::exchange(o.h_, nullptr); return *this; }
    EncodedChunk(const EncodedChunk&) = delete;
    EncodedChunk& operator=(const EncodedChunk&) = delete;
    ~EncodedChunk() { reset(); }
    uint32_t width() const { return alice_codec_chunk_width(h_); }
    uint32_t height() const { return alice_codec_chunk_height(h_); }
    uint32_t frames() const { return alice_codec_chunk_frames(h_); }
    WaveletType wavelet_type() const { return static_cast<WaveletType>(alice_codec_chunk_wavelet(h_)); }
    size_t compressed_size() const { return alice_codec_chunk_compressed_size(h_); }
    std::vector<uint8_t> to_bytes() const {
        uint64_t n = 0;
        uint8_t* p = alice_codec_chunk_to_bytes64(h_, &n);
        if (!p) detail::raise();
        return detail::take(p, n);
    }
    static EncodedChunk from_bytes(const uint8_t* data, size_t len) {
        static const uint8_t empty = 0;
        ::EncodedChunk* h = alice_codec_chunk_from_bytes64(data ? data : &empty, len);
        if (!h) detail::raise(ALICE_ERR_INVALID_BITSTREAM);
        return EncodedChunk(h);
    }
    static EncodedChunk from_bytes(const std::vector<uint8_t>& v) { return from_bytes(v.data(), v.size()); }
    const ::EncodedChunk* handle() const { return h_; }
    static EncodedChunk adopt(::EncodedChunk* h) { return EncodedChunk(h); }   // takes ownership of a handle from the C ABI
private:
    void reset() { if (h_) alice_codec_chunk_destroy(h_); h_ = nullptr; }
    ::EncodedChunk* h_;
};

class FrameEncoder {
public:
    static FrameEncoder new_(uint8_t quality) { return FrameEncoder(quality, WaveletType::Cdf53); }
    static FrameEncoder with_wavelet(uint8_t quality, WaveletType w) { return FrameEncoder(quality, w); }
    FrameEncoder(FrameEncoder&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
    FrameEncoder(const FrameEncoder&) = delete;
    ~FrameEncoder() { if (h_) alice_codec_encoder_destroy(h_); }
    EncodedChunk encode(const uint8_t* rgb, size_t len, uint32_t width, uint32_t height, uint32_t frames) const {
        static const uint8_t empty = 0;
        ::EncodedChunk* c = alice_codec_encode64(h_, rgb ? rgb : &empty, len, width, height, frames);
        if (!c) detail::raise();
        return EncodedChunk(c);
    }
    EncodedChunk encode(const std::vector<uint8_t>& rgb, uint32_t w, uint32_t h, uint32_t f) const {
        return encode(rgb.data(), rgb.size(), w, h, f);
    }
    const ::FrameEncoder* handle() const { return h_; }
private:
    FrameEncoder(uint8_t q, WaveletType w) : h_(alice_codec_encoder_create_ex(q, static_cast<uint8_t>(w))) { if (!h_) detail::raise(); }
    ::FrameEncoder* h_;
};

struct FrameDecoder {
    static FrameDecoder new_() { return {}; }
    std::vector<uint8_t> decode(const EncodedChunk& chunk) const {
        uint64_t n = 0;
        uint8_t* p = alice_codec_decode64(chunk.handle(), &n);
        if (!p) detail::raise();
        return detail::take(p, n);
    }
};

// Many equal-shaped chunks in one call (the 64-frame chunk driver, src/pipeline.rs:461-497).  devices empty: the calling
// thread's device; otherwise chunk k runs on devices[k mod n], one host thread per entry of the list.
inline std::vector<EncodedChunk> encode_many(const FrameEncoder& enc, const std::vector<uint8_t>& rgb, uint32_t w, uint32_t h, uint32_t f,
                                             uint32_t n_chunks, const std::vector<int>& devices = {}) {
    std::vector<::EncodedChunk*> raw(n_chunks, nullptr);
    static const uint8_t empty = 0;
    const uint8_t* p = rgb.empty() ? &empty : rgb.data();
    if (devices.empty()) detail::check(alice_codec_encode_many(enc.handle(), p, rgb.size(), w, h, f, n_chunks, raw.data()));
    else detail::check(alice_codec_encode_many_devices(enc.handle(), p, rgb.size(), w, h, f, n_chunks, devices.data(),
                                                       static_cast<uint32_t>(devices.size()), raw.data()));
    std::vector<EncodedChunk> out;
    out.reserve(n_chunks);
    for (auto* c : raw) out.push_back(EncodedChunk::adopt(c));
    return out;
}
inline std::vector<uint8_t> decode_many(const std::vector<EncodedChunk>& chunks, const std::vector<int>& devices = {}) {
    if (chunks.empty()) return {};
    std::vector<const ::EncodedChunk*> raw;
    for (const auto& c : chunks) raw.push_back(c.handle());
    std::vector<uint8_t> out((size_t)chunks[0].width() * chunks[0].height() * chunks[0].frames() * 3 * chunks.size());
    static uint8_t sink = 0;
    uint8_t* p = out.empty() ? &sink : out.data();
    if (devices.empty()) detail::check(alice_codec_decode_many(raw.data(), static_cast<uint32_t>(raw.size()), p, out.size()));
    else detail::check(alice_codec_decode_many_devices(raw.data(), static_cast<uint32_t>(raw.size()), devices.data(),
                                                       static_cast<uint32_t>(devices.size()), p, out.size()));
    return out;
}

class Wavelet1D {
public:
    static Wavelet1D cdf97() { return Wavelet1D(alice_codec_wavelet1d_cdf97()); }
    static Wavelet1D cdf53() { return Wavelet1D(alice_codec_wavelet1d_cdf53()); }
    static Wavelet1D haar() { return Wavelet1D(alice_codec_wavelet1d_haar()); }
    Wavelet1D(Wavelet1D&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
    Wavelet1D(const Wavelet1D&) = delete;
    ~Wavelet1D() { if (h_) alice_codec_wavelet1d_destroy(h_); }
    void forward(std::vector<int32_t>& s) const { run(s, alice_codec_wavelet1d_forward); }
    void inverse(std::vector<int32_t>& s) const { run(s, alice_codec_wavelet1d_inverse); }
private:
    explicit Wavelet1D(::Wavelet1D* h) : h_(h) {}
    template <typename F> void run(std::vector<int32_t>& s, F fn) const {
        if (s.empty()) return;
        fn(h_, s.data(), static_cast<uint32_t>(s.size()));
        if (alice_codec_last_error()) detail::raise();
    }
    ::Wavelet1D* h_;
};

struct Wavelet2D {
    WaveletType kind = WaveletType::Cdf53;
    static Wavelet2D cdf97() { return {WaveletType::Cdf97}; }
    static Wavelet2D cdf53() { return {WaveletType::Cdf53}; }
    void forward(std::vector<int32_t>& img, size_t w, size_t h) const { detail::check(alice_codec_wavelet2d_forward((uint8_t)kind, img.data(), w, h)); }
    void inverse(std::vector<int32_t>& img, size_t w, size_t h) const { detail::check(alice_codec_wavelet2d_inverse((uint8_t)kind, img.data(), w, h)); }
};

struct Wavelet3D {
    WaveletType kind = WaveletType::Cdf53;
    static Wavelet3D cdf97() { return {WaveletType::Cdf97}; }
    static Wavelet3D cdf53() { return {WaveletType::Cdf53}; }
    void forward(std::vector<int32_t>& v, size_t w, size_t h, size_t d) const { detail::check(alice_codec_wavelet3d_forward((uint8_t)kind, v.data(), w, h, d)); }
    void inverse(std::vector<int32_t>& v, size_t w, size_t h, size_t d) const { detail::check(alice_codec_wavelet3d_inverse((uint8_t)kind, v.data(), w, h, d)); }
};

struct Quantizer {  // src/quant.rs:57-153
    int32_t step, dead_zone;
    static Quantizer new_(int32_t step) { return {step, step}; }
    static Quantizer with_dead_zone(int32_t step, int32_t dz) { return {step, dz}; }
    void quantize_buffer(const std::vector<int32_t>& in, std::vector<int32_t>& out) const {
        detail::check(alice_codec_quantize_buffer(step, dead_zone, in.data(), in.size(), out.data(), out.size()));
    }
    void dequantize_buffer(const std::vector<int32_t>& in, std::vector<int32_t>& out) const {
        detail::check(alice_codec_dequantize_buffer(step, in.data(), in.size(), out.data(), out.size()));
    }
};

enum class SubBand3D : uint8_t { LLL = 0, LLH, LHL, LHH, HLL, HLH, HHL, HHH };  // src/lib.rs:115-132
inline bool is_temporal_high(SubBand3D s) { return (static_cast<uint8_t>(s) & 1u) != 0; }          // LLH, LHH, HLH, HHH
inline bool is_dc(SubBand3D s) { return s == SubBand3D::LLL; }
inline uint8_t quant_strength(SubBand3D s) { return alice_codec_subband_quant_strength(static_cast<uint8_t>(s)); }

class AnalyticalRDO {  // src/quant.rs:377-505
public:
    static AnalyticalRDO new_(double target_bpp) { return AnalyticalRDO(target_bpp, 75); }
    static AnalyticalRDO with_quality(uint8_t quality) {
        const uint8_t q = quality > 100 ? 100 : quality;
        return AnalyticalRDO(alice_codec_rdo_target_bpp(q), q);
    }
    Quantizer compute_quantizer(const std::vector<int32_t>& coeffs, SubBand3D subband) const {
        int32_t step = 1, dz = 1;
        static const int32_t empty = 0;
        detail::check(alice_codec_rdo_compute_quantizer(target_bpp_, coeffs.empty() ? &empty : coeffs.data(), coeffs.size(),
                                                        static_cast<uint8_t>(subband), &step, &dz));
        return Quantizer::with_dead_zone(step, dz);
    }
    std::array<Quantizer, 8> compute_all_quantizers(const std::array<std::vector<int32_t>, 8>& subbands) const {
        std::array<Quantizer, 8> q{};
        for (size_t i = 0; i < 8; ++i) q[i] = compute_quantizer(subbands[i], static_cast<SubBand3D>(i));
        return q;
    }
    uint8_t quality() const { return quality_; }
    double target_bpp() const { return target_bpp_; }
private:
    AnalyticalRDO(double bpp, uint8_t q) : target_bpp_(bpp), quality_(q) {}
    double target_bpp_;
    uint8_t quality_;
};

class FastQuantizer {  // src/quant.rs:171-359
public:
    static FastQuantizer new_(int32_t step) { return FastQuantizer(alice_codec_fastquant_new(step)); }
    static FastQuantizer with_dead_zone(int32_t step, int32_t dz) { return FastQuantizer(alice_codec_fastquant_with_dead_zone(step, dz)); }
    static FastQuantizer from(const Quantizer& q) { return with_dead_zone(q.step, q.dead_zone); }
    FastQuantizer(FastQuantizer&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
    FastQuantizer(const FastQuantizer&) = delete;
    ~FastQuantizer() { if (h_) alice_codec_fastquant_destroy(h_); }
    int32_t step() const { return alice_codec_fastquant_step(h_); }
    int32_t dead_zone() const { return alice_codec_fastquant_dead_zone(h_); }
    void quantize_buffer(const std::vector<int32_t>& in, std::vector<int32_t>& out) const {
        detail::check(alice_codec_fastquant_quantize_buffer(h_, in.data(), in.size(), out.data(), out.size()));
    }
    void quantize_buffer_simd(const std::vector<int32_t>& in, std::vector<int32_t>& out) const { quantize_buffer(in, out); }
    void dequantize_buffer(const std::vector<int32_t>& in, std::vector<int32_t>& out) const {
        detail::check(alice_codec_fastquant_dequantize_buffer(h_, in.data(), in.size(), out.data(), out.size()));
    }
private:
    explicit FastQuantizer(::FastQuantizer* h) : h_(h) { if (!h_) detail::raise(ALICE_ERR_INVALID_QUANT_STEP); }
    ::FastQuantizer* h_;
};

// quantize_subband / dequantize_subband (src/quant.rs:518-545)
inline void quantize_subband(const std::vector<int32_t>& coeffs, const Quantizer& q, std::vector<int32_t>& out) {
    detail::check(alice_codec_quantize_subband(q.step, q.dead_zone, coeffs.data(), coeffs.size(), out.data(), out.size()));
}
inline void dequantize_subband(const std::vector<int32_t>& coeffs, const Quantizer& q, std::vector<int32_t>& out) {
    detail::check(alice_codec_dequantize_subband(q.step, coeffs.data(), coeffs.size(), out.data(), out.size()));
}

inline void to_symbols(const std::vector<int32_t>& coeffs, std::vector<uint8_t>& symbols) {
    detail::check(alice_codec_to_symbols(coeffs.data(), coeffs.size(), symbols.data(), symbols.size()));
}
inline void from_symbols(const std::vector<uint8_t>& symbols, std::vector<int32_t>& coeffs) {
    detail::check(alice_codec_from_symbols(symbols.data(), symbols.size(), coeffs.data(), coeffs.size()));
}
inline std::array<uint32_t, 256> build_histogram(const std::vector<uint8_t>& symbols) {
    std::array<uint32_t, 256> h{};
    static const uint8_t empty = 0;
    detail::check(alice_codec_build_histogram(symbols.empty() ? &empty : symbols.data(), symbols.size(), h.data()));
    return h;
}

struct RansSymbol {  // src/rans.rs:59-72
    uint16_t cum_freq = 0, freq = 0;
};

struct FrequencyTable {  // src/rans.rs:85-219; n symbols, 1 <= n <= 256 (entries from n on are (0, 0))
    std::array<uint16_t, 256> cum_freq{}, freq{};
    size_t n_symbols = 256;
    static FrequencyTable from_histogram(const std::vector<uint32_t>& hist) {      // any slice length (src/rans.rs:102-104)
        FrequencyTable t;
        static const uint32_t empty = 0;
        detail::check(alice_codec_freq_table_from_histogram_n(hist.empty() ? &empty : hist.data(), static_cast<uint32_t>(hist.size()),
                                                              t.cum_freq.data(), t.freq.data()));
        t.n_symbols = hist.size();
        return t;
    }
    static FrequencyTable from_histogram(const std::array<uint32_t, 256>& hist) {
        FrequencyTable t;
        detail::check(alice_codec_freq_table_from_histogram(hist.data(), t.cum_freq.data(), t.freq.data()));
        return t;
    }
    static FrequencyTable uniform(size_t n = 256) { return from_histogram(std::vector<uint32_t>(n, 0u)); }   // :158-189
    RansSymbol get_symbol(uint8_t sym) const {                                                               // :194
        if (sym >= n_symbols) detail::raise(ALICE_ERR_INVALID_DIMENSIONS);   // the reference panics
        return RansSymbol{cum_freq[sym], freq[sym]};
    }
    size_t len() const { return n_symbols; }
    bool is_empty() const { return n_symbols == 0; }
};

class RansEncoder {  // src/rans.rs:238-309: lives across calls; encode / encode_symbols continue one state
public:
    static RansEncoder new_() { return RansEncoder(); }
    static RansEncoder with_capacity(size_t) { return RansEncoder(); }   // a hint in the reference too
    RansEncoder() : h_(alice_codec_rans_encoder_new()) { if (!h_) detail::raise(); }
    RansEncoder(RansEncoder&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
    RansEncoder(const RansEncoder&) = delete;
    ~RansEncoder() { if (h_) alice_codec_rans_encoder_destroy(h_); }
    void encode(const RansSymbol& sym) { detail::check(alice_codec_rans_encoder_encode(h_, sym.cum_freq, sym.freq)); }          // :269-285
    void encode_symbols(const std::vector<uint8_t>& symbols, const FrequencyTable& table) {                                    // :288-294
        if (!symbols.empty())
            detail::check(alice_codec_rans_encoder_encode_symbols(h_, symbols.data(), symbols.size(), table.cum_freq.data(), table.freq.data()));
    }
    std::vector<uint8_t> finish() {   // :298-308, consumes the encoder
        uint64_t n = 0;
        uint8_t* p = alice_codec_rans_encoder_finish(std::exchange(h_, nullptr), &n);
        if (!p) detail::raise();
        return detail::take(p, n);
    }
private:
    AliceRansEncoder* h_;
};

class RansDecoder {  // src/rans.rs:321-389: decode / decode_n continue from the current position
public:
    explicit RansDecoder(const std::vector<uint8_t>& input) {
        static const uint8_t empty = 0;
        h_ = alice_codec_rans_decoder_new(input.empty() ? &empty : input.data(), input.size());
        if (!h_) detail::raise();
    }
    RansDecoder(RansDecoder&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
    RansDecoder(const RansDecoder&) = delete;
    ~RansDecoder() { if (h_) alice_codec_rans_decoder_destroy(h_); }
    std::vector<uint8_t> decode_n(size_t n, const FrequencyTable& table) {                                                    // :375-381
        std::vector<uint8_t> out(n);
        uint8_t sink = 0;
        detail::check(alice_codec_rans_decoder_decode_n(h_, n, table.cum_freq.data(), table.freq.data(), n ? out.data() : &sink));
        return out;
    }
    uint8_t decode(const FrequencyTable& table) { return decode_n(1, table)[0]; }                                             // :351-371
    bool is_empty() const { return alice_codec_rans_decoder_is_empty(h_) != 0; }                                             // :385-389
private:
    AliceRansDecoder* h_ = nullptr;
};

class InterleavedRansEncoder {  // src/rans.rs:393-456 (opt-in 4-stream format)
public:
    static InterleavedRansEncoder new_() { return {}; }
    void encode(const std::vector<uint8_t>& symbols, const FrequencyTable& table) { sym_ = symbols; table_ = table; }
    std::vector<uint8_t> finish() {
        uint64_t n = 0;
        static const uint8_t empty = 0;
        uint8_t* p = alice_codec_rans_encode_interleaved(sym_.empty() ? &empty : sym_.data(), sym_.size(), table_.cum_freq.data(),
                                                         table_.freq.data(), &n);
        if (!p) detail::raise();
        return detail::take(p, n);
    }
private:
    std::vector<uint8_t> sym_;
    FrequencyTable table_ = FrequencyTable{};
};

class InterleavedRansDecoder {  // src/rans.rs:468-519
public:
    explicit InterleavedRansDecoder(std::vector<uint8_t> input) : in_(std::move(input)) {}
    std::vector<uint8_t> decode_n(size_t n, const FrequencyTable& table) const {
        std::vector<uint8_t> out(n);
        static const uint8_t empty = 0;
        uint8_t sink = 0;
        detail::check(alice_codec_rans_decode_interleaved(in_.empty() ? &empty : in_.data(), in_.size(), table.cum_freq.data(),
                                                          table.freq.data(), n, n ? out.data() : &sink));
        return out;
    }
private:
    std::vector<uint8_t> in_;
};
using SimdRansDecoder = InterleavedRansDecoder;  // src/rans.rs:531-666: same format, same symbols

inline double psnr(const std::vector<uint8_t>& a, const std::vector<uint8_t>& b) {
    if (a.size() != b.size()) return -1.0;
    static const uint8_t empty = 0;
    return alice_codec_psnr(a.empty() ? &empty : a.data(), b.empty() ? &empty : b.data(), static_cast<uint32_t>(a.size()));
}

inline double ssim(const std::vector<uint8_t>& a, const std::vector<uint8_t>& b, size_t width, size_t height) {  // src/ssim.rs:63
    static const uint8_t empty = 0;
    const double v = alice_codec_ssim(a.empty() ? &empty : a.data(), a.size(), b.empty() ? &empty : b.data(), b.size(), width, height);
    if (v == -1.0 && alice_codec_last_error() != 0) detail::raise();
    return v;
}
inline double ms_ssim(const std::vector<uint8_t>& a, const std::vector<uint8_t>& b, size_t width, size_t height) {  // src/ssim.rs:125
    static const uint8_t empty = 0;
    const double v = alice_codec_ms_ssim(a.empty() ? &empty : a.data(), a.size(), b.empty() ? &empty : b.data(), b.size(), width, height);
    if (v == -1.0 && alice_codec_last_error() != 0) detail::raise();
    return v;
}

// ---- person segmentation, src/segment.rs (GPU; crop / paste are host byte copies) ----
struct SegmentConfig {  // :42-63 (min_region_size is carried and, as in the reference, unused)
    uint8_t motion_threshold = 25;
    uint32_t min_region_size = 100;
    uint32_t dilate_radius = 2;
    uint32_t erode_radius = 1;
};

inline std::vector<uint8_t> rle_encode_mask(const std::vector<uint8_t>& mask) {  // :131-154
    static const uint8_t empty = 0;
    uint64_t n = 0;
    uint8_t* p = alice_codec_rle_encode_mask(mask.empty() ? &empty : mask.data(), mask.size(), &n);
    if (!p) detail::raise();
    return detail::take(p, n);
}

struct SegmentResult {  // :78-154
    std::vector<uint8_t> mask;
    uint32_t bbox[4] = {0, 0, 0, 0};
    uint32_t foreground_count = 0;
    uint32_t width = 0, height = 0;
    float coverage() const {  // :94-101, f32 arithmetic
        const uint64_t total = (uint64_t)width * height;
        if (total > 0xFFFFFFFFull) throw CodecError(ALICE_ERR_DIMENSION_OVERFLOW, "width * height does not fit u32");
        if (total == 0) return 0.0f;
        const float inv = 1.0f / (float)total;
        return (float)foreground_count * inv;
    }
    std::vector<uint8_t> extract_person_rgb(const std::vector<uint8_t>& frame_rgb) const {  // :107-125
        static const uint8_t empty = 0;
        std::vector<uint8_t> out((size_t)3 * bbox[2] * bbox[3]);
        uint64_t n = 0;
        detail::check(alice_codec_extract_person_rgb(mask.empty() ? &empty : mask.data(), mask.size(), width, bbox,
                                                     frame_rgb.empty() ? &empty : frame_rgb.data(), frame_rgb.size(),
                                                     out.empty() ? nullptr : out.data(), out.size(), &n));
        out.resize(n);
        return out;
    }
    std::vector<uint8_t> rle_encode_mask() const { return alice_codec::rle_encode_mask(mask); }
};

inline SegmentResult segment_by_motion(const std::vector<uint8_t>& current, const std::vector<uint8_t>& reference, uint32_t width,
                                       uint32_t height, const SegmentConfig& config = SegmentConfig()) {  // :172-230
    static const uint8_t empty = 0;
    SegmentResult r;
    r.width = width; r.height = height;
    const uint64_t total = (uint64_t)width * height;
    if (total <= 0xFFFFFFFFull) r.mask.resize(total);
    detail::check(alice_codec_segment_by_motion(current.empty() ? &empty : current.data(), current.size(),
                                                reference.empty() ? &empty : reference.data(), reference.size(), width, height,
                                                config.motion_threshold, config.dilate_radius, config.erode_radius,
                                                r.mask.empty() ? nullptr : r.mask.data(), r.mask.size(), r.bbox, &r.foreground_count));
    return r;
}

// :234-265; y and co are accepted and ignored, as there
inline SegmentResult segment_by_chroma(const std::vector<int16_t>& /*y*/, const std::vector<int16_t>& /*co*/, const std::vector<int16_t>& cg,
                                       uint32_t width, uint32_t height, int16_t green_threshold) {
    static const int16_t empty = 0;
    SegmentResult r;
    r.width = width; r.height = height;
    const uint64_t total = (uint64_t)width * height;
    if (total <= 0xFFFFFFFFull) r.mask.resize(total);
    detail::check(alice_codec_segment_by_chroma(cg.empty() ? &empty : cg.data(), cg.size(), width, height, green_threshold,
                                                r.mask.empty() ? nullptr : r.mask.data(), r.mask.size(), r.bbox, &r.foreground_count));
    return r;
}

namespace detail {
// row starts of crop_to_bbox / paste_from_bbox (:273-274, :288-289): u32 arithmetic, overflow is DimensionOverflow
inline uint64_t bbox_row_start(uint32_t frame_width, const uint32_t bbox[4], uint64_t row) {
    const uint64_t s = row * frame_width + bbox[0];
    if (s > 0xFFFFFFFFull) throw CodecError(ALICE_ERR_DIMENSION_OVERFLOW, "row * frame_width + x does not fit u32");
    return s;
}
inline void bbox_rows_fit(const uint32_t bbox[4]) {
    if ((uint64_t)bbox[1] + bbox[3] > 0xFFFFFFFFull) throw CodecError(ALICE_ERR_DIMENSION_OVERFLOW, "bbox y + h does not fit u32");
}
}  // namespace detail

inline std::vector<uint8_t> crop_to_bbox(const std::vector<uint8_t>& frame, uint32_t frame_width, const uint32_t bbox[4]) {  // :269-281
    detail::bbox_rows_fit(bbox);
    std::vector<uint8_t> out;
    for (uint64_t row = bbox[1]; row < (uint64_t)bbox[1] + bbox[3]; ++row) {
        const uint64_t start = detail::bbox_row_start(frame_width, bbox, row), end = start + bbox[2];
        if (end <= frame.size()) out.insert(out.end(), frame.begin() + start, frame.begin() + end);   // a partial row is skipped
    }
    return out;
}

inline void paste_from_bbox(std::vector<uint8_t>& frame, uint32_t frame_width, const std::vector<uint8_t>& person,
                            const uint32_t bbox[4]) {  // :284-298
    detail::bbox_rows_fit(bbox);
    uint64_t src = 0;
    for (uint64_t row = bbox[1]; row < (uint64_t)bbox[1] + bbox[3]; ++row) {
        const uint64_t d0 = detail::bbox_row_start(frame_width, bbox, row), d1 = d0 + bbox[2];
        if (d1 <= frame.size() && src + bbox[2] <= person.size())
            std::copy(person.begin() + src, person.begin() + src + bbox[2], frame.begin() + d0);
        src += bbox[2];
    }
}

// ---- rate control ----
// On the GPU: the guaranteed size bracket of a chunk at the 101 qualities (alice_codec_predict_sizes) and one encode at the
// highest quality that fits a byte budget (alice_codec_encode_to_size).
struct SizePrediction {
    std::array<uint64_t, 101> lo{}, hi{};
    std::array<uint8_t, 101> status{};   // ALICE_RATE_BOUNDED / _UNBOUNDED / _DIVERGES
};
inline SizePrediction predict_sizes(const std::vector<uint8_t>& rgb, uint32_t w, uint32_t h, uint32_t f,
                                     WaveletType wt = WaveletType::Cdf53) {
    static const uint8_t empty = 0;
    SizePrediction p;
    detail::check(alice_codec_predict_sizes(static_cast<uint8_t>(wt), rgb.empty() ? &empty : rgb.data(), rgb.size(), w, h, f,
                                            p.lo.data(), p.hi.data(), p.status.data()));
    return p;
}
struct SizedChunk { EncodedChunk chunk; uint8_t quality; bool fits; };
inline SizedChunk encode_to_size(const std::vector<uint8_t>& rgb, uint32_t w, uint32_t h, uint32_t f, uint64_t max_bytes,
                                 WaveletType wt = WaveletType::Cdf53, uint8_t min_quality = 10, uint8_t max_quality = 95) {
    static const uint8_t empty = 0;
    uint8_t q = 0, fits = 0;
    ::EncodedChunk* c = alice_codec_encode_to_size(static_cast<uint8_t>(wt), rgb.empty() ? &empty : rgb.data(), rgb.size(), w, h, f,
                                                   max_bytes, min_quality, max_quality, &q, &fits);
    if (!c) detail::raise();
    return SizedChunk{EncodedChunk::adopt(c), q, fits != 0};
}

// ---- split-stream format (.alc version 2) ----
// v1 (FrameEncoder::encode, EncodedChunk) is the reference's bitstream byte for byte; v2 keeps transform, quantiser and
// symbols and codes them as independent lanes with a table that sums to 4096: for video that comes back and for the
// latency of one chunk.  EncodedChunk::from_bytes refuses v2; alc_version tells the two apart.
constexpr uint32_t SPLIT_DEFAULT_LANE_SYMBOLS = ALICE_SPLIT_DEFAULT_LANE_SYMBOLS;
constexpr uint32_t SPLIT_HEADER_BYTES = ALICE_SPLIT_HEADER_BYTES;
struct SplitInfo {   // the validated header of a version 2 container
    uint32_t width = 0, height = 0, frames = 0, lane_symbols = 0;
    WaveletType wavelet_type = WaveletType::Cdf53;
    std::array<int32_t, 3> quant_step{}, dead_zone{};
    std::array<uint32_t, 3> num_symbols{}, n_blocks{};
    std::array<uint64_t, 3> payload_len{};
};
// header parsing and validation: host code, no device needed; CodecError(InvalidBitstream) on a malformed field
inline SplitInfo split_info(const uint8_t* data, size_t len) {
    static const uint8_t empty = 0;
    AliceSplitInfo c{};
    detail::check(alice_codec_split_info(data ? data : &empty, len, &c));
    SplitInfo i;
    i.width = c.width; i.height = c.height; i.frames = c.frames; i.lane_symbols = c.lane_symbols;
    i.wavelet_type = static_cast<WaveletType>(c.wavelet);
    for (int k = 0; k < 3; ++k) {
        i.quant_step[k] = c.quant_step[k]; i.dead_zone[k] = c.dead_zone[k];
        i.num_symbols[k] = c.num_symbols[k]; i.n_blocks[k] = c.n_blocks[k]; i.payload_len[k] = c.payload_len[k];
    }
    return i;
}
inline SplitInfo split_info(const std::vector<uint8_t>& v) { return split_info(v.data(), v.size()); }
inline int alc_version(const std::vector<uint8_t>& v) { return v.size() > 4 ? v[4] : 0; }
// one chunk as version 2 bytes, with the encoder's wavelet and quality (lane_symbols 0: the default)
inline std::vector<uint8_t> encode_split(const FrameEncoder& enc, const std::vector<uint8_t>& rgb, uint32_t w, uint32_t h, uint32_t f,
                                         uint32_t lane_symbols = 0) {
    static const uint8_t empty = 0;
    uint64_t n = 0;
    uint8_t* p = alice_codec_encode_split(enc.handle(), rgb.empty() ? &empty : rgb.data(), rgb.size(), w, h, f, lane_symbols, &n);
    if (!p) detail::raise();
    return detail::take(p, n);
}
inline std::vector<uint8_t> decode_split(const std::vector<uint8_t>& data) {
    static const uint8_t empty = 0;
    uint64_t n = 0;
    uint8_t* p = alice_codec_decode_split(data.empty() ? &empty : data.data(), data.size(), &n);
    if (!p) detail::raise(ALICE_ERR_INVALID_BITSTREAM);
    return detail::take(p, n);
}
// the 256 frequencies a version 2 header stores for this histogram (sum 4096), from the table kernel
inline std::array<uint16_t, 256> normalized_frequencies(const std::array<uint32_t, 256>& histogram) {
    std::array<uint16_t, 256> f{};
    detail::check(alice_codec_split_normalize(histogram.data(), f.data()));
    return f;
}
inline uint64_t split_stream_bound(uint64_t n, uint32_t lane_symbols = SPLIT_DEFAULT_LANE_SYMBOLS) {
    return alice_codec_split_stream_bound(n, lane_symbols);
}
// n_chunks packed device chunks -> version 2 bytes at d_out + i * out_stride; returns the sizes.  qualities empty: all at
// `quality`, else one per chunk.
inline std::vector<uint64_t> split_encode_device(const void* d_rgb, uint32_t w, uint32_t h, uint32_t f, uint32_t n_chunks, WaveletType wt,
                                                 uint8_t quality, void* d_out, uint64_t out_stride,
                                                 const std::vector<uint8_t>& qualities = {}, uint32_t lane_symbols = 0,
                                                 void* hip_stream = nullptr) {
    if (!qualities.empty() && qualities.size() != n_chunks) throw CodecError(ALICE_ERR_INVALID_BUFFER_SIZE, "one quality per chunk");
    std::vector<uint64_t> sizes(n_chunks);
    detail::check(alice_codec_dev_encode_split(d_rgb, w, h, f, n_chunks, static_cast<uint8_t>(wt), quality,
                                               qualities.empty() ? nullptr : qualities.data(), lane_symbols, d_out, out_stride,
                                               sizes.data(), hip_stream));
    return sizes;
}
inline void split_decode_device(const void* d_alc, uint64_t alc_stride, const std::vector<uint64_t>& sizes, void* d_rgb_out,
                                void* hip_stream = nullptr) {
    detail::check(alice_codec_dev_decode_split(d_alc, alc_stride, sizes.data(), static_cast<uint32_t>(sizes.size()), d_rgb_out, hip_stream));
}
// ---- wide format (.alc version 3) ----
// Version 2 with an untruncated symbol (coded symbol min(z, 255), escape 255 + a 12-bit residual in the same lane chain): the
// container for the top of the quality scale, where versions 1 and 2 wrap large coefficients modulo 256.  lane_symbols: a
// power of two in [64, 8192].  The header fields are version 2's (SplitInfo); each parser refuses the other versions.
constexpr uint32_t WIDE_MAX_LANE_SYMBOLS = 8192;
inline SplitInfo wide_info(const uint8_t* data, size_t len) {
    static const uint8_t empty = 0;
    AliceSplitInfo c{};
    detail::check(alice_codec_wide_info(data ? data : &empty, len, &c));
    SplitInfo i;
    i.width = c.width; i.height = c.height; i.frames = c.frames; i.lane_symbols = c.lane_symbols;
    i.wavelet_type = static_cast<WaveletType>(c.wavelet);
    for (int k = 0; k < 3; ++k) {
        i.quant_step[k] = c.quant_step[k]; i.dead_zone[k] = c.dead_zone[k];
        i.num_symbols[k] = c.num_symbols[k]; i.n_blocks[k] = c.n_blocks[k]; i.payload_len[k] = c.payload_len[k];
    }
    return i;
}
inline SplitInfo wide_info(const std::vector<uint8_t>& v) { return wide_info(v.data(), v.size()); }
inline std::vector<uint8_t> encode_wide(const FrameEncoder& enc, const std::vector<uint8_t>& rgb, uint32_t w, uint32_t h, uint32_t f,
                                        uint32_t lane_symbols = 0) {
    static const uint8_t empty = 0;
    uint64_t n = 0;
    uint8_t* p = alice_codec_encode_wide(enc.handle(), rgb.empty() ? &empty : rgb.data(), rgb.size(), w, h, f, lane_symbols, &n);
    if (!p) detail::raise();
    return detail::take(p, n);
}
inline std::vector<uint8_t> decode_wide(const std::vector<uint8_t>& data) {
    static const uint8_t empty = 0;
    uint64_t n = 0;
    uint8_t* p = alice_codec_decode_wide(data.empty() ? &empty : data.data(), data.size(), &n);
    if (!p) detail::raise(ALICE_ERR_INVALID_BITSTREAM);
    return detail::take(p, n);
}
inline uint64_t wide_stream_bound(uint64_t n, uint32_t lane_symbols = SPLIT_DEFAULT_LANE_SYMBOLS) {
    return alice_codec_wide_stream_bound(n, lane_symbols);
}
inline std::vector<uint64_t> wide_encode_device(const void* d_rgb, uint32_t w, uint32_t h, uint32_t f, uint32_t n_chunks, WaveletType wt,
                                                uint8_t quality, void* d_out, uint64_t out_stride,
                                                const std::vector<uint8_t>& qualities = {}, uint32_t lane_symbols = 0,
                                                void* hip_stream = nullptr) {
    if (!qualities.empty() && qualities.size() != n_chunks) throw CodecError(ALICE_ERR_INVALID_BUFFER_SIZE, "one quality per chunk");
    std::vector<uint64_t> sizes(n_chunks);
    detail::check(alice_codec_dev_encode_wide(d_rgb, w, h, f, n_chunks, static_cast<uint8_t>(wt), quality,
                                              qualities.empty() ? nullptr : qualities.data(), lane_symbols, d_out, out_stride,
                                              sizes.data(), hip_stream));
    return sizes;
}
inline void wide_decode_device(const void* d_alc, uint64_t alc_stride, const std::vector<uint64_t>& sizes, void* d_rgb_out,
                               void* hip_stream = nullptr) {
    detail::check(alice_codec_dev_decode_wide(d_alc, alc_stride, sizes.data(), static_cast<uint32_t>(sizes.size()), d_rgb_out, hip_stream));
}
// ---- reversible format (.alc version 4) ----
// Version 3 whose decoder runs the forward lifting's mirror: at quality 100 (quantiser step 1) the pixels come back exactly.
// The container for lossless archival and intermediate storage; below quality 100 prefer version 3 (or 2).  The encoder is
// version 3's -- the bytes are encode_wide's except byte 4 -- so predict_wide_sizes brackets a version 4 length and
// wide_stream_bound is its stream bound; there are no byte-budget calls.  Each parser refuses the other versions.
constexpr uint8_t LOSSLESS_QUALITY = 100;
inline SplitInfo reversible_info(const uint8_t* data, size_t len) {
    static const uint8_t empty = 0;
    AliceSplitInfo c{};
    detail::check(alice_codec_reversible_info(data ? data : &empty, len, &c));
    SplitInfo i;
    i.width = c.width; i.height = c.height; i.frames = c.frames; i.lane_symbols = c.lane_symbols;
    i.wavelet_type = static_cast<WaveletType>(c.wavelet);
    for (int k = 0; k < 3; ++k) {
        i.quant_step[k] = c.quant_step[k]; i.dead_zone[k] = c.dead_zone[k];
        i.num_symbols[k] = c.num_symbols[k]; i.n_blocks[k] = c.n_blocks[k]; i.payload_len[k] = c.payload_len[k];
    }
    return i;
}
inline SplitInfo reversible_info(const std::vector<uint8_t>& v) { return reversible_info(v.data(), v.size()); }
inline std::vector<uint8_t> encode_reversible(const FrameEncoder& enc, const std::vector<uint8_t>& rgb, uint32_t w, uint32_t h, uint32_t f,
                                              uint32_t lane_symbols = 0) {
    static const uint8_t empty = 0;
    uint64_t n = 0;
    uint8_t* p = alice_codec_encode_reversible(enc.handle(), rgb.empty() ? &empty : rgb.data(), rgb.size(), w, h, f, lane_symbols, &n);
    if (!p) detail::raise();
    return detail::take(p, n);
}
inline std::vector<uint8_t> decode_reversible(const std::vector<uint8_t>& data) {
    static const uint8_t empty = 0;
    uint64_t n = 0;
    uint8_t* p = alice_codec_decode_reversible(data.empty() ? &empty : data.data(), data.size(), &n);
    if (!p) detail::raise(ALICE_ERR_INVALID_BITSTREAM);
    return detail::take(p, n);
}
// encode_reversible at quality 100: decode_reversible (or decode_alc) returns rgb exactly
inline std::vector<uint8_t> encode_lossless(const std::vector<uint8_t>& rgb, uint32_t w, uint32_t h, uint32_t f,
                                            WaveletType wt = WaveletType::Cdf53, uint32_t lane_symbols = 0) {
    return encode_reversible(FrameEncoder::with_wavelet(LOSSLESS_QUALITY, wt), rgb, w, h, f, lane_symbols);
}
inline std::vector<uint64_t> reversible_encode_device(const void* d_rgb, uint32_t w, uint32_t h, uint32_t f, uint32_t n_chunks,
                                                      WaveletType wt, uint8_t quality, void* d_out, uint64_t out_stride,
                                                      const std::vector<uint8_t>& qualities = {}, uint32_t lane_symbols = 0,
                                                      void* hip_stream = nullptr) {
    if (!qualities.empty() && qualities.size() != n_chunks) throw CodecError(ALICE_ERR_INVALID_BUFFER_SIZE, "one quality per chunk");
    std::vector<uint64_t> sizes(n_chunks);
    detail::check(alice_codec_dev_encode_reversible(d_rgb, w, h, f, n_chunks, static_cast<uint8_t>(wt), quality,
                                                    qualities.empty() ? nullptr : qualities.data(), lane_symbols, d_out, out_stride,
                                                    sizes.data(), hip_stream));
    return sizes;
}
inline std::vector<uint64_t> encode_lossless_device(const void* d_rgb, uint32_t w, uint32_t h, uint32_t f, uint32_t n_chunks, void* d_out,
                                                    uint64_t out_stride, WaveletType wt = WaveletType::Cdf53, uint32_t lane_symbols = 0,
                                                    void* hip_stream = nullptr) {
    return reversible_encode_device(d_rgb, w, h, f, n_chunks, wt, LOSSLESS_QUALITY, d_out, out_stride, {}, lane_symbols, hip_stream);
}
inline void reversible_decode_device(const void* d_alc, uint64_t alc_stride, const std::vector<uint64_t>& sizes, void* d_rgb_out,
                                     void* hip_stream = nullptr) {
    detail::check(alice_codec_dev_decode_reversible(d_alc, alc_stride, sizes.data(), static_cast<uint32_t>(sizes.size()), d_rgb_out,
                                                    hip_stream));
}
// regions of device frames (alice_codec_dev_encode_reversible_regions / _dev_decode_reversible_regions): chunk i is frames
// [i * f, (i + 1) * f) cropped to w x h at origins[2i], origins[2i + 1]; a decode writes no byte outside the rectangles
inline std::vector<uint64_t> reversible_encode_regions_device(const void* d_frames, uint32_t frame_width, uint32_t frame_height,
                                                              const std::vector<uint32_t>& origins, uint32_t w, uint32_t h, uint32_t f,
                                                              WaveletType wt, uint8_t quality, void* d_out, uint64_t out_stride,
                                                              const std::vector<uint8_t>& qualities = {}, uint32_t lane_symbols = 0,
                                                              void* hip_stream = nullptr) {
    const uint32_t n_chunks = static_cast<uint32_t>(origins.size() / 2);
    if (origins.size() % 2) throw CodecError(ALICE_ERR_INVALID_BUFFER_SIZE, "origins: one (x, y) pair per chunk");
    if (!qualities.empty() && qualities.size() != n_chunks) throw CodecError(ALICE_ERR_INVALID_BUFFER_SIZE, "one quality per chunk");
    std::vector<uint64_t> sizes(n_chunks);
    detail::check(alice_codec_dev_encode_reversible_regions(d_frames, frame_width, frame_height, origins.data(), w, h, f, n_chunks,
                                                            static_cast<uint8_t>(wt), quality,
                                                            qualities.empty() ? nullptr : qualities.data(), lane_symbols, d_out,
                                                            out_stride, sizes.data(), hip_stream));
    return sizes;
}
inline void reversible_decode_regions_device(const void* d_alc, uint64_t alc_stride, const std::vector<uint64_t>& sizes, void* d_frames_out,
                                             uint32_t frame_width, uint32_t frame_height, const std::vector<uint32_t>& origins,
                                             void* hip_stream = nullptr) {
    if (origins.size() != 2 * sizes.size()) throw CodecError(ALICE_ERR_INVALID_BUFFER_SIZE, "origins: one (x, y) pair per chunk");
    detail::check(alice_codec_dev_decode_reversible_regions(d_alc, alc_stride, sizes.data(), static_cast<uint32_t>(sizes.size()),
                                                            d_frames_out, frame_width, frame_height, origins.data(), hip_stream));
}
// the RGB bytes of a container of any version: 1 (FrameDecoder), 2 (decode_split), 3 (decode_wide) or 4 (decode_reversible)
inline std::vector<uint8_t> decode_banded(const std::vector<uint8_t>& data);   // version 5, below
inline std::vector<uint8_t> decode_alc(const std::vector<uint8_t>& data) {
    const int version = alc_version(data);
    if (version == 2) return decode_split(data);
    if (version == 3) return decode_wide(data);
    if (version == 4) return decode_reversible(data);
    if (version == 5) return decode_banded(data);
    return FrameDecoder::new_().decode(EncodedChunk::from_bytes(data));
}

// ---- frame ranges of a version 2, 3 or 4 chunk ----
// frames [first, first + count) from the blocks they need; the end checks cover the blocks that are read
struct FramesWindow { uint32_t a, b; };
inline FramesWindow frames_window(WaveletType wt, uint32_t frames, uint32_t first, uint32_t count) {
    FramesWindow w{0, 0};
    detail::check(alice_codec_frames_window(static_cast<uint8_t>(wt), frames, first, count, &w.a, &w.b));
    return w;
}
inline std::vector<uint8_t> decode_frames(const uint8_t* data, uint64_t len, uint32_t first, uint32_t count) {
    static const uint8_t empty = 0;
    uint64_t n = 0;
    uint8_t* p = alice_codec_decode_frames(data ? data : &empty, data ? len : 0, first, count, &n);
    if (!p) detail::raise(ALICE_ERR_INVALID_BITSTREAM);
    return detail::take(p, n);
}
inline std::vector<uint8_t> decode_frames(const std::vector<uint8_t>& data, uint32_t first, uint32_t count) {
    return decode_frames(data.empty() ? nullptr : data.data(), data.size(), first, count);
}
inline void frames_decode_device(const void* d_alc, uint64_t length, uint32_t first, uint32_t count, void* d_rgb_out,
                                 void* hip_stream = nullptr) {
    detail::check(alice_codec_dev_decode_frames(d_alc, length, first, count, d_rgb_out, hip_stream));
}

// ---- half-resolution preview of a version 2, 3 or 4 chunk from the low band alone ----
// count * qh * qw * 3 packed RGB bytes of frames [first, first + count), qw x qh = ceil(width / 2) x ceil(height / 2)
struct PreviewDims { uint32_t qw, qh; };
inline PreviewDims preview_dims(uint32_t width, uint32_t height) {
    PreviewDims d{0, 0};
    detail::check(alice_codec_preview_dims(width, height, &d.qw, &d.qh));
    return d;
}
inline std::vector<uint8_t> decode_preview(const uint8_t* data, uint64_t len, uint32_t first, uint32_t count) {
    static const uint8_t empty = 0;
    uint64_t n = 0;
    uint8_t* p = alice_codec_decode_preview(data ? data : &empty, data ? len : 0, first, count, &n);
    if (!p) detail::raise(ALICE_ERR_INVALID_BITSTREAM);
    return detail::take(p, n);
}
inline std::vector<uint8_t> decode_preview(const std::vector<uint8_t>& data, uint32_t first, uint32_t count) {
    return decode_preview(data.empty() ? nullptr : data.data(), data.size(), first, count);
}
inline void preview_decode_device(const void* d_alc, uint64_t length, uint32_t first, uint32_t count, void* d_rgb_out,
                                  void* hip_stream = nullptr) {
    detail::check(alice_codec_dev_decode_preview(d_alc, length, first, count, d_rgb_out, hip_stream));
}

// ---- many previews in one call ----
// All or nothing: the CodecError of a refused or damaged call starts with "item <index>: " when an item decided it.
struct PreviewRequest { const uint8_t* data; uint64_t len; uint32_t first, count; };   // host call: one item
inline std::vector<std::vector<uint8_t>> decode_previews(const std::vector<PreviewRequest>& requests) {
    std::vector<alice_codec_preview_item> items(requests.size());
    for (size_t i = 0; i < requests.size(); ++i) items[i] = alice_codec_preview_item{requests[i].data, requests[i].len, requests[i].first, requests[i].count, nullptr};
    std::vector<uint64_t> offsets(requests.size() + 1, 0);
    static const alice_codec_preview_item none{};   // (an empty vector has no data(): the count is what the library refuses)
    uint8_t* p = alice_codec_decode_previews(items.empty() ? &none : items.data(), (uint32_t)std::min<size_t>(items.size(), 0xFFFFFFFFu),
                                             offsets.data(), nullptr);
    if (!p) detail::raise(ALICE_ERR_INVALID_BITSTREAM);
    std::vector<std::vector<uint8_t>> out(requests.size());
    for (size_t i = 0; i < requests.size(); ++i) out[i].assign(p + offsets[i], p + offsets[i + 1]);
    alice_codec_data_free64(p, offsets.back());
    return out;
}
// device call: containers and outputs on the device, the items as the C ABI declares them; *bad_item as there
inline void previews_decode_device(const std::vector<alice_codec_preview_item>& items, void* hip_stream = nullptr, uint32_t* bad_item = nullptr) {
    static const alice_codec_preview_item none{};
    detail::check(alice_codec_dev_decode_previews(items.empty() ? &none : items.data(), (uint32_t)std::min<size_t>(items.size(), 0xFFFFFFFFu),
                                                  bad_item, hip_stream));
}

// ---- a spatial rectangle of a frame range of a version 2, 3 or 4 chunk ----
// the w x h pixels at (x, y) of frames [first, first + count) from the blocks they need: count * h * w * 3 packed RGB bytes,
// or (device call, non-zero pitches) pasted into a pitched surface such as full-size frames
struct Rect { uint32_t x, y, w, h; };
struct RectWindow { uint32_t xa, xb, ya, yb; };
inline RectWindow rect_window(WaveletType wt, uint32_t width, uint32_t height, const Rect& r) {
    RectWindow v{0, 0, 0, 0};
    detail::check(alice_codec_rect_window(static_cast<uint8_t>(wt), width, height, r.x, r.y, r.w, r.h, &v.xa, &v.xb, &v.ya, &v.yb));
    return v;
}
inline std::vector<uint8_t> decode_rect(const uint8_t* data, uint64_t len, uint32_t first, uint32_t count, const Rect& r) {
    static const uint8_t empty = 0;
    uint64_t n = 0;
    uint8_t* p = alice_codec_decode_rect(data ? data : &empty, data ? len : 0, first, count, r.x, r.y, r.w, r.h, &n);
    if (!p) detail::raise(ALICE_ERR_INVALID_BITSTREAM);
    return detail::take(p, n);
}
inline std::vector<uint8_t> decode_rect(const std::vector<uint8_t>& data, uint32_t first, uint32_t count, const Rect& r) {
    return decode_rect(data.empty() ? nullptr : data.data(), data.size(), first, count, r);
}
inline void rect_decode_device(const void* d_alc, uint64_t length, uint32_t first, uint32_t count, const Rect& r, void* d_rgb_out,
                               uint64_t row_pitch = 0, uint64_t frame_pitch = 0, void* hip_stream = nullptr) {
    detail::check(alice_codec_dev_decode_rect(d_alc, length, first, count, r.x, r.y, r.w, r.h, d_rgb_out, row_pitch, frame_pitch,
                                              hip_stream));
}

// ---- many frame ranges and rectangles in one call ----
// All or nothing: the CodecError of a refused or damaged call starts with "item <index>: " when an item decided it.
// host call: one item; rect {0, 0, 0, 0} is the whole frame (a frame range)
struct RectRequest { const uint8_t* data; uint64_t len; uint32_t first, count; Rect rect; };
inline std::vector<std::vector<uint8_t>> decode_rects(const std::vector<RectRequest>& requests) {
    std::vector<alice_codec_rect_item> items(requests.size());
    for (size_t i = 0; i < requests.size(); ++i) {
        const RectRequest& r = requests[i];
        items[i] = alice_codec_rect_item{r.data, r.len, r.first, r.count, r.rect.x, r.rect.y, r.rect.w, r.rect.h, nullptr, 0, 0};
    }
    std::vector<uint64_t> offsets(requests.size() + 1, 0);
    static const alice_codec_rect_item none{};   // (an empty vector has no data(): the count is what the library refuses)
    uint8_t* p = alice_codec_decode_rects(items.empty() ? &none : items.data(), (uint32_t)std::min<size_t>(items.size(), 0xFFFFFFFFu),
                                          offsets.data(), nullptr);
    if (!p) detail::raise(ALICE_ERR_INVALID_BITSTREAM);
    std::vector<std::vector<uint8_t>> out(requests.size());
    for (size_t i = 0; i < requests.size(); ++i) out[i].assign(p + offsets[i], p + offsets[i + 1]);
    alice_codec_data_free64(p, offsets.back());
    return out;
}
// device call: containers and outputs on the device, the items as the C ABI declares them (outputs disjoint: byte ranges
// apart, or boxes of one pitched surface that are); *bad_item as there
inline void rects_decode_device(const std::vector<alice_codec_rect_item>& items, void* hip_stream = nullptr, uint32_t* bad_item = nullptr) {
    static const alice_codec_rect_item none{};
    detail::check(alice_codec_dev_decode_rects(items.empty() ? &none : items.data(), (uint32_t)std::min<size_t>(items.size(), 0xFFFFFFFFu),
                                               bad_item, hip_stream));
}

// version 2 rate control: the bracket of encode_split's length at the 101 qualities (every version 2 table
// is bounded: status stays ALICE_RATE_BOUNDED) and one encode at the quality the budget rule picks -- the largest whose
// upper bound fits, refined by at most ALICE_SPLIT_REFINE_TRIALS exact size counts among the straddling qualities
inline SizePrediction predict_split_sizes(const std::vector<uint8_t>& rgb, uint32_t w, uint32_t h, uint32_t f,
                                          WaveletType wt = WaveletType::Cdf53, uint32_t lane_symbols = 0) {
    static const uint8_t empty = 0;
    SizePrediction p;
    detail::check(alice_codec_predict_split_sizes(static_cast<uint8_t>(wt), rgb.empty() ? &empty : rgb.data(), rgb.size(), w, h, f,
                                                  lane_symbols, p.lo.data(), p.hi.data()));
    return p;
}
struct SizedSplit { std::vector<uint8_t> data; uint8_t quality; bool fits; };
inline SizedSplit encode_split_to_size(const std::vector<uint8_t>& rgb, uint32_t w, uint32_t h, uint32_t f, uint64_t max_bytes,
                                       WaveletType wt = WaveletType::Cdf53, uint8_t min_quality = 10, uint8_t max_quality = 95,
                                       uint32_t lane_symbols = 0) {
    static const uint8_t empty = 0;
    uint8_t q = 0, fits = 0;
    uint64_t n = 0;
    uint8_t* p = alice_codec_encode_split_to_size(static_cast<uint8_t>(wt), rgb.empty() ? &empty : rgb.data(), rgb.size(), w, h, f,
                                                  lane_symbols, max_bytes, min_quality, max_quality, &q, &fits, &n);
    if (!p) detail::raise();
    return SizedSplit{detail::take(p, n), q, fits != 0};
}

// version 3 rate control: the same two calls for the wide container -- the bracket prices the 12-bit
// residual of every escape, the budget rule and its trial cap are version 2's, the bytes are encode_wide's at the chosen
// quality.  lane_symbols: a power of two in [64, 8192], 0 for the default.
inline SizePrediction predict_wide_sizes(const std::vector<uint8_t>& rgb, uint32_t w, uint32_t h, uint32_t f,
                                         WaveletType wt = WaveletType::Cdf53, uint32_t lane_symbols = 0) {
    static const uint8_t empty = 0;
    SizePrediction p;
    detail::check(alice_codec_predict_wide_sizes(static_cast<uint8_t>(wt), rgb.empty() ? &empty : rgb.data(), rgb.size(), w, h, f,
                                                 lane_symbols, p.lo.data(), p.hi.data()));
    return p;
}
inline SizedSplit encode_wide_to_size(const std::vector<uint8_t>& rgb, uint32_t w, uint32_t h, uint32_t f, uint64_t max_bytes,
                                      WaveletType wt = WaveletType::Cdf53, uint8_t min_quality = 10, uint8_t max_quality = 95,
                                      uint32_t lane_symbols = 0) {
    static const uint8_t empty = 0;
    uint8_t q = 0, fits = 0;
    uint64_t n = 0;
    uint8_t* p = alice_codec_encode_wide_to_size(static_cast<uint8_t>(wt), rgb.empty() ? &empty : rgb.data(), rgb.size(), w, h, f,
                                                 lane_symbols, max_bytes, min_quality, max_quality, &q, &fits, &n);
    if (!p) detail::raise();
    return SizedSplit{detail::take(p, n), q, fits != 0};
}

// The reference's buffer-model rate control (src/rate_control.rs:7-219), host only, with the Rust integer behaviour:
// u32::midpoint start, buffer half full, 30-entry history, +-0.3 thresholds with +1 / -2 steps, saturating f64 casts
// (NaN -> 0), wrapping integer casts.
struct RateControlConfig {            // :7-31
    uint32_t target_bitrate_kbps = 5000;
    double framerate = 30.0;
    uint32_t min_quality = 10, max_quality = 95;
    uint64_t buffer_size_bits = 5000ull * 1000ull * 2ull;
};
namespace detail {
inline uint64_t f64_as_u64(double x) {   // Rust `as u64`: saturating, NaN -> 0
    if (!(x > 0.0)) return 0;
    if (x >= 18446744073709551616.0) return UINT64_MAX;
    return static_cast<uint64_t>(x);
}
inline uint32_t f64_as_u32(double x) {
    if (!(x > 0.0)) return 0;
    if (x >= 4294967296.0) return UINT32_MAX;
    return static_cast<uint32_t>(x);
}
template <typename T> T clamp_or_throw(T v, T lo, T hi) {   // Ord::clamp panics on an inverted range
    if (lo > hi) throw std::invalid_argument("clamp: min > max");
    return v < lo ? lo : (v > hi ? hi : v);
}
}  // namespace detail
class RateController {                // :34-190
public:
    explicit RateController(const RateControlConfig& c)
        : config_(c), fullness_(static_cast<int64_t>(c.buffer_size_bits) / 2),
          quality_(static_cast<uint32_t>(((uint64_t)c.min_quality + c.max_quality) >> 1)) {}
    static RateController with_defaults() { return RateController(RateControlConfig{}); }
    uint64_t target_bits_per_frame() const {
        if (config_.framerate <= 0.0) return 0;
        return detail::f64_as_u64(static_cast<double>(config_.target_bitrate_kbps) * 1000.0 / config_.framerate);
    }
    uint32_t recommended_quality() const { return quality_; }
    void update(uint64_t frame_size_bits) {
        const int64_t target = static_cast<int64_t>(target_bits_per_frame());
        const int64_t buf = static_cast<int64_t>(config_.buffer_size_bits);
        fullness_ = static_cast<int64_t>(static_cast<uint64_t>(fullness_) +
                                         (static_cast<uint64_t>(target) - frame_size_bits));   // wrapping, as release Rust
        fullness_ = detail::clamp_or_throw<int64_t>(fullness_, static_cast<int64_t>(0ull - static_cast<uint64_t>(buf)), buf);
        history_.push_back(frame_size_bits);
        if (history_.size() > 30) history_.erase(history_.begin());
        ++frames_;
        const double ratio = static_cast<double>(fullness_) / static_cast<double>(config_.buffer_size_bits);
        const int32_t adj = ratio > 0.3 ? 1 : (ratio < -0.3 ? -2 : 0);
        quality_ = static_cast<uint32_t>(detail::clamp_or_throw<int32_t>(
            static_cast<int32_t>(quality_ + static_cast<uint32_t>(adj)), static_cast<int32_t>(config_.min_quality),
            static_cast<int32_t>(config_.max_quality)));
    }
    double buffer_ratio() const {
        if (config_.buffer_size_bits == 0) return 0.0;
        return static_cast<double>(fullness_) / static_cast<double>(config_.buffer_size_bits);
    }
    uint64_t average_frame_size() const {
        if (history_.empty()) return 0;
        uint64_t s = 0;
        for (uint64_t v : history_) s += v;
        return s / history_.size();
    }
    uint64_t frame_count() const { return frames_; }
    uint32_t current_quality() const { return quality_; }
    double actual_to_target_ratio() const {
        const uint64_t t = target_bits_per_frame();
        if (t == 0) return 0.0;
        return static_cast<double>(average_frame_size()) / static_cast<double>(t);
    }
private:
    RateControlConfig config_;
    int64_t fullness_;
    uint32_t quality_;
    std::vector<uint64_t> history_;
    uint64_t frames_ = 0;
};
inline uint32_t estimate_quality(uint32_t target_bitrate_kbps, uint32_t width, uint32_t height, double fps) {   // :196-219
    if (fps <= 0.0 || width == 0 || height == 0) return 50;
    const double pps = static_cast<double>(width) * static_cast<double>(height) * fps;
    const double bpp = static_cast<double>(target_bitrate_kbps) * 1000.0 / pps;
    double q;
    if (bpp > 2.0) q = 95.0;
    else if (bpp > 0.5) q = __builtin_fma(bpp, 30.0, 35.0);
    else if (bpp > 0.1) q = __builtin_fma(bpp, 75.0, 12.5);
    else q = bpp * 100.0 + 5.0;
    return detail::clamp_or_throw<uint32_t>(detail::f64_as_u32(q), 5u, 100u);
}

// quality control: exact trial distortion and PSNR-floor encodes.  `format` is the container's version
// byte (ALICE_FORMAT_SPLIT / _WIDE / _REVERSIBLE); the device pointers may have any byte alignment.
inline double psnr_from_sse(uint64_t sse, uint64_t n_bytes) { return alice_codec_psnr_from_sse(sse, n_bytes); }
struct RgbPitches { uint64_t row = 0, frame = 0; };   // 0, 0: packed
// the n_frames u64 sums land at d_frame_sse (device)
inline void rgb_sse_device(const void* d_a, const void* d_b, uint32_t w, uint32_t h, uint64_t n_frames, void* d_frame_sse,
                           RgbPitches a = {}, RgbPitches b = {}, void* hip_stream = nullptr) {
    const uint64_t row = 3ull * w, frame = row * h;
    detail::check(alice_codec_dev_rgb_sse(d_a, a.row ? a.row : row, a.frame ? a.frame : frame, d_b, b.row ? b.row : row,
                                          b.frame ? b.frame : frame, w, h, n_frames, d_frame_sse, hip_stream));
}
// per-chunk squared error of the format's decode of the format's encode (chunk i at qualities[i] when given); packed chunks,
// or regions of frame_width x frame_height frames when origins (one (x, y) pair per chunk) is not empty
inline std::vector<uint64_t> trial_sse_device(uint8_t format, const void* d_frames, uint32_t w, uint32_t h, uint32_t f, uint32_t n_chunks,
                                              WaveletType wt, uint8_t quality, const std::vector<uint8_t>& qualities = {},
                                              uint32_t frame_width = 0, uint32_t frame_height = 0,
                                              const std::vector<uint32_t>& origins = {}, void* d_frame_sse = nullptr,
                                              void* hip_stream = nullptr) {
    if (!qualities.empty() && qualities.size() != n_chunks) throw CodecError(ALICE_ERR_INVALID_BUFFER_SIZE, "one quality per chunk");
    if (!origins.empty() && origins.size() != 2 * (size_t)n_chunks) throw CodecError(ALICE_ERR_INVALID_BUFFER_SIZE, "origins: one (x, y) pair per chunk");
    std::vector<uint64_t> sse(n_chunks ? n_chunks : 1);
    detail::check(alice_codec_dev_trial_sse(format, d_frames, frame_width, frame_height, origins.empty() ? nullptr : origins.data(), w, h, f,
                                            n_chunks, static_cast<uint8_t>(wt), quality, qualities.empty() ? nullptr : qualities.data(),
                                            sse.data(), d_frame_sse, hip_stream));
    sse.resize(n_chunks);
    return sse;
}
inline std::vector<double> trial_psnr_device(uint8_t format, const void* d_frames, uint32_t w, uint32_t h, uint32_t f, uint32_t n_chunks,
                                             WaveletType wt, uint8_t quality, const std::vector<uint8_t>& qualities = {},
                                             uint32_t frame_width = 0, uint32_t frame_height = 0,
                                             const std::vector<uint32_t>& origins = {}, void* hip_stream = nullptr) {
    const std::vector<uint64_t> sse = trial_sse_device(format, d_frames, w, h, f, n_chunks, wt, quality, qualities, frame_width,
                                                       frame_height, origins, nullptr, hip_stream);
    std::vector<double> db(sse.size());
    for (size_t i = 0; i < sse.size(); ++i) db[i] = psnr_from_sse(sse[i], 3ull * w * h * f);
    return db;
}
// the lowest quality in [min_quality, max_quality] whose measured PSNR reaches min_psnr (the rule: alice_codec.h); reached is
// false when not even max_quality does (the chunk is then coded at max_quality); psnr is the measured value of the point
struct PsnrEncode { std::vector<uint8_t> data; uint8_t quality; bool reached; double psnr; };
namespace detail {
inline PsnrEncode encode_to_psnr(uint8_t format, const std::vector<uint8_t>& rgb, uint32_t w, uint32_t h, uint32_t f, double min_psnr,
                                 WaveletType wt, uint8_t min_quality, uint8_t max_quality, uint32_t lane_symbols) {
    static const uint8_t empty = 0;
    uint8_t q = 0, reached = 0;
    double db = 0.0;
    uint64_t n = 0;
    uint8_t* p = alice_codec_encode_to_psnr(format, static_cast<uint8_t>(wt), rgb.empty() ? &empty : rgb.data(), rgb.size(), w, h, f,
                                            lane_symbols, min_psnr, min_quality, max_quality, &q, &reached, &db, &n);
    if (!p) raise();
    return PsnrEncode{take(p, n), q, reached != 0, db};
}
}  // namespace detail
inline PsnrEncode encode_split_to_psnr(const std::vector<uint8_t>& rgb, uint32_t w, uint32_t h, uint32_t f, double min_psnr,
                                       WaveletType wt = WaveletType::Cdf53, uint8_t min_quality = 10, uint8_t max_quality = 95,
                                       uint32_t lane_symbols = 0) {
    return detail::encode_to_psnr(ALICE_FORMAT_SPLIT, rgb, w, h, f, min_psnr, wt, min_quality, max_quality, lane_symbols);
}
inline PsnrEncode encode_wide_to_psnr(const std::vector<uint8_t>& rgb, uint32_t w, uint32_t h, uint32_t f, double min_psnr,
                                      WaveletType wt = WaveletType::Cdf53, uint8_t min_quality = 10, uint8_t max_quality = 95,
                                      uint32_t lane_symbols = 0) {
    return detail::encode_to_psnr(ALICE_FORMAT_WIDE, rgb, w, h, f, min_psnr, wt, min_quality, max_quality, lane_symbols);
}
struct PsnrChoices { std::vector<uint8_t> chosen, reached; std::vector<double> psnr; std::vector<uint64_t> sizes; };
namespace detail {
inline PsnrChoices encode_to_psnr_device(uint8_t format, const void* d_frames, uint32_t w, uint32_t h, uint32_t f, uint32_t n_chunks,
                                         WaveletType wt, double min_psnr, void* d_out, uint64_t out_stride, uint8_t min_quality,
                                         uint8_t max_quality, uint32_t lane_symbols, uint32_t frame_width, uint32_t frame_height,
                                         const std::vector<uint32_t>& origins, void* hip_stream) {
    if (!origins.empty() && origins.size() != 2 * (size_t)n_chunks) throw CodecError(ALICE_ERR_INVALID_BUFFER_SIZE, "origins: one (x, y) pair per chunk");
    const size_t m = n_chunks ? n_chunks : 1;
    PsnrChoices c{std::vector<uint8_t>(m), std::vector<uint8_t>(m), std::vector<double>(m), std::vector<uint64_t>(m)};
    check(alice_codec_dev_encode_to_psnr(format, d_frames, frame_width, frame_height, origins.empty() ? nullptr : origins.data(), w, h, f,
                                         n_chunks, static_cast<uint8_t>(wt), lane_symbols, min_psnr, min_quality, max_quality,
                                         c.chosen.data(), c.reached.data(), c.psnr.data(), d_out, out_stride, c.sizes.data(), hip_stream));
    c.chosen.resize(n_chunks); c.reached.resize(n_chunks); c.psnr.resize(n_chunks); c.sizes.resize(n_chunks);
    return c;
}
}  // namespace detail
inline PsnrChoices split_encode_to_psnr_device(const void* d_frames, uint32_t w, uint32_t h, uint32_t f, uint32_t n_chunks, WaveletType wt,
                                               double min_psnr, void* d_out, uint64_t out_stride, uint8_t min_quality = 10,
                                               uint8_t max_quality = 95, uint32_t lane_symbols = 0, uint32_t frame_width = 0,
                                               uint32_t frame_height = 0, const std::vector<uint32_t>& origins = {},
                                               void* hip_stream = nullptr) {
    return detail::encode_to_psnr_device(ALICE_FORMAT_SPLIT, d_frames, w, h, f, n_chunks, wt, min_psnr, d_out, out_stride, min_quality,
                                         max_quality, lane_symbols, frame_width, frame_height, origins, hip_stream);
}
inline PsnrChoices wide_encode_to_psnr_device(const void* d_frames, uint32_t w, uint32_t h, uint32_t f, uint32_t n_chunks, WaveletType wt,
                                              double min_psnr, void* d_out, uint64_t out_stride, uint8_t min_quality = 10,
                                              uint8_t max_quality = 95, uint32_t lane_symbols = 0, uint32_t frame_width = 0,
                                              uint32_t frame_height = 0, const std::vector<uint32_t>& origins = {},
                                              void* hip_stream = nullptr) {
    return detail::encode_to_psnr_device(ALICE_FORMAT_WIDE, d_frames, w, h, f, n_chunks, wt, min_psnr, d_out, out_stride, min_quality,
                                         max_quality, lane_symbols, frame_width, frame_height, origins, hip_stream);
}

// ---- transcode of a version 2, 3 or 4 chunk to a lower quality or a byte budget, without pixels ----
// The chunk at `quality` from its symbols alone: a channel whose step is already at or above the target's is untouched, so a
// quality at or above the source's returns the source's bytes; from a quality-100 source the result is the direct encode's.
// lane_symbols 0 keeps the source's; out_version 0 keeps the version, 3 and 4 may be exchanged.
inline std::vector<uint8_t> transcode(const uint8_t* data, uint64_t len, uint8_t quality, uint32_t lane_symbols = 0, uint8_t out_version = 0) {
    static const uint8_t empty = 0;
    uint64_t n = 0;
    uint8_t* p = alice_codec_transcode(data ? data : &empty, data ? len : 0, quality, lane_symbols, out_version, &n);
    if (!p) detail::raise(ALICE_ERR_INVALID_BITSTREAM);
    return detail::take(p, n);
}
inline std::vector<uint8_t> transcode(const std::vector<uint8_t>& data, uint8_t quality, uint32_t lane_symbols = 0, uint8_t out_version = 0) {
    return transcode(data.empty() ? nullptr : data.data(), data.size(), quality, lane_symbols, out_version);
}
// at the quality the version 2 / 3 budget rule picks for max_bytes; the bytes are transcode's at that quality
inline SizedSplit transcode_to_size(const std::vector<uint8_t>& data, uint64_t max_bytes, uint8_t min_quality = 10, uint8_t max_quality = 95,
                                    uint32_t lane_symbols = 0, uint8_t out_version = 0) {
    static const uint8_t empty = 0;
    uint8_t q = 0, fits = 0;
    uint64_t n = 0;
    uint8_t* p = alice_codec_transcode_to_size(data.empty() ? &empty : data.data(), data.size(), lane_symbols, out_version, max_bytes,
                                               min_quality, max_quality, &q, &fits, &n);
    if (!p) detail::raise(ALICE_ERR_INVALID_BITSTREAM);
    return SizedSplit{detail::take(p, n), q, fits != 0};
}
// lo[q] <= transcode(data, q, lane_symbols).size() <= hi[q]; status is always bounded
inline SizePrediction predict_transcode_sizes(const std::vector<uint8_t>& data, uint32_t lane_symbols = 0) {
    static const uint8_t empty = 0;
    SizePrediction p;
    detail::check(alice_codec_predict_transcode_sizes(data.empty() ? &empty : data.data(), data.size(), lane_symbols, p.lo.data(), p.hi.data()));
    return p;
}
// sizes.size() device containers of one version, wavelet, shape and lane_symbols, chunk i at d_alc + i * alc_stride -> chunk i at
// qualities[i] (empty: `quality`) at d_out + i * out_stride; returns the sizes
inline std::vector<uint64_t> transcode_device(const void* d_alc, uint64_t alc_stride, const std::vector<uint64_t>& sizes, uint8_t quality,
                                              void* d_out, uint64_t out_stride, const std::vector<uint8_t>& qualities = {},
                                              uint32_t lane_symbols = 0, uint8_t out_version = 0, void* hip_stream = nullptr) {
    if (!qualities.empty() && qualities.size() != sizes.size()) throw std::invalid_argument("one quality per chunk");
    std::vector<uint64_t> out(sizes.size(), 0);
    static const uint64_t none = 0;
    detail::check(alice_codec_dev_transcode(d_alc, alc_stride, sizes.empty() ? &none : sizes.data(), (uint32_t)std::min<size_t>(sizes.size(), 0xFFFFFFFFu),
                                            quality, qualities.empty() ? nullptr : qualities.data(), lane_symbols, out_version, d_out, out_stride,
                                            out.empty() ? nullptr : out.data(), hip_stream));
    return out;
}
struct TranscodeChoices { std::vector<uint8_t> chosen, fits; std::vector<uint64_t> sizes; };
inline TranscodeChoices transcode_to_budget_device(const void* d_alc, uint64_t alc_stride, const std::vector<uint64_t>& sizes,
                                                   const std::vector<uint64_t>& budgets, void* d_out, uint64_t out_stride, uint8_t min_quality = 10,
                                                   uint8_t max_quality = 95, uint32_t lane_symbols = 0, uint8_t out_version = 0,
                                                   void* hip_stream = nullptr) {
    if (budgets.size() != sizes.size()) throw std::invalid_argument("one budget per chunk");
    TranscodeChoices c{std::vector<uint8_t>(sizes.size(), 0), std::vector<uint8_t>(sizes.size(), 0), std::vector<uint64_t>(sizes.size(), 0)};
    static const uint64_t none = 0;
    detail::check(alice_codec_dev_transcode_to_budget(d_alc, alc_stride, sizes.empty() ? &none : sizes.data(),
                                                      (uint32_t)std::min<size_t>(sizes.size(), 0xFFFFFFFFu), lane_symbols, out_version,
                                                      budgets.empty() ? &none : budgets.data(), min_quality, max_quality,
                                                      c.chosen.empty() ? nullptr : c.chosen.data(), c.fits.empty() ? nullptr : c.fits.data(), d_out,
                                                      out_stride, c.sizes.empty() ? nullptr : c.sizes.data(), hip_stream));
    return c;
}
// stage call: the map alone, n device symbols (u8; wide: u16) from d_src to d_dst (the same address, or no overlap)
inline void requant_symbols_device(const void* d_src, void* d_dst, uint64_t n, bool wide, int32_t step_from, int32_t step_to,
                                   void* d_hist = nullptr, void* hip_stream = nullptr) {
    detail::check(alice_codec_dev_requant_symbols(d_src, d_dst, n, wide ? 1 : 0, step_from, step_to, d_hist, hip_stream));
}

// ---- banded format (.alc version 5) ----
// One frequency table per wavelet subband: the pixels of the base version (2, 3 or 4) in fewer bytes at chunk sizes (the
// 12 636-byte header makes thumbnails larger).  Frame ranges, previews, rectangles, budgets and transcodes stay with the base
// versions; from_banded returns the base chunk byte for byte.
constexpr size_t BANDED_HEADER_BYTES = ALICE_BANDED_HEADER_BYTES;
struct BandedInfo {   // the validated header of a version 5 container; n_blocks / payload_len: channel-major, band ascending
    uint32_t width = 0, height = 0, frames = 0, lane_symbols = 0;
    WaveletType wavelet_type = WaveletType::Cdf53;
    uint8_t base = 2;
    int32_t quant_step[3] = {0, 0, 0}, dead_zone[3] = {0, 0, 0};
    uint32_t num_symbols[3] = {0, 0, 0}, n_blocks[24] = {};
    uint64_t payload_len[24] = {};
};
inline BandedInfo banded_info(const uint8_t* data, size_t len) {
    static const uint8_t empty = 0;
    AliceBandedInfo c{};
    detail::check(alice_codec_banded_info(data ? data : &empty, len, &c));
    BandedInfo i;
    i.width = c.width; i.height = c.height; i.frames = c.frames; i.lane_symbols = c.lane_symbols;
    i.wavelet_type = static_cast<WaveletType>(c.wavelet); i.base = c.base;
    for (int k = 0; k < 3; ++k) { i.quant_step[k] = c.quant_step[k]; i.dead_zone[k] = c.dead_zone[k]; i.num_symbols[k] = c.num_symbols[k]; }
    for (int k = 0; k < 24; ++k) { i.n_blocks[k] = c.n_blocks[k]; i.payload_len[k] = c.payload_len[k]; }
    return i;
}
inline BandedInfo banded_info(const std::vector<uint8_t>& v) { return banded_info(v.data(), v.size()); }
inline uint64_t banded_stream_bound(uint64_t n_band, uint32_t lane_symbols = 512, uint8_t base = 2) {
    return alice_codec_banded_stream_bound(n_band, lane_symbols, base);
}
inline std::vector<uint8_t> encode_banded(const FrameEncoder& enc, const std::vector<uint8_t>& rgb, uint32_t w, uint32_t h, uint32_t f,
                                          uint32_t lane_symbols = 0, uint8_t base = 2) {
    static const uint8_t empty = 0;
    uint64_t n = 0;
    uint8_t* p = alice_codec_encode_banded(enc.handle(), rgb.empty() ? &empty : rgb.data(), rgb.size(), w, h, f, lane_symbols, base, &n);
    if (!p) detail::raise();
    return detail::take(p, n);
}
inline std::vector<uint8_t> decode_banded(const std::vector<uint8_t>& data) {
    static const uint8_t empty = 0;
    uint64_t n = 0;
    uint8_t* p = alice_codec_decode_banded(data.empty() ? &empty : data.data(), data.size(), &n);
    if (!p) detail::raise(ALICE_ERR_INVALID_BITSTREAM);
    return detail::take(p, n);
}
// repack without pixels: version 2, 3 or 4 -> version 5 of that base, and back, byte for byte what the encoders write
inline std::vector<uint8_t> to_banded(const std::vector<uint8_t>& data, uint32_t lane_symbols = 0) {
    static const uint8_t empty = 0;
    uint64_t n = 0;
    uint8_t* p = alice_codec_to_banded(data.empty() ? &empty : data.data(), data.size(), lane_symbols, &n);
    if (!p) detail::raise(ALICE_ERR_INVALID_BITSTREAM);
    return detail::take(p, n);
}
inline std::vector<uint8_t> from_banded(const std::vector<uint8_t>& data, uint32_t lane_symbols = 0) {
    static const uint8_t empty = 0;
    uint64_t n = 0;
    uint8_t* p = alice_codec_from_banded(data.empty() ? &empty : data.data(), data.size(), lane_symbols, &n);
    if (!p) detail::raise(ALICE_ERR_INVALID_BITSTREAM);
    return detail::take(p, n);
}
inline std::vector<uint64_t> banded_encode_device(const void* d_rgb, uint32_t w, uint32_t h, uint32_t f, uint32_t n_chunks, WaveletType wt,
                                                  uint8_t quality, void* d_out, uint64_t out_stride, const std::vector<uint8_t>& qualities = {},
                                                  uint32_t lane_symbols = 0, uint8_t base = 2, void* hip_stream = nullptr) {
    if (!qualities.empty() && qualities.size() != n_chunks) throw CodecError(ALICE_ERR_INVALID_BUFFER_SIZE, "one quality per chunk");
    std::vector<uint64_t> sizes(n_chunks);
    detail::check(alice_codec_dev_encode_banded(d_rgb, w, h, f, n_chunks, static_cast<uint8_t>(wt), quality,
                                                qualities.empty() ? nullptr : qualities.data(), lane_symbols, base, d_out, out_stride,
                                                sizes.data(), hip_stream));
    return sizes;
}
inline void banded_decode_device(const void* d_alc, uint64_t alc_stride, const std::vector<uint64_t>& sizes, void* d_rgb_out,
                                 void* hip_stream = nullptr) {
    detail::check(alice_codec_dev_decode_banded(d_alc, alc_stride, sizes.data(), static_cast<uint32_t>(sizes.size()), d_rgb_out, hip_stream));
}
inline std::vector<uint64_t> to_banded_device(const void* d_alc, uint64_t alc_stride, const std::vector<uint64_t>& sizes, void* d_out,
                                              uint64_t out_stride, uint32_t lane_symbols = 0, void* hip_stream = nullptr) {
    std::vector<uint64_t> out(sizes.size(), 0);
    static const uint64_t none = 0;
    detail::check(alice_codec_dev_to_banded(d_alc, alc_stride, sizes.empty() ? &none : sizes.data(), (uint32_t)std::min<size_t>(sizes.size(), 0xFFFFFFFFu),
                                            lane_symbols, d_out, out_stride, out.empty() ? nullptr : out.data(), hip_stream));
    return out;
}
inline std::vector<uint64_t> from_banded_device(const void* d_alc, uint64_t alc_stride, const std::vector<uint64_t>& sizes, void* d_out,
                                                uint64_t out_stride, uint32_t lane_symbols = 0, void* hip_stream = nullptr) {
    std::vector<uint64_t> out(sizes.size(), 0);
    static const uint64_t none = 0;
    detail::check(alice_codec_dev_from_banded(d_alc, alc_stride, sizes.empty() ? &none : sizes.data(), (uint32_t)std::min<size_t>(sizes.size(), 0xFFFFFFFFu),
                                              lane_symbols, d_out, out_stride, out.empty() ? nullptr : out.data(), hip_stream));
    return out;
}
// stage call: the 3 x 8 x 256 u32 band histograms (wide: of min(z, 255)) of one chunk's 3 * padded device symbols
inline void band_histograms_device(const void* d_symbols, uint32_t w, uint32_t h, uint32_t f, bool wide, void* d_hist, void* hip_stream = nullptr) {
    detail::check(alice_codec_dev_band_histograms(d_symbols, w, h, f, wide ? 1 : 0, d_hist, hip_stream));
}
// random access into a version 5 chunk: frames [first, first + count) and their half-size preview from the blocks of the
// range's window alone, bit for bit decode_frames / decode_preview of from_banded(data)
inline std::vector<uint8_t> decode_banded_frames(const uint8_t* data, uint64_t len, uint32_t first, uint32_t count) {
    static const uint8_t empty = 0;
    uint64_t n = 0;
    uint8_t* p = alice_codec_decode_banded_frames(data ? data : &empty, data ? len : 0, first, count, &n);
    if (!p) detail::raise(ALICE_ERR_INVALID_BITSTREAM);
    return detail::take(p, n);
}
inline std::vector<uint8_t> decode_banded_frames(const std::vector<uint8_t>& data, uint32_t first, uint32_t count) {
    return decode_banded_frames(data.empty() ? nullptr : data.data(), data.size(), first, count);
}
inline void banded_frames_decode_device(const void* d_alc, uint64_t length, uint32_t first, uint32_t count, void* d_rgb_out,
                                        void* hip_stream = nullptr) {
    detail::check(alice_codec_dev_decode_banded_frames(d_alc, length, first, count, d_rgb_out, hip_stream));
}
inline std::vector<uint8_t> decode_banded_preview(const uint8_t* data, uint64_t len, uint32_t first, uint32_t count) {
    static const uint8_t empty = 0;
    uint64_t n = 0;
    uint8_t* p = alice_codec_decode_banded_preview(data ? data : &empty, data ? len : 0, first, count, &n);
    if (!p) detail::raise(ALICE_ERR_INVALID_BITSTREAM);
    return detail::take(p, n);
}
inline std::vector<uint8_t> decode_banded_preview(const std::vector<uint8_t>& data, uint32_t first, uint32_t count) {
    return decode_banded_preview(data.empty() ? nullptr : data.data(), data.size(), first, count);
}
inline void banded_preview_decode_device(const void* d_alc, uint64_t length, uint32_t first, uint32_t count, void* d_rgb_out,
                                         void* hip_stream = nullptr) {
    detail::check(alice_codec_dev_decode_banded_preview(d_alc, length, first, count, d_rgb_out, hip_stream));
}

}  // namespace alice_codec
