// C++ mirror of the reversible format (include/alice_codec.hpp): the empty chunk, the parser separation and the argument
// checks, which are host code, one line each for tests/test_cpp_reversible.py to compare with the Python mirror.  Then, with
// a GPU, a lossless round trip through encode_lossless / decode_reversible and decode_alc on all four container versions.
#include <cstdio>
#include "alice_codec.hpp"
namespace ac = alice_codec;

template <typename Fn>
static void attempt(const char* name, Fn fn) {
    try {
        fn();
        std::printf("%s ok\n", name);
    } catch (const ac::CodecError& e) {
        std::printf("%s error %d: %s\n", name, (int)e.kind, e.what());
    }
}

int main(int argc, char** argv) {
    const std::vector<uint8_t> none, rgb(4 * 4 * 2 * 3, 7);
    const ac::FrameEncoder enc = ac::FrameEncoder::with_wavelet(100, ac::WaveletType::Haar);
    const std::vector<uint8_t> e4 = ac::encode_reversible(enc, none, 5, 0, 2, 128);
    std::vector<uint8_t> e3 = ac::encode_wide(enc, none, 5, 0, 2, 128);
    const ac::SplitInfo i = ac::reversible_info(e4);
    std::printf("empty n=%zu version=%d L=%u step=%d lossless=%d\n", e4.size(), ac::alc_version(e4), i.lane_symbols, i.quant_step[0],
                (int)(ac::encode_lossless(none, 5, 0, 2, ac::WaveletType::Haar, 128) == e4));
    std::printf("empty decode %zu %zu\n", ac::decode_reversible(e4).size(), ac::decode_alc(e4).size());
    e3[4] = 4;
    std::printf("bytes equal but byte 4: %d\n", (int)(e3 == e4));
    e3[4] = 3;
    attempt("v4 parser on v3", [&] { ac::reversible_info(e3); });
    attempt("v3 parser on v4", [&] { ac::wide_info(e4); });
    attempt("v2 parser on v4", [&] { ac::split_info(e4); });
    attempt("decode_reversible on v3", [&] { ac::decode_reversible(e3); });
    attempt("decode_wide on v4", [&] { ac::decode_wide(e4); });
    attempt("buffer", [&] { ac::encode_reversible(enc, std::vector<uint8_t>(3, 0), 0, 4, 4, 100); });
    attempt("lane", [&] { ac::encode_reversible(enc, rgb, 4, 4, 2, 100); });
    attempt("lane 16384", [&] { ac::encode_lossless(rgb, 4, 4, 2, ac::WaveletType::Cdf53, 16384); });
    attempt("lane 8192", [&] { ac::encode_lossless(none, 0, 4, 2, ac::WaveletType::Cdf53, 8192); });
    if (argc > 1 && alice_codec_device_count() > 0) {
        const uint32_t w = 33, h = 17, f = 5;
        std::vector<uint8_t> v((size_t)w * h * f * 3);
        for (size_t k = 0; k < v.size(); ++k) v[k] = (uint8_t)((k * 37 + k / 97 + (k % 7 == 0 ? 255 : 0)) & 0xFF);
        bool ok = true;
        for (ac::WaveletType wt : {ac::WaveletType::Cdf53, ac::WaveletType::Cdf97, ac::WaveletType::Haar}) {
            const ac::FrameEncoder e = ac::FrameEncoder::with_wavelet(100, wt);
            const std::vector<uint8_t> v4 = ac::encode_lossless(v, w, h, f, wt, 64);
            std::vector<uint8_t> v3 = ac::encode_wide(e, v, w, h, f, 64);
            const std::vector<uint8_t> v2 = ac::encode_split(e, v, w, h, f, 64);
            const std::vector<uint8_t> v1 = e.encode(v, w, h, f).to_bytes();
            ok = ok && ac::alc_version(v4) == 4 && ac::decode_reversible(v4) == v && ac::decode_alc(v4) == v;
            ok = ok && ac::decode_alc(v3) == ac::decode_wide(v3) && ac::decode_alc(v2) == ac::decode_split(v2);
            ok = ok && ac::decode_alc(v1) == ac::FrameDecoder::new_().decode(ac::EncodedChunk::from_bytes(v1));
            ok = ok && ac::decode_alc(v3) != v;      // the reference's inverse does not give the input back
            const ac::SizePrediction s = ac::predict_wide_sizes(v, w, h, f, wt, 64);
            ok = ok && s.lo[100] <= v4.size() && v4.size() <= s.hi[100];
            v3[4] = 4;
            ok = ok && v3 == v4;
        }
        if (!ok) {
            std::puts("DEVICE MISMATCH");
            return 1;
        }
        std::puts("device lossless");
    }
    return 0;
}
