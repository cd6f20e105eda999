// C++ mirror of the banded format (include/alice_codec.hpp): the empty chunk, the repack of empty chunks, the parser
// separation and the argument checks, which are host code, one line each for tests/test_cpp_banded.py to compare with the
// Python mirror.  Then, with a GPU, encode / decode / repack of bases 2, 3 and 4 against the base versions' own calls.
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
    const ac::FrameEncoder enc = ac::FrameEncoder::with_wavelet(50, ac::WaveletType::Cdf97);
    const std::vector<uint8_t> e5 = ac::encode_banded(enc, none, 5, 0, 2, 128, 3);
    const std::vector<uint8_t> e3 = ac::encode_wide(enc, none, 5, 0, 2, 128);
    const ac::BandedInfo i = ac::banded_info(e5);
    std::printf("empty n=%zu version=%d base=%d L=%u step=%d header=%zu\n", e5.size(), ac::alc_version(e5), (int)i.base, i.lane_symbols,
                i.quant_step[0], (size_t)ac::BANDED_HEADER_BYTES);
    std::printf("empty decode %zu %zu\n", ac::decode_banded(e5).size(), ac::decode_alc(e5).size());
    std::printf("empty repack %d %d %d\n", (int)(ac::to_banded(e3) == e5), (int)(ac::from_banded(e5) == e3),
                (int)(ac::from_banded(ac::to_banded(e3, 64), 128) == e3));
    std::printf("bounds %llu %llu %llu\n", (unsigned long long)ac::banded_stream_bound(4096, 64, 2),
                (unsigned long long)ac::banded_stream_bound(4097, 64, 3), (unsigned long long)ac::banded_stream_bound(1, 16384, 4));
    attempt("v5 parser on v3", [&] { ac::banded_info(e3); });
    attempt("v3 parser on v5", [&] { ac::wide_info(e5); });
    attempt("v2 parser on v5", [&] { ac::split_info(e5); });
    attempt("decode_banded on v3", [&] { ac::decode_banded(e3); });
    attempt("decode_wide on v5", [&] { ac::decode_wide(e5); });
    attempt("to_banded on v5", [&] { ac::to_banded(e5); });
    attempt("transcode on v5", [&] { ac::transcode(e5, 40); });
    attempt("buffer", [&] { ac::encode_banded(enc, std::vector<uint8_t>(3, 0), 0, 4, 4, 100, 9); });
    attempt("base", [&] { ac::encode_banded(enc, rgb, 4, 4, 2, 100, 9); });
    attempt("lane", [&] { ac::encode_banded(enc, rgb, 4, 4, 2, 100, 2); });
    attempt("lane 16384 base 3", [&] { ac::encode_banded(enc, rgb, 4, 4, 2, 16384, 3); });
    attempt("lane 16384 base 2", [&] { ac::encode_banded(enc, none, 0, 4, 2, 16384, 2); });
    if (argc > 1 && alice_codec_device_count() > 0) {
        const uint32_t w = 33, h = 17, f = 5;
        std::vector<uint8_t> v((size_t)w * h * f * 3);
        for (size_t k = 0; k < v.size(); ++k) v[k] = (uint8_t)((k * 37 + k / 97 + (k % 7 == 0 ? 255 : 0)) & 0xFF);
        bool ok = true;
        for (ac::WaveletType wt : {ac::WaveletType::Cdf53, ac::WaveletType::Cdf97, ac::WaveletType::Haar}) {
            const ac::FrameEncoder e = ac::FrameEncoder::with_wavelet(80, wt);
            const std::vector<uint8_t> v2 = ac::encode_split(e, v, w, h, f, 64), v3 = ac::encode_wide(e, v, w, h, f, 64);
            const std::vector<uint8_t> v4 = ac::encode_lossless(v, w, h, f, wt, 64);
            const std::vector<uint8_t> b2 = ac::encode_banded(e, v, w, h, f, 64, 2), b3 = ac::encode_banded(e, v, w, h, f, 64, 3);
            const std::vector<uint8_t> b4 = ac::encode_banded(ac::FrameEncoder::with_wavelet(100, wt), v, w, h, f, 64, 4);
            ok = ok && ac::alc_version(b2) == 5 && ac::banded_info(b3).base == 3 && ac::banded_info(b4).n_blocks[23] == 1;
            ok = ok && ac::decode_banded(b2) == ac::decode_split(v2) && ac::decode_alc(b3) == ac::decode_wide(v3) && ac::decode_banded(b4) == v;
            ok = ok && ac::to_banded(v2) == b2 && ac::to_banded(v3) == b3 && ac::to_banded(v4) == b4;
            ok = ok && ac::from_banded(b2) == v2 && ac::from_banded(b3) == v3 && ac::from_banded(b4) == v4;
            ok = ok && ac::to_banded(v2, 128) == ac::encode_banded(e, v, w, h, f, 128, 2) && ac::from_banded(ac::to_banded(v2, 128), 64) == v2;
        }
        if (!ok) {
            std::puts("DEVICE MISMATCH");
            return 1;
        }
        std::puts("device banded");
    }
    return 0;
}
