// C++ mirror of the version 3 rate control (include/alice_codec.hpp): the empty chunk and the argument checks, which are host
// code, one line each for tests/test_cpp_wide_rate.py to compare with the Python mirror.  Then, with a GPU, one
// encode_wide_to_size against predict_wide_sizes and encode_wide, on content whose top qualities escape.
#include <cstdio>
#include "alice_codec.hpp"
namespace ac = alice_codec;

template <typename Fn>
static void attempt(const char* name, Fn fn) {
    try {
        fn();
        std::printf("%s ok\n", name);
    } catch (const ac::CodecError& e) {
        std::printf("%s error %d\n", name, (int)e.kind);
    }
}

int main(int argc, char** argv) {
    const std::vector<uint8_t> none, rgb(4 * 4 * 2 * 3, 7), three(3, 0);
    const ac::SizePrediction p = ac::predict_wide_sizes(none, 0, 7, 3);
    std::printf("empty %llu %llu %llu %llu %d\n", (unsigned long long)p.lo[0], (unsigned long long)p.hi[0], (unsigned long long)p.lo[100],
                (unsigned long long)p.hi[100], (int)p.status[50]);
    const ac::SizedSplit a = ac::encode_wide_to_size(none, 5, 0, 2, 10000, ac::WaveletType::Haar, 20, 150, 128);
    std::printf("empty fits q=%u fits=%d n=%zu same=%d\n", a.quality, (int)a.fits, a.data.size(),
                (int)(a.data == ac::encode_wide(ac::FrameEncoder::with_wavelet(100, ac::WaveletType::Haar), none, 5, 0, 2, 128)));
    const ac::SizedSplit b = ac::encode_wide_to_size(none, 5, 0, 2, ac::SPLIT_HEADER_BYTES - 1, ac::WaveletType::Cdf53, 20, 30);
    std::printf("empty short q=%u fits=%d n=%zu\n", b.quality, (int)b.fits, b.data.size());
    attempt("overflow", [&] { ac::predict_wide_sizes(three, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, ac::WaveletType::Cdf53, 100); });
    attempt("buffer", [&] { ac::predict_wide_sizes(three, 0, 4, 4, ac::WaveletType::Cdf53, 100); });
    attempt("lane", [&] { ac::predict_wide_sizes(rgb, 4, 4, 2, ac::WaveletType::Cdf53, 100); });
    attempt("lane 16384", [&] { ac::predict_wide_sizes(rgb, 4, 4, 2, ac::WaveletType::Cdf53, 16384); });
    attempt("lane 8192", [&] { ac::predict_wide_sizes(none, 0, 4, 2, ac::WaveletType::Cdf53, 8192); });
    attempt("lane before range", [&] { ac::encode_wide_to_size(rgb, 4, 4, 2, 10000, ac::WaveletType::Cdf53, 60, 50, 100); });
    attempt("range", [&] { ac::encode_wide_to_size(none, 0, 4, 2, 10000, ac::WaveletType::Cdf53, 60, 50); });
    attempt("range above 100", [&] { ac::encode_wide_to_size(none, 0, 4, 2, 10000, ac::WaveletType::Cdf53, 200, 120); });
    if (argc > 1 && alice_codec_device_count() > 0) {
        std::vector<uint8_t> v(32 * 24 * 4 * 3);
        for (size_t i = 0; i < v.size(); ++i) v[i] = (uint8_t)((i * 37 + i / 97) & 0xFF);
        const ac::SizePrediction s = ac::predict_wide_sizes(v, 32, 24, 4, ac::WaveletType::Cdf97, 64);
        const ac::SizedSplit r = ac::encode_wide_to_size(v, 32, 24, 4, s.hi[97], ac::WaveletType::Cdf97, 10, 100, 64);
        const std::vector<uint8_t> same = ac::encode_wide(ac::FrameEncoder::with_wavelet(r.quality, ac::WaveletType::Cdf97), v, 32, 24, 4, 64);
        if (!r.fits || r.data.size() > s.hi[97] || r.quality < 97 || r.data != same || s.lo[r.quality] > r.data.size() ||
            r.data.size() > s.hi[r.quality] || ac::alc_version(r.data) != 3) {
            std::puts("DEVICE MISMATCH");
            return 1;
        }
        std::printf("device q=%u\n", r.quality);
    }
    return 0;
}
