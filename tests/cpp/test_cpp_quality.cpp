// C++ mirror of the quality control (include/alice_codec.hpp): the empty chunk and the refusals, which
// are host code, one line each for tests/test_cpp_quality.py to compare with the Python mirror.  Then, with a GPU, one
// encode_wide_to_psnr / encode_split_to_psnr whose choice the test compares with the rule on the CPU oracle's numbers.
#include <cmath>
#include <cstdio>
#include <cstdlib>
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
    void* const P = reinterpret_cast<void*>(0x1000);   // never followed: every refusal below is host code
    const double inf = INFINITY;
    std::printf("psnr %.17g %.17g %d %d\n", ac::psnr_from_sse(123456789, 73728), ac::psnr_from_sse(1, 1),
                (int)std::isinf(ac::psnr_from_sse(0, 10)), (int)std::isinf(ac::psnr_from_sse(7, 0)));
    const ac::PsnrEncode a = ac::encode_wide_to_psnr(none, 5, 0, 2, inf, ac::WaveletType::Haar, 20, 150, 128);
    std::printf("empty wide q=%u reached=%d inf=%d n=%zu same=%d\n", a.quality, (int)a.reached, (int)std::isinf(a.psnr), a.data.size(),
                (int)(a.data == ac::encode_wide(ac::FrameEncoder::with_wavelet(20, ac::WaveletType::Haar), none, 5, 0, 2, 128)));
    const ac::PsnrEncode b = ac::encode_split_to_psnr(none, 0, 3, 2, 40.0);
    std::printf("empty split q=%u reached=%d n=%zu\n", b.quality, (int)b.reached, b.data.size());
    attempt("overflow", [&] { ac::encode_wide_to_psnr(three, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 30.0, ac::WaveletType::Cdf53, 10, 95, 100); });
    attempt("buffer", [&] { ac::encode_split_to_psnr(three, 0, 4, 4, 30.0, ac::WaveletType::Cdf53, 10, 95, 100); });
    attempt("lane", [&] { ac::encode_wide_to_psnr(rgb, 4, 4, 2, 30.0, ac::WaveletType::Cdf53, 60, 50, 16384); });
    attempt("range", [&] { ac::encode_split_to_psnr(rgb, 4, 4, 2, 30.0, ac::WaveletType::Cdf53, 60, 50); });
    attempt("negative", [&] { ac::encode_wide_to_psnr(rgb, 4, 4, 2, -1.0); });
    attempt("nan", [&] { ac::encode_split_to_psnr(none, 0, 4, 2, NAN); });
    attempt("range above 100", [&] { ac::encode_wide_to_psnr(none, 0, 4, 2, inf, ac::WaveletType::Cdf53, 200, 120); });
    attempt("format", [&] { ac::trial_sse_device(1, P, 8, 8, 2, 1, ac::WaveletType::Cdf53, 80); });
    attempt("trial dims", [&] { ac::trial_sse_device(ALICE_FORMAT_REVERSIBLE, P, 8, 0, 2, 1, ac::WaveletType::Cdf53, 80); });
    attempt("trial region", [&] { ac::trial_sse_device(ALICE_FORMAT_WIDE, P, 8, 8, 2, 1, ac::WaveletType::Cdf53, 80, {}, 10, 10, {3, 1}); });
    attempt("sse pitch", [&] { ac::rgb_sse_device(P, P, 4, 4, 2, P, ac::RgbPitches{11, 48}); });
    attempt("sse frame pitch", [&] { ac::rgb_sse_device(P, P, 4, 4, 2, P, {}, ac::RgbPitches{16, 59}); });
    attempt("device lossless", [&] {
        uint8_t q = 0, ok = 0; double db = 0; uint64_t n = 0;
        if (alice_codec_dev_encode_to_psnr(ALICE_FORMAT_REVERSIBLE, P, 0, 0, nullptr, 8, 8, 2, 1, 0, 0, 30.0, 10, 95, &q, &ok, &db, P, 4096, &n,
                                           nullptr) != ALICE_OK)
            throw ac::CodecError(alice_codec_last_error(), "");
    });
    attempt("device range", [&] { ac::wide_encode_to_psnr_device(P, 8, 8, 2, 1, ac::WaveletType::Cdf53, 30.0, P, 4096, 60, 50); });
    if (argc > 2 && alice_codec_device_count() > 0) {
        const double target = std::atof(argv[2]);
        const uint32_t w = 32, h = 24, f = 4;
        std::vector<uint8_t> v((size_t)w * h * f * 3);
        for (size_t i = 0; i < v.size(); ++i) v[i] = (uint8_t)((i * 37 + i / 97) & 0xFF);
        const ac::PsnrEncode wide = ac::encode_wide_to_psnr(v, w, h, f, target, ac::WaveletType::Cdf97, 10, 100, 64);
        const ac::PsnrEncode split = ac::encode_split_to_psnr(v, w, h, f, target, ac::WaveletType::Cdf97, 10, 96, 64);
        const bool same = wide.data == ac::encode_wide(ac::FrameEncoder::with_wavelet(wide.quality, ac::WaveletType::Cdf97), v, w, h, f, 64) &&
                          split.data == ac::encode_split(ac::FrameEncoder::with_wavelet(split.quality, ac::WaveletType::Cdf97), v, w, h, f, 64);
        if (!same) {
            std::puts("DEVICE MISMATCH");
            return 1;
        }
        std::printf("device wide q=%u reached=%d db=%.17g\n", wide.quality, (int)wide.reached, wide.psnr);
        std::printf("device split q=%u reached=%d db=%.17g\n", split.quality, (int)split.reached, split.psnr);
    }
    return 0;
}
