// C++ mirror of the frame-range and preview calls on banded chunks (include/alice_codec.hpp): the refusals, which are host
// code, one line each for tests/test_cpp_banded_partial.py to compare with the Python mirror.  Then, with a GPU, both calls
// for bases 2, 3 and 4 against the base version's calls on from_banded of the same chunk, host and device.
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
    const std::vector<uint8_t> none;
    const ac::FrameEncoder enc = ac::FrameEncoder::with_wavelet(50, ac::WaveletType::Cdf97);
    const std::vector<uint8_t> e5 = ac::encode_banded(enc, none, 5, 0, 2, 128, 3);
    const std::vector<uint8_t> e3 = ac::encode_wide(enc, none, 5, 0, 2, 128);
    std::vector<uint8_t> magic = e5, reserved = e5;
    magic[0] = 'B';
    reserved[23] = 1;
    attempt("frames of an empty chunk", [&] { ac::decode_banded_frames(e5, 0, 1); });
    attempt("preview of an empty chunk", [&] { ac::decode_banded_preview(e5, 0, 1); });
    attempt("frames count 0", [&] { ac::decode_banded_frames(e5, 1, 0); });
    attempt("preview past the end", [&] { ac::decode_banded_preview(e5, 2, 1); });
    attempt("frames on v3", [&] { ac::decode_banded_frames(e3, 0, 1); });
    attempt("preview on v3", [&] { ac::decode_banded_preview(e3, 0, 0); });
    attempt("frames bad magic", [&] { ac::decode_banded_frames(magic, 0, 0); });
    attempt("preview reserved byte", [&] { ac::decode_banded_preview(reserved, 0, 1); });
    attempt("frames cut short", [&] { ac::decode_banded_frames(std::vector<uint8_t>(e5.begin(), e5.end() - 1), 0, 1); });
    attempt("preview of nothing", [&] { ac::decode_banded_preview(none, 0, 1); });
    attempt("decode_frames on v5", [&] { ac::decode_frames(e5, 0, 1); });
    attempt("decode_preview on v5", [&] { ac::decode_preview(e5, 0, 1); });
    attempt("device frames null", [&] { ac::banded_frames_decode_device(nullptr, 100, 0, 1, nullptr); });
    attempt("device preview null", [&] { ac::banded_preview_decode_device(nullptr, 100, 0, 1, nullptr); });
    if (argc > 1 && alice_codec_device_count() > 0) {
        const uint32_t w = 33, h = 17, f = 5;
        std::vector<uint8_t> v((size_t)w * h * f * 3);
        for (size_t k = 0; k < v.size(); ++k) v[k] = (uint8_t)((k * 37 + k / 97 + (k % 7 == 0 ? 255 : 0)) & 0xFF);
        const ac::PreviewDims q = ac::preview_dims(w, h);
        bool ok = true;
        for (ac::WaveletType wt : {ac::WaveletType::Cdf53, ac::WaveletType::Cdf97, ac::WaveletType::Haar})
            for (uint8_t base : {2, 3, 4}) {
                const std::vector<uint8_t> b = ac::encode_banded(ac::FrameEncoder::with_wavelet(base == 4 ? 100 : 80, wt), v, w, h, f, 64, base);
                const std::vector<uint8_t> plain = ac::from_banded(b);
                const std::vector<uint8_t> whole = ac::decode_banded(b);
                for (uint32_t t0 = 0; t0 < f; ++t0)
                    for (uint32_t n = 1; t0 + n <= f; n += 2) {
                        const std::vector<uint8_t> fr = ac::decode_banded_frames(b, t0, n), pv = ac::decode_banded_preview(b, t0, n);
                        ok = ok && fr == ac::decode_frames(plain, t0, n) && pv == ac::decode_preview(plain, t0, n);
                        ok = ok && fr == std::vector<uint8_t>(whole.begin() + (size_t)t0 * w * h * 3, whole.begin() + (size_t)(t0 + n) * w * h * 3);
                        ok = ok && pv.size() == (size_t)n * q.qw * q.qh * 3;
                    }
            }
        if (!ok) {
            std::puts("DEVICE MISMATCH");
            return 1;
        }
        std::puts("device banded partial");
    }
    return 0;
}
