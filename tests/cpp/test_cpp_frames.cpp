// C++ mirror of the frame-range calls (include/alice_codec.hpp): the window and the refusals, which are host code, one line
// each for tests/test_cpp_frames.py to compare with the Python mirror.  Then, with a GPU, one case per container version:
// decode_frames against the full decode's frames.  (The device twin needs device memory, which this program has no way to
// allocate without the HIP headers: its mirror is held to the null-argument refusal here and tested from Python.)
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
    for (ac::WaveletType wt : {ac::WaveletType::Cdf53, ac::WaveletType::Cdf97, ac::WaveletType::Haar}) {
        const ac::FramesWindow m = ac::frames_window(wt, 64, 31, 1), e = ac::frames_window(wt, 13, 12, 1), s = ac::frames_window(wt, 1, 0, 1);
        std::printf("window %d: %u %u, %u %u, %u %u\n", (int)wt, m.a, m.b, e.a, e.b, s.a, s.b);
    }
    attempt("window count 0", [&] { ac::frames_window(ac::WaveletType::Cdf53, 8, 0, 0); });
    attempt("window past the end", [&] { ac::frames_window(ac::WaveletType::Cdf53, 8, 7, 2); });
    const std::vector<uint8_t> none;
    const ac::FrameEncoder enc = ac::FrameEncoder::with_wavelet(80, ac::WaveletType::Cdf97);
    const std::vector<uint8_t> empty = ac::encode_wide(enc, none, 0, 4, 4, 64);
    attempt("empty chunk", [&] { ac::decode_frames(empty, 0, 1); });
    std::vector<uint8_t> v1 = empty;
    v1[4] = 1;
    attempt("version 1", [&] { ac::decode_frames(v1, 0, 1); });
    v1[4] = 9;
    attempt("version 9", [&] { ac::decode_frames(v1, 0, 1); });
    v1[0] = 'B';
    attempt("magic", [&] { ac::decode_frames(v1, 0, 1); });
    attempt("no data", [&] { ac::decode_frames(none, 0, 1); });
    attempt("device twin without pointers", [&] { ac::frames_decode_device(nullptr, 1630, 0, 1, nullptr); });
    if (argc > 1 && alice_codec_device_count() > 0) {
        const uint32_t w = 50, h = 38, f = 13;
        const size_t fb = (size_t)w * h * 3;
        std::vector<uint8_t> v(fb * f);
        for (size_t k = 0; k < v.size(); ++k) v[k] = (uint8_t)((k / 3 % w) * 5 + (k / fb) * 9 + (k * 2654435761u >> 28));
        bool ok = true;
        int version = 2;
        for (ac::WaveletType wt : {ac::WaveletType::Cdf97, ac::WaveletType::Cdf53, ac::WaveletType::Haar}) {
            const ac::FrameEncoder e = ac::FrameEncoder::with_wavelet(version == 4 ? 100 : 80, wt);
            const std::vector<uint8_t> blob = version == 2 ? ac::encode_split(e, v, w, h, f, 64)
                                            : version == 3 ? ac::encode_wide(e, v, w, h, f, 64) : ac::encode_reversible(e, v, w, h, f, 64);
            const std::vector<uint8_t> full = ac::decode_alc(blob);
            ok = ok && ac::alc_version(blob) == version && full.size() == v.size();
            const uint32_t ranges[4][2] = {{6, 1}, {0, 1}, {4, 5}, {0, f}};
            for (const auto& r : ranges) {
                const std::vector<uint8_t> want(full.begin() + r[0] * fb, full.begin() + (r[0] + r[1]) * fb);
                ok = ok && ac::decode_frames(blob, r[0], r[1]) == want;
                ok = ok && ac::decode_frames(blob.data(), blob.size(), r[0], r[1]) == want;
            }
            ++version;
        }
        if (!ok) {
            std::puts("DEVICE MISMATCH");
            return 1;
        }
        std::puts("device frames");
    }
    return 0;
}
