// C++ mirror of the rectangle calls (include/alice_codec.hpp): the windows and the refusals, which are host code, one line
// each for tests/test_cpp_rect.py to compare with the Python mirror.  Then, with a GPU, one case per container version:
// decode_rect of rectangles and ranges against the crop of the full decode.  (The device twin needs device memory, which
// this program has no way to allocate without the HIP headers: its mirror is held to the null-argument refusal here and
// tested from Python.)
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
    const uint32_t cases[5][6] = {{1, 1, 0, 0, 1, 1}, {33, 17, 32, 16, 1, 1}, {1920, 1080, 832, 412, 256, 256}, {1920, 1080, 0, 0, 1920, 1080},
                                  {0xFFFFFFFEu, 6, 0xFFFFFFF0u, 2, 3, 1}};
    for (ac::WaveletType wt : {ac::WaveletType::Cdf53, ac::WaveletType::Cdf97, ac::WaveletType::Haar})
        for (const auto& c : cases) {
            const ac::RectWindow v = ac::rect_window(wt, c[0], c[1], ac::Rect{c[2], c[3], c[4], c[5]});
            std::printf("window %d %u %u %u %u %u %u: %u %u %u %u\n", (int)wt, c[0], c[1], c[2], c[3], c[4], c[5], v.xa, v.xb, v.ya, v.yb);
        }
    attempt("window empty", [&] { ac::rect_window(ac::WaveletType::Cdf53, 8, 8, ac::Rect{0, 0, 0, 1}); });
    attempt("window outside", [&] { ac::rect_window(ac::WaveletType::Cdf53, 8, 8, ac::Rect{4, 0, 5, 1}); });
    attempt("window overflow", [&] { ac::rect_window(ac::WaveletType::Cdf53, 0xFFFFFFFFu, 8, ac::Rect{0, 0, 1, 1}); });
    const std::vector<uint8_t> none;
    const ac::FrameEncoder enc = ac::FrameEncoder::with_wavelet(80, ac::WaveletType::Cdf97);
    const std::vector<uint8_t> empty = ac::encode_wide(enc, none, 0, 4, 4, 64);
    const ac::Rect one{0, 0, 1, 1};
    attempt("empty chunk", [&] { ac::decode_rect(empty, 0, 1, one); });
    std::vector<uint8_t> v1 = empty;
    v1[4] = 1;
    attempt("version 1", [&] { ac::decode_rect(v1, 0, 1, one); });
    v1[4] = 9;
    attempt("version 9", [&] { ac::decode_rect(v1, 0, 1, one); });
    v1[0] = 'B';
    attempt("magic", [&] { ac::decode_rect(v1, 0, 1, one); });
    attempt("no data", [&] { ac::decode_rect(none, 0, 1, one); });
    attempt("device twin without pointers", [&] { ac::rect_decode_device(nullptr, 1630, 0, 1, one, nullptr); });
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
            const std::vector<uint8_t> whole = ac::decode_alc(blob);
            ok = ok && ac::alc_version(blob) == version && whole.size() == fb * f;
            if (version == 4) ok = ok && whole == v;
            const uint32_t ranges[4][2] = {{6, 1}, {0, 1}, {4, 5}, {12, 1}};
            const ac::Rect rects[4] = {{0, 0, w, h}, {11, 9, 17, 6}, {49, 37, 1, 1}, {0, 35, 50, 3}};
            for (const auto& r : ranges)
                for (const ac::Rect& q : rects) {
                    std::vector<uint8_t> want;
                    for (uint32_t t = r[0]; t < r[0] + r[1]; ++t)
                        for (uint32_t y = q.y; y < q.y + q.h; ++y) {
                            const size_t at = t * fb + ((size_t)y * w + q.x) * 3;
                            want.insert(want.end(), whole.begin() + at, whole.begin() + at + 3 * (size_t)q.w);
                        }
                    ok = ok && ac::decode_rect(blob, r[0], r[1], q) == want;
                    ok = ok && ac::decode_rect(blob.data(), blob.size(), r[0], r[1], q) == want;
                }
            ++version;
        }
        if (!ok) {
            std::puts("DEVICE MISMATCH");
            return 1;
        }
        std::puts("device rectangles");
    }
    return 0;
}
