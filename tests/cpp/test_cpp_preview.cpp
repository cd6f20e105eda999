// C++ mirror of the preview calls (include/alice_codec.hpp): the dimensions and the refusals, which are host code, one line
// each for tests/test_cpp_preview.py to compare with the Python mirror.  Then, with a GPU, one case per container version:
// decode_preview of ranges against the slices of decode_preview of the whole chunk, and its size against preview_dims.  (The
// device twin needs device memory, which this program has no way to allocate without the HIP headers: its mirror is held
// to the null-argument refusal here and tested from Python.)
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
    const uint32_t sizes[4][2] = {{1, 1}, {33, 17}, {1920, 1080}, {0xFFFFFFFFu, 2}};
    for (const auto& s : sizes) {
        const ac::PreviewDims d = ac::preview_dims(s[0], s[1]);
        std::printf("dims %u %u: %u %u\n", s[0], s[1], d.qw, d.qh);
    }
    attempt("dims width 0", [&] { ac::preview_dims(0, 4); });
    attempt("dims height 0", [&] { ac::preview_dims(4, 0); });
    const std::vector<uint8_t> none;
    const ac::FrameEncoder enc = ac::FrameEncoder::with_wavelet(80, ac::WaveletType::Cdf97);
    const std::vector<uint8_t> empty = ac::encode_wide(enc, none, 0, 4, 4, 64);
    attempt("empty chunk", [&] { ac::decode_preview(empty, 0, 1); });
    std::vector<uint8_t> v1 = empty;
    v1[4] = 1;
    attempt("version 1", [&] { ac::decode_preview(v1, 0, 1); });
    v1[4] = 9;
    attempt("version 9", [&] { ac::decode_preview(v1, 0, 1); });
    v1[0] = 'B';
    attempt("magic", [&] { ac::decode_preview(v1, 0, 1); });
    attempt("no data", [&] { ac::decode_preview(none, 0, 1); });
    attempt("device twin without pointers", [&] { ac::preview_decode_device(nullptr, 1630, 0, 1, nullptr); });
    if (argc > 1 && alice_codec_device_count() > 0) {
        const uint32_t w = 50, h = 38, f = 13;
        const ac::PreviewDims d = ac::preview_dims(w, h);
        const size_t fb = (size_t)w * h * 3, qb = (size_t)d.qw * d.qh * 3;
        std::vector<uint8_t> v(fb * f);
        for (size_t k = 0; k < v.size(); ++k) v[k] = (uint8_t)((k / 3 % w) * 5 + (k / fb) * 9 + (k * 2654435761u >> 28));
        bool ok = true;
        int version = 2;
        for (ac::WaveletType wt : {ac::WaveletType::Cdf97, ac::WaveletType::Cdf53, ac::WaveletType::Haar}) {
            const ac::FrameEncoder e = ac::FrameEncoder::with_wavelet(version == 4 ? 100 : 80, wt);
            const std::vector<uint8_t> blob = version == 2 ? ac::encode_split(e, v, w, h, f, 64)
                                            : version == 3 ? ac::encode_wide(e, v, w, h, f, 64) : ac::encode_reversible(e, v, w, h, f, 64);
            const std::vector<uint8_t> whole = ac::decode_preview(blob, 0, f);
            ok = ok && ac::alc_version(blob) == version && whole.size() == qb * f;
            const uint32_t ranges[4][2] = {{6, 1}, {0, 1}, {4, 5}, {12, 1}};
            for (const auto& r : ranges) {
                const std::vector<uint8_t> want(whole.begin() + r[0] * qb, whole.begin() + (r[0] + r[1]) * qb);
                ok = ok && ac::decode_preview(blob, r[0], r[1]) == want;
                ok = ok && ac::decode_preview(blob.data(), blob.size(), r[0], r[1]) == want;
            }
            ++version;
        }
        if (!ok) {
            std::puts("DEVICE MISMATCH");
            return 1;
        }
        std::puts("device previews");
    }
    return 0;
}
