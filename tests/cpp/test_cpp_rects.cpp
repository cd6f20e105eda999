// C++ mirror of the batched frame-range / rectangle calls (include/alice_codec.hpp): the refusals, which are host code, one
// line each for tests/test_cpp_rects.py to compare with the Python mirror.  Then, with a GPU, one batch over the three
// container versions: decode_rects of many ranges and rectangles against decode_rect and decode_frames of each.  (The device
// twin needs device memory, which this program has no way to allocate without the HIP headers: its mirror is held to the
// refusals here and tested from Python.)
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
    const ac::FrameEncoder enc = ac::FrameEncoder::with_wavelet(80, ac::WaveletType::Cdf97);
    const std::vector<uint8_t> empty = ac::encode_wide(enc, none, 0, 4, 4, 64);
    std::vector<uint8_t> v1 = empty;
    v1[4] = 1;
    const ac::Rect frame{0, 0, 0, 0}, one{0, 0, 1, 1};
    attempt("no items", [&] { ac::decode_rects({}); });
    attempt("too many items", [&] { ac::decode_rects(std::vector<ac::RectRequest>(1025, ac::RectRequest{empty.data(), empty.size(), 0, 1, frame})); });
    attempt("null data in item 1", [&] { ac::decode_rects({{empty.data(), empty.size(), 0, 1, frame}, {nullptr, 100, 0, 1, one}}); });
    attempt("empty chunk in item 0", [&] { ac::decode_rects({{empty.data(), empty.size(), 0, 1, one}}); });
    attempt("version 1 in item 2", [&] { ac::decode_rects({{v1.data(), 10, 0, 1, one}, {v1.data(), 10, 0, 1, one}, {v1.data(), v1.size(), 0, 1, one}}); });
    attempt("short data in item 0", [&] { ac::decode_rects({{v1.data(), 10, 0, 1, frame}, {v1.data(), v1.size(), 0, 1, frame}}); });
    attempt("device twin without items", [&] { ac::rects_decode_device({}); });
    {
        uint32_t bad = 7;
        std::vector<alice_codec_rect_item> items(3, alice_codec_rect_item{empty.data(), empty.size(), 0, 1, 0, 0, 0, 0, (void*)empty.data(), 0, 0});
        items[2].rgb_out = nullptr;
        attempt("device twin without an output in item 2", [&] { ac::rects_decode_device(items, nullptr, &bad); });
        std::printf("bad item %u\n", bad);
    }
    if (argc > 1 && alice_codec_device_count() > 0) {
        const uint32_t w = 50, h = 38, f = 13;
        const size_t fb = (size_t)w * h * 3;
        std::vector<uint8_t> v(fb * f);
        for (size_t k = 0; k < v.size(); ++k) v[k] = (uint8_t)((k / 3 % w) * 5 + (k / fb) * 9 + (k * 2654435761u >> 28));
        std::vector<std::vector<uint8_t>> blobs;
        int version = 2;
        for (ac::WaveletType wt : {ac::WaveletType::Cdf97, ac::WaveletType::Cdf53, ac::WaveletType::Haar}) {
            const ac::FrameEncoder e = ac::FrameEncoder::with_wavelet(version == 4 ? 100 : 80, wt);
            blobs.push_back(version == 2 ? ac::encode_split(e, v, w, h, f, 64) : version == 3 ? ac::encode_wide(e, v, w, h, f, 64)
                                                                                               : ac::encode_reversible(e, v, w, h, f, 64));
            ++version;
        }
        const uint32_t ranges[4][2] = {{6, 1}, {0, 1}, {4, 5}, {12, 1}};
        const ac::Rect rects[4] = {{0, 0, 0, 0}, {7, 5, 11, 9}, {0, 0, w, h}, {49, 37, 1, 1}};
        std::vector<ac::RectRequest> requests;
        for (const auto& b : blobs)
            for (int i = 0; i < 4; ++i) requests.push_back({b.data(), b.size(), ranges[i][0], ranges[i][1], rects[i]});
        const std::vector<std::vector<uint8_t>> got = ac::decode_rects(requests);
        bool ok = got.size() == requests.size();
        for (size_t i = 0; ok && i < requests.size(); ++i) {
            const ac::RectRequest& r = requests[i];
            ok = got[i] == (r.rect.w ? ac::decode_rect(r.data, r.len, r.first, r.count, r.rect) : ac::decode_frames(r.data, r.len, r.first, r.count));
        }
        if (!ok) {
            std::puts("DEVICE MISMATCH");
            return 1;
        }
        std::puts("device rects");
    }
    return 0;
}
