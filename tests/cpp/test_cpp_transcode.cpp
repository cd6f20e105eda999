// C++ mirror of the transcode calls (include/alice_codec.hpp): the refusals, which are host code, one line each for
// tests/test_cpp_transcode.py to compare with the Python mirror.  Then, with a GPU, one case per container version: the
// identities of a transcode (a finer target returns the source, a step-1 source gives the direct encode, lanes and the version
// byte change on the way, the brackets hold, the budget is met).  (The device twins need device memory, which this program
// has no way to allocate without the HIP headers: their mirrors are held to the null-argument refusal here and tested from
// Python.)
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
    const std::vector<uint8_t> empty3 = ac::encode_wide(enc, none, 0, 4, 4, 64);
    const std::vector<uint8_t> empty2 = ac::encode_split(enc, none, 0, 4, 4, 64);
    const std::vector<uint8_t> empty4 = ac::encode_reversible(enc, none, 0, 4, 4, 64);
    attempt("empty chunk", [&] {
        const std::vector<uint8_t> out = ac::transcode(empty3, 50, 128, 4);
        std::printf("empty chunk: %zu bytes, version %d, lanes %u, step %d\n", out.size(), ac::alc_version(out),
                    ac::reversible_info(out).lane_symbols, ac::reversible_info(out).quant_step[0]);
    });
    attempt("empty chunk kept", [&] { std::printf("kept %d\n", (int)(ac::transcode(empty2, 90) == empty2)); });
    attempt("empty chunk budget", [&] {
        const ac::SizedSplit s = ac::transcode_to_size(empty3, 1630, 10, 95);
        std::printf("budget: %zu bytes, quality %d, fits %d\n", s.data.size(), (int)s.quality, (int)s.fits);
    });
    attempt("empty chunk brackets", [&] {
        const ac::SizePrediction p = ac::predict_transcode_sizes(empty4);
        std::printf("brackets: %llu %llu\n", (unsigned long long)p.lo[0], (unsigned long long)p.hi[100]);
    });
    std::vector<uint8_t> bad = empty3;
    bad[4] = 1;
    attempt("version 1", [&] { ac::transcode(bad, 50); });
    attempt("version 1 budget", [&] { ac::transcode_to_size(bad, 5000); });
    attempt("version 1 brackets", [&] { ac::predict_transcode_sizes(bad); });
    bad[4] = 9;
    attempt("version 9", [&] { ac::transcode(bad, 50); });
    bad[0] = 'B';
    attempt("magic", [&] { ac::transcode(bad, 50); });
    attempt("no data", [&] { ac::transcode(none, 50); });
    bad = empty3;
    bad[5] = 3;
    attempt("wavelet byte", [&] { ac::transcode(bad, 50); });
    bad = empty3;
    bad.resize(1629);
    attempt("truncated header", [&] { ac::transcode(bad, 50); });
    attempt("lanes 100", [&] { ac::transcode(empty3, 50, 100); });
    attempt("lanes 16384 wide", [&] { ac::transcode(empty3, 50, 16384); });
    attempt("lanes 16384 split", [&] { ac::transcode(empty2, 50, 16384); });
    attempt("version 2 to 3", [&] { ac::transcode(empty2, 50, 0, 3); });
    attempt("version 2 to 2", [&] { ac::transcode(empty2, 50, 0, 2); });
    attempt("version 3 to 2", [&] { ac::transcode(empty3, 50, 0, 2); });
    attempt("version 4 to 5", [&] { ac::transcode(empty4, 50, 0, 5); });
    attempt("quality range", [&] { ac::transcode_to_size(empty3, 5000, 50, 40); });
    attempt("version 4 budget", [&] { ac::transcode_to_size(empty4, 5000); });
    attempt("version 3 to 4 budget", [&] { ac::transcode_to_size(empty3, 5000, 10, 95, 0, 4); });
    attempt("version 4 to 3 budget", [&] { ac::transcode_to_size(empty4, 5000, 10, 95, 0, 3); });
    attempt("device twin without pointers", [&] { ac::transcode_device(nullptr, 0, {1630}, 50, nullptr, 0); });
    attempt("budget twin without pointers", [&] { ac::transcode_to_budget_device(nullptr, 0, {1630}, {5000}, nullptr, 0); });
    attempt("stage call without pointers", [&] { ac::requant_symbols_device(nullptr, nullptr, 4, false, 1, 2); });
    attempt("stage call steps", [&] { ac::requant_symbols_device(&bad, &bad, 4, false, 1, 65); });
    if (argc > 1 && alice_codec_device_count() > 0) {
        const uint32_t w = 50, h = 38, f = 5;
        const size_t fb = (size_t)w * h * 3;
        std::vector<uint8_t> v(fb * f);
        for (size_t k = 0; k < v.size(); ++k) v[k] = (uint8_t)((k / 3 % w) * 5 + (k / fb) * 9 + (k * 2654435761u >> 28));
        bool ok = true;
        int version = 2;
        for (ac::WaveletType wt : {ac::WaveletType::Cdf97, ac::WaveletType::Cdf53, ac::WaveletType::Haar}) {
            auto encode = [&](int ver, uint8_t q, uint32_t lanes) {
                const ac::FrameEncoder e = ac::FrameEncoder::with_wavelet(q, wt);
                return ver == 2 ? ac::encode_split(e, v, w, h, f, lanes) : ver == 3 ? ac::encode_wide(e, v, w, h, f, lanes)
                                                                                  : ac::encode_reversible(e, v, w, h, f, lanes);
            };
            const std::vector<uint8_t> src = encode(version, 90, 64);
            ok = ok && ac::transcode(src, 89) == src && ac::transcode(src, 100) == src;         // the same step; a finer target
            const std::vector<uint8_t> low = ac::transcode(src, 40);
            ok = ok && low.size() < src.size() && ac::alc_version(low) == version && ac::decode_alc(low).size() == fb * f;
            ok = ok && ac::transcode(ac::transcode(src, 40, 256), 40, 64) == low;                // laned again, and back
            const ac::SizePrediction p = ac::predict_transcode_sizes(src);
            ok = ok && p.lo[40] <= low.size() && low.size() <= p.hi[40] && p.lo[95] <= src.size() && src.size() <= p.hi[95];
            if (version >= 3) {
                const std::vector<uint8_t> top = encode(version, 100, 64);                      // a step-1 source: the direct encode
                ok = ok && ac::transcode(top, 70) == encode(version, 70, 64);
                ok = ok && ac::transcode(top, 70, 0, (uint8_t)(7 - version)) == encode(7 - version, 70, 64);
            }
            if (version != 4) {
                const ac::SizedSplit s = ac::transcode_to_size(src, low.size(), 10, 95);
                ok = ok && s.fits && s.quality >= 40 && s.data.size() <= low.size() && s.data == ac::transcode(src, s.quality);
            }
            ++version;
        }
        if (!ok) {
            std::puts("DEVICE MISMATCH");
            return 1;
        }
        std::puts("device transcodes");
    }
    return 0;
}
