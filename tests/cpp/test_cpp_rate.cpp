// C++ mirror of the reference's rate control (include/alice_codec.hpp, src/rate_control.rs): prints the state after every
// update of a scripted series, and estimate_quality over a grid, one line each, for tests/test_cpp_rate.py to compare with
// the Python mirror.  Host only.  Then, with a GPU, one encode_to_size against predict_sizes.
#include <cmath>
#include <cstdio>
#include "alice_codec.hpp"
namespace ac = alice_codec;

static void run(const char* name, ac::RateControlConfig cfg, const std::vector<uint64_t>& sizes) {
    ac::RateController c(cfg);
    std::printf("%s start q=%u target=%llu ratio=%.17g\n", name, c.recommended_quality(), (unsigned long long)c.target_bits_per_frame(),
                c.buffer_ratio());
    for (uint64_t s : sizes) {
        c.update(s);
        std::printf("%s q=%u ratio=%.17g avg=%llu n=%llu att=%.17g\n", name, c.current_quality(), c.buffer_ratio(),
                    (unsigned long long)c.average_frame_size(), (unsigned long long)c.frame_count(), c.actual_to_target_ratio());
    }
}

int main(int argc, char** argv) {
    std::vector<uint64_t> sizes;
    for (int i = 0; i < 80; ++i) sizes.push_back((uint64_t)((i * 7919) % 23) * 40000ull + (i % 5 == 0 ? 900000ull : 0ull));
    run("default", ac::RateControlConfig{}, sizes);
    ac::RateControlConfig small; small.buffer_size_bits = 1000000; small.min_quality = 20; small.max_quality = 80;
    run("small", small, sizes);
    ac::RateControlConfig fast; fast.target_bitrate_kbps = 20000; fast.framerate = 59.94;
    run("fast", fast, sizes);
    ac::RateControlConfig zero; zero.framerate = 0.0;
    run("zero_fps", zero, {1, 2, 3});
    const double fpss[] = {0.0, -1.0, 24.0, 30.0, 60.0, 1e-9, NAN, INFINITY};
    const uint32_t kbps[] = {0, 1, 100, 1000, 5000, 20000, 100000};
    for (double fps : fpss)
        for (uint32_t k : kbps)
            std::printf("est %u %.17g %u\n", k, fps, ac::estimate_quality(k, 1920, 1080, fps));
    if (argc > 1 && alice_codec_device_count() > 0) {   // device check: encode_to_size picks what predict_sizes allows
        std::vector<uint8_t> rgb(32 * 24 * 4 * 3);
        for (size_t i = 0; i < rgb.size(); ++i) rgb[i] = (uint8_t)((i * 37 + i / 97) & 0xFF);
        const ac::SizePrediction p = ac::predict_sizes(rgb, 32, 24, 4, ac::WaveletType::Cdf97);
        const ac::SizedChunk r = ac::encode_to_size(rgb, 32, 24, 4, p.hi[60], ac::WaveletType::Cdf97, 10, 95);
        if (!r.fits || r.chunk.to_bytes().size() > p.hi[60] || r.quality < 60) { std::puts("DEVICE MISMATCH"); return 1; }
        std::printf("device q=%u\n", r.quality);
    }
    return 0;
}
