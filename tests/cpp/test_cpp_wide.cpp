// Host checks of the wide-format mirror in include/alice_codec.hpp (no device needed): wide_info and the header validation
// order on the files named on the command line, one line per file, in the format tests/test_wide_host.py produces through
// the Python mirror; the version 2 and version 1 parsers refuse every one of them.
#include <cstdio>
#include <fstream>
#include <iterator>

#include "alice_codec.hpp"

namespace ac = alice_codec;

static std::vector<uint8_t> slurp(const char* path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

int main(int argc, char** argv) {
    std::printf("bound %llu %llu %llu %llu\n", (unsigned long long)ac::wide_stream_bound(1000, 64), (unsigned long long)ac::wide_stream_bound(1000, 96),
                (unsigned long long)ac::wide_stream_bound(1000, 16384), (unsigned long long)ac::wide_stream_bound(132710400ull));
    std::printf("consts %u\n", ac::WIDE_MAX_LANE_SYMBOLS);
    for (int k = 1; k < argc; ++k) {
        const std::vector<uint8_t> data = slurp(argv[k]);
        std::printf("file %d version %d: ", k, ac::alc_version(data));
        try {
            const ac::SplitInfo i = ac::wide_info(data);
            std::printf("%ux%ux%u L=%u wavelet=%d", i.width, i.height, i.frames, i.lane_symbols, (int)i.wavelet_type);
            for (int c = 0; c < 3; ++c)
                std::printf(" [%d %d %u %u %llu]", i.quant_step[c], i.dead_zone[c], i.num_symbols[c], i.n_blocks[c],
                            (unsigned long long)i.payload_len[c]);
            std::printf("\n");
        } catch (const ac::CodecError& e) {
            std::printf("error %d: %s\n", (int)e.kind, e.what());
        }
        try {
            (void)ac::split_info(data);
            std::printf("file %d v2: accepted\n", k);
        } catch (const ac::CodecError& e) {
            std::printf("file %d v2: error %d\n", k, (int)e.kind);
        }
        try {
            (void)ac::EncodedChunk::from_bytes(data);
            std::printf("file %d v1: accepted\n", k);
        } catch (const ac::CodecError& e) {
            std::printf("file %d v1: error %d\n", k, (int)e.kind);
        }
    }
    return 0;
}
