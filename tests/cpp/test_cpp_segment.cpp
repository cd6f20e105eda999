// C++ mirror of person segmentation (include/alice_codec.hpp, reference src/segment.rs) exercised the way the
// reference's inline tests use it (:443-781).  Host-side checks (validation, crop / paste) run without a GPU; the
// walk-through runs on the device.  Prints "CPP SEGMENT OK" on success.  Links against libalice_codec.so only.
#include <cstdio>
#include "alice_codec.hpp"
namespace ac = alice_codec;
using ac::CodecError;
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "CHECK failed: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

int main() {
    const bool have_gpu = alice_codec_device_count() > 0;
    ac::SegmentConfig def;
    CHECK(def.motion_threshold == 25 && def.min_region_size == 100 && def.dilate_radius == 2 && def.erode_radius == 1);
    try { ac::segment_by_motion(std::vector<uint8_t>(99), std::vector<uint8_t>(100), 10, 10); CHECK(false); }
    catch (const CodecError& e) { CHECK(e.kind == CodecError::InvalidBufferSize); }
    try { ac::segment_by_chroma({}, {}, std::vector<int16_t>(49), 10, 5, 30); CHECK(false); }
    catch (const CodecError& e) { CHECK(e.kind == CodecError::InvalidBufferSize); }
    try { ac::segment_by_motion(std::vector<uint8_t>(1), std::vector<uint8_t>(1), 65536, 65536); CHECK(false); }
    catch (const CodecError& e) { CHECK(e.kind == CodecError::DimensionOverflow); }
    {   // crop / paste, :521-542, and the partial-row rule
        std::vector<uint8_t> frame(100, 0);
        for (int y = 2; y < 5; ++y) for (int x = 3; x < 7; ++x) frame[y * 10 + x] = 100;
        const uint32_t bbox[4] = {3, 2, 4, 3};
        auto crop = ac::crop_to_bbox(frame, 10, bbox);
        CHECK(crop.size() == 12);
        std::vector<uint8_t> restored(100, 0);
        ac::paste_from_bbox(restored, 10, crop, bbox);
        CHECK(restored == frame);
        const uint32_t partial[4] = {3, 3, 3, 3};
        std::vector<uint8_t> f30(30);
        for (int i = 0; i < 30; ++i) f30[i] = (uint8_t)i;
        CHECK((ac::crop_to_bbox(f30, 6, partial) == std::vector<uint8_t>{21, 22, 23, 27, 28, 29}));
        ac::SegmentResult empty;
        CHECK(empty.coverage() == 0.0f && empty.rle_encode_mask().empty());
    }
    if (!have_gpu) {
        try { ac::segment_by_motion(std::vector<uint8_t>(100), std::vector<uint8_t>(100), 10, 10); CHECK(false); }
        catch (const CodecError& e) { CHECK(e.kind == CodecError::DeviceError); }   // no CPU fallback
        std::puts("CPP SEGMENT OK (host-only checks; no GPU present)");
        return 0;
    }
    {   // :448-471 and :474-497
        std::vector<uint8_t> cur(200, 0), ref(200, 0);
        for (int y = 3; y < 7; ++y) for (int x = 5; x < 15; ++x) cur[y * 20 + x] = 200;
        ac::SegmentConfig c; c.motion_threshold = 50; c.dilate_radius = 0; c.erode_radius = 0;
        auto r = ac::segment_by_motion(cur, ref, 20, 10, c);
        CHECK(r.foreground_count == 40 && r.bbox[0] == 5 && r.bbox[1] == 3 && r.bbox[2] == 10 && r.bbox[3] == 4);
        CHECK(r.coverage() > 0.0f && r.coverage() < 0.5f);
        std::vector<uint8_t> cur2(600, 0);
        for (int y = 5; y < 15; ++y) for (int x = 8; x < 22; ++x) cur2[y * 30 + x] = 180;
        ac::SegmentConfig c2; c2.motion_threshold = 30;
        auto r2 = ac::segment_by_motion(cur2, std::vector<uint8_t>(600, 0), 30, 20, c2);
        CHECK(r2.coverage() > 0.1f && r2.coverage() < 0.8f);
        // erosion never eats in from the frame border
        ac::SegmentConfig c3; c3.motion_threshold = 0; c3.dilate_radius = 0; c3.erode_radius = 0xFFFFFFFFu;
        CHECK(ac::segment_by_motion(std::vector<uint8_t>(35, 9), std::vector<uint8_t>(35, 0), 7, 5, c3).foreground_count == 35);
    }
    {   // :749-771
        std::vector<int16_t> cg(50, 100);
        for (int row = 1; row < 4; ++row) for (int col = 2; col < 8; ++col) cg[row * 10 + col] = -10;
        CHECK(ac::segment_by_chroma({}, {}, cg, 10, 5, 50).foreground_count > 0);
    }
    {   // :500-518, :698-729, :561-594
        std::vector<uint8_t> m(40, 0);
        for (int i = 10; i < 30; ++i) m[i] = 1;
        CHECK(ac::rle_encode_mask(m).size() == 9);
        CHECK((ac::rle_encode_mask(std::vector<uint8_t>(100, 0)) == std::vector<uint8_t>{100, 0, 0}));
        ac::SegmentResult r;
        r.mask.assign(50, 0); r.width = 10; r.height = 5;
        r.bbox[0] = 3; r.bbox[1] = 2; r.bbox[2] = 3; r.bbox[3] = 2; r.foreground_count = 6;
        std::vector<uint8_t> rgb(150, 0);
        for (int y = 2; y < 4; ++y) for (int x = 3; x < 6; ++x) {
            r.mask[y * 10 + x] = 1;
            rgb[(y * 10 + x) * 3] = 255; rgb[(y * 10 + x) * 3 + 1] = 128; rgb[(y * 10 + x) * 3 + 2] = 64;
        }
        auto person = r.extract_person_rgb(rgb);
        CHECK(person.size() == 18 && person[0] == 255 && person[1] == 128 && person[2] == 64);
    }
    std::puts("CPP SEGMENT OK");
    return 0;
}
