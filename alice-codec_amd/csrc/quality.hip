// Quality measurement on the device: the exact squared error of two interleaved 8-bit RGB volumes,
// one u64 per frame.
//
// Layout.  A frame of either side is a set of RUNS of contiguous bytes: one run of 3wh bytes when both sides keep their rows
// back to back (row pitch 3w), else h runs of 3w bytes.  A run is cut into 16-byte WINDOWS on the 16-byte grid of side a's
// addresses, so a's load of a whole window is aligned whatever the base and the pitches are; side b reads the same run
// offsets at whatever alignment they have there (gfx950 global loads take any byte alignment).  The first and the last
// window of a run may hang over its ends: those, and only those, are walked byte by byte over the bytes that lie inside.
// No byte outside a run is ever read on either side.
//
// Arithmetic.  A whole window stays packed: sum (a - b)^2 = sum a^2 + sum b^2 - 2 sum ab, three v_dot4_u32_u8 per dword
// pair into three u32 lane accumulators.  Each grows by at most 255^2 per byte, so a lane may take kSseLaneFlushVectors
// windows (66 048 bytes: 66 048 * 65 025 < 2^32) before it folds them into its u64 (flush_lane).  Bytewise ends go to the
// u64 directly.  Every sum is an integer and every fold exact, so the result does not depend on the grid.
//
// Work.  A virtual block is kSseBlock * kSseVectorsPerLane consecutive windows of one frame (lane t takes windows t,
// t + 256, ...: a wavefront's 16-byte loads are 1 KiB contiguous).  Workgroups stride over the virtual blocks, whose frames
// never decrease along the way: a wavefront keeps its lanes' sums while the frame stays, and on a change of frame (and at
// the end) reduces them across its lanes and issues ONE 64-bit global_atomic_add_x2, none when the sum is 0.
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace alice {

namespace {

struct SseSide {
    const uint8_t* base;
    unsigned long long row_pitch, frame_pitch;
};
struct SseArgs {
    SseSide a, b;
    unsigned long long run_len;      // bytes of a run
    unsigned long long runs;         // runs of a frame (1: flat)
    unsigned long long nwin;         // windows a run can take at the worst alignment
    unsigned long long vb_per_frame; // virtual blocks of a frame
    unsigned long long n_vb;         // ... of the launch
    unsigned long long* out;         // [n_frames], zeroed
};

__device__ __forceinline__ void dot16(const uint4& x, const uint4& y, uint32_t& saa, uint32_t& sbb, uint32_t& sab) {
    saa = __builtin_amdgcn_udot4(x.x, x.x, saa, false); sbb = __builtin_amdgcn_udot4(y.x, y.x, sbb, false); sab = __builtin_amdgcn_udot4(x.x, y.x, sab, false);
    saa = __builtin_amdgcn_udot4(x.y, x.y, saa, false); sbb = __builtin_amdgcn_udot4(y.y, y.y, sbb, false); sab = __builtin_amdgcn_udot4(x.y, y.y, sab, false);
    saa = __builtin_amdgcn_udot4(x.z, x.z, saa, false); sbb = __builtin_amdgcn_udot4(y.z, y.z, sbb, false); sab = __builtin_amdgcn_udot4(x.z, y.z, sab, false);
    saa = __builtin_amdgcn_udot4(x.w, x.w, saa, false); sbb = __builtin_amdgcn_udot4(y.w, y.w, sbb, false); sab = __builtin_amdgcn_udot4(x.w, y.w, sab, false);
}

// kFlat: one run per frame (no row arithmetic at all); otherwise h runs
template <bool kFlat>
__global__ __launch_bounds__(kSseBlock) void rgb_sse_kernel(const SseArgs p) {
    constexpr unsigned long long kNone = ~0ull;
    uint32_t saa = 0u, sbb = 0u, sab = 0u, held = 0u;   // held: windows in the u32 sums since the last fold
    unsigned long long acc = 0ull, cur = kNone;
    auto flush_lane = [&]() {
        acc += (unsigned long long)saa + (unsigned long long)sbb - 2ull * (unsigned long long)sab;   // >= 0: a sum of squares
        saa = sbb = sab = 0u; held = 0u;
    };
    auto emit = [&]() {   // every lane of the workgroup arrives here together: frames change per virtual block
        flush_lane();
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
        if ((threadIdx.x & 63u) == 0u && acc) atomicAdd(p.out + cur, acc);
        acc = 0ull;
    };
    // (frame, segment) of the workgroup's virtual block, kept by addition: a stride of gridDim.x virtual blocks is
    // step_frames whole frames and step_seg segments, so a step costs one compare however small and many the frames are
    // (two divisions per launch, none per step)
    const unsigned long long step_frames = gridDim.x / p.vb_per_frame, step_seg = gridDim.x - step_frames * p.vb_per_frame;
    unsigned long long frame = blockIdx.x / p.vb_per_frame, seg = blockIdx.x - frame * p.vb_per_frame;
    for (unsigned long long vb = blockIdx.x; vb < p.n_vb; vb += gridDim.x, frame += step_frames, seg += step_seg) {
        if (seg >= p.vb_per_frame) { seg -= p.vb_per_frame; ++frame; }   // seg < 2 * vb_per_frame: both addends are below it
        if (frame != cur) {
            if (cur != kNone) emit();
            cur = frame;
        }
        if (held > kSseLaneFlushVectors - kSseVectorsPerLane) flush_lane();
        held += kSseVectorsPerLane;
        unsigned long long v = seg * (unsigned long long)(kSseBlock * kSseVectorsPerLane) + threadIdx.x, r = 0ull;
        if (!kFlat) {
            if ((p.vb_per_frame * (unsigned long long)(kSseBlock * kSseVectorsPerLane)) >> 32 == 0ull) {   // every window index fits 32 bits
                r = (uint32_t)v / (uint32_t)p.nwin; v = (uint32_t)v % (uint32_t)p.nwin;
            } else { r = v / p.nwin; v -= r * p.nwin; }
        }
        const uint8_t* fa = p.a.base + frame * p.a.frame_pitch;
        const uint8_t* fb = p.b.base + frame * p.b.frame_pitch;
        // where this lane's windows lie: window v of run r covers run offsets [lo, lo + 16), the 16-byte line of side a
        // that holds them.  Whole windows are the rule (every window but the first and last of a run), so when all of
        // a lane's windows are whole their loads are issued together, ahead of the arithmetic.
        const uint8_t* ra[kSseVectorsPerLane];
        const uint8_t* rb[kSseVectorsPerLane];
        long long lo[kSseVectorsPerLane];
        bool valid[kSseVectorsPerLane], whole[kSseVectorsPerLane];
        bool all_whole = true;
#pragma unroll
        for (uint32_t j = 0; j < kSseVectorsPerLane; ++j) {
            if (!kFlat) {
                while (v >= p.nwin && r < p.runs) { v -= p.nwin; ++r; }
            }
            valid[j] = kFlat ? v < p.nwin : r < p.runs;
            ra[j] = kFlat ? fa : fa + r * p.a.row_pitch;
            rb[j] = kFlat ? fb : fb + r * p.b.row_pitch;
            lo[j] = (long long)(v * 16ull) - (long long)((uintptr_t)ra[j] & 15u);
            whole[j] = valid[j] && lo[j] >= 0 && (unsigned long long)lo[j] + 16ull <= p.run_len;
            all_whole = all_whole && whole[j];
            v += kSseBlock;
        }
        if (all_whole) {
            uint4 x[kSseVectorsPerLane], y[kSseVectorsPerLane];
#pragma unroll
            for (uint32_t j = 0; j < kSseVectorsPerLane; ++j) {
                x[j] = *reinterpret_cast<const uint4*>(ra[j] + lo[j]);
                __builtin_memcpy(&y[j], rb[j] + lo[j], 16);
            }
#pragma unroll
            for (uint32_t j = 0; j < kSseVectorsPerLane; ++j) dot16(x[j], y[j], saa, sbb, sab);
        } else {
#pragma unroll
            for (uint32_t j = 0; j < kSseVectorsPerLane; ++j) {
                if (whole[j]) {
                    const uint4 x = *reinterpret_cast<const uint4*>(ra[j] + lo[j]);
                    uint4 y;
                    __builtin_memcpy(&y, rb[j] + lo[j], 16);
                    dot16(x, y, saa, sbb, sab);
                } else if (valid[j]) {
                    const unsigned long long k0 = lo[j] < 0 ? 0ull : (unsigned long long)lo[j];
                    const unsigned long long k1 = lo[j] + 16 < (long long)p.run_len ? (unsigned long long)(lo[j] + 16) : p.run_len;   // lo > -16
                    for (unsigned long long k = k0; k < k1; ++k) {
                        const int dd = (int)ra[j][k] - (int)rb[j][k];
                        acc += (unsigned long long)(dd * dd);
                    }
                }
            }
        }
    }
    if (cur != kNone) emit();
}

}  // namespace

bool rgb_sse_flat(const RgbLayout& a, const RgbLayout& b, uint64_t w, uint64_t h) {
    return h == 1 || (a.row_pitch == 3 * w && b.row_pitch == 3 * w);
}

hipError_t launch_rgb_sse(const RgbLayout& a, const RgbLayout& b, uint64_t w, uint64_t h, uint64_t n_frames,
                          unsigned long long* d_frame_sse, hipStream_t st) {
    if (!n_frames) return hipSuccess;
    const hipError_t zeroed = hipMemsetAsync(d_frame_sse, 0, n_frames * sizeof(unsigned long long), st);
    if (zeroed != hipSuccess) return zeroed;   // nothing is launched onto sums that were not zeroed
    if (!w || !h) return hipSuccess;
    SseArgs p;
    p.a = SseSide{a.base, a.row_pitch, a.frame_pitch};
    p.b = SseSide{b.base, b.row_pitch, b.frame_pitch};
    const bool flat = rgb_sse_flat(a, b, w, h);
    p.run_len = flat ? 3 * w * h : 3 * w;
    p.runs = flat ? 1 : h;
    p.nwin = (15 + p.run_len + 15) / 16;   // a run that starts on the last byte of a line
    const unsigned long long per_vb = (unsigned long long)kSseBlock * kSseVectorsPerLane;
    p.vb_per_frame = (p.runs * p.nwin + per_vb - 1) / per_vb;
    p.n_vb = p.vb_per_frame * n_frames;
    p.out = d_frame_sse;
    // grid_for counts items of 256 per workgroup: one workgroup per virtual block, under the suite's cap and the device's
    // eight resident workgroups per CU
    const unsigned grid = std::min(generic_grid_for(p.n_vb * 256ull), kSseMaxBlocks);
    if (flat) hipLaunchKernelGGL(rgb_sse_kernel<true>, dim3(grid), dim3(kSseBlock), 0, st, p);
    else hipLaunchKernelGGL(rgb_sse_kernel<false>, dim3(grid), dim3(kSseBlock), 0, st, p);
    return hipGetLastError();
}

}  // namespace alice
