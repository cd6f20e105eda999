// Probe: VGPR-index mode semantics on gfx950 (used by the rANS decode chain).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
__global__ __launch_bounds__(64) void probe(uint32_t* out, uint32_t row, uint32_t lanesel) {
  int lane = threadIdx.x;
  uint32_t r1, r2, r3;
  asm volatile(
    "v_lshlrev_b32 v64, 8, %[l]\n\t"            // v64+k = lane<<8 | k
    "v_or_b32 v65, 1, v64\n\t" "v_or_b32 v66, 2, v64\n\t" "v_or_b32 v67, 3, v64\n\t"
    "v_mov_b32 v70, 0x7777\n\t" "v_mov_b32 v71, 0x7778\n\t" "v_mov_b32 v72, 0x7779\n\t" "v_mov_b32 v73, 0x777a\n\t"
    "s_nop 4\n\t"
    "s_set_gpr_idx_on %[row], 0x1\n\t"          // src0 relative
    "v_mov_b32 v70, v64\n\t"                    // expect v70 = v[64+row]
    "s_nop 1\n\t"
    "v_readlane_b32 %[r1], v70, %[ls]\n\t"      // is src0 (v70) indexed too?  lane select masked to 6 bits?
    "v_readlane_b32 %[r2], v64, %[ls]\n\t"      // indexed readlane straight from the table?
    "s_set_gpr_idx_off\n\t"
    "s_nop 1\n\t"
    "v_readlane_b32 %[r3], v70, %[ls]\n\t"
    : [r1] "=&s"(r1), [r2] "=&s"(r2), [r3] "=&s"(r3)
    : [l] "v"(lane), [row] "s"(row), [ls] "s"(lanesel)
    : "v64","v65","v66","v67","v70","v71","v72","v73","m0","memory");
  if (lane == 0) { out[0] = r1; out[1] = r2; out[2] = r3; }
}
// Mode 0x6 (SRC1_REL | SRC2_REL), which the vector decode tile uses: VGPRs in the src1 and src2 positions are relative;
// src0, the destination, v_readlane's source row and its SGPR lane select, and v_writelane's row are not.
// v64+k = lane << 8 | k, v70+k = 0x10000 * (k + 1), v80+k = 0xDEAD0000 | k, v90+k = 0 (k = 0..3).
__global__ __launch_bounds__(64) void probe_vec(uint32_t* out, uint32_t row, uint32_t lanesel, uint32_t val) {
  int lane = threadIdx.x;
  uint32_t r[10];
  asm volatile(
    "v_lshlrev_b32 v64, 8, %[l]\n\t"
    "v_or_b32 v65, 1, v64\n\t" "v_or_b32 v66, 2, v64\n\t" "v_or_b32 v67, 3, v64\n\t"
    "v_mov_b32 v70, 0x10000\n\t" "v_mov_b32 v71, 0x20000\n\t" "v_mov_b32 v72, 0x30000\n\t" "v_mov_b32 v73, 0x40000\n\t"
    "v_mov_b32 v80, 0xDEAD0000\n\t" "v_mov_b32 v81, 0xDEAD0001\n\t" "v_mov_b32 v82, 0xDEAD0002\n\t" "v_mov_b32 v83, 0xDEAD0003\n\t"
    "v_mov_b32 v84, 0\n\t"
    "v_mov_b32 v90, 0\n\t" "v_mov_b32 v91, 0\n\t" "v_mov_b32 v92, 0\n\t" "v_mov_b32 v93, 0\n\t"
    "s_nop 4\n\t"
    "s_set_gpr_idx_on %[row], 0x6\n\t"
    "v_add_u32_e64 v80, v70, v64\n\t"           // expect v80 = v70 + v[64+row]: src1 relative, src0 and the destination not
    "v_mad_u32_u24 v84, 1, v64, v70\n\t"        // expect v84 = v[64+row] + v[70+row]: src1 and src2 relative
    "v_writelane_b32 v90, %[val], 5\n\t"        // expect v90 lane 5, whatever the row
    "s_nop 1\n\t"
    "v_readlane_b32 %[r0], v80, %[ls]\n\t"      // expect v80 (not v[80+row]) at lane ls & 63
    "s_set_gpr_idx_off\n\t"
    "s_nop 1\n\t"
    "v_readlane_b32 %[r1], v80, %[ls]\n\t"
    "v_readlane_b32 %[r2], v81, %[ls]\n\t" "v_readlane_b32 %[r3], v82, %[ls]\n\t" "v_readlane_b32 %[r4], v83, %[ls]\n\t"
    "v_readlane_b32 %[r5], v84, %[ls]\n\t"
    "v_readlane_b32 %[r6], v90, 5\n\t"
    "v_readlane_b32 %[r7], v91, 5\n\t" "v_readlane_b32 %[r8], v92, 5\n\t" "v_readlane_b32 %[r9], v93, 5\n\t"
    : [r0] "=&s"(r[0]), [r1] "=&s"(r[1]), [r2] "=&s"(r[2]), [r3] "=&s"(r[3]), [r4] "=&s"(r[4]), [r5] "=&s"(r[5]),
      [r6] "=&s"(r[6]), [r7] "=&s"(r[7]), [r8] "=&s"(r[8]), [r9] "=&s"(r[9])
    : [l] "v"(lane), [row] "s"(row), [ls] "s"(lanesel), [val] "s"(val)
    : "v64","v65","v66","v67","v70","v71","v72","v73","v80","v81","v82","v83","v84","v90","v91","v92","v93","m0","memory");
  if (lane == 0) for (int i = 0; i < 10; ++i) out[i] = r[i];
}
static int run_vec(uint32_t* d) {
  int bad = 0;
  for (uint32_t row = 0; row < 4; ++row) for (uint32_t ls : {5u, 64u + 7u, 0xfffff0c9u}) {
    const uint32_t val = 0xC0FFEE00u | row;
    hipLaunchKernelGGL(probe_vec, dim3(1), dim3(64), 0, 0, d, row, ls, val);
    uint32_t h[10]; hipMemcpy(h, d, 40, hipMemcpyDeviceToHost);
    const uint32_t l = ls & 63, sum = 0x10000u + ((l << 8) | row), mad = ((l << 8) | row) + 0x10000u * (row + 1);
    const uint32_t want[10] = {sum, sum, 0xDEAD0001u, 0xDEAD0002u, 0xDEAD0003u, mad, val, 0, 0, 0};
    bool ok = true;
    for (int i = 0; i < 10; ++i) ok &= h[i] == want[i];
    printf("mode 0x6 row %u lanesel 0x%x: add(src1 rel)=0x%x readlane(in mode)=0x%x v81..83=0x%x 0x%x 0x%x mad(src1,src2 rel)=0x%x writelane v90..93=0x%x 0x%x 0x%x 0x%x  %s\n",
           row, ls, h[1], h[0], h[2], h[3], h[4], h[5], h[6], h[7], h[8], h[9], ok ? "as expected" : "NOT AS EXPECTED");
    bad += !ok;
  }
  return bad;
}
int main() {
  uint32_t* d; hipMalloc(&d, 64);
  for (uint32_t row = 0; row < 4; ++row) for (uint32_t ls : {5u, 64u + 7u, 0xfffff0c9u}) {
    hipLaunchKernelGGL(probe, dim3(1), dim3(64), 0, 0, d, row, ls);
    uint32_t h[3]; hipMemcpy(h, d, 12, hipMemcpyDeviceToHost);
    printf("row %u lanesel 0x%x (lane %u): mov+readlane(in mode)=0x%x  readlane(v64,in mode)=0x%x  readlane(v70, mode off)=0x%x\n", row, ls, ls & 63, h[0], h[1], h[2]);
  }
  return run_vec(d) ? 1 : 0;
}
