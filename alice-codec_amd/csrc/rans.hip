// rANS stage for gfx950: frequency-table build, single-stream encode chain, decode chain.
//
// Reference behaviour restated (reference checkout, file:line):
//   FrequencyTable::from_histogram / uniform      src/rans.rs:102-189
//   RansEncoder::encode / encode_symbols / finish  src/rans.rs:269-308
//   RansDecoder::new / decode / decode_n           src/rans.rs:330-381
//
// The single-stream format is one strict dependency chain per channel (state
// transitions are injective, so chains cannot be split or speculated), which
// leaves two levers on a GPU: (1) strip every state-independent operation out of
// the chain and (2) run many chains (3 channels x chunks in flight) side by side,
// one wavefront each.
//
// Encode chain ("ripple"): a wavefront loads 64 consecutive symbols, one per lane,
// and gathers each lane's table parameters from LDS.  The state then ripples
// through the lanes: every lane executes
//     xin  = dpp_wave_shr1(xout) + c_prev          (lane 0 keeps the carry-in)
//     y    = xin >> {0,8,16}                       (renormalise against freq<<19)
//     xout = y + (umulhi(y, rcp) >> rsh) * (4096 - freq)
// 64 times.  Lanes 0..t hold their final values after step t and are fixed points
// of the update from then on, so no masking is needed; after 64 steps every lane
// holds the exact state before and after its own symbol.  The serial chain is 9
// VALU instructions per symbol (7 in blocks without a symbol of frequency <= 16,
// which carry the complement of the state: ripple64_comp_run) with no memory access
// and no cross-lane traffic other than the DPP operand.  Byte emission (0-2 bytes per symbol, taken from the
// low bytes of the pre-renormalisation state) is then a wave-parallel ballot/popcount
// compaction.  Bytes are written back to front so the stream comes out already
// "reversed" as RansEncoder::finish leaves it.
#include <cstdlib>
#include <cstring>

#include "common.h"
#include "freq_table.h"
#include "kernels.h"

namespace alice {

// ----------------------------------------------------------------------------------
// Encoder rows and decoder slots of a frequency table (the table itself: freq_table_256, freq_table.h)
// ----------------------------------------------------------------------------------

__device__ inline RansEncEntry make_enc_entry(uint32_t f, uint32_t c) {
    RansEncEntry e;
    e.freq = f;
    e.cum = c;
    // x_max = (L >> 12 << 8) * freq = freq << 19 (u64 in the reference, src/rans.rs:275);
    // states never reach 2^32-1, so saturation preserves every comparison.
    unsigned long long xm = (unsigned long long)f << 19;
    unsigned long long xm8 = (unsigned long long)f << 27;
    e.xmax = xm > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)xm;
    e.xmax8 = xm8 > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)xm8;
    if (f == 0u || f > kProbScale) {
        // handled by the exact serial path in the encode kernel
        e.xmax = f == 0u ? 0xFFFFFFFFu : e.xmax;
        e.xmax8 = f == 0u ? 0xFFFFFFFFu : e.xmax8;
        e.rcp = 0u; e.rsh = 0u; e.g = 0; e.cbias = 0u;
    } else if (f == 1u) {
        // floor(y/1) = y: umulhi(y, 2^32-1) = y-1 for y >= 1, compensated in the bias:
        // y + (y-1)*4095 + c + 4095 = 4096*y + c
        e.rcp = 0xFFFFFFFFu; e.rsh = 0u; e.g = 4095; e.cbias = c + 4095u;
    } else {
        // 2 <= f <= 4096, y < f*2^19.  L = ceil(log2 f), m = ceil(2^(31+L)/f) < 2^32,
        // floor(y/f) = (y*m) >> (31+L) because y*(m*f - 2^(31+L)) < 2^(19+2L) <= 2^(31+L).
        uint32_t L = 32u - (uint32_t)__clz((int)(f - 1u));
        unsigned long long p = 1ull << (31u + L);
        e.rcp = (uint32_t)((p + f - 1u) / f);
        e.rsh = L - 1u;
        e.g = (int32_t)kProbScale - (int32_t)f;
        e.cbias = c;
    }
    return e;
}

// Decoder slot tables, filled as the reference fills cum_to_sym (src/rans.rs:135-144): zero-initialised, then symbol by
// symbol in index order over [cum, min(cum + freq, 4096)), so the LAST symbol that covers a slot owns it (ranges built
// from a histogram are disjoint; caller-supplied tables may overlap) and an uncovered slot belongs to symbol 0.
// Called by all 256 threads of the block, s = threadIdx.x holding symbol s; scratch: 768 u32 in LDS.  Returns the
// kTableDec* flags of the slots this thread filled.
__device__ inline uint32_t build_dec_slots(uint32_t f, uint32_t c, uint32_t* scratch, RansDecSlots* __restrict__ out) {
    const int s = threadIdx.x;
    uint32_t end = c + f;
    if (end > kProbScale) end = kProbScale;
    __syncthreads();
    scratch[s] = c;
    scratch[256 + s] = c < end ? end : c;   // empty range when cum >= 4096 or freq == 0
    scratch[512 + s] = f;
    out->symtab[s] = (f & 0xFFFFu) | (c << 16);
    __syncthreads();
    uint32_t fl = 0u;
    for (uint32_t slot = (uint32_t)s; slot < kProbScale; slot += 256u) {
        uint32_t owner = 0u;
        for (uint32_t k = 0; k < 256u; ++k)
            if (slot >= scratch[k] && slot < scratch[256 + k]) owner = k;
        const uint32_t fo = scratch[512 + owner], co = scratch[owner];
        // x' = freq * (x >> 12) + slot - cum = umulhi(F', x) + B' with F' = freq << 20 and
        // B' = slot - cum - ((freq * slot) >> 12): with x = 4096 h + slot, floor(freq * x / 4096) =
        // freq * h + floor(freq * slot / 4096).  freq = 4096 would overflow F'; there F' = 2^32 - 1
        // (umulhi gives x - 1 for x >= 1) and B' carries the + 1.
        uint32_t fe, be;
        if (fo >= kProbScale) {
            fe = 0xFFFFFFFFu; be = (slot - co) - slot + 1u;
            fl |= fo > kProbScale ? kTableDecExact : kTableDecBig;
        } else {
            fe = fo << 20; be = (slot - co) - ((fo * slot) >> kProbBits);
        }
        out->ftab[slot] = fe;
        out->btab[slot] = be;
        out->c2s[slot] = (uint8_t)owner;
    }
    return fl;
}

// used (may be null): the histogram of the symbols that will be encoded, where that is not `hist` itself -- a caller's
// histogram need not be its data's.  kTableVerified promises that the generic / diverges flags speak for the DATA, so
// they are taken from `used`; the table comes from `hist` either way.
__global__ __launch_bounds__(256) void rans_table_kernel(const uint32_t* __restrict__ hist,
                                                         RansTable* __restrict__ tables, uint32_t n_sym,
                                                         const uint32_t* __restrict__ used) {
    __shared__ uint32_t scratch[768];
    const int chain = blockIdx.x;
    const int s = threadIdx.x;
    const uint32_t count = (uint32_t)s < n_sym ? hist[(size_t)chain * 256 + s] : 0u;
    uint32_t f, c;
    freq_table_256(count, n_sym, scratch, f, c);
    tables[chain].enc[s] = make_enc_entry(f, c);
    uint32_t fl = build_dec_slots(f, c, scratch, &tables[chain].dec);
    const uint32_t occurs = used ? used[(size_t)chain * 256 + s] : count;
    if (occurs > 0u && f == 0u) fl |= kTableDiverges;
    if (occurs > 0u && f > kProbScale) fl |= kTableNeedsGeneric;
    __shared__ uint32_t flags_sh;
    if (s == 0) flags_sh = 0u;
    __syncthreads();
    if (fl) atomicOr(&flags_sh, fl);
    __syncthreads();
    if (s == 0) tables[chain].flags = flags_sh | kTableVerified;
}

// Table from explicit (cum, freq) arrays -- stage-level API (FrequencyTable handle).
__global__ __launch_bounds__(256) void rans_table_from_arrays_kernel(const uint16_t* __restrict__ cum,
                                                                     const uint16_t* __restrict__ freq,
                                                                     RansTable* __restrict__ table) {
    __shared__ uint32_t scratch[768];
    __shared__ uint32_t flags_sh;
    const int s = threadIdx.x;
    if (s == 0) flags_sh = 0u;
    table->enc[s] = make_enc_entry(freq[s], cum[s]);
    const uint32_t fl = build_dec_slots(freq[s], cum[s], scratch, &table->dec);
    if (fl) atomicOr(&flags_sh, fl);
    __syncthreads();
    if (s == 0) table->flags = flags_sh;
}

// The same over n tables in one launch (the batched preview): workgroup blockIdx.x builds
// tables[blockIdx.x] from row blockIdx.x of cum and freq ([n][256]), byte for byte what the kernel above writes.
__global__ __launch_bounds__(256) void rans_tables_from_arrays_kernel(const uint16_t* __restrict__ cum,
                                                                      const uint16_t* __restrict__ freq,
                                                                      RansTable* __restrict__ tables) {
    __shared__ uint32_t scratch[768];
    __shared__ uint32_t flags_sh;
    const int s = threadIdx.x;
    const size_t t = blockIdx.x;
    RansTable* __restrict__ table = tables + t;
    const uint32_t f = freq[t * 256 + s], c = cum[t * 256 + s];
    if (s == 0) flags_sh = 0u;
    table->enc[s] = make_enc_entry(f, c);
    const uint32_t fl = build_dec_slots(f, c, scratch, &table->dec);
    if (fl) atomicOr(&flags_sh, fl);
    __syncthreads();
    if (s == 0) table->flags = flags_sh;
}

// Two chains on one SIMD (more than 1024 chains in flight): the SIMD's issue arbiter prefers the OLDER wave, so the older
// chain runs almost undisturbed and the younger one gets what is left -- and the step waits for the slowest chain.  Taking
// turns was the proposed cure (round 2): every wave derives its priority from a bit of the shader clock
// (the same for both waves of a SIMD) XOR the low bit of its wave slot (consecutive slots: different for the two),
// re-evaluated once per tile, so at any time one of the two has priority 1 and the other 0.  Waves never wait on each
// other: this is arbitration only.  MEASURED in round 3 (960x540x64 chunks, profiles/r03_chain_probe_960x540_turns_*.log):
//   1200 chains (176 SIMDs shared): the slowest encoder of a pair 61.0 instead of 63.5 cycles/symbol (kernel 25.6 instead of
//   26.6 ns/symbol), decoders 48.6 instead of 49.3 ns/symbol -- the pairs move closer but do not finish together;
//   2046 chains (every SIMD shared): encoders unchanged (38.0 ns/symbol), decoders 86.4 instead of 79.2 ns/symbol: WORSE.
// And two chains per SIMD buy little in the first place: 2046 chains encode 53.9 Gsym/s against 50.3 with 1023 (+7 %) and
// decode 25.8 against 26.4 (-2 %): eight decoders on a CU saturate its one scalar unit.  So it is OFF unless
// ALICE_CHAIN_TURNS=1, and one chain per SIMD stays the operating point.  kExclusive instances never evaluate it.
__device__ __forceinline__ void chain_take_turns(uint32_t enabled) {
    if (!enabled) return;
    const uint32_t turn = (uint32_t)(clock64() >> 17);                                   // ~55 us at 2.4 GHz
    const uint32_t slot = __builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 4);           // HW_REG_HW_ID[3:0]: wave slot on the SIMD
    if ((turn ^ slot) & 1u) __builtin_amdgcn_s_setprio(1);
    else __builtin_amdgcn_s_setprio(0);
}

// ----------------------------------------------------------------------------------
// Encode chain
// ----------------------------------------------------------------------------------

constexpr int kEncTile = 1024;  // symbols staged per global load (16 B per lane)
constexpr int kEncTilePad = 128;

// 64 ripple steps.  On entry lane 0 of xin holds the carry-in state and xout is
// don't-care; on exit every lane holds the state before (xin) and after (xout,
// without its own cum bias) its symbol.
__device__ __forceinline__ void ripple64(uint32_t& xin, uint32_t& xout, uint32_t xmax, uint32_t xmax8,
                                         uint32_t rcp, uint32_t rsh, int32_t g, uint32_t cprev) {
    uint32_t k, y, q;
    unsigned long long m1;
    // Wait states (gfx940-family): VALU-written SGPR/VCC -> VALU read needs 2 states
    // (the second compare and one SALU/nop sit between); VALU-written VGPR -> DPP read
    // needs 2 states (s_nop 1, or s_cmp + s_cbranch at the loop edge).
#define ALICE_RIPPLE_STEP(TAIL)                                                     \
    "v_add_u32_dpp %[xin], %[xout], %[cprev] wave_shr:1 row_mask:0xf bank_mask:0xf\n\t" \
    "v_cmp_ge_u32_e64 %[m1], %[xin], %[xmax]\n\t"                                  \
    "v_cmp_ge_u32_e32 vcc, %[xin], %[xmax8]\n\t"                                   \
    "s_nop 0\n\t"                                                                    \
    "v_cndmask_b32_e64 %[k], 0, 8, %[m1]\n\t"                                      \
    "v_cndmask_b32_e64 %[k], %[k], 16, vcc\n\t"                                    \
    "v_lshrrev_b32_e32 %[y], %[k], %[xin]\n\t"                                     \
    "v_mul_hi_u32 %[q], %[y], %[rcp]\n\t"                                          \
    "v_lshrrev_b32_e32 %[q], %[rsh], %[q]\n\t"                                     \
    "v_mad_i32_i24 %[xout], %[q], %[g], %[y]\n\t" TAIL
    // fully unrolled: a taken loop branch costs ~25 cycles on a lone wave (scripts/probes/latency_probe.hip)
#define ALICE_RIPPLE_STEP4 ALICE_RIPPLE_STEP("s_nop 1\n\t") ALICE_RIPPLE_STEP("s_nop 1\n\t") ALICE_RIPPLE_STEP("s_nop 1\n\t") ALICE_RIPPLE_STEP("s_nop 1\n\t")
#define ALICE_RIPPLE_STEP16 ALICE_RIPPLE_STEP4 ALICE_RIPPLE_STEP4 ALICE_RIPPLE_STEP4 ALICE_RIPPLE_STEP4
    asm volatile(
        "s_nop 1\n\t"
        ALICE_RIPPLE_STEP16 ALICE_RIPPLE_STEP16 ALICE_RIPPLE_STEP16 ALICE_RIPPLE_STEP16
        : [xin] "+v"(xin), [xout] "+v"(xout), [k] "=&v"(k), [y] "=&v"(y), [q] "=&v"(q), [m1] "=&s"(m1)
        : [xmax] "v"(xmax), [xmax8] "v"(xmax8), [rcp] "v"(rcp), [rsh] "v"(rsh), [g] "v"(g),
          [cprev] "v"(cprev)
        : "vcc");
#undef ALICE_RIPPLE_STEP16
#undef ALICE_RIPPLE_STEP4
#undef ALICE_RIPPLE_STEP
}

// The same 64 steps with ONE compare per step, for chains whose states stay in [2^23, 2^31 + 2^17): every symbol that
// occurs has a frequency in 1..4096 (kTableVerified without the generic / diverges flags) and the chain started from
// 2^23.  Then the renormalisation shift needs only one threshold per symbol:
//   freq <= 16: freq << 19 <= 2^23 <= x, the first shift always happens:   k = 8 + 8 * (x >= freq << 27)
//   freq >= 17: freq << 27 > 2^31 + 2^17 > x, the second never happens:    k = 8 * (x >= freq << 19)
// (x < 2^31 + 2^17: x' = (q << 12) + r + cum with q < 2^19, r < freq <= 4096, cum < 2^16.)  thr / k0 / k1 are the lane's
// threshold and the two shift candidates.  9 issue slots per symbol instead of 11.
__device__ __forceinline__ void ripple64_clean(uint32_t& xin, uint32_t& xout, uint32_t thr, uint32_t k0, uint32_t k1,
                                               uint32_t rcp, uint32_t rsh, int32_t g, uint32_t cprev) {
    uint32_t k, y, q;
#define ALICE_RIPPLE_STEP                                                            \
    "v_add_u32_dpp %[xin], %[xout], %[cprev] wave_shr:1 row_mask:0xf bank_mask:0xf\n\t" \
    "v_cmp_ge_u32_e32 vcc, %[xin], %[thr]\n\t"                                     \
    "s_nop 1\n\t"                                                                  \
    "v_cndmask_b32_e32 %[k], %[k0], %[k1], vcc\n\t"                                \
    "v_lshrrev_b32_e32 %[y], %[k], %[xin]\n\t"                                     \
    "v_mul_hi_u32 %[q], %[y], %[rcp]\n\t"                                          \
    "v_lshrrev_b32_e32 %[q], %[rsh], %[q]\n\t"                                     \
    "v_mad_i32_i24 %[xout], %[q], %[g], %[y]\n\t"                                  \
    "s_nop 1\n\t"
#define ALICE_RIPPLE_STEP4 ALICE_RIPPLE_STEP ALICE_RIPPLE_STEP ALICE_RIPPLE_STEP ALICE_RIPPLE_STEP
#define ALICE_RIPPLE_STEP16 ALICE_RIPPLE_STEP4 ALICE_RIPPLE_STEP4 ALICE_RIPPLE_STEP4 ALICE_RIPPLE_STEP4
    asm volatile(
        "s_nop 1\n\t"
        ALICE_RIPPLE_STEP16 ALICE_RIPPLE_STEP16 ALICE_RIPPLE_STEP16 ALICE_RIPPLE_STEP16
        : [xin] "+v"(xin), [xout] "+v"(xout), [k] "=&v"(k), [y] "=&v"(y), [q] "=&v"(q)
        : [thr] "v"(thr), [k0] "v"(k0), [k1] "v"(k1), [rcp] "v"(rcp), [rsh] "v"(rsh), [g] "v"(g), [cprev] "v"(cprev)
        : "vcc");
#undef ALICE_RIPPLE_STEP16
#undef ALICE_RIPPLE_STEP4
#undef ALICE_RIPPLE_STEP
}

// The step for a block whose 64 symbols are all in the big class (17 <= freq <= 4096), 7 issue slots: the chain carries the
// COMPLEMENT of the state, u = T - 1 - x (mod 2^32) with T = freq << 19, so that the choice between x and x >> 8 becomes
// an unsigned minimum and needs neither a compare nor VCC.  With x in [2^23, 2^31 + 2^17):
//   x <  T: u = T - 1 - x lies in [0, T);  x >= T: u wraps to above 2^31 (x - T + 1 < 2^31 because T > 2^17).
//   w = ashr(u, 8) + T'' with T'' = T - (T >> 8) is T - 1 - (x >> 8) in BOTH cases (256 divides T, so the floor of
//   (T - 1 - x) / 256 is T / 256 - 1 - floor(x / 256)), and x >> 8 < 2^23 + 2^9 < T puts it in [0, T) too.
//   x < T: w >= u (x >> 8 <= x), min = u; x >= T: w < T <= 2^31 < u, min = w.  So m = min_u32(u, w) = T - 1 - y.
// The division stays in the complement domain: T = freq * 2^19, so floor(y / freq) = 2^19 - 1 - floor(m / freq), and
// m < freq << 19 is the bound the reciprocal is exact for.  With qm = umulhi(m, rcp) >> rsh and z = qm * g + m
// (qm < 2^19, g = 4096 - freq: both fit v_mad_i32_i24) the new state is
//   x' = y + (2^19 - 1 - qm) * g + cum = C - z,   C = 2^31 - 4097 + freq + cum,
// and the next lane's complement is u' = T' - 1 - x' = z + kc with kc = T' - 1 - C (its own T, the previous lane's C),
// one v_add_u32_dpp as before.  On entry lane 0 of u holds T - 1 - x of the carry-in (the DPP read from an invalid lane
// leaves it alone); on exit every lane holds its own u (before its symbol) and z (after: x' = C - z).
// w = ashr(u, 8) + T'' is ONE instruction: v_mad_i64_i32 {w : lo} = u * 2^24 + {T'' : 0}.  The signed product's high dword is
// ashr(u, 8), the addend's low dword is 0, so nothing carries into the sum of the high dwords.  The product pair is named
// outright, v[62:63] (inline asm has no operand modifier for one half of a pair).  The step is used by ripple64_comp_run.

// The constants of a complement block that its chain reads in every step, and the block's C (which the block after it wants
// in lane 0 of its cc_prev).  A run keeps two of these sets and its blocks swap their roles, so nothing is copied.
struct CompSet { uint32_t kc, rcp, rsh, cc; int32_t g; };
// What a run hands on besides the next block's CompSet: the rest of that block's constants, which only the plain code after
// the run reads.
struct CompNext { uint32_t xmax, tpp, cbias, xmax8, tm1; };

// A RUN of complement blocks as one statement: the 64 complement steps of each block b of the run, with the
// state-independent work of its neighbours in the seventh slot of a step, which otherwise only provides the two wait states
// between the VALU write of z and its DPP read, and the comp -> comp block edge as one instruction.  Measured on a lone wave
// (scripts/probes/latency_probe.hip, profiles/r20_ripple_filler_probe.json): the step costs 32.0 cycles with s_nop 1, with one
// VALU or SALU instruction + s_nop 0, and with two VALU instructions; an LDS read or a byte store in the slot costs 8 cycles
// more.  So every slot holds two instructions (they are the two wait states) or one and s_nop 0: the ALU fillers for nothing,
// the three LDS reads and the byte store of a block for their 8 cycles each, beside an ALU filler.
//   for block b + 1: its table row (tab_ab, LDS address `ad` = tab + 16 * symbol) and this lane's symbol of block b + 2
//     (LDS address `sa`) are read in steps 0, 2 and 3, the row into v[52:59]; after the wait in step 20 the fillers compute
//     the small-frequency ballot, cc_prev (lane 0: THIS block's C[63] by wave_ror:1, the others by wave_shr:1 -- only
//     v_mov_b32_dpp carries lane traffic, see the v_subrev_u32_dpp trap in DESIGN.md section 4.3), tm1, kc, the row address
//     of block b + 2, copy the row out of the fixed registers into the OTHER CompSet, or the ballot with all ones when the
//     tile has no block b + 1 (`left` counts the blocks after this one), and the last slot makes {0, T''} of block b + 1
//     and compares the ballot with 0 for the branch that ends the run.
//   for block b - 1 (every block but the run's first): the sign test of its saved u into VCC -- v_mad_i64_i32's carry goes
//     to an SGPR pair of its own here -- the mbcnt pair on tw, the offset (span1 - off for lanes that emit, the lane's dummy
//     byte for the others), the byte ~u and tw += popcount in steps 0..5; the store in step 6.
// The edge: step 0 of every block but the first is u = wave_ror1(z) + kc: lane 0 gets z[63] + kc[0] =
// T'[0] - 1 - (C[63] - z[63]) with kc[0] = T'[0] - 1 - C[63] as the block before made it; the other lanes are overwritten by
// the later steps as always.  The first block enters with T - 1 - x in lane 0 of u0.
// The run ends when `stop` is not 0 after a block (block b + 1 holds a symbol of frequency <= 16, or the tile is over).  Then
// phase tells which set is which: 0 -- the last block ran on sa_ and u0, sb_ holds block b + 1's constants; 1 -- the reverse.
// The last block's own byte is NOT stored: the caller emits it from u0 / u1.  z is the last block's z.
__device__ __forceinline__ void ripple64_comp_run(uint32_t& u0, uint32_t& u1, uint32_t& z, uint32_t tpp, CompSet& sa_, CompSet& sb_,
                                                  uint32_t tab, uint32_t& ad, uint32_t& sa, uint32_t& sym1, CompNext& nx,
                                                  unsigned long long& stop, uint32_t& left, uint32_t& phase, uint32_t& tw,
                                                  uint32_t lane, uint32_t span1, const void* tb) {
    uint32_t m, q, ccp, cnt, off, byt;
    unsigned long long cy, end, tp = (unsigned long long)tpp << 32;   // {0, T''}
    // U: the block's u; S: the CompSet its chain reads; N: the one it fills; P: the u of the block before
#define ALICE_RUN_CHAIN(CTRL, U, S)                                                          \
    "v_add_u32_dpp %[" U "], %[z], %[kc" S "] " CTRL " row_mask:0xf bank_mask:0xf\n\t"      \
    "v_mad_i64_i32 v[62:63], %[cy], %[" U "], %[two24], %[tp]\n\t"                          \
    "v_min_u32_e32 %[m], %[" U "], v63\n\t"                                                 \
    "v_mul_hi_u32 %[q], %[m], %[rcp" S "]\n\t"                                              \
    "v_lshrrev_b32_e32 %[q], %[rsh" S "], %[q]\n\t"                                         \
    "v_mad_i32_i24 %[z], %[q], %[g" S "], %[m]\n\t"
#define ALICE_RUN_STEP(U, S, FILL) ALICE_RUN_CHAIN("wave_shr:1", U, S) FILL
#define ALICE_RUN_IDLE(U, S) ALICE_RUN_STEP(U, S, "s_nop 1\n\t")
#define ALICE_RUN_IDLE4(U, S) ALICE_RUN_IDLE(U, S) ALICE_RUN_IDLE(U, S) ALICE_RUN_IDLE(U, S) ALICE_RUN_IDLE(U, S)
#define ALICE_RUN_IDLE13(U, S) ALICE_RUN_IDLE4(U, S) ALICE_RUN_IDLE4(U, S) ALICE_RUN_IDLE4(U, S) ALICE_RUN_IDLE(U, S)
    // steps 7..63
#define ALICE_RUN_REST(U, S, N)                                                                                                   \
    ALICE_RUN_IDLE13(U, S)                                                                                                        \
    ALICE_RUN_STEP(U, S, "s_waitcnt lgkmcnt(0)\n\t s_nop 1\n\t")                                                                 \
    ALICE_RUN_STEP(U, S, "v_lshl_add_u32 %[ad], %[sy], 4, %[tab]\n\t v_cmp_ge_u32_e64 %[sm], %[rl], v52\n\t")                    \
    ALICE_RUN_STEP(U, S, "v_mov_b32_dpp %[ccp], %[cc" S "] wave_ror:1 row_mask:0xf bank_mask:0xf\n\t s_nop 0\n\t")              \
    ALICE_RUN_STEP(U, S, "v_mov_b32_dpp %[ccp], v57 wave_shr:1 row_mask:0xf bank_mask:0xf\n\t s_nop 0\n\t")                      \
    ALICE_RUN_STEP(U, S, "v_add_u32_e32 %[tmn], -1, v52\n\t s_nop 0\n\t")                                                        \
    ALICE_RUN_STEP(U, S, "v_sub_u32_e32 %[kc" N "], %[tmn], %[ccp]\n\t s_nop 0\n\t")                                             \
    ALICE_RUN_STEP(U, S, "v_mov_b32_e32 %[rcp" N "], v53\n\t v_mov_b32_e32 %[rsh" N "], v54\n\t")                                \
    ALICE_RUN_STEP(U, S, "v_mov_b32_e32 %[g" N "], v55\n\t v_mov_b32_e32 %[cc" N "], v57\n\t")                                   \
    ALICE_RUN_STEP(U, S, "v_mov_b32_e32 %[xmn], v52\n\t v_mov_b32_e32 %[cbn], v58\n\t")                                          \
    ALICE_RUN_STEP(U, S, "v_mov_b32_e32 %[x8n], v59\n\t v_mov_b32_e32 %[tpn], v56\n\t")                                          \
    ALICE_RUN_STEP(U, S, "s_cmp_eq_u32 %[left], 0\n\t s_cselect_b64 %[end], -1, 0\n\t")                                          \
    ALICE_RUN_STEP(U, S, "s_or_b64 %[sm], %[sm], %[end]\n\t s_sub_u32 %[left], %[left], 1\n\t")                                  \
    ALICE_RUN_IDLE13(U, S) ALICE_RUN_IDLE13(U, S) ALICE_RUN_IDLE4(U, S) ALICE_RUN_IDLE(U, S)                                      \
    ALICE_RUN_STEP(U, S, "v_lshlrev_b64 %[tp], 32, v[56:57]\n\t s_cmp_lg_u64 %[sm], 0\n\t")
#define ALICE_RUN_READ_A "ds_read_b128 v[52:55], %[ad]\n\t"
#define ALICE_RUN_READ_B "ds_read_b128 v[56:59], %[ad] offset:4096\n\t"
#define ALICE_RUN_READ_S "ds_read_u8 %[sy], %[sa]\n\t"
#define ALICE_RUN_FIRST(U, S, N)                                                                                                  \
    ALICE_RUN_STEP(U, S, ALICE_RUN_READ_A " s_nop 0\n\t")                                                                         \
    ALICE_RUN_IDLE(U, S)                                                                                                          \
    ALICE_RUN_STEP(U, S, ALICE_RUN_READ_B " s_nop 0\n\t")                                                                         \
    ALICE_RUN_STEP(U, S, ALICE_RUN_READ_S " s_nop 0\n\t")                                                                         \
    ALICE_RUN_IDLE(U, S) ALICE_RUN_IDLE(U, S)                                                                                     \
    ALICE_RUN_STEP(U, S, "v_subrev_u32_e32 %[sa], 64, %[sa]\n\t s_nop 0\n\t")                                                    \
    ALICE_RUN_REST(U, S, N)
#define ALICE_RUN_NEXT(U, P, S, N)                                                                                                \
    ALICE_RUN_CHAIN("wave_ror:1", U, S) "v_cmp_gt_i32_e32 vcc, 0, %[" P "]\n\t" ALICE_RUN_READ_A                                  \
    ALICE_RUN_STEP(U, S, "v_not_b32_e32 %[byt], %[" P "]\n\t s_bcnt1_i32_b64 %[cnt], vcc\n\t")                                   \
    ALICE_RUN_STEP(U, S, "v_mbcnt_lo_u32_b32 %[off], vcc_lo, %[tw]\n\t" ALICE_RUN_READ_B)                                         \
    ALICE_RUN_STEP(U, S, "v_mbcnt_hi_u32_b32 %[off], vcc_hi, %[off]\n\t" ALICE_RUN_READ_S)                                        \
    ALICE_RUN_STEP(U, S, "v_sub_u32_e32 %[off], %[span1], %[off]\n\t v_add_u32_e32 %[tw], %[cnt], %[tw]\n\t")                    \
    ALICE_RUN_STEP(U, S, "v_cndmask_b32_e32 %[off], %[lane], %[off], vcc\n\t s_nop 0\n\t")                                       \
    ALICE_RUN_STEP(U, S, "global_store_byte %[off], %[byt], %[tb]\n\t v_subrev_u32_e32 %[sa], 64, %[sa]\n\t")                    \
    ALICE_RUN_REST(U, S, N)
    asm volatile(
        "s_mov_b32 %[ph], 0\n\t"
        ALICE_RUN_FIRST("u0", "a", "b")
        "1:\n\t"
        "s_cbranch_scc1 3f\n\t"      // (SCC: stop != 0, from the last slot of the block before)
        ALICE_RUN_NEXT("u1", "u0", "b", "a")
        "s_cbranch_scc1 2f\n\t"
        ALICE_RUN_NEXT("u0", "u1", "a", "b")
        "s_branch 1b\n\t"
        "2:\n\t"
        "s_mov_b32 %[ph], 1\n\t"
        "3:\n\t"
        : [u0] "+v"(u0), [u1] "=&v"(u1), [z] "=&v"(z), [tp] "+v"(tp), [ad] "+v"(ad), [sa] "+v"(sa), [sy] "=&v"(sym1), [tw] "+v"(tw),
          [off] "=&v"(off), [byt] "=&v"(byt), [cnt] "=&s"(cnt), [m] "=&v"(m), [q] "=&v"(q), [ccp] "=&v"(ccp), [cy] "=&s"(cy),
          [sm] "=&s"(stop), [end] "=&s"(end), [left] "+s"(left), [ph] "=&s"(phase), [tmn] "=&v"(nx.tm1), [xmn] "=&v"(nx.xmax),
          [tpn] "=&v"(nx.tpp), [cbn] "=&v"(nx.cbias), [x8n] "=&v"(nx.xmax8),
          [kca] "+v"(sa_.kc), [rcpa] "+v"(sa_.rcp), [rsha] "+v"(sa_.rsh), [ga] "+v"(sa_.g), [cca] "+v"(sa_.cc),
          [kcb] "=&v"(sb_.kc), [rcpb] "=&v"(sb_.rcp), [rshb] "=&v"(sb_.rsh), [gb] "=&v"(sb_.g), [ccb] "=&v"(sb_.cc)
        : [tab] "s"(tab), [lane] "v"(lane), [span1] "s"(span1), [two24] "s"(1u << 24), [rl] "s"(kRansL), [tb] "s"(tb)
        : "v52", "v53", "v54", "v55", "v56", "v57", "v58", "v59", "v62", "v63", "vcc", "scc", "memory");
#undef ALICE_RUN_NEXT
#undef ALICE_RUN_FIRST
#undef ALICE_RUN_READ_S
#undef ALICE_RUN_READ_B
#undef ALICE_RUN_READ_A
#undef ALICE_RUN_REST
#undef ALICE_RUN_IDLE13
#undef ALICE_RUN_IDLE4
#undef ALICE_RUN_IDLE
#undef ALICE_RUN_STEP
#undef ALICE_RUN_CHAIN
}

// kExclusive: the kernel claims more than half of the SIMD's 512 registers (an AGPR clobber; nothing uses them), so
// the dispatcher cannot put two chains on one SIMD -- see launch_rans_encode.
template <bool kExclusive>
__global__ __launch_bounds__(64) void rans_encode_kernel(const uint8_t* __restrict__ sym_base,
                                                         unsigned long long sym_stride,
                                                         unsigned long long n_first,
                                                         const RansTable* __restrict__ tables,
                                                         uint8_t* __restrict__ out_base,
                                                         unsigned long long cap0,
                                                         unsigned long long group_stride,
                                                         unsigned long long group_head,
                                                         unsigned n_split,
                                                         RansResult* __restrict__ results,
                                                         unsigned long long cap1, unsigned long long cap2,
                                                         uint32_t x_init, uint32_t keep_open, uint32_t take_turns,
                                                         const RansEncodeDesc* __restrict__ descs) {
    // what the clean tile reads per symbol is in tab_ab; T'' and C are the complement step's per-lane constants
    // (ripple64_comp_run; meaningful for 17 <= freq <= 4096 only)
    // (one array: a run statement reads both rows of a symbol off one LDS address, the second at offset 4096)
    __shared__ uint4 tab_ab[512];  // [s]: xmax, rcp, rsh, g;  [256 + s]: T'' = xmax - (xmax >> 8), C = 2^31 - 4097 + freq + cum, cbias, xmax8
    __shared__ uint2 tab_c[256];  // freq, cum
    // the tile's 1024 symbols sit behind kEncTilePad bytes that are never written: the block pipeline reads two blocks
    // past the end of a tile (values it never uses), at plain descending addresses
    __shared__ __attribute__((aligned(16))) uint8_t tile[kEncTilePad + kEncTile];

    if constexpr (kExclusive) asm volatile("" ::: "a255");
    const int chain = blockIdx.x;
    const int lane = threadIdx.x;
    // chains from n_split on carry one symbol less (the sub-sequences of an interleaved stream)
    unsigned long long n = n_first - (((unsigned)chain >= n_split && n_first > 0ull) ? 1ull : 0ull);
    const uint8_t* __restrict__ sym = sym_base + (size_t)chain * sym_stride;
    const RansTable* __restrict__ tbl = tables + chain;
    // group_stride == 0: regions back to back.  Otherwise the three chains of chunk g write into the chunk's own
    // .alc buffer, behind `group_head` bytes kept free for the header (the streams are compacted in place later).
    const int gch = chain % 3;
    unsigned long long cap = group_stride == 0ull ? cap0 : (gch == 0 ? cap0 : (gch == 1 ? cap1 : cap2));
    uint8_t* region = group_stride == 0ull ? out_base + (size_t)chain * cap0
                                           : out_base + (size_t)(chain / 3) * group_stride + group_head +
                                                 (gch == 0 ? 0ull : (gch == 1 ? cap0 : cap0 + cap1));
    RansResult* res = results + chain;
    if (descs) {   // a merged launch (launch_rans_encode_descs): every chain spelled out
        const RansEncodeDesc ds = descs[chain];
        sym = ds.sym; n = ds.n; tbl = ds.table; region = ds.region; cap = ds.cap; res = ds.result;
        x_init = ds.x_init; keep_open = ds.keep_open;
    }
    uint8_t* const out_end = region + cap;
    // lanes that have nothing to emit store to a private byte at the unused front of the region instead
    // of branching around the store; the capacity test keeps real bytes 64 bytes away from it
    uint8_t* const dummy = region + lane;

    for (int s = lane; s < 256; s += 64) {
        const RansEncEntry e = tbl->enc[s];
        tab_ab[s] = make_uint4(e.xmax, e.rcp, e.rsh, (uint32_t)e.g);
        tab_ab[256 + s] = make_uint4(e.xmax - (e.xmax >> 8), e.cbias + e.freq + ((1u << 31) - kProbScale - 1u), e.cbias, e.xmax8);
        tab_c[s] = make_uint2(e.freq, e.cum);
    }

    // (a state carried in from an earlier call may lie outside the range the one-compare step assumes)
    // (readfirstlane: the load goes through a generic pointer, which alone would make every branch on it, and with them
    // `written`, look divergent to the compiler)
    const uint32_t tbl_flags = (uint32_t)__builtin_amdgcn_readfirstlane((int)tbl->flags);
    const bool table_clean = x_init == kRansL && (tbl_flags & (kTableVerified | kTableNeedsGeneric | kTableDiverges)) == kTableVerified;  // uniform
    uint32_t x = x_init;  // RansEncoder::new, src/rans.rs:249-254: 2^23; a continued encoder (:288-294) brings its state
    const unsigned long long clk0 = clock64(), rt0 = wall_clock64();
    unsigned long long written = 0ull;
    uint32_t flags = 0u;
    // which branches ran (kEncPath*): counted and marked only off the clean tile and the aligned load; the clean tiles
    // are what is left at the end.  load_paths is per lane (a tail tile's lanes take different load branches).
    uint32_t paths = 0u, load_paths = 0u, slow_tiles = 0u, comp_blocks = 0u;
    asm volatile("" : "+v"(load_paths));   // zeroed here, once: otherwise every load branch of the first tile, the aligned one included, zeroes it

    const unsigned long long ntiles = (n + kEncTile - 1) / kEncTile;
    // tile j covers symbol indices [hi - 1024, hi), hi = n - j*1024 (clipped at 0)
    auto load_tile = [&](unsigned long long j) -> uint4 {
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (j >= ntiles) return v;
        const long long hi = (long long)(n - j * kEncTile);
        const long long lo = hi - kEncTile + 16ll * lane;  // first index of this lane's 16 bytes
        if (lo >= 0) {
            const uint8_t* p = sym + lo;
            const uint32_t mis = (uint32_t)((uintptr_t)p & 3u);
            const uint32_t* p4 = (const uint32_t*)(p - mis);   // stays inside the allocation: lo >= 0
            if (mis == 0u) {
                v = make_uint4(p4[0], p4[1], p4[2], p4[3]);
            } else if (lo + 20 <= (long long)n || mis == 0u) {
                const uint32_t t0 = p4[0], t1 = p4[1], t2 = p4[2], t3 = p4[3], t4 = p4[4];
                const uint32_t sh = mis * 8u;
                load_paths |= kEncPathFunnel;
                v = make_uint4((t0 >> sh) | (t1 << (32u - sh)), (t1 >> sh) | (t2 << (32u - sh)),
                               (t2 >> sh) | (t3 << (32u - sh)), (t3 >> sh) | (t4 << (32u - sh)));
            } else {
                uint32_t w[4] = {0u, 0u, 0u, 0u};
                for (int b = 0; b < 16; ++b) w[b >> 2] |= (uint32_t)p[b] << (8 * (b & 3));
                v = make_uint4(w[0], w[1], w[2], w[3]);
                load_paths |= kEncPathBytewiseEnd;
            }
        } else {
            uint32_t w[4] = {0u, 0u, 0u, 0u};
            for (int b = 0; b < 16; ++b) {
                const long long idx = lo + b;
                if (idx >= 0) w[b >> 2] |= (uint32_t)sym[idx] << (8 * (b & 3));
            }
            v = make_uint4(w[0], w[1], w[2], w[3]);
            load_paths |= kEncPathBytewiseHead;
        }
        return v;
    };

    struct BlockParams { uint4 ea, eb; uint2 ec; };
    auto sym_of = [&](int b) -> uint32_t { return tile[kEncTilePad + kEncTile - 1 - lane - b * 64]; };   // b <= 17
    auto params_of = [&](uint32_t s) -> BlockParams { BlockParams p; p.ea = tab_ab[s]; p.eb = tab_ab[256 + s]; p.ec = tab_c[s]; return p; };

    uint4 cur = load_tile(0);
    for (unsigned long long j = 0; j < ntiles; ++j) {
        if (!kExclusive && (j & 7ull) == 0ull) chain_take_turns(take_turns);
        __syncthreads();
        ((uint4*)(tile + kEncTilePad))[lane] = cur;
        __syncthreads();
        cur = load_tile(j + 1);  // in flight while this tile's 16 blocks ripple
        const long long hi = (long long)(n - j * kEncTile);
        const int valid = hi >= kEncTile ? kEncTile : (int)hi;  // tile-local indices [1024-valid, 1024)
        const int nblocks = (valid + 63) / 64;

        // Three-stage pipeline over the blocks of a tile: while block b ripples (the asm statement touches
        // no memory), the table rows of block b+1 and the symbols of block b+2 are in flight from LDS.
        uint32_t sym1 = sym_of(1);
        BlockParams nxt = params_of(sym_of(0));
        // Full tile, table known to hold only frequencies 1..4096 for the symbols that occur, room for the worst
        // case of the whole tile: no per-block activity mask, table check or capacity test; the state is carried
        // from block to block inside the vector unit (lane 0 <- lane 63 by a wave rotate) instead of through
        // two readlanes and a scalar add.
        if (table_clean && valid == kEncTile && written + 2ull * kEncTile + 4ull + 320ull <= cap) {
            uint32_t xin = x;
            // One uniform base for all stores of the tile, kTileSpan bytes below the write position (the tile emits at
            // most 2 * 1024 bytes, the capacity test above keeps the base inside the region), and a 32-bit count of
            // the tile's bytes: every store is base + a 32-bit lane offset.  Byte i of the tile
            // goes to base[kTileSpan - 1 - i]; lanes with nothing to emit write their own byte of the 64 at the
            // bottom (stream space not yet written).
            constexpr uint32_t kTileSpan = 2u * kEncTile + 320u;
            const uintptr_t tb_v = (uintptr_t)(out_end - written - kTileSpan);
            // (global, not generic: the stores take the SGPR base and the lane's 32-bit offset as they are)
            typedef __attribute__((address_space(1))) uint8_t GlobalByte;
            GlobalByte* const tb = (GlobalByte*)(((uintptr_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(tb_v >> 32)) << 32) |
                                                 (uintptr_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)tb_v));
            // (kept in a VGPR, where mbcnt wants its start value: one v_add per block instead of s_add + v_mov)
            uint32_t tw = 0u, rare_blocks = 0u;
            asm volatile("" : "+v"(tw));
            // Carried from block to block: block b's constants, its small-frequency ballot and (for a complement block) tm1
            // and kc; the symbol of block b + 1 and the LDS address of its table row; the LDS address of this lane's symbol
            // of block b + 2; the number of blocks after this one.  A run statement advances all of them in its wait-state
            // slots, a rare block in plain code.
            uint32_t xmax = nxt.ea.x, tpp = nxt.eb.x, cbias = nxt.eb.z, xmax8 = nxt.eb.w;
            CompSet cs;
            cs.rcp = nxt.ea.y; cs.rsh = nxt.ea.z; cs.g = (int32_t)nxt.ea.w; cs.cc = nxt.eb.y;
            const uint32_t tab = (uint32_t)(uintptr_t)tab_ab;
            uint32_t ad = tab + 16u * sym1;
            uint32_t sa = (uint32_t)(uintptr_t)tile + (uint32_t)(kEncTilePad + kEncTile - 1 - 2 * 64) - (uint32_t)lane;
            // C of the lane before, as a value of its own: left to the compiler, the move folds into the subtraction as
            // v_subrev_u32_dpp, and that instruction gave tm1[lane - 1] - C[lane] on the MI355X.
            // Only v_mov_b32_dpp and v_add_u32_dpp carry lane traffic here.  (Lane 0's kc is not used: a block that takes
            // this kc enters with the plain state.)
            auto kc_of = [](uint32_t tm1_, uint32_t cc_) -> uint32_t {
                uint32_t cc_prev = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)cc_, 0x138, 0xf, 0xf, true);
                asm volatile("" : "+v"(cc_prev));
                return tm1_ - cc_prev;
            };
            // stop: lanes of block b with freq <= 16; out of a run statement also all ones when the tile has no block b + 1
            unsigned long long stop = __ballot(xmax <= kRansL);
            uint32_t tm1 = xmax - 1u;
            cs.kc = kc_of(tm1, cs.cc);
            uint32_t left = (uint32_t)(kEncTile / 64 - 1);
            while ((int32_t)left >= 0) {
                if (__builtin_expect(stop == 0ull, 1)) {
                    // A run of blocks whose lanes are all in the big class (17 <= freq <= 4096, so cbias = cum): the first
                    // enters with the plain state, the others through the one-instruction edge; each block stores the
                    // byte of the block before it, the last block's emission follows the run.
                    CompSet sa_ = cs, sb_;
                    CompNext nx;
                    uint32_t u0 = tm1 - xin, u1, z, phase;                   // lane 0: the carry-in; the others are overwritten
                    ripple64_comp_run(u0, u1, z, tpp, sa_, sb_, tab, ad, sa, sym1, nx, stop, left, phase, tw, (uint32_t)lane,
                                      kTileSpan - 1u, (const void*)tb);
                    const bool swapped = phase != 0u;                         // uniform
                    const uint32_t u = swapped ? u1 : u0, cc_last = swapped ? sb_.cc : sa_.cc;
                    cs.kc = swapped ? sa_.kc : sb_.kc; cs.rcp = swapped ? sa_.rcp : sb_.rcp; cs.rsh = swapped ? sa_.rsh : sb_.rsh;
                    cs.g = swapped ? sa_.g : sb_.g; cs.cc = swapped ? sa_.cc : sb_.cc;
                    xmax = nx.xmax; tpp = nx.tpp; cbias = nx.cbias; xmax8 = nx.xmax8; tm1 = nx.tm1;
                    // x >= T exactly when u wrapped; at most one byte, x & 0xFF = ~u & 0xFF (256 divides T)
                    const bool c1 = (int32_t)u < 0;
                    const unsigned long long b1 = __ballot(c1);
                    const uint32_t o1 = __builtin_amdgcn_mbcnt_hi((uint32_t)(b1 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b1, tw));
                    tb[c1 ? kTileSpan - 1u - o1 : (uint32_t)lane] = (uint8_t)(~u & 0xFFu);
                    tw += (uint32_t)__popcll(b1);
                    // wave_ror:1 -- lane 0 of the next block's xin receives the plain state x' = C[63] - z[63]
                    xin = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(cc_last - z), 0x13C, 0xf, 0xf, true);
                } else {
                    rare_blocks += 1u;
                    const BlockParams np = params_of(sym1);   // block b + 1's rows, in flight while this block ripples
                    sym1 = sym_of(kEncTile / 64 + 1 - (int)left);   // block b + 2
                    const bool small_f = xmax <= kRansL;            // freq <= 16
                    uint32_t xout = 0u;
                    const uint32_t cprev = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)cbias, 0x138, 0xf, 0xf, true);
                    const uint32_t k0 = small_f ? 8u : 0u;
                    ripple64_clean(xin, xout, small_f ? xmax8 : xmax, k0, k0 + 8u, cs.rcp, cs.rsh, cs.g, cprev);
                    const bool c1 = xin >= xmax;
                    const bool c2 = xin >= xmax8;
                    const unsigned long long b1 = __ballot(c1), b2 = __ballot(c2);
                    const uint32_t off = __builtin_amdgcn_mbcnt_hi((uint32_t)(b1 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b1, tw)) +
                                         __builtin_amdgcn_mbcnt_hi((uint32_t)(b2 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b2, 0u));
                    tb[c1 ? kTileSpan - 1u - off : (uint32_t)lane] = (uint8_t)(xin & 0xFFu);
                    tb[c2 ? kTileSpan - 2u - off : (uint32_t)lane] = (uint8_t)((xin >> 8) & 0xFFu);
                    tw += (uint32_t)__popcll(b1) + (uint32_t)__popcll(b2);
                    // wave_ror:1 -- lane 0 of the next block's xin receives xout[63] + cbias[63]
                    xin = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(xout + cbias), 0x13C, 0xf, 0xf, false);
                    xmax = np.ea.x; cs.rcp = np.ea.y; cs.rsh = np.ea.z; cs.g = (int32_t)np.ea.w;
                    tpp = np.eb.x; cs.cc = np.eb.y; cbias = np.eb.z; xmax8 = np.eb.w;
                    stop = __ballot(xmax <= kRansL);
                    tm1 = xmax - 1u; cs.kc = kc_of(tm1, cs.cc);
                    ad = tab + 16u * sym1; sa -= 64u;
                    left -= 1u;
                }
                asm volatile("" : "+v"(tw));
            }
            written += (unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)tw);
            comp_blocks += (uint32_t)(kEncTile / 64) - rare_blocks;
            x = (uint32_t)__builtin_amdgcn_readlane((int)xin, 0);
            continue;
        }
        slow_tiles += 1u;
        paths |= valid < kEncTile ? kEncPathTail : (table_clean ? kEncPathCapRefused : kEncPathNotClean);
        for (int b = 0; b < nblocks; ++b) {
            const BlockParams curp = nxt;
            nxt = params_of(sym1);
            sym1 = sym_of(b + 2);
            const bool active = (kEncTile - 1 - (b * 64 + lane)) >= kEncTile - valid;  // all lanes except in the last tile
            uint4 ea = curp.ea;
            uint4 eb = curp.eb;
            uint2 ec = curp.ec;
            if (!active) {  // identity step
                ea = make_uint4(0xFFFFFFFFu, 0u, 0u, 0u);
                eb = make_uint4(0u, 0u, 0u, 0xFFFFFFFFu);
                ec = make_uint2(1u, 0u);
            }
            const uint32_t xmax = ea.x, xmax8 = eb.w, rcp = ea.y, rsh = ea.z;
            const int32_t g = (int32_t)ea.w;
            const uint32_t cbias = eb.z, freq = ec.x, cum = ec.y;
            const bool bad = (freq - 1u) >= kProbScale;  // freq == 0 or freq > 4096 (identity lanes carry freq 1)

            uint32_t xin = x, xout = 0u;
            if (__builtin_expect(__ballot(bad) == 0ull, 1)) {
                uint32_t cprev = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)cbias, 0x138, 0xf, 0xf, true);
                ripple64(xin, xout, xmax, xmax8, rcp, rsh, g, cprev);
                x = (uint32_t)__builtin_amdgcn_readlane((int)xout, 63) +
                    (uint32_t)__builtin_amdgcn_readlane((int)cbias, 63);
            } else {
                // exact serial path (a table entry outside 1..4096 is in use): true division
                paths |= kEncPathExact;
                uint32_t xs = x;
                for (int i = 0; i < 64; ++i) {
                    if (lane == i) xin = xs;
                    const uint32_t fi = (uint32_t)__builtin_amdgcn_readlane((int)freq, i);
                    const uint32_t ci = (uint32_t)__builtin_amdgcn_readlane((int)cum, i);
                    const uint32_t ai = (uint32_t)__builtin_amdgcn_readlane((int)active, i);
                    if (!ai) continue;
                    if (fi == 0u) { flags |= kTableDiverges; continue; }
                    const unsigned long long xm = (unsigned long long)fi << 19;  // src/rans.rs:275
                    uint32_t ys = xs;
                    while ((unsigned long long)ys >= xm) ys >>= 8;              // :276-279
                    const uint32_t qs = ys / fi, rs = ys % fi;                  // :282-283
                    xs = (qs << kProbBits) + rs + ci;                           // :284
                }
                x = xs;
            }

            // byte emission, branch-free: lane i pushes the low k_i bytes of its pre-renormalisation state
            // (identity lanes have xmax = 2^32-1 and never emit)
            const bool c1 = xin >= xmax;
            const bool c2 = xin >= xmax8;
            const unsigned long long b1 = __ballot(c1), b2 = __ballot(c2);
            const uint32_t off = __builtin_amdgcn_mbcnt_hi((uint32_t)(b1 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b1, 0u)) +
                                 __builtin_amdgcn_mbcnt_hi((uint32_t)(b2 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b2, 0u));
            const uint32_t total = (uint32_t)__popcll(b1) + (uint32_t)__popcll(b2);
            const bool room = written + total + 4ull + 64ull <= cap;  // uniform
            flags |= room ? 0u : kRansOverflow;
            paths |= room ? 0u : kEncPathNoRoom;
            uint8_t* p = out_end - 1 - (written + off);
            uint8_t* p0 = (c1 && room) ? p : dummy;
            uint8_t* p1 = (c2 && room) ? p - 1 : dummy;
            *p0 = (uint8_t)(xin & 0xFFu);
            *p1 = (uint8_t)((xin >> 8) & 0xFFu);
            written += total;
        }
    }

    // finish (src/rans.rs:298-308): push the 4 state bytes LSB first; the reversal is implicit.  keep_open: the encoder
    // object lives on (more encode / encode_symbols calls follow): the state goes back to the host instead.
    if (!keep_open) {
        if (written + 4ull + 64ull <= cap) {
            if (lane < 4) out_end[-1 - (long long)(written + lane)] = (uint8_t)((x >> (8 * lane)) & 0xFFu);
        } else {
            flags |= kRansOverflow;
            paths |= kEncPathNoRoom;
        }
        written += 4ull;
    }
    for (uint32_t bit = kEncPathFunnel; bit <= kEncPathBytewiseHead; bit <<= 1)
        paths |= __ballot((load_paths & bit) != 0u) ? bit : 0u;
    const uint32_t clean_tiles = (uint32_t)ntiles - slow_tiles;
    paths |= clean_tiles ? kEncPathClean : 0u;
    if (lane == 0) {
        res->len = written;
        res->flags = flags;
        res->final_state = x;
        res->fast_tiles = clean_tiles;
        res->slow_tiles = slow_tiles;
        res->paths = paths;
        res->comp_blocks = comp_blocks;
        res->cycles_k = (uint32_t)((clock64() - clk0) >> 10);
        res->ticks_k = (uint32_t)((wall_clock64() - rt0) >> 10);
        res->hw_id = __builtin_amdgcn_s_getreg((31 << 11) | 4);
        res->xcc_id = __builtin_amdgcn_s_getreg((31 << 11) | 20);
    }
}

// ----------------------------------------------------------------------------------
// Decode chain
//
// Per symbol the reference does (src/rans.rs:351-371):
//     slot = x & 4095; sym = cum_to_sym[slot]; x = freq*(x >> 12) + slot - cum;
//     while x < 2^23 && pos < len { x = x << 8 | byte }
// Every step depends on the previous state, including the table lookup.  To keep memory out of
// the chain the 4096-entry slot table (freq | (slot - cum) << 16) lives in 64 VGPRs and is read
// in VGPR-index mode (s_set_gpr_idx_idx row = slot[11:6], then an indexed v_readlane with lane = slot[5:0],
// whose lane select the hardware masks to 6 bits); the state, the byte window
// and all arithmetic stay on the scalar unit.  The stream bytes of a tile also sit in VGPRs
// (big-endian dwords) and are pulled into a 64-bit scalar window by the same indexed readlane, about once per 4 consumed bytes.  The only per-symbol output is the pre-update state
// (one v_writelane); symbols are recovered from those states 64 at a time by the vector unit.
// Tiles that cannot use the fast path (initial state below 2^23, stream nearly exhausted) run
// an exact scalar-lane loop.
// ----------------------------------------------------------------------------------

constexpr int kDecBlocks = 64;                 // 64-symbol blocks per fast tile
constexpr int kDecTile = kDecBlocks * 64;      // 4096 symbols
constexpr int kDecWinBytes = 33 * 64 * 4;       // stream window held in 33 VGPRs (big-endian dwords): 2 B/symbol + slack
constexpr int kDecWinLds = kDecWinBytes;
constexpr int kDecResidentRun = 65536;          // most tiles of one resident statement: 65536 * kDecWinBytes < 2^30 stream bytes

// The tile body is generated (gen/gen_rans_decode_asm.py -> rans_decode_tile.inc, which documents the
// register plan and the measured instruction costs behind its shape); per symbol, all on the scalar side:
//     row = x[11:6]; freq = F[row][x[5:0]]; bias = B[row][x[5:0]]      (VGPR-index mode + two v_readlane)
//     x = freq * (x >> 12) + bias
//     sh = shift_by_clz[clz(x)]                                         (s_flbit + s_movrels: 0, 8 or 16)
//     {window : x} <<= sh                                               (64-bit scalar shifts)
// and once per two symbols a test whether the 64-bit byte window needs its next dword.
// The vector tile (rans_decode_tile_vec.inc) evaluates umulhi(F', x) + B' on the vector unit for the whole table row
// (VGPR-index mode with the rows as src1) and brings the finished state back with ONE v_readlane per symbol: ten issue
// slots per symbol instead of eleven.  Same tables, same window, same record.
// The shadow tile (rans_decode_tile_sh.inc) is the vector tile with the state alternating between two SGPR shift pairs, so
// that the record follows the lane read and rides in the VALU -> SALU stall, with both window shifts in wait-state slots and
// the refill branch in the same stall: 22 paid slots per symbol pair instead of 23, and the branch for nothing.
#include "rans_decode_tile.inc"
#include "rans_decode_tile_vec.inc"
// The in-hand tile (rans_decode_tile_ih.inc) is the shadow tile with the next window dword always in an SGPR: the refill is
// five scalar instructions without a lane read, and its out-of-line path runs on through the pair to the odd symbol's lane
// read, where the dword after it is read from a staging row in the same stall.
#include "rans_decode_tile_sh.inc"
#include "rans_decode_tile_ih.inc"
// The resident tile (rans_decode_tile_rs.inc) is the in-hand block loop inside one statement that decodes a run of full tiles:
// the tables stay in their registers, the window rows come straight from global memory, and the symbols of a tile are
// recovered and stored while the next tile's window loads are in flight.  A kernel instance of its own (kDecTileResident);
// every tile that the statement does not take runs the in-hand tile and the code around it, as in the in-hand instance.
#include "rans_decode_tile_rs.inc"

enum DecTile : int { kDecTileClassic = 0, kDecTileVector = 1, kDecTileShadow = 2, kDecTileInhand = 3, kDecTileResident = 4 };

// Decodes nblk*64 symbols on the fast path.  slots = the chain's RansDecSlots (F' at byte 0, B' at byte 16384, read with
// 128 global loads per lane: lane4 = 4 * lane); win_addr / rec_addr are this lane's LDS byte addresses (base + 4*lane;
// the record is 2 bytes per lane).  pos = byte offset of the next stream byte inside the window.
template <int kTile>
__device__ __forceinline__ void dec_tile_fast(uint32_t& x, uint32_t& pos, const RansDecSlots* slots, uint32_t lane4,
                                              uint32_t win_addr, uint32_t rec_addr, uint32_t nblk) {
    uint32_t xo, po;
    if constexpr (kTile == kDecTileInhand || kTile == kDecTileResident)
        asm volatile(ALICE_DEC_TILE_IH_ASM
                     : [xo] "=&s"(xo), [po] "=&s"(po), [ra] "+v"(rec_addr)
                     : [xi] "s"(x), [pi] "s"(pos), [nb] "s"(nblk), [tp] "s"(slots), [l4] "v"(lane4), [wa] "v"(win_addr)
                     : ALICE_DEC_TILE_IH_CLOBBERS);
    else if constexpr (kTile == kDecTileShadow)
        asm volatile(ALICE_DEC_TILE_SH_ASM
                     : [xo] "=&s"(xo), [po] "=&s"(po), [ra] "+v"(rec_addr)
                     : [xi] "s"(x), [pi] "s"(pos), [nb] "s"(nblk), [tp] "s"(slots), [l4] "v"(lane4), [wa] "v"(win_addr)
                     : ALICE_DEC_TILE_SH_CLOBBERS);
    else if constexpr (kTile == kDecTileVector)
        asm volatile(ALICE_DEC_TILE_VEC_ASM
                     : [xo] "=&s"(xo), [po] "=&s"(po), [ra] "+v"(rec_addr)
                     : [xi] "s"(x), [pi] "s"(pos), [nb] "s"(nblk), [tp] "s"(slots), [l4] "v"(lane4), [wa] "v"(win_addr)
                     : ALICE_DEC_TILE_VEC_CLOBBERS);
    else
        asm volatile(ALICE_DEC_TILE_ASM
                     : [xo] "=&s"(xo), [po] "=&s"(po), [ra] "+v"(rec_addr)
                     : [xi] "s"(x), [pi] "s"(pos), [nb] "s"(nblk), [tp] "s"(slots), [l4] "v"(lane4), [wa] "v"(win_addr)
                     : ALICE_DEC_TILE_CLOBBERS);
    x = xo;
    pos = po;
}

// Decodes up to max_tiles full tiles in one statement (rans_decode_tile_rs.inc) and stores their symbols at out.  in_win
// = the stream at the first tile's window base, dword aligned, with at least kDecWinBytes of the stream behind it; len_rel
// = stream bytes from there on; pos = the position's offset from it (0 .. 3), on return the position after the last tile
// decoded.  The statement goes on to the next tile exactly when rans_decode_kernel would take the fast path on a whole
// window for it.  Returns the number of tiles decoded (at least 1).
__device__ __forceinline__ uint32_t dec_tiles_resident(uint32_t& x, uint32_t& pos, const uint8_t* in_win, uint32_t len_rel,
                                                       uint32_t max_tiles, uint8_t* out, const RansDecSlots* slots,
                                                       uint32_t lane4, uint32_t c2s_addr, uint32_t rec_addr) {
    // the scalar operands are uniform, but the compiler cannot always see it
    const auto uni = [](uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); };
    const auto uni64 = [&](unsigned long long v) { return (unsigned long long)uni((uint32_t)v) | ((unsigned long long)uni((uint32_t)(v >> 32)) << 32); };
    in_win = (const uint8_t*)uni64((unsigned long long)(uintptr_t)in_win);
    out = (uint8_t*)uni64((unsigned long long)(uintptr_t)out);
    len_rel = uni(len_rel);
    max_tiles = uni(max_tiles);
    x = uni(x);
    pos = uni(pos);
    uint32_t xo, po, to;
    asm volatile(ALICE_DEC_TILE_RS_ASM
                 : [xo] "=&s"(xo), [po] "=&s"(po), [to] "=&s"(to)
                 : [xi] "s"(x), [pi] "s"(pos), [nt] "s"(max_tiles), [ln] "s"(len_rel), [ip] "s"(in_win), [op] "s"(out),
                   [tp] "s"(slots), [cs] "s"(c2s_addr), [l4] "v"(lane4), [ra] "v"(rec_addr)
                 : ALICE_DEC_TILE_RS_CLOBBERS);
    x = xo;
    pos = po;
    return to;
}

// The same lookup and update with the stream exhausted: nothing is shifted in any more (src/rans.rs:365-368 reads
// no byte once pos == len), the state just evolves.  A frequency-4096 entry is only right for x >= 1 (see
// build_dec_slots); the caller checks that.
__device__ __forceinline__ void dec_tile_dry(uint32_t& x, const RansDecSlots* slots, uint32_t lane4, uint32_t rec_addr, uint32_t nblk) {
    uint32_t xo;
    asm volatile(ALICE_DEC_DRY_TILE_ASM
                 : [xo] "=&s"(xo), [ra] "+v"(rec_addr)
                 : [xi] "s"(x), [nb] "s"(nblk), [tp] "s"(slots), [l4] "v"(lane4)
                 : ALICE_DEC_DRY_TILE_CLOBBERS);
    x = xo;
}

// LDS per chain: cum_to_sym 4 KB + exact-loop symbol table 1 KB + stream window 8.25 KB + state record 8 KB
// (the exact loop's output bytes share the record's space) = 21.3 KB.  The launcher adds dynamic LDS so that at most
// four (up to 1024 chains: one per SIMD) or seven chains share a CU.
// kTile: which fast tile (classic, vector, shadow, in-hand, resident); everything around it (window staging, speculation, symbol recovery,
// the exact loop, the dry tile) is the same code.
template <bool kExclusive, int kTile>
__global__ __launch_bounds__(64) void rans_decode_kernel(const RansDecodeDesc* __restrict__ descs,
                                                         RansResult* __restrict__ results, uint32_t take_turns) {
    if constexpr (kExclusive) asm volatile("" ::: "a63");   // 226 (vector and shadow tile: 227, in-hand tile: 228, resident tile: 245) VGPRs + 64 AGPRs > 256: one chain per SIMD
    __shared__ __attribute__((aligned(16))) uint8_t c2s[kProbScale];                  // cum_to_sym
    __shared__ uint32_t symtab[256];                                                    // freq | cum << 16 (exact loop)
    __shared__ __attribute__((aligned(16))) uint8_t win[kDecWinLds];
    __shared__ __attribute__((aligned(16))) uint16_t rec[kDecTile];                     // low 16 bits of the pre-update states
    uint8_t* const obuf = (uint8_t*)rec;                                                // exact loop / unaligned output staging

    const RansDecodeDesc d = descs[blockIdx.x];
    const int lane = threadIdx.x;
    const RansDecSlots* const slots = &d.table->dec;
    uint32_t flags = 0u;
    const uint32_t tflags = d.table->flags;
    const bool big_freq = (tflags & kTableDecBig) != 0u;   // some slot belongs to a symbol of frequency 4096 (uniform)
    const bool exact_only = (tflags & kTableDecExact) != 0u;
    for (int i = lane; i < (int)kProbScale / 16; i += 64) ((uint4*)c2s)[i] = ((const uint4*)slots->c2s)[i];
    for (int i = lane; i < 256; i += 64) symtab[i] = slots->symtab[i];
    __syncthreads();
    bool slot0_big = false, one_owner = false;   // uniform
    if (big_freq) {
        const uint32_t o0 = c2s[0];
        slot0_big = symtab[o0] == kProbScale;     // freq 4096, cum 0
        bool same = true;
        for (int i = lane; i < (int)kProbScale; i += 64) same &= c2s[i] == o0;
        one_owner = __ballot(!same) == 0ull;
    }

    // RansDecoder::new (src/rans.rs:330-347); a decoder object that has decoded before resumes from its state
    // (decode / decode_n continue, :351-381)
    uint32_t x = 0u;
    unsigned long long pos = 0ull;
    const unsigned long long len = d.in_len;
    if (d.resume) {
        x = d.x0; pos = d.pos0;
    } else if (len >= 4ull) {
        x = ((uint32_t)d.in[0] << 24) | ((uint32_t)d.in[1] << 16) | ((uint32_t)d.in[2] << 8) | (uint32_t)d.in[3];
        pos = 4ull;
    }
    bool pending = false;  // renormalisation owed by the previous symbol
    const unsigned long long clk0 = clock64(), rt0 = wall_clock64();
    unsigned long long done = 0ull;
    uint32_t n_fast = 0u, n_slow = 0u, paths = 0u;

    while (done < d.n) {
        if (!kExclusive) chain_take_turns(take_turns);
        const unsigned long long remain = d.n - done;
        const uint32_t want = remain < (unsigned long long)kDecTile ? (uint32_t)remain : (uint32_t)kDecTile;
        // A frequency-4096 entry is wrong for x = 0 only (build_dec_slots), and x = 0 looks up slot 0: the dry tile is
        // safe unless such a symbol owns slot 0; if it does and owns every slot, x' = x - cum = x and a non-zero state
        // stays what it is.
        const bool dry_ok = !exact_only && (!slot0_big || (one_owner && x != 0u));
        if (want == (uint32_t)kDecTile && pos >= len && dry_ok) {
            // stream exhausted (a desynchronised decoder runs dry long before its last symbol): no window, no shifts
            uint32_t xs = (uint32_t)__builtin_amdgcn_readfirstlane((int)x);
            __syncthreads();
            dec_tile_dry(xs, slots, 4u * lane, (uint32_t)(uintptr_t)rec + 2u * lane, (uint32_t)kDecBlocks);
            x = xs;
            __syncthreads();
            const bool out_al = (((uintptr_t)(d.out + done)) & 3u) == 0u;
            paths |= kDecPathDry | (out_al ? 0u : kDecPathUnaligned);
            for (int i = lane * 4; i < kDecTile; i += 256) {
                const uint2 r4 = *(const uint2*)&rec[i];
                const uint32_t packed = (uint32_t)c2s[r4.x & (kProbScale - 1u)] | ((uint32_t)c2s[(r4.x >> 16) & (kProbScale - 1u)] << 8) |
                                        ((uint32_t)c2s[r4.y & (kProbScale - 1u)] << 16) | ((uint32_t)c2s[(r4.y >> 16) & (kProbScale - 1u)] << 24);
                if (out_al) *(uint32_t*)(d.out + done + i) = packed;
                else for (int b = 0; b < 4; ++b) d.out[done + i + b] = (uint8_t)(packed >> (8 * b));
            }
            done += (unsigned long long)kDecTile;
            ++n_fast;
            continue;
        }
        // Stage the stream window [wbase, wbase + kDecWinLds) into LDS (zero beyond len).  The base is chosen so
        // that its global address is dword aligned; when the whole window lies inside the stream all 33 dword
        // loads of a lane are issued back to back (one memory latency per tile instead of 33).
        unsigned long long wbase = pos & ~3ull;
        {
            const unsigned long long mis = (unsigned long long)((uintptr_t)(d.in + pos) & 3u);
            if (pos >= mis) wbase = pos - mis;
        }
        const bool whole = (len - wbase >= (unsigned long long)kDecWinLds) && ((((uintptr_t)(d.in + wbase)) & 3u) == 0u);
        __syncthreads();
        if constexpr (kTile == kDecTileResident) {
            // A run of full tiles in one statement: the fast path on a whole window with nothing owed, and an aligned output.
            // The statement works with 32-bit offsets from the window base: kDecResidentRun tiles move it by less than 2^30.
            if (whole && want == (uint32_t)kDecTile && pos < len && !exact_only && !pending && x >= kRansL &&
                ((((uintptr_t)(d.out + done)) & 3u) == 0u)) {
                const unsigned long long left = remain / (unsigned long long)kDecTile, rel = len - wbase;
                uint32_t nt = left < (unsigned long long)kDecResidentRun ? (uint32_t)left : (uint32_t)kDecResidentRun;
                if (!kExclusive && take_turns) nt = 1u;   // the turn is taken once per tile
                uint32_t prel = (uint32_t)(pos - wbase), xs = x;
                const uint32_t got_tiles = dec_tiles_resident(xs, prel, d.in + wbase, rel < 0xFFFFFFFFull ? (uint32_t)rel : 0xFFFFFFFFu,
                                                              nt, d.out + done, slots, 4u * lane, (uint32_t)(uintptr_t)c2s,
                                                              (uint32_t)(uintptr_t)rec + 2u * lane);
                x = xs;
                pos = wbase + prel;
                done += (unsigned long long)got_tiles * (unsigned long long)kDecTile;
                n_fast += got_tiles;
                paths |= kDecPathWhole;
                continue;
            }
        }
        if (whole) {
            const uint32_t* g = (const uint32_t*)(d.in + wbase) + lane;
            uint32_t wv[kDecWinLds / 256];
#pragma unroll
            for (int k = 0; k < kDecWinLds / 256; ++k) wv[k] = g[k * 64];
#pragma unroll
            for (int k = 0; k < kDecWinLds / 256; ++k) ((uint32_t*)win)[k * 64 + lane] = wv[k];
        } else {
            for (int i = lane * 4; i < kDecWinLds; i += 64 * 4) {
                const unsigned long long o = wbase + (unsigned long long)i;
                uint32_t w = 0u;
                for (int b = 0; b < 4; ++b)
                    if (o + (unsigned long long)b < len) w |= (uint32_t)d.in[o + b] << (8 * b);
                *(uint32_t*)(win + i) = w;
            }
        }
        __syncthreads();

        // the owed renormalisation first (src/rans.rs:365-368); it needs at most a few window bytes
        // unless the state is 0, which the exact loop below handles byte by byte
        uint32_t got = 0u;
        // Near the end of the stream the window is zero-padded and the fast tile runs speculatively: if it
        // turns out to have consumed padding (it ran dry part-way) its result is dropped and the exact loop redoes
        // the tile from the saved state.  A desynchronised decoder that eats a fraction of a bit per symbol spends
        // hundreds of tiles inside the last window; they all stay on the fast path this way.
        bool fast = (want == (uint32_t)kDecTile) && pos < len && !exact_only;
        const uint32_t x_save = x;
        const unsigned long long pos_save = pos;
        const bool pending_save = pending;
        if (fast && pending) {
            uint32_t xs = x;
            unsigned long long ps = pos;
            int guard = 0;
            while (xs < kRansL && ps < len && guard < 8) { xs = (xs << 8) | (uint32_t)win[ps - wbase]; ps += 1ull; ++guard; }
            if (xs < kRansL) { fast = false; paths |= kDecPathStillStarved; }  // still starved: leave x/pos untouched for the exact loop
            else { x = xs; pos = ps; pending = false; paths |= kDecPathPendingFed; }
        }
        if (fast && x < kRansL) { fast = false; paths |= kDecPathBelowL; }  // only the very first symbol of a malformed stream
        if (fast) {
            uint32_t prel = (uint32_t)(pos - wbase);
            uint32_t xs = (uint32_t)__builtin_amdgcn_readfirstlane((int)x);
            prel = (uint32_t)__builtin_amdgcn_readfirstlane((int)prel);
            dec_tile_fast<kTile>(xs, prel, slots, 4u * lane, (uint32_t)(uintptr_t)win + 4u * lane,
                                 (uint32_t)(uintptr_t)rec + 2u * lane, (uint32_t)kDecBlocks);
            x = xs;
            pos = wbase + prel;
            pending = false;  // the fast path renormalises right after each update
            __syncthreads();
            if (pos > len) {  // uniform: padding was consumed
                x = x_save; pos = pos_save; pending = pending_save;
                fast = false;
                paths |= kDecPathSpecDropped;
            } else {
                paths |= whole ? kDecPathWhole : kDecPathSpecKept;
            }
        }
        if (fast) {
            // symbols from the recorded states, 4 per lane; straight to global memory when the output is aligned
            const bool out_aligned = (((uintptr_t)(d.out + done)) & 3u) == 0u;
            for (int i = lane * 4; i < kDecTile; i += 256) {
                const uint2 r4 = *(const uint2*)&rec[i];
                const uint32_t packed = (uint32_t)c2s[r4.x & (kProbScale - 1u)] | ((uint32_t)c2s[(r4.x >> 16) & (kProbScale - 1u)] << 8) |
                                        ((uint32_t)c2s[r4.y & (kProbScale - 1u)] << 16) | ((uint32_t)c2s[(r4.y >> 16) & (kProbScale - 1u)] << 24);
                if (out_aligned) *(uint32_t*)(d.out + done + i) = packed;
                else *(uint32_t*)(obuf + i) = packed;
            }
            paths |= out_aligned ? 0u : kDecPathUnaligned;
            got = out_aligned ? 0u : (uint32_t)kDecTile;   // 0: nothing left in obuf to flush
            done += out_aligned ? (unsigned long long)kDecTile : 0ull;
            ++n_fast;
        } else {
            ++n_slow;
            paths |= kDecPathExact | (want < (uint32_t)kDecTile ? kDecPathTail : 0u);
            // exact scalar-lane loop over what the window can feed
            __shared__ uint32_t sh_state, sh_cnt, sh_starved;
            __shared__ unsigned long long sh_pos;
            if (lane == 0) {
                uint32_t j = 0u, xs = x;
                unsigned long long ps = pos;
                bool pend = pending;
                const unsigned long long wend = wbase + (unsigned long long)kDecWinBytes;
                bool starved = false;
                while (j < want) {
                    if (pend) {
                        while (xs < kRansL && ps < len) {
                            if (ps >= wend) { starved = true; break; }
                            xs = (xs << 8) | (uint32_t)win[ps - wbase];
                            ps += 1ull;
                        }
                        if (starved) break;
                    }
                    const uint32_t slot = xs & (kProbScale - 1u);                 // src/rans.rs:353
                    const uint32_t sy = c2s[slot];                                // :356
                    const uint32_t fc = symtab[sy];
                    xs = (fc & 0xFFFFu) * (xs >> kProbBits) + slot - (fc >> 16);  // :361-362 (mod 2^32)
                    obuf[j] = (uint8_t)sy;
                    pend = true;
                    ++j;
                }
                sh_state = xs; sh_pos = ps; sh_cnt = j; sh_starved = starved ? 1u : 0u;
            }
            __syncthreads();
            x = sh_state; pos = sh_pos; got = sh_cnt;
            paths |= sh_starved ? kDecPathStarved : 0u;
            pending = true;
        }
        __syncthreads();
        for (uint32_t i = lane; i < got; i += 64) d.out[done + i] = obuf[i];
        done += got;
    }
    // the reference renormalises right after every symbol (src/rans.rs:365-368): settle what the exact loop still owes,
    // so that the reported state and position are the decoder object's
    if (pending) {
        while (x < kRansL && pos < len) { x = (x << 8) | (uint32_t)d.in[pos]; pos += 1ull; }
    }
    if (lane == 0) {
        RansResult* const res = d.result ? d.result : results + blockIdx.x;
        res->len = pos;
        res->flags = flags;
        res->final_state = x;
        res->fast_tiles = n_fast;
        res->slow_tiles = n_slow;
        res->paths = paths;
        res->cycles_k = (uint32_t)((clock64() - clk0) >> 10);
        res->ticks_k = (uint32_t)((wall_clock64() - rt0) >> 10);
        res->hw_id = __builtin_amdgcn_s_getreg((31 << 11) | 4);
        res->xcc_id = __builtin_amdgcn_s_getreg((31 << 11) | 20);
    }
}

// ----------------------------------------------------------------------------------
// launchers
// ----------------------------------------------------------------------------------

void launch_rans_table(const uint32_t* d_hist, RansTable* d_tables, int n_chains, hipStream_t st, uint32_t n_symbols,
                       const uint32_t* d_used) {
    if (n_chains <= 0) return;
    hipLaunchKernelGGL(rans_table_kernel, dim3(n_chains), dim3(256), 0, st, d_hist, d_tables, n_symbols, d_used);
}

void launch_rans_table_from_arrays(const uint16_t* d_cum, const uint16_t* d_freq, RansTable* d_table,
                                   hipStream_t st) {
    hipLaunchKernelGGL(rans_table_from_arrays_kernel, dim3(1), dim3(256), 0, st, d_cum, d_freq, d_table);
}

void launch_rans_tables_from_arrays(const uint16_t* d_cum, const uint16_t* d_freq, RansTable* d_tables, int n,
                                    hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(rans_tables_from_arrays_kernel, dim3((unsigned)n), dim3(256), 0, st, d_cum, d_freq, d_tables);
}

// A chain is one wavefront that runs for seconds, and waves never migrate: two chains that the dispatcher puts on one
// SIMD while another SIMD idles run at 0.7 / 1.0 of their speed to the end (measured: with 900 chains, 4 single-wave
// workgroups per CU, a tenth of the SIMDs hosted two encoder waves).  Up to 1024 chains the kernels therefore claim more
// than half of a SIMD's register file, which leaves the dispatcher no choice but one chain per SIMD.  Beyond that two
// chains per SIMD cannot be avoided; they buy little (measured in round 3, see chain_take_turns above and DESIGN section
// 4.3: encoders +7 %, decoders -2 % and worse, because eight decoders on a CU saturate its one scalar unit -- not the
// "1.5x the rate of one" this comment used to promise).  Dynamic LDS that the kernels never touch then caps the workgroups
// per CU at 8 so that the surplus spreads over all CUs.
// ALICE_CHAIN_TURNS=1 switches the priority alternation of shared SIMDs on (developer A/B, scripts/chain_probe.py)
static uint32_t chain_turns_enabled() {
    static const uint32_t on = [] { const char* v = getenv("ALICE_CHAIN_TURNS"); return (v && *v == '1') ? 1u : 0u; }();
    return on;
}

// ALICE_DEC_TILE=classic / vector / shadow / inhand selects an earlier decode tile instead of the resident tile, resident names
// the default (developer A/B, read once)
static int dec_tile_choice() {
    static const int tile = [] {
        const char* v = getenv("ALICE_DEC_TILE");
        if (v && strcmp(v, "classic") == 0) return (int)kDecTileClassic;
        if (v && strcmp(v, "vector") == 0) return (int)kDecTileVector;
        if (v && strcmp(v, "shadow") == 0) return (int)kDecTileShadow;
        if (v && strcmp(v, "inhand") == 0) return (int)kDecTileInhand;
        if (v && strcmp(v, "resident") == 0) return (int)kDecTileResident;
        return (int)kDecTileResident;
    }();
    return tile;
}
using DecKernel = void (*)(const RansDecodeDesc*, RansResult*, uint32_t);
static DecKernel dec_kernel(bool exclusive) {
    switch (dec_tile_choice()) {
        case kDecTileClassic: return exclusive ? rans_decode_kernel<true, kDecTileClassic> : rans_decode_kernel<false, kDecTileClassic>;
        case kDecTileVector: return exclusive ? rans_decode_kernel<true, kDecTileVector> : rans_decode_kernel<false, kDecTileVector>;
        case kDecTileShadow: return exclusive ? rans_decode_kernel<true, kDecTileShadow> : rans_decode_kernel<false, kDecTileShadow>;
        case kDecTileInhand: return exclusive ? rans_decode_kernel<true, kDecTileInhand> : rans_decode_kernel<false, kDecTileInhand>;
        default: return exclusive ? rans_decode_kernel<true, kDecTileResident> : rans_decode_kernel<false, kDecTileResident>;
    }
}

static unsigned chain_lds_pad(int n_chains, unsigned static_lds) {
    if (n_chains <= 1024 || n_chains > 2048) return 0u;
    const unsigned want = 163840u / 8u - 1024u;   // a ninth workgroup no longer fits (160 KB of LDS per CU)
    return want > static_lds ? want - static_lds : 0u;
}

// The placement above rests on two things the compiler decides: that the empty AGPR clobber counts towards the kernel's
// register allocation, and how much static LDS the kernels use.  Both are read back from the runtime here (once), so a
// compiler update or a kernel edit that breaks either shows up as a failed check instead of a slower headline number.
struct ChainKernelFacts { bool ok; unsigned enc_regs, enc_lds, enc_wg_per_cu, dec_regs, dec_lds, dec_wg_per_cu, enc_lds_plain, dec_lds_plain; };
static const ChainKernelFacts& chain_kernel_facts() {
    static const ChainKernelFacts f = [] {
        ChainKernelFacts r{};
        hipFuncAttributes a{};
        int nb = 0;
        r.ok = true;
        auto q = [&](const void* fn, unsigned& regs, unsigned& lds, unsigned* wg) {
            if (hipFuncGetAttributes(&a, fn) != hipSuccess) { r.ok = false; (void)hipGetLastError(); return; }
            regs = (unsigned)a.numRegs; lds = (unsigned)a.sharedSizeBytes;
            if (wg) {
                if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, 64, 0) != hipSuccess) { r.ok = false; (void)hipGetLastError(); return; }
                *wg = (unsigned)nb;
            }
        };
        unsigned dummy = 0;
        q((const void*)rans_encode_kernel<true>, r.enc_regs, r.enc_lds, &r.enc_wg_per_cu);
        q((const void*)dec_kernel(true), r.dec_regs, r.dec_lds, &r.dec_wg_per_cu);
        q((const void*)rans_encode_kernel<false>, dummy, r.enc_lds_plain, nullptr);
        q((const void*)dec_kernel(false), dummy, r.dec_lds_plain, nullptr);
        return r;
    }();
    return f;
}
bool chain_kernel_occupancy(uint32_t out[6]) {
    const ChainKernelFacts& f = chain_kernel_facts();
    out[0] = f.enc_regs; out[1] = f.enc_lds; out[2] = f.enc_wg_per_cu;
    out[3] = f.dec_regs; out[4] = f.dec_lds; out[5] = f.dec_wg_per_cu;
    return f.ok;
}

void launch_rans_encode(const uint8_t* d_sym, uint64_t sym_stride, uint64_t n, const RansTable* d_tables,
                        uint8_t* d_out, uint64_t cap, RansResult* d_results, int n_chains, hipStream_t st,
                        uint64_t group_stride, uint64_t group_head, unsigned n_split, uint64_t cap_co, uint64_t cap_cg,
                        uint32_t x_init, bool keep_open) {
    if (n_chains <= 0) return;
    auto kern = n_chains <= 1024 ? rans_encode_kernel<true> : rans_encode_kernel<false>;
    const ChainKernelFacts& facts = chain_kernel_facts();   // real static LDS of the plain instance (9216 if the query failed)
    hipLaunchKernelGGL(kern, dim3(n_chains), dim3(64), chain_lds_pad(n_chains, facts.ok ? facts.enc_lds_plain : 9216u), st, d_sym,
                       (unsigned long long)sym_stride, (unsigned long long)n, d_tables, d_out,
                       (unsigned long long)cap, (unsigned long long)group_stride, (unsigned long long)group_head, n_split,
                       d_results, (unsigned long long)(cap_co ? cap_co : cap), (unsigned long long)(cap_cg ? cap_cg : cap),
                       x_init, keep_open ? 1u : 0u, chain_turns_enabled(), (const RansEncodeDesc*)nullptr);
}

void launch_rans_encode_descs(const RansEncodeDesc* d_descs, int n_chains, hipStream_t st) {
    if (n_chains <= 0) return;
    auto kern = n_chains <= 1024 ? rans_encode_kernel<true> : rans_encode_kernel<false>;
    const ChainKernelFacts& facts = chain_kernel_facts();
    hipLaunchKernelGGL(kern, dim3(n_chains), dim3(64), chain_lds_pad(n_chains, facts.ok ? facts.enc_lds_plain : 9216u), st,
                       (const uint8_t*)nullptr, 0ull, 0ull, (const RansTable*)nullptr, (uint8_t*)nullptr, 0ull, 0ull, 0ull, 0xFFFFFFFFu,
                       (RansResult*)nullptr, 0ull, 0ull, kRansL, 0u, chain_turns_enabled(), d_descs);
}

void launch_rans_decode(const RansDecodeDesc* d_descs, RansResult* d_results, int n_chains, hipStream_t st) {
    if (n_chains <= 0) return;
    auto kern = dec_kernel(n_chains <= 1024);
    const ChainKernelFacts& facts = chain_kernel_facts();
    hipLaunchKernelGGL(kern, dim3(n_chains), dim3(64), chain_lds_pad(n_chains, facts.ok ? facts.dec_lds_plain : 21776u + 256u), st, d_descs, d_results,
                       chain_turns_enabled());
}

}  // namespace alice
