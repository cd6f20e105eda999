#!/usr/bin/env python3
"""Generates rans_decode_tile.inc, rans_decode_tile_vec.inc, rans_decode_tile_sh.inc, rans_decode_tile_ih.inc and
rans_decode_tile_rs.inc: the inline-asm bodies of the rANS decode fast tile (gfx950).

    python gen_rans_decode_asm.py        writes ../rans_decode_tile.inc (classic and dry tile), ../rans_decode_tile_vec.inc,
                                         ../rans_decode_tile_sh.inc, ../rans_decode_tile_ih.inc and ../rans_decode_tile_rs.inc

fast_tile(), vector_tile(), shadow_tile(), inhand_tile(), resident_tile() and dry_tile() return the instruction lists, so the
programs can be checked without a GPU (tests/test_decode_tile_model.py, tests/test_decode_tile_vec_model.py,
tests/test_decode_tile_shadow_model.py, tests/test_decode_tile_inhand_model.py and tests/test_decode_tile_resident_model.py
interpret them); main() writes the files.
The vector tile (state update on the vector side, ten slots per symbol) is described where it is defined, below render();
the shadow tile (the record in the stall behind the lane read, both window shifts in wait-state slots, 22 paid slots per
symbol pair, the refill branch inside the stall) below the vector tile; the in-hand tile (the shadow tile's main line; the next
window dword always in s65, so the refill is five scalar instructions, and its out-of-line path runs on to the odd symbol's
lane read, where the dword after it is read in the same stall) below the shadow tile; the resident tile (the in-hand block
loop in one statement that decodes a run of full tiles: tables loaded once, window rows straight from global memory, a tile's
symbols recovered while the next tile's window loads fly) below the in-hand tile.  Which of them is the kernel's default:
dec_tile_choice() in rans.hip.

Costs measured on MI355X with scripts/probes/latency_probe.hip (one wave alone on its SIMD):
  any SALU or VALU instruction ~4 cycles; the first SALU instruction after a VALU instruction that wrote
  an SGPR (v_readlane) stalls ~20 cycles whatever it reads, while further VALU instructions do not;
  an untaken branch ~10 cycles, a taken one ~25 -- but an untaken branch directly behind a v_readlane (and the VALU
  instructions that follow it) overlaps the stall and costs next to nothing (profiles/r25_decode_shadow_probe.json).
Hence: exactly one VALU->SALU crossing per symbol (both table readlanes back to back, the record
v_writelane right behind them, inside the stall), no branch in the per-symbol code (renormalisation shift from an SGPR table
indexed by the leading-zero count), and the window refill test once per two symbols with the refill
itself out of line.

Slot budget: 11 issue slots per symbol + 3 per symbol pair = 12.5 per symbol (13 before the window carried its own fill
level: the odd symbol's wait-state slot was a no-op and the pair tail had an add that only fed a valid-bit counter).
Measured at 1011 chains (profiles/r09_decode_sentinel_window_ab.json): 38.16 ns per symbol instead of 38.93 / 38.92 (two runs
of the 13-slot tile), rans_decode 5064.6 ms per step instead of 5166.3 / 5165.0; loop phase 0 mod 8: 5072.6 ms.

The window.  s[62:63] holds V valid stream bits, left-aligned; directly below them one 1 bit, the sentinel; below that
zeros.  V is a multiple of 8 (symbols consume 0, 8 or 16 bits, refills add 32).  Invariant at the start of every symbol
pair: 32 <= V <= 63, so the upper dword s63 is all stream.  A pair consumes at most 24 bits (a 16-bit shift leaves the
state at 2^27 or above, and the next symbol's state is then at least 2^15: 8 bits at the most), so V never drops below 8
inside the tile; the sequences are nevertheless right down to V = 0.  After the pair's shifts the sentinel has moved into s63 exactly
when V <= 31, which is when 32 more bits fit: the refill test is "s62 == 0".
In the shadow tile the odd symbol's shift is applied, and the test made, in the NEXT pair's even symbol, in front of that
pair's copy of s63; the invariant 32 <= V <= 63 holds where the copy is taken, which is the only place that relies on it.
The refill.  The window dwords sit in v[192:224] with their top bit flipped (one v_xor per row at tile load), and
s64 = 0x80000000 for the whole tile.  With q = ff1(s63) the sentinel's bit in s63 (V = 31 - q):
    s[62:63] ^= {s64 : flipped dword} >> V
The flipped top bit of the new dword lands on the sentinel and leaves the true stream bit there; the other 31 bits fall on
zeros; the constant lower half supplies the new sentinel 32 bits further down.  Nine slots with the branch back (ten before).

Register plan (all literal, all listed as clobbers by the including statement):
  v[64:127]   F'[slot] = freq << 20 (row = slot[11:6], lane = slot[5:0])
  v[128:191]  B'[slot] = slot - cum - ((freq * slot) >> 12), so that x' = umulhi(F', x) + B' = freq * (x >> 12) + slot - cum
  v[192:224]  stream window, big-endian dwords, top bit flipped (dword d in row d >> 6, lane d & 63)
  v225        record: pre-update state of the 64 symbols of the current block
  s[60:61]    {window copy : x} shift pair      s[62:63] 64-bit big-endian byte window with its sentinel
  s[56:57]    shadow tile only: the odd symbols' {window copy : x} shift pair (even symbols read x' into s57, odd into s61)
  v226        vector, shadow and in-hand tile: the updated state of every slot of the current table row
  v227        in-hand tile only: staging row, the 64 window dwords from s73 on (lane d & 63 <- dword d)
  s[54:55]    in-hand tile only: EXEC of the surrounding code (the staging narrows EXEC for one v_mov)
  s[64:65]    refill pair {0x80000000 : new dword}      s[66:67] refill scratch pair (s67 is F' inside a symbol)
              (in-hand tile: s65 is ALWAYS the dword with index s73, top bit flipped)
  s67 F'   s69 B'   s70 product   s71 shift   s73 next window dword
  s74 blocks left   s75 byte-swap selector   s76 row   s77 shift of the odd symbol   s78 scratch
              (shadow tile: s77 stays pending until hole 1 of the next pair's even symbol, or the tile exit; 0 on entry)
  s79..s99    renormalisation shift (0, 8 or 16) by count-leading-zeros of the state (0 .. 20: the updated state is at
              least 2^11).  Not s100 and up: the compiler keeps those for itself and ignores them in a clobber list.
  s59         M0 of the surrounding code.  M0 is written by every s_set_gpr_idx_on (the row) and by s_flbit (the index of
              s_movrels); the compiler reserves it and does not honour an "m0" clobber, so the statement saves it first and
              restores it last -- whatever the compiler keeps in M0 survives, and the clobber lists need not name it.
Operands: %[tp] (SGPR pair: the chain's RansDecSlots in global memory, F' then B'), %[l4] (VGPR: 4 * lane),
          %[wa] (VGPR: per-lane LDS byte address of the window), %[ra] (VGPR in/out: record address, 2 B per lane),
          %[xi] %[pi] %[nb] (SGPR in), %[xo] %[po] (SGPR out).
Every tile but the resident one is a statement of its own and re-reads the tables from global memory (L2) at its top: 128
loads per 4096 symbols, because the compiled code between two statements may use v64 and up.  The resident tile loads them
once per statement, which runs over all consecutive full tiles with a whole window.  Nothing of the tables lives in LDS,
which is what bounds the number of chains a CU can host.
"""
import os

WIN_ROWS = 33   # stream window: 33 VGPRs x 64 lanes x 4 B = 8448 bytes >= 2 * 4096 symbols + refill look-ahead
REC = 192 + WIN_ROWS
M0_SAVE = "s59"
# Code placement: the block loop is pinned to a 64-byte boundary + LOOP_PHASE bytes (0 or 4).  Measured
# (scripts/chain_probe.py): loop starts at 4 mod 8 bytes decode faster than starts at 0 mod 8, and without the pin the phase
# is whatever the compiler-generated code in front of the asm statement happens to leave.  (The assembler pads with s_nop.)
LOOP_PHASE = 4


def table_loads():
    """F' then B' (contiguous in RansDecSlots): 128 rows of 256 bytes, row r into v[64 + r], lane l <- dword 64 r + l.
    global_load's immediate offset is 13 bits signed, so the scalar base moves on every 16 rows (the address is read
    when the load issues)."""
    L = [f"s_mov_b32 {M0_SAVE}, m0", "s_mov_b64 s[64:65], %[tp]"]
    for r in range(128):
        L.append(f"global_load_dword v{64 + r}, %[l4], s[64:65] offset:{256 * (r % 16)}")
        if r % 16 == 15 and r != 127:
            L.append("s_add_u32 s64, s64, 0x1000")
            L.append("s_addc_u32 s65, s65, 0")
    return L


def lookup_update(lane):
    """The part of a symbol that the fast and the dry tile share: table lookup, record, state update."""
    return ["s_bfe_u32 s76, s61, 0x60006",
            "s_set_gpr_idx_on s76, 0x1",
            "v_readlane_b32 s67, v64, s61",
            "v_readlane_b32 s69, v128, s61",
            f"v_writelane_b32 v{REC}, s61, {lane}",   # VALU work issues during the VALU->SALU stall; SALU work would not
            "s_mul_hi_u32 s70, s67, s61",
            "s_add_u32 s61, s70, s69"]


def block_end():
    return ["s_set_gpr_idx_off",
            f"ds_write_b16 %[ra], v{REC}",
            "v_add_u32_e32 %[ra], 0x80, %[ra]",
            "s_sub_u32 s74, s74, 1",
            "s_cmp_lg_u32 s74, 0",
            "s_cbranch_scc1 2b"]


def loop_pin(phase):
    assert phase in (0, 4)
    return [".p2align 6"] + ["s_nop 0"] * (phase // 4) + ["2:"]


def refill():
    """Appends the next window dword below the V <= 31 valid bits (the sentinel is in s63).  Needs s64 = 0x80000000."""
    return ["s_lshr_b32 s76, s73, 6",
            "s_set_gpr_idx_on s76, 0x1",
            "s_ff1_i32_b32 s78, s63",                   # the sentinel's bit in s63: 31 - V
            "s_sub_u32 s78, 31, s78",                   # V
            "v_readlane_b32 s65, v192, s73",
            "s_add_u32 s73, s73, 1",
            "s_lshr_b64 s[66:67], s[64:65], s78",       # into a scratch pair: s64 stays
            "s_xor_b64 s[62:63], s[62:63], s[66:67]"]


def window_fixups():
    """The window rows as the refill wants them: big-endian dwords (s75 = the byte-swap selector), top bit flipped."""
    L = []
    for r in range(WIN_ROWS):
        L.append(f"v_perm_b32 v{192 + r}, v{192 + r}, v{192 + r}, s75")
    for r in range(WIN_ROWS):
        L.append(f"v_xor_b32_e32 v{192 + r}, 0x80000000, v{192 + r}")   # see "The refill" above
    return L


def shift_table():
    L = []
    for c in range(21):
        sh = 0 if c <= 8 else (8 if c <= 16 else 16)
        L.append(f"s_mov_b32 s{79 + c}, {sh}")
    return L


def prime(pi="%[pi]"):
    """The window primed with {first dword : sentinel} << 8 * (pos & 3); unless pos & 3 == 0 that leaves V = 32 - shift < 32
    and one refill brings it to 64 - shift.  pi: the position's byte offset inside the window rows."""
    L = ["s_mov_b32 s64, 0x80000000",
         f"s_lshr_b32 s73, {pi}, 2",
         f"s_and_b32 s71, {pi}, 3",
         "s_lshl_b32 s71, s71, 3",
         "s_lshr_b32 s76, s73, 6",
         "s_set_gpr_idx_on s76, 0x1",
         "s_nop 1",
         "v_readlane_b32 s63, v192, s73",
         "s_add_u32 s73, s73, 1",
         "s_xor_b32 s63, s63, s64",                    # the true first dword
         "s_mov_b32 s62, s64",
         "s_lshl_b64 s[62:63], s[62:63], s71",
         "s_cmp_eq_u32 s62, 0",
         "s_cbranch_scc0 6f"]
    L += refill()
    L.append("6:")
    return L


def tile_entry():
    """Tables and window rows into VGPRs, the shift table, the scalar state and the primed window (shared by all fast tiles)."""
    L = table_loads()
    for r in range(WIN_ROWS):
        L.append(f"ds_read_b32 v{192 + r}, %[wa] offset:{256 * r}")
    L.append("s_mov_b32 s75, 0x00010203")
    L.append("s_waitcnt vmcnt(0) lgkmcnt(0)")
    L += window_fixups()
    L += shift_table()
    L += ["s_mov_b32 s61, %[xi]",
          "s_mov_b32 s74, %[nb]"]
    L += prime()
    return L


def tile_exit():
    """The position from the window's fill level and the dwords taken, the state, M0 back."""
    return ["s_ff1_i32_b64 s71, s[62:63]",                # 63 - V
            "s_sub_u32 s71, 63, s71",
            "s_lshr_b32 s71, s71, 3",                     # bytes read ahead of the decoder's position
            "s_lshl_b32 s70, s73, 2",
            "s_sub_u32 %[po], s70, s71",
            "s_mov_b32 %[xo], s61",
            "s_waitcnt lgkmcnt(0)",
            f"s_mov_b32 m0, {M0_SAVE}"]


def fast_tile(loop_phase=LOOP_PHASE, symbol=lookup_update):
    L = tile_entry()
    L += loop_pin(loop_phase)
    # Symbols go in pairs.  At the start of a pair the window holds at least 32 valid bits, so its upper dword s63 is all
    # stream.  s60 takes a copy of it ONCE per pair: the even symbol's shift of {s60:s61} feeds the state and leaves
    # s60 = s63 << sh with 32 - sh >= 16 valid bits on top, enough for the odd symbol (a symbol consumes at most 16 bits).
    # The window itself is shifted by the even symbol's amount in the odd symbol's wait-state slot and by the odd symbol's
    # amount in the pair tail.
    for lane in range(64):
        sh = "s77" if lane & 1 else "s71"
        L += symbol(lane)
        L.append("s_flbit_i32_b32 m0, s61")
        # one instruction must sit between the SALU write of M0 and s_movrels (wait state): the copy for the even symbol,
        # the window shift that the even symbol owes for the odd one (it touches neither M0 nor the table)
        L.append("s_mov_b32 s60, s63" if not lane & 1 else "s_lshl_b64 s[62:63], s[62:63], s71")
        L.append(f"s_movrels_b32 {sh}, s79")
        L.append(f"s_lshl_b64 s[60:61], s[60:61], {sh}")
        if lane & 1:
            L.append("s_lshl_b64 s[62:63], s[62:63], s77")
            L.append("s_cmp_eq_u32 s62, 0")             # the sentinel has left the lower dword <=> V <= 31
            L.append(f"s_cbranch_scc1 3{lane:02d}f")
            L.append(f"4{lane:02d}:")
    L += block_end()
    L.append("s_branch 5f")
    for lane in range(1, 64, 2):   # out-of-line refills
        L.append(f"3{lane:02d}:")
        L += refill()
        L.append(f"s_branch 4{lane:02d}b")
    L.append("5:")
    L += tile_exit()
    return L


def dry_tile():
    """The stream is exhausted (pos >= len), so the reference's refill loop reads nothing any more
    (src/rans.rs:365-368) and the state simply evolves: the same lookup and update, no window, no shift."""
    D = table_loads()
    D += ["s_mov_b32 s61, %[xi]",
          "s_mov_b32 s74, %[nb]",
          "s_waitcnt vmcnt(0)"]
    D += loop_pin(4)
    for lane in range(64):
        D += lookup_update(lane)
    D += block_end()
    D += ["s_mov_b32 %[xo], s61",
          "s_waitcnt lgkmcnt(0)",
          f"s_mov_b32 m0, {M0_SAVE}"]
    return D


def fast_clobbers():
    return (["memory", "scc"] + [f"s{i}" for i in range(59, 79) if i != 72] + [f"s{79 + c}" for c in range(21)] +
            [f"v{r}" for r in range(64, REC + 1)])


def dry_clobbers():
    return (["memory", "scc", "s59", "s61", "s64", "s65", "s67", "s69", "s70", "s74", "s76"] +
            [f"v{r}" for r in range(64, 192)] + [f"v{REC}"])


def render(loop_phase=LOOP_PHASE):
    def macro(name, lines):
        return f"#define {name} \\\n" + "".join(f'    "{s}\\n\\t" \\\n' for s in lines) + '    ""\n'

    def clobbers(name, regs):
        return f"#define {name} " + ", ".join(f'"{c}"' for c in regs) + "\n"

    return ("// GENERATED by gen/gen_rans_decode_asm.py -- do not edit.\n" +
            macro("ALICE_DEC_TILE_ASM", fast_tile(loop_phase)) + clobbers("ALICE_DEC_TILE_CLOBBERS", fast_clobbers()) +
            macro("ALICE_DEC_DRY_TILE_ASM", dry_tile()) + clobbers("ALICE_DEC_DRY_TILE_CLOBBERS", dry_clobbers()))


# ---- the vector tile: the state update on the vector side, one lane read per symbol ------------------------------------
# The classic symbol carries F' and B' across to the scalar unit with one v_readlane each and combines them there
# (s_mul_hi, s_add).  The vector unit can do umulhi(F', x) + B' for the whole table row at once -- x is an SGPR operand,
# every lane computes the update its slot would give -- and one v_readlane of lane x[5:0] brings back the finished x':
#     s_bfe / s_set_gpr_idx_on row, 0x6 / v_mul_hi_u32 / v_add_u32 / v_writelane (record) / v_readlane / s_flbit ...
# ten slots instead of eleven.  Mode 0x6 is SRC1_REL | SRC2_REL (M0 bits 13 and 14): the table rows are the src1 operands
# of the multiply and the add, while src0 (x, the scratch row, the source of v_readlane) and every destination stay where
# they are named, and v_readlane's src1 is an SGPR, which the mode does not touch (scripts/probes/gpr_idx_probe.hip).
# The record takes the pre-update state, so its v_writelane sits in front of the v_readlane that overwrites s61; it is
# independent of the multiply-add and stands as the one wait state that gfx940 and later want between a VALU write of a
# VGPR (the add) and a v_readlane of it.  Everything else -- pair structure, sentinel
# window, refill, shift table, block end, M0 save / restore -- is the classic tile's, and so are the tables: a
# frequency-4096 entry is F' = 2^32 - 1 and right for x >= 1 here as there.
VT = REC + 1    # scratch row: the updated state of every slot of the current table row


def lookup_update_vector(lane):
    return ["s_bfe_u32 s76, s61, 0x60006",
            "s_set_gpr_idx_on s76, 0x6",
            f"v_mul_hi_u32 v{VT}, s61, v64",               # src1 relative: the F' row
            f"v_add_u32_e64 v{VT}, v{VT}, v128",           # src1 relative: the B' row
            f"v_writelane_b32 v{REC}, s61, {lane}",        # the pre-update state, before s61 goes
            f"v_readlane_b32 s61, v{VT}, s61"]             # src0 not relative; the hardware masks the lane select to 6 bits


def vector_tile(loop_phase=LOOP_PHASE):
    """fast_tile() with lookup_update_vector() as the symbol body.  The refills and the window priming read the window rows
    as src0 of a v_readlane and switch to mode 0x1 for that, as the classic tile does; the next symbol sets 0x6 again."""
    return fast_tile(loop_phase, lookup_update_vector)


def vector_clobbers():
    return fast_clobbers() + [f"v{VT}"]


def render_vector(loop_phase=LOOP_PHASE):
    def macro(name, lines):
        return f"#define {name} \\\n" + "".join(f'    "{s}\\n\\t" \\\n' for s in lines) + '    ""\n'

    return ("// GENERATED by gen/gen_rans_decode_asm.py -- do not edit.\n" +
            macro("ALICE_DEC_TILE_VEC_ASM", vector_tile(loop_phase)) +
            "#define ALICE_DEC_TILE_VEC_CLOBBERS " + ", ".join(f'"{c}"' for c in vector_clobbers()) + "\n")


# ---- the shadow tile: the record in the stall shadow, the pair tail in the wait-state holes ------------------------------
# The vector symbol pays for its record: the v_writelane stands in front of the v_readlane because the lane read overwrites
# s61.  Here the state alternates between two shift pairs -- even symbols have x in s61 (pair s[60:61]) and read x' into s57,
# odd symbols have x in s57 (pair s[56:57]) and read x' into s61 -- so the record follows the lane read and rides in the
# VALU -> SALU stall, as the classic tile's does.  The wait state between the v_add and the v_readlane of its result then
# becomes a free hole in every symbol, next to the M0 hole between s_flbit and s_movrels: four holes per pair, which carry
# the pair's copy, the hand-over of the shifted copy to the other pair, and BOTH window shifts.  Of the pair tail only the
# sentinel compare and the branch remain; the compare stands in front of the lane read (SCC survives VALU instructions) and
# the branch directly behind lane read and record:
#     even  s_bfe / s_set_gpr_idx_on 0x6 / v_mul_hi / v_add / s_lshl_b64 window, s77 (hole 1: the PREVIOUS pair's odd shift) /
#           s_cmp_eq_u32 s62, 0 / v_readlane s57 / v_writelane (record) / s_cbranch_scc1 refill / s_flbit m0, s57 /
#           s_mov_b32 s56, s63 (hole 2: the copy) / s_movrels s71 / s_lshl_b64 s[56:57], s71
#     odd   s_bfe / s_set_gpr_idx_on 0x6 / v_mul_hi / v_add / s_lshl_b64 window, s71 (hole 1: the even symbol's shift) /
#           v_readlane s61 / v_writelane (record) / s_flbit m0, s61 / s_mov_b32 s60, s56 (hole 2: the shifted copy changes
#           pairs) / s_movrels s77 / s_lshl_b64 s[60:61], s77
# Slot budget: 13 + 11 instructions per pair of which the two records ride in the stall: 22 paid slots per pair, 11 per
# symbol (the vector tile: 10 per symbol + 3 per pair = 11.5).  The untaken branch behind the lane read overlaps the stall
# too.  Lone wave: 125.0 cycles per pair against 144.5 (136.0 with compare and branch together in front of the lane read).
# Measured at 1011 chains (profiles/r25_decode_shadow_ab.json): 31.25 ns per symbol instead of 36.93 / 36.95, rans_decode
# 4146.5 / 4147.6 ms per step instead of 4899.6 / 4903.3; loop phase 0 mod 8: 4173.3 ms.
# The window invariant is the sentinel window's, at a new place: when the copy is taken (hole 2 of the even symbol) all
# shifts of the symbols before it have been applied -- the last of them in hole 1 of this very symbol -- the test "s62 == 0"
# has seen that window, and the refill, if taken, has run: 32 <= V <= 63 at the copy.  What moves is where the odd symbol's
# shift is applied: s77 stays pending from the end of a pair to hole 1 of the next pair's even symbol, across the block end
# (nothing there reads the window) and, after the last pair, to the tile exit, which applies it before it derives the
# position.  s77 is therefore 0 on tile entry.  The refill is refill() as it is; it now runs between the lane read and the
# s_flbit, leaves M0 to the s_flbit as before, and neither s56 nor s57 is among its registers (s65 .. s67, s73, s76, s78).
# Register plan: the vector tile's plus s[56:57], the odd symbols' {window copy : x} shift pair.
def shadow_symbol(lane):
    x, xn, owed, sh = ("s61", "s57", "s77", "s71") if not lane & 1 else ("s57", "s61", "s71", "s77")
    L = [f"s_bfe_u32 s76, {x}, 0x60006",
         "s_set_gpr_idx_on s76, 0x6",
         f"v_mul_hi_u32 v{VT}, {x}, v64",
         f"v_add_u32_e64 v{VT}, v{VT}, v128",
         f"s_lshl_b64 s[62:63], s[62:63], {owed}"]         # hole 1: the shift the symbol before this one chose
    if not lane & 1:
        L.append("s_cmp_eq_u32 s62, 0")                    # the sentinel has left the lower dword <=> V <= 31
    L += [f"v_readlane_b32 {xn}, v{VT}, {x}",
          f"v_writelane_b32 v{REC}, {x}, {lane}"]          # x is still there: the record rides in the stall
    if not lane & 1:
        L += [f"s_cbranch_scc1 3{lane:02d}f",
              f"4{lane:02d}:"]
    pair = "s[56:57]" if not lane & 1 else "s[60:61]"
    L += [f"s_flbit_i32_b32 m0, {xn}",
          "s_mov_b32 s56, s63" if not lane & 1 else "s_mov_b32 s60, s56",   # hole 2
          f"s_movrels_b32 {sh}, s79",
          f"s_lshl_b64 {pair}, {pair}, {sh}"]
    return L


def shadow_tile(loop_phase=LOOP_PHASE):
    L = tile_entry()
    L.append("s_mov_b32 s77, 0")                           # no shift is pending
    L += loop_pin(loop_phase)
    for lane in range(64):
        L += shadow_symbol(lane)
    L += block_end()
    L.append("s_branch 5f")
    for lane in range(0, 64, 2):   # out-of-line refills
        L.append(f"3{lane:02d}:")
        L += refill()
        L.append(f"s_branch 4{lane:02d}b")
    L += ["5:",
          "s_lshl_b64 s[62:63], s[62:63], s77"]            # the last odd symbol's shift is still pending
    L += tile_exit()
    return L


def shadow_clobbers():
    return vector_clobbers() + ["s56", "s57"]


def render_shadow(loop_phase=LOOP_PHASE):
    def macro(name, lines):
        return f"#define {name} \\\n" + "".join(f'    "{s}\\n\\t" \\\n' for s in lines) + '    ""\n'

    return ("// GENERATED by gen/gen_rans_decode_asm.py -- do not edit.\n" +
            macro("ALICE_DEC_TILE_SH_ASM", shadow_tile(loop_phase)) +
            "#define ALICE_DEC_TILE_SH_CLOBBERS " + ", ".join(f'"{c}"' for c in shadow_clobbers()) + "\n")


# ---- the in-hand tile: the refill takes a dword that is already in an SGPR -----------------------------------------------
# The shadow tile's refill switches the index mode and reads the window dword with a lane read of its own: a second
# VALU -> SALU crossing, then the taken branch back.  Here s65 ALWAYS holds the window dword with index s73 (the next one
# that is not yet in the window, top bit flipped), so the refill is SALU work on registers that are already there:
#     s_ff1_i32_b32 s78, s63 / s_sub_u32 s78, 31, s78 / s_lshr_b64 s[66:67], s[64:65], s78 /
#     s_xor_b64 s[62:63], s[62:63], s[66:67] / s_add_u32 s73, s73, 1
# The dword after it is fetched by a v_readlane that stands directly behind the ODD symbol's own lane read, so both pay one
# crossing.  That read must not switch the index mode (the odd symbol's multiply-add needs 0x6 and src0 is not relative in
# 0x6), so it reads a staging row v227 that holds the 64 window dwords from s73 on, lane d & 63 <- dword d (the hardware masks
# the lane select to 6 bits).  v227 is rebuilt in tile_entry() and at every block end from rows s73 >> 6 (all lanes) and
# (s73 >> 6) + 1 (the lanes below s73 & 63, through EXEC); a block consumes at most 24 dwords and reads one ahead, well inside
# the 64.  Row 33 is the record row: those lanes stand for dwords behind the 33-row window, which no tile reaches.
# The out-of-line path of an even symbol does not return at once: behind the refill it carries the even symbol's tail and the
# odd symbol's head, copied from the main line, up to the odd symbol's lane read, the prefetch and the record, and only then
# branches back, to the odd symbol's s_flbit (label 6xx):
#     3xx: refill (5) / s_flbit m0, s57 / s_mov_b32 s56, s63 / s_movrels s71 / s_lshl_b64 s[56:57], s71 /
#          s_bfe / s_set_gpr_idx_on 0x6 / v_mul_hi / v_add / s_lshl_b64 window, s71 /
#          v_readlane s61 / v_readlane s65, v227, s73 / v_writelane (record) / s_branch 6xx
# The main line is the shadow tile's, instruction for instruction; only the label 6xx in the odd symbol is new.  Two refills in
# consecutive pairs work: the next even symbol tests the refilled window, and s65 is the next dword by then.
# Register plan: the shadow tile's plus v227 (staging row) and s[54:55] (EXEC of the surrounding code).
VW = VT + 1     # staging row: the 64 window dwords from s73 on
EXEC_SAVE = "s[54:55]"


def stage():
    """v227[d & 63] = window dword d for s73 <= d < s73 + 64.  Leaves index mode 0x1 on and EXEC as it was."""
    return ["s_lshr_b32 s76, s73, 6",
            "s_set_gpr_idx_on s76, 0x1",
            f"v_mov_b32_e32 v{VW}, v192",                  # src0 relative: row s73 >> 6
            "s_bfm_b64 exec, s73, 0",                      # the lanes below s73 & 63 (the width is S0[5:0])
            f"v_mov_b32_e32 v{VW}, v193",                  # ... take the row after it
            f"s_mov_b64 exec, {EXEC_SAVE}"]


def inhand_refill():
    """refill() without its lane read: the dword is in s65.  Needs s64 = 0x80000000; the caller reads the next s65."""
    return ["s_ff1_i32_b32 s78, s63",                      # the sentinel's bit in s63: 31 - V
            "s_sub_u32 s78, 31, s78",                      # V
            "s_lshr_b64 s[66:67], s[64:65], s78",
            "s_xor_b64 s[62:63], s[62:63], s[66:67]",
            "s_add_u32 s73, s73, 1"]


def inhand_entry():
    L = tile_entry()
    at = L.index(f"s_mov_b32 {M0_SAVE}, m0")
    L.insert(at + 1, f"s_mov_b64 {EXEC_SAVE}, exec")
    L += ["s_lshr_b32 s76, s73, 6",                        # prime s65: the dword with index s73
          "s_set_gpr_idx_on s76, 0x1",
          "s_nop 1",
          "v_readlane_b32 s65, v192, s73"]
    L += stage()
    L.append("s_mov_b32 s77, 0")                           # no shift is pending
    return L


def inhand_path(lane):
    """The out-of-line path of the even symbol `lane`: refill, the rest of the pair up to the odd symbol's record."""
    even, odd = shadow_symbol(lane), shadow_symbol(lane + 1)
    rd = odd.index(f"v_readlane_b32 s61, v{VT}, s57")
    return ([f"3{lane:02d}:"] + inhand_refill() + even[even.index(f"4{lane:02d}:") + 1:] + odd[:rd + 1] +
            [f"v_readlane_b32 s65, v{VW}, s73",            # shares the odd symbol's crossing; src0 is not relative in 0x6
             odd[rd + 1],                                  # the record
             f"s_branch 6{lane:02d}b"])


def inhand_tile(loop_phase=LOOP_PHASE):
    L = inhand_entry()
    L += loop_pin(loop_phase)
    for lane in range(64):
        body = shadow_symbol(lane)
        if lane & 1:
            body.insert(body.index("s_flbit_i32_b32 m0, s61"), f"6{lane - 1:02d}:")
        L += body
    L += stage()
    L += block_end()
    L.append("s_branch 5f")
    for lane in range(0, 64, 2):
        L += inhand_path(lane)
    L += ["5:",
          "s_lshl_b64 s[62:63], s[62:63], s77"]            # the last odd symbol's shift is still pending
    L += tile_exit()
    return L


def inhand_clobbers():
    return shadow_clobbers() + ["s54", "s55", f"v{VW}"]


def render_inhand(loop_phase=LOOP_PHASE):
    def macro(name, lines):
        return f"#define {name} \\\n" + "".join(f'    "{s}\\n\\t" \\\n' for s in lines) + '    ""\n'

    return ("// GENERATED by gen/gen_rans_decode_asm.py -- do not edit.\n" +
            macro("ALICE_DEC_TILE_IH_ASM", inhand_tile(loop_phase)) +
            "#define ALICE_DEC_TILE_IH_CLOBBERS " + ", ".join(f'"{c}"' for c in inhand_clobbers()) + "\n")


# ---- the resident tile: one statement decodes a run of full tiles, the tables stay in their registers ---------------------
# The tiles above are one asm statement per 4096 symbols, and compiled code runs between two statements: the window goes
# global -> VGPR -> LDS -> VGPR, the tables are loaded again because the compiler may use v64 and up, and the symbols are
# recovered from the record only after the statement.  Measured in the chain (profiles/r30_decode_edge_probe.json): 9.5 k
# cycles per tile outside the block loop -- 1.8 k window fetch and staging, 2.3 k statement entry, 5.2 k recovery.
# This statement keeps going while the kernel's own conditions for the next fast `whole` tile hold, evaluated on the scalar
# side at the end of every tile (tile_conditions()).  Per statement: M0 and EXEC saved, the 128 table loads, the shift table.
# Per tile: the 33 window loads straight from global memory into v[192:224] (lane l of row r <- dword 64 r + l of the window
# base, which is the position rounded down to a dword: the statement's stream pointer is dword aligned); while they fly
# the PREVIOUS tile's symbols are recovered from the record through cum_to_sym and stored (recover()); then the wait, the
# byte swap and the flipped top bits, the priming, and the in-hand block loop instruction for instruction.  On leaving the
# last tile is recovered.  All positions inside the statement are 32-bit offsets from the statement's stream pointer; the
# kernel bounds the tile count so that they cannot wrap, and clamps the stream length it passes in accordingly.
# Register plan: the in-hand tile's plus v228 (the block loop's moving record address), v229 (record read address,
# 8 B per lane), v[230:233] (two pairs of record words), v[234:241] (two sets of four slot addresses / symbols), v242 / v243
# (packed symbols), s[40:41] (window load address), s[42:43] (output address of the tile being recovered), s44 (window base),
# s45 (tiles left), s46 (tiles done), s48 (position).
# Operands: %[ip] (SGPR pair: stream pointer, dword aligned), %[ln] (stream bytes from there, clamped to 32 bits), %[pi]
# (position, 0 .. 3), %[nt] (most tiles to decode, at least 1), %[op] (SGPR pair: output of the first tile, dword aligned),
# %[cs] (SGPR: LDS address of cum_to_sym), %[ra] (VGPR in: record address, 2 B per lane), %[xi], %[tp], %[l4]; out: %[xo],
# %[po], %[to] (tiles decoded).
RS_RA, RS_RB, RS_A, RS_B, RS_P = VW + 1, VW + 2, (VW + 3, VW + 5), (VW + 7, VW + 11), (VW + 15, VW + 16)
RECOVER_TRIPS = 16
WIN_BYTES = WIN_ROWS * 256


def window_loads():
    """Lane l of row r reads dword 64 r + l of the stream from s44 on; the scalar base moves every 16 rows (13-bit offset)."""
    L = ["s_and_b32 s44, s48, 0xfffffffc",
         "s_mov_b64 s[40:41], %[ip]",
         "s_add_u32 s40, s40, s44",
         "s_addc_u32 s41, s41, 0"]
    for r in range(WIN_ROWS):
        L.append(f"global_load_dword v{192 + r}, %[l4], s[40:41] offset:{256 * (r % 16)}")
        if r % 16 == 15:
            L.append("s_add_u32 s40, s40, 0x1000")
            L.append("s_addc_u32 s41, s41, 0")
    return L


def recover():
    """Symbols of the tile in the record, four per lane and trip: lane l of trip t reads states 256 t + 4 l .. + 3 (one
    ds_read_b64), looks their slots up in cum_to_sym (four ds_read_u8) and stores the packed dword at s[42:43] + 256 t + 4 l.
    Software pipeline: the record words are read two trips ahead, the symbols are packed and stored one trip after their
    lookups were issued; LDS returns in order, so every wait is a count of the LDS instructions issued since.  Then the
    output address moves on by a tile."""
    L, issued = [], []

    def issue(tag, line):
        issued.append(tag)
        L.append(line)

    def wait(tag):
        after = len(issued) - 1 - max(i for i, t in enumerate(issued) if t == tag)
        L.append(f"s_waitcnt lgkmcnt({after})")

    def read(t):
        issue(("a", t), f"ds_read_b64 v[{RS_A[t % 2]}:{RS_A[t % 2] + 1}], v{RS_RB} offset:{512 * t}")

    def finish(t):
        b, p = RS_B[t % 2], RS_P[t % 2]
        wait(("b", t))
        L.extend([f"v_lshl_or_b32 v{p}, v{b + 1}, 8, v{b}",
                  f"v_lshl_or_b32 v{p}, v{b + 2}, 16, v{p}",
                  f"v_lshl_or_b32 v{p}, v{b + 3}, 24, v{p}",
                  f"global_store_dword %[l4], v{p}, s[42:43] offset:{256 * t}"])

    read(0)
    read(1)
    for t in range(RECOVER_TRIPS):
        a, b = RS_A[t % 2], RS_B[t % 2]
        wait(("a", t))
        L.extend([f"v_and_b32_e32 v{b}, 0xfff, v{a}",
                  f"v_bfe_u32 v{b + 1}, v{a}, 16, 12",
                  f"v_and_b32_e32 v{b + 2}, 0xfff, v{a + 1}",
                  f"v_bfe_u32 v{b + 3}, v{a + 1}, 16, 12"])
        for k in range(4):
            L.append(f"v_add_u32_e32 v{b + k}, %[cs], v{b + k}")
        for k in range(4):
            issue(("b", t), f"ds_read_u8 v{b + k}, v{b + k}")
        if t + 2 < RECOVER_TRIPS:
            read(t + 2)
        if t:
            finish(t - 1)
    finish(RECOVER_TRIPS - 1)
    L += ["s_add_u32 s42, s42, 0x1000",
          "s_addc_u32 s43, s43, 0"]
    return L


def tile_conditions():
    """What lets rans_decode_kernel take the fast `whole` path for the next tile, in its order: a full tile is left to
    decode, the stream is not exhausted, the state is renormalised, and the whole window lies inside the stream (its base
    is dword aligned because the statement's stream pointer is).  Leaves to 9 unless all hold."""
    return ["s_add_u32 s46, s46, 1",
            "s_sub_u32 s45, s45, 1",
            "s_cmp_eq_u32 s45, 0",
            "s_cbranch_scc1 9f",
            "s_cmp_ge_u32 s48, %[ln]",
            "s_cbranch_scc1 9f",
            "s_cmp_lt_u32 s61, 0x800000",
            "s_cbranch_scc1 9f",
            "s_and_b32 s70, s48, 0xfffffffc",
            "s_sub_u32 s70, %[ln], s70",
            f"s_cmp_lt_u32 s70, {WIN_BYTES}",
            "s_cbranch_scc1 9f"]


def resident_tile(loop_phase=LOOP_PHASE):
    ra = lambda lines: [s.replace("%[ra]", f"v{RS_RA}") for s in lines]
    L = table_loads()
    L.insert(1, f"s_mov_b64 {EXEC_SAVE}, exec")
    L += shift_table()
    L += ["s_mov_b32 s75, 0x00010203",
          "s_mov_b32 s61, %[xi]",
          "s_mov_b32 s48, %[pi]",
          "s_mov_b32 s45, %[nt]",
          "s_mov_b32 s46, 0",
          "s_mov_b64 s[42:43], %[op]",
          f"v_lshrrev_b32_e32 v{RS_RB}, 1, %[l4]",         # record read address: 8 B per lane = ra + 6 * lane
          f"v_add_u32_e32 v{RS_RB}, %[l4], v{RS_RB}",
          f"v_add_u32_e32 v{RS_RB}, %[ra], v{RS_RB}",
          "7:"]
    L += window_loads()
    L += ["s_cmp_eq_u32 s46, 0",                           # the first tile has no tile in front of it to recover
          "s_cbranch_scc1 8f"]
    L += recover()
    L += ["8:",
          f"v_mov_b32_e32 v{RS_RA}, %[ra]",
          "s_waitcnt vmcnt(0)"]
    L += window_fixups()
    L += ["s_mov_b32 s74, 64",
          "s_sub_u32 s70, s48, s44"]                       # the position inside the window rows: pos & 3
    L += prime("s70")
    L += ["s_lshr_b32 s76, s73, 6",                        # prime s65: the dword with index s73
          "s_set_gpr_idx_on s76, 0x1",
          "s_nop 1",
          "v_readlane_b32 s65, v192, s73"]
    L += stage()
    L.append("s_mov_b32 s77, 0")                           # no shift is pending
    L += loop_pin(loop_phase)
    for lane in range(64):
        body = shadow_symbol(lane)
        if lane & 1:
            body.insert(body.index("s_flbit_i32_b32 m0, s61"), f"6{lane - 1:02d}:")
        L += body
    L += stage()
    L += ra(block_end())
    L.append("s_branch 5f")
    for lane in range(0, 64, 2):
        L += inhand_path(lane)
    L += ["5:",
          "s_lshl_b64 s[62:63], s[62:63], s77",            # the last odd symbol's shift is still pending
          "s_ff1_i32_b64 s71, s[62:63]",                   # 63 - V
          "s_sub_u32 s71, 63, s71",
          "s_lshr_b32 s71, s71, 3",                        # bytes read ahead of the decoder's position
          "s_lshl_b32 s70, s73, 2",
          "s_sub_u32 s70, s70, s71",
          "s_add_u32 s48, s44, s70",
          "s_waitcnt lgkmcnt(0)"]
    L += tile_conditions()
    L += ["s_branch 7b",
          "9:"]
    L += recover()
    L += ["s_waitcnt vmcnt(0)",
          "s_mov_b32 %[xo], s61",
          "s_mov_b32 %[po], s48",
          "s_mov_b32 %[to], s46",
          f"s_mov_b32 m0, {M0_SAVE}"]
    return L


def resident_clobbers():
    return (inhand_clobbers() + [f"v{r}" for r in range(RS_RA, RS_P[1] + 1)] +
            ["s40", "s41", "s42", "s43", "s44", "s45", "s46", "s48"])


def render_resident(loop_phase=LOOP_PHASE):
    def macro(name, lines):
        return f"#define {name} \\\n" + "".join(f'    "{s}\\n\\t" \\\n' for s in lines) + '    ""\n'

    return ("// GENERATED by gen/gen_rans_decode_asm.py -- do not edit.\n" +
            macro("ALICE_DEC_TILE_RS_ASM", resident_tile(loop_phase)) +
            "#define ALICE_DEC_TILE_RS_CLOBBERS " + ", ".join(f'"{c}"' for c in resident_clobbers()) + "\n")


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    out = os.path.join(here, "..", "rans_decode_tile.inc")
    with open(out, "w") as f:
        f.write(render())
    print("wrote", out, len(fast_tile()), "asm lines")
    out = os.path.join(here, "..", "rans_decode_tile_vec.inc")
    with open(out, "w") as f:
        f.write(render_vector())
    print("wrote", out, len(vector_tile()), "asm lines")
    out = os.path.join(here, "..", "rans_decode_tile_sh.inc")
    with open(out, "w") as f:
        f.write(render_shadow())
    print("wrote", out, len(shadow_tile()), "asm lines")
    out = os.path.join(here, "..", "rans_decode_tile_ih.inc")
    with open(out, "w") as f:
        f.write(render_inhand())
    print("wrote", out, len(inhand_tile()), "asm lines")
    out = os.path.join(here, "..", "rans_decode_tile_rs.inc")
    with open(out, "w") as f:
        f.write(render_resident())
    print("wrote", out, len(resident_tile()), "asm lines")


if __name__ == "__main__":
    main()
