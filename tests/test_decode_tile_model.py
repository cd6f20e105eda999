"""The generated rANS decode tile (alice-codec_amd/csrc/gen/gen_rans_decode_asm.py) run on a model of the machine.

A small interpreter for exactly the instructions the tile uses executes the generator's instruction list on streams
that the numpy oracle encoded, and the recorded states (-> symbols through cum_to_sym), the final state and the final
position must be the oracle decoder's.  At every symbol-pair start the 64-bit window must hold 32 <= V <= 63 valid bits
above its sentinel bit, V a multiple of 8, and those bits must be the stream at the decoder's position.

What the model knows: SALU arithmetic / shifts / compares / branches with SCC, s_flbit / s_ff1, s_movrels with M0,
VGPR-index mode (s_set_gpr_idx_on / off; the index lives in M0[7:0], which s_flbit overwrites), v_readlane / v_writelane
with the 6-bit lane mask, v_perm, the table loads (global memory) and the window / record traffic (LDS).  An instruction
it does not know is an error.  It cannot see wait-state hazards, except the one slot that s_movrels needs after a write of
M0; the GPU tests cover the rest.

A well-formed table keeps the state at 2^23 or above after every symbol, and then a symbol pair consumes at most 24 bits
(after a 16-bit shift the state is at least 2^27, so the next symbol's is at least 2^15 and shifts by 8 at the most).  From
V >= 32 the tile therefore never drains the window below V = 8; test_refill_sequence_alone covers V = 0 .. 24 directly,
V = 0 included (two 16-bit shifts from V = 32), which only a malformed table can reach."""
import functools
import importlib.util
import os
import sys

import numpy as np
import pytest

from oracle import alice_oracle_np as onp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_tile_ref as R  # noqa: E402
from decode_tile_ref import KINDS, M32, TILE  # noqa: E402

M0 = 124            # M0's SGPR number
WIN_BYTES = 33 * 64 * 4

# the statement's operands, bound the way a compiler might bind them
OPERANDS = {"%[xi]": "s10", "%[pi]": "s11", "%[nb]": "s12", "%[tp]": "s[14:15]", "%[xo]": "s16", "%[po]": "s17",
            "%[l4]": "v0", "%[wa]": "v1", "%[ra]": "v2"}
TABLE_ADDR = 0x00007F12FFFFC000   # the 64-bit base crosses a 4 GiB boundary inside the tables: the scalar add must carry
WIN_BASE, REC_BASE, LDS_BYTES = 5120, 5120 + WIN_BYTES, 5120 + WIN_BYTES + 2 * TILE


def _generator():
    spec = importlib.util.spec_from_file_location(
        "gen_rans_decode_asm", os.path.join(ROOT, "alice-codec_amd", "csrc", "gen", "gen_rans_decode_asm.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def gen():
    return _generator()


class Machine:
    """One wave, all 64 lanes active.  The program is translated once into closures; run() executes from the top."""

    def __init__(self, program):
        self.S = [0xDEAD0000 + i for i in range(128)]   # nothing may rely on a register it did not write
        self.scc = 0
        self.idx_on = False
        self.V = np.full((256, 64), 0xA5A5A5A5, np.uint32)
        self.lds = np.zeros(LDS_BYTES, np.uint8)
        self.table = None               # u32 array at TABLE_ADDR
        self.watch = {}                 # pc -> callback(machine)
        self.executed = 0
        self.m0_written_at = -10
        self.text = []
        labels = []
        for line in program:
            for k, v in OPERANDS.items():
                line = line.replace(k, v)
            line = line.strip()
            if line.startswith("."):
                continue
            if line.endswith(":"):
                labels.append((line[:-1], len(self.text)))
                continue
            self.text.append(line)
        self.labels = labels
        self.code = [self._translate(pc, line) for pc, line in enumerate(self.text)]

    # ---- operands
    def _target(self, pc, ref):
        name, way = ref[:-1], ref[-1]
        if way == "f":
            return min(at for n, at in self.labels if n == name and at > pc)
        assert way == "b", ref
        return max(at for n, at in self.labels if n == name and at <= pc)

    @staticmethod
    def _sreg(a):
        if a == "m0":
            return M0
        if a.startswith("s["):
            lo, hi = a[2:-1].split(":")
            assert int(hi) == int(lo) + 1 and int(lo) % 2 == 0, a
            return int(lo)
        assert a[0] == "s" and a[1:].isdigit(), a
        return int(a[1:])

    def _src(self, a, wide=False):
        S = self.S
        if a[0].isdigit():
            c = int(a, 0)
            return lambda: c
        n = self._sreg(a)
        if wide:
            assert a.startswith("s["), a
            return lambda: S[n] | (S[n + 1] << 32)
        assert not a.startswith("s["), a
        return lambda: S[n]

    def _dst(self, pc, a, wide=False):
        S = self.S
        n = self._sreg(a)
        assert n < 100 or n == M0, a      # the tile keeps off the registers the compiler reserves
        if wide:
            assert a.startswith("s["), a

            def put64(v):
                S[n] = v & M32
                S[n + 1] = (v >> 32) & M32
            return put64
        if n == M0:
            def put_m0(v):
                S[M0] = v & M32
                self.m0_written_at = self.executed
            return put_m0

        def put(v):
            S[n] = v & M32
        return put

    @staticmethod
    def _vreg(a):
        assert a[0] == "v" and a[1:].isdigit(), a
        return int(a[1:])

    def _src0_row(self, n):
        """VGPR-index mode: src0 of a VALU instruction is relative when MODE.gpr_idx_en and M0[12] (SRC0_REL)."""
        if self.idx_on and (self.S[M0] >> 12) & 1:
            n += self.S[M0] & 0xFF
        assert n < 256
        return n

    def _dst_row(self, n):
        if self.idx_on and (self.S[M0] >> 15) & 1:
            n += self.S[M0] & 0xFF
        assert n < 256
        return n

    # ---- instructions
    def _translate(self, pc, line):
        op, _, rest = line.partition(" ")
        args = [a.strip() for a in rest.split(",")] if rest else []
        S, V = self.S, self.V

        def scc_nz(put, f):
            def run():
                r = f()
                put(r)
                self.scc = int(r != 0)
            return run

        if op in ("s_nop", "s_waitcnt"):
            return lambda: None
        if op in ("s_mov_b32", "s_mov_b64"):
            w = op.endswith("64")
            put, a = self._dst(pc, args[0], w), self._src(args[1], w)
            return lambda: put(a())
        if op in ("s_add_u32", "s_addc_u32", "s_sub_u32"):
            put, a, b = self._dst(pc, args[0]), self._src(args[1]), self._src(args[2])

            def arith():
                r = a() - b() if op == "s_sub_u32" else a() + b() + (self.scc if op == "s_addc_u32" else 0)
                put(r)
                self.scc = int(r < 0 or r > M32)
            return arith
        if op in ("s_lshl_b32", "s_lshr_b32", "s_lshl_b64", "s_lshr_b64"):
            w = op.endswith("64")
            bits = 64 if w else 32
            put, a, b = self._dst(pc, args[0], w), self._src(args[1], w), self._src(args[2])
            if "lshl" in op:
                return scc_nz(put, lambda: (a() << (b() & (bits - 1))) & ((1 << bits) - 1))
            return scc_nz(put, lambda: a() >> (b() & (bits - 1)))
        if op in ("s_and_b32", "s_xor_b32", "s_xor_b64", "s_or_b64"):
            w = op.endswith("64")
            put, a, b = self._dst(pc, args[0], w), self._src(args[1], w), self._src(args[2], w)
            f = {"and": lambda: a() & b(), "xor": lambda: a() ^ b(), "or": lambda: a() | b()}[op.split("_")[1]]
            return scc_nz(put, f)
        if op == "s_bfe_u32":
            put, a, b = self._dst(pc, args[0]), self._src(args[1]), self._src(args[2])
            return scc_nz(put, lambda: (a() >> (b() & 31)) & ((1 << ((b() >> 16) & 0x7F)) - 1))
        if op == "s_mul_hi_u32":
            put, a, b = self._dst(pc, args[0]), self._src(args[1]), self._src(args[2])
            return lambda: put((a() * b()) >> 32)
        if op == "s_flbit_i32_b32":
            put, a = self._dst(pc, args[0]), self._src(args[1])
            return lambda: put(32 - a().bit_length() if a() else M32)
        if op in ("s_ff1_i32_b32", "s_ff1_i32_b64"):
            put, a = self._dst(pc, args[0]), self._src(args[1], op.endswith("64"))
            return lambda: put((a() & -a()).bit_length() - 1 if a() else M32)
        if op == "s_movrels_b32":
            put, base = self._dst(pc, args[0]), self._sreg(args[1])

            def movrels():
                assert self.executed - self.m0_written_at >= 2, f"pc {pc}: s_movrels right behind a write of M0"
                n = base + S[M0]
                assert base <= n <= base + 20, f"pc {pc}: s_movrels index {S[M0]} outside the shift table"
                put(S[n])
            return movrels
        if op in ("s_cmp_eq_u32", "s_cmp_lg_u32"):
            a, b = self._src(args[0]), self._src(args[1])
            eq = op == "s_cmp_eq_u32"

            def cmp():
                self.scc = int((a() == b()) == eq)
            return cmp
        if op in ("s_cbranch_scc0", "s_cbranch_scc1"):
            to, want = self._target(pc, args[0]), int(op[-1])
            return lambda: to if self.scc == want else None
        if op == "s_branch":
            to = self._target(pc, args[0])
            return lambda: to
        if op == "s_set_gpr_idx_on":
            a, imm = self._src(args[0]), int(args[1], 0)

            def idx_on():
                S[M0] = (S[M0] & ~0xF0FF & M32) | (a() & 0xFF) | (imm << 12)
                self.m0_written_at = self.executed
                self.idx_on = True
            return idx_on
        if op == "s_set_gpr_idx_off":
            def idx_off():
                self.idx_on = False
            return idx_off
        if op == "v_readlane_b32":
            put, row = self._dst(pc, args[0]), self._vreg(args[1])
            lane = self._src(args[2])
            return lambda: put(int(V[self._src0_row(row), lane() & 63]))
        if op == "v_writelane_b32":
            row, a, lane = self._vreg(args[0]), self._src(args[1]), self._src(args[2])

            def writelane():
                V[self._dst_row(row), lane() & 63] = a()
            return writelane
        if op == "v_perm_b32":
            d, r0, r1, sel = self._vreg(args[0]), self._vreg(args[1]), self._vreg(args[2]), self._src(args[3])

            def perm():
                both = V[r1].astype(np.uint64) | (V[self._src0_row(r0)].astype(np.uint64) << np.uint64(32))
                out = np.zeros(64, np.uint32)
                for k in range(4):
                    pick = (sel() >> (8 * k)) & 0xFF
                    assert pick < 8, "only byte picks are modelled"
                    out |= ((both >> np.uint64(8 * pick)) & np.uint64(0xFF)).astype(np.uint32) << np.uint32(8 * k)
                V[self._dst_row(d)] = out
            return perm
        if op in ("v_xor_b32_e32", "v_add_u32_e32"):
            d, r1 = self._vreg(args[0]), self._vreg(args[2])
            if args[1][0] == "v":
                r0 = self._vreg(args[1])
                a = lambda: V[self._src0_row(r0)]
            else:
                s = self._src(args[1])
                a = lambda: np.uint32(s())
            if op == "v_xor_b32_e32":
                def vxor():
                    V[self._dst_row(d)] = a() ^ V[r1]
                return vxor

            def vadd():
                V[self._dst_row(d)] = ((a().astype(np.uint64) + V[r1]) & np.uint64(M32)).astype(np.uint32)
            return vadd
        if op == "global_load_dword":
            d, off = self._vreg(args[0]), self._vreg(args[1])
            pair, _, imm = args[2].partition(" offset:")
            base, imm = self._src(pair, True), int(imm or 0)

            def gload():
                assert not self.idx_on
                byte = base() + imm - TABLE_ADDR + V[off].astype(np.int64)
                assert (byte % 4 == 0).all() and byte.min() >= 0 and byte.max() < 4 * self.table.size, f"pc {pc}: load outside the tables"
                V[d] = self.table[byte // 4]
            return gload
        if op == "ds_read_b32":
            d = self._vreg(args[0])
            a, _, imm = args[1].partition(" offset:")
            a, imm = self._vreg(a), int(imm or 0)

            def dsread():
                at = V[a].astype(np.int64) + imm
                assert at.min() >= WIN_BASE and at.max() + 4 <= WIN_BASE + WIN_BYTES, f"pc {pc}: LDS read outside the window"
                b = self.lds
                V[d] = b[at].astype(np.uint32) | (b[at + 1].astype(np.uint32) << 8) | (b[at + 2].astype(np.uint32) << 16) | (b[at + 3].astype(np.uint32) << 24)
            return dsread
        if op == "ds_write_b16":
            a, d = self._vreg(args[0]), self._vreg(args[1])

            def dswrite():
                assert not self.idx_on
                at = V[a].astype(np.int64)
                assert at.min() >= REC_BASE and at.max() + 2 <= REC_BASE + 2 * TILE, f"pc {pc}: LDS write outside the record"
                self.lds[at] = V[d] & 0xFF
                self.lds[at + 1] = (V[d] >> 8) & 0xFF
            return dswrite
        raise NotImplementedError(f"the tile uses an instruction the model does not know: {line}")

    def run(self, limit=4_000_000):
        pc, code, watch = 0, self.code, self.watch
        while pc < len(code):
            if pc in watch:
                watch[pc](self)
            to = code[pc]()
            self.executed += 1
            assert self.executed < limit, "the program does not end"
            pc = pc + 1 if to is None else to


# ---- tables and streams -------------------------------------------------------------------------------------------

def _slots(cum, freq, c2s):
    """The decoder's slot tables F' then B' (rans.hip: build_dec_slots)."""
    slot = np.arange(4096, dtype=np.int64)
    f, c = np.asarray(freq, np.int64)[c2s], np.asarray(cum, np.int64)[c2s]
    return np.concatenate([(f << 20) & M32, (slot - c - ((f * slot) >> 12)) & M32]).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def _case(kind):
    """Stream, tables and the oracle's trace of 2 tiles, computed once per table kind."""
    cum, freq, _ = R.table(kind)
    # spare stream behind the decoded part: the tile reads ahead
    sym, data = R.stream(kind, 2 * TILE + (40000 if kind == "peaked" else 600))
    c2s = R.cum_to_sym(cum, freq)
    states, marks = R.trace(data, 2 * TILE, cum, freq, c2s)
    ref = onp.rans_decode(data, 2 * TILE, cum, freq, [int(v) for v in c2s])
    assert np.array_equal(c2s[states & 4095], ref) and np.array_equal(ref, sym[: 2 * TILE])
    assert marks[2 * TILE][1] + 8 <= len(data)
    return data, c2s, _slots(cum, freq, c2s), states, marks, cum, freq


def _pair_starts(m):
    """The pair's copy of the window's upper dword is where the tile relies on 32 <= V."""
    at = [pc for pc, line in enumerate(m.text) if line == "s_mov_b32 s60, s63"]
    assert len(at) == 32
    return at


def _run_tiles(program, kind, entry, seen_v):
    data, c2s, slots, states, marks, _, _ = _case(kind)
    m = Machine(program)
    m.table = slots
    lanes = np.arange(64, dtype=np.uint32)
    wbase = [0]

    def check_window(mm):
        w = mm.S[62] | (mm.S[63] << 32)
        assert w, "the window lost its sentinel"
        v = 63 - ((w & -w).bit_length() - 1)
        seen_v.append(v)
        assert 32 <= v <= 63 and v % 8 == 0, f"{v} valid window bits at a pair start"
        at = wbase[0] + 4 * mm.S[73] - v // 8            # the decoder's position
        assert w >> (64 - v) == int.from_bytes(data[at: at + v // 8], "big"), "the window is not the stream at the decoder's position"

    for pc in _pair_starts(m):
        m.watch[pc] = check_window
    x, pos = marks[0]
    for t in range(2):
        assert (x, pos) == marks[t * TILE]
        wbase[0] = pos - (entry + t) % 4                  # the window base is wherever the stream's dword alignment puts it
        win = np.zeros(WIN_BYTES, np.uint8)
        part = np.frombuffer(data[wbase[0]: wbase[0] + WIN_BYTES], np.uint8)
        win[: part.size] = part
        m.lds[WIN_BASE: WIN_BASE + WIN_BYTES] = win
        m.lds[REC_BASE:] = 0xEE
        m.V[0], m.V[1], m.V[2] = 4 * lanes, WIN_BASE + 4 * lanes, REC_BASE + 2 * lanes
        m.S[10], m.S[11], m.S[12] = x, pos - wbase[0], TILE // 64
        m.S[14], m.S[15] = TABLE_ADDR & M32, TABLE_ADDR >> 32
        m.S[M0] = 0x1234ABCD
        m.run()
        assert m.S[M0] == 0x1234ABCD and not m.idx_on     # the surrounding code's M0, index mode off
        assert np.array_equal(m.V[2], REC_BASE + 2 * TILE + 2 * lanes)
        rec = m.lds[REC_BASE::2].astype(np.int64) | (m.lds[REC_BASE + 1:: 2].astype(np.int64) << 8)
        want = states[t * TILE: (t + 1) * TILE]
        assert np.array_equal(rec, want & 0xFFFF), (kind, entry, t, int(np.argmax(rec != (want & 0xFFFF))))
        assert np.array_equal(c2s[rec & 4095], c2s[want & 4095])
        x, pos = m.S[16], wbase[0] + m.S[17]
        assert (x, pos) == marks[(t + 1) * TILE], (kind, entry, t)


@pytest.mark.parametrize("entry", range(4))
@pytest.mark.parametrize("kind", KINDS)
def test_fast_tile_decodes_like_the_oracle(gen, kind, entry):
    seen_v = []
    _run_tiles(gen.fast_tile(), kind, entry, seen_v)
    assert len(seen_v) == 2 * TILE // 2
    if kind == "flat":
        assert min(seen_v) == 32           # drained to the refill threshold again and again
    if kind == "peaked":
        assert max(seen_v) == 56           # the ceiling: a refill at V = 24
    if kind == "sparse":
        assert min(seen_v) == 32 and max(seen_v) == 56


def test_both_loop_phases_decode(gen):
    _run_tiles(gen.fast_tile(0), "random", 1, [])
    _run_tiles(gen.fast_tile(4), "random", 2, [])


def test_sparse_table_consumes_24_bits_in_a_pair():
    """The most a pair can consume: a 16-bit and an 8-bit shift; from V = 32 that leaves V = 8 after the pair."""
    data, c2s, slots, states, marks, cum, freq = _case("sparse")
    shifts = []
    for x in (int(v) for v in states):
        slot = x & 4095
        s = int(c2s[slot])
        u = freq[s] * (x >> 12) + slot - cum[s]
        shifts.append(0 if u >= 1 << 23 else (8 if u >= 1 << 15 else 16))
    assert max(a + b for a, b in zip(shifts[0::2], shifts[1::2])) == 24 and shifts.count(16) > 100


def test_dry_tile_only_evolves_the_state(gen):
    data, c2s, slots, states, marks, cum, freq = _case("random")
    m = Machine(gen.dry_tile())
    m.table = slots
    lanes = np.arange(64, dtype=np.uint32)
    m.V[0], m.V[2] = 4 * lanes, REC_BASE + 2 * lanes
    x = 0x00ABCDEF
    m.S[10], m.S[12] = x, 3
    m.S[14], m.S[15] = TABLE_ADDR & M32, TABLE_ADDR >> 32
    m.S[M0] = 77
    m.run()
    want = []
    for _ in range(3 * 64):
        want.append(x & 0xFFFF)
        slot = x & 4095
        s = int(c2s[slot])
        x = (freq[s] * (x >> 12) + slot - cum[s]) & M32
    rec = m.lds[REC_BASE::2].astype(np.int64) | (m.lds[REC_BASE + 1:: 2].astype(np.int64) << 8)
    assert np.array_equal(rec[: 3 * 64], want) and m.S[16] == x and m.S[M0] == 77


@pytest.mark.parametrize("v", [0, 8, 16, 24])
def test_refill_sequence_alone(gen, v):
    """The refill on a window of V valid bits, V = 0 (only the sentinel left) included."""
    rng = np.random.default_rng(v)
    for _ in range(20):
        bits = int(rng.integers(0, 1 << 62)) >> (62 - v) if v else 0
        new = int(rng.integers(0, 1 << 32))
        m = Machine(gen.refill())
        m.S[62], m.S[63] = 0, ((bits << 1 | 1) << (31 - v)) & M32
        m.S[64], m.S[73] = 0x80000000, 64 * 5 + 9
        m.V[192 + 5, 9] = new ^ 0x80000000
        m.run()
        w = m.S[62] | (m.S[63] << 32)
        assert w == ((bits << 32 | new) << 1 | 1) << (31 - v), (v, hex(bits), hex(new), hex(w))
        assert m.S[73] == 64 * 5 + 10 and m.S[64] == 0x80000000


def test_mis_edits_are_caught(gen):
    """The checks above see a wrong refill and a wrong pair tail: each single-line mis-edit fails the model run."""
    good = gen.fast_tile()
    edits = [("s_sub_u32 s78, 31, s78", "s_sub_u32 s78, 32, s78"),                                # refill: shift off by one
             ("s_xor_b64 s[62:63], s[62:63], s[66:67]", "s_or_b64 s[62:63], s[62:63], s[66:67]"),    # refill: the sentinel stays
             ("s_cmp_eq_u32 s62, 0", "s_cmp_eq_u32 s63, 0"),                                        # tail: wrong dword tested
             ("s_lshl_b64 s[62:63], s[62:63], s77", "s_lshl_b64 s[62:63], s[62:63], s71")]          # tail: wrong shift
    for old, new in edits:
        assert old in good
        bad = [new if line == old else line for line in good]
        with pytest.raises(AssertionError):
            _run_tiles(bad, "random", 1, [])   # not the flat table: there every shift is 8 and the two tail shifts agree


def test_generated_file_is_current(gen):
    inc = os.path.join(ROOT, "alice-codec_amd", "csrc", "rans_decode_tile.inc")
    with open(inc) as f:
        assert f.read() == gen.render(), "rans_decode_tile.inc is not what gen_rans_decode_asm.py writes: regenerate it"
    assert gen.render() == gen.render()
    assert "s72" not in gen.fast_clobbers()
