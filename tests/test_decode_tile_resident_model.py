"""The resident decode tile (gen_rans_decode_asm.py: resident_tile(), rans_decode_tile_rs.inc) run on the model of the machine.

One statement decodes a run of full tiles: the tables are loaded once, every tile's 33 window rows come straight from the
stream in global memory, the symbols of a tile are recovered from the record through cum_to_sym and stored while the next
tile's window loads are in flight (the last tile's on leaving), and at the end of every tile the scalar side decides, by the
conditions rans_decode_kernel has for its fast `whole` path, whether the statement goes on.

The machine is test_decode_tile_inhand_model's and learns: a flat byte memory with the tables, the stream and the output in
it (a load outside the tables and [in, in + len) is an error, and so is a store outside the 4096 output bytes of the tile
being recovered: the k-th group of sixteen stores belongs to tile k), ds_read_b64 (inside the record), ds_read_u8 (inside
cum_to_sym), the vector instructions of the recovery, s_cmp_ge_u32 and s_cmp_lt_u32.  At every pair start it asserts the
in-hand tile's invariant against the stream itself: s65 is the flipped dword with index s73 of the window that starts at s44.
The runner binds the operands the way the kernel computes them (window base, position, clamped length), and its mirror of
the kernel's conditions says how many tiles the statement has to take."""
import functools
import os
import re
import sys

import numpy as np
import pytest

from oracle import alice_oracle_np as onp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_tile_ref as R  # noqa: E402
import test_decode_tile_inhand_model as TI  # noqa: E402
import test_decode_tile_model as T  # noqa: E402
import test_decode_tile_vec_model as TV  # noqa: E402
from decode_tile_ref import M32, TILE  # noqa: E402

ROOT = T.ROOT
FULL = TI.FULL
WIN = T.WIN_BYTES
IN_ADDR = 0x00007F2400001000      # dword aligned; the tests add 0 .. 3
OUT_ADDR = 0x00007F2500000040
GUARD = 64
OPERANDS = {"%[ip]": "s[18:19]", "%[ln]": "s20", "%[nt]": "s21", "%[op]": "s[22:23]", "%[cs]": "s24", "%[to]": "s25"}
C2S_BASE = 0                      # cum_to_sym sits in front of the window in LDS, as in the kernel


class ResidentMachine(TI.InhandMachine):
    def __init__(self, program):
        bound = []
        for line in program:
            for k, v in OPERANDS.items():
                line = line.replace(k, v)
            bound.append(line)
        self.in_addr, self.stream, self.out = IN_ADDR, b"", np.zeros(0, np.uint8)
        self.rel0 = 0                   # the statement's stream pointer is in + rel0
        self.stores = 0
        self.window_loads = 0
        super().__init__(bound)
        for pc, line in enumerate(self.text):
            if line == TI.PAIR_START:
                self.watch[pc] = ResidentMachine._pair_start

    def _pair_start(self):
        self.pair_no += 1
        at = self.rel0 + self.S[44] + 4 * self.S[73]    # s44 counts from the statement's stream pointer
        assert at + 4 <= len(self.stream), "s73 left the stream"
        assert self.S[65] == int.from_bytes(self.stream[at: at + 4], "big") ^ 0x80000000, \
            f"pair {self.pair_no}: s65 is not the dword with index s73 = {self.S[73]} of the window at {self.S[44]}"
        TI.InhandMachine.in_hand_checks += 1

    def _translate(self, pc, line):
        op, _, rest = line.partition(" ")
        args = [a.strip() for a in rest.split(",")] if rest else []
        S, V = self.S, self.V

        def vector(run):
            def full_exec():
                assert self.exec == FULL, f"pc {pc}: {op} with EXEC = {self.exec:#x}"
                assert not self.idx_on, f"pc {pc}: {op} in VGPR-index mode"
                return run()
            return full_exec

        def vsrc(a):
            if a[0] == "v":
                n = self._vreg(a)
                return lambda: V[n].astype(np.int64)
            s = self._src(a)
            return lambda: np.int64(s())

        if op in ("s_cmp_ge_u32", "s_cmp_lt_u32"):
            a, b = self._src(args[0]), self._src(args[1])
            ge = op == "s_cmp_ge_u32"

            def cmp():
                self.scc = int((a() >= b()) == ge)
            return cmp
        if op == "global_load_dword" and args[2].startswith("s[40:41]"):
            d, off = self._vreg(args[0]), self._vreg(args[1])
            imm = int(args[2].partition(" offset:")[2] or 0)
            base = self._src("s[40:41]", True)

            def wload():
                byte = base() + imm - self.in_addr + V[off].astype(np.int64)
                assert ((base() + imm + V[off].astype(np.int64)) % 4 == 0).all(), f"pc {pc}: unaligned window load"
                assert byte.min() >= 0 and byte.max() + 4 <= len(self.stream), f"pc {pc}: window load outside the stream"
                raw = np.frombuffer(self.stream, np.uint8).astype(np.uint32)
                V[d] = raw[byte] | (raw[byte + 1] << 8) | (raw[byte + 2] << 16) | (raw[byte + 3] << 24)
                self.window_loads += 1
            return vector(wload)
        if op == "global_store_dword":
            off, src = self._vreg(args[0]), self._vreg(args[1])
            pair, _, imm = args[2].partition(" offset:")
            base, imm = self._src(pair, True), int(imm or 0)

            def store():
                tile = self.stores // 16
                byte = base() + imm - OUT_ADDR + V[off].astype(np.int64)
                assert byte.min() >= tile * TILE and byte.max() + 4 <= (tile + 1) * TILE, f"pc {pc}: store outside tile {tile}'s output"
                assert (byte % 4 == 0).all()
                for k in range(4):
                    self.out[GUARD + byte + k] = (V[src] >> np.uint32(8 * k)) & 0xFF
                self.stores += 1
            return vector(store)
        if op in ("ds_read_b64", "ds_read_u8"):
            a, _, imm = args[1].partition(" offset:")
            a, imm = self._vreg(a), int(imm or 0)
            if op == "ds_read_b64":
                lo, hi = args[0][2:-1].split(":")
                lo = int(lo)
                assert args[0].startswith("v[") and int(hi) == lo + 1

                def read64():
                    at = V[a].astype(np.int64) + imm
                    assert at.min() >= T.REC_BASE and at.max() + 8 <= T.REC_BASE + 2 * TILE and (at % 8 == 0).all(), f"pc {pc}: LDS read outside the record"
                    b = self.lds.astype(np.uint32)
                    V[lo] = b[at] | (b[at + 1] << 8) | (b[at + 2] << 16) | (b[at + 3] << 24)
                    V[lo + 1] = b[at + 4] | (b[at + 5] << 8) | (b[at + 6] << 16) | (b[at + 7] << 24)
                return vector(read64)
            d = self._vreg(args[0])

            def read8():
                at = V[a].astype(np.int64) + imm
                assert at.min() >= C2S_BASE and at.max() < C2S_BASE + 4096, f"pc {pc}: LDS read outside cum_to_sym"
                V[d] = self.lds[at].astype(np.uint32)
            return vector(read8)
        if op == "v_and_b32_e32":
            d, a, b = self._vreg(args[0]), vsrc(args[1]), vsrc(args[2])
            return vector(lambda: V.__setitem__(d, (a() & b()).astype(np.uint32)))
        if op == "v_lshrrev_b32_e32":
            d, a, b = self._vreg(args[0]), vsrc(args[1]), vsrc(args[2])
            return vector(lambda: V.__setitem__(d, (b() >> (a() & 31)).astype(np.uint32)))
        if op == "v_bfe_u32":
            d, a, o, w = self._vreg(args[0]), vsrc(args[1]), int(args[2]), int(args[3])
            return vector(lambda: V.__setitem__(d, ((a() >> o) & ((1 << w) - 1)).astype(np.uint32)))
        if op == "v_lshl_or_b32":
            d, a, sh, c = self._vreg(args[0]), vsrc(args[1]), int(args[2]), vsrc(args[3])
            return vector(lambda: V.__setitem__(d, (((a() << sh) & M32) | c()).astype(np.uint32)))
        return super()._translate(pc, line)


# ---- streams ---------------------------------------------------------------------------------------------------------

def _build(cum, freq, sym, tiles):
    data = onp.rans_encode(sym, cum, freq)
    c2s = R.cum_to_sym(cum, freq)
    states, marks = R.trace(data, tiles * TILE, cum, freq, c2s)
    assert np.array_equal(c2s[states & 4095], sym[: tiles * TILE])
    return bytes(data), c2s, T._slots(cum, freq, c2s), marks, np.asarray(sym[: tiles * TILE], np.uint8)


@functools.lru_cache(maxsize=None)
def _case(kind):
    if kind == "ones":       # every symbol has frequency 1: 12 bits per symbol, the window base moves 6 KB per tile
        freq = [1] * 200 + [0] * 55 + [4096 - 200]
        cum = [int(v) for v in np.concatenate([[0], np.cumsum(freq)[:-1]])]
        sym = np.random.default_rng(12).integers(0, 200, 3 * TILE + 6000).astype(np.uint8)
        return _build(cum, freq, sym, 3)
    if kind == "two":        # two symbols, one of them rare: a few dozen bytes per tile, so every pos & 3 turns up at a tile start
        freq = [4064, 32] + [0] * 254
        cum = [0, 4064] + [4096] * 254
        rng = np.random.default_rng(5)
        sym = (rng.random(8 * TILE + 400 * TILE) < 32 / 4096).astype(np.uint8)
        return _build(cum, freq, sym, 8)
    if kind == "big":        # a symbol of frequency 4096: the state never moves and nothing is consumed (two tiles)
        data, c2s, slots, states, marks, _, _ = TV._big_case()
        return bytes(data), c2s, slots, marks, np.full(2 * TILE, 5, np.uint8)
    cum, freq, _ = R.table(kind)
    sym, data = R.stream(kind, 3 * TILE + (400 * TILE if kind == "peaked" else 3 * WIN))
    c2s = R.cum_to_sym(cum, freq)
    states, marks = R.trace(data, 3 * TILE, cum, freq, c2s)
    return bytes(data), c2s, T._slots(cum, freq, c2s), marks, sym[: 3 * TILE]


def _kernel_window(in_addr, pos, length):
    """rans_decode_kernel's choice of the window base, and whether the window is whole."""
    mis = (in_addr + pos) & 3
    wbase = pos - mis if pos >= mis else pos & ~3
    return wbase, length - wbase >= WIN and (in_addr + wbase) & 3 == 0


def _expected_tiles(in_addr, marks, length, max_tiles):
    """How many tiles the kernel's conditions let one statement take, from the oracle's positions."""
    k = 0
    while True:
        k += 1
        x, pos = marks[k * TILE]
        if k == max_tiles or not pos < length or x < 1 << 23 or not _kernel_window(in_addr, pos, length)[1]:
            return k


def _run(program, kind, max_tiles, off=0, length=None, first=0):
    """One statement from tile `first` of the case on; returns (tiles taken, pos & 3 at every tile start, machine)."""
    data, c2s, slots, marks, sym = _case(kind)
    length = len(data) if length is None else length
    in_addr = IN_ADDR + off
    x, pos = marks[first * TILE]
    wbase, whole = _kernel_window(in_addr, pos, length)
    assert whole and pos < length and x >= 1 << 23, "the kernel would not enter the statement here"
    m = ResidentMachine(program)
    m.table, m.in_addr, m.stream, m.rel0 = slots, in_addr, data[:length], wbase
    m.out = np.full(2 * GUARD + max_tiles * TILE, 0xEE, np.uint8)
    lanes = np.arange(64, dtype=np.uint32)
    m.lds[C2S_BASE: C2S_BASE + 4096] = c2s
    m.lds[T.REC_BASE:] = 0xEE
    m.V[0], m.V[2] = 4 * lanes, T.REC_BASE + 2 * lanes
    S = m.S
    S[10], S[11] = x, pos - wbase
    S[14], S[15] = T.TABLE_ADDR & M32, T.TABLE_ADDR >> 32
    S[18], S[19] = (in_addr + wbase) & M32, (in_addr + wbase) >> 32
    S[20], S[21] = min(length - wbase, M32), max_tiles
    S[22], S[23] = OUT_ADDR & M32, OUT_ADDR >> 32
    S[24] = C2S_BASE
    S[T.M0] = 0x1234ABCD
    starts = []
    top = m.text.index("s_and_b32 s44, s48, 0xfffffffc")
    m.watch[top] = lambda mm: starts.append(mm.S[48] & 3)
    m.run(limit=40_000_000)
    assert S[T.M0] == 0x1234ABCD and not m.idx_on
    took = S[25]
    want = _expected_tiles(in_addr, {k - first * TILE: v for k, v in marks.items() if k >= first * TILE}, length, max_tiles)
    assert took == want, f"{kind}: the statement took {took} tiles, the kernel's conditions say {want}"
    assert (S[16], wbase + S[17]) == marks[(first + took) * TILE], (kind, off, took)
    assert m.stores == 16 * took and m.window_loads == 33 * took
    out = m.out[GUARD: GUARD + took * TILE]
    assert np.array_equal(out, sym[first * TILE: (first + took) * TILE]), (kind, int(np.argmax(out != sym[first * TILE: (first + took) * TILE])))
    assert (m.out[:GUARD] == 0xEE).all() and (m.out[GUARD + took * TILE:] == 0xEE).all()
    assert m.pair_no == took * TILE // 2
    return took, starts, m


@pytest.fixture(scope="module")
def gen():
    return T._generator()


@pytest.fixture(autouse=True)
def _reset():
    TI.TS.ShadowMachine.taken = []
    TI.InhandMachine.refill_pairs = []
    TI.InhandMachine.in_hand_checks = 0


@pytest.mark.parametrize("kind", ["random", "flat", "sparse"])
def test_three_tiles_in_one_statement(gen, kind):
    took, _, _ = _run(gen.resident_tile(), kind, 3)
    assert took == 3                                          # left by the symbol count: the stream goes on
    assert TI.InhandMachine.in_hand_checks == 3 * TILE // 2


def test_leaves_after_the_tile_count_it_was_given(gen):
    assert _run(gen.resident_tile(), "random", 2)[0] == 2
    assert _run(gen.resident_tile(), "random", 1)[0] == 1
    assert _run(gen.resident_tile(), "random", 2, first=1)[0] == 2


def test_next_window_must_be_whole(gen):
    """The stream ends exactly kDecWinBytes behind the second tile's window base: the statement stays; one byte less: it
    leaves after the first tile, and the exact loop's territory begins."""
    data, _, _, marks, _ = _case("flat")
    wbase = _kernel_window(IN_ADDR, marks[TILE][1], len(data))[0]
    assert _run(gen.resident_tile(), "flat", 2, length=wbase + WIN)[0] == 2
    assert _run(gen.resident_tile(), "flat", 2, length=wbase + WIN - 1)[0] == 1
    assert _run(gen.resident_tile(), "flat", 3, length=wbase + WIN)[0] == 2   # ... and the third tile's window is not


def test_every_position_in_a_dword_at_a_tile_start(gen):
    took, starts, _ = _run(gen.resident_tile(), "two", 8)
    assert took == 8 and set(starts) == {0, 1, 2, 3}, starts
    data, _, _, marks, _ = _case("two")
    assert marks[8 * TILE][1] < 1200                          # the window base moves a few dozen bytes per tile


def test_frequency_one_table(gen):
    took, _, m = _run(gen.resident_tile(), "ones", 3)
    data, _, _, marks, _ = _case("ones")
    assert took == 3 and marks[TILE][1] - marks[0][1] == TILE * 3 // 2   # 12 bits per symbol: 6 KB per tile
    runs = TI._runs(TI.InhandMachine.refill_pairs)
    assert max(runs) == 3


def test_frequency_4096_table(gen):
    took, starts, _ = _run(gen.resident_tile(), "big", 2)
    assert took == 2 and starts == [0, 0]                     # nothing is consumed: the same window twice


@pytest.mark.parametrize("off", [1, 2, 3])
def test_stream_base_off_a_dword(gen, off):
    took, starts, _ = _run(gen.resident_tile(), "random", 3, off=off)
    assert took == 3 and starts[0] == off                     # pos = 4: the window base is the aligned dword in front of it


def test_both_loop_phases_decode(gen):
    _run(gen.resident_tile(0), "random", 2, off=1)
    _run(gen.resident_tile(4), "random", 2, off=2)
    assert gen.resident_tile(0) != gen.resident_tile(4)


def test_tile_shape(gen):
    """The block loop is the in-hand tile's, instruction for instruction; the tables are loaded once, in front of the tile
    loop; no load or store other than the tables, the window rows and the symbols; the earlier tiles are what they were."""
    rs, ih = gen.resident_tile(), gen.inhand_tile()
    body = lambda L: [s.replace("v228", "%[ra]") for s in L[L.index("2:"): L.index("5:")]]
    assert body(rs) == body(ih)
    top = rs.index("7:")
    assert sum(s.startswith("global_load_dword v") and "s[64:65]" in s for s in rs[:top]) == 128
    assert not [s for s in rs[top:] if "s[64:65]" in s and s.startswith("global_")]
    assert sum(s.startswith("global_load_dword") for s in rs[top:]) == 33
    assert sum(s.startswith("global_store_dword") for s in rs) == 32   # sixteen per recovery: in the tile loop and on leaving
    assert not [s for s in rs if s.startswith("ds_read_b32")]  # the window does not pass through LDS
    assert set(gen.inhand_clobbers()) < set(gen.resident_clobbers()) and "s72" not in gen.resident_clobbers()
    used = {int(r) for s in rs for r in re.findall(r"\bv(\d+)\b", s)}
    assert max(used) <= 255 and {f"v{r}" for r in used if r >= 64} <= set(gen.resident_clobbers())


def _replace_nth(good, old, new, n=0):
    at = [i for i, s in enumerate(good) if s == old][n]
    return good[:at] + [new] + good[at + 1:]


def test_mis_edits_are_caught(gen):
    good = gen.resident_tile()
    data, _, _, marks, _ = _case("flat")
    exact = _kernel_window(IN_ADDR, marks[TILE][1], len(data))[0] + WIN
    three = lambda prog: _run(prog, "random", 3, off=1)
    edge = lambda prog: _run(prog, "flat", 2, length=exact)
    far = lambda prog: _run(prog, "ones", 2)                  # 6 KB per tile: the rows behind the sixteenth are read
    edits = {
        "a recovery trip dropped": (three, _replace_nth(good, "global_store_dword %[l4], v242, s[42:43] offset:512", "s_nop 0")),
        "a recovery trip dropped on leaving": (three, _replace_nth(good, "global_store_dword %[l4], v243, s[42:43] offset:3840", "s_nop 0", 1)),
        "the whole compare off by one": (edge, _replace_nth(good, "s_cmp_lt_u32 s70, 8448", "s_cmp_lt_u32 s70, 8449")),
        "the window load's row stride": (three, _replace_nth(good, "global_load_dword v193, %[l4], s[40:41] offset:256", "global_load_dword v193, %[l4], s[40:41] offset:512")),
        "the window base not moved after sixteen rows": (far, _replace_nth(good, "s_add_u32 s40, s40, 0x1000", "s_add_u32 s40, s40, 0x800")),
        "the second symbol's slot cut short": (three, _replace_nth(good, "v_bfe_u32 v235, v230, 16, 12", "v_bfe_u32 v235, v230, 16, 8")),
        "the output advanced by half a tile": (three, _replace_nth(good, "s_add_u32 s42, s42, 0x1000", "s_add_u32 s42, s42, 0x800")),
        "recovery in front of the first tile": (three, _replace_nth(good, "s_cmp_eq_u32 s46, 0", "s_cmp_eq_u32 s46, 1")),
        "the position inside the window negated": (three, _replace_nth(good, "s_sub_u32 s70, s48, s44", "s_sub_u32 s70, s44, s48")),
        "the record address not rewound": (three, _replace_nth(good, "v_mov_b32_e32 v228, %[ra]", "s_nop 0")),
        "two tiles counted for one": (three, _replace_nth(good, "s_add_u32 s46, s46, 1", "s_add_u32 s46, s46, 2")),
    }
    for name, (run, bad) in edits.items():
        assert bad != good and len(bad) == len(good), name
        with pytest.raises(AssertionError):
            run(bad)
            print("not caught:", name)
    three(good)
    edge(good)
    far(good)


def test_generated_files_are_current(gen):
    csrc = os.path.join(ROOT, "alice-codec_amd", "csrc")
    with open(os.path.join(csrc, "rans_decode_tile_rs.inc")) as f:
        assert f.read() == gen.render_resident(), "rans_decode_tile_rs.inc is not what gen_rans_decode_asm.py writes: regenerate it"
    assert gen.render_resident() == gen.render_resident()
