"""The in-hand decode tile (gen_rans_decode_asm.py: inhand_tile(), rans_decode_tile_ih.inc) run on the model of the machine.

The tile is the shadow tile with another refill: s65 always holds the window dword with index s73 (top bit flipped), the
refill is five SALU instructions on it, and the out-of-line path carries on through the rest of the pair -- the even symbol's
tail, the odd symbol's head, its lane read, the read of the next s65 from the staging row v227 in the same stall, the record
-- before it branches back to the odd symbol's s_flbit.  v227 holds the 64 window dwords from s73 on and is rebuilt at the
tile entry and at every block end, through EXEC.

The machine is test_decode_tile_shadow_model's and learns what the staging uses: EXEC as the operand of s_mov_b64 and
s_bfm_b64, and v_mov_b32 under EXEC with a relative src0.  Every other vector or memory instruction must find EXEC full.
The runner, the oracle traces and the window check are test_decode_tile_model's; the window check stands at the pair's copy,
which exists twice per pair here (main line and out-of-line path) and runs once.  At every pair start (the even symbol's
first instruction) the machine itself asserts the tile's new invariant: s65 is the flipped dword at index s73 of the window
in LDS.  It numbers the pairs and notes the pair of every refill it takes, which is how the tests find consecutive refills."""
import os
import sys

import numpy as np
import pytest

from oracle import alice_oracle_np as onp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_tile_ref as R  # noqa: E402
import test_decode_tile_model as T  # noqa: E402
import test_decode_tile_shadow_model as TS  # noqa: E402
import test_decode_tile_vec_model as TV  # noqa: E402
from decode_tile_ref import KINDS, M32, TILE  # noqa: E402

ROOT = T.ROOT
COPY = TS.COPY
PAIR_START = "s_bfe_u32 s76, s61, 0x60006"
FULL = (1 << 64) - 1


class InhandMachine(TS.ShadowMachine):
    refill_pairs = []   # the running pair number of every refill taken; reset by the fixture
    in_hand_checks = 0

    def __init__(self, program):
        self.exec = FULL
        self.pair_no = 0
        super().__init__(program)
        starts = [pc for pc, line in enumerate(self.text) if line == PAIR_START]
        assert len(starts) == 32
        for pc in starts:
            self.watch[pc] = InhandMachine._pair_start

    def _pair_start(self):
        self.pair_no += 1
        at = T.WIN_BASE + 4 * self.S[73]
        assert at + 4 <= T.WIN_BASE + T.WIN_BYTES, "s73 left the window"
        assert self.S[65] == int.from_bytes(bytes(self.lds[at: at + 4]), "big") ^ 0x80000000, \
            f"pair {self.pair_no}: s65 is not the dword with index s73 = {self.S[73]}"
        InhandMachine.in_hand_checks += 1

    def _translate(self, pc, line):
        op, _, rest = line.partition(" ")
        args = [a.strip() for a in rest.split(",")] if rest else []
        S, V = self.S, self.V
        if op == "s_mov_b64" and args[1] == "exec":
            put = self._dst(pc, args[0], True)
            return lambda: put(self.exec)
        if op == "s_mov_b64" and args[0] == "exec":
            a = self._src(args[1], True)

            def set_exec():
                self.exec = a()
            return set_exec
        if op == "s_bfm_b64":
            assert args[0] == "exec", line
            width, shift = self._src(args[1]), self._src(args[2])

            def bfm():
                self.exec = (((1 << (width() & 63)) - 1) << (shift() & 63)) & FULL
            return bfm
        if op == "v_mov_b32_e32":
            d, r0 = self._vreg(args[0]), self._vreg(args[1])

            def vmov():
                on = np.array([(self.exec >> l) & 1 for l in range(64)], bool)
                V[self._dst_row(d)][on] = V[self._src0_row(r0)][on]
            return vmov
        run = super()._translate(pc, line)
        if op.startswith(("v_", "ds_", "global_")):
            def full_exec():
                assert self.exec == FULL, f"pc {pc}: {op} with EXEC = {self.exec:#x}"
                return run()
            return full_exec
        if line.startswith("s_cbranch_scc1 3"):
            def branch():
                to = run()
                if to is not None:
                    InhandMachine.refill_pairs.append(self.pair_no)
                return to
            return branch
        return run

    def run(self, limit=4_000_000):
        super().run(limit)
        assert self.exec == FULL, "EXEC was not restored"


def _copies(m):
    at = [pc for pc, line in enumerate(m.text) if line == COPY]
    assert len(at) == 64                                      # main line and out-of-line path: one of the two runs per pair
    return at


@pytest.fixture(scope="module")
def gen():
    return T._generator()


@pytest.fixture()
def runner(monkeypatch):
    monkeypatch.setattr(T, "Machine", InhandMachine)
    monkeypatch.setattr(T, "_pair_starts", _copies)
    TS.ShadowMachine.taken = []
    InhandMachine.refill_pairs = []
    InhandMachine.in_hand_checks = 0
    return T._run_tiles


def _runs(pairs):
    """Lengths of the runs of consecutive pair numbers."""
    out, n = [], 0
    for i, p in enumerate(pairs):
        n = n + 1 if i and p == pairs[i - 1] + 1 else 1
        if i + 1 == len(pairs) or pairs[i + 1] != p + 1:
            out.append(n)
    return out


def _ones_case():
    """Every symbol of the stream has frequency 1: x' = x >> 12, a 16-bit and an 8-bit shift in every pair, 12 bits per
    symbol, so three pairs in a row refill and the fourth does not."""
    freq = [1] * 200 + [0] * 55 + [4096 - 200]
    cum = [int(v) for v in np.concatenate([[0], np.cumsum(freq)[:-1]])]
    sym = np.random.default_rng(12).integers(0, 200, 2 * TILE + 600).astype(np.uint8)
    data = onp.rans_encode(sym, cum, freq)
    c2s = R.cum_to_sym(cum, freq)
    states, marks = R.trace(data, 2 * TILE, cum, freq, c2s)
    assert np.array_equal(c2s[states & 4095], sym[: 2 * TILE]) and marks[2 * TILE][1] + 8 <= len(data)
    return data, c2s, T._slots(cum, freq, c2s), states, marks, cum, freq


@pytest.mark.parametrize("entry", range(4))
@pytest.mark.parametrize("kind", KINDS)
def test_inhand_tile_decodes_like_the_oracle(gen, runner, kind, entry):
    seen_v = []
    runner(gen.inhand_tile(), kind, entry, seen_v)
    assert len(seen_v) == 2 * TILE // 2 and InhandMachine.in_hand_checks == 2 * TILE // 2
    if kind == "flat":
        assert min(seen_v) == 32
    if kind == "peaked":
        assert max(seen_v) == 56
    if kind == "sparse":
        assert min(seen_v) == 32 and max(seen_v) == 56
    assert TS.ShadowMachine.taken and all(v <= 24 and v % 8 == 0 for _, _, _, v in TS.ShadowMachine.taken)


def test_both_loop_phases_decode(gen, runner):
    runner(gen.inhand_tile(0), "random", 1, [])
    runner(gen.inhand_tile(4), "random", 2, [])
    assert gen.inhand_tile(0) != gen.inhand_tile(4)


def test_sixteen_bit_shifts_on_even_and_odd_symbols(gen, runner):
    sh = TS._shifts("sparse")
    assert sh[0::2].count(16) > 20 and sh[1::2].count(16) > 20
    assert any(sh[i] == 16 for i in range(63, 2 * TILE, 64))
    runner(gen.inhand_tile(), "sparse", 0, [])
    assert any(p == 16 for _, _, p, _ in TS.ShadowMachine.taken)
    assert 2 in _runs(InhandMachine.refill_pairs)             # ... and refills in two consecutive pairs


def test_refills_in_three_consecutive_pairs(gen, runner, monkeypatch):
    case = _ones_case()
    monkeypatch.setattr(T, "_case", lambda kind: case)
    seen_v = []
    runner(gen.inhand_tile(), "ones", 2, seen_v)
    runs = _runs(InhandMachine.refill_pairs)
    assert max(runs) == 3 and runs.count(3) > 400             # three of every four pairs
    assert min(seen_v) == 32 and max(seen_v) == 56


def test_refill_at_the_first_pair_of_a_block(gen, runner):
    runner(gen.inhand_tile(), "flat", 0, [])
    edge = [t for t in TS.ShadowMachine.taken if t[0] == 0 and t[1] < TILE // 64]
    assert edge and all(p == 8 for _, _, p, _ in edge)


def test_refill_at_the_last_pair_of_the_tile(gen, runner):
    """The out-of-line path of lane 62 returns into the tile's last symbol; the exit applies the shift that is pending."""
    for kind in KINDS:
        for entry in range(4):
            TS.ShadowMachine.taken = []
            runner(gen.inhand_tile(), kind, entry, [])
            if any(lane == 62 and left == 1 for lane, left, _, _ in TS.ShadowMachine.taken):
                return
    assert False, "no stream refills at the last pair of a tile"


def _run_tiles_at(program, kind, entry_bytes):
    """test_decode_tile_model._run_tiles with the entry position anywhere in the window's first rows (there it is 0 .. 3)."""
    data, c2s, slots, states, marks, _, _ = T._case(kind)
    m = InhandMachine(program)
    m.table = slots
    lanes = np.arange(64, dtype=np.uint32)
    x, pos = marks[0]
    junk = np.random.default_rng(entry_bytes).integers(0, 256, entry_bytes, dtype=np.uint8)
    for t in range(2):
        win = np.zeros(T.WIN_BYTES, np.uint8)
        win[:entry_bytes] = junk                              # what lies in front of the entry position is never stream
        part = np.frombuffer(data[pos: pos + T.WIN_BYTES - entry_bytes], np.uint8)
        win[entry_bytes: entry_bytes + part.size] = part
        m.lds[T.WIN_BASE: T.WIN_BASE + T.WIN_BYTES] = win
        m.V[0], m.V[1], m.V[2] = 4 * lanes, T.WIN_BASE + 4 * lanes, T.REC_BASE + 2 * lanes
        m.S[10], m.S[11], m.S[12] = x, entry_bytes, TILE // 64
        m.S[14], m.S[15] = T.TABLE_ADDR & M32, T.TABLE_ADDR >> 32
        m.S[T.M0] = 0x1234ABCD
        m.run()
        assert m.S[T.M0] == 0x1234ABCD and not m.idx_on
        rec = m.lds[T.REC_BASE::2].astype(np.int64) | (m.lds[T.REC_BASE + 1:: 2].astype(np.int64) << 8)
        want = states[t * TILE: (t + 1) * TILE]
        assert np.array_equal(rec, want & 0xFFFF), (kind, entry_bytes, t, int(np.argmax(rec != (want & 0xFFFF))))
        x, pos = m.S[16], pos - entry_bytes + m.S[17]
        assert (x, pos) == marks[(t + 1) * TILE], (kind, entry_bytes, t)
    return m


@pytest.mark.parametrize("dword,byte", [(61, 1), (62, 0), (62, 2), (63, 0), (63, 3), (127, 0)])
def test_entry_at_the_end_of_a_window_row(gen, dword, byte):
    """After the priming s73 is 63 or 64 mod 64: the staging row takes one lane from a row and 63 from the next (or starts
    a row), and the first refills of the first block cross from one window row into the next."""
    InhandMachine.refill_pairs = []
    TS.ShadowMachine.taken = []
    m = _run_tiles_at(gen.inhand_tile(), "flat", 4 * dword + byte)
    # the priming leaves V <= 56 and a pair of the flat table takes 16 bits: the first refill is in the third pair at the latest
    assert InhandMachine.refill_pairs[0] <= 3 and m.pair_no == TILE
    if dword < 64:
        assert 1024 <= m.S[73] - dword <= 1027                # a byte per symbol: the tile crossed sixteen window rows


def test_frequency_4096_table(gen, runner, monkeypatch):
    case = TV._big_case()
    monkeypatch.setattr(T, "_case", lambda kind: case)
    for entry in range(4):
        seen_v = []
        runner(gen.inhand_tile(), "big", entry, seen_v)
        assert len(set(seen_v)) <= 2 and all(32 <= v <= 63 for v in seen_v)


def test_tile_shape(gen):
    """The main line is the shadow tile's; the refill has no lane read and no mode switch; the prefetch stands between the
    odd symbol's lane read and its record."""
    ih, sh = gen.inhand_tile(), gen.shadow_tile()
    main = lambda L: [s for s in L[L.index("2:"): L.index("s_set_gpr_idx_off")] if not (s.startswith("6") and s.endswith(":"))]
    assert main(ih)[:-len(gen.stage())] == main(sh)
    assert not [s for s in gen.inhand_refill() if s.startswith(("v_", "s_set_gpr_idx"))] and len(gen.inhand_refill()) == 5
    path = gen.inhand_path(6)
    rd = path.index("v_readlane_b32 s61, v226, s57")
    assert path[rd + 1: rd + 4] == ["v_readlane_b32 s65, v227, s73", "v_writelane_b32 v225, s57, 7", "s_branch 606b"]
    assert path.index("s_add_u32 s73, s73, 1") < rd
    assert ih[ih.index("606:") + 1] == "s_flbit_i32_b32 m0, s61"
    assert {"s54", "s55", "v227"} <= set(gen.inhand_clobbers()) and "s72" not in gen.inhand_clobbers()
    assert gen.VW == 227


def _replace_nth(good, old, new, n):
    at = [i for i, s in enumerate(good) if s == old][n]
    return good[:at] + [new] + good[at + 1:]


def test_mis_edits_are_caught(gen, runner):
    good = gen.inhand_tile()
    loop = good.index("2:")
    prefetch = "v_readlane_b32 s65, v227, s73"

    def prefetch_first():
        out = []
        for s in good:
            if s == prefetch:
                at = len(out) - 1 - out[::-1].index("s_add_u32 s73, s73, 1")
                out.insert(at, s)
            else:
                out.append(s)
        return out

    def label_late():
        out, held = [], None
        for s in good:
            if s.startswith("6") and s.endswith(":") and len(s) == 4:
                held = s
                continue
            out.append(s)
            if held:
                out.append(held)
                held = None
        return out

    n_prime = [s for s in good[:loop] if s == "v_readlane_b32 s65, v192, s73"]
    assert len(n_prime) == 2                                  # the entry's refill() and the priming
    in_loop = lambda old, new: good[:loop] + [new if s == old else s for s in good[loop:]]
    edits = {
        "the prefetch in front of the s_add": ("random", prefetch_first()),
        "v227 rebuilt from the wrong row": ("flat", [("v_mov_b32_e32 v227, v192" if s == "v_mov_b32_e32 v227, v193" else s) for s in good]),
        "the return label one instruction late": ("random", label_late()),
        "the refill's shift from the wrong register": ("random", [s.replace("s[64:65], s78", "s[64:65], s77") for s in good]),
        "the priming omitted": ("random", _replace_nth(good[:loop], "v_readlane_b32 s65, v192, s73", "s_nop 0", 1) + good[loop:]),
        "no staging at the block end": ("flat", in_loop("v_mov_b32_e32 v227, v192", "s_nop 0")),
        "staging of the next row only": ("flat", in_loop("v_mov_b32_e32 v227, v193", "s_nop 0")),
        "EXEC not restored at the block end": ("flat", in_loop("s_mov_b64 exec, s[54:55]", "s_nop 0")),
        "the refill without its s_add": ("random", in_loop("s_add_u32 s73, s73, 1", "s_nop 0")),
    }
    for name, (kind, bad) in edits.items():
        assert bad != good and len(bad) == len(good), name
        with pytest.raises(AssertionError):
            runner(bad, kind, 1, [])
    runner(good, "random", 1, [])
    runner(good, "flat", 1, [])


def test_generated_files_are_current(gen):
    csrc = os.path.join(ROOT, "alice-codec_amd", "csrc")
    for name, text in (("rans_decode_tile_ih.inc", gen.render_inhand()), ("rans_decode_tile_sh.inc", gen.render_shadow()),
                       ("rans_decode_tile.inc", gen.render()), ("rans_decode_tile_vec.inc", gen.render_vector())):
        with open(os.path.join(csrc, name)) as f:
            assert f.read() == text, f"{name} is not what gen_rans_decode_asm.py writes: regenerate it"
    assert gen.render_inhand() == gen.render_inhand()
