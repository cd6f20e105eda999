"""The shadow decode tile (gen_rans_decode_asm.py: shadow_tile(), rans_decode_tile_sh.inc) run on the model of the machine.

The tile keeps the vector tile's arithmetic and moves three things: the state alternates between the shift pairs s[60:61]
and s[56:57], so that the record's v_writelane follows the lane read; both window shifts sit in wait-state holes, the odd
symbol's one pending until the next pair's even symbol (across the block end, and to the tile exit after the last pair); the
sentinel test stands in the even symbol, in front of the pair's copy.  The machine is test_decode_tile_vec_model's, the
runner, the oracle traces and the window check are test_decode_tile_model's, used as they are; only the place of the check
moves with the copy: "s_mov_b32 s56, s63" is where the tile relies on 32 <= V <= 63, and the runner asserts it there, with
the window's bits being the stream at the decoder's position, for every one of the 2 x 2048 copies of a run.

The machine also notes every refill branch it takes (lane of the symbol, blocks left, the shift that was pending, the fill
level after the pending shift), which is how the tests know that the streams reach the cases they are about."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_decode_tile_model as T  # noqa: E402
import test_decode_tile_vec_model as TV  # noqa: E402
from decode_tile_ref import KINDS, TILE  # noqa: E402

ROOT = T.ROOT
COPY = "s_mov_b32 s56, s63"


class ShadowMachine(TV.VecMachine):
    taken = []      # (lane, blocks left, pending shift, V at the test) of every refill branch taken; reset by the fixture

    def _translate(self, pc, line):
        run = super()._translate(pc, line)
        if not line.startswith("s_cbranch_scc1 3"):
            return run
        lane = int(line.split()[1][1:3])

        def branch():
            to = run()
            if to is not None:
                w = self.S[62] | (self.S[63] << 32)
                ShadowMachine.taken.append((lane, self.S[74], self.S[77], 63 - ((w & -w).bit_length() - 1)))
            return to
        return branch


def _copies(m):
    at = [pc for pc, line in enumerate(m.text) if line == COPY]
    assert len(at) == 32
    return at


@pytest.fixture(scope="module")
def gen():
    return T._generator()


@pytest.fixture()
def runner(monkeypatch):
    """test_decode_tile_model's runner on the shadow machine, with the window check at the shadow tile's copy."""
    monkeypatch.setattr(T, "Machine", ShadowMachine)
    monkeypatch.setattr(T, "_pair_starts", _copies)
    ShadowMachine.taken = []
    return T._run_tiles


def _shifts(kind):
    data, c2s, slots, states, marks, cum, freq = T._case(kind)
    out = []
    for x in (int(v) for v in states):
        slot = x & 4095
        s = int(c2s[slot])
        u = freq[s] * (x >> 12) + slot - cum[s]
        out.append(0 if u >= 1 << 23 else (8 if u >= 1 << 15 else 16))
    return out


@pytest.mark.parametrize("entry", range(4))
@pytest.mark.parametrize("kind", KINDS)
def test_shadow_tile_decodes_like_the_oracle(gen, runner, kind, entry):
    seen_v = []
    runner(gen.shadow_tile(), kind, entry, seen_v)
    assert len(seen_v) == 2 * TILE // 2                       # the invariant was checked at every copy
    if kind == "flat":
        assert min(seen_v) == 32                              # V = 32 exactly at a copy, again and again
    if kind == "peaked":
        assert max(seen_v) == 56
    if kind == "sparse":
        assert min(seen_v) == 32 and max(seen_v) == 56
    # a refill is taken exactly where the pending shifts left V <= 31
    assert ShadowMachine.taken and all(v <= 24 and v % 8 == 0 for _, _, _, v in ShadowMachine.taken)


def test_both_loop_phases_decode(gen, runner):
    runner(gen.shadow_tile(0), "random", 1, [])
    runner(gen.shadow_tile(4), "random", 2, [])
    assert gen.shadow_tile(0) != gen.shadow_tile(4)


def test_sixteen_bit_shifts_on_even_and_odd_symbols(gen, runner):
    """The sparse table shifts by 16 on both parities; an even symbol's 16 goes through s71 and hole 1 of the odd symbol,
    an odd symbol's through s77 and hole 1 of the next pair (or the tile exit)."""
    sh = _shifts("sparse")
    assert sh[0::2].count(16) > 20 and sh[1::2].count(16) > 20
    assert any(sh[i] == 16 for i in range(63, 2 * TILE, 64))   # ... and a 16 pending across a block end
    runner(gen.shadow_tile(), "sparse", 0, [])
    assert any(p == 16 for _, _, p, _ in ShadowMachine.taken)


def test_refill_at_the_first_pair_of_a_block(gen, runner):
    """Lane 0 of a block that is not the tile's first: the shift was pending across the record's ds_write, the counter and the
    loop branch, and the refill follows it at once."""
    runner(gen.shadow_tile(), "flat", 0, [])
    edge = [t for t in ShadowMachine.taken if t[0] == 0 and t[1] < TILE // 64]
    assert edge and all(p == 8 for _, _, p, _ in edge)


def _last_pair_case(gen, runner):
    for kind in KINDS:
        for entry in range(4):
            ShadowMachine.taken = []
            runner(gen.shadow_tile(), kind, entry, [])
            if any(lane == 62 and left == 1 for lane, left, _, _ in ShadowMachine.taken):
                return kind, entry
    return None


def test_refill_at_the_last_pair_of_the_tile(gen, runner):
    """The refill in the even symbol of the tile's last pair, then two more shifts of which one is applied only by the tile
    exit: the runner compares the exit's position with the oracle's."""
    assert _last_pair_case(gen, runner) is not None


@pytest.mark.parametrize("entry", range(4))
def test_frequency_4096_table(gen, runner, monkeypatch, entry):
    case = TV._big_case()
    monkeypatch.setattr(T, "_case", lambda kind: case)
    seen_v = []
    runner(gen.shadow_tile(), "big", entry, seen_v)
    assert len(set(seen_v)) <= 2 and all(32 <= v <= 63 for v in seen_v)


def test_symbol_shape(gen):
    """22 paid slots per pair: 13 + 11 instructions, the two records behind their lane reads."""
    even, odd = [s for s in gen.shadow_symbol(6) if not s.endswith(":")], gen.shadow_symbol(7)
    assert len(even) == 13 and len(odd) == 11
    for body, x, xn in ((even, "s61", "s57"), (odd, "s57", "s61")):
        rd = body.index(f"v_readlane_b32 {xn}, v226, {x}")
        assert body[rd + 1].startswith(f"v_writelane_b32 v225, {x}, ")            # the record, with x still there
        # gfx940 and later want one wait state between a VALU write of a VGPR and a v_readlane of it: hole 1
        assert rd - body.index("v_add_u32_e64 v226, v226, v128") >= 2
        assert body[body.index(f"s_flbit_i32_b32 m0, {xn}") + 2].startswith("s_movrels_b32")   # hole 2: the M0 wait state
        for line in body:
            if line.startswith("v_"):
                sregs = {a.strip() for a in line.partition(" ")[2].split(",")[1:] if a.strip().startswith("s")}
                assert len(sregs) <= 1, line
    assert even.index("s_cmp_eq_u32 s62, 0") < even.index("v_readlane_b32 s57, v226, s61") < even.index(COPY)
    used = " ".join(gen.refill()).replace("[", " s").replace(":", " s").replace("]", " ").replace(",", " ").split()
    assert not {"s56", "s57", "s60", "s61"} & set(used)
    assert {"s56", "s57", "v226"} <= set(gen.shadow_clobbers()) and "s72" not in gen.shadow_clobbers()
    assert len(gen.shadow_tile()) < len(gen.fast_tile())


def _replace(good, old, new):
    assert old in good
    return [new if line == old else line for line in good]


def _move(good, line, after):
    """Inside the block loop, every `line` moves behind the next `after` that follows it."""
    top = good.index("2:")
    out, held = good[:top], None
    for s in good[top:]:
        if s == line or (line.endswith("*") and s.startswith(line[:-1])):
            assert held is None
            held = s
            continue
        out.append(s)
        if held is not None and s == after:
            out.append(held)
            held = None
    assert held is None and len(out) == len(good) and out != good
    return out


def test_mis_edits_are_caught(gen, runner):
    good = gen.shadow_tile()
    refill = gen.refill()
    at = good.index("300:")
    assert good[at + 1: at + 1 + len(refill)] == refill and good[at + 1 + len(refill)] == "s_branch 400b"
    bad_refill = [s.replace("s78", "s57") for s in refill]
    scratch = list(good)
    for at in [i for i, s in enumerate(good) if s.startswith("3") and s.endswith(":")]:
        scratch[at + 1: at + 1 + len(refill)] = bad_refill
    edits = {
        # the even symbol's record only after the odd symbol has read its state into s61
        "record after the pair is reused": ("random", _move(good, "v_writelane_b32 v225, s61, *", "v_readlane_b32 s61, v226, s57")),
        "s77 not zero on entry": ("random", _replace(good, "s_mov_b32 s77, 0", "s_mov_b32 s77, 8")),
        # flat table: every shift is 8, so the last one is pending for certain
        "exit without the pending shift": ("flat", [s for i, s in enumerate(good) if not (i and good[i - 1] == "5:")]),
        "hole 2 of the odd symbol dropped": ("random", _replace(good, "s_mov_b32 s60, s56", "s_nop 0")),
        "compare behind the copy": ("random", _move(good, "s_cmp_eq_u32 s62, 0", COPY)),
        "refill scratch is s57": ("random", scratch),
    }
    assert len(edits["exit without the pending shift"][1]) == len(good) - 1
    for name, (kind, bad) in edits.items():
        assert bad != good, name
        with pytest.raises(AssertionError):
            runner(bad, kind, 1, [])
    runner(good, "random", 1, [])
    runner(good, "flat", 1, [])


def test_generated_files_are_current(gen):
    csrc = os.path.join(ROOT, "alice-codec_amd", "csrc")
    for name, text in (("rans_decode_tile_sh.inc", gen.render_shadow()), ("rans_decode_tile.inc", gen.render()),
                       ("rans_decode_tile_vec.inc", gen.render_vector())):
        with open(os.path.join(csrc, name)) as f:
            assert f.read() == text, f"{name} is not what gen_rans_decode_asm.py writes: regenerate it"
    assert gen.render_shadow() == gen.render_shadow()
