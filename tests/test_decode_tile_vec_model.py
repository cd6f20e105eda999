"""The vector decode tile (gen_rans_decode_asm.py: vector_tile(), rans_decode_tile_vec.inc) run on the model of the machine.

The tile evaluates umulhi(F', x) + B' on the vector unit for a whole table row and reads the finished state back with one
v_readlane.  The machine is tests/test_decode_tile_model.py's, subclassed: it learns v_mul_hi_u32 and v_add_u32_e64 and the
VGPR-index mode bits M0[13] (SRC1_REL) and M0[14] (SRC2_REL); everything else -- the runner, the window check at every pair
start, the oracle traces -- is that file's, used as it is.

VGPR-index mode as the model has it (gfx9 ISA, confirmed on the hardware by scripts/probes/gpr_idx_probe.hip): a VGPR in
the src1 / src2 position of a VALU instruction is relative when the bit is set; src0, the destination and an SGPR or a
constant in any position are not."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_tile_ref as R  # noqa: E402
import test_decode_tile_model as T  # noqa: E402
from decode_tile_ref import KINDS, M32, TILE  # noqa: E402

ROOT = T.ROOT
M0 = T.M0


class VecMachine(T.Machine):
    def _rel(self, n, bit):
        if self.idx_on and (self.S[M0] >> bit) & 1:
            n += self.S[M0] & 0xFF
        assert n < 256
        return n

    def _translate(self, pc, line):
        op, _, rest = line.partition(" ")
        if op not in ("v_mul_hi_u32", "v_add_u32_e64"):
            return super()._translate(pc, line)
        args = [a.strip() for a in rest.split(",")]
        assert len(args) == 3, line
        V = self.V
        d, r1 = self._vreg(args[0]), self._vreg(args[2])      # src1 is a VGPR in both uses
        if args[1][0] == "v":
            r0 = self._vreg(args[1])
            a = lambda: V[self._src0_row(r0)].astype(np.uint64)
        else:                                                 # VOP3: one SGPR or an inline constant
            s = self._src(args[1])
            a = lambda: np.uint64(s())
        b = lambda: V[self._rel(r1, 13)].astype(np.uint64)
        if op == "v_mul_hi_u32":
            def vmulhi():
                V[self._dst_row(d)] = ((a() * b()) >> np.uint64(32)).astype(np.uint32)
            return vmulhi

        def vadd():
            V[self._dst_row(d)] = ((a() + b()) & np.uint64(M32)).astype(np.uint32)
        return vadd


@pytest.fixture(scope="module")
def gen():
    return T._generator()


@pytest.fixture()
def vec_runner(monkeypatch):
    """test_decode_tile_model's runner, on the machine that knows the vector instructions."""
    monkeypatch.setattr(T, "Machine", VecMachine)
    return T._run_tiles


def test_model_multiplies_like_the_hardware():
    """umulhi over 64 lanes, 64-bit products that do not fit a float, and the relative src1."""
    m = VecMachine(["s_set_gpr_idx_on s20, 0x6", "v_mul_hi_u32 v226, s21, v64", "v_add_u32_e64 v226, v226, v128",
                    "v_readlane_b32 s22, v226, s21", "s_set_gpr_idx_off"])
    rng = np.random.default_rng(1)
    f, b = rng.integers(0, 1 << 32, 64, dtype=np.uint64), rng.integers(0, 1 << 32, 64, dtype=np.uint64)
    m.V[64 + 9], m.V[128 + 9] = f.astype(np.uint32), b.astype(np.uint32)
    m.S[20], m.S[21] = 9, 0xFEDCBA67
    m.run()
    want = [((int(f[l]) * 0xFEDCBA67 >> 32) + int(b[l])) & M32 for l in range(64)]
    assert [int(v) for v in m.V[226]] == want and m.S[22] == want[0x67 & 63]
    assert (m.V[64] == 0xA5A5A5A5).all()                      # nothing was written through the index


@pytest.mark.parametrize("entry", range(4))
@pytest.mark.parametrize("kind", KINDS)
def test_vector_tile_decodes_like_the_oracle(gen, vec_runner, kind, entry):
    seen_v = []
    vec_runner(gen.vector_tile(), kind, entry, seen_v)
    assert len(seen_v) == 2 * TILE // 2
    if kind == "flat":
        assert min(seen_v) == 32
    if kind == "peaked":
        assert max(seen_v) == 56
    if kind == "sparse":                   # 16-bit shifts, 24 bits in a pair (test_sparse_table_consumes_24_bits_in_a_pair)
        assert min(seen_v) == 32 and max(seen_v) == 56


def test_both_loop_phases_decode(gen, vec_runner):
    vec_runner(gen.vector_tile(0), "random", 1, [])
    vec_runner(gen.vector_tile(4), "random", 2, [])


def _big_case():
    """One symbol of frequency 4096: F' = 2^32 - 1, B' = 1 (rans.hip: build_dec_slots), the state never moves and no byte is
    consumed.  The stream is the state's four bytes; what follows them in the window is never read as stream."""
    freq, cum = [0] * 256, [0] * 6 + [4096] * 250
    freq[5] = 4096
    c2s = R.cum_to_sym(cum, freq)
    assert (c2s == 5).all()
    data = (1 << 23).to_bytes(4, "big") + np.random.default_rng(4096).integers(0, 256, T.WIN_BYTES + 64, dtype=np.uint8).tobytes()
    states, marks = R.trace(data, 2 * TILE, cum, freq, c2s)
    assert (states == 1 << 23).all() and marks[2 * TILE] == (1 << 23, 4)
    slots = np.concatenate([np.full(4096, M32, np.uint32), np.ones(4096, np.uint32)])
    return data, c2s, slots, states, marks, cum, freq


@pytest.mark.parametrize("entry", range(4))
def test_frequency_4096_table(gen, vec_runner, monkeypatch, entry):
    case = _big_case()
    monkeypatch.setattr(T, "_case", lambda kind: case)
    seen_v = []
    vec_runner(gen.vector_tile(), "big", entry, seen_v)
    assert len(set(seen_v)) <= 2 and all(32 <= v <= 63 for v in seen_v)   # nothing is consumed: the window stays as primed


@pytest.mark.parametrize("v", [0, 8, 16, 24])
def test_refill_from_the_vector_mode(gen, v):
    """The refill reads the window row as src0 of a v_readlane: it must set its own mode, whatever the symbol body left."""
    tile = gen.vector_tile()
    refill = gen.refill()
    at = tile.index("331:")
    assert tile[at + 1: at + 1 + len(refill)] == refill and tile[at + 1 + len(refill)] == "s_branch 431b"
    rng = np.random.default_rng(v)
    for _ in range(20):
        bits = int(rng.integers(0, 1 << 62)) >> (62 - v) if v else 0
        new = int(rng.integers(0, 1 << 32))
        m = VecMachine(["s_mov_b32 s76, 37", "s_set_gpr_idx_on s76, 0x6"] + refill)
        m.S[62], m.S[63] = 0, ((bits << 1 | 1) << (31 - v)) & M32
        m.S[64], m.S[73] = 0x80000000, 64 * 5 + 9
        m.V[192 + 5, 9] = new ^ 0x80000000
        m.run()
        w = m.S[62] | (m.S[63] << 32)
        assert w == ((bits << 32 | new) << 1 | 1) << (31 - v), (v, hex(bits), hex(new), hex(w))
        assert m.S[73] == 64 * 5 + 10 and m.S[64] == 0x80000000


def test_symbol_body_shape(gen):
    """Ten slots per symbol; each VOP3 instruction names at most one SGPR; the record is written before s61 goes."""
    body = gen.lookup_update_vector(7)
    assert len(body) == len(gen.lookup_update(7)) - 1
    for line in body:
        if line.startswith("v_"):
            sregs = {a.strip() for a in line.partition(" ")[2].split(",")[1:] if a.strip().startswith("s")}
            assert len(sregs) <= 1, line
    assert body.index("v_writelane_b32 v225, s61, 7") < body.index("v_readlane_b32 s61, v226, s61")
    # gfx940 and later want one wait state between a VALU write of a VGPR and a v_readlane of it (the model cannot see
    # that): the record's v_writelane stands between the add and the lane read
    assert body.index("v_readlane_b32 s61, v226, s61") - body.index("v_add_u32_e64 v226, v226, v128") >= 2
    fast, vec = gen.fast_tile(), gen.vector_tile()
    assert len(vec) == len(fast) - 64
    assert f"v{gen.VT}" in gen.vector_clobbers() and gen.VT == 226


def test_mis_edits_are_caught(gen, vec_runner):
    good = gen.vector_tile()
    edits = [("v_add_u32_e64 v226, v226, v128", "v_add_u32_e64 v226, v226, v64"),      # the add takes the F' row
             ("v_add_u32_e64 v226, v226, v128", "v_add_u32_e64 v226, v225, v128"),     # the add takes the record
             ("v_readlane_b32 s61, v226, s61", "v_readlane_b32 s61, v226, s76"),       # the lane select is the row
             ("v_readlane_b32 s61, v226, s61", "v_readlane_b32 s61, v128, s61"),       # reads the table (src0 is not relative)
             ("v_mul_hi_u32 v226, s61, v64", "v_mul_hi_u32 v226, s61, v128"),          # multiplies by B'
             ("s_set_gpr_idx_on s76, 0x6", "s_set_gpr_idx_on s76, 0x1")]               # src1 not relative: always row 0
    for old, new in edits:
        assert old in good
        bad = [new if line == old else line for line in good]
        with pytest.raises(AssertionError):
            vec_runner(bad, "random", 1, [])
    # the record after the lane read: it would hold the updated state
    at = good.index("v_writelane_b32 v225, s61, 0")
    bad = good[:at] + [good[at + 1], good[at]] + good[at + 2:]
    with pytest.raises(AssertionError):
        vec_runner(bad, "random", 1, [])


def test_generated_file_is_current(gen):
    inc = os.path.join(ROOT, "alice-codec_amd", "csrc", "rans_decode_tile_vec.inc")
    with open(inc) as f:
        assert f.read() == gen.render_vector(), "rans_decode_tile_vec.inc is not what gen_rans_decode_asm.py writes: regenerate it"
    assert gen.render_vector() == gen.render_vector()
    assert "s72" not in gen.vector_clobbers()
