"""The complement step of the rANS encode chain on the GPU (alice-codec_amd/csrc/rans.hip, ripple64_comp and the block
choice of the clean tile): ONE launch of two dozen chains through alice_codec_test_encode_chains_blocks, each compared with
the oracle's RansEncoder byte for byte, and the number of blocks that took the new step compared with the number the symbols
and the table give on the host.  A block of a clean tile takes it when none of its 64 symbols has a frequency of 16 or less."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE = 1024
GUARD = 0xEE
CLEAN_ROOM = 2 * TILE + 4 + 320      # room a clean tile wants: written + this <= cap (rans.hip)
BAND = 64                            # least capacity for a stream of len bytes: len + 64


def _from_table(rng, n, f):
    """n symbols drawn from the distribution that a table which IS its histogram describes (f sums to 4096)"""
    assert int(np.sum(f)) == 4096
    return rng.choice(256, n, p=np.asarray(f, np.float64) / 4096.0).astype(np.uint8)


def _bench_like(o):
    """bench.py's synthetic content (moving sinusoids with periods in pixels + integer noise in [-4, 4]) at a small size,
    through the oracle's front half: CDF 9/7, quality 80.  -> (3, n) symbols: Y, Co, Cg"""
    w, h, f = 128, 72, 16
    rng = np.random.default_rng(1234)
    t = np.arange(f, dtype=np.float32).reshape(f, 1, 1, 1)
    y = np.arange(h, dtype=np.float32).reshape(1, h, 1, 1)
    x = np.arange(w, dtype=np.float32).reshape(1, 1, w, 1)
    s = np.array([23.0, 31.0, 17.0], np.float32).reshape(1, 1, 1, 3)
    ph = np.array([0.0, 1.0, 2.0], np.float32).reshape(1, 1, 1, 3)
    base = 128 + 90 * np.sin((x + 2 * t) / s + ph) * np.cos((y - t) / (0.7 * s))
    rgb = np.clip(np.round(base + rng.integers(-4, 5, (f, h, w, 3))), 0, 255).astype(np.uint8)
    return o.encode_symbols(rgb, w, h, f, 80, 1)      # 1 = CDF 9/7


def _chains(o):
    rng = np.random.default_rng(20261019)
    out = []

    def add(name, sym, hist=None, cap=None, sym_off=0, reg_off=0, built_for_it=True):
        sym = np.ascontiguousarray(sym, np.uint8)
        hist = np.bincount(sym, minlength=256).astype(np.uint32) if hist is None else np.asarray(hist, np.uint32)
        table = o.FrequencyTable(hist)
        f = table.freq.astype(np.int64)
        used = f[np.unique(sym)]
        assert ((used >= 1) & (used <= 4096)).all(), name      # every chain here is a clean chain
        ref = o.rans_encode(sym, table)
        # (default: room for every tile's worst case, a single tile's included)
        out.append(SimpleNamespace(name=name, sym=sym, hist=hist, table=table, f=f, ref=ref, sym_off=sym_off, reg_off=reg_off,
                                   cap=2 * len(sym) + 4 + 320 + 128 if cap is None else cap(len(ref)), built_for_it=built_for_it))
        return out[-1]

    # every used symbol in the big class: every block of every full tile takes the new step
    big = np.zeros(256, np.uint32)
    big[:32] = 100
    big[32:40] = [17, 17, 18, 30, 200, 300, 150, 164]
    assert big.sum() == 4096
    ch = add("all-big", _from_table(rng, 4 * TILE, big), hist=big)
    assert (ch.f[:40] == big[:40]).all()
    # one symbol of frequency 4096: T = 2^31
    ch = add("freq-4096", np.zeros(3 * TILE, np.uint8))
    assert ch.f[0] == 4096
    # frequencies 4079 and 17
    two = np.zeros(256, np.uint32)
    two[[5, 200]] = [4079, 17]
    ch = add("4079-and-17", _from_table(rng, 4 * TILE + 100, two), hist=two)
    assert ch.f[5] == 4079 and ch.f[200] == 17
    # frequencies 16 and 17 side by side
    f1617 = np.array([16] * 120 + [17] * 120 + [8] * 15 + [16], np.uint32)
    sym = _from_table(rng, 6 * TILE, f1617)
    sym[2 * TILE: 3 * TILE] = rng.integers(120, 240, TILE)      # one tile of 17s only, so that some blocks qualify
    ch = add("16-and-17", sym, hist=f1617 * 3)
    assert ch.f[0] == 16 and ch.f[120] == 17 and {16, 17} <= set(ch.f[np.unique(sym)])
    # a rare symbol in every other block of the tiles; in lane 0 only; in lane 63 only.  Block b of the tile that ends at
    # symbol index hi holds symbols hi - 64 (b + 1) .. hi - 64 b - 1, lane l the one at hi - 1 - 64 b - l.
    mix = np.zeros(256, np.uint32)
    mix[:10] = 400
    mix[10], mix[200], mix[201] = 72, 16, 8
    assert mix.sum() == 4096
    common = mix.copy()
    common[200] = common[201] = 0
    common[10] += 24
    n = 4 * TILE
    for name, blocks, lanes in (("rare-every-other-block", range(0, 16, 2), None), ("rare-in-lane-0", (1, 2, 5, 15), 0),
                                ("rare-in-lane-63", (0, 3, 4, 14), 63)):
        sym = _from_table(rng, n, common)
        for hi in range(n, 0, -TILE):
            for b in blocks:
                lane = int(rng.integers(0, 64)) if lanes is None else lanes
                sym[hi - 1 - 64 * b - lane] = 200 + (b & 1)
        ch = add(name, sym, hist=mix)
        assert ch.f[200] == 16 and ch.f[201] == 8 and (ch.f[:11] >= 17).all()
    # bench-like content: its own histograms
    for name, sym in zip(("bench-like-Y", "bench-like-Co", "bench-like-Cg"), _bench_like(o)):
        add(name, sym)
    # lengths; a distribution with a few rare symbols, so that both steps run
    few = mix.copy()
    few[10], few[200], few[201], few[202] = 56, 16, 8, 16
    assert few.sum() == 4096
    for n in (1024, 1025, 4096 + 63, 65536 + 37, (1 << 20) - 5):
        add(f"len-{n}", _from_table(rng, n, few), hist=few)
    # unaligned symbol pointers
    for off in (1, 2, 3):
        add(f"unaligned-{off}", _from_table(rng, 3 * TILE + 7 * off, few), hist=few, sym_off=off, reg_off=off)
    # the promised minimum capacity, and a little more: the last tiles leave the clean path
    for k in (0, 700):
        add(f"cap-len+64+{k}", _from_table(rng, 6 * TILE, few), hist=few, cap=lambda ln: ln + BAND + k, reg_off=1,
            built_for_it=True)
    add("cap-len+64-short", _from_table(rng, 2 * TILE, few), hist=few, cap=lambda ln: ln + BAND, built_for_it=False)
    assert 20 <= len(out) <= 28 and all(len(c.sym) <= 1 << 20 for c in out)
    return out


def _expected_blocks(o, ch):
    """Full tiles with room for a tile's worst case, back to front; of their blocks, those without a symbol of frequency <= 16."""
    n = len(ch.sym)
    small = ch.f[ch.sym] <= 16
    count = 0
    for j in range(n // TILE):
        hi = n - j * TILE
        if ch.cap < len(ch.ref) + CLEAN_ROOM:      # only then can a tile be refused: ask the oracle what was written before it
            written = len(o.rans_encode(ch.sym[hi:], ch.table)) - 4 if j else 0
            if written + CLEAN_ROOM > ch.cap:
                continue
        blocks = small[hi - TILE: hi].reshape(16, 64)
        count += int((~blocks.any(axis=1)).sum())
    return count


@pytest.fixture(scope="module")
def run(gpu_codec, oracle_mod):
    import torch
    lib, o = gpu_codec.load_library(), oracle_mod
    chains = _chains(o)
    k = len(chains)
    rng = np.random.default_rng(3)
    sym_at, reg_at, pos = [], [], 0
    for ch in chains:      # symbols inside one buffer of random bytes, regions inside one guard-filled buffer
        pos = (pos + 3) // 4 * 4 + 64
        sym_at.append(pos + ch.sym_off)
        pos += ch.sym_off + len(ch.sym) + 64
    host_sym = rng.integers(0, 256, (pos + 3) // 4 * 4, dtype=np.uint8)
    for ch, at in zip(chains, sym_at):
        host_sym[at: at + len(ch.sym)] = ch.sym
    pos = 0
    for ch in chains:
        pos = (pos + 3) // 4 * 4 + 64
        reg_at.append(pos + ch.reg_off)
        pos += ch.reg_off + ch.cap + 64
    d_sym = torch.from_numpy(host_sym).cuda()
    d_out = torch.full((pos,), GUARD, dtype=torch.uint8, device="cuda")
    assert d_sym.data_ptr() % 4 == 0 and d_out.data_ptr() % 4 == 0
    vp = C.c_void_p
    syms, regions = (vp * k)(), (vp * k)()
    ns, caps = np.zeros(k, np.uint64), np.zeros(k, np.uint64)
    hists = np.zeros((k, 256), np.uint32)
    for c, ch in enumerate(chains):
        assert ch.cap >= 64
        syms[c], regions[c] = d_sym.data_ptr() + sym_at[c], d_out.data_ptr() + reg_at[c]
        ns[c], caps[c], hists[c] = len(ch.sym), ch.cap, ch.hist
    res = np.zeros((k, 7), np.uint32)
    u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    fn = lib.alice_codec_test_encode_chains_blocks
    fn.restype = C.c_int
    rc = fn(C.c_uint32(k), syms, ns.ctypes.data_as(u64p), hists.ctypes.data_as(u32p), None, None, regions,
            caps.ctypes.data_as(u64p), None, None, res.ctypes.data_as(u32p), None)
    assert rc == 0
    host_out = d_out.cpu().numpy()
    outside = np.ones(len(host_out), bool)
    for ch, at in zip(chains, reg_at):
        outside[at: at + ch.cap] = False
    for c, ch in enumerate(chains):
        ln, state, flags, paths, fast, slow, blocks = (int(v) for v in res[c])
        end = reg_at[c] + ch.cap
        ch.got = SimpleNamespace(len=ln, state=state, flags=flags, paths=paths, fast=fast, slow=slow, blocks=blocks,
                                 stream=bytes(host_out[end - ln: end]) if ln <= ch.cap else None)
        ch.want_blocks = _expected_blocks(o, ch)
    return SimpleNamespace(chains=chains, guards_intact=bool((host_out[outside] == GUARD).all()),
                           symbols_intact=bool(np.array_equal(d_sym.cpu().numpy(), host_sym)))


def test_streams_lengths_and_final_states_equal_the_oracles(run):
    for ch in run.chains:
        g = ch.got
        where = (ch.name, len(ch.sym), ch.cap, hex(g.flags), hex(g.paths), g.fast, g.slow, g.blocks)
        assert g.flags == 0, where
        assert g.len == len(ch.ref), where
        assert g.stream == ch.ref, where
        assert g.state == int.from_bytes(ch.ref[:4], "big"), where      # finish() leaves the state in front, MSB first


def test_nothing_written_outside_the_regions(run):
    assert run.guards_intact, "bytes outside [region, region + cap) changed"
    assert run.symbols_intact, "symbol buffer changed"


def test_blocks_that_took_the_new_step(run):
    by_name = {ch.name: ch for ch in run.chains}
    for ch in run.chains:
        print(ch.name, "blocks", ch.got.blocks, "expected", ch.want_blocks, "of", 16 * (len(ch.sym) // TILE))
        assert ch.got.blocks == ch.want_blocks, (ch.name, ch.got.blocks, ch.want_blocks, ch.got.fast, ch.got.slow)
        if ch.built_for_it:
            assert ch.got.blocks > 0, ch.name
    full = lambda ch: 16 * (len(ch.sym) // TILE)
    assert by_name["all-big"].got.blocks == full(by_name["all-big"])
    assert by_name["freq-4096"].got.blocks == full(by_name["freq-4096"])
    assert by_name["4079-and-17"].got.blocks == full(by_name["4079-and-17"])
    assert by_name["rare-every-other-block"].got.blocks == full(by_name["rare-every-other-block"]) // 2
    for name in ("rare-in-lane-0", "rare-in-lane-63"):
        assert by_name[name].got.blocks == full(by_name[name]) - 4 * (len(by_name[name].sym) // TILE)
    assert 0 < by_name["16-and-17"].got.blocks < full(by_name["16-and-17"])
    assert 0 < by_name["cap-len+64+0"].got.blocks < by_name["cap-len+64+700"].got.blocks
    for name in ("bench-like-Y", "bench-like-Co", "bench-like-Cg"):      # most blocks of such content qualify
        assert 2 * by_name[name].got.blocks > full(by_name[name])
