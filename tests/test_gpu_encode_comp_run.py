"""Runs of complement blocks in the rANS encode chain on the GPU (alice-codec_amd/csrc/rans.hip, ripple64_comp_run and the clean
tile's loop around it): ONE launch of some thirty chains of one to three tiles through alice_codec_test_encode_chains_blocks,
each compared with the oracle's encoder byte for byte and, in RansResult, with the counts its symbols imply.  A run is a
sequence of blocks of one tile in which no symbol has a frequency of 16 or less: its first block enters with the plain state,
the others through the one-instruction edge, every block stores the byte of the block before it, and the last block's byte
follows the run.  The chains put the ends of runs at every block position and on both of the statement's two phases."""
import ctypes as C
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_encode_comp_step import BAND, CLEAN_ROOM, GUARD, TILE, _from_table  # noqa: E402

pytestmark = pytest.mark.gpu

L = 1 << 23


def _tables():
    mix = np.zeros(256, np.uint32)            # ten common symbols, a filler, two rare ones (frequencies 16 and 8)
    mix[:10] = 400
    mix[10], mix[200], mix[201] = 72, 16, 8
    assert mix.sum() == 4096
    common = mix.copy()                       # what the chains draw from: the rare ones are placed by hand
    common[200] = common[201] = 0
    common[10] += 24
    # the most a complement block can emit: every used symbol has the least frequency of the big class, 7.91 bits, so 99 lanes
    # in 100 emit (a byte per lane in every block would take 8 bits per symbol: frequency 16, not a complement block)
    all17 = np.array([17] * 240 + [16] + [0] * 15, np.uint32)
    two = np.zeros(256, np.uint32)            # 4079 emits about once in 1300 symbols, 17 nearly always
    two[[5, 200]] = [4079, 17]
    return mix, common, all17, two


def _chains(o):
    rng = np.random.default_rng(20261020)
    mix, common, all17, two = _tables()
    out = []

    def add(name, sym, hist, cap=None, sym_off=0, x_init=L, ref=None):
        sym = np.ascontiguousarray(sym, np.uint8)
        table = o.FrequencyTable(np.asarray(hist, np.uint32))
        f = table.freq.astype(np.int64)
        used = f[np.unique(sym)]
        assert ((used >= 1) & (used <= 4096)).all(), name
        ref = o.rans_encode(sym, table) if ref is None else ref
        out.append(SimpleNamespace(name=name, sym=sym, hist=np.asarray(hist, np.uint32), table=table, f=f, ref=ref, sym_off=sym_off,
                                   x_init=x_init, cap=2 * len(sym) + 4 + 320 + 128 if cap is None else cap(len(ref))))
        return out[-1]

    def with_rare(n, where):
        """symbols without a rare one, then one of frequency 16 or 8 in a random lane of each (tile, block) of `where`;
        tile j is the j-th from the END of the symbols (the chain runs back to front), block b its b-th from the end"""
        sym = _from_table(rng, n, common)
        for j, b in where:
            hi = n - j * TILE
            sym[hi - 1 - 64 * b - int(rng.integers(0, 64))] = 200 + int(rng.integers(0, 2))
        return sym

    # one rare block at each block position of a tile: a run ends in front of it on either phase, the next starts behind it
    for p in range(16):
        ch = add(f"rare-at-{p}", with_rare(2 * TILE, [(p & 1, p)]), mix)
        assert ch.f[200] == 16 and ch.f[201] == 8 and (ch.f[:11] >= 17).all()
    add("no-rare-2-tiles", with_rare(2 * TILE, []), mix)
    add("rare-adjacent", with_rare(2 * TILE, [(0, 5), (0, 6), (0, 15), (1, 0), (1, 1), (1, 14), (1, 15)]), mix)
    add("rare-alternating-even", with_rare(2 * TILE, [(j, b) for j in (0, 1) for b in range(0, 16, 2)]), mix)
    add("rare-alternating-odd", with_rare(2 * TILE, [(j, b) for j in (0, 1) for b in range(1, 16, 2)]), mix)
    add("rare-all-but-one", with_rare(2 * TILE, [(j, b) for j in (0, 1) for b in range(16) if (j, b) != (0, 7)]), mix)
    # three tiles: runs of 16, of 4 + 11 and of 9 + 6 blocks, a tile edge behind a run of either phase
    add("no-rare-3-tiles", with_rare(3 * TILE, []), mix)
    add("rare-3-tiles", with_rare(3 * TILE, [(0, 4), (1, 9)]), mix)
    # emission extremes
    ch = add("emits-nothing", np.zeros(2 * TILE, np.uint8), np.bincount([0] * 2 * TILE, minlength=256))
    assert ch.f[0] == 4096 and len(ch.ref) == 4
    ch = add("nearly-every-lane-emits", rng.integers(0, 240, 2 * TILE).astype(np.uint8), all17 * 3)
    assert (ch.f[:240] == 17).all() and len(ch.ref) - 4 >= 2000
    for lane in (0, 63):      # the 17 in one lane of every block: that lane emits, hardly any other
        sym = np.full(2 * TILE, 5, np.uint8)
        sym[np.arange(2 * TILE - 1 - lane, -1, -64)] = 200
        ch = add(f"emits-in-lane-{lane}", sym, two)
        assert ch.f[5] == 4079 and ch.f[200] == 17 and 28 <= len(ch.ref) - 4 <= 80
    # a tail tile behind the runs, unaligned symbols
    for off in (1, 2, 3):
        add(f"tail-unaligned-{off}", with_rare(2 * TILE + 37, [(1, 3 + off)]), mix, sym_off=off)
    # the region takes the first tile's worst case only: the other tiles go block by block, behind a flushed run
    for k in (1200, 1201):
        ch = add(f"cap-len+64+{k}", with_rare(3 * TILE, [(0, 11)] if k & 1 else []), mix, cap=lambda ln: ln + BAND + k)
        assert _expected(o, ch)[1:] == (1, 2), (ch.name, len(ch.ref), _expected(o, ch))
    # a state carried in (a RansEncoder object that goes on): not the clean path, the same bytes
    sym = with_rare(3 * TILE, [(0, 2)])
    table = o.FrequencyTable(mix)
    whole, behind = o.rans_encode(sym, table), o.rans_encode(sym[2 * TILE:], table)      # the LAST tile is encoded first
    x_in = int.from_bytes(behind[:4], "big")
    assert x_in != L
    add("state-carried-in", sym[:2 * TILE], mix, x_init=x_in, ref=whole[:len(whole) - (len(behind) - 4)])
    assert 30 <= len(out) <= 48 and all(len(c.sym) <= 3 * TILE + 64 for c in out)
    return out


def _expected(o, ch):
    """(complement blocks, clean tiles, other tiles) that the symbols, the table, the capacity and the start state imply"""
    n = len(ch.sym)
    tiles = (n + TILE - 1) // TILE
    small = ch.f[ch.sym] <= 16
    blocks = clean = 0
    for j in range(n // TILE if ch.x_init == L else 0):
        hi = n - j * TILE
        if ch.cap < len(ch.ref) + CLEAN_ROOM:      # only then can a tile be refused: ask the oracle what was written before it
            written = len(o.rans_encode(ch.sym[hi:], ch.table)) - 4 if j else 0
            if written + CLEAN_ROOM > ch.cap:
                continue
        clean += 1
        blocks += int((~small[hi - TILE: hi].reshape(16, 64).any(axis=1)).sum())
    return blocks, clean, tiles - clean


@pytest.fixture(scope="module")
def run(gpu_codec, oracle_mod):
    import torch
    lib, o = gpu_codec.load_library(), oracle_mod
    chains = _chains(o)
    k = len(chains)
    rng = np.random.default_rng(4)
    sym_at, reg_at, pos = [], [], 0
    for ch in chains:      # symbols inside one buffer of random bytes, regions inside one guard-filled buffer
        pos = (pos + 3) // 4 * 4 + 64
        sym_at.append(pos + ch.sym_off)
        pos += ch.sym_off + len(ch.sym) + 64
    host_sym = rng.integers(0, 256, (pos + 3) // 4 * 4, dtype=np.uint8)
    for ch, at in zip(chains, sym_at):
        host_sym[at: at + len(ch.sym)] = ch.sym
    pos = 0
    for c, ch in enumerate(chains):
        pos = (pos + 3) // 4 * 4 + 64
        reg_at.append(pos + (c & 3))
        pos += 3 + ch.cap + 64
    d_sym = torch.from_numpy(host_sym).cuda()
    d_out = torch.full((pos,), GUARD, dtype=torch.uint8, device="cuda")
    assert d_sym.data_ptr() % 4 == 0 and d_out.data_ptr() % 4 == 0
    vp = C.c_void_p
    syms, regions = (vp * k)(), (vp * k)()
    ns, caps = np.zeros(k, np.uint64), np.zeros(k, np.uint64)
    x_init, keep_open = np.zeros(k, np.uint32), np.zeros(k, np.uint32)
    hists = np.zeros((k, 256), np.uint32)
    for c, ch in enumerate(chains):
        assert ch.cap >= 64
        syms[c], regions[c] = d_sym.data_ptr() + sym_at[c], d_out.data_ptr() + reg_at[c]
        ns[c], caps[c], hists[c], x_init[c] = len(ch.sym), ch.cap, ch.hist, ch.x_init
    res = np.zeros((k, 7), np.uint32)
    u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    fn = lib.alice_codec_test_encode_chains_blocks
    fn.restype = C.c_int
    rc = fn(C.c_uint32(k), syms, ns.ctypes.data_as(u64p), hists.ctypes.data_as(u32p), None, None, regions,
            caps.ctypes.data_as(u64p), x_init.ctypes.data_as(u32p), keep_open.ctypes.data_as(u32p), res.ctypes.data_as(u32p),
            None)
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
        ch.want = _expected(o, ch)
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


def test_counters_equal_what_the_symbols_imply(run):
    by_name = {ch.name: ch for ch in run.chains}
    for ch in run.chains:
        g = ch.got
        print(ch.name, "blocks / clean / other", (g.blocks, g.fast, g.slow), "expected", ch.want)
        assert (g.blocks, g.fast, g.slow) == ch.want, ch.name
    for p in range(16):
        assert by_name[f"rare-at-{p}"].want == (31, 2, 0)
    assert by_name["no-rare-2-tiles"].want == (32, 2, 0) and by_name["no-rare-3-tiles"].want == (48, 3, 0)
    assert by_name["rare-adjacent"].want == (25, 2, 0) and by_name["rare-all-but-one"].want == (1, 2, 0)
    assert by_name["rare-alternating-even"].want == by_name["rare-alternating-odd"].want == (16, 2, 0)
    assert by_name["rare-3-tiles"].want == (46, 3, 0)
    assert by_name["emits-nothing"].want == by_name["nearly-every-lane-emits"].want == by_name["emits-in-lane-0"].want == (32, 2, 0)
    assert by_name["tail-unaligned-1"].want == (31, 2, 1)
    assert by_name["cap-len+64+1200"].want == (16, 1, 2) and by_name["cap-len+64+1201"].want == (15, 1, 2)
    assert by_name["state-carried-in"].want == (0, 0, 2)
