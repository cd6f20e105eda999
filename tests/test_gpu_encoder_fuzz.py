"""Randomised parity of the rANS encode chain kernel (alice-codec_amd/csrc/rans.hip, rans_encode_kernel, both instances)
against the oracle's RansEncoder (reference behaviour: src/rans.rs:269-308), byte for byte, aimed at the places where the
kernel changes path: clean one-compare tiles handing over to general blocks when the region runs short, tail tiles, the exact
serial block, refused blocks, and the three symbol loads (aligned, funnel shift, bytewise).  Chains are launched directly
(alice_codec_test_encode_chains: one launch, no retry, flags and the kEncPath* mask as the kernel left them) with every
region inside a guard-filled buffer.  For every chain the mask and the tile counts the kernel reports are compared with
what its documented conditions predict from the oracle's stream lengths, and over the file every path bit must be seen."""
import ctypes as C
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rans_tables import custom_oracle_table  # noqa: E402

pytestmark = pytest.mark.gpu

L = 1 << 23
TILE = 1024
GUARD = 0xEE
OVERFLOW, DIVERGES = 4, 2      # RansResult.flags: kRansOverflow (kernels.h), kTableDiverges (common.h)
CLEAN, CAP_REFUSED, NOT_CLEAN, TAIL, EXACT, NO_ROOM, FUNNEL, BYTES_END, BYTES_HEAD = (1 << i for i in range(9))
PATHS = {CLEAN: "clean tile", CAP_REFUSED: "general block: capacity test refused the clean tile",
         NOT_CLEAN: "general block: table or start state not clean", TAIL: "tail tile", EXACT: "exact serial block",
         NO_ROOM: "block or finish refused for lack of room", FUNNEL: "funnel-shift load",
         BYTES_END: "bytewise load near the end of the symbols", BYTES_HEAD: "bytewise head load"}
# the clean tile wants room for its worst case: written + 2 * 1024 + 4 + 320 <= cap (rans.hip)
CLEAN_ROOM = 2 * TILE + 4 + 320
# a block is written while written + total + 4 + 64 <= cap: the four state bytes and the 64 dummy-store bytes at the
# front of the region.  So the least capacity that takes a stream of len bytes is len + 64.
BAND = 64


def _symbols(rng, n, p0, alphabet):
    s = rng.integers(1, alphabet, n)
    return (s * (rng.random(n) >= p0)).astype(np.uint8)


def _chain(o, name, sym, hist=None, cum=None, freq=None, cap=None, sym_off=0, reg_off=0, x_init=L, keep_open=0, expect="equal",
           table=None, **extra):
    sym = np.ascontiguousarray(sym, np.uint8)
    ch = SimpleNamespace(name=name, sym=sym, hist=None, cum=None, freq=None, sym_off=sym_off, reg_off=reg_off, x_init=x_init,
                         keep_open=keep_open, expect=expect, **extra)
    if cum is None:
        ch.hist = np.bincount(sym, minlength=256).astype(np.uint32) if hist is None else np.asarray(hist, np.uint32)
        ch.table = o.FrequencyTable(ch.hist)
        ch.f = ch.table.freq.astype(np.int64)
    else:
        ch.cum, ch.freq = np.asarray(cum, np.uint16), np.asarray(freq, np.uint16)
        ch.table = custom_oracle_table(o, cum, freq)
        ch.f = ch.freq.astype(np.int64)
    used = ch.f[np.unique(sym)]
    ch.diverges = bool((used == 0).any())
    ch.exact = bool(((used == 0) | (used > 4096)).any())
    if expect in ("equal", "overflow"):
        ch.ref = o.rans_encode(sym, ch.table)
    worst = 2 * len(sym) + 4 + 64 + 64
    ch.cap = worst if cap is None else (cap(len(ch.ref)) if callable(cap) else cap)
    return ch


def _load_bits(ptr, n):
    """Which loads the lanes of a chain take (load_tile in rans.hip): tile j covers [hi - 1024, hi), hi = n - 1024 j, and lane
    l loads the 16 bytes from lo = hi - 1024 + 16 l."""
    bits = 0
    ntiles = (n + TILE - 1) // TILE
    if not ntiles:
        return 0
    lo = (n - TILE * np.arange(ntiles)[:, None]) - TILE + 16 * np.arange(64)[None, :]
    if (lo < 0).any():
        bits |= BYTES_HEAD
    inside = lo[lo >= 0]
    mis = (ptr + inside) & 3
    if ((mis != 0) & (inside + 20 <= n)).any():
        bits |= FUNNEL
    if ((mis != 0) & (inside + 20 > n)).any():
        bits |= BYTES_END
    return bits


def _expected(o, ch, ptr):
    """(path mask, clean tiles, other tiles) that the kernel's conditions give for this chain."""
    n = len(ch.sym)
    full, tail = n // TILE, 1 if n % TILE else 0
    paths = _load_bits(ptr, n)
    slow = tail
    if tail:
        paths |= TAIL
    if full:
        if not (ch.hist is not None and not ch.exact and ch.x_init == L):
            paths |= NOT_CLEAN
            slow += full
        elif ch.cap < len(ch.ref) + CLEAN_ROOM:
            # bytes written before tile j = the stream of the symbols behind it, without its four state bytes
            refused = sum(1 for j in range(full)
                          if (len(o.rans_encode(ch.sym[n - j * TILE:], ch.table)) - 4 if j else 0) + CLEAN_ROOM > ch.cap)
            if refused:
                paths |= CAP_REFUSED
                slow += refused
    if full + tail - slow:
        paths |= CLEAN
    if ch.exact and n:
        paths |= EXACT
    if ch.expect == "overflow":
        paths |= NO_ROOM
    return paths, full + tail - slow, slow


def _launch(lib, chains, seed):
    import torch
    rng = np.random.default_rng(seed)
    k = len(chains)
    sym_at, reg_at, pos = [], [], 0
    for ch in chains:      # symbols in the middle of one large buffer of random bytes, 64 of them on either side
        pos = (pos + 3) // 4 * 4 + 64
        sym_at.append(pos + ch.sym_off)
        pos += ch.sym_off + len(ch.sym) + 64
    host_sym = rng.integers(0, 256, (pos + 3) // 4 * 4, dtype=np.uint8)
    for ch, at in zip(chains, sym_at):
        host_sym[at: at + len(ch.sym)] = ch.sym
    pos = 0
    for ch in chains:      # regions inside one large guard-filled buffer
        pos = (pos + 3) // 4 * 4 + 64
        reg_at.append(pos + ch.reg_off)
        pos += ch.reg_off + ch.cap + 64
    d_sym = torch.from_numpy(host_sym).cuda()
    d_out = torch.full((pos,), GUARD, dtype=torch.uint8, device="cuda")
    assert d_sym.data_ptr() % 4 == 0 and d_out.data_ptr() % 4 == 0
    vp = C.c_void_p
    syms, regions = (vp * k)(), (vp * k)()
    ns, caps = np.zeros(k, np.uint64), np.zeros(k, np.uint64)
    x_init, keep_open = np.zeros(k, np.uint32), np.zeros(k, np.uint32)
    by_hist = chains[0].hist is not None
    assert all((ch.hist is not None) == by_hist for ch in chains)
    hists, cums, freqs = np.zeros((k, 256), np.uint32), np.zeros((k, 256), np.uint16), np.zeros((k, 256), np.uint16)
    for c, ch in enumerate(chains):
        assert ch.cap >= 64        # the dummy-store band must lie inside the region
        syms[c], regions[c] = d_sym.data_ptr() + sym_at[c], d_out.data_ptr() + reg_at[c]
        ns[c], caps[c], x_init[c], keep_open[c] = len(ch.sym), ch.cap, ch.x_init, ch.keep_open
        if by_hist:
            hists[c] = ch.hist
        else:
            cums[c], freqs[c] = ch.cum, ch.freq
    res = np.zeros((k, 6), np.uint32)
    u16p, u32p, u64p = C.POINTER(C.c_uint16), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    rc = lib.alice_codec_test_encode_chains(k, syms, ns.ctypes.data_as(u64p), hists.ctypes.data_as(u32p) if by_hist else None,
                                            cums.ctypes.data_as(u16p), freqs.ctypes.data_as(u16p), regions, caps.ctypes.data_as(u64p),
                                            x_init.ctypes.data_as(u32p), keep_open.ctypes.data_as(u32p), res.ctypes.data_as(u32p), None)
    assert rc == 0
    host_out = d_out.cpu().numpy()
    outside = np.ones(len(host_out), bool)
    for ch, at in zip(chains, reg_at):
        outside[at: at + ch.cap] = False
    run = SimpleNamespace(chains=chains, guards_intact=bool((host_out[outside] == GUARD).all()),
                          symbols_intact=bool(np.array_equal(d_sym.cpu().numpy(), host_sym)))
    for c, ch in enumerate(chains):
        ln, state, flags, paths, fast, slow = (int(v) for v in res[c])
        end = reg_at[c] + ch.cap
        ch.got = SimpleNamespace(len=ln, state=state, flags=flags, paths=paths, fast=fast, slow=slow,
                                 stream=bytes(host_out[end - ln: end]) if ln <= ch.cap else None, ptr=d_sym.data_ptr() + sym_at[c])
    return run


def _check(o, ch):
    g = ch.got
    where = (ch.name, len(ch.sym), ch.cap, ch.sym_off, ch.reg_off, hex(g.flags), hex(g.paths))
    if ch.expect == "diverges":
        assert g.flags & DIVERGES, where
    elif ch.expect == "overflow":
        assert g.flags == OVERFLOW, where
        assert g.len == len(ch.ref), where      # a refused block stores nothing but is counted: the host sizes its retry from this
    elif ch.expect == "equal":
        assert g.flags == 0, where
        assert g.len == len(ch.ref) and g.stream == ch.ref, where
    elif ch.keep_open:      # continued state, left open: the state goes back, its four bytes are not in the stream
        assert g.flags == 0 and g.state == ch.x_final, where
        assert g.len == len(ch.total) - 4 - (ch.len_first - 4) and g.stream == ch.total[4: 4 + g.len], where
    else:                   # continued state, finished: what a two-part encoder leaves in front of the first part's bytes
        assert g.flags == 0, where
        assert g.stream == ch.total[: g.len] and len(ch.total) - g.len == ch.len_first - 4, where
    if ch.expect != "diverges":     # (a table that diverges has no reference stream to predict the capacity test from)
        assert (g.paths, g.fast, g.slow) == _expected(o, ch, g.ptr), where
    else:
        assert g.paths & EXACT, where


# ---- the cases ----

def _table_cases(o, rng, count, tag):
    out = []
    f1617 = np.array([16] * 120 + [17] * 120 + [8] * 15 + [16], np.uint32)      # sums to 4096: the table is the histogram
    for i in range(count):
        kind = i % 9
        n = int(rng.integers(3 * TILE, 6 * TILE))
        if kind == 0:
            n = n // TILE * TILE
        hist = None
        if kind == 5:      # all-zero channel: symbol 0 at frequency 4096
            sym = np.zeros(n, np.uint8)
        elif kind == 6:    # one symbol s > 0 only
            sym = np.full(n, int(rng.integers(1, 256)), np.uint8)
        elif kind == 7:    # frequencies of exactly 16 and 17, either side of the small_f split of the one-compare step
            sym = rng.choice(256, n, p=f1617 / 4096.0).astype(np.uint8)
            hist = f1617 * 3
        else:
            sym = _symbols(rng, n, float(rng.choice([0.2, 0.7, 0.96])), int(rng.choice([3, 17, 256])))
        if kind == 8:      # the data's own table with freq[255] wrapped above 4096 (src/rans.rs:125-131) and 255 in use
            sym = _symbols(rng, n, 0.7, 17)
            sym[rng.integers(0, n, 4)] = 255
        ch = _chain(o, f"{tag}{i}/kind{kind}", sym, hist=hist, sym_off=i % 4, reg_off=i // 4 % 4,
                    cap=None if i % 2 else (lambda ln: ln + BAND + CLEAN_ROOM + int(rng.integers(0, 2000))))
        if kind == 5:
            assert ch.f[0] == 4096
        if kind == 7:
            assert ch.f[0] == 16 and ch.f[120] == 17 and {16, 17} <= set(ch.f[np.unique(sym)])
        assert not ch.diverges and (ch.exact if kind == 8 else not ch.exact or kind < 5)   # (a random draw may use a wrapped 255 too)
        out.append(ch)
    return out


def _residue_cases(o, rng, tag):
    """n = 3 * 1024 + r for every r: every number of blocks in the tail tile, every number of idle lanes in its last block"""
    return [_chain(o, f"{tag}{r}", _symbols(rng, 3 * TILE + r, 0.7, 17), sym_off=r % 4, reg_off=r // 4 % 4) for r in range(TILE)]


KS = (1, 64, 700, 1500, 2200, 2500)


def _capacity_cases(o, rng, tag):
    out = []
    for i in range(8):
        # five tiles of at least 600 bytes each: longer than the 2372 bytes a clean tile wants, so the chain starts clean
        n = 5 * TILE + (0 if i % 2 == 0 else int(rng.integers(1, TILE)))
        sym = _symbols(rng, n, 0.2, [40, 256][i // 4])
        out.append(_chain(o, f"{tag}{i}/len+64", sym, cap=lambda ln: ln + BAND, reg_off=i % 4, k=0))
        out.append(_chain(o, f"{tag}{i}/len+63", sym, cap=lambda ln: ln + BAND - 1, reg_off=i % 4, expect="overflow", k=-1))
        for k in KS:
            out.append(_chain(o, f"{tag}{i}/len+64+{k}", sym, cap=lambda ln: ln + BAND + k, reg_off=(i + k) % 4, k=k))
    return out


def _alignment_cases(o, rng, tag):
    out = []
    for off in range(4):
        for r in (0, 1, 15, 16, 17, 19, 20, 21, 63, 64, 65, 1023):
            n = int(rng.integers(3, 6)) * TILE + r
            out.append(_chain(o, f"{tag}{off}+{r}", _symbols(rng, n, 0.6, 40), sym_off=off, reg_off=(off + r) % 4))
        for n in (0, 1, 3, 16, 19, 20, 21, 100, 1023, 1024, 1025):
            out.append(_chain(o, f"{tag}short{off}+{n}", _symbols(rng, n, 0.6, 40), sym_off=off, reg_off=(off + n) % 4))
    return out


def _continued_cases(o, rng, tag, count):
    out = []
    for i in range(count):
        low, keep_open = i % 2 == 1, i // 2 % 2
        n = int(rng.integers(3 * TILE, 6 * TILE))
        sym = _symbols(rng, n, 0.7, 17)
        table = o.FrequencyTable(np.bincount(sym, minlength=256))
        for first_len in range(200, 1200):      # a first part after which encode(7, 60000) leaves a state below 2^23
            first = sym[:first_len]
            enc, alone = o.RansEncoder(), o.RansEncoder()
            for e in (enc, alone):
                e.encode_symbols(first, table)
                if low:
                    e.encode(7, 60000)
            if not low or enc.state < L:
                break
        x0 = enc.state
        assert (x0 < L) == low
        rest = sym[first_len:]
        if len(rest) < 3 * TILE:
            rest = np.concatenate([rest, sym])
        enc.encode_symbols(rest, table)
        x_final = enc.state
        out.append(_chain(o, f"{tag}{i}/{'low' if low else 'cont'}/{'open' if keep_open else 'finish'}", rest,
                          hist=np.bincount(sym, minlength=256), x_init=x0, keep_open=keep_open, expect="continued",
                          sym_off=i % 4, reg_off=i // 4 % 4, x_final=x_final, total=enc.finish(), len_first=len(alone.finish())))
    return out


def _array_cases(o, rng, count):
    out = []
    for i in range(count):
        kind = i % 5
        freq = rng.integers(1, 64, 256).astype(np.uint16)
        cum = np.minimum(np.cumsum(np.concatenate([[0], freq[:-1]])), 65535).astype(np.uint16)
        n = int(rng.integers(3 * TILE, 6 * TILE))
        if i % 3 == 0:
            n = n // TILE * TILE
        sym = _symbols(rng, n, 0.5, 200)      # symbols 0..199 in use, 200..255 not
        expect = "equal"
        if kind == 1:      # overlapping cum ranges
            cum = rng.integers(0, 4200, 256).astype(np.uint16)
        elif kind == 2:    # frequencies above 4096 in use
            for s in rng.integers(0, 200, 3):
                freq[s] = int(rng.integers(4097, 65536))
                cum[s] = int(rng.integers(0, 4000))
        elif kind == 3:    # a frequency of 0 in use: the reference does not terminate, the kernel reports it
            freq[int(rng.integers(1, 200))] = 0
            expect = "diverges"
        elif kind == 4:    # a frequency of 0 that is not in use
            freq[int(rng.integers(200, 256))] = 0
        ch = _chain(o, f"arrays{i}/kind{kind}", sym, cum=cum, freq=freq, expect=expect, sym_off=i % 4, reg_off=i // 4 % 4)
        assert ch.diverges == (kind == 3) and ch.exact == (kind in (2, 3))
        out.append(ch)
    return out


@pytest.fixture(scope="module")
def runs(gpu_codec, oracle_mod):
    lib, o = gpu_codec.load_library(), oracle_mod
    rng = np.random.default_rng(20261018)
    groups = {
        # up to 1024 chains in a launch: rans_encode_kernel<true>
        "mixed": _table_cases(o, rng, 240, "table") + _capacity_cases(o, rng, "cap") + _alignment_cases(o, rng, "align")
                 + _continued_cases(o, rng, "cont", 24),
        "residues": _residue_cases(o, rng, "residue"),
        "arrays": _array_cases(o, rng, 300),
        # more: rans_encode_kernel<false>
        "plain": _residue_cases(o, rng, "plain-residue")[::16] + _table_cases(o, rng, 900, "plain-table")
                 + _capacity_cases(o, rng, "plain-cap") + _alignment_cases(o, rng, "plain-align")
                 + _continued_cases(o, rng, "plain-cont", 16),
    }
    # the caller tables again, more than 1024 of them (same symbols and tables, other alignments)
    groups["plain-arrays"] = [SimpleNamespace(**{**vars(ch), "name": f"plain-{ch.name}/{i}", "sym_off": (ch.sym_off + 1 + i // 300) % 4,
                                                 "reg_off": (ch.reg_off + i // 300) % 4})
                              for i, ch in ((i, groups["arrays"][i % 300]) for i in range(1100))]
    assert all((300 <= len(g) <= 1024) != name.startswith("plain") for name, g in groups.items())
    assert all(len(g) >= 1100 for name, g in groups.items() if name.startswith("plain"))
    return {name: _launch(lib, chains, seed) for seed, (name, chains) in enumerate(groups.items())}


def _of(run, prefix):
    chains = [ch for ch in run.chains if ch.name.startswith(prefix)]
    assert chains
    return chains


@pytest.mark.parametrize("group", ["mixed", "residues", "arrays", "plain", "plain-arrays"])
def test_nothing_written_outside_the_regions(runs, group):
    assert runs[group].guards_intact, "bytes outside [region, region + cap) changed"
    assert runs[group].symbols_intact, "symbol buffer changed"


def test_histogram_tables(runs, oracle_mod):
    for ch in _of(runs["mixed"], "table"):
        _check(oracle_mod, ch)
        # never off the clean path with this much room, unless the table itself sends every block through the table check
        assert len(ch.sym) >= 3 * TILE and ch.got.fast == (0 if ch.exact else len(ch.sym) // TILE)


def test_every_residue_of_the_tile_size(runs, oracle_mod):
    for ch in _of(runs["residues"], "residue"):
        _check(oracle_mod, ch)


def _check_capacity(o, chains):
    both = 0
    for ch in chains:
        _check(o, ch)      # len + 64: equal; len + 63: kRansOverflow; len + 64 + k: equal, tiles as the room test predicts
        if ch.k > 0:
            # k < 2 * 1024 + 4 + 320 - 64 - 4 = 2304 - (bytes of the last tiles) is what refuses a clean tile: 2500 never does
            assert bool(ch.got.paths & CAP_REFUSED) == (ch.got.slow > (1 if len(ch.sym) % TILE else 0)), ch.name
            assert ch.k < 2304 or not ch.got.paths & CAP_REFUSED, ch.name
            if ch.k <= 64:     # the last full tile and the tail tile together stay below 2 * 1024 bytes < 2304 - 64
                assert ch.got.paths & CLEAN and ch.got.paths & CAP_REFUSED, (ch.name, hex(ch.got.paths))
            both += bool(ch.got.paths & CLEAN and ch.got.paths & CAP_REFUSED)
    assert both >= 8 * 2


def test_capacity_edges(runs, oracle_mod):
    _check_capacity(oracle_mod, _of(runs["mixed"], "cap"))


def test_symbol_alignment(runs, oracle_mod):
    seen = 0
    for ch in _of(runs["mixed"], "align"):
        _check(oracle_mod, ch)
        seen |= ch.got.paths
    assert seen & FUNNEL and seen & BYTES_END and seen & BYTES_HEAD


def _check_caller_tables(o, chains):
    kinds = set()
    for ch in chains:
        _check(o, ch)
        assert ch.got.fast == 0      # arrays carry no promise about the data: no clean tile
        kinds.add((ch.expect, ch.exact))
    assert kinds == {("equal", False), ("equal", True), ("diverges", True)}


def test_caller_tables(runs, oracle_mod):
    _check_caller_tables(oracle_mod, _of(runs["arrays"], "arrays"))


def test_continued_state(runs, oracle_mod):
    low = 0
    for ch in _of(runs["mixed"], "cont"):
        _check(oracle_mod, ch)
        low += ch.x_init < L
    assert low >= 8


def test_more_than_1024_chains(runs, oracle_mod):
    run = runs["plain"]
    assert len(run.chains) > 1024
    for ch in run.chains:
        _check(oracle_mod, ch)
    _check_capacity(oracle_mod, _of(run, "plain-cap"))
    assert len(runs["plain-arrays"].chains) > 1024
    _check_caller_tables(oracle_mod, runs["plain-arrays"].chains)


def test_every_encode_path_was_taken(runs):
    for groups in (("mixed", "residues", "arrays"), ("plain", "plain-arrays")):      # each instance of the kernel on its own
        seen = 0
        for name in groups:
            for ch in runs[name].chains:
                seen |= ch.got.paths
        missing = [text for bit, text in PATHS.items() if not seen & bit]
        assert not missing, f"encode branches never taken by {groups}: {missing} (mask {seen:#x})"


# ---- alice_codec_dev_rans_encode, the public call ----

def _dev_encode(lib, sym, hist, cap, sym_off, out_off):
    """-> (return code, stream or None, guards intact)"""
    import torch
    n = len(sym)
    buf = torch.full((n + 136,), 0xA5, dtype=torch.uint8, device="cuda")
    if n:
        buf[64 + sym_off: 64 + sym_off + n] = torch.from_numpy(np.ascontiguousarray(sym)).cuda()
    out = torch.full((cap + 136,), GUARD, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 4 == 0 and out.data_ptr() % 4 == 0
    off, ln = C.c_uint64(0), C.c_uint64(0)
    before = buf.cpu().numpy()
    rc = lib.alice_codec_dev_rans_encode(buf.data_ptr() + 64 + sym_off, n, hist.ctypes.data_as(C.POINTER(C.c_uint32)),
                                         out.data_ptr() + 64 + out_off, cap, C.byref(off), C.byref(ln), None)
    host = out.cpu().numpy()
    at = 64 + out_off
    intact = bool((host[:at] == GUARD).all() and (host[at + cap:] == GUARD).all() and np.array_equal(buf.cpu().numpy(), before))
    if rc != 0:
        return rc, None, intact
    assert off.value + ln.value == cap
    return rc, bytes(host[at + off.value: at + cap]), intact


def test_public_call_every_alignment_at_the_promised_capacity(gpu_codec, oracle_mod):
    lib = gpu_codec.load_library()
    rng = np.random.default_rng(11)
    for sym_off in range(4):
        for out_off in range(4):
            n = int(rng.integers(3 * TILE, 6 * TILE))
            sym = _symbols(rng, n, 0.6, 40)
            hist = np.bincount(sym, minlength=256).astype(np.uint32)
            ref = oracle_mod.rans_encode(sym, oracle_mod.FrequencyTable(hist))
            caps = (int(lib.alice_codec_rans_stream_bound(hist.ctypes.data_as(C.POINTER(C.c_uint32)), n)),
                    int(lib.alice_codec_rans_stream_bound(None, n)))
            assert caps[0] <= caps[1]
            for cap in caps:
                rc, got, intact = _dev_encode(lib, sym, hist, cap, sym_off, out_off)
                assert rc == 0 and got == ref and intact, (sym_off, out_off, n, cap)


def test_public_call_refuses_a_region_that_is_too_small(gpu_codec, oracle_mod):
    lib = gpu_codec.load_library()
    rng = np.random.default_rng(12)
    sym = _symbols(rng, 4 * TILE + 77, 0.2, 256)
    hist = np.bincount(sym, minlength=256).astype(np.uint32)
    ref = oracle_mod.rans_encode(sym, oracle_mod.FrequencyTable(hist))
    for cap, out_off in ((len(ref) + BAND - 1, 1), (len(ref) // 2, 2), (4 + 64 + 64, 3), (100, 0)):
        rc, _, intact = _dev_encode(lib, sym, hist, cap, 3, out_off)
        assert rc == 1 and gpu_codec.load_library().alice_codec_last_error() == 1, cap      # InvalidBufferSize
        assert intact, cap
    rc, got, intact = _dev_encode(lib, sym, hist, len(ref) + BAND, 3, 1)
    assert rc == 0 and got == ref and intact


def test_public_call_with_a_histogram_that_is_not_the_datas(gpu_codec, oracle_mod):
    """FrequencyTable::from_histogram(hist) + RansEncoder is defined for any symbols.  hist = {3: 1000}: symbol 3 gets
    frequency 4096, every other symbol 1, and the reference's correction wraps freq[255] to 65282 (src/rans.rs:125-131).
    A 255 in the data is then encoded with x' = ((x / 65282) << 12) + x % 65282 + cum: the exact serial block's job."""
    lib = gpu_codec.load_library()
    rng = np.random.default_rng(13)
    hist = np.zeros(256, np.uint32)
    hist[3] = 1000
    table = oracle_mod.FrequencyTable(hist)
    assert table.freq[255] == 65282 and table.freq[3] == 4096
    for sym_off in (0, 1):
        n = 4 * TILE + 100
        sym = np.full(n, 3, np.uint8)
        sym[rng.integers(0, n, 300)] = rng.integers(0, 255, 300)      # other symbols of frequency 1
        sym[n - 2 * TILE - rng.integers(100, 900, 5)] = 255             # a few 255s in a middle tile
        ref = oracle_mod.rans_encode(sym, table)
        rc, got, intact = _dev_encode(lib, sym, hist, int(lib.alice_codec_rans_stream_bound(None, n)), sym_off, 2)
        assert rc == 0 and intact
        assert got == ref, (sym_off, len(got), len(ref))
    # a symbol whose frequency in that table is 0 does not exist for the reference: reported, not encoded
    hist2 = np.zeros(256, np.uint32)
    hist2[:255] = 16
    hist2[0] = 32      # sums to 4096: symbols 0..254 keep their counts, symbol 255 gets 1, and the correction takes it to 0
    assert oracle_mod.FrequencyTable(hist2).freq[255] == 0
    sym = np.zeros(3 * TILE, np.uint8)
    sym[1500] = 255
    rc, _, intact = _dev_encode(lib, sym, hist2, int(lib.alice_codec_rans_stream_bound(None, len(sym))), 0, 0)
    assert rc == 6 and intact      # ReferenceDiverges
