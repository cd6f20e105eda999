"""The lane coders of .alc version 2 and 3 at their edges, on the MI355X, bit for bit against tests/split_ref.py and
tests/wide_ref.py (which take any table that covers the data):

  a. stage encodes with a histogram that is not the data's but covers it (phantom symbols, other data's histogram, a
     starved table in which every coded step costs 12 bits), at three lane lengths, four output alignments and the two
     capacity edges;
  b. the longest lane stream either format can hold (24580 bytes, below the u16 directory entry's 65536);
  c. histograms that MISS a symbol of the data: the stage encodes refuse them (InvalidBufferSize, *out_len = 0, not a byte
     written, the symbol named) instead of dropping the symbol, and the next correct call succeeds;
  d. payloads of 256, 257 and 601 blocks: split_scan_kernel carries its running offset across rounds of 256 blocks, and
     damage behind the first round must still end in the reference's verdict;
  e. 2000+ seeded histograms through the table kernel against split_ref.normalize.

Every output buffer has guard bytes on both sides and every byte of it is checked.  Nothing here is built to fault: each
damaged payload is one the decoder's clamps turn into a verdict, and is checked on the CPU before it goes to the device."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import split_ref as R2  # noqa: E402
import wide_ref as R3  # noqa: E402
from test_gpu_split import corruption_cases  # noqa: E402
from test_split_host import LONGEST, lane_directories, starved_full_block  # noqa: E402

import torch  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64
FILL = 0xAB
UNSET = 0x5EED5EED          # what *out_len holds before a call
INVALID_BUFFER_SIZE = 1


class Fmt:
    """One of the two lane formats: its reference, its stage calls, its symbol type."""

    def __init__(self, version, ref, enc, dec, bound, dtype, max_lane):
        self.version, self.name, self.ref, self.enc, self.dec, self.bound, self.dtype, self.max_lane = version, f"v{version}", ref, enc, dec, bound, dtype, max_lane

    def __repr__(self):
        return self.name

    def coded(self, sym):
        return np.minimum(np.asarray(sym, np.int64), 255)

    def hist(self, sym):
        return np.bincount(self.coded(sym).reshape(-1), minlength=256).astype(np.uint32)


V2 = Fmt(2, R2, "alice_codec_dev_split_encode", "alice_codec_dev_split_decode", "split_stream_bound", np.uint8, 16384)
V3 = Fmt(3, R3, "alice_codec_dev_wide_encode", "alice_codec_dev_wide_decode", "wide_stream_bound", np.uint16, 8192)
FORMATS = [V2, V3]


def to_device(fmt, sym):
    host = np.ascontiguousarray(sym, fmt.dtype)
    if fmt.dtype is np.uint16:
        host = host.view(np.int16)
    return torch.from_numpy(host.copy()).to(DEV)


def dev_encode(codec, fmt, sym, hist, L, align=0, cap=None):
    """The stage encode of host symbols with the caller's histogram -> (rc, *out_len, payload, message).  The output starts
    GUARD + align bytes into a buffer of FILL bytes that ends GUARD bytes after the capacity; every byte the call did not
    announce must still be FILL, whatever it returned."""
    lib = codec.load_library()
    n = int(sym.size)
    d_sym = to_device(fmt, sym)
    cap = getattr(codec, fmt.bound)(n, L) if cap is None else cap
    out = torch.full((GUARD + align + cap + GUARD,), FILL, dtype=torch.uint8, device=DEV)
    h = np.ascontiguousarray(hist, np.uint32)
    got = C.c_uint64(UNSET)
    rc = getattr(lib, fmt.enc)(d_sym.data_ptr(), n, h.ctypes.data_as(C.POINTER(C.c_uint32)), L, out.data_ptr() + GUARD + align, cap,
                               C.byref(got), None)
    msg = (lib.alice_codec_last_error_message() or b"").decode()
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    lo = GUARD + align
    written = int(got.value) if rc == 0 else 0
    assert written <= cap
    assert (host[:lo] == FILL).all() and (host[lo + written:] == FILL).all(), "bytes outside the stream were written"
    assert np.array_equal(d_sym.cpu().numpy().view(fmt.dtype)[:n], np.asarray(sym, fmt.dtype)), "the symbols were modified"
    return rc, int(got.value), host[lo:lo + written].tobytes(), msg


def dev_decode(codec, fmt, payload, freq, L, n, align=0):
    """The stage decode -> (rc, symbols); guard elements on both sides of the symbol buffer"""
    lib = codec.load_library()
    buf = np.zeros(len(payload) + align + 1, np.uint8)
    buf[align:align + len(payload)] = np.frombuffer(payload, np.uint8)
    d_in = torch.from_numpy(buf).to(DEV)
    item = np.dtype(fmt.dtype).itemsize
    guard = np.full(GUARD + n + GUARD, 0x5A, fmt.dtype)
    d_out = to_device(fmt, guard)
    f = np.ascontiguousarray(freq, np.uint16)
    rc = getattr(lib, fmt.dec)(d_in.data_ptr() + align, len(payload), f.ctypes.data_as(C.POINTER(C.c_uint16)), L,
                               d_out.data_ptr() + item * GUARD, n, None)
    torch.cuda.synchronize()
    host = d_out.cpu().numpy().view(fmt.dtype)
    assert (host[:GUARD] == 0x5A).all() and (host[GUARD + n:] == 0x5A).all(), "symbols were stored outside the buffer"
    assert np.array_equal(d_in.cpu().numpy(), buf), "the payload was modified"
    return rc, host[GUARD:GUARD + n]


def sparse_symbols(fmt, n, seed, support=60, share=0.1):
    """n symbols over `support` of the 256 coded symbols (so absent ones exist); v3: about `share` of them escapes, with the
    smallest and the largest residual among them"""
    rng = np.random.default_rng(seed)
    top = 255 if fmt is V3 else 256
    alphabet = np.sort(rng.choice(top, support, replace=False))
    sym = alphabet[rng.choice(support, n, p=rng.dirichlet(np.ones(support) * 0.3))].astype(np.int64)
    if fmt is V3:
        esc = rng.random(n) < share
        sym = np.where(esc, 255 + rng.integers(0, 4096, n), sym)
        if n > 4:
            sym[1] = 255
            sym[n - 2] = 255 + 4095
    return sym.astype(fmt.dtype)


# ---- a. foreign histograms that cover the data ----

def move_to(hist, dst, amount):
    """`amount` counts from the largest bin to bin dst: the total stays"""
    h = hist.astype(np.int64).copy()
    src = int(np.argmax(h))
    assert src != dst and h[src] > amount
    h[src] -= amount
    h[dst] += amount
    return h


def foreign_histograms(fmt, sym, seed):
    """(kind, histogram): three histograms that total n, cover the data and are not the data's"""
    rng = np.random.default_rng(seed)
    n = sym.size
    own = fmt.hist(sym).astype(np.int64)
    absent = np.flatnonzero(own == 0)
    assert absent.size >= 8 and n >= 2048
    phantom = own.copy()
    for p in absent[[0, absent.size // 2, -1]]:
        phantom = move_to(phantom, int(p), int(rng.integers(1, n // 64)))
    other = np.bincount(np.concatenate([np.arange(256), rng.choice(256, n - 256, p=rng.dirichlet(np.ones(256) * 0.3))]), minlength=256)
    starved = (own > 0).astype(np.int64)
    starved[absent[-1]] = n - int(starved.sum())
    out = [("phantom", phantom), ("other data", other), ("starved", starved)]
    for kind, h in out:
        assert int(h.sum()) == n and (h[own > 0] > 0).all() and not np.array_equal(h, own), kind
    f = fmt.ref.normalize(starved)
    assert (f[own > 0] == 1).all()      # 12 bits per coded step
    return [(kind, h.astype(np.uint32)) for kind, h in out]


# (lane_symbols or None for the format's maximum, n): three blocks and 17 symbols of a fourth; one block and a second of 65
# symbols (lane 0 holds two, the others one); one partial block at the largest lane length (the full one is test b's)
FOREIGN_SHAPES = [(64, 64 * 64 * 3 + 17), (512, 64 * 512 + 65), (None, 70_001)]


@pytest.mark.parametrize("fmt", FORMATS, ids=repr)
@pytest.mark.parametrize("L,n", FOREIGN_SHAPES)
def test_foreign_histograms_that_cover_the_data(gpu_codec, fmt, L, n):
    L = L or fmt.max_lane
    sym = sparse_symbols(fmt, n, seed=n + L)
    ran = 0
    for kind, hist in foreign_histograms(fmt, sym, seed=L):
        freq = fmt.ref.normalize(hist)
        assert np.array_equal(gpu_codec.normalized_frequencies(hist), freq), kind
        want = fmt.ref.encode_channel(sym, freq, L)
        assert len(want) <= getattr(gpu_codec, fmt.bound)(n, L), kind
        for align in range(4):
            rc, got_len, got, _ = dev_encode(gpu_codec, fmt, sym, hist, L, align)
            assert rc == 0 and got_len == len(want) and got == want, (kind, align)
            rc, dec = dev_decode(gpu_codec, fmt, got, freq, L, n, align)
            assert rc == 0 and np.array_equal(dec, sym), (kind, align)
            ran += 1
        # a capacity of exactly the stream's length is enough; one byte less is refused with nothing written
        rc, got_len, got, _ = dev_encode(gpu_codec, fmt, sym, hist, L, 1, cap=len(want))
        assert rc == 0 and got == want, kind
        rc, got_len, got, msg = dev_encode(gpu_codec, fmt, sym, hist, L, 2, cap=len(want) - 1)
        assert rc == INVALID_BUFFER_SIZE and got_len == 0 and got == b"" and str(len(want)) in msg, (kind, msg)
        ran += 2
    assert ran == 3 * (4 + 2)


# ---- b. the longest lane stream ----

@pytest.mark.parametrize("fmt", FORMATS, ids=repr)
def test_longest_lane_stream(gpu_codec, fmt):
    sym, hist, L = starved_full_block(fmt.version)
    n = sym.size
    lane, length, bound = LONGEST[fmt.version]
    freq = fmt.ref.normalize(hist)
    want = fmt.ref.encode_channel(sym, freq, L)
    assert len(want) == length and getattr(gpu_codec, fmt.bound)(n, L) == bound
    ran = 0
    for align in (0, 3):
        rc, got_len, got, _ = dev_encode(gpu_codec, fmt, sym, hist, L, align)
        assert rc == 0 and got_len == length and got == want, align
        # the u16 directory entries as the device wrote them
        blen, dirs = lane_directories(got, n, L)
        assert dirs.shape == (2, 64) and (dirs[0] == lane).all() and int(dirs.max()) == lane < 65536
        assert (dirs[1, :5] == (5 if fmt is V2 else 7)).all() and (dirs[1, 5:] == 0).all()
        assert (blen == dirs.sum(axis=1) + 128).all()
        rc, dec = dev_decode(gpu_codec, fmt, got, freq, L, n, align)
        assert rc == 0 and np.array_equal(dec, sym), align
        ran += 1
    assert ran == 2


# ---- c. histograms that miss a symbol ----

MISS_L = 64
MISS_N = 64 * 64 * 2 + 64 * 3 + 5      # two full blocks and a partial one whose last row only lanes 0..4 reach
MISS_SYMBOL = 201


def missing_cases(fmt):
    """(name, symbols, histogram, first uncovered symbol, its count).  Every histogram totals n."""
    n = MISS_N
    base = sparse_symbols(fmt, n, seed=77, share=0.0 if fmt is V2 else 0.05)
    base[base == MISS_SYMBOL] = MISS_SYMBOL + 1
    places = [("index 0", 0), ("index n - 1", n - 1), ("last row of the partial block", 2 * 64 * 64 + 64 * 3 + 2),
              ("second block", 64 * 64 + 64 * 17 + 40)]
    cases = []
    for name, at in places:
        sym = base.copy()
        sym[at] = MISS_SYMBOL
        hist = move_to(fmt.hist(sym), MISS_SYMBOL, -1)          # the one count goes to the largest bin
        cases.append((name, sym, hist, MISS_SYMBOL, 1))
    own = fmt.hist(base)
    nowhere = np.zeros(256, np.int64)
    nowhere[np.flatnonzero(own == 0)[:2]] = [n - 1, 1]
    first = int(np.flatnonzero(own)[0])
    cases.append(("every symbol", base, nowhere, first, int(own[first])))
    if fmt is V3:
        plain = np.minimum(base, 250).astype(fmt.dtype)         # no escape, no 254
        sym = plain.copy()
        sym[n // 2] = 300
        cases.append(("an escape while hist[255] == 0", sym, move_to(fmt.hist(sym), 255, -1), 255, 1))
        sym = base.copy()
        sym[sym == 254] = 253
        sym[n // 3] = 254
        assert fmt.hist(sym)[255] > 0
        cases.append(("254 beside a covered 255", sym, move_to(fmt.hist(sym), 254, -1), 254, 1))
    for name, sym, hist, s, k in cases:
        used = fmt.hist(sym)
        assert int(hist.sum()) == n and hist[s] == 0 and used[s] == k and (hist[:s][used[:s] > 0] > 0).all(), name
    return [(name, sym, np.asarray(hist, np.uint32), s, k) for name, sym, hist, s, k in cases]


@pytest.mark.parametrize("fmt", FORMATS, ids=repr)
def test_a_histogram_that_misses_a_symbol_is_refused(gpu_codec, fmt):
    """The row of a frequency-0 symbol is the identity step of the lane coder: without the check the symbol is dropped by
    the count pass and the write pass alike, and the call returns 0 with a well-formed payload of other data."""
    ran = 0
    for k, (name, sym, hist, s, count) in enumerate(missing_cases(fmt)):
        rc, got_len, got, msg = dev_encode(gpu_codec, fmt, sym, hist, MISS_L, align=k % 4)
        print(f"{fmt} {name}: rc {rc}, *out_len {got_len}, message {msg!r}")
        assert rc == INVALID_BUFFER_SIZE and got_len == 0 and got == b"", (name, rc, got_len)
        assert re.search(rf"\bsymbol {s}\b", msg) and re.search(rf"\bcount {count}\b", msg), (name, msg)
        # no flag of the refusal survives: the same thread's next, correct call succeeds
        own = fmt.hist(sym)
        want = fmt.ref.encode_channel(sym, fmt.ref.normalize(own), MISS_L)
        rc, got_len, got, msg = dev_encode(gpu_codec, fmt, sym, own, MISS_L, align=k % 4)
        assert rc == 0 and got == want and msg == "", (name, msg)
        ran += 1
    assert ran == (5 if fmt is V2 else 7)


# ---- d. directories longer than one scan round ----

SCAN_L = 64
SCAN_N = [64 * 64 * 256, 64 * 64 * 257 - 1, 64 * 64 * 600 + 17]      # 256, 257 and 601 blocks
_scan_refs = {}


def scan_reference(fmt, n):
    """(symbols, frequencies, reference payload), computed once per shape and never modified"""
    key = (fmt.name, n)
    if key not in _scan_refs:
        sym = sparse_symbols(fmt, n, seed=n % 1000, support=40, share=0.02)
        freq = fmt.ref.normalize(fmt.hist(sym))
        _scan_refs[key] = (sym, freq, fmt.ref.encode_channel(sym, freq, SCAN_L))
    return _scan_refs[key]


@pytest.mark.parametrize("fmt", FORMATS, ids=repr)
@pytest.mark.parametrize("n", SCAN_N)
def test_directories_longer_than_one_scan_round(gpu_codec, fmt, n):
    sym, freq, want = scan_reference(fmt, n)
    assert R2.n_blocks_of(n, SCAN_L) == {SCAN_N[0]: 256, SCAN_N[1]: 257, SCAN_N[2]: 601}[n]
    ran = 0
    for align in (0, 1):
        rc, got_len, got, _ = dev_encode(gpu_codec, fmt, sym, fmt.hist(sym), SCAN_L, align)
        assert rc == 0 and got_len == len(want) and got == want, align
        rc, dec = dev_decode(gpu_codec, fmt, want, freq, SCAN_L, n, align)
        assert rc == 0 and np.array_equal(dec, sym), align
        ran += 1
    assert ran == 2


def late_damage(payload, n, L, seed):
    """(name, bytes): single-bit flips behind the scan's first round of 256 blocks -- block-table entries above index 256,
    the last one among them, and the last block's lane directory"""
    rng = np.random.default_rng(seed)
    nb = R2.n_blocks_of(n, L)
    blen = np.frombuffer(payload, "<u4", nb).astype(np.int64)
    last = 4 * nb + int(blen[:-1].sum())
    cases = []

    def flip(name, pos, bit):
        p = bytearray(payload)
        p[pos] ^= 1 << bit
        cases.append((f"{name} at {pos} bit {bit}", bytes(p)))

    for entry in (257, 300, 511, 512, nb - 1):
        flip(f"block table entry {entry}", 4 * entry + int(rng.integers(4)), int(rng.integers(8)))
    for lane in (0, 16, 17, 32, 63):
        flip(f"last block's directory, lane {lane}", last + 2 * lane + int(rng.integers(2)), int(rng.integers(8)))
    return cases


DAMAGE_PARTS = 4


@pytest.mark.parametrize("part", range(DAMAGE_PARTS))
def test_damage_behind_the_first_scan_round(gpu_codec, part):
    """test_gpu_split's corruption_cases at 601 blocks plus flips placed behind block 256 (the cases are dealt over
    DAMAGE_PARTS tests to keep each short).  Bounds safety as there: every read of the decoder is clamped to its lane
    stream and every store to its block, so a damaged payload ends in a verdict; no case is built to fault the device."""
    n, seed = SCAN_N[2], 6
    sym, freq, payload = scan_reference(V2, n)
    assert R2.n_blocks_of(n, SCAN_L) == 601
    generated = corruption_cases(payload, n, SCAN_L, seed)
    assert len(generated) == 54
    late_entries = [int(name.rsplit(" ", 1)[1]) // 4 for name, _ in generated if name.startswith("block table flip")]
    assert sum(e > 256 for e in late_entries) >= 3 and sum(e < 256 for e in late_entries) >= 1
    cases = generated + late_damage(payload, n, SCAN_L, seed)
    assert len(cases) == 54 + 10
    mine = cases[part::DAMAGE_PARTS]
    ran = 0
    for name, bad in mine:
        _, ref_ok = R2.decode_channel(bad, freq, SCAN_L, n)
        assert ref_ok is False, name      # (checked on the CPU when the cases were chosen: every one of them is detected)
        rc, _ = dev_decode(gpu_codec, V2, bad, freq, SCAN_L, n, align=(seed + ran) % 4)
        assert (rc == 0) == ref_ok and rc in (0, 4), (name, rc)
        ran += 1
    assert ran == len(cases) // DAMAGE_PARTS
    rc, dec = dev_decode(gpu_codec, V2, payload, freq, SCAN_L, n)
    assert rc == 0 and np.array_equal(dec, sym)


# ---- e. normalisation sweep ----

def peaks_beside_singletons(rng):
    """sum of the floors above 4096 and the largest frequency changing hands while the excess is taken back: many count-1
    symbols (each lifted to 1) beside two or three peaks whose frequencies are within a few steps of each other"""
    h = np.zeros(256, np.int64)
    singles = int(rng.integers(100, 253))
    where = rng.permutation(256)
    h[where[:singles]] = 1
    peaks = where[singles:singles + int(rng.integers(2, 4))]
    base = int(rng.integers(100_000, 10_000_000))      # a count of 1 is below one step of the scale
    h[peaks] = base + rng.integers(0, max(2, base // 2000), peaks.size)
    return h


def ties_at_the_maximum(rng):
    h = (rng.pareto(0.8, 256) * 50).astype(np.int64)
    h[rng.random(256) < 0.5] = 0
    k = int(rng.integers(2, 9))
    h[rng.choice(256, k, replace=False)] = int(h.max()) + int(rng.integers(1, 1000))
    return h


def short_sum(rng):
    """floors that sum to less than 4096: a few symbols with counts that divide badly"""
    k = int(rng.integers(2, 200))
    h = np.zeros(256, np.int64)
    h[rng.choice(256, k, replace=False)] = rng.integers(1000, 2000, k)
    return h


def one_symbol(rng):
    h = np.zeros(256, np.int64)
    h[int(rng.integers(256))] = int(rng.integers(1, 1 << 32))
    return h


def huge_total(rng):
    """totals at and above 2^32"""
    kind = int(rng.integers(3))
    if kind == 0:
        h = np.full(256, 1 << 24, np.int64)                     # exactly 2^32
        h[int(rng.integers(256))] += int(rng.integers(0, 3))
    elif kind == 1:
        h = rng.integers(0, 1 << 32, 256).astype(np.int64)
        h[rng.random(256) < 0.3] = 0
    else:
        h = np.full(256, (1 << 32) - 1, np.int64)               # up to the largest total there is
        h = np.where(rng.random(256) < rng.random() * 0.5, rng.integers(0, 3, 256), h)
    return h


def floor_boundary(rng):
    """a count on either side of the step from floor(count * 4096 / total) = q - 1 to q"""
    h = (rng.pareto(1.0, 256) * rng.integers(10, 10_000)).astype(np.int64)
    h[rng.random(256) < 0.3] = 0
    s = int(rng.integers(256))
    h[s] = 0
    rest = int(h.sum())
    q = int(rng.integers(1, 2000))
    # the smallest count c with c * 4096 >= q * (rest + c), minus 0 or 1
    c = -(-q * rest // (4096 - q))
    h[s] = min(max(1, c - int(rng.integers(2))), (1 << 32) - 1)
    return h


def general(rng):
    h = (rng.pareto(0.7, 256) * rng.integers(1, 100_000)).astype(np.int64)
    h[rng.random(256) < rng.random()] = 0
    return np.minimum(h, (1 << 32) - 1)


FAMILIES = [peaks_beside_singletons, ties_at_the_maximum, short_sum, one_symbol, huge_total, floor_boundary, general]
PER_FAMILY = 300


@pytest.mark.parametrize("family", FAMILIES, ids=lambda f: f.__name__)
def test_normalisation_sweep(gpu_codec, family):
    rng = np.random.default_rng(FAMILIES.index(family) + 100)
    ran = handed_over = short = 0
    hists = [family(rng) for _ in range(PER_FAMILY)]
    if family is general:
        hists[0] = np.zeros(256, np.int64)
    for h in hists:
        assert h.min() >= 0 and h.max() < 1 << 32
        want = R2.normalize(h)
        got = gpu_codec.normalized_frequencies(h.astype(np.uint32))
        assert np.array_equal(got, want), h.tolist()
        assert int(got.astype(np.int64).sum()) == (4096 if h.any() else 0)
        assert (got[h > 0] >= 1).all() and not got[h == 0].any()
        ran += 1
        floors = np.where(h > 0, np.maximum(1, h * 4096 // max(1, int(h.sum()))), 0)
        if family is short_sum:
            assert floors.sum() <= 4096
            short += bool(floors.sum() < 4096)
        if family is ties_at_the_maximum:
            assert (floors == floors.max()).sum() >= 2
        if family is peaks_beside_singletons:
            assert floors.sum() > 4096
            top_before = int(np.argmax(floors))
            handed_over += bool(floors[top_before] - want[top_before] < floors.sum() - 4096)   # someone else gave too
    assert ran == PER_FAMILY
    if family is peaks_beside_singletons:
        assert handed_over > PER_FAMILY // 2
    if family is short_sum:
        assert short > PER_FAMILY // 2
    if family is huge_total:
        assert sum(int(h.sum()) >= 1 << 32 for h in hists) > PER_FAMILY // 2 and any(int(h.sum()) == 1 << 32 for h in hists)
