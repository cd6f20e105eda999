"""Cases for the rANS decode chain in merged launches (tests/test_gpu_decode_chain_fuzz.py) and a model of the kernel's tile
loop that predicts, per case, which branches the chain takes.  CPU only; nothing here imports the library.

A case is (table, stream bytes, symbol count, stream misalignment 0..3, output misalignment 0..3, optional resume point).
The content classes are those of tests/test_gpu_decoder_fuzz.py (intact, truncated, corrupted, short, overlong, constant
channels on garbage, zero runs, garbage) and its caller tables (overlaps and gaps, a frequency above 4096 that owns slots, a
frequency of 4096 at a non-zero cum), at 3 to 5 tiles of 4096 symbols with every class of tail, plus chains of 0 and 1
symbols, chains that resume an oracle decoder object in the middle of its stream, and streams with a head below 2^23 that go
on (the first tile refused, its last symbol's renormalisation settled, or not, in front of the second).

The model (predict) transcribes only the DECISIONS of rans_decode_kernel (alice-codec_amd/csrc/rans.hip), as the kDecPath*
comments in csrc/kernels.h name them: the dry tile, the window base and whether the window lies wholly inside the stream, the
owed renormalisation fed or still starved, a state below 2^23, a speculative tile kept or dropped, the exact loop and its
starvation at the end of the window, the tail, the unaligned output.  All arithmetic is the oracle's: every state, position
and symbol comes from an oracle RansDecoder stepped over the stream, or, for a speculative tile, over a copy of the stream
padded with one window of zero bytes."""
import functools
import os
import sys
from dataclasses import dataclass
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [p for p in (_HERE, os.path.dirname(_HERE)) if p not in sys.path]
from rans_tables import custom_oracle_table  # noqa: E402
from test_gpu_decoder_fuzz import PATHS, _symbols  # noqa: E402

TILE = 4096
WINDOW = 8448              # kDecWinBytes: 33 dwords per lane
RANS_L = 1 << 23
DRY, WHOLE, SPEC_KEPT, SPEC_DROPPED, PENDING_FED, EXACT, STARVED, TAIL, UNALIGNED, BELOW_L, STILL_STARVED = (1 << b for b in range(11))
TAILS = (1, 63, 64, 65, 4095)
HIST_CLASSES = ("multiple of 4096", "tail", "truncated", "truncated in last window", "late corruption", "early corruption",
                "shorter than the state", "more symbols than encoded", "all-zero channel", "single-symbol channel", "zero run",
                "garbage")
TABLE_CLASSES = ("caller table", "overlaps and gaps", "frequency above 4096", "frequency 4096 at a cum")


@dataclass(eq=False)
class Case:
    cls: str
    data: bytes
    n: int                            # symbols the chain decodes
    in_mis: int
    out_mis: int
    hist: Optional[np.ndarray] = None     # 256 counts (the table is FrequencyTable::from_histogram's), or
    cum: Optional[np.ndarray] = None      # explicit arrays
    freq: Optional[np.ndarray] = None
    n1: Optional[int] = None          # resume: symbols an oracle decoder object has decoded before the chain takes over
    note: str = ""

    def __str__(self):
        res = "" if self.n1 is None else f", resumes after {self.n1}"
        return f"{self.cls}{' ' + self.note if self.note else ''} (n {self.n}, {len(self.data)} bytes, in+{self.in_mis}, out+{self.out_mis}{res})"


class _Oracle:
    """The oracle's decoder over one case's stream: state, position and symbols after any number of symbols, each from a fresh
    oracle RansDecoder object."""

    def __init__(self, case):
        import oracle
        self._o = oracle
        self.table = oracle.FrequencyTable(case.hist) if case.hist is not None else custom_oracle_table(oracle, case.cum, case.freq)
        self.data = case.data
        self.padded = case.data + bytes(WINDOW)
        self._at = {}
        c2s, freq, cum = self.table.cum_to_sym, self.table.freq.astype(np.int64), self.table.cum_freq.astype(np.int64)
        owner_freq = freq[c2s]
        # RansTable.flags as build_dec_slots sets them, and what the kernel derives from them
        self.exact_only = bool((owner_freq > 4096).any())                      # kTableDecExact
        big = bool((owner_freq == 4096).any())                                   # kTableDecBig
        o0 = int(c2s[0])
        self.slot0_big = big and int(freq[o0]) == 4096 and int(cum[o0]) == 0
        self.one_owner = big and bool((c2s == o0).all())

    def _run(self, padded, i):
        key = (padded, i)
        if key not in self._at:
            d = self._o.RansDecoder(self.padded if padded else self.data)
            sym = d.decode_n(i, self.table)
            self._at[key] = (d.state, d.pos, sym)
        return self._at[key]

    def at(self, i, padded=False):
        """(state, position) of a decoder object that has decoded i symbols"""
        return self._run(padded, i)[:2]

    def symbols(self, lo, hi, padded=False):
        return self._run(padded, hi)[2][lo:hi]


@functools.lru_cache(maxsize=None)
def oracle_of(case):
    return _Oracle(case)


def start_of(case):
    """(resume, x0, pos0) of the chain's descriptor"""
    if case.n1 is None:
        return 0, 0, 0
    x, pos = oracle_of(case).at(case.n1)
    return 1, x, pos


def expected(case):
    """(symbols, len, final state): the oracle's plain decode, or for a resume case the next n symbols of its decoder object
    and the object's state and position afterwards"""
    import oracle
    o = oracle_of(case)
    if case.n1 is None:
        sym = oracle.rans_decode(case.data, case.n, o.table)
        d = oracle.RansDecoder(case.data)
        d.decode_n(case.n, o.table)
    else:
        d = oracle.RansDecoder(case.data)
        d.decode_n(case.n1, o.table)
        sym = d.decode_n(case.n, o.table)
    return sym, d.pos, d.state


def predict(case, in_mis=None, out_mis=None):
    """What rans_decode_kernel does with this case: dict(paths, fast_tiles, slow_tiles, symbols, len, state)."""
    in_mis = case.in_mis if in_mis is None else in_mis
    out_mis = case.out_mis if out_mis is None else out_mis
    o = oracle_of(case)
    ln, n, base = len(case.data), case.n, case.n1 or 0
    x, pos = o.at(base)            # RansDecoder::new, or the object's state and position (resume / x0 / pos0)
    pending = False                # the last symbol came from the exact loop: its renormalisation is owed, `pos` is where it starts
    done = paths = n_fast = n_slow = 0
    out = []
    while done < n:
        want = min(n - done, TILE)
        # while bytes are owed x is not the kernel's, but the only use of it before they are fed is the dry tile's, and with
        # pos >= len nothing can be owed
        dry_ok = not o.exact_only and (not o.slot0_big or (o.one_owner and x != 0))
        unaligned = UNALIGNED if (out_mis + done) & 3 else 0
        if want == TILE and pos >= ln and dry_ok:                     # kDecPathDry
            paths |= DRY | unaligned
            out.append(o.symbols(base + done, base + done + TILE))
            done += TILE
            x = o.at(base + done)[0]
            n_fast += 1
            continue
        mis = (in_mis + pos) & 3                                       # the window's base: dword aligned in memory
        wbase = pos - mis if pos >= mis else pos & ~3
        whole = ln - wbase >= WINDOW and (in_mis + wbase) & 3 == 0
        fast = want == TILE and pos < ln and not o.exact_only
        saved = (x, pos, pending)
        if fast and pending:
            xs, ps = o.at(base + done)                                 # where the owed renormalisation ends
            if xs >= RANS_L and ps - pos <= 8:
                x, pos, pending = xs, ps, False
                paths |= PENDING_FED
            else:                                                      # the stream ends first, or more than 8 bytes are owed
                fast = False
                paths |= STILL_STARVED
        if fast and x < RANS_L:
            fast = False
            paths |= BELOW_L
        if fast:
            xs, ps = o.at(base + done + TILE, padded=True)
            if ps > ln:                                                # padding consumed
                x, pos, pending = saved
                fast = False
                paths |= SPEC_DROPPED
            else:
                paths |= WHOLE if whole else SPEC_KEPT
                out.append(o.symbols(base + done, base + done + TILE, padded=True))
                x, pos = xs, ps
        if fast:
            paths |= unaligned
            done += TILE
            n_fast += 1
            continue
        n_slow += 1
        paths |= EXACT | (TAIL if want < TILE else 0)
        # The exact loop settles what symbol j - 1 owes before it decodes symbol j, from the window only: it stops in front of
        # the first symbol whose predecessor's renormalisation ends behind the window.  Positions only grow: bisect.
        wend = wbase + WINDOW
        fits = lambda j: (o.at(base + done + j)[1] if pending or j else pos) <= wend   # noqa: E731
        got = want
        if not fits(want - 1):
            lo, hi = 0, want - 1                                       # fits(lo - 1) holds or lo == 0; fits(hi) fails
            while lo < hi:
                mid = (lo + hi) // 2
                lo, hi = (mid + 1, hi) if fits(mid) else (lo, mid)
            got = lo
            paths |= STARVED
            pos = wend
        elif pending or want > 1:
            pos = o.at(base + done + want - 1)[1]
        out.append(o.symbols(base + done, base + done + got))
        done += got
        x = o.at(base + done)[0]
        pending = True
    if pending:                                                        # settled behind the loop
        x, pos = o.at(base + n)
    sym = np.concatenate(out) if out else np.zeros(0, np.uint8)
    return dict(paths=paths, fast_tiles=n_fast, slow_tiles=n_slow, symbols=sym, len=pos, state=x)


def path_names(mask):
    return [name for bit, name in PATHS.items() if mask & bit]


# ---- the case list ----

def _damage(kind, rng, data, n, variant):
    """The stream classes 2 .. 11 of test_decoder_fuzz_histogram_tables; returns (stream, symbols to ask for)."""
    data = bytearray(data)
    n_dec = n
    if kind == 2:
        data = data[: int(rng.integers(0, len(data) + 1))]
    elif kind == 3:
        data = data[: max(0, len(data) - int(rng.integers(1, 9000)))]
    elif kind == 4:
        for _ in range(int(rng.integers(1, 6))):
            if data:
                data[max(0, len(data) - 1 - int(rng.integers(0, WINDOW)))] ^= int(rng.integers(1, 256))
    elif kind == 5:
        for _ in range(int(rng.integers(1, 4))):
            if data:
                data[int(rng.integers(0, min(len(data), 64)))] ^= int(rng.integers(1, 256))
    elif kind == 6:
        data = bytearray(rng.integers(0, 256, int(rng.integers(0, 12)), dtype=np.uint8).tobytes())
    elif kind == 7:
        n_dec = n + TILE        # one more tile than was encoded (a random surplus would leave the 3 .. 5 tiles)
    elif kind in (8, 9):
        if variant % 3 == 1:
            data = bytearray(rng.integers(0, 256, int(rng.integers(0, 40)), dtype=np.uint8).tobytes())
        elif variant % 3 == 2:
            data = bytearray(rng.integers(0, 256, int(rng.integers(9000, 30000)), dtype=np.uint8).tobytes())
    elif kind == 10:
        data = bytearray(int(rng.integers(9000, 40000))) + bytearray(rng.integers(0, 256, 5000, dtype=np.uint8).tobytes())
    elif kind == 11:
        data = bytearray(rng.integers(0, 256, max(16, len(data)), dtype=np.uint8).tobytes())
    return bytes(data), n_dec


def _hist_case(rng, kind, variant, n, in_mis, out_mis):
    import oracle
    p0 = (0.2, 0.7, 0.96)[variant % 3]
    alphabet = (256, 17, 3)[(variant // 3 + variant) % 3]
    sym = _symbols(rng, n, p0, alphabet)
    if kind == 8:
        sym[:] = 0
    elif kind == 9:
        sym[:] = int(rng.integers(1, 200))
    hist = np.bincount(sym, minlength=256).astype(np.uint32)
    good = oracle.rans_encode(sym, oracle.FrequencyTable(hist))
    data, n_dec = _damage(kind, rng, good, n, variant)
    return Case(HIST_CLASSES[kind], data, n_dec, in_mis, out_mis, hist=hist)


def _caller_table(rng, kind):
    """The table classes of test_decoder_fuzz_caller_tables"""
    freq = rng.integers(1, 64, 256).astype(np.uint16)
    cum = np.minimum(np.cumsum(np.concatenate([[0], freq[:-1]])), 65535).astype(np.uint16)
    if kind == 1:
        cum = rng.integers(0, 4200, 256).astype(np.uint16)
    elif kind == 2:
        k = int(rng.integers(0, 256))
        freq[k] = int(rng.integers(4097, 65535)); cum[k] = int(rng.integers(0, 4000))
    elif kind == 3:
        k = int(rng.integers(0, 128))
        freq[k] = 4096; cum[k] = int(rng.integers(0, 300))
    return cum, freq


def _n_for(i):
    """3 to 5 tiles: whole tiles, or 3 or 4 tiles and one of the tails"""
    if i % 3 == 0:
        return (3 + i // 3 % 3) * TILE
    return (3 + i // 3 % 2) * TILE + TAILS[i // 2 % len(TAILS)]


def _resume_cases(rng):
    """Chains that take over an oracle decoder object after n1 symbols: every residue of pos0 mod 4 against every stream
    misalignment, the start of the stream on a stream misaligned by 3, the dry stream, the last window."""
    import oracle
    out = []

    def stream(n, p0, alphabet):
        sym = _symbols(rng, n, p0, alphabet)
        hist = np.bincount(sym, minlength=256).astype(np.uint32)
        return hist, oracle.rans_encode(sym, oracle.FrequencyTable(hist))

    # one long intact stream; n1 searched upwards until pos0 has the residue
    n = 5 * TILE + 65
    hist, data = stream(n, 0.2, 256)
    probe = Case("resume", data, 0, 0, 0, hist=hist)
    n1 = 700
    for in_mis in range(4):
        for residue in range(4):
            n1 += 97
            while oracle_of(probe).at(n1)[1] % 4 != residue:
                n1 += 1
            n2 = (3 * TILE, 3 * TILE + 63, 3 * TILE + 4095, 4 * TILE)[(in_mis + residue) % 4]
            out.append(Case("resume", data, min(n2, n - n1), in_mis, (in_mis + residue) % 4, hist=hist, n1=n1, note=f"pos0 % 4 == {residue}"))
    # pos0 of 4 and of 4 or 5 on a stream misaligned by 3
    for n1 in (0, 1):
        out.append(Case("resume", data, 3 * TILE + 1, 3, n1, hist=hist, n1=n1, note="at the head"))
    # inside the last window of an intact stream, and of a long one that is cut: the speculative tile kept and dropped
    hist2, data2 = stream(5 * TILE, 0.2, 17)
    cut = data2[: len(data2) * 4 // 5]
    for k, (d, cls_note) in enumerate(((data2, "last window"), (cut, "last window, cut"), (data2, "last window"), (cut, "last window, cut"))):
        probe = Case("resume", d, 0, 0, 0, hist=hist2)
        n1 = 300 + 50 * k
        while oracle_of(probe).at(n1)[1] <= len(d) - WINDOW + 2000 * (k // 2):
            n1 += 64
        out.append(Case("resume", d, 3 * TILE + (0, 64)[k % 2], k, 3 - k, hist=hist2, n1=n1, note=cls_note))
    # pos0 == len: the object has run its stream dry (a cut stream; a stream of a few bytes)
    for k, d in enumerate((cut, data2[:9000], data2[:7], data2[:4])):
        probe = Case("resume", d, 0, 0, 0, hist=hist2)
        n1 = 0
        while oracle_of(probe).at(n1)[1] < len(d):
            n1 += 512
        out.append(Case("resume", d, 3 * TILE + (0, 1, 65, 4095)[k], (k + 1) % 4, (k + 2) % 4, hist=hist2, n1=n1 + k, note="pos0 == len"))
    # an exact-only table and a constant channel picked up in mid-stream
    cum, freq = _caller_table(rng, 2)
    out.append(Case("resume", rng.integers(0, 256, 12000, dtype=np.uint8).tobytes(), 3 * TILE + 63, 1, 2, cum=cum, freq=freq, n1=777,
                    note="frequency above 4096"))
    sym = np.full(4 * TILE, 9, np.uint8)
    hist3 = np.bincount(sym, minlength=256).astype(np.uint32)
    out.append(Case("resume", rng.integers(0, 256, 20000, dtype=np.uint8).tobytes(), 3 * TILE, 2, 1, hist=hist3, n1=4097,
                    note="single-symbol channel"))
    return out


def _small_head_cases(rng):
    """Streams whose head is below 2^23 and that go on: the first tile is refused and runs the exact loop, and what its last
    symbol owes is settled in front of the second tile -- or cannot be, where the stream ends inside those bytes."""
    import oracle
    out = []
    k = 0
    while len(out) < 8:
        n = (3 + k % 2) * TILE + (0, 65)[k // 2 % 2]
        sym = _symbols(rng, n, 0.2, 256)
        hist = np.bincount(sym, minlength=256).astype(np.uint32)
        data = bytearray(oracle.rans_encode(sym, oracle.FrequencyTable(hist)))
        data[0], data[1] = 0, int(rng.integers(0, 0x80))
        k += 1
        if len(out) % 2 == 0:
            out.append(Case("small head", bytes(data), n, k % 4, (k + 1) % 4, hist=hist))
            continue
        o = oracle_of(Case("small head", bytes(data), n, 0, 0, hist=hist))
        before, after = o.at(TILE - 1)[1], o.at(TILE)[1]
        if after - before >= 2:           # symbol 4095 owes two bytes: leave it one
            out.append(Case("small head", bytes(data[: after - 1]), n, k % 4, (k + 2) % 4, hist=hist, note="ends in the owed bytes"))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(20261020)
    out = []
    # the twelve stream classes on histogram tables
    i = 0
    for variant in range(13):
        for kind in range(12):
            if kind == 0:
                n = (3 + variant % 3) * TILE
            elif kind == 1:
                n = (3 + variant % 2) * TILE + (TAILS[variant % 5] if variant < 10 else int(rng.integers(1, TILE)))
            else:
                n = _n_for(i)
            if kind == 7 and n >= 5 * TILE:     # this class asks for one tile more
                n -= TILE
            out.append(_hist_case(rng, kind, variant, n, i % 4, (i // 4 + i) % 4))
            i += 1
    # caller tables on garbage, on a state of exactly 2^23 and nothing behind it, on nothing
    for j in range(32):
        kind = j % 4
        cum, freq = _caller_table(rng, kind)
        data = (rng.integers(0, 256, int(rng.integers(0, 20000)), dtype=np.uint8).tobytes(), rng.integers(0, 256, 18000, dtype=np.uint8).tobytes(),
                b"\x00\x80\x00\x00", b"")[j // 4 % 4]
        out.append(Case(TABLE_CLASSES[kind], data, _n_for(j + 1), j % 4, (j // 4) % 4, cum=cum, freq=freq))
    # the short chains: nothing to decode (a chain that only reports), and one symbol
    sym = _symbols(rng, 3 * TILE, 0.7, 17)
    hist = np.bincount(sym, minlength=256).astype(np.uint32)
    import oracle
    data = oracle.rans_encode(sym, oracle.FrequencyTable(hist))
    out.append(Case("no symbols", data, 0, 1, 2, hist=hist))
    out.append(Case("no symbols", b"", 0, 0, 0, hist=hist))
    out.append(Case("no symbols", data[:3], 0, 3, 1, hist=hist, note="short stream"))
    out.append(Case("one symbol", data, 1, 2, 3, hist=hist))
    out += _resume_cases(rng)
    out += _small_head_cases(rng)
    return tuple(out)
