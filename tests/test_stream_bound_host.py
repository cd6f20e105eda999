"""alice_codec_rans_stream_bound(hist, n) promises the capacity alice_codec_dev_rans_encode needs: the stream of n symbols
with that histogram (the oracle's RansEncoder, src/rans.rs:269-308) plus the 64 dummy-store bytes the encode chain keeps
free at the front of its region -- the kernel writes a stream of len bytes into any region of len + 64 or more
(tests/test_gpu_encoder_fuzz.py pins that edge on the device).  Host only: the bound is arithmetic on the histogram."""
import ctypes as C

import numpy as np
import pytest

U32P = C.POINTER(C.c_uint32)


def _draw(rng, n, p):
    p = np.asarray(p, np.float64)
    return rng.choice(256, n, p=p / p.sum()).astype(np.uint8)


def _families(rng, n):
    """(name, draw): draw() gives n fresh symbols of the family"""
    ranks = np.arange(1, 257, dtype=np.float64)
    yield "flat", lambda: _draw(rng, n, np.ones(256))
    for e in (0.5, 1.0, 2.0, 3.0):
        yield f"power law {e}", lambda e=e: _draw(rng, n, ranks ** -e)
        yield f"power law {e}, shuffled alphabet", lambda e=e: _draw(rng, n, rng.permutation(ranks ** -e))

    def rare():
        sym = np.zeros(n, np.uint8)
        sym[int(rng.integers(0, n))] = int(rng.integers(1, 256))
        return sym
    yield "one dominant symbol plus a rare one", rare

    def sparse():
        live = rng.choice(256, int(rng.integers(2, 12)), replace=False)
        p = np.zeros(256)
        p[live] = rng.random(len(live)) + 0.01
        return _draw(rng, n, p)
    yield "sparse random", sparse
    heavy = ranks ** -1.5
    heavy[0] = heavy.sum() * 4
    yield "symbol 0 heavy, sorted data", lambda: np.sort(_draw(rng, n, heavy))
    last = np.full(256, 0.02 / 255)
    last[255] = 0.98
    yield "255 dominant", lambda: _draw(rng, n, last)

    def lopsided():
        p = np.zeros(256)
        p[0], p[int(rng.integers(1, 256))] = 4000.0, 1.0
        return _draw(rng, n, p)
    yield "one symbol at 4000:1", lopsided


def _assert_bound(lib, oracle_mod, name, sym):
    n = len(sym)
    hist = np.bincount(sym, minlength=256).astype(np.uint32)
    table = oracle_mod.FrequencyTable(hist)
    if (table.freq[hist > 0] == 0).any():
        return False       # the correction wrapped the frequency of a 255 that occurs to 0: no stream exists (ReferenceDiverges)
    stream = oracle_mod.rans_encode(sym, table)
    bound = int(lib.alice_codec_rans_stream_bound(hist.ctypes.data_as(U32P), n))
    worst = int(lib.alice_codec_rans_stream_bound(None, n))
    assert bound >= len(stream) + 64, (name, n, bound, len(stream))
    assert bound <= worst, (name, n, bound, worst)
    assert worst >= 2 * n + 4 + 64        # two bytes per symbol is the format's worst case, plus the state and the band
    return True


@pytest.mark.parametrize("n", [1, 2, 17, 99, 1000, 4096, 30011, 200000])
def test_stream_bound_covers_the_oracles_stream(codec, oracle_mod, n):
    lib = codec.load_library()
    rng = np.random.default_rng(1000 + n)
    names = []
    for name, draw in _families(rng, n):
        # a draw in which a 255 occurs and the table's correction takes its frequency to exactly 0 has no stream: draw again
        assert any(_assert_bound(lib, oracle_mod, name, draw()) for _ in range(8)), (name, n, "no draw of this family has a stream")
        names.append(name)
    assert len(names) == 14


def test_stream_bound_at_a_few_million_symbols(codec, oracle_mod):
    lib = codec.load_library()
    rng = np.random.default_rng(5)
    ranks = np.arange(1, 257, dtype=np.float64)
    for name, p in (("flat", np.ones(256)), ("power law 1.5", ranks ** -1.5)):
        assert _assert_bound(lib, oracle_mod, name, _draw(rng, 3_000_000, p))
