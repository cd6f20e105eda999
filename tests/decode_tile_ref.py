"""Tables, streams and the written-down oracle decoder shared by tests/test_decode_tile_model.py (the generated decode tile
on a model of the machine) and tests/test_gpu_decode_window.py (the same cases on the GPU).  TEST INFRASTRUCTURE ONLY."""
import numpy as np

from oracle import alice_oracle_np as onp

M32 = 0xFFFFFFFF
TILE = 4096
KINDS = ("flat", "peaked", "sparse", "random")


def table(kind):
    """(cum[256], freq[256], symbol probabilities of the stream) of a well-formed table: the frequencies sum to 4096."""
    rng = np.random.default_rng(KINDS.index(kind) + 20261018)
    if kind == "flat":                 # one byte per symbol: a refill at every second pair end
        freq = np.full(256, 16)
        p = freq / 4096
    elif kind == "peaked":             # one symbol of frequency 4000: refills are rare, the window stays as full as the last one left it
        freq = np.zeros(256, np.int64)
        freq[7] = 4000
        freq[100:196] = 1
        p = freq / 4096
    elif kind == "sparse":             # the stream's frequent symbols have frequency below 16: 16-bit shifts, 24 bits in a pair
        freq = np.zeros(256, np.int64)
        freq[:200] = rng.integers(1, 4, 200)
        rest = 4096 - int(freq.sum())
        freq[200:] = rest // 56
        freq[255] += rest - int(freq[200:].sum())
        p = np.where(np.arange(256) < 200, 1.0, 0.02)
        p = p / p.sum()
    else:
        w = rng.random(256) ** 3 + 1e-3
        freq = np.maximum((w / w.sum() * 3800).astype(np.int64), 1)
        freq[int(np.argmax(freq))] += 4096 - int(freq.sum())
        p = freq / 4096
    assert freq.sum() == 4096 and freq.min() >= 0 and freq.max() < 4096
    cum = np.concatenate([[0], np.cumsum(freq)[:-1]])
    return [int(v) for v in cum], [int(v) for v in freq], p


def cum_to_sym(cum, freq):
    """As the reference fills it (src/rans.rs:135-144)."""
    c2s = np.zeros(4096, np.int64)
    for s in range(256):
        c2s[cum[s]: min(cum[s] + freq[s], 4096)] = s
    return c2s


def stream(kind, n_symbols, seed=0):
    """(symbols, stream bytes) of n_symbols symbols drawn for this table and encoded by the numpy oracle."""
    cum, freq, p = table(kind)
    sym = np.random.default_rng([KINDS.index(kind), seed, n_symbols]).choice(256, n_symbols, p=p)
    return sym.astype(np.uint8), onp.rans_encode(sym, cum, freq)


def trace(data, n, cum, freq, c2s, every=TILE):
    """The oracle's decoder (oracle/alice_oracle_np.py: rans_decode, src/rans.rs:330-381) with its states written down:
    (pre-update state of every symbol, {i: (state, position) before symbol i, for i % every == 0 and i = n})."""
    data = bytes(data)
    x, pos = 0, 0
    if len(data) >= 4:
        x, pos = int.from_bytes(data[:4], "big"), 4
    states, marks = [], {}
    for i in range(n):
        if i % every == 0:
            marks[i] = (x, pos)
        states.append(x)
        slot = x & 4095
        s = int(c2s[slot])
        x = (freq[s] * (x >> 12) + slot - cum[s]) & M32
        while x < (1 << 23) and pos < len(data):
            x = ((x << 8) | data[pos]) & M32
            pos += 1
    marks[n] = (x, pos)
    return np.array(states, np.int64), marks
