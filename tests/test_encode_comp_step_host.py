"""The complement step of the rANS encode chain (alice-codec_amd/csrc/rans.hip, ripple64_comp), modelled instruction by
instruction in 32-bit wrap-around arithmetic and compared with the reference step (src/rans.rs:269-284): for every frequency
of the big class (17..4096) at the edge states and a few hundred random ones, and as a 64-lane ripple with lane-0 carry-in
and block exit against the oracle encoder's state sequence and bytes.  No GPU."""
import numpy as np
import pytest

M32 = np.uint64(0xFFFFFFFF)
L = 1 << 23
X_END = (1 << 31) + (1 << 17)      # states of a clean chain lie in [2^23, 2^31 + 2^17)


def u32(a):
    return np.asarray(a, np.uint64) & M32


def sext(a, bits):
    a = np.asarray(a, np.uint64).astype(np.int64) & ((1 << bits) - 1)
    return a - ((a >> (bits - 1)) << bits)


# ---- the instructions ----

def v_add_u32(a, b):
    return u32(np.asarray(a, np.uint64) + np.asarray(b, np.uint64))


def v_sub_u32(a, b):
    return u32(np.asarray(a, np.uint64) + (np.uint64(1 << 32) - u32(b)))


def v_ashrrev_i32(sh, a):
    return u32((sext(a, 32) >> sh).astype(np.uint64))


def v_min_u32(a, b):
    return np.minimum(u32(a), u32(b))


def v_mul_hi_u32(a, b):
    a, b = u32(a), u32(b)      # 32 x 32 -> high 32, without overflowing 64 bits
    al, ah, bl, bh = a & 0xFFFF, a >> 16, b & 0xFFFF, b >> 16
    mid = ah * bl + ((al * bl) >> 16)
    mid2 = al * bh + (mid & 0xFFFF)
    return u32(ah * bh + (mid >> 16) + (mid2 >> 16))


def v_lshrrev_b32(sh, a):
    return u32(a) >> (np.asarray(sh, np.uint64) & np.uint64(31))


def v_mad_i32_i24(a, b, c):
    """D = sext24(a) * sext24(b) + c, low 32 bits"""
    return u32((sext(a, 24) * sext(b, 24) + u32(c).astype(np.int64)).astype(np.uint64))


# ---- the table entries the kernel derives (make_enc_entry and the encode kernel's LDS rows, rans.hip) ----

def entries(f, cum):
    f, cum = np.asarray(f, np.int64), np.asarray(cum, np.int64)
    assert ((f >= 17) & (f <= 4096)).all()
    lg = np.array([int(v - 1).bit_length() for v in f.reshape(-1)], np.int64).reshape(f.shape)      # ceil(log2 f)
    rcp = np.array([((1 << (31 + int(l))) + int(v) - 1) // int(v) for v, l in zip(f.reshape(-1), lg.reshape(-1))],
                   np.uint64).reshape(f.shape)
    assert (rcp < (1 << 32)).all()
    t = u32(f << 19)
    return dict(T=t, tm1=v_sub_u32(t, 1), tpp=v_sub_u32(t, t >> np.uint64(8)), rcp=rcp, rsh=u32(lg - 1), g=u32(4096 - f),
                C=u32((1 << 31) - 4097 + f + cum))


def v_mad_i64_i32_hi(a, b, c_hi):
    """high dword of sext32(a) * sext32(b) + {c_hi : 0}, a 64-bit sum (Python integers: the product needs 56 bits)"""
    a, b, c_hi = np.broadcast_arrays(sext(a, 32), sext(b, 32), u32(c_hi).astype(np.int64))
    out = [(((int(x) * int(y) + (int(c) << 32)) & 0xFFFFFFFFFFFFFFFF) >> 32) for x, y, c in zip(a.flat, b.flat, c_hi.flat)]
    return np.array(out, np.uint64).reshape(a.shape)


def comp_step(u, e, one_mad=False):
    """the instructions behind the lane hop: u -> (m, qm, z).  w = ashr(u, 8) + T'' is one v_mad_i64_i32 in the kernel (the
    7-slot step, one_mad) and was an arithmetic shift and an add in the 8-slot step the issue describes."""
    if one_mad:
        w = v_mad_i64_i32_hi(u, 1 << 24, e["tpp"])
    else:
        w = v_ashrrev_i32(8, u)
        w = v_add_u32(w, e["tpp"])
    m = v_min_u32(u, w)
    q = v_mul_hi_u32(m, e["rcp"])
    q = v_lshrrev_b32(e["rsh"], q)
    z = v_mad_i32_i24(q, e["g"], m)
    return m, q, z


def reference_step(x, f, cum):
    """src/rans.rs:275-284 for states that need at most one byte: -> (x', emitted, byte)"""
    x, f, cum = np.asarray(x, np.int64), np.asarray(f, np.int64), np.asarray(cum, np.int64)
    emit = x >= (f << 19)
    y = np.where(emit, x >> 8, x)
    assert (y < (f << 19)).all()
    return ((y // f) << 12) + y % f + cum, emit, x & 0xFF


def test_every_big_class_frequency_at_edge_and_random_states():
    rng = np.random.default_rng(20261019)
    f = np.arange(17, 4097, dtype=np.int64)[:, None]
    t = f << 19
    edges = [t - 1, t, t + 1, np.full_like(t, (1 << 31) - 1), np.full_like(t, 1 << 31), np.full_like(t, L),
             np.full_like(t, X_END - 1), np.full_like(t, L + 1), t + 255, t + 256]
    x = np.concatenate(edges + [rng.integers(L, X_END, (len(f), 300))], axis=1)
    assert ((x >= L) & (x < X_END)).all()
    cum = rng.integers(0, 4097 - f, x.shape)
    cum[:, 0], cum[:, 1] = 0, (4096 - f)[:, 0]
    e = entries(np.broadcast_to(f, x.shape), cum)
    u = v_sub_u32(e["tm1"], x)                      # entry conversion
    m, qm, z = comp_step(u, e)
    want, emit, byte = reference_step(x, f, cum)
    assert x.size >= 4080 * 300
    assert np.array_equal(v_sub_u32(e["C"], z), u32(want))          # x' = C - z
    assert np.array_equal(sext(u, 32) < 0, emit)                    # a byte leaves exactly when u wrapped
    assert np.array_equal((~u & np.uint64(0xFF))[emit], u32(byte)[emit])
    assert (m < e["T"]).all() and (qm < (1 << 19)).all()            # what the reciprocal and the 24-bit multiply need
    assert np.array_equal(m, v_sub_u32(e["tm1"], np.where(emit, x >> 8, x)))
    # the one-instruction form of w, for every eighth frequency (it goes through Python integers)
    pick = (slice(None, None, 8), slice(None))
    sub = {k: v[pick] for k, v in e.items()}
    m7, q7, z7 = comp_step(u[pick], sub, one_mad=True)
    assert np.array_equal(m7, m[pick]) and np.array_equal(q7, qm[pick]) and np.array_equal(z7, z[pick])


def ripple64(u0, e):
    """64 steps over all 64 lanes at once, as the wave runs them: v_add_u32_dpp wave_shr:1 leaves lane 0 alone, every other
    lane takes its left neighbour's z (whatever that is at the time) plus its kc; lanes are right after their own step."""
    kc = v_sub_u32(e["tm1"], np.roll(e["C"], 1))            # lane 0's is never used
    rng = np.random.default_rng(5)
    u = rng.integers(0, 1 << 32, 64, dtype=np.uint64)      # registers hold anything on entry
    z = rng.integers(0, 1 << 32, 64, dtype=np.uint64)
    u[0] = u0
    for _ in range(64):
        u[1:] = v_add_u32(z[:-1], kc[1:])
        _, _, z = comp_step(u, e, one_mad=True)
    return u, z


@pytest.mark.parametrize("seed", range(6))
def test_ripple_of_64_lanes_against_the_oracle(oracle_mod, seed):
    o = oracle_mod
    rng = np.random.default_rng(100 + seed)
    # tables whose used symbols are all in the big class; the odd seeds include the extremes 17 and 4079
    if seed % 2:
        hist = np.zeros(256, np.uint32)
        hist[[3, 250]] = [4079, 17]
    else:
        hist = np.zeros(256, np.uint32)
        used = rng.choice(256, 30, replace=False)
        hist[used] = rng.integers(20, 200, 30)
    table = o.FrequencyTable(hist)
    freq, cum = table.freq.astype(np.int64), table.cum_freq.astype(np.int64)
    alphabet = np.flatnonzero((freq >= 17) & (freq <= 4096))      # (a sparse histogram wraps freq[255] above 4096)
    assert len(alphabet) >= 2 and (seed % 2 == 0 or sorted(freq[alphabet]) == [17, 4079])
    prefix = rng.choice(alphabet, int(rng.integers(0, 300)), p=freq[alphabet] / freq[alphabet].sum())
    block = rng.choice(alphabet, 64, p=freq[alphabet] / freq[alphabet].sum())
    enc = o.RansEncoder()
    for s in prefix:
        enc.encode(int(cum[s]), int(freq[s]))
    x0 = enc.state
    states = []
    for s in block:
        enc.encode(int(cum[s]), int(freq[s]))
        states.append(enc.state)
    assert L <= x0 < X_END
    e = entries(freq[block], cum[block])
    u, z = ripple64(v_sub_u32(e["tm1"][0], x0), e)
    after = v_sub_u32(e["C"], z)
    assert np.array_equal(after, np.array(states, np.uint64))                  # every lane's state after its symbol
    before = np.concatenate([[x0], states[:-1]]).astype(np.uint64)
    assert np.array_equal(v_sub_u32(e["tm1"], u), before)                      # ... and before it
    assert int(after[63]) == states[-1]                                        # block exit: x = C[63] - z[63]
    # the bytes, in the order the encoder pushed them (finish() reverses, and appends the state LSB first)
    n_before = len(_pushed(o, prefix, cum, freq))
    pushed = _pushed(o, np.concatenate([prefix, block]), cum, freq)[n_before:]
    emit = sext(u, 32) < 0
    assert bytes((~u & np.uint64(0xFF))[emit].astype(np.uint8)) == pushed


def _pushed(o, symbols, cum, freq):
    enc = o.RansEncoder()
    for s in symbols:
        enc.encode(int(cum[s]), int(freq[s]))
    out = enc.finish()
    return out[::-1][:-4]
