"""The vector decode tile (alice-codec_amd/csrc/rans_decode_tile_vec.inc: the state update on the vector side, one lane read
per symbol) on the MI355X, through the stage-level device decode that tests/test_gpu_decode_window.py uses.  ONE launch of
32 chains: two lengths (4096 symbols: exactly one fast tile; 8192 + 100: two tiles and an exact tail) x four tables x
stream base addresses misaligned by 0 .. 3 bytes.  The tables: 256 equal symbols (one byte per symbol, a refill almost
every pair); one symbol at 4095/4096 (rare refills); rare symbols of frequency 1 (16-bit shifts); a single symbol of
frequency 4096 (F' = 2^32 - 1, the state never moves).  Symbols, RansResult.len and final_state must be the oracle
decoder's, and every full tile must have run on the fast path.  A second run in a fresh child process with
ALICE_DEC_TILE=classic must give the same bytes and the same RansResult.paths.

Run as a program (the child): python tests/test_gpu_decode_tile_vec.py OUT.npz"""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (os.path.dirname(os.path.abspath(__file__)), ROOT) if p not in sys.path]   # the child has neither
import decode_tile_ref as R  # noqa: E402
from decode_tile_ref import TILE  # noqa: E402

pytestmark = pytest.mark.gpu

LENGTHS = (TILE, 2 * TILE + 100)
TABLES = ("equal", "peaked", "rare1", "single")
SPARE = 100     # symbols encoded behind the decoded ones: the final state is not the encoder's first, the stream does not end


def _table(name):
    """(cum, freq, probabilities the stream's symbols are drawn with)"""
    freq = np.zeros(256, np.int64)
    if name == "equal":
        freq[:] = 16
        p = freq / 4096
    elif name == "peaked":          # the rare symbol is drawn more often than its frequency says, so that the stream has bytes
        freq[9], freq[200] = 4095, 1
        p = np.zeros(256)
        p[9], p[200] = 0.98, 0.02
    elif name == "rare1":           # 16 symbols of frequency 1: a 16-bit shift behind each of them
        freq[:16] = 1
        freq[16:] = 17
        p = np.where(np.arange(256) < 16, 0.004, 0.0)
        p[16:] = (1 - p.sum()) / 240
    else:
        freq[5] = 4096
        p = freq / 4096
    assert freq.sum() == 4096
    cum = np.concatenate([[0], np.cumsum(freq)[:-1]])
    return [int(v) for v in cum], [int(v) for v in freq], p


@functools.lru_cache(maxsize=None)
def _cases():
    """(name, cum, freq, stream, n, reference symbols, (final state, len)) per table and length, from the oracle."""
    from oracle import alice_oracle_np as onp
    cases = []
    for ti, name in enumerate(TABLES):
        cum, freq, p = _table(name)
        c2s = R.cum_to_sym(cum, freq)
        for n in LENGTHS:
            if name == "single":    # nothing to encode: the state's four bytes, and bytes behind them that no decoder reads
                data = (1 << 23).to_bytes(4, "big") + np.random.default_rng(n).integers(0, 256, 600, dtype=np.uint8).tobytes()
                sym = np.full(n + SPARE, 5, np.uint8)
            else:
                sym = np.random.default_rng([ti, n]).choice(256, n + SPARE, p=p).astype(np.uint8)
                data = onp.rans_encode(sym, cum, freq)
            states, marks = R.trace(data, n, cum, freq, c2s)
            ref = np.asarray(onp.rans_decode(data, n, cum, freq, [int(v) for v in c2s]), np.uint8)
            assert np.array_equal(ref, sym[:n]) and np.array_equal(c2s[states & 4095], ref)
            assert marks[n][1] < len(data)          # every full tile starts with stream left: the fast tile, not the dry one
            if name == "rare1":
                assert np.count_nonzero(ref < 16) >= 10
            cases.append((f"{name}/{n}", cum, freq, bytes(data), n, ref, marks[n]))
    return cases


def _launch(lib):
    import torch
    chains = [(f"{name}+{m}", cum, freq, data, n, m) for name, cum, freq, data, n, _, _ in _cases() for m in range(4)]
    k = len(chains)
    assert k == 32
    slot = (max(len(c[3]) for c in chains) + 4 + 511) // 512 * 512
    width = (max(LENGTHS) + 511) // 512 * 512
    d_in = torch.zeros(k * slot, dtype=torch.uint8, device="cuda")
    d_out = torch.full((k, width), 0xEE, dtype=torch.uint8, device="cuda")
    assert d_in.data_ptr() % 4 == 0 and d_out.data_ptr() % 4 == 0
    vp = C.c_void_p
    u16p, u32p = C.POINTER(C.c_uint16), C.POINTER(C.c_uint32)
    streams, outs, lens, ns = (vp * k)(), (vp * k)(), (C.c_uint64 * k)(), (C.c_uint64 * k)()
    cums, freqs = np.zeros((k, 256), np.uint16), np.zeros((k, 256), np.uint16)
    for c, (_, cum, freq, data, n, m) in enumerate(chains):
        at = c * slot + m
        d_in[at: at + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
        streams[c], outs[c], lens[c], ns[c] = d_in.data_ptr() + at, d_out[c].data_ptr(), len(data), n
        cums[c], freqs[c] = cum, freq
    res = np.zeros((k, 4), np.uint32)
    rc = lib.alice_codec_test_decode_chains_n(k, streams, lens, cums.ctypes.data_as(u16p), freqs.ctypes.data_as(u16p), outs, ns,
                                              res.ctypes.data_as(u32p), None)
    assert rc == 0
    return [c[0] for c in chains], d_out.cpu().numpy(), res


@pytest.fixture(scope="module")
def launch(gpu_codec):
    return _launch(gpu_codec.load_library())


def test_symbols_len_and_final_state(launch):
    names, out, res = launch
    for c, name in enumerate(names):
        _, _, _, _, n, ref, (state, length) = _cases()[c // 4]
        assert np.array_equal(out[c, :n], ref), (name, int(np.argmax(out[c, :n] != ref)))
        assert (out[c, n:] == 0xEE).all(), name
        assert (int(res[c, 0]), int(res[c, 1])) == (length, state), name


def test_every_full_tile_ran_fast(launch):
    names, _, res = launch
    for c, name in enumerate(names):
        n = _cases()[c // 4][4]
        assert int(res[c, 3]) == n // TILE, (name, int(res[c, 3]), hex(int(res[c, 2])))


def test_classic_tile_gives_the_same_bytes(launch, tmp_path):
    names, out, res = launch
    dump = str(tmp_path / "classic.npz")
    env = dict(os.environ, ALICE_DEC_TILE="classic")
    flags = ["-s"] if sys.flags.no_user_site else []
    subprocess.run([sys.executable, *flags, os.path.abspath(__file__), dump], env=env, check=True, timeout=300)
    with np.load(dump) as z:
        assert np.array_equal(z["out"], out)
        assert np.array_equal(z["res"][:, :3], res[:, :3]) and np.array_equal(z["res"][:, 3], res[:, 3])   # len, state, paths, fast tiles


if __name__ == "__main__":
    import alice_codec_amd
    assert alice_codec_amd.device_count() >= 1
    alice_codec_amd.set_device(0)
    _, child_out, child_res = _launch(alice_codec_amd.load_library())
    np.savez(sys.argv[1], out=child_out, res=child_res)
