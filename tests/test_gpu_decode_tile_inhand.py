"""The in-hand decode tile (alice-codec_amd/csrc/rans_decode_tile_ih.inc: the next window dword always in an SGPR, the refill
without a lane read, its out-of-line path running on to the odd symbol's lane read) against the shadow tile on the MI355X.

Launch 1: the 228 chains of tests/decode_chain_cases.py in ONE alice_codec_test_decode_chains_ex launch, laid out and launched
by tests/test_gpu_decode_chain_fuzz.py's run A.  Launch 2: fifteen chains of 8192 + 100 symbols (two fast tiles and a tail) --
a uniform 256-symbol table (a refill every second pair), a table whose stream symbols all have frequency 1 (12 bits per
symbol: refills in three consecutive pairs), a two-symbol table (a refill every few hundred symbols) -- each with its stream
starting at dword k of a 256-byte line, k in {0, 31, 32, 62, 63}.  (The kernel bases a tile's window at the decoder's position,
so a tile always enters at dword 0 of its window and crosses a window row every 64 dwords it consumes; entries at the end of a
row are tests/test_decode_tile_inhand_model.py's.)

This process runs both launches with the default tile, a fresh child runs them with ALICE_DEC_TILE set to the other of the two
tiles (two processes with the GPU open at most).  Symbols, len and final state must be the oracle's, the path mask and the tile
counts the model's, and the two processes must agree on every byte of the output buffers and on all six outputs per chain.

Run as a program (the child): python tests/test_gpu_decode_tile_inhand.py OUT.npz"""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (os.path.dirname(os.path.abspath(__file__)), ROOT) if p not in sys.path]   # the child has neither
import decode_chain_cases as D  # noqa: E402
import test_gpu_decode_chain_fuzz as F  # noqa: E402

pytestmark = pytest.mark.gpu

CHILD_TILE = "shadow"        # the default tile is the in-hand tile
TILES = ("default", CHILD_TILE)
N2 = 2 * D.TILE + 100
STARTS = (0, 31, 32, 62, 63)
GUARD = 64


def _tables():
    cum = lambda f: np.concatenate([[0], np.cumsum(f)[:-1]]).astype(np.uint16)
    uniform = np.full(256, 16, np.uint16)
    ones = np.zeros(256, np.uint16)
    ones[:200], ones[255] = 1, 4096 - 200
    two = np.zeros(256, np.uint16)
    two[0], two[1] = 4000, 96
    p_ones = np.where(np.arange(256) < 200, 1.0 / 200, 0.0)
    return (("uniform", cum(uniform), uniform, uniform / 4096), ("frequency 1", cum(ones), ones, p_ones),
            ("two symbols", cum(two), two, two / 4096))


@functools.lru_cache(maxsize=None)
def _cases2():
    from oracle import alice_oracle_np as onp
    out = []
    for t, (name, cum, freq, p) in enumerate(_tables()):
        for k in STARTS:
            sym = np.random.default_rng([26, t, k]).choice(256, N2 + 400, p=p).astype(np.uint8)
            data = onp.rans_encode(sym, [int(v) for v in cum], [int(v) for v in freq])
            out.append((k, D.Case(name, bytes(data), N2, 0, k % 4, cum=cum, freq=freq, note=f"stream at dword {k}")))
    return out


@functools.lru_cache(maxsize=None)
def _layout2():
    in_at, out_at, i, o = [], [], 0, 0
    for k, case in _cases2():
        in_at.append(i + 4 * k)
        i += (4 * k + len(case.data) + 1 + 255) // 256 * 256
        out_at.append(o + GUARD + case.out_mis)
        o += (GUARD + case.out_mis + case.n + GUARD + 15) // 16 * 16
    return in_at, out_at, i + 16, o + 16


def _launch2(lib):
    import torch
    cases = [c for _, c in _cases2()]
    in_at, out_at, in_size, out_size = _layout2()
    k = len(cases)
    h_in = np.zeros(in_size, np.uint8)
    hists, cums, freqs = np.ones((k, 256), np.uint32), np.zeros((k, 256), np.uint16), np.zeros((k, 256), np.uint16)
    from_arrays, zero, own = np.ones(k, np.uint32), np.zeros(k, np.uint32), np.ones(k, np.uint32)
    pos0, lens, ns = (np.zeros(k, np.uint64) for _ in range(3))
    for c, case in enumerate(cases):
        h_in[in_at[c]: in_at[c] + len(case.data)] = np.frombuffer(case.data, np.uint8)
        cums[c], freqs[c], lens[c], ns[c] = case.cum, case.freq, len(case.data), case.n
    d_in = torch.from_numpy(h_in).cuda()
    d_out = torch.full((out_size,), 0xEE, dtype=torch.uint8, device="cuda")
    assert d_in.data_ptr() % 256 == 0 and d_out.data_ptr() % 16 == 0
    vp = C.c_void_p
    streams, outs = (vp * k)(), (vp * k)()
    for c in range(k):
        streams[c], outs[c] = d_in.data_ptr() + in_at[c], d_out.data_ptr() + out_at[c]
    res = np.zeros((k, 6), np.uint32)
    u16p, u32p, u64p = C.POINTER(C.c_uint16), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    p32 = lambda a: a.ctypes.data_as(u32p)   # noqa: E731
    rc = lib.alice_codec_test_decode_chains_ex(k, streams, lens.ctypes.data_as(u64p), outs, ns.ctypes.data_as(u64p), p32(hists),
                                               cums.ctypes.data_as(u16p), freqs.ctypes.data_as(u16p), p32(from_arrays), p32(zero), p32(zero),
                                               pos0.ctypes.data_as(u64p), p32(own), p32(res), None)
    assert rc == 0, rc
    return d_out.cpu().numpy(), res


def _both(lib):
    out1, res1 = F._launch(lib, "A")
    out2, res2 = _launch2(lib)
    return {"out1": out1, "res1": res1, "out2": out2, "res2": res2}


@pytest.fixture(scope="module")
def runs(gpu_codec, tmp_path_factory):
    assert os.environ.get("ALICE_DEC_TILE") is None
    assert len(F._plan("A")) == len(D.cases()) == 228
    mine = _both(gpu_codec.load_library())
    dump = str(tmp_path_factory.mktemp("decode_tile_inhand") / "child.npz")
    flags = ["-s"] if sys.flags.no_user_site else []
    subprocess.run([sys.executable, *flags, os.path.abspath(__file__), dump], env=dict(os.environ, ALICE_DEC_TILE=CHILD_TILE), check=True,
                   timeout=300)
    with np.load(dump) as z:
        theirs = {name: z[name] for name in z.files}
    return {"default": mine, CHILD_TILE: theirs}


@pytest.mark.parametrize("tile", TILES)
def test_symbols_len_and_final_state_are_the_oracles(runs, oracle_mod, tile):
    out, res = runs[tile]["out1"], runs[tile]["res1"]
    out_at = F._layout("A")[1]
    for c, (case, _, _, _) in enumerate(F._plan("A")):
        sym, length, state = F._expected(case)
        got = out[out_at[c]: out_at[c] + case.n]
        assert np.array_equal(got, sym), (tile, F._name("A", c), "first difference at", int(np.argmax(got != sym)))
        assert (int(res[c, 0]), int(res[c, 1])) == (length, state), (tile, F._name("A", c))
        assert int(res[c, 5]) == 0, (tile, F._name("A", c), hex(int(res[c, 5])))


@pytest.mark.parametrize("tile", TILES)
def test_paths_and_tile_counts_are_the_models(runs, oracle_mod, tile):
    res = runs[tile]["res1"]
    full_tiles = 0
    for c, (case, in_mis, out_mis, _) in enumerate(F._plan("A")):
        paths, n_fast, n_slow = F._predicted(case, in_mis, out_mis)
        got = (int(res[c, 2]), int(res[c, 3]), int(res[c, 4]))
        assert got == (paths, n_fast, n_slow), (tile, F._name("A", c), "kernel", D.path_names(got[0]), got[1:], "model", D.path_names(paths),
                                                (n_fast, n_slow))
        full_tiles += n_fast
    assert full_tiles >= 100


@pytest.mark.parametrize("tile", TILES)
def test_long_chains_at_every_start_are_the_oracles(runs, oracle_mod, tile):
    out, res = runs[tile]["out2"], runs[tile]["res2"]
    out_at = _layout2()[1]
    inside = np.zeros(out.size, bool)
    for c, (k, case) in enumerate(_cases2()):
        sym, length, state = D.expected(case)
        got = out[out_at[c]: out_at[c] + case.n]
        assert np.array_equal(got, sym), (tile, str(case), "first difference at", int(np.argmax(got != sym)))
        assert (int(res[c, 0]), int(res[c, 1]), int(res[c, 5])) == (length, state, 0), (tile, str(case))
        p = D.predict(case, 0, case.out_mis)
        assert (p["fast_tiles"], p["slow_tiles"]) == (2, 1)                              # two fast tiles and the tail
        assert (int(res[c, 2]), int(res[c, 3]), int(res[c, 4])) == (p["paths"], 2, 1), (tile, str(case), D.path_names(int(res[c, 2])))
        inside[out_at[c]: out_at[c] + case.n] = True
    assert (out[~inside] == 0xEE).all()


def test_the_streams_refill_as_often_as_they_should():
    """bits per symbol of the three tables: 8 (a refill every second pair), 12 (three pairs of four) and well under 1"""
    per = {case.cls: 8 * len(case.data) / (N2 + 400) for _, case in _cases2()}
    assert 7.9 < per["uniform"] < 8.1 and 11.9 < per["frequency 1"] < 12.1 and 0.05 < per["two symbols"] < 0.4, per


def test_both_tiles_give_the_same_bytes(runs):
    mine, theirs = runs["default"], runs[CHILD_TILE]
    for j, name in enumerate(F.OUTPUTS):
        for key in ("res1", "res2"):
            bad = np.flatnonzero(mine[key][:, j] != theirs[key][:, j])
            assert bad.size == 0, (key, name, int(bad[0]))
    assert np.array_equal(mine["out1"], theirs["out1"]) and np.array_equal(mine["out2"], theirs["out2"])   # guards and gaps included


if __name__ == "__main__":
    import alice_codec_amd
    assert alice_codec_amd.device_count() >= 1
    alice_codec_amd.set_device(0)
    np.savez(sys.argv[1], **_both(alice_codec_amd.load_library()))
