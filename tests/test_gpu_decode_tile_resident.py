"""The resident decode tile (alice-codec_amd/csrc/rans_decode_tile_rs.inc: one statement decodes a run of full tiles, the
tables stay in their registers, the window rows come straight from global memory, a tile's symbols are recovered while the next
tile's window loads fly) against the in-hand tile on the MI355X.

Launch 1: the 228 chains of tests/decode_chain_cases.py in ONE alice_codec_test_decode_chains_ex launch, laid out and launched
by tests/test_gpu_decode_chain_fuzz.py's run A.  Launch 2: 29 chains over four tables -- uniform (a byte per symbol),
frequency 1 (12 bits per symbol: the window base moves 6 KB per tile), two symbols (a few dozen bytes per tile: every
pos & 3 at a tile start) and one symbol of frequency 4096 (nothing is consumed) -- of 4096, 2 * 4096 and 3 * 4096 + 100 symbols,
the longest also with the stream at dword 31 and 63 of a 256-byte line; per table one chain whose output is off a dword by one
byte (the statement is not entered: same bytes through the old path) and one resumed decoder object; and one uniform chain
whose stream ends too early for the second tile's window to be whole.  Every other stream carries kDecWinBytes of bytes behind
what its decoder reads, so that every full tile has a whole window and the statement runs on from tile to tile.

This process runs both launches with the default tile (the resident tile), a fresh child runs them with
ALICE_DEC_TILE=inhand.  Symbols, len and final state must be the oracle's, the path mask and the tile counts the model's
(decode_chain_cases.predict: the resident statement takes exactly the tiles the kernel's fast `whole` path takes), the 64
guard bytes around every output untouched, and the two processes must agree on every byte of the output buffers and on all
six outputs per chain.

Run as a program (a child): python tests/test_gpu_decode_tile_resident.py OUT.npz"""
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

CHILD_TILES = ("inhand",)      # the default tile is the resident tile
TILES = ("default",) + CHILD_TILES
SHAPES = (D.TILE, 2 * D.TILE, 3 * D.TILE + 100)
STARTS = (0, 31, 63)
GUARD = 64


def _tables():
    cum = lambda f: np.concatenate([[0], np.cumsum(f)[:-1]]).astype(np.uint16)
    uniform = np.full(256, 16, np.uint16)
    ones = np.zeros(256, np.uint16)
    ones[:200], ones[255] = 1, 4096 - 200
    two = np.zeros(256, np.uint16)
    two[0], two[1] = 4000, 96
    big = np.zeros(256, np.uint16)
    big[5] = 4096
    p_ones = np.where(np.arange(256) < 200, 1.0 / 200, 0.0)
    return (("uniform", cum(uniform), uniform, uniform / 4096), ("frequency 1", cum(ones), ones, p_ones),
            ("two symbols", cum(two), two, two / 4096), ("frequency 4096", cum(big), big, big / 4096))


@functools.lru_cache(maxsize=None)
def _cases2():
    """[(start dword, Case)]"""
    from oracle import alice_oracle_np as onp
    out = []

    def add(t, n, k, out_mis=0, n1=None, spare=True, note=""):
        name, cum, freq, p = _tables()[t]
        rng = np.random.default_rng([30, t, n, k, out_mis, n1 or 0])
        total = n + (n1 or 0) + 400
        if name == "frequency 4096":
            data = (D.RANS_L + 77).to_bytes(4, "big")     # the state never moves
        else:
            sym = rng.choice(256, total, p=p).astype(np.uint8)
            data = bytes(onp.rans_encode(sym, [int(v) for v in cum], [int(v) for v in freq]))
        if spare:
            data += rng.integers(0, 256, D.WINDOW, dtype=np.uint8).tobytes()   # never read as stream: whole windows to the last tile
        out.append((k, D.Case(name, data, n, 0, out_mis, cum=cum, freq=freq, n1=n1, note=note or f"stream at dword {k}")))

    for t in range(4):
        for n in SHAPES:
            add(t, n, 0)
        for k in STARTS[1:]:
            add(t, SHAPES[2], k)
        add(t, SHAPES[1], 0, out_mis=1, note="output off a dword")
        add(t, SHAPES[1], 0, n1=100, note="resumed")
    add(0, SHAPES[1], 0, spare=False, note="second window not whole")
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
    from_arrays, own = np.ones(k, np.uint32), np.ones(k, np.uint32)
    resume, x0 = np.zeros(k, np.uint32), np.zeros(k, np.uint32)
    pos0, lens, ns = (np.zeros(k, np.uint64) for _ in range(3))
    for c, case in enumerate(cases):
        h_in[in_at[c]: in_at[c] + len(case.data)] = np.frombuffer(case.data, np.uint8)
        cums[c], freqs[c], lens[c], ns[c] = case.cum, case.freq, len(case.data), case.n
        resume[c], x0[c], pos0[c] = D.start_of(case)
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
                                               cums.ctypes.data_as(u16p), freqs.ctypes.data_as(u16p), p32(from_arrays), p32(resume), p32(x0),
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
    assert len(F._plan("A")) == len(D.cases()) == 228 and len(_cases2()) <= 48
    got = {"default": _both(gpu_codec.load_library())}
    flags = ["-s"] if sys.flags.no_user_site else []
    for tile in CHILD_TILES:                                  # two processes with the GPU open at most
        dump = str(tmp_path_factory.mktemp("decode_tile_resident") / f"{tile}.npz")
        subprocess.run([sys.executable, *flags, os.path.abspath(__file__), dump], env=dict(os.environ, ALICE_DEC_TILE=tile), check=True,
                       timeout=300)
        with np.load(dump) as z:
            got[tile] = {name: z[name] for name in z.files}
    return got


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
    for c, (case, in_mis, out_mis, _) in enumerate(F._plan("A")):
        paths, n_fast, n_slow = F._predicted(case, in_mis, out_mis)
        got = (int(res[c, 2]), int(res[c, 3]), int(res[c, 4]))
        assert got == (paths, n_fast, n_slow), (tile, F._name("A", c), "kernel", D.path_names(got[0]), got[1:], "model", D.path_names(paths),
                                                (n_fast, n_slow))


@pytest.mark.parametrize("tile", TILES)
def test_runs_of_tiles_are_the_oracles_and_the_models(runs, oracle_mod, tile):
    out, res = runs[tile]["out2"], runs[tile]["res2"]
    out_at = _layout2()[1]
    inside = np.zeros(out.size, bool)
    whole_runs = 0
    for c, (k, case) in enumerate(_cases2()):
        sym, length, state = D.expected(case)
        got = out[out_at[c]: out_at[c] + case.n]
        assert np.array_equal(got, sym), (tile, str(case), "first difference at", int(np.argmax(got != sym)))
        assert (int(res[c, 0]), int(res[c, 1]), int(res[c, 5])) == (length, state, 0), (tile, str(case))
        p = D.predict(case, case.in_mis, case.out_mis)
        assert (int(res[c, 2]), int(res[c, 3]), int(res[c, 4])) == (p["paths"], p["fast_tiles"], p["slow_tiles"]), \
            (tile, str(case), D.path_names(int(res[c, 2])), D.path_names(p["paths"]))
        assert p["fast_tiles"] == case.n // D.TILE             # every full tile is a fast tile ...
        if case.note == "second window not whole":
            assert p["paths"] & D.SPEC_KEPT and p["paths"] & D.WHOLE
        else:
            assert not p["paths"] & (D.SPEC_KEPT | D.SPEC_DROPPED | D.DRY)   # ... on a whole window
            whole_runs += case.out_mis == 0 and case.n >= 2 * D.TILE
        assert bool(p["paths"] & D.UNALIGNED) == (case.out_mis != 0)
        inside[out_at[c]: out_at[c] + case.n] = True
    assert whole_runs >= 20                                    # chains whose statement runs over two or three tiles
    assert (out[~inside] == 0xEE).all()                        # the guard bytes around every output


def test_the_window_base_moves_as_it_should():
    per = {case.cls: 8 * (len(case.data) - D.WINDOW) / (case.n + 400) for _, case in _cases2() if case.n == SHAPES[2] and case.cls != "frequency 4096"}
    assert 7.9 < per["uniform"] < 8.1 and 11.9 < per["frequency 1"] < 12.1 and 0.05 < per["two symbols"] < 0.4, per


def test_all_tiles_give_the_same_bytes(runs):
    mine = runs["default"]
    for tile in CHILD_TILES:
        theirs = runs[tile]
        for j, name in enumerate(F.OUTPUTS):
            for key in ("res1", "res2"):
                bad = np.flatnonzero(mine[key][:, j] != theirs[key][:, j])
                assert bad.size == 0, (tile, key, name, int(bad[0]))
        assert np.array_equal(mine["out1"], theirs["out1"]) and np.array_equal(mine["out2"], theirs["out2"])   # guards and gaps included


if __name__ == "__main__":
    import alice_codec_amd
    assert alice_codec_amd.device_count() >= 1
    alice_codec_amd.set_device(0)
    np.savez(sys.argv[1], **_both(alice_codec_amd.load_library()))
