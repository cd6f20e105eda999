"""The decode fast tile's bit window on the MI355X (alice-codec_amd/csrc/rans_decode_tile.inc: the sentinel-bit window
and its refill), on the cases tests/test_decode_tile_model.py runs on a model of the machine -- here with the hardware's
wait states.  ONE launch of 17 chains: four tables (one byte per symbol: a refill at every second pair end; one symbol of
frequency 4000: refills are rare; frequent symbols of frequency below 16: 16-bit shifts; random) x stream base addresses
misaligned by 0 .. 3 bytes, n = 2 * 4096 + 37 symbols each (two fast tiles and a tail), and one chain whose stream ends
inside the last window, so that one speculative tile is kept and one dropped.  Symbols, RansResult.len, final_state and
the path mask must be the oracle decoder's, byte for byte; the path mask is derived from the oracle's trace by the rules
of the kernel's tile loop (rans.hip, rans_decode_kernel)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_tile_ref as R  # noqa: E402
from decode_tile_ref import KINDS, TILE  # noqa: E402

pytestmark = pytest.mark.gpu

N = 2 * TILE + 37
WIN_BYTES = 33 * 64 * 4
SPEC_KEPT, SPEC_DROPPED, WHOLE, EXACT, TAIL = 4, 8, 2, 32, 128
CUT = TILE + 2000          # the extra chain: the flat stream (one byte per symbol) cut inside the second tile


def _expected_paths(states, marks, n, length, misalign):
    """The tile loop's branches for a fresh decoder of a well-formed stream whose symbol output is dword aligned."""
    paths, done = 0, 0
    pending = False
    while done < n:
        want = min(TILE, n - done)
        x, pos = marks[done]
        assert not (want == TILE and pos >= length), "a dry tile: not one of this file's cases"
        mis = (misalign + pos) & 3
        wbase = pos - mis if pos >= mis else pos & ~3
        whole = length - wbase >= WIN_BYTES and (misalign + wbase) & 3 == 0
        fast = want == TILE and pos < length
        if fast:
            assert not pending and x >= 1 << 23
            # the tile shifts a byte in whenever the state is below 2^23, the decoder only while bytes are left: the tile
            # consumed padding exactly if the decoder was ever left starving inside it
            after = [int(v) for v in states[done + 1: done + TILE]] + [marks[done + TILE][0]]
            if min(after) < 1 << 23:
                paths |= SPEC_DROPPED
                fast = False
            else:
                paths |= WHOLE if whole else SPEC_KEPT
        if not fast:
            paths |= EXACT | (TAIL if want < TILE else 0)
            pending = True
        done += want
    return paths


@pytest.fixture(scope="module")
def launch(gpu_codec):
    import torch
    lib = gpu_codec.load_library()
    chains = []     # (name, cum, freq, data, misalign, reference symbols, (state, len), paths)
    for kind in KINDS:
        cum, freq, _ = R.table(kind)
        c2s = R.cum_to_sym(cum, freq)
        sym, data = R.stream(kind, N + 100)     # a hundred symbols more than are decoded: the final state is not the encoder's first
        cuts = [(len(data), m) for m in range(4)] + ([(CUT, 2)] if kind == "flat" else [])
        for length, m in cuts:
            part = data[:length]
            states, marks = R.trace(part, N, cum, freq, c2s)
            ref = c2s[states & 4095].astype(np.uint8)
            if length == len(data):
                assert np.array_equal(ref, sym[:N])
            chains.append((f"{kind}+{m}" + ("" if length == len(data) else " cut"), cum, freq, part, m, ref, marks[N],
                           _expected_paths(states, marks, N, length, m)))
    k = len(chains)
    assert k == 17
    slot = (max(len(c[3]) for c in chains) + 4 + 511) // 512 * 512
    d_in = torch.zeros(k * slot, dtype=torch.uint8, device="cuda")
    d_out = torch.full((k, (N + 511) // 512 * 512), 0xEE, dtype=torch.uint8, device="cuda")
    assert d_in.data_ptr() % 4 == 0 and d_out.data_ptr() % 4 == 0
    vp = C.c_void_p
    streams, outs, lens = (vp * k)(), (vp * k)(), (C.c_uint64 * k)()
    cums, freqs = np.zeros((k, 256), np.uint16), np.zeros((k, 256), np.uint16)
    for c, (_, cum, freq, data, m, _, _, _) in enumerate(chains):
        at = c * slot + m
        d_in[at: at + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
        streams[c], outs[c], lens[c] = d_in.data_ptr() + at, d_out[c].data_ptr(), len(data)
        cums[c], freqs[c] = cum, freq
    res = np.zeros((k, 4), np.uint32)
    u16p, u32p = C.POINTER(C.c_uint16), C.POINTER(C.c_uint32)
    rc = lib.alice_codec_test_decode_chains(k, streams, lens, cums.ctypes.data_as(u16p), freqs.ctypes.data_as(u16p), outs, N,
                                            res.ctypes.data_as(u32p), None)
    assert rc == 0
    return chains, d_out.cpu().numpy(), res


def test_symbols(launch):
    chains, out, _ = launch
    for c, (name, *_, ref, _, _) in enumerate(chains):
        assert np.array_equal(out[c, :N], ref), (name, int(np.argmax(out[c, :N] != ref)))
        assert (out[c, N:] == 0xEE).all(), name


def test_len_and_final_state(launch):
    chains, _, res = launch
    for c, (name, *_, (state, length), _) in enumerate(chains):
        assert (int(res[c, 0]), int(res[c, 1])) == (length, state), name


def test_path_masks(launch):
    chains, _, res = launch
    for c, (name, *_, paths) in enumerate(chains):
        assert int(res[c, 2]) == paths, (name, hex(int(res[c, 2])), hex(paths))
    regular = [c for c, ch in enumerate(chains) if not ch[0].endswith("cut")]
    assert all(int(res[c, 3]) == 2 and int(res[c, 2]) & (EXACT | TAIL) == EXACT | TAIL for c in regular)   # two fast tiles, then the tail
    assert {int(res[c, 2]) & (WHOLE | SPEC_KEPT) for c in regular} == {SPEC_KEPT, WHOLE | SPEC_KEPT}       # both kinds of window


def test_one_speculative_tile_kept_one_dropped(launch):
    chains, _, res = launch
    (c,) = [c for c, ch in enumerate(chains) if ch[0].endswith("cut")]
    assert int(res[c, 2]) == SPEC_KEPT | SPEC_DROPPED | EXACT | TAIL and int(res[c, 3]) == 1
    assert int(res[c, 0]) == CUT
