"""Randomised parity of the rANS decode chain kernel (alice-codec_amd/csrc/rans.hip, rans_decode_kernel + the generated
tile) against the oracle's RansDecoder (reference behaviour: src/rans.rs:330-371), aimed at the transitions between the
kernel's tile paths: whole-window fast tiles, speculative tiles on the zero-padded last window (kept and dropped), the
dry-stream tile, the exact scalar-lane loop (tail tiles, starved states, tables the packed entries cannot express) and
unaligned buffers.  Every case has at least three 4096-symbol tiles.  The path mask the kernel reports
(alice_codec_test_last_decode_stats) must show that every branch ran at least once."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rans_tables import custom_oracle_table as _custom_oracle_table  # noqa: E402

pytestmark = pytest.mark.gpu

PATHS = {1: "dry", 2: "whole-window fast", 4: "speculative kept", 8: "speculative dropped", 16: "pending fed", 32: "exact loop",
         64: "exact loop starved at window end", 128: "tail tile", 256: "unaligned output", 512: "state below L",
         1024: "still starved"}


def _stats(codec):
    out = (C.c_uint32 * 4)()
    codec.load_library().alice_codec_test_last_decode_stats(out)
    return list(out)


def _symbols(rng, n, p0, alphabet):
    s = rng.integers(1, alphabet, n)
    return (s * (rng.random(n) >= p0)).astype(np.uint8)


def test_decoder_fuzz_histogram_tables(gpu_codec, oracle_mod):
    rng = np.random.default_rng(20261005)
    seen = 0
    n_cases = 0
    for i in range(336):
        kind = i % 12
        n = int(rng.integers(3 * 4096, 6 * 4096))
        if kind in (0, 1):
            n = (n // 4096) * 4096 + (0 if kind == 0 else int(rng.integers(1, 4096)))
        p0 = float(rng.choice([0.2, 0.7, 0.96]))
        alphabet = int(rng.choice([3, 17, 256]))
        sym = _symbols(rng, n, p0, alphabet)
        if kind == 8:      # all-zero channel: symbol 0 gets frequency 4096 and owns every slot
            sym[:] = 0
        elif kind == 9:    # one symbol s > 0: frequency 4096 at cum = s, slots below s belong to frequency-1 symbols
            sym[:] = int(rng.integers(1, 200))
        hist = np.bincount(sym, minlength=256).astype(np.uint32)
        tg, to = gpu_codec.FrequencyTable.from_histogram(hist), oracle_mod.FrequencyTable(hist)
        good = oracle_mod.rans_encode(sym, to)
        data = bytearray(good)
        n_dec = n
        if kind == 2:      # truncated somewhere
            data = data[: int(rng.integers(0, len(data) + 1))]
        elif kind == 3:    # truncated inside the last window
            data = data[: max(0, len(data) - int(rng.integers(1, 9000)))]
        elif kind == 4:    # corruption inside the last window: the decoder desynchronises near the end
            for _ in range(int(rng.integers(1, 6))):
                if data:
                    data[max(0, len(data) - 1 - int(rng.integers(0, 8448)))] ^= int(rng.integers(1, 256))
        elif kind == 5:    # early corruption: desynchronised for (almost) the whole stream, runs dry or starves
            for _ in range(int(rng.integers(1, 4))):
                if data:
                    data[int(rng.integers(0, min(len(data), 64)))] ^= int(rng.integers(1, 256))
        elif kind == 6:    # streams shorter than the 4-byte state, or barely longer
            data = bytearray(rng.integers(0, 256, int(rng.integers(0, 12)), dtype=np.uint8).tobytes())
        elif kind == 7:    # more symbols asked for than were encoded: the stream runs out
            n_dec = n + int(rng.integers(1, 3 * 4096))
        elif kind in (8, 9):
            choice = i // 12 % 3
            if choice == 1:
                data = bytearray(rng.integers(0, 256, int(rng.integers(0, 40)), dtype=np.uint8).tobytes())
            elif choice == 2:
                data = bytearray(rng.integers(0, 256, int(rng.integers(9000, 30000)), dtype=np.uint8).tobytes())
        elif kind == 10:   # a long run of zero bytes: the state stays 0 and one symbol's refill loop eats whole windows
            data = bytearray(int(rng.integers(9000, 40000))) + bytearray(rng.integers(0, 256, 5000, dtype=np.uint8).tobytes())
        elif kind == 11:   # pure garbage of a realistic length
            data = bytearray(rng.integers(0, 256, max(16, len(data)), dtype=np.uint8).tobytes())
        data = bytes(data)
        ref = oracle_mod.rans_decode(data, n_dec, to)
        got = gpu_codec.RansDecoder(data).decode_n(n_dec, tg)
        assert np.array_equal(got, ref), (i, kind, n, n_dec, len(data), int(np.argmax(got != ref)))
        # (no comparison with `sym`: the reference decoder desynchronises on most intact streams too -- SURVEY.md fact 3)
        fast, slow, paths, consumed = _stats(gpu_codec)
        assert fast + slow >= 3
        seen |= paths
        n_cases += 1
    assert n_cases >= 300
    missing = [name for bit, name in PATHS.items() if bit != 256 and not seen & bit]
    assert not missing, f"tile-loop branches never taken by the fuzz set: {missing} (mask {seen:#x})"


def test_decoder_fuzz_caller_tables(gpu_codec, oracle_mod):
    """Tables that no histogram produces (the stage API takes explicit arrays): overlapping slot ranges -- the last symbol
    wins, as in the reference's fill loop -- uncovered slots (symbol 0), and frequencies above 4096 that own slots, which
    the kernel's packed entries cannot express: there the exact loop must take every tile."""
    rng = np.random.default_rng(77)
    exact_seen = 0
    for i in range(40):
        freq = rng.integers(1, 64, 256).astype(np.uint16)
        cum = np.minimum(np.cumsum(np.concatenate([[0], freq[:-1]])), 65535).astype(np.uint16)
        if i % 4 == 1:     # overlaps and gaps
            cum = rng.integers(0, 4200, 256).astype(np.uint16)
        elif i % 4 == 2:   # a frequency above 4096 with live slots
            k = int(rng.integers(0, 256))
            freq[k] = int(rng.integers(4097, 65535)); cum[k] = int(rng.integers(0, 4000))
        elif i % 4 == 3:   # exactly 4096 at a non-zero cum, others overlapping it
            k = int(rng.integers(0, 128))
            freq[k] = 4096; cum[k] = int(rng.integers(0, 300))
        to = _custom_oracle_table(oracle_mod, cum, freq)
        tg = gpu_codec.FrequencyTable(cum, freq)
        n = int(rng.integers(3 * 4096, 4 * 4096 + 500))
        for data in (bytes(rng.integers(0, 256, int(rng.integers(0, 20000)), dtype=np.uint8)), b"\x00\x80\x00\x00", b""):
            ref = oracle_mod.rans_decode(data, n, to)
            got = gpu_codec.RansDecoder(data).decode_n(n, tg)
            assert np.array_equal(got, ref), (i, len(data), int(np.argmax(got != ref)))
            fast, slow, paths, consumed = _stats(gpu_codec)
            owners = {int(to._t.cum_to_sym[k]) for k in range(4096)}
            if any(int(freq[o]) > 4096 for o in owners):
                assert fast == 0 and slow >= 3   # kTableDecExact: no packed entry for that symbol's slots
                exact_seen += 1
    assert exact_seen >= 3


def test_decoder_unaligned_device_buffers(gpu_codec, oracle_mod):
    """Stream and symbol buffers at every byte alignment, through the device-pointer entry point the slab path uses."""
    import torch
    lib = gpu_codec.load_library()
    rng = np.random.default_rng(5)
    seen = 0
    for off_in in range(4):
        for off_out in range(4):
            n = int(rng.integers(3 * 4096, 4 * 4096 + 300))
            sym = _symbols(rng, n, 0.6, 40)
            hist = np.bincount(sym, minlength=256).astype(np.uint32)
            to = oracle_mod.FrequencyTable(hist)
            data = bytearray(oracle_mod.rans_encode(sym, to))
            if (off_in + off_out) % 3 == 1:
                data[len(data) // 3] ^= 0x55      # desynchronise part of the way in
            if (off_in + off_out) % 3 == 2:
                data = data[: len(data) * 2 // 3]
            data = bytes(data)
            ref = oracle_mod.rans_decode(data, n, to)
            buf = torch.zeros(len(data) + 16, dtype=torch.uint8, device="cuda")
            buf[off_in: off_in + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
            out = torch.full((n + 16,), 0xEE, dtype=torch.uint8, device="cuda")
            rc = lib.alice_codec_dev_rans_decode(buf.data_ptr() + off_in, len(data), hist.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                 out.data_ptr() + off_out, n, None)
            assert rc == 0
            host = out.cpu().numpy()
            assert np.array_equal(host[off_out: off_out + n], ref), (off_in, off_out)
            assert (host[:off_out] == 0xEE).all() and (host[off_out + n:] == 0xEE).all()   # nothing written outside
            seen |= _stats(gpu_codec)[2]
    assert seen & 256, "no tile saw an unaligned output pointer"
