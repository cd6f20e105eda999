"""Frame ranges on the MI355X: alice_codec_dev_decode_frames and alice_codec_decode_frames against
the library's own full decode sliced to the range (and against the CPU references for the smallest shapes), with the plan
of tests/frames_ref.py held against what the calls report they did -- a decode that did everything and sliced would
pass the parity and fail there.  Lane size 64 (a block is 4096 symbols); the shapes and what each is for are listed at
frames_ref.SHAPES.  130x66 has a padded width that is no multiple of 4, so the band plan never cuts it: the banded case
sets the band target for it all the same, and proves a real cut on 96x70x24."""
import ctypes as C
import os
import struct
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle.alice_oracle_np as o  # noqa: E402
import frames_ref as FR  # noqa: E402
import split_ref as R2  # noqa: E402
import wide_oracle as WO  # noqa: E402
import wide_ref as R3  # noqa: E402
from test_frames_host import _decode_syms  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 256
L = FR.LANE
HEADER = 1630
# qualities whose steps select the inverse variants the suite names: steps 1, 5, 14, 64 for the wide symbols of versions 3
# and 4, q = 50, 80, 96 for version 2
QUALITIES = {2: (50, 80, 96), 3: (100, 95, 80, 0), 4: (100, 95, 80, 0)}
REFERENCE_SHAPES = {(33, 17, 5), (5, 3, 7), (40, 24, 1), (40, 24, 2)}


def quality_for(shape, kind, version):
    qs = QUALITIES[version]
    return qs[(FR.SHAPES.index(tuple(shape)) + kind) % len(qs)]


def _guard_pattern(n):
    return torch.tensor([0, 255], dtype=torch.uint8, device=DEV).repeat((n + 1) // 2)[:n]


def _encode(a, version, rgb, w, h, f, q, kind, lane=L):
    enc = a.FrameEncoder.with_wavelet(q, a.WaveletType(kind))
    return {2: a.encode_split, 3: a.encode_wide, 4: a.encode_reversible}[version](enc, rgb, w, h, f, lane)


def _full_decode(a, version, blob):
    return {2: a.decode_split, 3: a.decode_wide, 4: a.decode_reversible}[version](blob)


def _info(a, version, blob):
    return {2: a.split_info, 3: a.wide_info, 4: a.reversible_info}[version](blob)


class Chunk:
    """One encoded chunk, its full decode on the device, and the buffers of the calls: the container at an odd device
    address, the output between guard bytes of 0 and 255."""

    def __init__(self, a, version, shape, kind, q=None, seed=None, lane=L, blob=None):
        """blob: a container made elsewhere (nothing is encoded or fully decoded here: full and full_dev stay None)"""
        self.a, self.version, self.shape, self.kind = a, version, tuple(shape), kind
        w, h, f = shape
        if blob is None:
            self.q = quality_for(shape, kind, version) if q is None else q
            self.rgb = WO.smooth_plus_noise(w, h, f, seed=(w * 7 + f) if seed is None else seed)
            self.blob = _encode(a, version, self.rgb, w, h, f, self.q, kind, lane)
            self.full = np.asarray(_full_decode(a, version, self.blob))
            self.full_dev = torch.from_numpy(self.full.copy()).to(DEV)
        else:
            self.q, self.rgb, self.blob, self.full, self.full_dev = None, None, bytes(blob), None, None
        self.frame_bytes = w * h * 3
        self.out = torch.empty(2 * GUARD + f * self.frame_bytes, dtype=torch.uint8, device=DEV)
        self.pattern = _guard_pattern(self.out.numel())
        self.set_container(self.blob)

    def set_container(self, blob):
        raw = np.frombuffer(bytes(blob), np.uint8)
        self.d_alc = torch.empty(raw.size + 8, dtype=torch.uint8, device=DEV)
        off = 1 if self.d_alc.data_ptr() % 2 == 0 else 2
        self.alc_view = self.d_alc[off:off + raw.size]
        self.alc_view.copy_(torch.from_numpy(raw.copy()))
        assert self.alc_view.data_ptr() % 2 == 1
        self.alc_len = raw.size

    def dev_frames(self, t0, t1):
        """-> the (t1 - t0) frames on the device, after the guards and everything behind the frames were checked"""
        n = (t1 - t0) * self.frame_bytes
        self.out.copy_(self.pattern)
        self.a.frames_decode_device(self.alc_view.data_ptr(), self.alc_len, t0, t1 - t0, self.out.data_ptr() + GUARD)
        torch.cuda.synchronize()
        assert torch.equal(self.out[:GUARD], self.pattern[:GUARD]), "bytes before the output were written"
        assert torch.equal(self.out[GUARD + n:], self.pattern[GUARD + n:]), "bytes behind the output were written"
        return self.out[GUARD:GUARD + n]

    def untouched(self):
        torch.cuda.synchronize()
        return torch.equal(self.out, self.pattern)

    def want_dev(self, t0, t1):
        return self.full_dev[t0 * self.frame_bytes:t1 * self.frame_bytes]

    def planned_bytes(self, plan):
        """sum of the planned blocks' lengths over the three channels, read from the container"""
        info = _info(self.a, self.version, self.blob)
        pos, total = HEADER, 0
        for c in range(3):
            table = np.frombuffer(self.blob, "<u4", info.n_blocks[c], pos)
            total += int(table[plan["planned"]].astype(np.int64).sum())
            pos += info.payload_len[c]
        return total


def _check_stats(a, plan, count, uploaded):
    assert a._test_last_frames_stats() == (plan["a"], plan["b"], 3 * plan["n_planned"], uploaded, count)


@pytest.mark.parametrize("version", [2, 3, 4])
@pytest.mark.parametrize("shape", FR.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ranges_equal_the_full_decode_and_do_partial_work(gpu_codec, shape, version):
    a = gpu_codec
    w, h, f = shape
    for kind in FR.WAVELETS:
        ch = Chunk(a, version, shape, kind)
        if tuple(shape) in REFERENCE_SHAPES:      # the library's full decode is the reference's
            _, syms, unmap, to_rgb = _decode_syms(version, ch.blob)
            assert np.array_equal(to_rgb([unmap(s) for s in syms], R2.padded_dims(w, h, f), f), ch.full), (shape, version, kind)
        named = set(FR.named_ranges(kind, f))
        for t0, t1 in FR.ranges_for(shape, kind):
            plan = FR.frame_plan(kind, w, h, f, L, t0, t1)
            got = ch.dev_frames(t0, t1)
            assert torch.equal(got, ch.want_dev(t0, t1)), (shape, version, kind, ch.q, (t0, t1))
            _check_stats(a, plan, t1 - t0, 0)
            if (t0, t1) in named:
                host = np.asarray(a.decode_frames(ch.blob, t0, t1 - t0))
                assert np.array_equal(host, ch.full[t0 * ch.frame_bytes:t1 * ch.frame_bytes]), (shape, version, kind, (t0, t1))
                _check_stats(a, plan, t1 - t0, ch.planned_bytes(plan))


def test_every_inverse_variant_ran(gpu_codec):
    """The qualities of the case table select all four instances of the inverse on the tile-eligible shapes."""
    lib = gpu_codec.load_library()
    seen = {2: set(), 3: set(), 4: set()}
    for shape in FR.SHAPES:
        if min(shape[0], shape[1]) < 6:
            continue
        for kind in FR.WAVELETS:
            for version in (2, 3, 4):
                step = _step_of(quality_for(shape, kind, version))
                seen[version].add(lib.alice_codec_test_inverse_variant(kind, (C.c_int32 * 3)(step, step, step), int(version != 2)))
    print("inverse variants by version:", seen)
    assert seen[3] == {0, 1, 2, 3} and seen[4] == {0, 1, 2, 3}
    assert seen[2] | seen[3] == {0, 1, 2, 3} and len(seen[2]) >= 2


def _step_of(q):
    return o.quality_to_step(q)


def test_the_steps_are_the_named_ones():
    assert [_step_of(q) for q in QUALITIES[3]] == [1, 5, 14, 64]


def test_banded_window(gpu_codec):
    """A band target that cuts the slot of the kept frames: 96x70 (three tile rows) is cut, and 130x66 runs under the same
    target.  The pixels are the uncut decode's; the target is restored afterwards."""
    a = gpu_codec
    lib = a.load_library()
    chunks = [Chunk(a, v, shape, kind, q) for shape in ((96, 70, 24), (130, 66, 40))
              for v, kind, q in ((2, FR.CDF97, 80), (3, FR.CDF53, 95), (4, FR.HAAR, 100), (4, FR.CDF97, 80))]
    uncut = lib.alice_codec_test_inverse_scratch_bytes(96, 70, 3, 1)
    try:
        lib.alice_codec_test_set_tuning(1)
        assert 0 < lib.alice_codec_test_inverse_scratch_bytes(96, 70, 3, 1) < uncut, "the band target does not cut 96x70"
        for ch in chunks:
            f = ch.shape[2]
            for t0, t1 in ((0, 1), (f // 2, f // 2 + 3), (f - 2, f), (0, f)):
                assert torch.equal(ch.dev_frames(t0, t1), ch.want_dev(t0, t1)), (ch.shape, ch.version, ch.kind, (t0, t1))
            host = np.asarray(a.decode_frames(ch.blob, 5, 3))
            assert np.array_equal(host, ch.full[5 * ch.frame_bytes:8 * ch.frame_bytes])
    finally:
        lib.alice_codec_test_set_tuning(1024 * 1024)


# ---- damage ----
def _channel_layout(blob):
    """lane_symbols and, per channel, (payload offset, n_blocks, block offsets inside the payload, block lengths,
    payload length, num_symbols), read from the container's header and block tables"""
    lane_symbols = struct.unpack_from("<I", blob, 18)[0]
    out, pos = [], HEADER
    for c in range(3):
        ns, nb, plen = struct.unpack_from("<IIQ", blob, 22 + c * 536 + 8)
        lens = np.frombuffer(blob, "<u4", nb, pos).astype(np.int64)
        offs = 4 * nb + np.concatenate([[0], np.cumsum(lens)[:-1]])
        out.append((pos, nb, offs, lens, plen, ns))
        pos += plen
    return lane_symbols, out


def _lane_flip(version, blob, channel, block):
    """The container with one byte flipped inside the longest lanes of `block` of `channel`, chosen so that the reference
    decoder's end check of that channel fails on the CPU."""
    lane_symbols, lay = _channel_layout(blob)
    pos, nb, offs, lens, plen, ns = lay[channel]
    blk = pos + int(offs[block])
    lane_len = np.frombuffer(blob, "<u2", 64, blk).astype(np.int64)
    starts = blk + 128 + np.concatenate([[0], np.cumsum(lane_len)[:-1]])
    freq = np.frombuffer(blob, "<u2", 256, 22 + channel * 536 + 24).astype(np.uint16)
    decode = R2.decode_channel if version == 2 else R3.decode_channel
    for lane in np.argsort(-lane_len, kind="stable")[:8]:
        assert lane_len[lane] >= 12, "the lanes of this block are too short for a flip that cannot resynchronise"
        bad = bytearray(blob)
        bad[int(starts[lane]) + 1] ^= 0x5A          # the second state byte: every later slot of the chain changes
        _, ok = decode(bytes(bad[pos:pos + plen]), freq, lane_symbols, ns)
        if not ok:
            return bytes(bad)
    raise AssertionError("no flip that the reference decoder refuses")


@pytest.mark.parametrize("version", [2, 3, 4])
def test_damage(gpu_codec, version):
    a = gpu_codec
    shape, kind = (64, 64, 16), FR.CDF53
    w, h, f = shape
    ch = Chunk(a, version, shape, kind, q=80)
    t0, t1 = 9, 10
    plan = FR.frame_plan(kind, w, h, f, L, t0, t1)
    outside = [b for b in range(plan["n_blocks"]) if b not in plan["planned"]]
    assert outside and "blocks_skipped" in plan["classes"]
    want = ch.want_dev(t0, t1).clone()
    full_decode = {2: a.decode_split, 3: a.decode_wide, 4: a.decode_reversible}[version]

    # a lane of a planned block: refused by both calls
    for channel, block in ((0, plan["planned"][0]), (2, plan["planned"][-1])):
        bad = _lane_flip(version, ch.blob, channel, block)
        ch.set_container(bad)
        with pytest.raises(a.CodecError) as e:
            ch.dev_frames(t0, t1)
        assert e.value.code == 4 and "end check" in str(e.value)
        with pytest.raises(a.CodecError) as e:
            a.decode_frames(bad, t0, t1 - t0)
        assert e.value.code == 4

    # a lane of a block outside the plan: the frames come back as from the undamaged file, the full decode refuses it
    for channel, block in ((0, outside[0]), (1, outside[-1])):
        bad = _lane_flip(version, ch.blob, channel, block)
        ch.set_container(bad)
        assert torch.equal(ch.dev_frames(t0, t1), want)
        assert np.array_equal(np.asarray(a.decode_frames(bad, t0, t1 - t0)), want.cpu().numpy())
        with pytest.raises(a.CodecError) as e:
            full_decode(bad)
        assert e.value.code == 4

    # a block-length entry outside the plan: the scan covers the whole table
    _, lay = _channel_layout(ch.blob)
    for delta in (1, -1):
        bad = bytearray(ch.blob)
        pos = lay[1][0] + 4 * outside[0]
        v = int.from_bytes(bad[pos:pos + 4], "little") + delta
        bad[pos:pos + 4] = v.to_bytes(4, "little")
        ch.set_container(bytes(bad))
        with pytest.raises(a.CodecError) as e:
            ch.dev_frames(t0, t1)
        assert e.value.code == 4 and "directory" in str(e.value)
        with pytest.raises(a.CodecError) as e:
            a.decode_frames(bytes(bad), t0, t1 - t0)
        assert e.value.code == 4


def test_refusals_write_nothing(gpu_codec):
    a = gpu_codec
    shape, kind = (33, 17, 5), FR.CDF97
    w, h, f = shape
    ch = Chunk(a, 3, shape, kind, q=80)
    ch.out.copy_(ch.pattern)
    a.decode_frames(ch.blob, 0, 1)
    stats = a._test_last_frames_stats()
    out = ch.out.data_ptr() + GUARD
    for first, count in ((0, 0), (0, f + 1), (f, 1), (3, 3)):
        with pytest.raises(a.CodecError) as e:
            a.frames_decode_device(ch.alc_view.data_ptr(), ch.alc_len, first, count, out)
        assert e.value.code == 2
        assert ch.untouched()
    v1 = o.encode(ch.rgb, w, h, f, 80, kind)
    ch.set_container(v1)
    with pytest.raises(a.CodecError, match=r"version 1 has no random access \(one serial chain per channel\)"):
        a.frames_decode_device(ch.alc_view.data_ptr(), ch.alc_len, 0, 1, out)
    assert ch.untouched()
    for damage in ((0, ord("B")), (5, 7), (18, 3)):       # magic, wavelet byte, lane_symbols
        bad = bytearray(ch.blob)
        bad[damage[0]] = damage[1]
        ch.set_container(bytes(bad))
        with pytest.raises(a.CodecError) as e:
            a.frames_decode_device(ch.alc_view.data_ptr(), ch.alc_len, 0, 1, out)
        assert e.value.code == 4
        assert ch.untouched()
    ch.set_container(ch.blob)
    with pytest.raises(a.CodecError) as e:                # a container cut short
        a.frames_decode_device(ch.alc_view.data_ptr(), ch.alc_len - 1, 0, 1, out)
    assert e.value.code == 4 and ch.untouched()
    assert a._test_last_frames_stats() == stats, "a refused call must not report work"
