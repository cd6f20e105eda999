"""Frame ranges and half-size previews of a banded chunk on the MI355X: the four new calls against
the numpy references (tests/banded_ref.py sliced, tests/preview_ref.py on its symbols) and against the library's own base
route (decode_frames / decode_preview of from_banded), bit for bit, with the plan of tests/banded_partial_ref.py held against
what the calls report they did -- a decode that did every block and sliced would pass the parity and fail there.  Lane size
64 unless stated; the shapes and what each is for are listed at banded_partial_ref.SHAPES and in the design section."""
import os
import sys
import threading

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import banded_partial_ref as BP  # noqa: E402
import banded_ref as B  # noqa: E402
import frames_extreme_cases as F  # noqa: E402
import frames_ref as FR  # noqa: E402
import preview_ref as PR  # noqa: E402
import wide_oracle as WO  # noqa: E402
from test_gpu_banded import clip  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 256
L = BP.LANE
QUALITIES = {2: (50, 80, 96), 3: (100, 95, 80, 0), 4: (100,)}


def _guard_pattern(n):
    return torch.tensor([0, 255], dtype=torch.uint8, device=DEV).repeat((n + 1) // 2)[:n]


class Banded:
    """One banded container on the device at a chosen byte offset from a 4-byte boundary, and the outputs of the device
    calls between guard bytes of 0 and 255."""

    def __init__(self, a, blob, shape, offset=1):
        self.a, self.shape, self.offset = a, tuple(shape), offset
        w, h, f = shape
        qw, qh = PR.preview_dims(w, h)
        self.frame_bytes = {BP.FRAMES: w * h * 3, BP.PREVIEW: qw * qh * 3}
        self.out = torch.empty(2 * GUARD + f * w * h * 3, dtype=torch.uint8, device=DEV)
        self.pattern = _guard_pattern(self.out.numel())
        self.set_container(blob)

    def set_container(self, blob):
        self.blob = bytes(blob)
        raw = np.frombuffer(self.blob, np.uint8)
        self.d_alc = torch.empty(raw.size + 16, dtype=torch.uint8, device=DEV)
        off = (-self.d_alc.data_ptr()) % 4 + self.offset
        self.alc_view = self.d_alc[off:off + raw.size]
        assert self.alc_view.data_ptr() % 4 == self.offset % 4
        self.alc_view.copy_(torch.from_numpy(raw.copy()))
        self.alc_len = raw.size

    def dev(self, mode, t0, t1, stream=0):
        """-> frames or preview of [t0, t1) as numpy, after the guards and everything behind the result were checked"""
        n = (t1 - t0) * self.frame_bytes[mode]
        self.out.copy_(self.pattern)
        torch.cuda.synchronize()
        call = self.a.banded_frames_decode_device if mode == BP.FRAMES else self.a.banded_preview_decode_device
        call(self.alc_view.data_ptr(), self.alc_len, t0, t1 - t0, self.out.data_ptr() + GUARD, stream)
        torch.cuda.synchronize()
        assert torch.equal(self.out[:GUARD], self.pattern[:GUARD]), "bytes before the output were written"
        assert torch.equal(self.out[GUARD + n:], self.pattern[GUARD + n:]), "bytes behind the output were written"
        return self.out[GUARD:GUARD + n].cpu().numpy()

    def untouched(self):
        torch.cuda.synchronize()
        return torch.equal(self.out, self.pattern)


def _host(a, mode, blob, t0, t1):
    return np.asarray((a.decode_banded_frames if mode == BP.FRAMES else a.decode_banded_preview)(blob, t0, t1 - t0))


def _base(a, mode, plain, t0, t1):
    return np.asarray((a.decode_frames if mode == BP.FRAMES else a.decode_preview)(plain, t0, t1 - t0))


def _check_stats(a, mode, plan, count, uploaded):
    got = a._test_last_banded_partial_stats(mode)
    assert got == (plan["a"], plan["b"], plan["blocks_total"], uploaded, count, plan["stored"]), (mode, got)


def _encode(a, rgb, shape, q, kind, base, lane=L):
    enc = a.FrameEncoder.with_wavelet(q, a.WaveletType(kind))
    return a.encode_banded(enc, rgb, *shape, lane, base)


def _check_against_base(a, bd, plain, kind, lane, ranges, host_ranges, where):
    """both device calls on every range (and the host calls on host_ranges) against the library's base route, with the plan"""
    w, h, f = bd.shape
    for t0, t1 in ranges:
        for mode in (BP.FRAMES, BP.PREVIEW):
            want = _base(a, mode, plain, t0, t1)
            plan = BP.plan(mode, kind, w, h, f, lane, t0, t1)
            got = bd.dev(mode, t0, t1)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (where, mode, (t0, t1), bad.size, bad[:4].tolist())
            _check_stats(a, mode, plan, t1 - t0, 0)
            if (t0, t1) in host_ranges:
                assert np.array_equal(_host(a, mode, bd.blob, t0, t1), want), (where, mode, (t0, t1), "host call")
                _check_stats(a, mode, plan, t1 - t0, BP.planned_payload_bytes(bd.blob, plan))


# ---- 1. the case table ----
@pytest.mark.parametrize("base", [2, 3, 4])
@pytest.mark.parametrize("shape", BP.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_case_table_equals_the_references_and_does_partial_work(gpu_codec, shape, base):
    a = gpu_codec
    w, h, f = shape
    dims = BP.padded(w, h, f)
    for kind in BP.kinds_for(shape):
        q = QUALITIES[base][(BP.SHAPES.index(tuple(shape)) + kind) % len(QUALITIES[base])]
        rgb = WO.smooth_plus_noise(w, h, f, seed=w * 7 + f)
        blob = _encode(a, rgb, shape, q, kind, base)
        info, syms = B.decode_container(blob)
        assert (info["width"], info["height"], info["frames"], info["wavelet"], info["base"]) == (w, h, f, kind, base)
        full = B.pixels(info, syms, base).reshape(f, -1)
        plain = a.from_banded(blob)
        bd = Banded(a, blob, shape)
        host_ranges = set(FR.named_ranges(kind, f))
        for t0, t1 in BP.ranges_for(shape, kind):
            where = (shape, base, kind, q, (t0, t1))
            want = {BP.FRAMES: full[t0:t1].reshape(-1), BP.PREVIEW: PR.preview(syms, dims, f, kind, info["step"], base, t0, t1)}
            for mode in (BP.FRAMES, BP.PREVIEW):
                plan = BP.plan(mode, kind, w, h, f, L, t0, t1)
                got = bd.dev(mode, t0, t1)
                bad = np.flatnonzero(got != want[mode])
                assert bad.size == 0, (where, mode, bad.size, bad[:4].tolist())
                _check_stats(a, mode, plan, t1 - t0, 0)
                assert np.array_equal(_base(a, mode, plain, t0, t1), want[mode]), (where, mode, "the base route")
                if (t0, t1) in host_ranges:
                    assert np.array_equal(_host(a, mode, blob, t0, t1), want[mode]), (where, mode, "host call")
                    _check_stats(a, mode, plan, t1 - t0, BP.planned_payload_bytes(blob, plan))


# ---- 2. lane sizes ----
LANE_SHAPE = (128, 96, 40)          # n_band = 61 440: 7.5 blocks at L = 128, two (one short) at 512, one short block at the maximum


@pytest.mark.parametrize("base,lane", [(2, 128), (2, 512), (2, 16384), (3, 128), (3, 512), (3, 8192)])
def test_lane_sizes(gpu_codec, base, lane):
    a = gpu_codec
    w, h, f = LANE_SHAPE
    kind = (lane // 128 + base) % 2
    p = BP.plan(BP.FRAMES, kind, w, h, f, lane, 0, f)
    assert p["n_band"] == 61440 and p["n_blocks"] == {128: 8, 512: 2}.get(lane, 1)
    rgb = WO.smooth_plus_noise(w, h, f, seed=40 + kind)
    blob = _encode(a, rgb, LANE_SHAPE, 80 if base == 2 else 100, kind, base, lane)      # step 1 gives the wide symbols escapes
    assert a.banded_info(blob).lane_symbols == lane
    bd = Banded(a, blob, LANE_SHAPE)
    _check_against_base(a, bd, a.from_banded(blob), kind, lane, F.lane_ranges(kind, f), {(0, f), (f // 2, f // 2 + 1)}, (base, lane, kind))


# ---- 3. wide content ----
@pytest.mark.parametrize("base", [3, 4])
def test_low_band_escapes_alone(gpu_codec, base):
    """q = 100 gradients: band 0 alone holds escapes, so the preview's two bands run different paths of the wide chain"""
    a = gpu_codec
    shape = (32, 16, 4)
    rgb = clip("smooth", shape)
    for kind in (BP.CDF53, BP.CDF97):
        blob = _encode(a, rgb, shape, 100, kind, base)
        info = B.parse_container(blob)
        assert info["freq"][0][255] > 0 and all(info["freq"][k][255] == 0 for k in range(1, 8))
        bd = Banded(a, blob, shape)
        rs = BP.ranges_for(shape, kind)
        _check_against_base(a, bd, a.from_banded(blob), kind, L, rs, set(rs), (base, kind))


@pytest.mark.parametrize("base", [2, 3])
def test_flat_grey(gpu_codec, base):
    """seven bands per channel code one symbol: a single frequency of 4096 and four state bytes a lane"""
    a = gpu_codec
    shape = (33, 17, 5)
    rgb = clip("flat_grey", shape)
    for kind in (BP.CDF53, BP.CDF97):
        blob = _encode(a, rgb, shape, 80, kind, base)
        info = B.parse_container(blob)
        assert all(int(info["freq"][8 * c + k].max()) == 4096 for c in range(3) for k in range(1, 8))
        bd = Banded(a, blob, shape)
        rs = BP.ranges_for(shape, kind)
        _check_against_base(a, bd, a.from_banded(blob), kind, L, rs, set(rs), (base, kind))
        assert np.array_equal(bd.dev(BP.FRAMES, 0, shape[2]), np.asarray(a.decode_banded(blob)))


# ---- 4. every instance class of the two finishes, at an edge step ----
@pytest.mark.parametrize("version", [2, 3, 4])
@pytest.mark.parametrize("kind", BP.WAVELETS)
def test_inverse_classes_at_an_edge_step(gpu_codec, kind, version):
    """104x40x16: the worst-sign volume of tests/transform_extremes.py at an edge step of every instance class the launcher
    can pick, repacked with to_banded"""
    a = gpu_codec
    lib = a.load_library()
    shape = (104, 40, 16)
    f = shape[2]
    T = F.centre_frame(kind, shape)
    edges = F.class_edges(lib, kind, version)
    assert set(edges) == F.EXPECTED[version][kind]
    bd = None
    for v, edge in sorted(edges.items()):
        steps = sorted(edge)[-1]
        assert F.variant(lib, kind, steps, version) == v
        plain = F.container(kind, shape, "worst", steps, version)
        blob = a.to_banded(plain)
        assert a.from_banded(blob) == plain
        if bd is None:
            bd = Banded(a, blob, shape)
        else:
            bd.set_container(blob)
        _check_against_base(a, bd, plain, kind, F.LANE_SYMBOLS, [(0, f), (T, T + 1), (T + 1, T + 2), (f - 1, f)], {(T, T + 1)},
                            (kind, version, v, steps))


# ---- 5. alignment ----
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_container_at_every_byte_offset(gpu_codec, offset):
    a = gpu_codec
    shape, kind = (50, 38, 13), BP.CDF97
    rgb = WO.smooth_plus_noise(*shape, seed=3)
    for base in (2, 3):
        blob = _encode(a, rgb, shape, 80, kind, base)
        bd = Banded(a, blob, shape, offset)
        _check_against_base(a, bd, a.from_banded(blob), kind, L, FR.named_ranges(kind, shape[2]), set(), (base, offset))


# ---- 6. damage: flipped payload bytes and table entries only ----
def _layout(blob):
    """per stream j: (payload offset, block offsets inside the payload, block lengths)"""
    info = B.parse_container(blob)
    out, pos = [], B.HEADER
    for j in range(24):
        nb = info["n_blocks"][j]
        lens = np.frombuffer(blob, "<u4", nb, pos).astype(np.int64)
        offs = 4 * nb + np.concatenate([[0], np.cumsum(lens)[:-1]])
        out.append((pos, offs, lens))
        pos += info["payload_len"][j]
    return info, out


def _lane_flip(blob, j, block):
    """The container with one byte flipped in one of the longest lanes of `block` of stream j, chosen so that the reference
    decoder's end check of that band fails on the CPU."""
    info, lay = _layout(blob)
    pos, offs, lens = lay[j]
    blk = pos + int(offs[block])
    lane_len = np.frombuffer(blob, "<u2", 64, blk).astype(np.int64)
    starts = blk + 128 + np.concatenate([[0], np.cumsum(lane_len)[:-1]])
    decode = B.coder(info["base"]).decode_channel
    n_band = info["num_symbols"][0] // 8
    for lane in np.argsort(-lane_len, kind="stable")[:8]:
        assert lane_len[lane] >= 12, "the lanes of this block are too short for a flip that cannot resynchronise"
        bad = bytearray(blob)
        bad[int(starts[lane]) + 1] ^= 0x5A          # the second state byte: every later slot of the chain changes
        _, ok = decode(bytes(bad[pos:pos + info["payload_len"][j]]), info["freq"][j], info["lane_symbols"], n_band)
        if not ok:
            return bytes(bad)
    raise AssertionError("no flip that the reference decoder refuses")


@pytest.mark.parametrize("base", [2, 3])
def test_damage(gpu_codec, base):
    a = gpu_codec
    shape, kind = (160, 96, 16), BP.CDF53
    w, h, f = shape
    t0, t1 = 6, 7
    rgb = WO.smooth_plus_noise(w, h, f, seed=11)
    blob = _encode(a, rgb, shape, 96 if base == 2 else 100, kind, base)       # small steps: no lane is short
    plan = BP.plan(BP.FRAMES, kind, w, h, f, L, t0, t1)
    assert (plan["blk_first"], plan["blk_count"], plan["n_blocks"]) == (1, 4, 8) and {"first_block_clipped", "last_block_clipped"} <= plan["classes"]
    plain = a.from_banded(blob)
    want = {m: _base(a, m, plain, t0, t1) for m in (BP.FRAMES, BP.PREVIEW)}
    bd = Banded(a, blob, shape)
    for m in (BP.FRAMES, BP.PREVIEW):
        assert np.array_equal(bd.dev(m, t0, t1), want[m])

    def refused(bad, modes, words, host_words=None):
        bd.set_container(bad)
        for m in modes:
            before = a._test_last_banded_partial_stats(m)
            with pytest.raises(a.CodecError) as e:
                bd.dev(m, t0, t1)
            assert e.value.code == 4 and all(x in str(e.value) for x in words), (m, str(e.value))
            assert bd.untouched(), "a refused call wrote to its output"
            with pytest.raises(a.CodecError) as e:
                _host(a, m, bad, t0, t1)
            assert e.value.code == 4 and all(x in str(e.value) for x in (host_words or words)), (m, str(e.value))
            assert a._test_last_banded_partial_stats(m) == before, "a refused call must not report work"

    # a lane of a planned block of a kept band: refused with the stream's number, the output untouched
    for (c, k), block, modes in (((0, 0), 1, (BP.FRAMES, BP.PREVIEW)), ((2, 4), 4, (BP.FRAMES, BP.PREVIEW)), ((1, 7), 2, (BP.FRAMES,))):
        refused(_lane_flip(blob, 8 * c + k, block), modes, (f"stream {8 * c + k}:", "end check"))

    # a lane of a block outside the window, and of a band the preview does not keep: not seen; the full decode refuses
    for (c, k), block, modes in (((0, 0), 0, (BP.FRAMES, BP.PREVIEW)), ((1, 4), 5, (BP.FRAMES, BP.PREVIEW)), ((0, 1), 2, (BP.PREVIEW,)),
                                 ((2, 6), 3, (BP.PREVIEW,))):
        bad = _lane_flip(blob, 8 * c + k, block)
        bd.set_container(bad)
        for m in modes:
            assert np.array_equal(bd.dev(m, t0, t1), want[m]), ((c, k), block, m)
            assert np.array_equal(_host(a, m, bad, t0, t1), want[m]), ((c, k), block, m)
        with pytest.raises(a.CodecError) as e:
            a.decode_banded(bad)
        assert e.value.code == 4

    # a short block-length entry in any of the 24 tables, planned or not, kept or not: the scan covers them all
    _, lay = _layout(blob)
    for (c, k), block in (((0, 0), 6), ((2, 7), 0)):
        bad = bytearray(blob)
        at = lay[8 * c + k][0] + 4 * block
        bad[at:at + 4] = (127).to_bytes(4, "little")
        refused(bytes(bad), (BP.FRAMES, BP.PREVIEW), (f"stream {8 * c + k}:", "directory"),
                (f"channel {c} band {k}: block {block} is shorter than its lane directory",))

    # a lane directory that does not sum to its block (a planned block of a kept band): the kernel's own check
    pos, offs, _ = lay[4]
    bad = bytearray(blob)
    at = pos + int(offs[2]) + 2 * 5
    bad[at:at + 2] = (int.from_bytes(bad[at:at + 2], "little") + 1).to_bytes(2, "little")
    refused(bytes(bad), (BP.FRAMES, BP.PREVIEW), ("stream 4:", "directory"))

    bd.set_container(blob)
    for m in (BP.FRAMES, BP.PREVIEW):
        assert np.array_equal(bd.dev(m, t0, t1), want[m]), "a refusal left something behind"


def test_refusals_write_nothing(gpu_codec):
    a = gpu_codec
    shape, kind = (33, 17, 5), BP.CDF97
    w, h, f = shape
    rgb = WO.smooth_plus_noise(w, h, f)
    blob = _encode(a, rgb, shape, 80, kind, 3)
    bd = Banded(a, blob, shape)
    bd.dev(BP.FRAMES, 0, 1)
    bd.dev(BP.PREVIEW, 0, 1)
    stats = {m: a._test_last_banded_partial_stats(m) for m in (BP.FRAMES, BP.PREVIEW)}
    bd.out.copy_(bd.pattern)
    out = bd.out.data_ptr() + GUARD
    calls = {BP.FRAMES: a.banded_frames_decode_device, BP.PREVIEW: a.banded_preview_decode_device}
    for m, call in calls.items():
        for first, count in ((0, 0), (0, f + 1), (f, 1), (3, 3), (0xFFFFFFFF, 2)):
            with pytest.raises(a.CodecError) as e:
                call(bd.alc_view.data_ptr(), bd.alc_len, first, count, out)
            assert e.value.code == 2 and bd.untouched()
        with pytest.raises(a.CodecError) as e:                # a container cut short
            call(bd.alc_view.data_ptr(), bd.alc_len - 1, 0, 1, out)
        assert e.value.code == 4 and "length mismatch" in str(e.value) and bd.untouched()
    bd.set_container(a.from_banded(blob))                     # the base version through the new calls
    for m, call in calls.items():
        with pytest.raises(a.CodecError, match=r"unsupported version: 3 \(expected 5\)"):
            call(bd.alc_view.data_ptr(), bd.alc_len, 0, 1, out)
        assert bd.untouched()
    # and the existing calls keep refusing version 5
    for call in (a.decode_frames, a.decode_preview):
        with pytest.raises(a.CodecError, match="unsupported version: 5"):
            call(blob, 0, 1)
    assert {m: a._test_last_banded_partial_stats(m) for m in stats} == stats, "a refused call must not report work"


# ---- 7. two threads on their own streams ----
def test_two_threads_on_their_own_streams(gpu_codec):
    a = gpu_codec
    jobs = []
    for i, (shape, kind, base, r) in enumerate((((50, 38, 13), BP.CDF97, 2, (5, 8)), ((160, 96, 16), BP.CDF53, 3, (6, 7)))):
        rgb = WO.smooth_plus_noise(*shape, seed=60 + i)
        blob = _encode(a, rgb, shape, 80, kind, base)
        plain = a.from_banded(blob)
        want = {m: _base(a, m, plain, *r) for m in (BP.FRAMES, BP.PREVIEW)}
        plans = {m: BP.plan(m, kind, *shape, L, *r) for m in want}
        jobs.append((Banded(a, blob, shape), r, want, plans))
    errors = []
    start = threading.Barrier(2)

    def work(bd, r, want, plans):
        try:
            torch.cuda.set_device(0)
            st = torch.cuda.Stream()
            n = {m: (r[1] - r[0]) * bd.frame_bytes[m] for m in want}
            outs = {m: torch.zeros(n[m], dtype=torch.uint8, device=DEV) for m in want}
            torch.cuda.synchronize()
            start.wait()
            for it in range(12):
                for m in ((BP.FRAMES, BP.PREVIEW) if it % 2 else (BP.PREVIEW, BP.FRAMES)):
                    call = a.banded_frames_decode_device if m == BP.FRAMES else a.banded_preview_decode_device
                    outs[m].zero_()
                    torch.cuda.synchronize()
                    call(bd.alc_view.data_ptr(), bd.alc_len, r[0], r[1] - r[0], outs[m].data_ptr(), st.cuda_stream)
                    assert np.array_equal(outs[m].cpu().numpy(), want[m]), (bd.shape, m, it)
                    p = plans[m]
                    assert a._test_last_banded_partial_stats(m) == (p["a"], p["b"], p["blocks_total"], 0, r[1] - r[0], p["stored"])
                    assert np.array_equal(_host(a, m, bd.blob, *r), want[m]), (bd.shape, m, it, "host call")
                    assert a._test_last_banded_partial_stats(m)[3] == BP.planned_payload_bytes(bd.blob, p)
        except BaseException as e:       # noqa: BLE001  (reported by the main thread)
            errors.append(e)
            start.abort()

    threads = [threading.Thread(target=work, args=j) for j in jobs]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
