"""Spatial rectangles of frame ranges on the MI355X: alice_codec_dev_decode_rect and
alice_codec_decode_rect against the numpy full decode cropped to [t0, t1) x rectangle, bit for bit, with the plan of
tests/rect_ref.py held against what the calls report they did -- a decode that did everything and cropped would pass the
parity and fail there.  Symbols come from the reference lane decoders (split_ref / wide_ref) or are the volumes the containers
were written from, the pixels from the numpy inverses; the library's own full decode is not the yardstick.  Containers sit at
odd device addresses, outputs between guard bytes of 0 and 255, and with a pitched destination the gaps between rows and
frames are guard bytes too.  Lane size 64 unless stated; the shapes and what each is for are listed at rect_ref.SHAPES."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle.alice_oracle_np as o  # noqa: E402
import frames_extreme_cases as F  # noqa: E402
import frames_ref as FR  # noqa: E402
import rect_ref as RF  # noqa: E402
import reversible_ref as RR  # noqa: E402
import wide_oracle as WO  # noqa: E402
import wide_ref as R3  # noqa: E402
from test_frames_host import _encode_ref  # noqa: E402
from test_gpu_frames import DEV, GUARD, HEADER, QUALITIES, _channel_layout, _encode, _guard_pattern, _info, _lane_flip  # noqa: E402
from test_gpu_frames_extremes import _reference_decode  # noqa: E402

pytestmark = pytest.mark.gpu

L = RF.LANE
_ran = {}      # (version, kind) -> {instance class: steps the window inverse ran at}


class Rects:
    """One container at an odd device address and an output buffer of full-size frames between guard bytes."""

    def __init__(self, a, blob, shape, kind, version, extra=0):
        self.a, self.shape, self.kind, self.version = a, tuple(shape), kind, version
        w, h, f = shape
        self.out = torch.empty(2 * GUARD + f * h * w * 3 + extra, dtype=torch.uint8, device=DEV)
        self.pattern = _guard_pattern(self.out.numel())
        self.pattern_host = self.pattern.cpu().numpy()
        self.set_container(blob)

    def set_container(self, blob):
        self.blob = bytes(blob)
        raw = np.frombuffer(self.blob, np.uint8)
        self.d_alc = torch.empty(raw.size + 8, dtype=torch.uint8, device=DEV)
        off = 1 if self.d_alc.data_ptr() % 2 == 0 else 2
        self.alc_view = self.d_alc[off:off + raw.size]
        self.alc_view.copy_(torch.from_numpy(raw.copy()))
        assert self.alc_view.data_ptr() % 2 == 1
        self.alc_len = raw.size

    def call(self, t0, t1, rect, at=0, row_pitch=0, frame_pitch=0):
        self.a.rect_decode_device(self.alc_view.data_ptr(), self.alc_len, t0, t1 - t0, *rect, self.out.data_ptr() + GUARD + at,
                                  row_pitch, frame_pitch)

    def dev(self, t0, t1, rect, at=0, row_pitch=0, frame_pitch=0):
        """-> the (t1 - t0, rh, rw, 3) pixels the call wrote, after every other byte of the buffer (guards, gaps between rows
        and frames, everything behind) was found unchanged"""
        _, _, rw, rh = rect
        self.out.copy_(self.pattern)
        self.call(t0, t1, rect, at, row_pitch, frame_pitch)
        torch.cuda.synchronize()
        got = self.out.cpu().numpy()
        rp = row_pitch or 3 * rw
        fp = frame_pitch or rp * rh
        idx = (GUARD + at + np.arange(t1 - t0)[:, None, None] * fp + np.arange(rh)[None, :, None] * rp + np.arange(3 * rw)[None, None, :])
        pixels = got[idx].reshape(t1 - t0, rh, rw, 3)
        rest = got.copy()
        rest[idx.reshape(-1)] = self.pattern_host[idx.reshape(-1)]
        bad = np.flatnonzero(rest != self.pattern_host)
        assert bad.size == 0, ("bytes outside the rectangle were written", bad.size, bad[:4].tolist())
        return pixels

    def untouched(self):
        torch.cuda.synchronize()
        return torch.equal(self.out, self.pattern)

    def planned_bytes(self, plan):
        info = _info(self.a, self.version, self.blob)
        pos, total = HEADER, 0
        for c in range(3):
            table = np.frombuffer(self.blob, "<u4", info.n_blocks[c], pos)
            total += int(table[plan["planned"]].astype(np.int64).sum())
            pos += info.payload_len[c]
        return total


def _crop(full, t0, t1, rect):
    x, y, rw, rh = rect
    return full[t0:t1, y:y + rh, x:x + rw]


def _check_stats(a, plan, count, uploaded):
    want = (plan["ta"], plan["tb"], plan["xa"], plan["xb"], plan["ya"], plan["yb"], 3 * plan["n_planned"], uploaded, count, plan["stored"])
    assert a._test_last_rect_stats() == want, (a._test_last_rect_stats(), want)


def _check(a, ch, full, lane, cases, host_rects, where):
    """every (range, rectangle) through the device call, the rectangles of host_rects through the host call too; both against
    the crop of `full` ((f, h, w, 3), the numpy decode) and rect_ref's plan"""
    w, h, f = ch.shape
    for (t0, t1), rect in cases:
        want = _crop(full, t0, t1, rect)
        plan = RF.rect_plan(ch.kind, w, h, f, lane, t0, t1, rect, classes=False)
        got = ch.dev(t0, t1, rect)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (where, (t0, t1), rect, bad.size, bad[:4].tolist())
        _check_stats(a, plan, t1 - t0, 0)
        if rect in host_rects:
            host = np.asarray(a.decode_rect(ch.blob, t0, t1 - t0, *rect))
            assert np.array_equal(host, want.reshape(-1)), (where, (t0, t1), rect, "host call")
            _check_stats(a, plan, t1 - t0, ch.planned_bytes(plan))


def _numpy_decode(version, blob, shape, kind):
    w, h, f = shape
    info, _, rgb = _reference_decode(version, blob, shape, kind)
    return info, np.asarray(rgb).reshape(f, h, w, 3)


# ---- 1. the case table ----
@pytest.mark.parametrize("version", [2, 3, 4])
@pytest.mark.parametrize("shape", RF.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_case_table_equals_the_numpy_decode_and_does_partial_work(gpu_codec, shape, version):
    a = gpu_codec
    w, h, f = shape
    for kind in RF.WAVELETS:
        q = QUALITIES[version][(RF.SHAPES.index(tuple(shape)) + kind) % len(QUALITIES[version])]
        rgb = WO.smooth_plus_noise(w, h, f, seed=w * 7 + f)
        blob = _encode(a, version, rgb, w, h, f, q, kind)
        _, full = _numpy_decode(version, blob, shape, kind)
        ch = Rects(a, blob, shape, kind, version)
        for rect in RF.rects_for(shape, kind):
            assert a.rect_window(a.WaveletType(kind), w, h, *rect) == tuple(
                v for win in RF.windows(kind, w, h, f, 0, 1, rect)[:0:-1] for v in win)
        _check(a, ch, full, L, RF.cases_for(shape, kind), RF.named_rects(shape, kind), (shape, version, kind, q))


# ---- 2. pitched destinations and the paths of the paste kernel ----
@pytest.fixture
def grid_cap(gpu_codec):
    lib = gpu_codec.load_library()
    yield lambda max_blocks: lib.alice_codec_test_set_grid_cap(max_blocks)
    lib.alice_codec_test_set_grid_cap(0)


@pytest.mark.parametrize("version,kind", [(2, RF.CDF97), (3, RF.CDF53), (4, RF.HAAR)])
def test_paste_into_full_size_frames(gpu_codec, version, kind):
    """The rectangle pasted at its own place into full-size frames that hold a pattern: the frames afterwards are the pattern
    with the rectangle's pixels, and nothing else."""
    a = gpu_codec
    for shape in ((50, 38, 13), (64, 64, 16), (33, 17, 5)):
        w, h, f = shape
        rgb = WO.smooth_plus_noise(w, h, f, seed=w * 7 + f)
        blob = _encode(a, version, rgb, w, h, f, QUALITIES[version][1], kind)
        _, full = _numpy_decode(version, blob, shape, kind)
        ch = Rects(a, blob, shape, kind, version)
        for rect in RF.rects_for(shape, kind):
            x, y, rw, rh = rect
            for t0, t1 in ((0, f), (f // 2, f // 2 + 2)):
                got = ch.dev(t0, t1, rect, at=3 * (y * w + x), row_pitch=3 * w, frame_pitch=3 * w * h)
                assert np.array_equal(got, _crop(full, t0, t1, rect)), (shape, version, rect, (t0, t1))
                _check_stats(a, RF.rect_plan(kind, w, h, f, L, t0, t1, rect, classes=False), t1 - t0, 0)


def test_paste_kernel_paths_and_grid_wrap(gpu_codec, grid_cap):
    """64x64x16 (Haar: a halo of 2): with a full-width rectangle the temporary's rows are 192 bytes at multiples of 16, so a
    destination at a multiple of 16 with pitches that are multiples of 16 takes the 16-byte copies, one at a multiple of 4
    the dword copies, any other the byte copies; x = 1 .. 5 and odd 3 w start the source rows at every residue.  Rows of 16
    bytes and more end in a byte tail when 3 w is no multiple of the piece.  A grid cap of 1 and of 3 workgroups wraps the
    row loop."""
    a = gpu_codec
    shape, kind, version = (64, 64, 16), RF.HAAR, 3
    w, h, f = shape
    rgb = WO.smooth_plus_noise(w, h, f, seed=3)
    blob = _encode(a, version, rgb, w, h, f, 95, kind)
    _, full = _numpy_decode(version, blob, shape, kind)
    ch = Rects(a, blob, shape, kind, version, extra=4096)
    assert (ch.out.data_ptr() + GUARD) % 16 == 0
    # (1, 1, 62, 62): not the whole frame, but both windows span their axis: whole planes through the temporary and the paste
    assert RF.windows(kind, w, h, f, 5, 8, (1, 1, 62, 62))[1:] == ((0, 64), (0, 64))
    rects = [(0, 20, 64, 5), (0, 0, 64, 64), (1, 1, 62, 62), (0, 59, 64, 5)] + [(x, 7, rw, 3) for x in (1, 2, 3, 4, 5) for rw in (1, 2, 5, 16, 21)]
    t0, t1 = 5, 8
    for cap in (0, 1, 3):
        grid_cap(cap)
        for rect in rects if cap == 0 else rects[:6]:
            _, _, rw, rh = rect
            want = _crop(full, t0, t1, rect)
            for at, rp, fp in ((0, 0, 0), (0, 208, 208 * rh + 32), (4, 196, 196 * rh + 8), (1, 3 * rw + 5, (3 * rw + 5) * rh + 7),
                               (2, 3 * rw, 0), (0, 0, 3 * rw * rh + 48)):
                if rp and rp < 3 * rw:
                    continue
                got = ch.dev(t0, t1, rect, at=at, row_pitch=rp, frame_pitch=fp)
                assert np.array_equal(got, want), (cap, rect, at, rp, fp)


def test_whole_frame_rectangle_equals_the_frame_range_call(gpu_codec):
    a = gpu_codec
    for shape, kind, version in (((50, 38, 13), RF.CDF97, 2), ((33, 17, 5), RF.CDF53, 3), ((64, 64, 16), RF.HAAR, 4), ((5, 3, 7), RF.CDF97, 4)):
        w, h, f = shape
        rgb = WO.smooth_plus_noise(w, h, f, seed=w + f)
        blob = _encode(a, version, rgb, w, h, f, QUALITIES[version][1], kind)
        ch = Rects(a, blob, shape, kind, version)
        frames = torch.empty(f * h * w * 3, dtype=torch.uint8, device=DEV)
        for t0, t1 in FR.named_ranges(kind, f):
            a.frames_decode_device(ch.alc_view.data_ptr(), ch.alc_len, t0, t1 - t0, frames.data_ptr())
            fst = a._test_last_frames_stats()
            got = ch.dev(t0, t1, (0, 0, w, h))
            assert np.array_equal(got.reshape(-1), frames[:(t1 - t0) * h * w * 3].cpu().numpy()), (shape, version, (t0, t1))
            st = a._test_last_rect_stats()
            assert (st[0], st[1], st[6], st[8]) == (fst[0], fst[1], fst[2], fst[4])


# ---- 3. every inverse instance class at its edge steps ----
@pytest.mark.parametrize("version", [2, 3, 4])
@pytest.mark.parametrize("kind", RF.WAVELETS)
def test_instances_at_their_edge_steps(gpu_codec, kind, version):
    """104x40x16: the worst-sign volume (every sample at the largest magnitude the format decodes to) and a loud random
    one, at the first and last quantiser step of every instance class alice_codec_test_inverse_variant names, through one
    interior rectangle whose virtual chunk takes the tile path."""
    a = gpu_codec
    lib = a.load_library()
    shape = (104, 40, 16)
    w, h, f = shape
    m = RF.LIFT_STEPS[kind] + 2
    rect = (m + 1, m, w - 2 * m - 1, h - 2 * m)
    T = F.centre_frame(kind, shape)
    ranges = [(0, f), (T, T + 1), (T + 1, T + 2)]
    plan = RF.rect_plan(kind, w, h, f, F.LANE_SYMBOLS, T, T + 1, rect)
    assert {"x_interior", "y_interior", "virtual_tiles"} <= plan["classes"]
    ch = None
    for name, steps, v in F.cases(lib, kind, shape, version):
        assert F.variant(lib, kind, steps, version) == v
        blob = F.container(kind, shape, name, steps, version)
        if ch is None:
            ch = Rects(a, blob, shape, kind, version)
        else:
            ch.set_container(blob)
        full = np.asarray(F.reference(kind, shape, version, name, steps, 0, f)).reshape(f, h, w, 3)
        _check(a, ch, full, F.LANE_SYMBOLS, [(r, rect) for r in ranges], {rect} if name == "worst" else set(), (kind, version, name, steps, v))
        _ran.setdefault((version, kind), {}).setdefault(v, set()).add(tuple(steps))
    edges = F.class_edges(lib, kind, version)
    assert set(edges) == F.EXPECTED[version][kind]
    for v, edge in edges.items():
        assert edge <= _ran[(version, kind)][v], (version, kind, v, edge)


# ---- 4. lane sizes ----
@pytest.mark.parametrize("version,lane", [(v, n) for v in F.VERSIONS for n in F.LANE_SIZES[v]])
def test_lane_sizes(gpu_codec, version, lane):
    """128x96x40 encoded by the library at L = 128, 512, 2048 and the format's maximum (one partly filled block)"""
    a = gpu_codec
    shape = F.LANE_SHAPE
    w, h, f = shape
    kind = F.lane_kind(version, lane)
    rgb = WO.smooth_plus_noise(w, h, f, seed=40 + kind)
    blob = _encode(a, version, rgb, w, h, f, F.LANE_QUALITY[version], kind, lane)
    info, full = _numpy_decode(version, blob, shape, kind)
    assert info["lane_symbols"] == lane
    ch = Rects(a, blob, shape, kind, version)
    rects = [(0, 0, w, h), (37, 21, 50, 40), (w // 2, h // 2, 1, 1), (w - 5, 0, 5, 4)]
    cases = [(r, rect) for rect in rects for r in ((0, 1), (19, 21), (f - 1, f), (0, f))]
    _check(a, ch, full, lane, cases, {rects[1]}, (version, lane, kind))


# ---- 5. damage ----
@pytest.mark.parametrize("version", [2, 3, 4])
def test_damage(gpu_codec, version):
    """160x104x6, L = 64: a plane is 4.06 blocks, and a small rectangle leaves the blocks between a plane's low and high rows
    and the planes outside the window unplanned."""
    a = gpu_codec
    shape, kind = (160, 104, 6), RF.CDF53
    w, h, f = shape
    rgb = WO.smooth_plus_noise(w, h, f, seed=11)
    blob = _encode_ref(version, rgb, w, h, f, {2: 96, 3: 100, 4: 100}[version], kind, L)      # small steps: no short lanes
    _, full = _numpy_decode(version, blob, shape, kind)
    ch = Rects(a, blob, shape, kind, version)
    t0, t1, rect = 2, 3, (70, 40, 9, 7)
    plan = RF.rect_plan(kind, w, h, f, L, t0, t1, rect)
    assert {"gap_inside_plane", "blocks_skipped"} <= plan["classes"]
    outside = [b for b in range(plan["n_blocks"]) if b not in plan["planned"]]
    assert outside
    want = _crop(full, t0, t1, rect)
    assert np.array_equal(ch.dev(t0, t1, rect), want)
    stats = a._test_last_rect_stats()
    full_decode = {2: a.decode_split, 3: a.decode_wide, 4: a.decode_reversible}[version]

    # a lane of a planned block: refused by both calls, the output untouched, the stats unchanged
    for channel, block in ((0, plan["planned"][0]), (2, plan["planned"][-1])):
        bad = _lane_flip(version, blob, channel, block)
        ch.set_container(bad)
        ch.out.copy_(ch.pattern)
        with pytest.raises(a.CodecError) as e:
            ch.call(t0, t1, rect)
        assert e.value.code == 4 and "end check" in str(e.value)
        assert ch.untouched(), "a refused rectangle wrote to its output"
        with pytest.raises(a.CodecError) as e:
            a.decode_rect(bad, t0, t1 - t0, *rect)
        assert e.value.code == 4
        assert a._test_last_rect_stats() == stats, "a refused call must not report work"

    # a lane of a block outside the plan: not seen, the pixels are the clean file's; the full decode refuses the file
    inside_gap = [b for b in outside if plan["planned"][0] < b < plan["planned"][-1]]
    for channel, block in ((0, outside[0]), (1, inside_gap[0]), (2, outside[-1])):
        bad = _lane_flip(version, blob, channel, block)
        ch.set_container(bad)
        assert np.array_equal(ch.dev(t0, t1, rect), want)
        assert np.array_equal(np.asarray(a.decode_rect(bad, t0, t1 - t0, *rect)), want.reshape(-1))
        with pytest.raises(a.CodecError) as e:
            full_decode(bad)
        assert e.value.code == 4

    # a block-length entry anywhere (here: of an unplanned block): the scan covers the whole table
    _, lay = _channel_layout(blob)
    for delta in (1, -1):
        bad = bytearray(blob)
        pos = lay[1][0] + 4 * outside[0]
        v = int.from_bytes(bad[pos:pos + 4], "little") + delta
        bad[pos:pos + 4] = v.to_bytes(4, "little")
        ch.set_container(bytes(bad))
        ch.out.copy_(ch.pattern)
        with pytest.raises(a.CodecError) as e:
            ch.call(t0, t1, rect)
        assert e.value.code == 4 and "directory" in str(e.value)
        assert ch.untouched()
        with pytest.raises(a.CodecError) as e:
            a.decode_rect(bytes(bad), t0, t1 - t0, *rect)
        assert e.value.code == 4
    ch.set_container(blob)
    assert np.array_equal(ch.dev(t0, t1, rect), want), "a refusal left something behind"


# ---- 6. refusals ----
def test_refusals_write_nothing(gpu_codec):
    a = gpu_codec
    shape, kind = (33, 17, 5), RF.CDF97
    w, h, f = shape
    rgb = WO.smooth_plus_noise(w, h, f)
    blob = _encode(a, 3, rgb, w, h, f, 80, kind)
    ch = Rects(a, blob, shape, kind, 3)
    ch.out.copy_(ch.pattern)
    a.decode_rect(blob, 0, 1, 2, 3, 4, 5)
    stats = a._test_last_rect_stats()
    assert stats[:6] == (0, 6, 0, 10, 0, 12) and stats[8] == 1

    def refused(code, t0, count, rect, rp=0, fp=0, length=None, match=None):
        with pytest.raises(a.CodecError) as e:
            a.rect_decode_device(ch.alc_view.data_ptr(), ch.alc_len if length is None else length, t0, count, *rect,
                                 ch.out.data_ptr() + GUARD, rp, fp)
        assert e.value.code == code, (t0, count, rect, rp, fp, str(e.value))
        if match:
            assert match in str(e.value), str(e.value)
        assert ch.untouched()

    for first, count in ((0, 0), (0, f + 1), (f, 1), (3, 3)):
        refused(2, first, count, (0, 0, 1, 1), match="frames")
        refused(2, first, count, (0, 0, 0, 0), match="frames")             # the range comes before the rectangle
    for rect in ((0, 0, 0, 1), (0, 0, 1, 0), (w, 0, 1, 1), (0, h, 1, 1), (1, 0, w, 1), (0, 1, 1, h), (0xFFFFFFFF, 0, 2, 1),
                 (0, 0xFFFFFFFF, 1, 2)):
        refused(2, 0, 1, rect, match="rectangle")
        refused(2, 0, 1, rect, rp=1, fp=1, match="rectangle")              # the rectangle comes before the pitches
    for rp, fp in ((3 * 4 - 1, 0), (3 * 4 - 1, 1 << 20), (3 * 4, 3 * 4 * 5 - 1), (64, 64 * 5 - 1), (0, 3 * 4 * 5 - 1), (1 << 63, 1 << 63)):
        refused(2, 0, 2, (2, 3, 4, 5), rp=rp, fp=fp, match="pitches")
    ch.set_container(o.encode(rgb, w, h, f, 80, kind))
    refused(4, 0, 1, (0, 0, 1, 1), match="version 1 has no random access (one serial chain per channel)")
    refused(4, 0, 0, (0, 0, 0, 0), match="version 1 has no random access")
    for damage in ((0, ord("B")), (5, 7), (18, 3)):       # magic, wavelet byte, lane_symbols
        bad = bytearray(blob)
        bad[damage[0]] = damage[1]
        ch.set_container(bytes(bad))
        refused(4, 0, 1, (0, 0, 1, 1))
    ch.set_container(blob)
    refused(4, 0, 1, (0, 0, 1, 1), length=ch.alc_len - 1)                   # a container cut short
    with pytest.raises(a.CodecError) as e:
        a.rect_decode_device(ch.alc_view.data_ptr(), ch.alc_len, 0, 1, 0, 0, 1, 1, 0)
    assert e.value.code == 9
    assert a._test_last_rect_stats() == stats, "a refused call must not report work"
    # and the accepted edge of the pitch rule
    got = ch.dev(0, 2, (2, 3, 4, 5), row_pitch=12, frame_pitch=60)
    _, full = _numpy_decode(3, blob, shape, kind)
    assert np.array_equal(got, _crop(full, 0, 2, (2, 3, 4, 5)))
