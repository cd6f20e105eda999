"""Many frame ranges and rectangles in one call on the MI355X: alice_codec_dev_decode_rects and
alice_codec_decode_rects against the numpy full decode cropped to [t0, t1) x rectangle, bit for bit, and the statistics of
the call against the sums of the plans of tests/rect_ref.py -- neither is the library's own single call (one test holds the
batch against the loop of single calls as well).  Symbols come from the reference lane decoders or are the volumes the
containers were written from, the pixels from the numpy inverses.  Every item's output sits between guard bytes of one
buffer, every second one at an odd address; every container sits at an odd device address.  Lane size 64 unless stated."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle.alice_oracle_np as o  # noqa: E402
import frames_extreme_cases as F  # noqa: E402
import rect_ref as RF  # noqa: E402
import temporal_cases as TC  # noqa: E402
import wide_oracle as WO  # noqa: E402
from test_frames_host import _encode_ref  # noqa: E402
from test_gpu_frames import DEV, GUARD, HEADER, QUALITIES, _channel_layout, _encode, _guard_pattern, _info, _lane_flip  # noqa: E402
from test_gpu_frames_extremes import _reference_decode  # noqa: E402

pytestmark = pytest.mark.gpu

L = RF.LANE
_containers = {}


def _container(a, shape, kind, version, q=None, seed=None, reference_encoder=False):
    """(blob, steps, full (f, h, w, 3) numpy decode), once per container for all tests of this module"""
    key = (tuple(shape), kind, version, q, seed, reference_encoder)
    if key not in _containers:
        w, h, f = shape
        quality = QUALITIES[version][1] if q is None else q
        rgb = WO.smooth_plus_noise(w, h, f, seed=w * 7 + f if seed is None else seed)
        blob = _encode_ref(version, rgb, w, h, f, quality, kind, L) if reference_encoder else _encode(a, version, rgb, w, h, f, quality, kind)
        info, _, full = _reference_decode(version, blob, shape, kind)
        full = np.asarray(full).reshape(f, h, w, 3)
        full.setflags(write=False)
        _containers[key] = (bytes(blob), tuple(info["step"]), full)
    return _containers[key]


class Item:
    """One request: the rectangle `rect` = (x, y, w, h) of frames [t0, t1) of `blob`, or (rect None) the whole frames as a
    frame-range item (x = y = w = h = 0).  Items that pass the same blob object name one container."""

    def __init__(self, blob, shape, kind, version, steps, full, t0, t1, rect=None, lane=L):
        self.blob, self.shape, self.kind, self.version, self.steps, self.full = blob, tuple(shape), kind, version, tuple(steps), full
        self.t0, self.t1, self.lane, self.rect = t0, t1, lane, rect
        w, h, _ = self.shape
        self.box = tuple(rect) if rect is not None else (0, 0, w, h)
        self.bytes = (t1 - t0) * self.box[2] * self.box[3] * 3
        self._plan = None

    def want(self):
        x, y, rw, rh = self.box
        return self.full[self.t0:self.t1, y:y + rh, x:x + rw].reshape(-1)

    def plan(self):
        if self._plan is None:
            w, h, f = self.shape
            self._plan = RF.rect_plan(self.kind, w, h, f, self.lane, self.t0, self.t1, self.box, classes=False)
        return self._plan

    def call_rect(self):
        return (0, 0, 0, 0) if self.rect is None else tuple(self.rect)

    @property
    def whole(self):
        return self.box == (0, 0, self.shape[0], self.shape[1])

    def planes(self):
        p = self.plan()
        return p["xa"] == 0 and p["xb"] == p["dims"][0] and p["ya"] == 0 and p["yb"] == p["dims"][1]

    def vdims(self):
        """(width, height) of the virtual chunk's planes"""
        p = self.plan()
        return p["dims"][:2] if self.whole else p["vdims"][:2]

    def generic(self):
        return min(self.vdims()) < 6

    def tiles(self):
        """tiles of the tile role: 96 x 32 over the real size of the virtual chunk, per kept frame"""
        p = self.plan()
        vw, vh = (self.shape[0], self.shape[1]) if self.whole else p["vdims"][:2]
        return -(-vw // 96) * -(-vh // 32) * (self.t1 - self.t0)


class Batch:
    """The distinct containers of the items at odd device addresses of one arena, the outputs between guard bytes of 0 and
    255 in one buffer, the gaps alternately GUARD and GUARD + 1 bytes so that every other output starts at an odd address."""

    def __init__(self, a, items):
        self.a, self.items = a, list(items)
        blobs = {}
        for it in self.items:
            blobs.setdefault(id(it.blob), it.blob)
        self.arena = torch.empty(sum(len(b) + 2 for b in blobs.values()) + 8, dtype=torch.uint8, device=DEV)
        pos = 1 if self.arena.data_ptr() % 2 == 0 else 2
        self.at = {}
        for key, blob in blobs.items():
            self.at[key] = pos
            self.put(key, blob)
            pos += len(blob) + (2 if len(blob) % 2 == 0 else 1)
        assert all((self.arena.data_ptr() + p) % 2 == 1 for p in self.at.values())
        self.off, pos = [], GUARD
        for k, it in enumerate(self.items):
            self.off.append(pos)
            pos += it.bytes + GUARD + (k & 1)
        self.out = torch.empty(pos, dtype=torch.uint8, device=DEV)
        self.pattern = _guard_pattern(pos)
        if len(self.items) > 2:
            assert {(self.out.data_ptr() + p) % 2 for p in self.off} == {0, 1}

    def put(self, key, blob):
        raw = np.frombuffer(bytes(blob), np.uint8)
        self.arena[self.at[key]:self.at[key] + raw.size].copy_(torch.from_numpy(raw.copy()))

    def dst(self):
        return [self.out.data_ptr() + p for p in self.off]

    def rows(self):
        return [(self.arena.data_ptr() + self.at[id(it.blob)], len(it.blob), it.t0, it.t1 - it.t0, *it.call_rect(),
                 self.out.data_ptr() + self.off[k], 0, 0) for k, it in enumerate(self.items)]

    def run(self, rows=None):
        """-> every item's bytes as numpy, after everything between and around the outputs was checked"""
        self.out.copy_(self.pattern)
        self.a.rects_decode_device(self.rows() if rows is None else rows)
        torch.cuda.synchronize()
        mask = torch.ones(self.out.numel(), dtype=torch.bool, device=DEV)
        for k, it in enumerate(self.items):
            mask[self.off[k]:self.off[k] + it.bytes] = False
        assert torch.equal(self.out[mask], self.pattern[mask]), "bytes outside the outputs were written"
        host = self.out.cpu().numpy()
        return [host[self.off[k]:self.off[k] + it.bytes] for k, it in enumerate(self.items)]

    def refused(self, rows=None):
        """-> the CodecError of a call that must be refused and must have written nothing"""
        self.out.copy_(self.pattern)
        with pytest.raises(self.a.CodecError) as e:
            self.a.rects_decode_device(self.rows() if rows is None else rows)
        torch.cuda.synchronize()
        assert torch.equal(self.out, self.pattern), "a refused call wrote to an output"
        return e.value

    def check(self, where=""):
        got = self.run()
        for k, it in enumerate(self.items):
            want = it.want()
            bad = np.flatnonzero(got[k] != want)
            assert bad.size == 0, (where, k, it.shape, it.version, it.kind, (it.t0, it.t1), it.rect, bad.size, bad[:4].tolist())
        return got


def _paste_piece(it, dst, row_pitch=0, frame_pitch=0):
    """the piece width the paste of a rectangle takes: the single launcher's alignment test on the packed temporary (a
    256-byte aligned sub-range of a pool buffer) and on the destination"""
    p = it.plan()
    x, y, rw, rh = it.box
    vw, vh = p["vdims"][:2]
    rp = row_pitch or 3 * rw
    fp = frame_pitch or rp * rh
    bits = ((y - p["ya"]) * 3 * vw + 3 * (x - p["xa"])) | 3 * vw | 3 * vw * vh | dst | rp | fp
    if bits % 16 == 0 and 3 * rw >= 16:
        return 16
    return 4 if bits % 4 == 0 and 3 * rw >= 4 else 1


def _finish_launches(lib, items, dst, pitches=None, fallback=()):
    """the launches of the batched finish: the temporal, tile and paste classes present among the items it takes"""
    t_cls, xy_cls, pieces = set(), set(), set()
    for k, it in enumerate(items):
        if it.generic() or k in fallback:
            continue
        v = F.variant(lib, it.kind, it.steps, it.version)
        ns4 = it.kind == RF.CDF97
        t_cls.add((ns4, min(v, 2), it.version))
        xy_cls.add((ns4, v, it.version == 4))
        if not it.whole:
            pieces.add(_paste_piece(it, dst[k], *(pitches[k] if pitches else (0, 0))))
    return len(t_cls) + len(xy_cls) + len(pieces)


def _check_stats(a, items, containers, dst, uploaded=0, pitches=None, fallback=None):
    s = a._test_last_rects_stats()
    lib = a.load_library()
    plans = [it.plan() for it in items]
    groups = {(it.planes(), it.version == 2) for it in items}
    cut = set() if fallback is None else set(fallback)
    assert s[0] == len(items) and s[1] == containers, s
    assert s[2] == 1, ("table launches", s)
    assert s[3] == len(groups) <= 4, ("lane launches", s, groups)
    assert s[4] == _finish_launches(lib, items, dst, pitches, cut), ("finish launches", s)
    assert s[5] == sum(1 for k, it in enumerate(items) if it.generic() or k in cut), ("per-item finishes", s)
    assert s[6] <= 3, ("stream drains", s)
    assert s[7] == sum(3 * p["n_planned"] for p in plans), ("blocks", s)
    assert s[8] == uploaded, ("uploaded", s)
    assert s[9] == sum(p["stored"] for p in plans), ("stored", s)
    assert s[10] == sum(it.t1 - it.t0 for it in items), ("frames", s)


def _planned_bytes(a, version, blob, planned):
    info = _info(a, version, blob)
    pos, total = HEADER, 0
    for c in range(3):
        table = np.frombuffer(blob, "<u4", info.n_blocks[c], pos)
        total += int(table[sorted(planned)].astype(np.int64).sum())
        pos += info.payload_len[c]
    return total


def _host(a, items):
    """the host call on the items -> the outputs; the hook held to the union of the plans per container"""
    got = a.decode_rects([(it.blob, it.t0, it.t1 - it.t0) if it.rect is None else (it.blob, it.t0, it.t1 - it.t0, *it.rect) for it in items])
    for k, it in enumerate(items):
        assert np.array_equal(np.asarray(got[k]), it.want()), ("host call", k, it.shape, it.rect)
    union = {}
    for it in items:
        union.setdefault(id(it.blob), (it, set()))[1].update(it.plan()["planned"])
    uploaded = sum(_planned_bytes(a, it.version, it.blob, planned) for it, planned in union.values())
    offsets = np.cumsum([0] + [it.bytes for it in items])[:-1].tolist()
    _check_stats(a, items, len(union), offsets, uploaded=uploaded)
    return got


def _item(a, shape, kind, version, t0, t1, rect=None, q=None, seed=None):
    blob, steps, full = _container(a, shape, kind, version, q, seed)
    return Item(blob, shape, kind, version, steps, full, t0, t1, rect)


# ---- 1. the mixed batch ----
def _picks(si, shape, kind, version):
    """two (range, rectangle) cases of the shape's table, walking with the version and the wavelet; the shape with an
    interior tile also gives its whole frame"""
    cases = RF.cases_for(shape, kind)
    out = [cases[(5 * si + 3 * version + kind) % len(cases)], cases[(7 * si + version + 2 * kind + 11) % len(cases)]]
    if shape == (224, 104, 4):
        out.append(cases[(version + kind) % len(RF.ranges_for(shape))])
    return out


@pytest.mark.parametrize("kind", RF.WAVELETS)
@pytest.mark.parametrize("version", [2, 3, 4])
def test_case_table_in_one_call(gpu_codec, version, kind):
    """every shape of rect_ref's case table, a rectangle and a range each, the picks walking through the table's rectangles
    so that over the nine cases every plan class of section 16.6 appears"""
    a = gpu_codec
    items = []
    for si, shape in enumerate(RF.SHAPES):
        q = QUALITIES[version][(si + kind) % len(QUALITIES[version])]
        for (t0, t1), rect in _picks(si, shape, kind, version):
            items.append(_item(a, shape, kind, version, t0, t1, rect, q=q))
    batch = Batch(a, items)
    batch.check((version, kind))
    _check_stats(a, items, len(RF.SHAPES), batch.dst())
    assert any(it.generic() for it in items) and any(not it.generic() and not it.whole for it in items)
    _host(a, items)


def test_plan_classes_of_the_case_table_picks():
    """the picks of the test above, over its nine cases, meet every class rect_ref requires of the case table"""
    seen = set()
    for version in (2, 3, 4):
        for kind in RF.WAVELETS:
            for si, shape in enumerate(RF.SHAPES):
                for (t0, t1), rect in _picks(si, shape, kind, version):
                    seen |= RF.rect_plan(kind, *shape, L, t0, t1, rect)["classes"]
    assert RF.REQUIRED_CLASSES <= seen, RF.REQUIRED_CLASSES - seen


def test_versions_and_wavelets_mixed_in_one_call(gpu_codec):
    a = gpu_codec
    items = []
    for si, shape in enumerate([(64, 64, 16), (50, 38, 13), (33, 17, 5), (5, 3, 7), (40, 24, 1)]):
        for version in (2, 3, 4):
            kind = RF.WAVELETS[(si + version) % 3]
            q = QUALITIES[version][(si + kind) % len(QUALITIES[version])]
            cases = RF.cases_for(shape, kind)
            (t0, t1), rect = cases[(3 * si + version) % len(cases)]
            items.append(_item(a, shape, kind, version, t0, t1, rect, q=q))
            items.append(_item(a, shape, kind, version, shape[2] // 2, shape[2] // 2 + 1, None, q=q))
    batch = Batch(a, items)
    batch.check("mixed")
    _check_stats(a, items, 15, batch.dst())
    assert a._test_last_rects_stats()[3] == 4, "planes and boxes of both symbol widths"
    _host(a, items)


# ---- 2. the edges of the work lists ----
@pytest.mark.parametrize("version,kind", [(2, RF.HAAR), (3, RF.CDF53), (4, RF.HAAR)])
def test_one_tile_beside_an_interior_tile(gpu_codec, version, kind):
    """224x104x4: the whole frame (a tile with neighbours on every side) beside a 1 x 1 rectangle whose virtual chunk is 6 x 6
    (one tile, one workgroup of each role), in both orders and alone"""
    a = gpu_codec
    shape = (224, 104, 4)
    big = _item(a, shape, kind, version, 1, 3, (0, 0, 224, 104))
    small = _item(a, shape, kind, version, 2, 3, (112, 52, 1, 1))
    assert small.plan()["vdims"][:2] == (6, 6) and small.tiles() == 1
    assert big.plan()["vdims"][0] >= 196 and big.plan()["vdims"][1] >= 68
    for order in ([big, small], [small, big], [small], [big]):
        batch = Batch(a, order)
        batch.check((version, kind, len(order)))
        _check_stats(a, order, 1, batch.dst())


@pytest.mark.parametrize("version,kind", [(2, RF.CDF97), (4, RF.CDF53)])
def test_tile_totals_and_record_counts(gpu_codec, version, kind):
    """33x17x5 is one tile per frame: totals of 1, 7, 8 and 9 tiles (the padding of the XCD order empty, partial and full), and
    lists of 3 and of 5 records (odd and even splits of the bisection)"""
    a = gpu_codec
    shape = (33, 17, 5)
    for counts in ([1], [5, 2], [5, 3], [5, 4], [1, 1, 1], [1, 2, 1, 3, 1], [2, 1, 1, 2, 1, 1, 1, 1]):
        items = []
        for i, n in enumerate(counts):
            t0 = (i * 2) % (shape[2] - n + 1)
            items.append(_item(a, shape, kind, version, t0, t0 + n, None if i % 2 == 0 else (0, 0, 33, 17)))
        assert sum(it.tiles() for it in items) == sum(counts)
        batch = Batch(a, items)
        batch.check((version, kind, counts))
        _check_stats(a, items, 1, batch.dst())


# ---- 3. whole-frame items ----
def test_whole_frame_items_equal_the_frame_range_call(gpu_codec):
    a = gpu_codec
    for shape, kind, version in (((50, 38, 13), RF.CDF97, 2), ((33, 17, 5), RF.CDF53, 3), ((64, 64, 16), RF.HAAR, 4), ((5, 3, 7), RF.CDF97, 4)):
        w, h, f = shape
        ranges = [(0, 1), (f - 1, f), (0, f), (f // 2, f // 2 + 2)]
        items = [_item(a, shape, kind, version, t0, t1, None) for t0, t1 in ranges]
        batch = Batch(a, items)
        got = batch.check((shape, version))
        _check_stats(a, items, 1, batch.dst())
        explicit = [_item(a, shape, kind, version, t0, t1, (0, 0, w, h)) for t0, t1 in ranges]
        again = Batch(a, explicit).check((shape, version, "explicit"))
        frames = torch.empty(f * h * w * 3, dtype=torch.uint8, device=DEV)
        for k, (t0, t1) in enumerate(ranges):
            a.frames_decode_device(batch.arena.data_ptr() + batch.at[id(items[k].blob)], len(items[k].blob), t0, t1 - t0, frames.data_ptr())
            single = frames[:(t1 - t0) * h * w * 3].cpu().numpy()
            assert np.array_equal(got[k], single) and np.array_equal(again[k], single), (shape, version, (t0, t1))


# ---- 4. the mosaic and the paste widths ----
def test_mosaic_of_four_containers(gpu_codec):
    """four 20 x 12 crops of two frames from four containers pasted 2 x 2 into one 40 x 24 pitched surface that holds a
    pattern: the surface afterwards is the pattern with the four rectangles, and nothing else"""
    a = gpu_codec
    picks = [((64, 64, 16), RF.HAAR, 2, (9, 30, 20, 12)), ((50, 38, 13), RF.CDF97, 3, (30, 0, 20, 12)),
             ((160, 104, 6), RF.CDF53, 4, (70, 40, 20, 12)), ((224, 104, 4), RF.HAAR, 3, (100, 92, 20, 12))]
    items = [_item(a, shape, kind, version, 1, 3, rect) for shape, kind, version, rect in picks]
    batch = Batch(a, items)
    rp, fp = 3 * 40 + 8, (3 * 40 + 8) * 24 + 40
    surface = torch.empty(2 * GUARD + 2 * fp, dtype=torch.uint8, device=DEV)
    pattern = _guard_pattern(surface.numel())
    surface.copy_(pattern)
    base = surface.data_ptr() + GUARD
    at = [j * 12 * rp + i * 60 for j in range(2) for i in range(2)]
    rows = [r[:8] + (base + at[k], rp, fp) for k, r in enumerate(batch.rows())]
    a.rects_decode_device(rows)
    torch.cuda.synchronize()
    got = surface.cpu().numpy()
    want = pattern.cpu().numpy().copy()
    for k, it in enumerate(items):
        idx = GUARD + at[k] + np.arange(2)[:, None, None] * fp + np.arange(12)[None, :, None] * rp + np.arange(60)[None, None, :]
        want[idx.reshape(-1)] = it.want()
    assert np.array_equal(got, want)
    _check_stats(a, items, 4, [base + x for x in at], pitches=[(rp, fp)] * 4)
    # one tile shifted by one pixel into its neighbour: refused, naming the later item, nothing written
    surface.copy_(pattern)
    shifted = list(rows)
    shifted[1] = rows[1][:8] + (rows[1][8] - 3, rp, fp)
    with pytest.raises(a.CodecError) as e:
        a.rects_decode_device(shifted)
    assert e.value.code == 2 and e.value.bad_item == 1 and "overlaps" in str(e.value)
    torch.cuda.synchronize()
    assert torch.equal(surface, pattern)


def test_three_paste_widths_with_their_tails(gpu_codec):
    """64x64x16 Haar: (0, 0, 13, 9) has a temporary of 16-pixel rows at offset 0, so with a destination and pitches at multiples
    of 16 its 39-byte rows are two 16-byte pieces and a tail of 7; at multiples of 4, nine dwords and a tail of 3; anywhere
    else bytes.  Two items of each width in one call: three paste launches."""
    a = gpu_codec
    shape, kind, version = (64, 64, 16), RF.HAAR, 3
    rect = (0, 0, 13, 9)
    items = [_item(a, shape, kind, version, t0, t0 + 2, rect) for t0 in (0, 3, 5, 8, 11, 14)]
    assert items[0].plan()["vdims"][:2] == (16, 12)
    batch = Batch(a, items)
    slot = 4096
    buf = torch.empty(2 * GUARD + 6 * slot + 16, dtype=torch.uint8, device=DEV)
    pattern = _guard_pattern(buf.numel())
    buf.copy_(pattern)
    base = buf.data_ptr() + GUARD
    base += -base % 16
    layouts = [(0, 64, 64 * 9 + 16), (0, 48, 0), (4, 44, 44 * 9 + 4), (8, 40, 0), (1, 39, 0), (2, 41, 41 * 9 + 3)]
    dst = [base + k * slot + off for k, (off, _, _) in enumerate(layouts)]
    pitches = [(rp, fp) for _, rp, fp in layouts]
    assert [_paste_piece(it, d, *p) for it, d, p in zip(items, dst, pitches)] == [16, 16, 4, 4, 1, 1]
    a.rects_decode_device([r[:8] + (dst[k], *pitches[k]) for k, r in enumerate(batch.rows())])
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    want = pattern.cpu().numpy().copy()
    for k, it in enumerate(items):
        rp = pitches[k][0]
        fp = pitches[k][1] or rp * 9
        idx = dst[k] - buf.data_ptr() + np.arange(2)[:, None, None] * fp + np.arange(9)[None, :, None] * rp + np.arange(39)[None, None, :]
        want[idx.reshape(-1)] = it.want()
    assert np.array_equal(got, want)
    _check_stats(a, items, 1, dst, pitches=pitches)


# ---- 5. many items of one container ----
@pytest.mark.parametrize("version,kind", [(2, RF.CDF53), (3, RF.CDF97), (4, RF.HAAR)])
def test_every_range_of_one_container_crossed_with_two_rectangles(gpu_codec, version, kind):
    a = gpu_codec
    shape = (50, 38, 13)
    f = shape[2]
    items = [_item(a, shape, kind, version, t0, t1, rect) for t0 in range(f) for t1 in range(t0 + 1, f + 1)
             for rect in ((7, 5, 11, 9), (31, 20, 19, 18))]
    batch = Batch(a, items)
    batch.check((version, kind))
    _check_stats(a, items, 1, batch.dst())
    _host(a, items)
    few = [it for it in items if it.t1 <= 2 and it.rect == (7, 5, 11, 9)]
    _host(a, few)
    assert a._test_last_rects_stats()[8] < _planned_bytes(a, version, items[0].blob, set().union(*[it.plan()["planned"] for it in items]))


# ---- 6. the instance classes of the inverse ----
@pytest.mark.parametrize("version", [2, 3, 4])
@pytest.mark.parametrize("kind", RF.WAVELETS)
def test_instances_at_their_edge_steps_in_one_call(gpu_codec, kind, version):
    """104x40x16: the worst-sign volume and a loud random one at the first and last quantiser step of every instance class,
    one interior rectangle of the centre frame each, ALL IN ONE CALL: every class present runs its `many` instance, and the
    classes are mixed"""
    a = gpu_codec
    lib = a.load_library()
    shape = (104, 40, 16)
    w, h, f = shape
    m = RF.LIFT_STEPS[kind] + 2
    rect = (m + 1, m, w - 2 * m - 1, h - 2 * m)
    T = F.centre_frame(kind, shape)
    items, ran = [], {}
    for name, steps, v in F.cases(lib, kind, shape, version):
        blob = F.container(kind, shape, name, steps, version)
        full = np.asarray(F.reference(kind, shape, version, name, steps, 0, f)).reshape(f, h, w, 3)
        items.append(Item(blob, shape, kind, version, steps, full, T, T + 1, rect, F.LANE_SYMBOLS))
        ran.setdefault(v, set()).add(tuple(steps))
    assert not items[0].generic() and not items[0].planes()
    for v, edge in F.class_edges(lib, kind, version).items():
        assert edge <= ran[v], (version, kind, v, edge)
    assert set(ran) == F.EXPECTED[version][kind] and len(ran) >= 2
    batch = Batch(a, items)
    batch.check((version, kind))
    _check_stats(a, items, len({id(it.blob) for it in items}), batch.dst())


# ---- 7. the frame-count classes ----
@pytest.mark.parametrize("kind", [RF.CDF97, RF.CDF53])
def test_every_frame_count_class_in_one_call(gpu_codec, kind):
    """12x10 at every frame count of tests/temporal_cases.py, one range each, the versions and the instance classes taking
    turns: the window bodies' peeled temporal loops under per-record planes, lo and hi"""
    a = gpu_codec
    lib = a.load_library()
    items, seen = [], set()
    for i, (w, h, f) in enumerate(s for s in TC.shapes() if s[:2] == TC.SHAPE):
        version = (2, 3, 4)[i % 3]
        cases = TC.step_cases(lib, kind, int(version != 2))
        steps, _ = cases[(i // 3) % len(cases)]
        blob = TC.container(kind, w, h, f, version, steps)
        full = np.asarray(TC.reference(kind, w, h, f, version, steps)).reshape(f, h, w, 3)
        rs = list(dict.fromkeys([(0, 1), (f - 1, f), (0, f), (f // 2, f // 2 + 1), (f // 3, f - f // 4)]))
        t0, t1 = rs[i % len(rs)]
        items.append(Item(blob, (w, h, f), kind, version, steps, full, t0, t1, None if i % 2 else (1, 1, 9, 7), TC.LANE_SYMBOLS))
        seen.add(TC.window_class(kind, f, t0, t1))
    assert len(seen) >= 6, seen
    batch = Batch(a, items)
    batch.check(kind)
    _check_stats(a, items, len(items), batch.dst())


# ---- 8. an inverse cut into bands ----
def test_band_cut_item_takes_the_per_item_path(gpu_codec):
    """Under a band target of 1 KiB the kept frames of the whole 64x64 frame (two tile rows, a padded width that is a multiple
    of 4) are cut into bands; the 12x12 and the 8x8 virtual chunks beside it are one tile row.  Same pixels, one per-item finish."""
    a = gpu_codec
    lib = a.load_library()
    shape, kind, version = (64, 64, 16), RF.HAAR, 2
    items = [_item(a, shape, kind, version, 4, 6, (10, 10, 8, 8)), _item(a, shape, kind, version, 3, 6, None),
             _item(a, shape, kind, version, 0, 1, (30, 31, 3, 2))]
    batch = Batch(a, items)
    clean = batch.check("uncut")
    _check_stats(a, items, 1, batch.dst())
    try:
        lib.alice_codec_test_set_tuning(1)
        cut = batch.check("cut")
        _check_stats(a, items, 1, batch.dst(), fallback={1})
        assert a._test_last_rects_stats()[5] == 1
    finally:
        lib.alice_codec_test_set_tuning(1024 * 1024)
    assert all(np.array_equal(x, y) for x, y in zip(clean, cut))


# ---- 9. the item limit ----
def test_item_limit(gpu_codec):
    a = gpu_codec
    shape, kind, version = (33, 17, 5), RF.CDF97, 3
    f = shape[2]
    rects = [None, (16, 8, 1, 1), (0, 0, 3, 17), (28, 0, 5, 4)]
    items = [_item(a, shape, kind, version, k % f, k % f + 1, rects[(k // f) % 4]) for k in range(1025)]
    batch = Batch(a, items[:1024])
    got = batch.run()
    for k in list(range(0, 1024, 37)) + [1023]:
        assert np.array_equal(got[k], items[k].want()), k
    _check_stats(a, items[:1024], 1, batch.dst())
    stats = a._test_last_rects_stats()
    e = Batch(a, items).refused()
    assert e.code == 2 and e.bad_item is None and "1025 items" in str(e)
    assert a._test_last_rects_stats() == stats


# ---- 10. refusals on the device path ----
@pytest.mark.parametrize("k", [0, 1, 3])
def test_refusals_write_nothing(gpu_codec, k):
    a = gpu_codec
    shape, kind = (33, 17, 5), RF.CDF97
    w, h, f = shape
    items = [_item(a, shape, kind, version, i, i + 1, rect, q=80, seed=version + i)
             for i, (version, rect) in enumerate(((2, (2, 3, 4, 5)), (3, None), (4, (0, 0, 33, 17)), (3, (20, 9, 6, 6))))]
    batch = Batch(a, items)
    batch.check("clean")
    stats = a._test_last_rects_stats()
    preview_stats, rect_stats = a._test_last_previews_stats(), a._test_last_rect_stats()
    rows = batch.rows()

    def with_row(row):
        r = list(rows)
        r[k] = tuple(row)
        return batch.refused(r)

    alc, length, first, count, x, y, rw, rh, out, rp, fp = rows[k]
    for bad_first, bad_count in ((0, 0), (0, f + 1), (f, 1), (3, 3)):
        e = with_row((alc, length, bad_first, bad_count, x, y, rw, rh, out, rp, fp))
        assert e.code == 2 and e.bad_item == k and f"item {k}: " in str(e) and "frames" in str(e)
    for rect in ((0, 0, 0, 1), (0, 0, 1, 0), (w, 0, 1, 1), (0, h, 1, 1), (1, 0, w, 1), (0, 1, 1, h), (0xFFFFFFFF, 0, 2, 1)):
        e = with_row((alc, length, first, count, *rect, out, 1, 1))           # the rectangle comes before the pitches
        assert e.code == 2 and e.bad_item == k and "rectangle" in str(e)
    for bad_rp, bad_fp in ((3 * 4 - 1, 0), (3 * 4, 3 * 4 * 5 - 1), (0, 3 * 4 * 5 - 1), (1 << 63, 1 << 63)):
        e = with_row((alc, length, first, count, 2, 3, 4, 5, out, bad_rp, bad_fp))
        assert e.code == 2 and e.bad_item == k and "pitches" in str(e)
    e = with_row((alc, length, first, count, x, y, rw, rh, None, rp, fp))
    assert e.code == 9 and e.bad_item == k
    e = with_row((None, length, first, count, x, y, rw, rh, out, rp, fp))
    assert e.code == 9 and e.bad_item == k
    e = with_row((alc, length - 1, first, count, x, y, rw, rh, out, rp, fp))   # a container cut short
    assert e.code == 4 and e.bad_item == k
    other = (k + 1) % len(rows)
    e = with_row((alc, length, first, count, x, y, rw, rh, rows[other][8] + items[other].bytes - 1, rp, fp))
    assert e.code == 2 and e.bad_item == max(k, other) and "overlaps" in str(e)
    v1 = o.encode(WO.smooth_plus_noise(w, h, f), w, h, f, 80, kind)
    d_v1 = torch.from_numpy(np.frombuffer(bytes(v1), np.uint8).copy()).to(DEV)
    e = with_row((d_v1.data_ptr(), len(v1), 0, 1, x, y, rw, rh, out, rp, fp))
    assert e.code == 4 and e.bad_item == k and "version 1 has no random access (one serial chain per channel)" in str(e)
    assert a._test_last_rects_stats() == stats, "a refused call must not report work"
    assert (a._test_last_previews_stats(), a._test_last_rect_stats()) == (preview_stats, rect_stats), "the other hooks are not this call's"
    batch.check("a refusal left something behind")


# ---- 11. damage ----
@pytest.mark.parametrize("version", [2, 3, 4])
def test_damage_refuses_the_whole_call(gpu_codec, version):
    """160x104x6, L = 64: a plane is 4.06 blocks, and a small rectangle leaves the blocks between a plane's low and high rows
    unplanned.  Five copies of the container, so that the damage is one item's alone."""
    a = gpu_codec
    shape, kind = (160, 104, 6), RF.CDF53
    q = {2: 96, 3: 100, 4: 100}[version]                         # small steps: no short lanes
    blob, steps, full = _container(a, shape, kind, version, q, seed=11, reference_encoder=True)
    asks = [((2, 3), (70, 40, 9, 7)), ((0, 1), (3, 3, 20, 10)), ((1, 2), (100, 80, 30, 20)), ((2, 3), (70, 40, 9, 7)), ((4, 6), (0, 50, 5, 5))]
    items = [Item(bytes(bytearray(blob)), shape, kind, version, steps, full, t0, t1, rect) for (t0, t1), rect in asks]
    assert len({id(it.blob) for it in items}) == 5
    batch = Batch(a, items)
    clean = batch.check("clean")
    _check_stats(a, items, 5, batch.dst())
    stats = a._test_last_rects_stats()
    k = 3
    plan = RF.rect_plan(kind, *shape, L, 2, 3, (70, 40, 9, 7))
    assert {"gap_inside_plane", "blocks_skipped"} <= plan["classes"]
    outside = [b for b in range(plan["n_blocks"]) if b not in plan["planned"]]
    gap = [b for b in outside if plan["planned"][0] < b < plan["planned"][-1]]
    key = id(items[k].blob)
    for channel, block in ((0, plan["planned"][0]), (2, plan["planned"][-1])):
        flipped = _lane_flip(version, blob, channel, block)
        batch.put(key, flipped)
        e = batch.refused()
        assert e.code == 4 and e.bad_item == k and "end check" in str(e), str(e)
        with pytest.raises(a.CodecError) as eh:
            a.decode_rects([(flipped if i == k else it.blob, it.t0, it.t1 - it.t0, *it.rect) for i, it in enumerate(items)])
        assert eh.value.code == 4 and eh.value.bad_item == k
    for channel, block in ((0, outside[0]), (1, gap[0]), (2, outside[-1])):     # a block item 3 does not plan: not seen
        batch.put(key, _lane_flip(version, blob, channel, block))
        got = batch.run()
        assert all(np.array_equal(x, y) for x, y in zip(got, clean))
    _, lay = _channel_layout(blob)
    bad = bytearray(blob)                                      # a block-length entry of a block nobody plans
    pos = lay[1][0] + 4 * outside[0]
    bad[pos:pos + 4] = (int.from_bytes(bad[pos:pos + 4], "little") + 1).to_bytes(4, "little")
    batch.put(key, bytes(bad))
    e = batch.refused()
    assert e.code == 4 and e.bad_item == k and "directory" in str(e)
    batch.put(key, blob)
    assert a._test_last_rects_stats() == stats, "a refused call must not report work"
    got = batch.run()
    assert all(np.array_equal(x, y) for x, y in zip(got, clean)), "a refusal left something behind"


# ---- 12. the batch against the loop of single calls ----
def test_batch_equals_the_loop_of_single_calls(gpu_codec):
    a = gpu_codec
    items = []
    for si, shape in enumerate([(64, 64, 16), (50, 38, 13), (33, 17, 5), (5, 3, 7), (160, 104, 6)]):
        for version in (2, 3, 4):
            kind = RF.WAVELETS[(si + version + 1) % 3]
            q = QUALITIES[version][(si + kind) % len(QUALITIES[version])]
            cases = RF.cases_for(shape, kind)
            (t0, t1), rect = cases[(5 * si + version) % len(cases)]
            items.append(_item(a, shape, kind, version, t0, t1, rect if (si + version) % 3 else None, q=q))
    batch = Batch(a, items)
    got = batch.check("batch")
    loop = torch.empty_like(batch.out)
    loop.copy_(batch.pattern)
    for k, (alc, length, first, count, x, y, rw, rh, out, _, _) in enumerate(batch.rows()):
        dst = loop.data_ptr() + batch.off[k]
        if items[k].rect is None:
            a.frames_decode_device(alc, length, first, count, dst)
        else:
            a.rect_decode_device(alc, length, first, count, x, y, rw, rh, dst)
    torch.cuda.synchronize()
    assert torch.equal(loop, batch.out)
