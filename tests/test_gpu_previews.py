"""Many previews in one call on the MI355X: alice_codec_dev_decode_previews and
alice_codec_decode_previews against the numpy restatement of tests/preview_ref.py, bit for bit, and the statistics of the
call against the plans of that module -- neither is the library's own single-item call.  Every item's output sits between
guard bytes of one buffer, every second one at an odd address; every container sits at an odd device address.  Lane size 64."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frames_extreme_cases as F  # noqa: E402
import preview_ref as PR  # noqa: E402
import temporal_cases as TC  # noqa: E402
import wide_oracle as WO  # noqa: E402
from test_gpu_frames import DEV, GUARD, HEADER, QUALITIES, _channel_layout, _encode, _guard_pattern, _info, _lane_flip  # noqa: E402
from test_gpu_frames_extremes import _symbols_of  # noqa: E402

pytestmark = pytest.mark.gpu

L = PR.LANE


class Item:
    """One request: frames [t0, t1) of `blob`; items that pass the same blob object name one container"""

    def __init__(self, blob, shape, kind, version, steps, syms, t0, t1, lane=L):
        self.blob, self.shape, self.kind, self.version, self.steps, self.syms = blob, tuple(shape), kind, version, tuple(steps), syms
        self.t0, self.t1, self.lane = t0, t1, lane
        qw, qh = PR.preview_dims(shape[0], shape[1])
        self.bytes = (t1 - t0) * qw * qh * 3

    def want(self):
        w, h, f = self.shape
        return PR.preview(self.syms, TC.dims(w, h, f), f, self.kind, self.steps, self.version, self.t0, self.t1)

    def plan(self):
        w, h, f = self.shape
        return PR.preview_plan(self.kind, w, h, f, self.lane, self.t0, self.t1)


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

    def rows(self):
        return [(self.arena.data_ptr() + self.at[id(it.blob)], len(it.blob), it.t0, it.t1 - it.t0, self.out.data_ptr() + self.off[k])
                for k, it in enumerate(self.items)]

    def run(self, rows=None):
        """-> every item's bytes as numpy, after everything between and around the outputs was checked"""
        self.out.copy_(self.pattern)
        self.a.previews_decode_device(self.rows() if rows is None else rows)
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
            self.a.previews_decode_device(self.rows() if rows is None else rows)
        torch.cuda.synchronize()
        assert torch.equal(self.out, self.pattern), "a refused call wrote to an output"
        return e.value

    def check(self, where=""):
        got = self.run()
        for k, it in enumerate(self.items):
            want = it.want()
            bad = np.flatnonzero(got[k] != want)
            assert bad.size == 0, (where, k, it.shape, it.version, it.kind, (it.t0, it.t1), bad.size, bad[:4].tolist())
        return got


def _finish_class(lib, it):
    """the instance class of the finish kernel: symbol format, lifting steps, exact or not"""
    return it.version, it.kind == PR.CDF97, F.variant(lib, it.kind, it.steps, it.version) == 0


def _check_stats(a, items, containers, finishes, uploaded=0, lanes=None):
    s = a._test_last_previews_stats()
    plans = [it.plan() for it in items]
    widths = {it.version == 2 for it in items}
    assert s[0] == len(items) and s[1] == containers, s
    assert s[2] == 1, ("table launches", s)
    assert s[3] == (len(widths) if lanes is None else lanes), ("lane launches", s)
    assert s[4] == finishes, ("finish launches", s)
    assert s[5] <= 3, ("stream drains", s)
    assert s[6] == sum(3 * p["n_planned"] for p in plans), ("blocks", s)
    assert s[7] == uploaded, ("uploaded", s)
    assert s[8] == sum(p["stored"] for p in plans), ("stored", s)


def _encoded(a, shape, kind, version, q, seed=None):
    w, h, f = shape
    rgb = WO.smooth_plus_noise(w, h, f, seed=w * 7 + f if seed is None else seed)
    blob = _encode(a, version, rgb, w, h, f, q, kind)
    info, syms = _symbols_of(version, blob)
    assert (info["width"], info["height"], info["frames"], info["wavelet"]) == (w, h, f, kind)
    return blob, info["step"], syms


def _planned_bytes(a, version, blob, planned):
    info = _info(a, version, blob)
    pos, total = HEADER, 0
    for c in range(3):
        table = np.frombuffer(blob, "<u4", info.n_blocks[c], pos)
        total += int(table[sorted(planned)].astype(np.int64).sum())
        pos += info.payload_len[c]
    return total


# ---- 1. the mixed batch ----
def test_mixed_batch(gpu_codec):
    """every shape of the preview's case table x versions 2, 3, 4 x the three wavelets, one or two ranges each, in one call"""
    a = gpu_codec
    lib = a.load_library()
    items = []
    for si, shape in enumerate(PR.SHAPES):
        for version in (2, 3, 4):
            for kind in PR.WAVELETS:
                q = QUALITIES[version][(si + kind) % len(QUALITIES[version])]
                blob, steps, syms = _encoded(a, shape, kind, version, q)
                ranges = PR.ranges_for(shape, kind)
                picks = {ranges[(si + version + kind) % len(ranges)], ranges[(3 * si + kind) % len(ranges)]}
                for t0, t1 in sorted(picks):
                    items.append(Item(blob, shape, kind, version, steps, syms, t0, t1))
    batch = Batch(a, items)
    batch.check("mixed")
    classes = {_finish_class(lib, it) for it in items}
    assert len(classes) >= 6, classes
    _check_stats(a, items, len({id(it.blob) for it in items}), len(classes), lanes=2)
    # the host call on the same items
    got = a.decode_previews([(it.blob, it.t0, it.t1 - it.t0) for it in items])
    for k, it in enumerate(items):
        assert np.array_equal(np.asarray(got[k]), it.want()), ("host call", k)
    union = {}
    for it in items:
        union.setdefault(id(it.blob), (it, set()))[1].update(it.plan()["planned"])
    uploaded = sum(_planned_bytes(a, it.version, it.blob, planned) for it, planned in union.values())
    _check_stats(a, items, len(union), len(classes), uploaded=uploaded, lanes=2)


# ---- 2. size extremes in one finish launch ----
@pytest.mark.parametrize("version,kind", [(2, PR.CDF97), (3, PR.CDF53), (4, PR.HAAR), (4, PR.CDF97)])
def test_size_extremes_in_one_launch(gpu_codec, version, kind):
    """q = 1 (pw = 2), q = 6 (no multiple of 4), q = 153 (odd frame bytes) and 128x128 side by side in both orders: the work
    list gives every item its own workgroups, whatever its neighbours' sizes"""
    a = gpu_codec
    lib = a.load_library()
    shapes = [(2, 2, 1), (5, 3, 7), (33, 17, 5), (128, 128, 8)]
    items = []
    for shape in shapes:
        blob, steps, syms = _encoded(a, shape, kind, version, QUALITIES[version][1])
        f = shape[2]
        items.append(Item(blob, shape, kind, version, steps, syms, 0, f))
        items.append(Item(blob, shape, kind, version, steps, syms, f // 2, f // 2 + 1))
    assert len({_finish_class(lib, it) for it in items}) == 1
    for order in (items, items[::-1]):
        Batch(a, order).check((version, kind))
        _check_stats(a, order, len(shapes), 1)
    for it in (items[0], items[-1], items[3]):
        Batch(a, [it]).check("one item")
        _check_stats(a, [it], 1, 1)


# ---- 3. one container, many ranges ----
@pytest.mark.parametrize("version,kind", [(2, PR.CDF53), (3, PR.CDF97), (4, PR.HAAR)])
def test_one_container_many_ranges(gpu_codec, version, kind):
    a = gpu_codec
    shape = PR.ALL_RANGES_SHAPE
    f = shape[2]
    blob, steps, syms = _encoded(a, shape, kind, version, QUALITIES[version][0])
    items = [Item(blob, shape, kind, version, steps, syms, t0, t1) for t0 in range(f) for t1 in range(t0 + 1, f + 1)]
    Batch(a, items).check((version, kind))
    _check_stats(a, items, 1, 1)
    got = a.decode_previews([(blob, it.t0, it.t1 - it.t0) for it in items])
    for k, it in enumerate(items):
        assert np.array_equal(np.asarray(got[k]), it.want()), ("host call", k)
    union = set()
    for it in items:
        union.update(it.plan()["planned"])
    _check_stats(a, items, 1, 1, uploaded=_planned_bytes(a, version, blob, union))
    # fewer ranges, fewer blocks: the union is the items', not the container's
    few = [it for it in items if it.t1 <= 2]
    a.decode_previews([(blob, it.t0, it.t1 - it.t0) for it in few])
    small = set()
    for it in few:
        small.update(it.plan()["planned"])
    assert small < union
    _check_stats(a, few, 1, 1, uploaded=_planned_bytes(a, version, blob, small))


# ---- 4. instance classes ----
@pytest.mark.parametrize("version", [2, 3, 4])
def test_two_instance_classes_in_one_call(gpu_codec, version):
    """104x40x16, the worst-sign volume, at the last step before the exact class and at its first step: two finish launches"""
    a = gpu_codec
    lib = a.load_library()
    shape = (104, 40, 16)
    for kind in PR.WAVELETS:
        classes = F.X.classes(lib, kind, int(version != 2))
        (_, _, last), (v_exact, first, _) = classes[-2], classes[-1]
        assert v_exact == 0 and first == last + 1
        T = F.centre_frame(kind, shape)
        items = []
        for s in (last, first):
            steps = (s, s, s)
            blob = F.container(kind, shape, "worst", steps, version)
            items.append(Item(blob, shape, kind, version, steps, F.volumes(kind, shape, version)["worst"], T, T + 1, F.LANE_SYMBOLS))
        assert [_finish_class(lib, it)[2] for it in items] == [False, True]
        Batch(a, items).check((version, kind))
        _check_stats(a, items, 2, 2)


# ---- 5. the item limit ----
def test_item_limit(gpu_codec):
    a = gpu_codec
    shape, kind, version = (5, 3, 7), PR.CDF97, 3
    blob, steps, syms = _encoded(a, shape, kind, version, 80)
    f = shape[2]
    items = [Item(blob, shape, kind, version, steps, syms, k % f, k % f + 1 + (k // f) % (f - k % f)) for k in range(1025)]
    batch = Batch(a, items[:1024])
    got = batch.run()
    for k in list(range(0, 1024, 37)) + [1023]:
        assert np.array_equal(got[k], items[k].want()), k
    _check_stats(a, items[:1024], 1, 1)
    stats = a._test_last_previews_stats()
    over = Batch(a, items)
    e = over.refused()
    assert e.code == 2 and e.bad_item is None and "1025 items" in str(e)
    assert a._test_last_previews_stats() == stats


# ---- 6. refusals on the device path ----
@pytest.mark.parametrize("k", [0, 1, 3])
def test_refusals_write_nothing(gpu_codec, k):
    a = gpu_codec
    import oracle.alice_oracle_np as o
    shape, kind = (33, 17, 5), PR.CDF97
    w, h, f = shape
    items = []
    for version in (2, 3, 4, 3):
        blob, steps, syms = _encoded(a, shape, kind, version, 80, seed=version + len(items))
        items.append(Item(blob, shape, kind, version, steps, syms, len(items), len(items) + 1))
    batch = Batch(a, items)
    batch.check("clean")
    stats = a._test_last_previews_stats()
    rows = batch.rows()

    def with_row(row):
        r = list(rows)
        r[k] = row
        return batch.refused(r)

    alc, length, first, count, out = rows[k]
    for bad_first, bad_count in ((0, 0), (0, f + 1), (f, 1), (3, 3)):
        e = with_row((alc, length, bad_first, bad_count, out))
        assert e.code == 2 and e.bad_item == k and f"item {k}: " in str(e)
    e = with_row((alc, length, first, count, None))
    assert e.code == 9 and e.bad_item == k
    e = with_row((None, length, first, count, out))
    assert e.code == 9 and e.bad_item == k
    e = with_row((alc, length - 1, first, count, out))            # a container cut short
    assert e.code == 4 and e.bad_item == k
    # overlapping outputs: item k's first byte is another item's last
    other = (k + 1) % len(rows)
    e = with_row((alc, length, first, count, rows[other][4] + items[other].bytes - 1))
    assert e.code == 2 and e.bad_item == max(k, other) and "overlaps" in str(e)
    e = with_row((alc, length, first, count, rows[other][4]))
    assert e.code == 2 and e.bad_item == max(k, other)
    # a version 1 container in item k
    v1 = o.encode(WO.smooth_plus_noise(w, h, f), w, h, f, 80, kind)
    d_v1 = torch.from_numpy(np.frombuffer(bytes(v1), np.uint8).copy()).to(DEV)
    e = with_row((d_v1.data_ptr(), len(v1), 0, 1, out))
    assert e.code == 4 and e.bad_item == k and "version 1 has no random access (one serial chain per channel)" in str(e)
    assert a._test_last_previews_stats() == stats, "a refused call must not report work"
    batch.check("a refusal left something behind")


# ---- 7. damage ----
@pytest.mark.parametrize("version", [2, 3, 4])
def test_damage_refuses_the_whole_call(gpu_codec, version):
    """128x64x8, L = 64: every odd block is a bottom half, which the preview never decodes.  Five copies of the container,
    so that the damage is item k's alone."""
    a = gpu_codec
    shape, kind = (128, 64, 8), PR.CDF53
    w, h, f = shape
    q = {2: 96, 3: 100, 4: 100}[version]                         # small steps: no lane of a bottom-half block is short
    blob, steps, syms = _encoded(a, shape, kind, version, q, seed=11)
    ranges = [(3, 5), (0, 1), (2, 6), (7, 8), (0, 8)]
    items = [Item(bytes(bytearray(blob)), shape, kind, version, steps, syms, t0, t1) for t0, t1 in ranges]
    assert len({id(it.blob) for it in items}) == 5
    batch = Batch(a, items)
    clean = batch.check("clean")
    _check_stats(a, items, 5, 1)
    stats = a._test_last_previews_stats()
    for k, channel, pick in ((2, 0, 0), (4, 2, -1)):
        plan = items[k].plan()
        assert all(b % 2 == 0 for b in plan["planned"])
        key = id(items[k].blob)
        flipped = _lane_flip(version, blob, channel, plan["planned"][pick])
        batch.put(key, flipped)
        e = batch.refused()
        assert e.code == 4 and e.bad_item == k and "end check" in str(e), (k, str(e))
        with pytest.raises(a.CodecError) as eh:
            a.decode_previews([(flipped if i == k else it.blob, it.t0, it.t1 - it.t0) for i, it in enumerate(items)])
        assert eh.value.code == 4 and eh.value.bad_item == k
        # the same flip in a bottom-half block: not seen
        batch.put(key, _lane_flip(version, blob, channel % 2, plan["planned"][pick] + 1))
        got = batch.run()
        assert all(np.array_equal(x, y) for x, y in zip(got, clean))
        # a block-length entry of a block nobody plans: the scan covers the whole table
        _, lay = _channel_layout(blob)
        bad = bytearray(blob)
        pos = lay[channel][0] + 4 * (plan["planned"][0] + 1)
        bad[pos:pos + 4] = (int.from_bytes(bad[pos:pos + 4], "little") + 1).to_bytes(4, "little")
        batch.put(key, bytes(bad))
        e = batch.refused()
        assert e.code == 4 and e.bad_item == k and "directory" in str(e)
        batch.put(key, blob)
    assert a._test_last_previews_stats() == stats, "a refused call must not report work"
    got = batch.run()
    assert all(np.array_equal(x, y) for x, y in zip(got, clean)), "a refusal left something behind"


# ---- 8. frame-count classes ----
@pytest.mark.parametrize("kind", [PR.CDF97, PR.CDF53])
def test_every_frame_count_class_in_one_call(gpu_codec, kind):
    """12x10 at every frame count of tests/temporal_cases.py, one range each, the versions and the instance classes taking
    turns: the finish kernel's peeled temporal loop under per-record planes, lo and hi"""
    a = gpu_codec
    lib = a.load_library()
    items, seen = [], set()
    for i, (w, h, f) in enumerate(s for s in TC.shapes() if s[:2] == TC.SHAPE):
        version = (2, 3, 4)[i % 3]
        cases = TC.step_cases(lib, kind, int(version != 2))
        steps, _ = cases[(i // 3) % len(cases)]
        blob = TC.container(kind, w, h, f, version, steps)
        syms = TC.byte_symbols(kind, w, h, f).reshape(3, -1) if version == 2 else TC.wide_symbols(kind, w, h, f)
        rs = PR.class_ranges(kind, f)
        t0, t1 = rs[i % len(rs)]
        items.append(Item(blob, (w, h, f), kind, version, steps, syms, t0, t1, TC.LANE_SYMBOLS))
        wa, wb = PR.FR.frame_window(kind, f, t0, t1)
        seen.add(TC.inverse_class((wb - wa) // 2))
    assert len(seen) >= 6, seen
    Batch(a, items).check(kind)
    _check_stats(a, items, len(items), len({_finish_class(lib, it) for it in items}), lanes=2)
