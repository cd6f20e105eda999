"""Half-resolution preview on the MI355X: alice_codec_dev_decode_preview and
alice_codec_decode_preview against the numpy restatement of tests/preview_ref.py, bit for bit, with the plan of that module
held against what the calls report they did -- a decode that did everything and cropped would pass the parity and fail
there.  Symbols come from the reference lane decoders (split_ref / wide_ref) or are the volumes the containers were written
from; nothing is compared with the library's own full decode.  Lane size 64 unless stated; the shapes and what each is for
are listed at preview_ref.SHAPES."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frames_extreme_cases as F  # noqa: E402
import frames_ref as FR  # noqa: E402
import preview_ref as PR  # noqa: E402
import reversible_ref as RR  # noqa: E402
import temporal_cases as TC  # noqa: E402
import wide_ref as R3  # noqa: E402
from test_gpu_frames import DEV, GUARD, HEADER, QUALITIES, _channel_layout, _encode, _guard_pattern, _info, _lane_flip  # noqa: E402
from test_gpu_frames_extremes import _symbols_of  # noqa: E402
import wide_oracle as WO  # noqa: E402

pytestmark = pytest.mark.gpu

L = PR.LANE
_ran = {}      # (version, kind) -> {instance class: steps the finish kernel ran at}


class Preview:
    """One container at an odd device address and the output of the device call between guard bytes of 0 and 255."""

    def __init__(self, a, blob, shape, kind, version):
        self.a, self.shape, self.kind, self.version = a, tuple(shape), kind, version
        w, h, f = shape
        self.qw, self.qh = PR.preview_dims(w, h)
        self.frame_bytes = self.qw * self.qh * 3
        self.out = torch.empty(2 * GUARD + f * self.frame_bytes, dtype=torch.uint8, device=DEV)
        self.pattern = _guard_pattern(self.out.numel())
        self.set_container(blob)

    def set_container(self, blob):
        self.blob = bytes(blob)
        raw = np.frombuffer(self.blob, np.uint8)
        self.d_alc = torch.empty(raw.size + 8, dtype=torch.uint8, device=DEV)
        off = 1 if self.d_alc.data_ptr() % 2 == 0 else 2
        self.alc_view = self.d_alc[off:off + raw.size]
        self.alc_view.copy_(torch.from_numpy(raw.copy()))
        self.alc_len = raw.size

    def dev(self, t0, t1):
        """-> the preview of [t0, t1) as numpy, after the guards and everything behind the frames were checked"""
        n = (t1 - t0) * self.frame_bytes
        self.out.copy_(self.pattern)
        self.a.preview_decode_device(self.alc_view.data_ptr(), self.alc_len, t0, t1 - t0, self.out.data_ptr() + GUARD)
        torch.cuda.synchronize()
        assert torch.equal(self.out[:GUARD], self.pattern[:GUARD]), "bytes before the output were written"
        assert torch.equal(self.out[GUARD + n:], self.pattern[GUARD + n:]), "bytes behind the output were written"
        return self.out[GUARD:GUARD + n].cpu().numpy()

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


def _check_stats(a, plan, count, uploaded):
    assert a._test_last_preview_stats() == (plan["a"], plan["b"], 3 * plan["n_planned"], uploaded, count, plan["stored"])


def _check(a, pv, syms, steps, lane, ranges, host_ranges, where):
    """every range through the device call, the ranges of host_ranges through the host call too; both against preview_ref"""
    w, h, f = pv.shape
    dims = TC.dims(w, h, f)
    for t0, t1 in ranges:
        want = PR.preview(syms, dims, f, pv.kind, steps, pv.version, t0, t1)
        plan = PR.preview_plan(pv.kind, w, h, f, lane, t0, t1)
        got = pv.dev(t0, t1)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (where, (t0, t1), bad.size, bad[:4].tolist())
        _check_stats(a, plan, t1 - t0, 0)
        if (t0, t1) in host_ranges:
            host = np.asarray(a.decode_preview(pv.blob, t0, t1 - t0))
            assert np.array_equal(host, want), (where, (t0, t1), "host call")
            _check_stats(a, plan, t1 - t0, pv.planned_bytes(plan))


# ---- 1. the case table ----
@pytest.mark.parametrize("version", [2, 3, 4])
@pytest.mark.parametrize("shape", PR.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_case_table_equals_the_reference_and_does_partial_work(gpu_codec, shape, version):
    a = gpu_codec
    w, h, f = shape
    assert a.preview_dims(w, h) == PR.preview_dims(w, h)
    for kind in PR.WAVELETS:
        q = QUALITIES[version][(PR.SHAPES.index(tuple(shape)) + kind) % len(QUALITIES[version])]
        rgb = WO.smooth_plus_noise(w, h, f, seed=w * 7 + f)
        blob = _encode(a, version, rgb, w, h, f, q, kind)
        info, syms = _symbols_of(version, blob)
        assert (info["width"], info["height"], info["frames"], info["wavelet"]) == (w, h, f, kind)
        pv = Preview(a, blob, shape, kind, version)
        _check(a, pv, syms, info["step"], L, PR.ranges_for(shape, kind), set(FR.named_ranges(kind, f)), (shape, version, kind, q))


# ---- 2. every instance of the finish kernel: classes at their edge steps, worst-sign and loud volumes ----
@pytest.mark.parametrize("version", [2, 3, 4])
@pytest.mark.parametrize("kind", PR.WAVELETS)
def test_instances_at_their_edge_steps(gpu_codec, kind, version):
    """104x40x16: the worst-sign volume (every sample at the largest magnitude the format decodes to) and a loud random
    one, at the first and last quantiser step of every instance class alice_codec_test_inverse_variant names."""
    a = gpu_codec
    lib = a.load_library()
    shape = (104, 40, 16)
    w, h, f = shape
    T = F.centre_frame(kind, shape)
    ranges = [(0, f), (T, T + 1), (T + 1, T + 2), (0, 1), (f - 1, f)]
    pv = None
    for name, steps, v in F.cases(lib, kind, shape, version):
        assert F.variant(lib, kind, steps, version) == v
        blob = F.container(kind, shape, name, steps, version)
        if pv is None:
            pv = Preview(a, blob, shape, kind, version)
        else:
            pv.set_container(blob)
        _check(a, pv, F.volumes(kind, shape, version)[name], steps, F.LANE_SYMBOLS, ranges, {(T, T + 1)}, (kind, version, name, steps, v))
        _ran.setdefault((version, kind), {}).setdefault(v, set()).add(tuple(steps))
    edges = F.class_edges(lib, kind, version)
    assert set(edges) == F.EXPECTED[version][kind]
    for v, edge in edges.items():
        assert edge <= _ran[(version, kind)][v], (version, kind, v, edge)


@pytest.mark.parametrize("version", [2, 3, 4])
def test_every_frame_count_class(gpu_codec, version):
    """12x10 at every frame count of tests/temporal_cases.py and 70x34 at its steady-loop counts, loud random volumes, one
    step of every instance class: the finish kernel's stream at every half a window can have."""
    a = gpu_codec
    lib = a.load_library()
    wide = int(version != 2)
    for kind in PR.WAVELETS:
        cases = TC.step_cases(lib, kind, wide)
        seen = set()
        for i, (w, h, f) in enumerate(TC.shapes()):
            steps, _ = cases[i % len(cases)]
            blob = TC.container(kind, w, h, f, version, steps)
            syms = TC.byte_symbols(kind, w, h, f).reshape(3, -1) if version == 2 else TC.wide_symbols(kind, w, h, f)
            pv = Preview(a, blob, (w, h, f), kind, version)
            rs = PR.class_ranges(kind, f)
            _check(a, pv, syms, steps, TC.LANE_SYMBOLS, rs, set(), (kind, version, (w, h, f), steps))
            for t0, t1 in rs:
                wa, wb = FR.frame_window(kind, f, t0, t1)
                seen.add(TC.inverse_class((wb - wa) // 2))
        assert seen >= set(TC.INVERSE_CLASSES), (kind, set(TC.INVERSE_CLASSES) - seen)


# ---- 3. lane sizes ----
@pytest.mark.parametrize("version,lane", [(v, n) for v in F.VERSIONS for n in F.LANE_SIZES[v]])
def test_lane_sizes(gpu_codec, version, lane):
    """128x96x40 encoded by the library at L = 128, 512, 2048 and the format's maximum (one partly filled block)"""
    a = gpu_codec
    shape = F.LANE_SHAPE
    w, h, f = shape
    kind = F.lane_kind(version, lane)
    rgb = WO.smooth_plus_noise(w, h, f, seed=40 + kind)
    blob = _encode(a, version, rgb, w, h, f, F.LANE_QUALITY[version], kind, lane)
    info, syms = _symbols_of(version, blob)
    assert info["lane_symbols"] == lane
    pv = Preview(a, blob, shape, kind, version)
    _check(a, pv, syms, info["step"], lane, F.lane_ranges(kind, f), set(FR.named_ranges(kind, f)), (version, lane, kind))


@pytest.mark.parametrize("version,lane", [(v, n) for v in (3, 4) for n in F.ESCAPE_LANES])
def test_lanes_of_escapes_only(gpu_codec, version, lane):
    """the worst-sign wide volume of 104x40x16: every coded symbol is an escape"""
    a = gpu_codec
    shape = F.ESCAPE_SHAPE
    w, h, f = shape
    kind = (version + F.ESCAPE_LANES.index(lane)) % 3
    z = F.volumes(kind, shape, version)["worst"]
    assert all(int(zz.min()) >= 255 for zz in z)
    blob = RR.with_version(R3.write_container(kind, w, h, f, lane, F.ESCAPE_STEPS, z), version)
    pv = Preview(a, blob, shape, kind, version)
    _check(a, pv, z, F.ESCAPE_STEPS, lane, F.lane_ranges(kind, f), {(0, f), (0, 1)}, (version, lane, kind))


# ---- 4. damage ----
@pytest.mark.parametrize("version", [2, 3, 4])
def test_damage(gpu_codec, version):
    """128x64x8, L = 64: a plane is two blocks, the first its top half and the second its bottom half, so every odd block
    is one the preview never decodes."""
    a = gpu_codec
    shape, kind = (128, 64, 8), PR.CDF53
    w, h, f = shape
    rgb = WO.smooth_plus_noise(w, h, f, seed=11)
    blob = _encode(a, version, rgb, w, h, f, {2: 96, 3: 100, 4: 100}[version], kind)      # small steps: no lane of a bottom-half block is short
    info, syms = _symbols_of(version, blob)
    pv = Preview(a, blob, shape, kind, version)
    t0, t1 = 3, 5
    plan = PR.preview_plan(kind, w, h, f, L, t0, t1)
    assert all(b % 2 == 0 for b in plan["planned"]) and "blocks_skipped_inside_a_plane" in plan["classes"]
    bottom = [b + 1 for b in plan["planned"]]                       # inside the window's planes, bottom halves
    dims = plan["dims"]
    want = PR.preview(syms, dims, f, kind, info["step"], version, t0, t1)
    assert np.array_equal(pv.dev(t0, t1), want)
    stats = a._test_last_preview_stats()
    full_decode = {2: a.decode_split, 3: a.decode_wide, 4: a.decode_reversible}[version]

    # a lane of a planned block: refused by both calls, the output untouched, the stats unchanged
    for channel, block in ((0, plan["planned"][0]), (2, plan["planned"][-1])):
        bad = _lane_flip(version, blob, channel, block)
        pv.set_container(bad)
        with pytest.raises(a.CodecError) as e:
            pv.dev(t0, t1)
        assert e.value.code == 4 and "end check" in str(e.value)
        assert pv.untouched(), "a refused preview wrote to its output"
        with pytest.raises(a.CodecError) as e:
            a.decode_preview(bad, t0, t1 - t0)
        assert e.value.code == 4
        assert a._test_last_preview_stats() == stats, "a refused call must not report work"

    # a lane of a bottom-half block: not seen, the preview is the clean file's; the full decode refuses the file
    for channel, block in ((0, bottom[0]), (1, bottom[-1])):
        bad = _lane_flip(version, blob, channel, block)
        pv.set_container(bad)
        assert np.array_equal(pv.dev(t0, t1), want)
        assert np.array_equal(np.asarray(a.decode_preview(bad, t0, t1 - t0)), want)
        with pytest.raises(a.CodecError) as e:
            full_decode(bad)
        assert e.value.code == 4

    # a block-length entry anywhere (here: of a bottom-half block): the scan covers the whole table
    _, lay = _channel_layout(blob)
    for delta in (1, -1):
        bad = bytearray(blob)
        pos = lay[1][0] + 4 * bottom[0]
        v = int.from_bytes(bad[pos:pos + 4], "little") + delta
        bad[pos:pos + 4] = v.to_bytes(4, "little")
        pv.set_container(bytes(bad))
        with pytest.raises(a.CodecError) as e:
            pv.dev(t0, t1)
        assert e.value.code == 4 and "directory" in str(e.value)
        assert pv.untouched()
        with pytest.raises(a.CodecError) as e:
            a.decode_preview(bytes(bad), t0, t1 - t0)
        assert e.value.code == 4
    pv.set_container(blob)
    assert np.array_equal(pv.dev(t0, t1), want), "a refusal left something behind"


def test_refusals_write_nothing(gpu_codec):
    a = gpu_codec
    import oracle.alice_oracle_np as o
    shape, kind = (33, 17, 5), PR.CDF97
    w, h, f = shape
    rgb = WO.smooth_plus_noise(w, h, f)
    blob = _encode(a, 3, rgb, w, h, f, 80, kind)
    pv = Preview(a, blob, shape, kind, 3)
    pv.out.copy_(pv.pattern)
    a.decode_preview(blob, 0, 1)
    stats = a._test_last_preview_stats()
    out = pv.out.data_ptr() + GUARD
    for first, count in ((0, 0), (0, f + 1), (f, 1), (3, 3)):
        with pytest.raises(a.CodecError) as e:
            a.preview_decode_device(pv.alc_view.data_ptr(), pv.alc_len, first, count, out)
        assert e.value.code == 2 and pv.untouched()
    pv.set_container(o.encode(rgb, w, h, f, 80, kind))
    with pytest.raises(a.CodecError, match=r"version 1 has no random access \(one serial chain per channel\)"):
        a.preview_decode_device(pv.alc_view.data_ptr(), pv.alc_len, 0, 1, out)
    assert pv.untouched()
    pv.set_container(blob)
    with pytest.raises(a.CodecError) as e:                # a container cut short
        a.preview_decode_device(pv.alc_view.data_ptr(), pv.alc_len - 1, 0, 1, out)
    assert e.value.code == 4 and pv.untouched()
    assert a._test_last_preview_stats() == stats, "a refused call must not report work"
