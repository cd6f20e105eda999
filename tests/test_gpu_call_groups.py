"""Calls of more than one group on the MI355X.  At the suite's shapes split_group() is 21845 chunks and chunks_that_fit()
the whole call, so the group loops of the device-resident calls of versions 2-5 and of encode_many / decode_many make one
trip; the hook alice_codec_test_set_group_chunks makes groups of 1, 2 and 3 out of calls of seven chunks (7 x 1, 2 + 2 + 2 + 1,
3 + 3 + 1).  Every chunk differs from every other in content, quality and budget (tests/group_cases.py, held to that by
tests/test_call_groups_host.py), every expected value is the CPU reference's for that chunk, and every output lies between
guard bytes.  Then the verdicts of a call whose second group fails (every call that places its output at a stride refuses
one that is a byte short), and decode groups that hold both band-slot widths."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import group_cases as G  # noqa: E402

import torch  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 256
FILL = 0xCD
N = G.N
CASES = [(shape, cap) for shape in G.SHAPES for cap in G.CAPS]


@contextlib.contextmanager
def groups_of(a, cap, band_kb=None):
    lib = a.load_library()
    try:
        lib.alice_codec_test_set_group_chunks(cap)
        if band_kb is not None:
            lib.alice_codec_test_set_tuning(band_kb)
        yield
    finally:
        lib.alice_codec_test_set_group_chunks(0)
        if band_kb is not None:
            lib.alice_codec_test_set_tuning(1024 * 1024)


class Guarded:
    """n_bytes of device memory between two guards, everything pre-filled"""

    def __init__(self, n_bytes, fill=FILL):
        self.n, self.fill = int(n_bytes), fill
        self.t = torch.full((GUARD + self.n + GUARD,), fill, dtype=torch.uint8, device=DEV)
        self.ptr = self.t.data_ptr() + GUARD

    def host(self):
        """the body, after checking both guards"""
        h = self.t.cpu().numpy()
        assert (h[:GUARD] == self.fill).all() and (h[GUARD + self.n:] == self.fill).all(), "a guard was written"
        return h[GUARD:GUARD + self.n]


def stride_of(blobs):
    return (max(len(b) for b in blobs) + 255) & ~255


def upload(blobs, stride):
    inp = np.zeros(len(blobs) * stride, np.uint8)
    for i, b in enumerate(blobs):
        inp[i * stride:i * stride + len(b)] = np.frombuffer(b, np.uint8)
    return torch.from_numpy(inp).to(DEV)


def check_slots(out: Guarded, stride, want, sizes=None, written=None):
    """slot i holds want[i] and the fill behind it (written: the slots a failed call got to; the others hold the fill)"""
    host = out.host()
    for i, data in enumerate(want):
        slot = host[i * stride:(i + 1) * stride]
        if written is not None and i not in written:
            assert (slot == out.fill).all(), i
            continue
        if sizes is not None:
            assert int(sizes[i]) == len(data), (i, int(sizes[i]), len(data))
        assert slot[:len(data)].tobytes() == data, i
        assert (slot[len(data):] == out.fill).all(), i
    assert (host[len(want) * stride:] == out.fill).all()


def split_trials(a, n):
    out = np.zeros(n, np.uint32)
    assert a.load_library().alice_codec_test_last_split_trials(out.ctypes.data_as(C.POINTER(C.c_uint32)), n) == n
    return [int(v) for v in out]


def quality_trials(a, n):
    out = np.zeros(n, np.uint32)
    assert a.load_library().alice_codec_test_last_quality_trials(out.ctypes.data_as(C.POINTER(C.c_uint32)), n) == n
    return [int(v) for v in out]


def encoder(a, version):
    return {2: a.split_encode_device, 3: a.wide_encode_device, 4: a.reversible_encode_device}[version]


def decoder(a, version):
    return {2: a.split_decode_device, 3: a.wide_decode_device, 4: a.reversible_decode_device}[version]


# ---- 1. encodes with per-chunk qualities, decodes of the reference's containers ----

@pytest.mark.parametrize("shape,cap", CASES)
@pytest.mark.parametrize("version", [2, 3, 4])
def test_encodes_and_decodes(gpu_codec, version, shape, cap):
    a = gpu_codec
    w, h, f = G.SHAPES[shape]
    qs = G.QUALITIES[version]
    blobs = G.containers(version, shape)
    stride = stride_of(blobs)
    d_rgb = torch.from_numpy(G.clips(shape)).to(DEV)
    out = Guarded(N * stride)
    px = Guarded(N * w * h * f * 3, 0xEE)
    d_alc = upload(blobs, stride)
    with groups_of(a, cap):
        sizes = encoder(a, version)(d_rgb.data_ptr(), w, h, f, N, a.WaveletType(G.KIND[version]), 0, out.ptr, stride, qualities=qs,
                                    lane_symbols=G.L)
        decoder(a, version)(d_alc.data_ptr(), stride, [len(b) for b in blobs], px.ptr)
    check_slots(out, stride, blobs, sizes)
    got = px.host().reshape(N, -1)
    for i in range(N):
        assert np.array_equal(got[i], G.pixels(version, shape, i, qs[i])), i
    assert torch.equal(d_rgb.cpu(), torch.from_numpy(G.clips(shape)))


@pytest.mark.parametrize("cap", G.CAPS)
def test_regions_at_seven_origins(gpu_codec, cap):
    a = gpu_codec
    version, shape = 3, "tile"
    w, h, f = G.SHAPES[shape]
    FW, FH = G.FRAME
    qs = G.QUALITIES[version]
    blobs = G.containers(version, shape)
    stride = stride_of(blobs)
    frames = np.random.default_rng(77).integers(0, 256, (N * f, FH, FW, 3), dtype=np.uint8)
    for i, (x0, y0) in enumerate(G.ORIGINS):
        frames[i * f:(i + 1) * f, y0:y0 + h, x0:x0 + w] = G.clip(shape, i).reshape(f, h, w, 3)
    d_frames = torch.from_numpy(frames.reshape(-1)).to(DEV)
    out = Guarded(N * stride)
    back = Guarded(frames.size, 0x5A)
    d_alc = upload(blobs, stride)
    with groups_of(a, cap):
        sizes = a.wide_encode_regions_device(d_frames.data_ptr(), FW, FH, G.ORIGINS, w, h, f, a.WaveletType(G.KIND[version]), 0, out.ptr,
                                             stride, qualities=qs, lane_symbols=G.L)
        a.wide_decode_regions_device(d_alc.data_ptr(), stride, [len(b) for b in blobs], back.ptr, FW, FH, G.ORIGINS)
    check_slots(out, stride, blobs, sizes)
    got = back.host().reshape(N * f, FH, FW, 3).copy()
    for i, (x0, y0) in enumerate(G.ORIGINS):
        rect = got[i * f:(i + 1) * f, y0:y0 + h, x0:x0 + w]
        assert np.array_equal(rect.reshape(-1), G.pixels(version, shape, i, qs[i])), i
        rect[...] = 0x5A
    assert (got == 0x5A).all()                       # nothing outside the rectangles was written
    assert torch.equal(d_frames.cpu(), torch.from_numpy(frames.reshape(-1)))


# ---- 2. size prediction ----

@pytest.mark.parametrize("shape,cap", CASES)
@pytest.mark.parametrize("version", [2, 3])
def test_size_prediction(gpu_codec, version, shape, cap):
    a = gpu_codec
    w, h, f = G.SHAPES[shape]
    d_rgb = torch.from_numpy(G.clips(shape)).to(DEV)
    kind = a.WaveletType(G.KIND[version])
    with groups_of(a, cap):
        if version == 2:
            p = a.predict_split_sizes_device(d_rgb.data_ptr(), w, h, f, N, kind, G.L)
        else:
            rows = Guarded(N * 64 * 3 * 256 * 4, 0x7F)
            p = a.predict_wide_sizes_device(d_rgb.data_ptr(), w, h, f, N, kind, G.L, d_step_hist=rows.ptr)
            bare = a.predict_wide_sizes_device(d_rgb.data_ptr(), w, h, f, N, kind, G.L)          # d_step_hist may be NULL
    assert p.lo.shape == p.hi.shape == (N, 101)
    for i in range(N):
        lo, hi = G.brackets(version, shape, i)
        assert np.array_equal(p.lo[i], lo) and np.array_equal(p.hi[i], hi), i
    if version == 3:
        got = rows.host().view(np.uint32).reshape(N, 64, 3, 256)
        for i in range(N):
            assert np.array_equal(got[i], G.step_hists(3, shape, i)), i
        assert np.array_equal(bare.lo, p.lo) and np.array_equal(bare.hi, p.hi)


# ---- 3. byte budgets ----

@pytest.mark.parametrize("shape,cap", CASES)
@pytest.mark.parametrize("version", [2, 3])
def test_budget_encodes(gpu_codec, version, shape, cap):
    a = gpu_codec
    w, h, f = G.SHAPES[shape]
    plan = G.budget_plan(version, shape)
    min_q, max_q = G.BUDGET_RANGE[version]
    stride = stride_of(G.containers(version, shape))
    assert all(len(data) <= stride for *_, data in plan)
    d_rgb = torch.from_numpy(G.clips(shape)).to(DEV)
    out = Guarded(N * stride)
    call = a.split_encode_to_budget_device if version == 2 else a.wide_encode_to_budget_device
    with groups_of(a, cap):
        chosen, fits, sizes = call(d_rgb.data_ptr(), w, h, f, N, a.WaveletType(G.KIND[version]), [b for b, *_ in plan], out.ptr, stride,
                                   min_q, max_q, G.L)
        trials = split_trials(a, N)
    print(f"v{version} {shape} cap {cap}: chose {list(chosen)} fits {list(fits)} trials {trials}; reference {[p[1:4] for p in plan]}")
    assert [(int(chosen[i]), bool(fits[i])) for i in range(N)] == [(q, fit) for _, q, fit, _, _ in plan]
    assert trials == [t for _, _, _, t, _ in plan]
    check_slots(out, stride, [data for *_, data in plan], sizes)


# ---- 4. trials ----

@pytest.mark.parametrize("shape,cap", CASES)
@pytest.mark.parametrize("version", [2, 3, 4])
def test_trial_sse_rows(gpu_codec, version, shape, cap):
    a = gpu_codec
    w, h, f = G.SHAPES[shape]
    qs = G.QUALITIES[version]
    d_rgb = torch.from_numpy(G.clips(shape)).to(DEV)
    rows = Guarded(N * f * 8, 0x7F)
    kind = a.WaveletType(G.KIND[version])
    with groups_of(a, cap):
        sse = a.trial_sse_device(version, d_rgb.data_ptr(), w, h, f, N, kind, 0, qualities=qs, d_frame_sse_ptr=rows.ptr)
        lent = a.trial_sse_device(version, d_rgb.data_ptr(), w, h, f, N, kind, 0, qualities=qs)      # the call's own rows
    want = [G.sse(version, shape, i, qs[i]) for i in range(N)]
    assert [int(s) for s in sse] == want and [int(s) for s in lent] == want
    got = rows.host().view(np.uint64).reshape(N, f)
    for i in range(N):
        assert np.array_equal(got[i], G.frame_sse(version, shape, i, qs[i])), i


# ---- 5. PSNR floors ----

@pytest.mark.parametrize("shape,cap", CASES)
@pytest.mark.parametrize("version", [2, 3])
def test_psnr_floor_encodes(gpu_codec, version, shape, cap):
    a = gpu_codec
    w, h, f = G.SHAPES[shape]
    plan = G.psnr_plan(version, shape)
    min_q, max_q = G.PSNR_RANGE[version]
    stride = stride_of([data for *_, data in plan])
    d_rgb = torch.from_numpy(G.clips(shape)).to(DEV)
    out = Guarded(N * stride)
    call = a.split_encode_to_psnr_device if version == 2 else a.wide_encode_to_psnr_device
    with groups_of(a, cap):
        chosen, reached, db, sizes = call(d_rgb.data_ptr(), w, h, f, N, a.WaveletType(G.KIND[version]), G.PSNR_TARGET[version, shape],
                                          out.ptr, stride, min_quality=min_q, max_quality=max_q, lane_symbols=G.L)
        trials = quality_trials(a, N)
    print(f"v{version} {shape} cap {cap}: chose {list(chosen)} dB {list(db)} trials {trials}; reference {[p[:4] for p in plan]}")
    assert [(int(chosen[i]), bool(reached[i]), float(db[i])) for i in range(N)] == [(q, ok, want_db) for q, ok, _, want_db, _ in plan]
    assert trials == [t for _, _, t, _, _ in plan]
    check_slots(out, stride, [data for *_, data in plan], sizes)


# ---- 6. transcodes ----

@pytest.mark.parametrize("shape,cap", CASES)
@pytest.mark.parametrize("version", [2, 3])
def test_transcodes(gpu_codec, version, shape, cap):
    a = gpu_codec
    srcs = G.sources(version, shape)
    stride = stride_of(srcs)
    d_in = upload(srcs, stride)
    lens = [len(s) for s in srcs]
    want = G.transcode_plan(version, shape)
    plan = G.transcode_budget_plan(version, shape)
    min_q, max_q = G.TRANSCODE_RANGE
    out, out_b = Guarded(N * stride), Guarded(N * stride)
    with groups_of(a, cap):
        sizes = a.transcode_device(d_in.data_ptr(), stride, lens, 0, out.ptr, stride, qualities=G.TARGETS[version])
        chosen, fits, sizes_b = a.transcode_to_budget_device(d_in.data_ptr(), stride, lens, [b for b, *_ in plan], out_b.ptr, stride,
                                                             min_q, max_q)
        trials = split_trials(a, N)
    check_slots(out, stride, want, sizes)
    print(f"v{version} {shape} cap {cap}: chose {list(chosen)} fits {list(fits)} trials {trials}; reference {[p[1:4] for p in plan]}")
    assert [(int(chosen[i]), bool(fits[i])) for i in range(N)] == [(q, fit) for _, q, fit, _, _ in plan]
    assert trials == [t for _, _, _, t, _ in plan]
    check_slots(out_b, stride, [data for *_, data in plan], sizes_b)
    assert torch.equal(d_in.cpu(), upload(srcs, stride).cpu())              # the sources are only read


# ---- 7. version 1 host calls: passes of chunks_that_fit ----

@pytest.mark.parametrize("shape", list(G.SHAPES))
def test_version_1_host_calls(gpu_codec, oracle_mod, shape):
    a = gpu_codec
    w, h, f = G.SHAPES[shape]
    kind = G.KIND[1]
    qs = G.QUALITIES[1]
    stored = [oracle_mod.encode(G.clip(shape, i), w, h, f, qs[i], kind) for i in range(N)]
    flat = [oracle_mod.encode(G.clip(shape, i), w, h, f, 80, kind) for i in range(N)]     # encode_many has one quality per call
    assert len({len(b) for b in stored}) == N and len({len(b) for b in flat}) == N
    with groups_of(a, 2):
        chunks = a.encode_many(a.FrameEncoder.with_wavelet(80, a.WaveletType(kind)), G.clips(shape), w, h, f)
        pixels = a.decode_many([a.EncodedChunk.from_bytes(b) for b in stored])
    assert [c.to_bytes() for c in chunks] == flat
    assert pixels.shape == (N, w * h * f * 3)
    for i in range(N):
        assert np.array_equal(pixels[i], oracle_mod.decode(stored[i])), i


# ---- 8. version 5: the banded encode and decode, the repack in both directions ----

@pytest.mark.parametrize("shape,cap", CASES)
@pytest.mark.parametrize("base", G.BASES)
def test_banded_calls(gpu_codec, base, shape, cap):
    a = gpu_codec
    w, h, f = G.SHAPES[shape]
    qs = G.QUALITIES[base]
    plain, blobs = G.containers(base, shape), G.bandeds(base, shape)
    stride = stride_of(blobs + plain)
    d_rgb = torch.from_numpy(G.clips(shape)).to(DEV)
    d_plain, d_v5 = upload(plain, stride), upload(blobs, stride)
    out, there, back = Guarded(N * stride), Guarded(N * stride), Guarded(N * stride)
    px = Guarded(N * w * h * f * 3, 0xEE)
    with groups_of(a, cap):
        sizes = a.banded_encode_device(d_rgb.data_ptr(), w, h, f, N, a.WaveletType(G.KIND[base]), 0, out.ptr, stride, qualities=qs,
                                       lane_symbols=G.L, base=base)
        a.banded_decode_device(d_v5.data_ptr(), stride, [len(b) for b in blobs], px.ptr)
        sizes_there = a.to_banded_device(d_plain.data_ptr(), stride, [len(b) for b in plain], there.ptr, stride)
        sizes_back = a.from_banded_device(d_v5.data_ptr(), stride, [len(b) for b in blobs], back.ptr, stride)
    check_slots(out, stride, blobs, sizes)
    got = px.host().reshape(N, -1)
    for i in range(N):
        assert np.array_equal(got[i], G.pixels(base, shape, i, qs[i])), i
    check_slots(there, stride, G.to_banded_plan(base, shape), sizes_there)
    check_slots(back, stride, G.from_banded_plan(base, shape), sizes_back)
    assert torch.equal(d_rgb.cpu(), torch.from_numpy(G.clips(shape)))       # the inputs are only read
    assert torch.equal(d_plain.cpu(), upload(plain, stride).cpu()) and torch.equal(d_v5.cpu(), upload(blobs, stride).cpu())


# ---- verdicts of a call whose second group fails (3 + 3 + 1: chunks 0-2 have been written by then) ----

def refused(a, code, fn):
    with pytest.raises(a.CodecError) as e:
        fn()
    assert e.value.code == code, str(e.value)
    return str(e.value)


def test_output_stride_one_byte_short_of_the_largest_chunk(gpu_codec):
    a = gpu_codec
    shape = "tile"
    w, h, f = G.SHAPES[shape]
    # the encode
    blobs = G.containers(2, shape)
    short = len(blobs[G.BIG]) - 1
    assert all(len(b) <= short for i, b in enumerate(blobs) if i != G.BIG)
    d_rgb = torch.from_numpy(G.clips(shape)).to(DEV)
    out = Guarded(N * short)
    with groups_of(a, G.VERDICT_CAP):
        msg = refused(a, 1, lambda: a.split_encode_device(d_rgb.data_ptr(), w, h, f, N, a.WaveletType(G.KIND[2]), 0, out.ptr, short,
                                                          qualities=G.QUALITIES[2], lane_symbols=G.L))
    assert f"chunk {G.BIG} " in msg, msg
    check_slots(out, short, blobs, written={0, 1, 2})
    # the transcode
    for version in (2, 3):
        srcs = G.sources(version, shape)
        want = G.transcode_plan(version, shape)
        short = len(want[G.BIG]) - 1
        assert all(len(b) <= short for i, b in enumerate(want) if i != G.BIG)
        stride = stride_of(srcs)
        d_in = upload(srcs, stride)
        out = Guarded(N * short)
        with groups_of(a, G.VERDICT_CAP):
            msg = refused(a, 1, lambda: a.transcode_device(d_in.data_ptr(), stride, [len(s) for s in srcs], 0, out.ptr, short,
                                                           qualities=G.TARGETS[version]))
        assert f"chunk {G.BIG} " in msg, msg
        check_slots(out, short, want, written={0, 1, 2})


UNTOUCHED = 0xA5A5A5A5A5A5A5A5


def _strided_call(a, family, shape, d_in, in_stride, in_lens, d_out, out_stride, sizes):
    """the family's C entry point on chunks in G.STRIDE_ORDER, with the caller's own sizes array -> its return code"""
    lib = a.load_library()
    w, h, f = G.SHAPES[shape]
    v = G.STRIDE_VERSION[family]
    u8 = lambda values: np.array(G.in_stride_order(values), np.uint8)      # noqa: E731
    p_sizes = sizes.ctypes.data_as(C.POINTER(C.c_uint64))
    if d_in is None:
        q = u8(G.QUALITIES[v])
        d_rgb = torch.from_numpy(np.concatenate(G.in_stride_order([G.clip(shape, i) for i in range(N)]))).to(DEV)
        head = (d_rgb.data_ptr(), w, h, f, N, G.KIND[v], 0, q.ctypes.data_as(C.POINTER(C.c_uint8)), G.L)
        if family == "banded":
            return lib.alice_codec_dev_encode_banded(*head, v, d_out, out_stride, p_sizes, None)
        return getattr(lib, f"alice_codec_dev_encode_{family}")(*head, d_out, out_stride, p_sizes, None)
    lens = np.array(in_lens, np.uint64)
    p_lens = lens.ctypes.data_as(C.POINTER(C.c_uint64))
    if family == "transcode":
        q = u8(G.TARGETS[v])
        return lib.alice_codec_dev_transcode(d_in.data_ptr(), in_stride, p_lens, N, 0, q.ctypes.data_as(C.POINTER(C.c_uint8)), 0, 0, d_out,
                                             out_stride, p_sizes, None)
    return getattr(lib, f"alice_codec_dev_{family}")(d_in.data_ptr(), in_stride, p_lens, N, 0, d_out, out_stride, p_sizes, None)


@pytest.mark.parametrize("family", G.STRIDE_FAMILIES)
def test_output_stride_refused_in_the_second_group(gpu_codec, family):
    """Groups of two; the stride is one byte short of chunk 3 alone, the second chunk of the second group.  The call names
    that chunk by its index in the call, group 0 has been written, nothing else has, and sizes holds group 0's entries."""
    a = gpu_codec
    shape = "tile"
    inputs, want = G.stride_plan(family, shape)
    short = len(want[G.STRIDE_AT]) - 1
    assert all(len(b) <= short for i, b in enumerate(want) if i != G.STRIDE_AT)
    d_in = in_stride = in_lens = None
    if inputs is not None:
        in_stride, in_lens = stride_of(inputs), [len(b) for b in inputs]
        d_in = upload(inputs, in_stride)
    out = Guarded(N * short)
    sizes = np.full(N, UNTOUCHED, np.uint64)
    lib = a.load_library()
    with groups_of(a, G.STRIDE_CAP):
        rc = _strided_call(a, family, shape, d_in, in_stride, in_lens, out.ptr, short, sizes)
        code, msg = lib.alice_codec_last_error(), lib.alice_codec_last_error_message().decode()
    print(f"{family}: rc {rc} code {code}: {msg}; sizes {[hex(int(s)) for s in sizes]}")
    assert rc == 1 and code == 1, (rc, code, msg)                       # kInvalidBufferSize
    assert f"chunk {G.STRIDE_AT} needs {len(want[G.STRIDE_AT])} bytes" in msg and f"stride is {short}" in msg, msg
    first = set(range(G.STRIDE_CAP))
    check_slots(out, short, want, written=first)
    assert [int(s) for s in sizes[:G.STRIDE_CAP]] == [len(want[i]) for i in sorted(first)]
    assert (sizes[G.STRIDE_CAP:] == UNTOUCHED).all()


@pytest.mark.parametrize("version", [2, 3])
def test_damaged_chunk_in_a_transcode(gpu_codec, version):
    a = gpu_codec
    srcs = G.sources(version, "tile")
    want = G.transcode_plan(version, "tile")
    bad = list(srcs)
    bad[G.BIG] = G.damaged(srcs[G.BIG])
    stride = stride_of(srcs)
    d_in = upload(bad, stride)
    out = Guarded(N * stride)
    with groups_of(a, G.VERDICT_CAP):
        refused(a, 4, lambda: a.transcode_device(d_in.data_ptr(), stride, [len(s) for s in bad], 0, out.ptr, stride,
                                                 qualities=G.TARGETS[version]))
    # the verdict of a group is read before its maps are queued: nothing of chunks 3-5 is written
    check_slots(out, stride, want, written={0, 1, 2})


def test_damaged_chunk_in_a_decode(gpu_codec):
    a = gpu_codec
    shape = "tile"
    w, h, f = G.SHAPES[shape]
    qs = G.QUALITIES[2]
    blobs = list(G.containers(2, shape))
    blobs[G.BIG] = G.damaged(blobs[G.BIG])
    stride = stride_of(blobs)
    d_alc = upload(blobs, stride)
    px = Guarded(N * w * h * f * 3, 0xEE)
    with groups_of(a, G.VERDICT_CAP):
        refused(a, 4, lambda: a.split_decode_device(d_alc.data_ptr(), stride, [len(b) for b in blobs], px.ptr))
    got = px.host().reshape(N, -1)
    for i in range(3):
        assert np.array_equal(got[i], G.pixels(2, shape, i, qs[i])), i
    # chunks 3-5: the inverse of a group is queued before its verdict is read; their content is not defined
    assert (got[6] == 0xEE).all()


# ---- both band-slot widths in one decode group (256x256x16 under a 4 MiB band target: the i16 plan's slot is the larger) ----

def _mixed_decode(a, version, qualities):
    w, h, f = G.MIXED_SHAPE
    blobs = [G.mixed_container(version, q) for q in qualities]
    stride = stride_of(blobs)
    d_alc = upload(blobs, stride)
    px = Guarded(len(blobs) * w * h * f * 3, 0xEE)
    with groups_of(a, 0, G.MIXED_BAND_KB):
        lib = a.load_library()
        i16, i32 = (int(lib.alice_codec_test_inverse_scratch_bytes(w, h, f, m)) for m in (1, 0))
        assert i16 > i32 > 0 and int(lib.alice_codec_test_group_scratch_bytes(w, h, f, 1, 1)) == i16
        decoder(a, version)(d_alc.data_ptr(), stride, [len(b) for b in blobs], px.ptr)
    got = px.host().reshape(len(blobs), -1)
    for i, q in enumerate(qualities):
        assert np.array_equal(got[i], G.mixed_pixels(version, q)), (version, i, q)


@pytest.mark.parametrize("version", [2, 3, 4])
def test_mixed_widths_in_one_banded_decode_group(gpu_codec, version):
    q16, q32 = G.MIXED_QUALITIES[version]
    _mixed_decode(gpu_codec, version, [q16, q32])


def test_mixed_widths_group_of_three(gpu_codec):
    q16, q32 = G.MIXED_QUALITIES[3]
    _mixed_decode(gpu_codec, 3, [q32, q16, q32])


def test_mixed_widths_in_one_banded_decode_many(gpu_codec, oracle_mod):
    a = gpu_codec
    w, h, f = G.MIXED_SHAPE
    stored = [oracle_mod.encode(G.mixed_clip(), w, h, f, q, G.MIXED_KIND) for q in G.MIXED_QUALITIES[1]]
    with groups_of(a, 0, G.MIXED_BAND_KB):
        pixels = a.decode_many([a.EncodedChunk.from_bytes(b) for b in stored])
    for i, b in enumerate(stored):
        assert np.array_equal(pixels[i], oracle_mod.decode(b)), i
