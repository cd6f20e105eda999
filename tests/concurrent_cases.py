"""The job table of tests/test_gpu_concurrent_calls.py: one call of every entry-point family with the value it must return,
so that the families can be run side by side from many threads and every result still be held to a reference.

A job is (family, name, run(codec, stream_or_None) -> result, expected).  expected is bytes, an ndarray or a tuple of such
(and of plain numbers), or ("error", kind) for a call that must be refused with that error code.  Every expected value comes
from the CPU references -- the oracle for version 1 and the stage level, split_ref / wide_ref / reversible_ref for the
containers, frames_ref / preview_ref / rect_ref for the partial decodes, rate_ref / split_rate_ref / wide_rate_ref /
quality_ref for the rate and quality calls, segment_ref for segmentation -- and never from the library.  Containers that a
decode job reads are the references' bytes too.  Lane size 64 (a block is 4096 symbols); the shapes are the small ones
the references declare; (5, 3, 7) takes the generic path.

JOBS holds the host calls (run ignores its stream), DEVICE_JOBS the device-pointer calls: run(codec, stream) gets a
torch.cuda.Stream, fills its inputs by a non-blocking copy from pinned host memory on that stream immediately before the
call, pre-fills its outputs with 0xEE and reads them back after stream.synchronize().  No job touches a process-wide
tuning hook: such a hook would make concurrent neighbours wrong by design.  Nothing here imports torch at module level."""
from __future__ import annotations

import functools
import os
import sys
from collections import namedtuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import oracle  # noqa: E402
import oracle.alice_oracle_np as o  # noqa: E402
import frames_ref as FR  # noqa: E402
import preview_ref as PR  # noqa: E402
import quality_ref as Q  # noqa: E402
import rate_ref  # noqa: E402
import rect_ref as RF  # noqa: E402
import reversible_ref as RR  # noqa: E402
import segment_ref as SG  # noqa: E402
import split_rate_ref as SR  # noqa: E402
import split_ref as R2  # noqa: E402
import wide_oracle as WO  # noqa: E402
import wide_rate_ref as WR  # noqa: E402
import wide_ref as R3  # noqa: E402
from test_frames_host import _encode_ref  # noqa: E402

Job = namedtuple("Job", "family name run expected")

LANE = 64
DEV = "cuda:0"
FILL = 0xEE
CDF53, CDF97, HAAR = FR.CDF53, FR.CDF97, FR.HAAR
SHAPES = [(64, 64, 16), (50, 38, 13), (33, 17, 5), (5, 3, 7), (40, 24, 1)]
FAMILIES = ("v1", "v2", "v3", "v4", "rate", "quality", "frames", "preview", "rect", "previews", "segment", "stage", "refusal")
# error kinds of include/alice_codec.h
INVALID_DIMENSIONS, INVALID_BITSTREAM = 2, 4
Q_OF_STEP = WR.q_of_step()


def same(got, want) -> bool:
    """bit-exact equality of a job's result with its expected value"""
    if isinstance(want, tuple):
        return isinstance(got, (tuple, list)) and len(got) == len(want) and all(same(g, w) for g, w in zip(got, want))
    if isinstance(want, np.ndarray):
        g = np.asarray(got)
        return g.size == want.size and bool(np.array_equal(g.reshape(-1), want.reshape(-1)))
    if isinstance(want, (bytes, bytearray)):
        return isinstance(got, (bytes, bytearray)) and bytes(got) == bytes(want)
    return type(got) is not np.ndarray and got == want


def is_refusal(expected) -> bool:
    return isinstance(expected, tuple) and len(expected) == 2 and isinstance(expected[0], str) and expected[0] == "error"


# ---------------------------------------------------------------------------------------------------------------------
# sources, containers and their reference decodes (each computed once, never modified)
# ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def source(shape, seed=None):
    w, h, f = shape
    rgb = WO.smooth_plus_noise(w, h, f, seed=(w * 7 + f) if seed is None else seed)
    rgb.setflags(write=False)
    return rgb


@functools.lru_cache(maxsize=None)
def container(shape, kind, version, quality) -> bytes:
    """the reference's container bytes: split_ref / wide_ref write_container of the oracle's quantised coefficients"""
    w, h, f = shape
    return _encode_ref(version, source(shape), w, h, f, quality, kind, LANE)


Decoded = namedtuple("Decoded", "steps dims syms qvols")


@functools.lru_cache(maxsize=None)
def decoded(shape, kind, version, quality) -> Decoded:
    """the container through the reference lane decoder: steps, (pw, ph, pf), the three symbol arrays and the three
    (pf, ph, pw) volumes of quantised coefficients"""
    blob = container(shape, kind, version, quality)
    if version == 2:
        info, syms = R2.decode_container(blob)
        qs = [np.asarray(o.from_symbols(s), np.int64) for s in syms]
    else:
        info, syms = R3.decode_container(RR.with_version(blob, 3))
        qs = [np.asarray(R3.from_wide_symbols(s), np.int64) for s in syms]
    assert (info["width"], info["height"], info["frames"], info["wavelet"], info["lane_symbols"]) == (*shape, kind, LANE)
    pw, ph, pf = R2.padded_dims(*shape)
    return Decoded(tuple(info["step"]), (pw, ph, pf), syms, [q.reshape(pf, ph, pw) for q in qs])


def _inverse(version, kind, steps, qvols):
    """three (vf, vh, vw) volumes of quantised coefficients -> the three sample volumes: the reference's inverse for
    versions 2 and 3, the mirrored one for version 4"""
    out = []
    for q, step in zip(qvols, steps):
        vf, vh, vw = q.shape
        coef = o._wrap32(np.asarray(q, np.int64).reshape(-1) * int(step))
        vol = RR.mirror_wavelet3d(kind, coef, vw, vh, vf) if version == 4 else o.wavelet3d(kind, coef, vw, vh, vf, inverse=True)
        out.append(np.asarray(vol).reshape(vf, vh, vw))
    return out


def _rgb(chans) -> np.ndarray:
    return np.asarray(o.ycocg_r_to_rgb(*[o._wrap16(np.ascontiguousarray(c).reshape(-1)) for c in chans]), np.uint8)


@functools.lru_cache(maxsize=None)
def full_decode(shape, kind, version, quality) -> np.ndarray:
    """(f, h, w, 3): the whole chunk through the inverse of the whole volume"""
    w, h, f = shape
    d = decoded(shape, kind, version, quality)
    out = _rgb([c[:f, :h, :w] for c in _inverse(version, kind, d.steps, d.qvols)]).reshape(f, h, w, 3)
    out.setflags(write=False)
    return out


def frames_expected(case, t0, t1) -> np.ndarray:
    """frames_ref: the inverse of the window's virtual chunk, cut to the range"""
    shape, kind, version, _ = case
    w, h, f = shape
    d = decoded(*case)
    a, b = FR.frame_window(kind, f, t0, t1)
    chans = _inverse(version, kind, d.steps, [FR.window_volume(q, d.dims, a, b) for q in d.qvols])
    return _rgb([c[t0 - a:t1 - a, :h, :w] for c in chans])


def rect_expected(case, t0, t1, rect) -> np.ndarray:
    """rect_ref: the inverse of the three windows' virtual chunk, cut to range x rectangle; (t1 - t0) * rh * rw * 3 bytes"""
    shape, kind, version, _ = case
    w, h, f = shape
    x, y, rw, rh = rect
    d = decoded(*case)
    win = RF.windows(kind, w, h, f, t0, t1, rect)
    (ta, _), (ya, _), (xa, _) = win
    chans = _inverse(version, kind, d.steps, [RF.cut(q, d.dims, win) for q in d.qvols])
    return _rgb([c[t0 - ta:t1 - ta, y - ya:y - ya + rh, x - xa:x - xa + rw] for c in chans])


def preview_expected(case, t0, t1) -> np.ndarray:
    shape, kind, version, _ = case
    d = decoded(*case)
    return np.asarray(PR.preview(d.syms, d.dims, shape[2], kind, d.steps, version, t0, t1), np.uint8)


# the containers of the table: every shape, every wavelet and every version at least once
V2_A, V2_B = ((64, 64, 16), CDF97, 2, 80), ((33, 17, 5), CDF53, 2, 50)
V3_A, V3_B = ((50, 38, 13), CDF53, 3, 95), ((5, 3, 7), HAAR, 3, 100)
V4_A, V4_B = ((33, 17, 5), HAAR, 4, 100), ((40, 24, 1), CDF97, 4, 80)
V4_LOSSLESS = ((50, 38, 13), CDF97, 4, 100)
PARTIAL_A, PARTIAL_B, PARTIAL_C = ((64, 64, 16), CDF53, 3, 80), ((50, 38, 13), CDF97, 2, 80), ((5, 3, 7), HAAR, 4, 100)


def _wt(a, kind):
    return a.WaveletType(kind)


def _encoder(a, case):
    return a.FrameEncoder.with_wavelet(case[3], _wt(a, case[1]))


def _encode_call(a, version):
    return {2: a.encode_split, 3: a.encode_wide, 4: a.encode_reversible}[version]


def _decode_call(a, version):
    return {2: a.decode_split, 3: a.decode_wide, 4: a.decode_reversible}[version]


# ---------------------------------------------------------------------------------------------------------------------
# v1
# ---------------------------------------------------------------------------------------------------------------------

def _v1_jobs():
    out = []
    for shape, kind, q in (((64, 64, 16), CDF97, 80), ((5, 3, 7), HAAR, 100)):
        w, h, f = shape
        rgb = source(shape)
        ref = oracle.encode(rgb, w, h, f, q, kind)
        out.append(Job("v1", f"v1/encode {shape} wavelet {kind}",
                       lambda a, s, rgb=rgb, w=w, h=h, f=f, q=q, kind=kind: a.FrameEncoder.with_wavelet(q, _wt(a, kind)).encode(rgb, w, h, f).to_bytes(),
                       ref))
    for shape, kind, q in (((50, 38, 13), CDF53, 90), ((40, 24, 1), CDF97, 75)):
        w, h, f = shape
        ref = oracle.encode(source(shape), w, h, f, q, kind)
        out.append(Job("v1", f"v1/decode {shape} wavelet {kind}",
                       lambda a, s, ref=ref: np.asarray(a.FrameDecoder().decode(a.EncodedChunk.from_bytes(ref))), np.asarray(oracle.decode(ref))))
    shape, kind, q = (33, 17, 5), HAAR, 80
    w, h, f = shape
    chunks = np.stack([source(shape, seed=40 + i) for i in range(3)])
    refs = tuple(oracle.encode(c, w, h, f, q, kind) for c in chunks)

    def many(a, s):
        got = a.encode_many(a.FrameEncoder.with_wavelet(q, _wt(a, kind)), chunks, w, h, f)
        return tuple(c.to_bytes() for c in got), np.asarray(a.decode_many(got))
    out.append(Job("v1", f"v1/encode_many+decode_many 3 x {shape} wavelet {kind}", many,
                   (refs, np.stack([np.asarray(oracle.decode(r)) for r in refs]))))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# v2, v3, v4
# ---------------------------------------------------------------------------------------------------------------------

def _container_jobs():
    out = []
    for case_a, case_b in ((V2_A, V2_B), (V3_A, V3_B), (V4_A, V4_B)):
        version = case_a[2]
        fam = f"v{version}"
        for enc_case, dec_case in ((case_a, case_b), (case_b, case_a)):
            (w, h, f), kind = enc_case[0], enc_case[1]
            out.append(Job(fam, f"{fam}/encode {enc_case[0]} wavelet {kind} q {enc_case[3]}",
                           lambda a, s, c=enc_case, w=w, h=h, f=f: _encode_call(a, c[2])(_encoder(a, c), source(c[0]), w, h, f, LANE),
                           container(*enc_case)))
            out.append(Job(fam, f"{fam}/decode {dec_case[0]} wavelet {dec_case[1]} q {dec_case[3]}",
                           lambda a, s, c=dec_case: np.asarray(_decode_call(a, c[2])(container(*c))), full_decode(*dec_case)))
    shape, kind = V4_LOSSLESS[0], V4_LOSSLESS[1]
    w, h, f = shape
    out.append(Job("v4", f"v4/encode_lossless {shape} wavelet {kind}",
                   lambda a, s: a.encode_lossless(source(shape), w, h, f, _wt(a, kind), LANE), container(*V4_LOSSLESS)))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# rate and quality
# ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _v1_prediction(shape, kind):
    w, h, f = shape
    hists = rate_ref.oracle_step_hists(oracle, source(shape), w, h, f, kind)
    return rate_ref.chunk_prediction(oracle, hists, SR.log_table())


@functools.lru_cache(maxsize=None)
def _step_symbols(shape, kind, wide):
    """[step - 1][channel]: the symbols of the padded volume at a quality of every step 1..64"""
    w, h, f = shape
    if wide:
        return WR.oracle_step_symbols_wide(o, source(shape), w, h, f, kind)
    return [oracle.encode_symbols(source(shape), w, h, f, Q_OF_STEP[s], kind).reshape(3, -1) for s in range(1, 65)]


@functools.lru_cache(maxsize=None)
def _bracket(shape, kind, wide):
    syms = _step_symbols(shape, kind, wide)
    if wide:
        hists = np.stack([np.stack([R3.histogram(z) for z in zs]) for zs in syms])
        return WR.chunk_prediction(hists, LANE)
    hists = np.stack([np.stack([np.bincount(s, minlength=256) for s in zs]) for zs in syms])
    return SR.chunk_prediction(hists, LANE)


@functools.lru_cache(maxsize=None)
def _step_container(shape, kind, wide, step) -> bytes:
    w, h, f = shape
    ref = R3 if wide else R2
    return ref.write_container(kind, w, h, f, LANE, [step] * 3, _step_symbols(shape, kind, wide)[step - 1])


@functools.lru_cache(maxsize=None)
def budget_choice(shape, kind, wide):
    """(budget, quality, fits, trials, bytes): the budget is the exact size of quality 60's container, so that the upper
    bounds alone do not decide and the refinement has to count"""
    lo, hi = _bracket(shape, kind, wide)
    budget = len(_step_container(shape, kind, wide, SR.quality_to_step(60)))
    q, fits, trials = SR.choose(lo, hi, budget, 10, 95, lambda qq: len(_step_container(shape, kind, wide, SR.quality_to_step(qq))))
    return budget, q, fits, trials, _step_container(shape, kind, wide, SR.quality_to_step(q))


def _rate_jobs():
    out = []
    for shape, kind in (((33, 17, 5), CDF53), ((40, 24, 1), CDF97)):
        w, h, f = shape

        def v1(a, s, shape=shape, kind=kind, w=w, h=h, f=f):
            p = a.predict_sizes(source(shape), w, h, f, _wt(a, kind))
            return p.lo, p.hi, p.status
        out.append(Job("rate", f"rate/predict_sizes {shape} wavelet {kind}", v1, tuple(_v1_prediction(shape, kind))))
    for wide, shape_a, shape_b in ((False, ((33, 17, 5), CDF97), ((5, 3, 7), CDF53)), (True, ((40, 24, 1), HAAR), ((33, 17, 5), CDF53))):
        name = "wide" if wide else "split"
        for shape, kind in (shape_a, shape_b):
            w, h, f = shape

            def predict(a, s, wide=wide, shape=shape, kind=kind, w=w, h=h, f=f):
                p = (a.predict_wide_sizes if wide else a.predict_split_sizes)(source(shape), w, h, f, _wt(a, kind), LANE)
                return p.lo, p.hi
            out.append(Job("rate", f"rate/predict_{name}_sizes {shape} wavelet {kind}", predict, tuple(_bracket(shape, kind, wide))))
        shape, kind = shape_a
        w, h, f = shape
        budget, q, fits, _, data = budget_choice(shape, kind, wide)

        def to_size(a, s, wide=wide, shape=shape, kind=kind, w=w, h=h, f=f, budget=budget):
            return (a.encode_wide_to_size if wide else a.encode_split_to_size)(source(shape), w, h, f, budget, _wt(a, kind), 10, 95, LANE)
        out.append(Job("rate", f"rate/encode_{name}_to_size {shape} wavelet {kind}", to_size, (data, q, fits)))
    return out


@functools.lru_cache(maxsize=None)
def psnr_choice(shape, kind, version):
    """(target dB, quality, reached, trials, dB of the point, bytes) for a target midway between two adjacent steps"""
    w, h, f = shape
    n = w * h * f * 3
    max_q = 96 if version == 2 else 100
    table = Q.step_table(version, source(shape), w, h, f, kind, max_q)
    targets = Q.midway_targets(table, n)
    t = targets[len(targets) // 3]
    q, reached, trials = Q.choose(table, n, t, 0, max_q)
    return t, q, reached, trials, Q.psnr_from_sse(table[Q.step_of(q)], n), _encode_ref(version, source(shape), w, h, f, q, kind, LANE)


def _quality_jobs():
    out = []
    for version, shape, kind in ((2, (33, 17, 5), CDF97), (3, (40, 24, 1), HAAR), (3, (5, 3, 7), CDF53)):
        w, h, f = shape
        t, q, reached, _, db, data = psnr_choice(shape, kind, version)
        name = "split" if version == 2 else "wide"

        def run(a, s, version=version, shape=shape, kind=kind, w=w, h=h, f=f, t=t):
            call = a.encode_split_to_psnr if version == 2 else a.encode_wide_to_psnr
            return call(source(shape), w, h, f, t, _wt(a, kind), 0, 96 if version == 2 else 100, LANE)
        out.append(Job("quality", f"quality/encode_{name}_to_psnr {shape} wavelet {kind}", run, (data, q, reached, db)))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# frames, preview, rect, previews
# ---------------------------------------------------------------------------------------------------------------------

FRAMES_CASES = [(PARTIAL_A, 9, 10), (PARTIAL_B, 0, 13), (PARTIAL_C, 6, 7)]
PREVIEW_CASES = [(PARTIAL_A, 0, 1), (PARTIAL_B, 5, 8), (PARTIAL_C, 0, 7)]
RECT_CASES = [(PARTIAL_A, 7, 9, (20, 30, 9, 7)), (PARTIAL_B, 12, 13, (45, 35, 5, 3)), (PARTIAL_C, 0, 7, (0, 0, 5, 3))]
# one mixed-version item list; items 0 and 2 name one container
PREVIEWS_ITEMS = [(PARTIAL_A, 3, 5), (PARTIAL_B, 12, 13), (PARTIAL_A, 15, 16), (PARTIAL_C, 2, 3), (V4_B, 0, 1)]
PREVIEWS_ITEMS_B = [(PARTIAL_C, 0, 7), (V2_B, 1, 4), (V3_A, 6, 7)]


def _previews_run(items):
    def run(a, s):
        return tuple(np.asarray(x) for x in a.decode_previews([(container(*c), t0, t1 - t0) for c, t0, t1 in items]))
    return run


def _partial_jobs():
    out = []
    for case, t0, t1 in FRAMES_CASES:
        out.append(Job("frames", f"frames/decode_frames v{case[2]} {case[0]} wavelet {case[1]} [{t0}, {t1})",
                       lambda a, s, c=case, t0=t0, t1=t1: np.asarray(a.decode_frames(container(*c), t0, t1 - t0)), frames_expected(case, t0, t1)))
    for case, t0, t1 in PREVIEW_CASES:
        out.append(Job("preview", f"preview/decode_preview v{case[2]} {case[0]} wavelet {case[1]} [{t0}, {t1})",
                       lambda a, s, c=case, t0=t0, t1=t1: np.asarray(a.decode_preview(container(*c), t0, t1 - t0)), preview_expected(case, t0, t1)))
    for case, t0, t1, rect in RECT_CASES:
        out.append(Job("rect", f"rect/decode_rect v{case[2]} {case[0]} wavelet {case[1]} [{t0}, {t1}) {rect}",
                       lambda a, s, c=case, t0=t0, t1=t1, r=rect: np.asarray(a.decode_rect(container(*c), t0, t1 - t0, *r)),
                       rect_expected(case, t0, t1, rect)))
    for tag, items in (("five items", PREVIEWS_ITEMS), ("three items", PREVIEWS_ITEMS_B)):
        out.append(Job("previews", f"previews/decode_previews {tag} of versions {sorted({c[2] for c, _, _ in items})}",
                       _previews_run(items), tuple(preview_expected(c, t0, t1) for c, t0, t1 in items)))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# segmentation
# ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def motion_frames(w, h, n=1):
    """reference and current frames (n, h, w) with moved rectangles and speckles"""
    rng = np.random.default_rng(w * 31 + h)
    ref = rng.integers(0, 256, (n, h, w), dtype=np.uint8)
    cur = ref.copy()
    for k in range(n):
        for _ in range(3):
            y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w))
            y1, x1 = min(h, y0 + int(rng.integers(1, max(2, h // 2)))), min(w, x0 + int(rng.integers(1, max(2, w // 2))))
            cur[k, y0:y1, x0:x1] = 255 - cur[k, y0:y1, x0:x1]
        speck = rng.random((h, w)) < 0.01
        cur[k][speck] = rng.integers(0, 256, int(speck.sum()), dtype=np.uint8)
    cur.setflags(write=False); ref.setflags(write=False)
    return cur, ref


def _seg_result(r):
    return np.asarray(r.mask), tuple(int(v) for v in r.bbox), int(r.foreground_count)


def _seg_expected(mask, stats):
    return np.asarray(mask[0], np.uint8).reshape(-1), tuple(int(v) for v in stats[0][:4]), int(stats[0][4])


def _segment_jobs():
    out = []
    for (w, h), (thr, rd, re) in (((64, 64), (25, 2, 1)), ((50, 38), (100, 1, 1)), ((33, 17), (0, 0, 0))):
        cur, ref = motion_frames(w, h)
        want = _seg_expected(*SG.vec_motion(cur, ref, thr, rd, re))
        out.append(Job("segment", f"segment/segment_by_motion {w}x{h} radii {rd}, {re}",
                       lambda a, s, cur=cur, ref=ref, w=w, h=h, cfg=(thr, 100, rd, re): _seg_result(a.segment_by_motion(cur[0], ref[0], w, h, a.SegmentConfig(*cfg))),
                       want))
        mask, bbox = want[0], want[1]
        out.append(Job("segment", f"segment/rle_encode_mask {w}x{h}", lambda a, s, mask=mask: a.rle_encode_mask(mask), SG.vec_rle(mask)))
        frame = source((w, h, {64: 16, 50: 13, 33: 5}[w]))[:w * h * 3]
        out.append(Job("segment", f"segment/extract_person_rgb {w}x{h}",
                       lambda a, s, mask=mask, w=w, bbox=bbox, frame=frame: a.extract_person_rgb(mask, w, list(bbox), frame),
                       SG.vec_extract(mask, w, bbox, frame)))
    for shape, thr in (((50, 38, 13), 30), ((40, 24, 1), -5)):
        w, h, _ = shape
        cg = SG.vec_cg_of_rgb(np.asarray(source(shape)[:w * h * 3]).reshape(h, w, 3))
        out.append(Job("segment", f"segment/segment_by_chroma {w}x{h} threshold {thr}",
                       lambda a, s, cg=cg, w=w, h=h, thr=thr: _seg_result(a.segment_by_chroma(None, None, cg, w, h, thr)),
                       _seg_expected(*SG.vec_chroma(cg[None], thr))))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the stage-level objects
# ---------------------------------------------------------------------------------------------------------------------

DECODER_CALLS = (5000, 1, 9000, 4096, 4095)


def skewed(seed, n):
    rng = np.random.default_rng(seed)
    p = 1.0 / (1.0 + np.arange(256)) ** 1.3
    return rng.choice(256, size=n, p=p / p.sum()).astype(np.uint8)


def _hist(sym):
    return np.bincount(sym, minlength=256).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def decoder_stream(seed, n):
    """(symbols, histogram, the oracle's stream) of a single-chain decode job"""
    sym = skewed(seed, n)
    return sym, _hist(sym), oracle.rans_encode(sym, oracle.FrequencyTable(_hist(sym)))


def decoder_expected(seed, n, calls=DECODER_CALLS):
    """per call: (symbols, state, position) of the oracle's RansDecoder"""
    _, hist, data = decoder_stream(seed, n)
    to = oracle.FrequencyTable(hist)
    d = oracle.RansDecoder(data)
    out = []
    for c in calls:
        out.append((np.asarray(d.decode_n(c, to)), int(d.state), int(d.pos)))
    return tuple(out)


def decoder_steps(a, seed, n, calls=DECODER_CALLS):
    """a generator: one RansDecoder, one decode_n per step -> (symbols, state, position); the caller may interleave the
    steps of several objects"""
    _, hist, data = decoder_stream(seed, n)
    tg = a.FrequencyTable.from_histogram(hist)
    d = a.RansDecoder(data)
    for c in calls:
        yield np.asarray(d.decode_n(c, tg)), int(d.state), int(d.position)


def single_symbols_expected(seed, n, count=5):
    _, hist, data = decoder_stream(seed, n)
    return tuple(int(v) for v in oracle.rans_decode(data, count, oracle.FrequencyTable(hist)))


def single_symbols(a, seed, n, count=5):
    """decode(), one symbol at a time"""
    _, hist, data = decoder_stream(seed, n)
    tg = a.FrequencyTable.from_histogram(hist)
    d = a.RansDecoder(data)
    return tuple(int(d.decode(tg)) for _ in range(count))


def _stage_jobs():
    out = []
    for seed, sizes in ((5, (5000, 7, 4096)), (6, (9000, 1, 300))):
        parts = [skewed(seed * 10 + i, n) for i, n in enumerate(sizes)]
        hist = _hist(np.concatenate(parts))
        to = oracle.FrequencyTable(hist)
        eo = oracle.RansEncoder()
        want = []
        for p in parts:
            eo.encode_symbols(p, to)
            want.append(int(eo.state))
        want.append(eo.finish())

        def enc(a, s, parts=parts, hist=hist):
            tg = a.FrequencyTable.from_histogram(hist)
            e = a.RansEncoder()
            got = []
            for p in parts:
                e.encode_symbols(p, tg)
                got.append(int(e.state))
            return (*got, e.finish())
        out.append(Job("stage", f"stage/RansEncoder encode_symbols x 3 {sizes}", enc, tuple(want)))
    for seed, n in ((7, 30000), (8, 23000)):
        out.append(Job("stage", f"stage/RansDecoder decode_n {DECODER_CALLS} of {n}",
                       lambda a, s, seed=seed, n=n: tuple(decoder_steps(a, seed, n)), decoder_expected(seed, n)))
    for seed, n in ((9, 4097), (10, 10001)):
        sym = skewed(seed, n)
        hist = _hist(sym)
        ref = oracle.rans_encode(sym, oracle.FrequencyTable(hist), interleaved=True)

        def ienc(a, s, sym=sym, hist=hist):
            e = a.InterleavedRansEncoder()
            e.encode(sym, a.FrequencyTable.from_histogram(hist))
            return e.finish()
        out.append(Job("stage", f"stage/InterleavedRansEncoder {n}", ienc, ref))
        out.append(Job("stage", f"stage/InterleavedRansDecoder {n}",
                       lambda a, s, ref=ref, n=n, hist=hist: np.asarray(a.InterleavedRansDecoder(ref).decode_n(n, a.FrequencyTable.from_histogram(hist))),
                       np.asarray(oracle.rans_decode(ref, n, oracle.FrequencyTable(hist), interleaved=True))))
    for (w, h, d), kind in (((64, 64, 16), CDF53), ((33, 17, 5), CDF97), ((5, 3, 7), HAAR)):
        vol = np.random.default_rng(w + d).integers(-1000, 1000, w * h * d).astype(np.int32)
        fwd = np.asarray(oracle.wavelet3d(kind, vol, w, h, d))
        out.append(Job("stage", f"stage/Wavelet3D forward {(w, h, d)} wavelet {kind}",
                       lambda a, s, vol=vol, w=w, h=h, d=d, kind=kind: np.asarray(a.Wavelet3D(_wt(a, kind)).forward(vol, w, h, d)), fwd))
        out.append(Job("stage", f"stage/Wavelet3D inverse {(w, h, d)} wavelet {kind}",
                       lambda a, s, fwd=fwd, w=w, h=h, d=d, kind=kind: np.asarray(a.Wavelet3D(_wt(a, kind)).inverse(fwd, w, h, d)),
                       np.asarray(oracle.wavelet3d(kind, fwd, w, h, d, inverse=True))))
    vals = np.concatenate([np.random.default_rng(13).integers(-10000, 10001, 5000), [0, 1, -1, 2**31 - 1, -2**31, -2**31 + 1]]).astype(np.int32)
    for step in (7, 14):
        out.append(Job("stage", f"stage/Quantizer.quantize_buffer step {step}",
                       lambda a, s, step=step: np.asarray(a.Quantizer(step).quantize_buffer(vals)), np.asarray(oracle.quantize_buffer(step, vals))))
    for w, h in ((64, 64), (50, 38)):
        rng = np.random.default_rng(w)
        x = rng.integers(0, 256, w * h, dtype=np.uint8)
        y = np.clip(x.astype(np.int32) + rng.integers(-12, 13, w * h), 0, 255).astype(np.uint8)
        out.append(Job("stage", f"stage/ssim {w}x{h}", lambda a, s, x=x, y=y, w=w, h=h: float(a.ssim(x, y, w, h)), float(oracle.ssim(x, y, w, h))))
    for n, q, sb in ((4096, 80, 0), (1001, 37, 7)):
        c = (np.random.default_rng(n).standard_normal(n) * 40).astype(np.int32)
        want = tuple(int(v) for v in oracle.rdo_compute_quantizer(oracle.rdo_target_bpp(q), c, sb))

        def rdo(a, s, c=c, q=q, sb=sb):
            qz = a.AnalyticalRDO.with_quality(q).compute_quantizer(c, a.SubBand3D(sb))
            return int(qz.step), int(qz.dead_zone)
        out.append(Job("stage", f"stage/AnalyticalRDO.compute_quantizer {n} q {q} subband {sb}", rdo, want))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------

REFUSAL_FRAMES_CASE = ((64, 64, 16), CDF53, 3, 80)     # PARTIAL_A: a plane is one block, so a range leaves blocks unplanned
REFUSAL_RANGE = (9, 10)


@functools.lru_cache(maxsize=None)
def lane_damaged(case, block=None, channel=0) -> bytes:
    """the container with a lane of `block` (default: the first block the range REFUSAL_RANGE plans) that fails its end
    check in the reference decoder"""
    from test_gpu_frames import _lane_flip
    shape, kind, version, _ = case
    if block is None:
        block = FR.frame_plan(kind, *shape, LANE, *REFUSAL_RANGE)["planned"][0] if shape[2] > REFUSAL_RANGE[0] else 0
    return _lane_flip(version, container(*case), channel, block)


@functools.lru_cache(maxsize=None)
def directory_damaged(case, channel=1, block=0) -> bytes:
    """the container with one block-length entry raised by one: the directory does not add up"""
    from test_gpu_frames import _channel_layout
    blob = container(*case)
    _, lay = _channel_layout(blob)
    bad = bytearray(blob)
    pos = lay[channel][0] + 4 * block
    bad[pos:pos + 4] = (int.from_bytes(bad[pos:pos + 4], "little") + 1).to_bytes(4, "little")
    return bytes(bad)


@functools.lru_cache(maxsize=None)
def v1_blob(shape=(33, 17, 5), kind=CDF97, q=80) -> bytes:
    w, h, f = shape
    return oracle.encode(source(shape), w, h, f, q, kind)


def previews_with_damage(k=1):
    """PREVIEWS_ITEMS with item k's container damaged in a block its range plans -> [(blob, first, count)]"""
    rows = []
    for i, (c, t0, t1) in enumerate(PREVIEWS_ITEMS):
        blob = container(*c)
        if i == k:
            plan = PR.preview_plan(c[1], *c[0], LANE, t0, t1)
            blob = lane_damaged(c, plan["planned"][0], 2)
        rows.append((blob, t0, t1 - t0))
    return rows


def _refusal_jobs():
    out = []
    bad = ("error", INVALID_BITSTREAM)
    for case in (V2_A, V3_A, V4_A):
        v = case[2]
        out.append(Job("refusal", f"refusal/decode v{v} {case[0]}: a lane fails its end check",
                       lambda a, s, c=case: _decode_call(a, c[2])(lane_damaged(c, 0)), bad))
    for case in (PARTIAL_B, REFUSAL_FRAMES_CASE, PARTIAL_C):
        v = case[2]
        out.append(Job("refusal", f"refusal/decode_frames v{v} {case[0]}: the directory does not add up",
                       lambda a, s, c=case: a.decode_frames(directory_damaged(c), 0, 1), bad))
    c = REFUSAL_FRAMES_CASE
    t0, t1 = REFUSAL_RANGE
    out.append(Job("refusal", f"refusal/decode_frames v{c[2]} {c[0]}: a planned lane fails its end check",
                   lambda a, s: a.decode_frames(lane_damaged(c), t0, t1 - t0), bad))
    out.append(Job("refusal", "refusal/decode_frames: a frame range outside the chunk",
                   lambda a, s: a.decode_frames(container(*c), c[0][2], 1), ("error", INVALID_DIMENSIONS)))
    out.append(Job("refusal", "refusal/decode_rect: a rectangle outside the frame",
                   lambda a, s: a.decode_rect(container(*c), 0, 1, c[0][0] - 1, 0, 2, 1), ("error", INVALID_DIMENSIONS)))
    out.append(Job("refusal", "refusal/decode_frames: a version 1 container", lambda a, s: a.decode_frames(v1_blob(), 0, 1), bad))
    out.append(Job("refusal", "refusal/decode_previews: item 1 damaged", lambda a, s: a.decode_previews(previews_with_damage(1)), bad))
    return out


@functools.lru_cache(maxsize=None)
def jobs():
    """the host job table"""
    return tuple(_v1_jobs() + _container_jobs() + _rate_jobs() + _quality_jobs() + _partial_jobs() + _segment_jobs() + _stage_jobs()
                 + _refusal_jobs())


def by_family(table=None):
    out = {}
    for j in (jobs() if table is None else table):
        out.setdefault(j.family, []).append(j)
    return out


def check(job, codec, stream=None):
    """runs the job once and holds the result to its expected value; -> the result"""
    if is_refusal(job.expected):
        try:
            got = job.run(codec, stream)
        except codec.CodecError as e:
            assert e.code == job.expected[1], (job.name, "refused with", e.code, str(e), "instead of", job.expected[1])
            return e
        raise AssertionError((job.name, "was not refused", type(got)))
    got = job.run(codec, stream)
    assert same(got, job.expected), (job.name, "differs from its reference", _describe(got, job.expected))
    return got


def _describe(got, want, depth=0):
    if isinstance(want, tuple) and isinstance(got, (tuple, list)) and len(got) == len(want) and depth < 2:
        return [(_describe(g, w, depth + 1)) for g, w in zip(got, want) if not same(g, w)][:3]
    if isinstance(want, np.ndarray):
        g = np.asarray(got).reshape(-1)
        if g.size != want.size:
            return ("sizes", g.size, want.size)
        bad = np.flatnonzero(g != want.reshape(-1))
        return ("elements", int(bad.size), bad[:4].tolist())
    if isinstance(want, (bytes, bytearray)) and isinstance(got, (bytes, bytearray)):
        return ("bytes", len(got), len(want))
    return (repr(got)[:80], repr(want)[:80])


# ---------------------------------------------------------------------------------------------------------------------
# the device-pointer calls on a caller's stream
# ---------------------------------------------------------------------------------------------------------------------

class OnStream:
    """The buffers of one device job: inputs go up by a non-blocking copy from pinned memory on the stream and nothing
    waits for them; outputs start as 0xEE.  Everything is allocated and run with the stream as torch's current one."""

    def __init__(self, stream):
        import torch
        self.torch, self.stream, self.cs, self.keep = torch, stream, stream.cuda_stream, []

    def __enter__(self):
        self.ctx = self.torch.cuda.stream(self.stream)
        self.ctx.__enter__()
        return self

    def __exit__(self, *exc):
        self.stream.synchronize()
        return self.ctx.__exit__(*exc)

    def up(self, host):
        t = self.torch
        pinned = t.from_numpy(np.ascontiguousarray(host).copy()).pin_memory()
        dev = t.empty(pinned.shape, dtype=pinned.dtype, device=DEV)
        dev.copy_(pinned, non_blocking=True)
        self.keep.append(pinned)
        return dev

    def up_bytes(self, blob):
        return self.up(np.frombuffer(bytes(blob), np.uint8))

    def out(self, n):
        return self.torch.full((int(n),), FILL, dtype=self.torch.uint8, device=DEV)

    def back(self, dev) -> np.ndarray:
        self.stream.synchronize()
        return dev.cpu().numpy()


def _padded(shape):
    pw, ph, pf = R2.padded_dims(*shape)
    return pw * ph * pf


def _stride(a, shape):
    return (a.SPLIT_HEADER_BYTES + 3 * a.wide_stream_bound(_padded(shape), LANE) + 255) & ~255


def _filled(n, at=0, data=None):
    v = np.full(int(n), FILL, np.uint8)
    if data is not None:
        d = np.frombuffer(bytes(data), np.uint8) if isinstance(data, (bytes, bytearray)) else np.asarray(data, np.uint8).reshape(-1)
        v[at:at + d.size] = d
    return v


def _dev_encode_job(case):
    shape, kind, version, q = case
    w, h, f = shape

    def run(a, stream):
        call = {2: a.split_encode_device, 3: a.wide_encode_device, 4: a.reversible_encode_device}[version]
        with OnStream(stream) as s:
            stride = _stride(a, shape)
            out = s.out(stride)
            d = s.up(source(shape))
            sizes = call(d.data_ptr(), w, h, f, 1, _wt(a, kind), q, out.data_ptr(), stride, None, LANE, s.cs)
            host = s.back(out)
            return int(sizes[0]), host
    blob = container(*case)
    return Job(f"v{version}", f"device/v{version} encode {shape} wavelet {kind}", run, ("stride", blob))


def _dev_decode_job(case):
    shape, kind, version, q = case
    n = int(np.prod(shape)) * 3

    def run(a, stream):
        call = {2: a.split_decode_device, 3: a.wide_decode_device, 4: a.reversible_decode_device}[version]
        blob = container(*case)
        with OnStream(stream) as s:
            out = s.out(n + 64)
            d = s.up_bytes(blob)
            call(d.data_ptr(), len(blob), [len(blob)], out.data_ptr(), s.cs)
            return s.back(out)
    return Job(f"v{version}", f"device/v{version} decode {shape} wavelet {kind}", run, _filled(n + 64, 0, full_decode(*case)))


def _dev_partial_jobs():
    out = []
    case, t0, t1 = FRAMES_CASES[0]
    want = frames_expected(case, t0, t1)

    def frames(a, stream):
        blob = container(*case)
        with OnStream(stream) as s:
            o_ = s.out(want.size + 64)
            d = s.up_bytes(blob)
            a.frames_decode_device(d.data_ptr(), len(blob), t0, t1 - t0, o_.data_ptr() + 32, s.cs)
            return s.back(o_)
    out.append(Job("frames", f"device/frames v{case[2]} {case[0]} [{t0}, {t1})", frames, _filled(want.size + 64, 32, want)))

    pcase, p0, p1 = PREVIEW_CASES[1]
    pwant = preview_expected(pcase, p0, p1)

    def preview(a, stream):
        blob = container(*pcase)
        with OnStream(stream) as s:
            o_ = s.out(pwant.size + 64)
            d = s.up_bytes(blob)
            a.preview_decode_device(d.data_ptr(), len(blob), p0, p1 - p0, o_.data_ptr() + 32, s.cs)
            return s.back(o_)
    out.append(Job("preview", f"device/preview v{pcase[2]} {pcase[0]} [{p0}, {p1})", preview, _filled(pwant.size + 64, 32, pwant)))

    # the rectangle pasted into full-size frames: every byte outside it stays 0xEE
    rcase, r0, r1, rect = RECT_CASES[0]
    w, h, _ = rcase[0]
    x, y, rw, rh = rect
    frames_buf = np.full((r1 - r0, h, w, 3), FILL, np.uint8)
    frames_buf[:, y:y + rh, x:x + rw] = rect_expected(rcase, r0, r1, rect).reshape(r1 - r0, rh, rw, 3)

    def rect_run(a, stream):
        blob = container(*rcase)
        with OnStream(stream) as s:
            o_ = s.out(frames_buf.size)
            d = s.up_bytes(blob)
            a.rect_decode_device(d.data_ptr(), len(blob), r0, r1 - r0, x, y, rw, rh, o_.data_ptr() + (y * w + x) * 3, 3 * w, 3 * w * h, s.cs)
            return s.back(o_)
    out.append(Job("rect", f"device/rect v{rcase[2]} {rcase[0]} [{r0}, {r1}) {rect} pasted", rect_run, frames_buf.reshape(-1)))

    wants = [preview_expected(c, a_, b_) for c, a_, b_ in PREVIEWS_ITEMS]
    offs, pos = [], 32
    for wnt in wants:
        offs.append(pos)
        pos += wnt.size + 33
    whole = _filled(pos)
    for off, wnt in zip(offs, wants):
        whole[off:off + wnt.size] = wnt

    def previews(a, stream, rows_of=None):
        with OnStream(stream) as s:
            o_ = s.out(whole.size)
            devs = {}
            rows = []
            for (c, a_, b_), off in zip(PREVIEWS_ITEMS, offs):
                blob = container(*c)
                if c not in devs:
                    devs[c] = s.up_bytes(blob)
                rows.append((devs[c].data_ptr(), len(blob), a_, b_ - a_, o_.data_ptr() + off))
            a.previews_decode_device(rows, s.cs)
            return s.back(o_)
    out.append(Job("previews", f"device/previews {len(wants)} items", previews, whole))
    return out


def _dev_measure_jobs():
    out = []
    shape, kind = (33, 17, 5), CDF97
    w, h, f = shape
    rgb = source(shape)
    other = Q.reconstruct(2, rgb, w, h, f, 50, kind)
    sse_want = np.concatenate([_filled(8), Q.frame_sse(rgb, other, f).astype("<u8").view(np.uint8), _filled(8)])

    def rgb_sse(a, stream):
        with OnStream(stream) as s:
            o_ = s.out(8 * (f + 2))
            da, db = s.up(rgb), s.up(other)
            a.rgb_sse_device(da.data_ptr(), db.data_ptr(), w, h, f, None, None, o_.data_ptr() + 8, s.cs)
            return s.back(o_)
    out.append(Job("quality", f"device/rgb_sse {shape}", rgb_sse, sse_want))

    for version, q, tshape, tkind in ((2, 80, (33, 17, 5), CDF53), (4, 80, (40, 24, 1), HAAR)):
        tw, th, tf = tshape
        pixels = Q.reconstruct(version, source(tshape), tw, th, tf, q, tkind)
        want = (Q.sse_of(source(tshape), pixels),
                np.concatenate([_filled(8), Q.frame_sse(source(tshape), pixels, tf).astype("<u8").view(np.uint8), _filled(8)]))

        def trial(a, stream, version=version, q=q, tshape=tshape, tkind=tkind, tw=tw, th=th, tf=tf):
            with OnStream(stream) as s:
                o_ = s.out(8 * (tf + 2))
                d = s.up(source(tshape))
                sse = a.trial_sse_device(version, d.data_ptr(), tw, th, tf, 1, _wt(a, tkind), q, d_frame_sse_ptr=o_.data_ptr() + 8, stream=s.cs)
                return int(sse[0]), s.back(o_)
        out.append(Job("quality", f"device/trial_sse v{version} {tshape} wavelet {tkind} q {q}", trial, want))

    pshape, pkind = (33, 17, 5), CDF97

    def predict(a, stream):
        with OnStream(stream) as s:
            d = s.up(source(pshape))
            p = a.predict_split_sizes_device(d.data_ptr(), *pshape, 1, _wt(a, pkind), LANE, s.cs)
            return p.lo[0], p.hi[0]
    out.append(Job("rate", f"device/predict_split_sizes {pshape} wavelet {pkind}", predict, tuple(_bracket(pshape, pkind, False))))
    return out


def _dev_segment_jobs():
    out = []
    w, h, n = 50, 38, 3
    cur, ref = motion_frames(w, h, n)
    thr, rd, re = 25, 2, 1
    mask, stats = SG.vec_motion(cur, ref, thr, rd, re)

    def motion(a, stream):
        with OnStream(stream) as s:
            d_stats, d_mask = s.out(n * 5 * 4), s.out(n * h * w + 16)
            dc, dr = s.up(cur), s.up(ref)
            a.segment_motion_device(dc.data_ptr(), dr.data_ptr(), w * h, w, h, n, d_stats.data_ptr(), d_mask.data_ptr(),
                                    a.SegmentConfig(thr, 100, rd, re), s.cs)
            return s.back(d_stats), s.back(d_mask)
    out.append(Job("segment", f"device/segment_motion {n} x {w}x{h}", motion,
                   (np.asarray(stats, "<u4").reshape(-1).view(np.uint8), _filled(n * h * w + 16, 0, mask))))

    flat = np.asarray(mask, np.uint8).reshape(-1)
    rle = SG.vec_rle(flat)

    def rle_run(a, stream):
        with OnStream(stream) as s:
            cap = a.rle_bound(flat.size)
            o_ = s.out(cap + 16)
            d = s.up(flat)
            written = a.rle_encode_mask_device(d.data_ptr(), flat.size, o_.data_ptr(), cap, s.cs)
            host = s.back(o_)
            return int(written), host[:written].tobytes(), bool((host[max(written, cap):] == FILL).all())
    out.append(Job("segment", f"device/rle_encode_mask {flat.size}", rle_run, (len(rle), rle, True)))
    return out


def _dev_batch_job():
    shape, kind, q, n = (50, 38, 13), CDF97, 80, 3
    w, h, f = shape
    chunks = np.stack([source(shape, seed=70 + i) for i in range(n)])
    refs = tuple(oracle.encode(c, w, h, f, q, kind) for c in chunks)

    def run(a, stream):
        from alice_codec_amd import multi
        with OnStream(stream) as s:
            bt = a.Batch(w, h, f, n, q, _wt(a, kind))
            d = s.up(chunks)
            bt.encode(d.data_ptr(), s.cs)
            sizes = bt.encode_finish()
            packed = s.out(int(sizes.sum()) + 16)
            bt.pack_alc(sizes, packed.data_ptr(), int(sizes.sum()), s.cs)
            bt.decode(bt.alc_ptr(0), bt.alc_stride, None, s.cs)
            bt.decode_finish()
            host = s.back(packed)
            pixels = np.stack([multi.DeviceView(bt.rgb_ptr(i), w * h * f * 3).tensor(DEV).cpu().numpy() for i in range(n)])
            return tuple(int(v) for v in sizes), host, pixels
    packed_want = _filled(sum(len(r) for r in refs) + 16, 0, b"".join(refs))
    return Job("v1", f"device/Batch of {n} x {shape} wavelet {kind}", run,
               (tuple(len(r) for r in refs), packed_want, np.stack([np.asarray(oracle.decode(r)) for r in refs])))


def is_strided(expected) -> bool:
    return isinstance(expected, tuple) and len(expected) == 2 and isinstance(expected[0], str) and expected[0] == "stride"


def check_device(job, codec, stream):
    """check() for DEVICE_JOBS: an encode job's expected value depends on the library's stride, so it is built here"""
    if is_strided(job.expected):
        blob = job.expected[1]
        size, host = job.run(codec, stream)
        assert size == len(blob) and same(host, _filled(host.size, 0, blob)), (job.name, "differs from its reference", size, len(blob))
        return size, host
    return check(job, codec, stream)


@functools.lru_cache(maxsize=None)
def device_jobs():
    return tuple([_dev_encode_job(c) for c in (V2_B, V3_A, V4_A)] + [_dev_decode_job(c) for c in (V2_A, V3_B, V4_B)]
                 + _dev_partial_jobs() + _dev_measure_jobs() + _dev_segment_jobs() + [_dev_batch_job()])
