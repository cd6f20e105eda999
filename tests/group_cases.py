"""The plan of the many-group tests (tests/test_call_groups_host.py on the CPU, tests/test_gpu_call_groups.py on the device):
calls of seven chunks that the group hook (alice_codec_test_set_group_chunks) cuts into 7 x 1, 2 + 2 + 2 + 1 and 3 + 3 + 1.

Every chunk of a call differs from every other in content (a seeded smooth-plus-noise clip with a noise amplitude of its
own), in quality and in budget, so that a result written to, or read from, another chunk's row or slot cannot pass.  Every
expected value comes from the CPU references, chunk by chunk, each built once: the oracle's transform and quantiser, the
containers of split_ref / wide_ref / reversible_ref, the brackets and the chooser of split_rate_ref / wide_rate_ref, the
squared errors and the search of quality_ref, the maps of transcode_ref, the version 5 containers and repacks of banded_ref."""
from __future__ import annotations

import functools

import numpy as np

import banded_ref as B5
import oracle.alice_oracle_np as o
import quality_ref as Q
import reversible_ref as R4
import split_rate_ref as SR
import split_ref as R2
import transcode_ref as T
import wide_oracle as WO
import wide_rate_ref as WR
import wide_ref as W3

N = 7                      # chunks per call
CAPS = (1, 2, 3)           # 7 x 1, 2 + 2 + 2 + 1, 3 + 3 + 1: a ragged last group every time
VERDICT_CAP = 3
BIG = 4                    # the chunk with the largest container: second of the second group under VERDICT_CAP
L = 64                     # lane_symbols: a block is 4096 symbols
SHAPES = {
    "tile": (66, 32, 2),       # the tile kernels, 4224 symbols per channel: two lane blocks
    "generic": (3, 40, 4),     # padded width below 6: the generic path
}
KIND = {1: 1, 2: 1, 3: 0, 4: 2}            # wavelet of each version's calls: CDF 9/7, CDF 9/7, CDF 5/3, Haar
# noise amplitude and gradient range (around mid grey) of chunk i; the loudest chunk is BIG.  Found by a search: a quantiser
# step decides most of a PSNR, so seven contents that take seven different qualities under ONE floor are rare
AMPLITUDE = (9, 27, 10, 20, 40, 5, 25)
CONTRAST = (174, 15, 238, 14, 255, 13, 89)
# quality of chunk i: seven quantiser steps, the finest at BIG, inverse instances on both sides of 2 (the host test checks)
QUALITIES = {
    1: (90, 40, 75, 20, 96, 60, 85),
    2: (90, 40, 75, 20, 96, 60, 85),
    3: (97, 50, 99, 30, 100, 80, 92),
    4: (97, 50, 99, 30, 100, 80, 92),
}
BUDGET_RANGE = {2: (10, 95), 3: (10, 100)}     # min_quality, max_quality of the budget encodes
PSNR_RANGE = {2: (5, 96), 3: (5, 100)}         # version 2 up to where its symbols do not wrap
# dB: one floor per call, at which the seven contents choose seven qualities
PSNR_TARGET = {(2, "tile"): 12.9, (3, "tile"): 16.0, (2, "generic"): 13.1, (3, "generic"): 16.7}
TRANSCODE_RANGE = (10, 95)
# the transcodes: quality of source i (all fine enough to leave room below), and its target: mapped / untouched / mapped far,
# BIG untouched (its output stays the largest)
SOURCES = {
    2: (90, 80, 75, 70, 96, 60, 85),
    3: (97, 88, 99, 84, 100, 80, 92),
}
TARGETS = {
    2: (70, 85, 10, 50, 96, 5, 65),
    3: (80, 90, 15, 60, 100, 8, 75),
}
FRAME = (100, 50)          # frames of the region calls, seven origins of a tile-shaped rectangle inside
ORIGINS = ((0, 0), (34, 18), (7, 3), (1, 17), (33, 0), (20, 9), (13, 18))
Q_OF_STEP = WR.q_of_step()


@functools.lru_cache(maxsize=None)
def clip(shape: str, i: int) -> np.ndarray:
    """wide_oracle.smooth_plus_noise with chunk i's seed and noise amplitude"""
    w, h, f = SHAPES[shape]
    rng = np.random.default_rng(1000 * i + w + h + f)
    t, y, x = np.meshgrid(np.arange(f), np.arange(h), np.arange(w), indexing="ij")
    base = np.stack([(x * 255) // max(w - 1, 1), (y * 255) // max(h - 1, 1), ((x + y + 9 * t) * 255) // max(w + h + 9 * f - 3, 1)], axis=-1)
    a, c = AMPLITUDE[i], CONTRAST[i]
    rgb = np.clip((255 - c) // 2 + (base * c) // 255 + rng.integers(-a, a + 1, base.shape), 0, 255).astype(np.uint8).reshape(-1)
    rgb.setflags(write=False)
    return rgb


def clips(shape: str) -> np.ndarray:
    return np.concatenate([clip(shape, i) for i in range(N)])


@functools.lru_cache(maxsize=None)
def _coefficients(shape: str, i: int, kind: int):
    """the oracle's forward transform of the three padded channels (wide_oracle.forward_quantised before its quantiser)"""
    w, h, f = SHAPES[shape]
    out = []
    for ch in o.rgb_to_ycocg_r(clip(shape, i)):
        v, pw, ph, pf = o._pad(ch, w, h, f)
        out.append(o.wavelet3d(kind, v, pw, ph, pf))
    return out


@functools.lru_cache(maxsize=None)
def symbols(version: int, shape: str, i: int, step: int):
    """[Y, Co, Cg] symbols of chunk i at a quantiser step: u8 for version 2, the untruncated z for versions 3 and 4"""
    qs = [np.asarray(o.quantize(c, step, step), np.int64) for c in _coefficients(shape, i, KIND[version])]
    return [o.to_symbols(q) for q in qs] if version == 2 else [W3.wide_symbols(q) for q in qs]


@functools.lru_cache(maxsize=None)
def _container_at_step(version: int, shape: str, i: int, step: int) -> bytes:
    w, h, f = SHAPES[shape]
    write = R2.write_container if version == 2 else W3.write_container
    blob = write(KIND[version], w, h, f, L, (step,) * 3, symbols(version, shape, i, step))
    return R4.with_version(blob, 4) if version == 4 else blob


def container(version: int, shape: str, i: int, quality: int) -> bytes:
    """what the version's encoder writes for chunk i at this quality"""
    return _container_at_step(version, shape, i, SR.quality_to_step(quality))


def containers(version: int, shape: str):
    """the seven containers of a call at QUALITIES[version]"""
    return [container(version, shape, i, QUALITIES[version][i]) for i in range(N)]


def sources(version: int, shape: str):
    """the seven containers a transcode call reads, at SOURCES[version]"""
    return [container(version, shape, i, SOURCES[version][i]) for i in range(N)]


@functools.lru_cache(maxsize=None)
def pixels(version: int, shape: str, i: int, quality: int) -> np.ndarray:
    """what the version's decoder returns for container(version, shape, i, quality)"""
    w, h, f = SHAPES[shape]
    out = Q.reconstruct(version, clip(shape, i), w, h, f, quality, KIND[version])
    out.setflags(write=False)
    return out


def sse(version: int, shape: str, i: int, quality: int) -> int:
    return Q.sse_of(clip(shape, i), pixels(version, shape, i, quality))


def frame_sse(version: int, shape: str, i: int, quality: int) -> np.ndarray:
    return Q.frame_sse(clip(shape, i), pixels(version, shape, i, quality), SHAPES[shape][2])


# ---- sizes before encoding, byte budgets ----

@functools.lru_cache(maxsize=None)
def step_hists(version: int, shape: str, i: int) -> np.ndarray:
    """(64, 3, 256): histograms of the coded symbol of chunk i at every quantiser step"""
    hist = (lambda s: np.bincount(s, minlength=256)) if version == 2 else W3.histogram
    out = np.stack([np.stack([hist(s) for s in symbols(version, shape, i, step)]) for step in range(1, 65)]).astype(np.uint32)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def brackets(version: int, shape: str, i: int):
    """(lo[101], hi[101]) of chunk i's container"""
    return (SR if version == 2 else WR).chunk_prediction(step_hists(version, shape, i), L)


def _budget(rule: str, lo, hi, exact) -> int:
    """a budget that leads the chooser one way, from the brackets and exact sizes of the chunk it is for"""
    return {"hi66": lambda: int(hi[66]),                              # exactly an upper bound
            "exact50": lambda: exact(50),                             # exactly a size: the refinement looks for it
            "exact85": lambda: exact(85),
            "below_exact50": lambda: exact(50) - 1,                   # one byte short of a size
            "below_hi60": lambda: int(hi[60]) - 1,                    # one below an upper bound
            "below_hi45": lambda: int(hi[45]) - 1,
            "inside80": lambda: (int(lo[80]) + int(hi[80])) // 2,     # inside a bracket
            "nothing": lambda: int(lo.min()) - 1,                     # nothing can fit: min_quality, fits = 0
            "everything": lambda: int(hi.max()) + 1}[rule]()          # everything fits: max_quality at once


# rule of chunk i: the flattest chunk (5) takes the one that does not depend on how its sizes spread
ENCODE_BUDGETS = ("hi66", "below_hi60", "nothing", "inside80", "below_exact50", "everything", "exact85")
TRANSCODE_BUDGETS = ("hi66", "below_hi60", "below_hi45", "nothing", "exact50", "everything", "inside80")


@functools.lru_cache(maxsize=None)
def budget_plan(version: int, shape: str):
    """-> [(budget, quality, fits, trials, bytes)] of the seven chunks of a budget encode"""
    min_q, max_q = BUDGET_RANGE[version]
    out = []
    for i in range(N):
        lo, hi = brackets(version, shape, i)
        exact = lambda q, i=i: len(container(version, shape, i, q))   # noqa: E731
        budget = _budget(ENCODE_BUDGETS[i], lo, hi, exact)
        q, fits, trials = SR.choose(lo, hi, budget, min_q, max_q, exact)
        out.append((budget, q, fits, trials, container(version, shape, i, q)))
    return out


# ---- PSNR floors ----

class _StepSSE(dict):
    """{quantiser step: squared error of chunk i}, each entry computed when the search first asks for it"""

    def __init__(self, version, shape, i):
        super().__init__()
        self.key = (version, shape, i)

    def __missing__(self, step):
        self[step] = sse(*self.key, Q_OF_STEP[step])
        return self[step]


@functools.lru_cache(maxsize=None)
def psnr_plan(version: int, shape: str):
    """-> [(quality, reached, trials, dB, bytes)] of the seven chunks of a PSNR-floor encode at PSNR_TARGET[version, shape]"""
    w, h, f = SHAPES[shape]
    n = w * h * f * 3
    min_q, max_q = PSNR_RANGE[version]
    out = []
    for i in range(N):
        table = _StepSSE(version, shape, i)
        q, reached, trials = Q.choose(table, n, PSNR_TARGET[version, shape], min_q, max_q)
        out.append((q, reached, trials, Q.psnr_from_sse(table[Q.step_of(q)], n), container(version, shape, i, q)))
    return out


# ---- transcodes ----

@functools.lru_cache(maxsize=None)
def transcode_plan(version: int, shape: str):
    """-> [bytes] of sources(version, shape) transcoded to TARGETS[version]"""
    return [T.transcode(src, q) for src, q in zip(sources(version, shape), TARGETS[version])]


@functools.lru_cache(maxsize=None)
def transcode_budget_plan(version: int, shape: str):
    """-> [(budget, quality, fits, trials, bytes)] of the seven sources of a budget transcode"""
    min_q, max_q = TRANSCODE_RANGE
    out = []
    for i, src in enumerate(sources(version, shape)):
        lo, hi = T.predict(src)
        exact = lambda q, src=src: len(T.transcode(src, q))   # noqa: E731
        budget = _budget(TRANSCODE_BUDGETS[i], lo, hi, exact)
        out.append((budget,) + T.choose_transcode(src, budget, min_q, max_q))
    return out


# ---- version 5: the banded twins of the containers above, one table per subband (banded_ref) ----

BASES = (2, 3, 4)


@functools.lru_cache(maxsize=None)
def banded(base: int, shape: str, i: int, quality: int) -> bytes:
    """what the banded encoder of this base writes for chunk i at this quality"""
    w, h, f = SHAPES[shape]
    step = SR.quality_to_step(quality)
    return B5.write_container(base, KIND[base], w, h, f, L, (step,) * 3, (step,) * 3, symbols(base, shape, i, step))


def bandeds(base: int, shape: str):
    """the seven version 5 containers of a call at QUALITIES[base]"""
    return [banded(base, shape, i, QUALITIES[base][i]) for i in range(N)]


@functools.lru_cache(maxsize=None)
def to_banded_plan(base: int, shape: str):
    """-> [bytes] of containers(base, shape) repacked to version 5"""
    return [B5.to_banded(b) for b in containers(base, shape)]


@functools.lru_cache(maxsize=None)
def from_banded_plan(base: int, shape: str):
    """-> [bytes] of bandeds(base, shape) repacked to their base version"""
    return [B5.from_banded(b) for b in bandeds(base, shape)]


# ---- an output stride that is one byte short (cap 2) ----

# The chunks of such a call in this order: BIG, whose output is the largest in every family, is chunk STRIDE_AT, the second
# of the second group of two.  Its index in the call (3) is not its index in the group (1), and groups 2 and 3 are never run.
STRIDE_CAP = 2
STRIDE_ORDER = (0, 1, 2, BIG, 3, 5, 6)
STRIDE_AT = 3
STRIDE_FAMILIES = ("split", "wide", "reversible", "banded", "transcode", "to_banded", "from_banded")
STRIDE_BANDED_BASE = 3                     # of the banded encode; the repacks take the two other bases
STRIDE_VERSION = {"split": 2, "wide": 3, "reversible": 4, "banded": STRIDE_BANDED_BASE, "transcode": 3, "to_banded": 2, "from_banded": 4}


def in_stride_order(items):
    return [items[i] for i in STRIDE_ORDER]


@functools.lru_cache(maxsize=None)
def stride_plan(family: str, shape: str = "tile"):
    """-> (inputs or None for the encodes from pixels, outputs) of the family's call, both in STRIDE_ORDER"""
    v = STRIDE_VERSION[family]
    if family in ("split", "wide", "reversible"):
        return None, in_stride_order(containers(v, shape))
    if family == "banded":
        return None, in_stride_order(bandeds(v, shape))
    if family == "transcode":
        return in_stride_order(sources(v, shape)), in_stride_order(transcode_plan(v, shape))
    if family == "to_banded":
        return in_stride_order(containers(v, shape)), in_stride_order(to_banded_plan(v, shape))
    return in_stride_order(bandeds(v, shape)), in_stride_order(from_banded_plan(v, shape))


def damaged(blob: bytes) -> bytes:
    """a flipped byte in a lane stream of the first block of the first channel"""
    info = (R2 if blob[4] == 2 else W3).parse_container(R4.with_version(blob, 3) if blob[4] == 4 else blob)
    bad = bytearray(blob)
    bad[R2.HEADER + 4 * info["n_blocks"][0] + 128 + 9] ^= 0x40
    return bytes(bad)


# ---- two sample widths in one decode group, under a band target that cuts the two plans differently ----

MIXED_SHAPE = (256, 256, 16)
MIXED_BAND_KB = 4096
MIXED_KIND = 1
MIXED_QUALITIES = {1: (80, 40), 2: (80, 40), 3: (100, 80), 4: (100, 80)}   # (an i16 step, an i32 step) of CDF 9/7


@functools.lru_cache(maxsize=None)
def mixed_clip() -> np.ndarray:
    rgb = WO.smooth_plus_noise(*MIXED_SHAPE, seed=2)
    rgb.setflags(write=False)
    return rgb


@functools.lru_cache(maxsize=None)
def mixed_container(version: int, quality: int) -> bytes:
    """versions 2, 3 and 4 (version 1 comes from the C oracle)"""
    w, h, f = MIXED_SHAPE
    if version == 4:
        return R4.with_version(mixed_container(3, quality), 4)
    step, _, qs = WO.forward_quantised(o, mixed_clip(), w, h, f, quality, MIXED_KIND)
    if version == 2:
        return R2.write_container(MIXED_KIND, w, h, f, L, (step,) * 3, [o.to_symbols(q) for q in qs])
    return W3.write_container(MIXED_KIND, w, h, f, L, (step,) * 3, [W3.wide_symbols(q) for q in qs])


@functools.lru_cache(maxsize=None)
def mixed_pixels(version: int, quality: int) -> np.ndarray:
    w, h, f = MIXED_SHAPE
    out = Q.reconstruct(version, mixed_clip(), w, h, f, quality, MIXED_KIND)
    out.setflags(write=False)
    return out
