"""The case table of the squared-error kernel (alice-codec_amd/csrc/quality.hip), and the model of its work split that says
which class a case falls into.  The limits come from csrc/kernels.h by name, so a change of a constant moves the cases with
it; tests/test_quality_host.py holds the table to every class the constants define."""
from __future__ import annotations

import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS_H = os.path.join(ROOT, "alice-codec_amd", "csrc", "kernels.h")


def kernel_constants() -> dict:
    text = open(KERNELS_H).read()
    out = {}
    for name in ("kSseBlock", "kSseVectorsPerLane", "kSseLaneFlushVectors", "kSseMaxBlocks"):
        m = re.search(r"constexpr\s+uint32_t\s+" + name + r"\s*=\s*(\d+)\s*;", text)
        assert m, f"{name} is not a named constant of kernels.h"
        out[name] = int(m.group(1))
    return out


K = kernel_constants()
BLOCK, VPL, FLUSH, MAX_BLOCKS = K["kSseBlock"], K["kSseVectorsPerLane"], K["kSseLaneFlushVectors"], K["kSseMaxBlocks"]
PER_VB = BLOCK * VPL                      # windows of a virtual block
FLUSH_VB = FLUSH // VPL                   # virtual blocks of one frame a lane takes before it must fold
MAX_TERM = 255 * 255
GUARD = 64                                # guard bytes around every buffer (0 on side a, 255 on side b)


class Case:
    """Two volumes of n frames of w x h RGB.  Side s sits at byte offset off[s] of a 256-aligned allocation (behind the guard),
    with row pitch 3w + row_pad[s] and frame pitch rows + frame_pad[s].  content: 'random', 'extreme' (all 0 against all 255)
    or 'count' (frame k sums to exactly k + 1: it differs in k + 1 bytes by 1 each while the frame has as many bytes, and by
    2 or 3 in as few bytes as it takes beyond that).  cap: alice_codec_test_set_grid_cap for the launch (0: none)."""

    def __init__(self, name, w, h, n, off=(0, 0), row_pad=(0, 0), frame_pad=(0, 0), content="random", cap=0):
        self.name, self.w, self.h, self.n = name, w, h, n
        self.off, self.row_pad, self.frame_pad, self.content, self.cap = off, row_pad, frame_pad, content, cap

    def __repr__(self):
        return self.name

    def row_pitch(self, s):
        return 3 * self.w + self.row_pad[s]

    def frame_pitch(self, s):
        return (self.h - 1) * self.row_pitch(s) + 3 * self.w + self.frame_pad[s]

    def span(self, s):
        return (self.n - 1) * self.frame_pitch(s) + (self.h - 1) * self.row_pitch(s) + 3 * self.w

    # ---- the kernel's work split, restated ----
    def flat(self):
        return self.h == 1 or (self.row_pad[0] == 0 and self.row_pad[1] == 0)

    def run_len(self):
        return 3 * self.w * self.h if self.flat() else 3 * self.w

    def runs(self):
        return 1 if self.flat() else self.h

    def vb_per_frame(self):
        nwin = (15 + self.run_len() + 15) // 16
        return -(-self.runs() * nwin // PER_VB)

    def grid(self):
        g = self.vb_per_frame() * self.n
        if self.cap:
            g = min(g, self.cap)
        return min(g, MAX_BLOCKS)

    def flush_class(self):
        """'below' / 'at' / 'above' the fold limit for the workgroup that takes the most virtual blocks of one frame in a row."""
        most = -(-self.vb_per_frame() // self.grid())   # a workgroup takes every grid-th virtual block; held restarts per frame
        return "below" if most < FLUSH_VB else ("at" if most == FLUSH_VB else "above")

    def classes(self):
        c = {"flat" if self.flat() else "rows", "flush:" + self.flush_class(), "a%16=" + str(self.off[0] % 16),
             "b-a%16=" + str((self.off[1] - self.off[0]) % 16), "len%16=" + str(self.run_len() % 16)}
        if self.run_len() < 16:
            c.add("run<window")
        if self.vb_per_frame() > 1:
            c.add("frame>vb")
        if self.vb_per_frame() * self.n > self.grid():
            c.add("grid-stride")
        if self.vb_per_frame() == 1 and self.n > self.grid():
            c.add("frames-per-workgroup>1")
        if self.row_pad[0] != self.row_pad[1]:
            c.add("pitches-differ")
        if MAX_TERM * 3 * self.w * self.h >= 1 << 32 and self.content == "extreme":
            c.add("frame>=2^32")
        return c

    # ---- data ----
    def build(self, seed=0):
        """-> (buf_a, buf_b) host arrays with guards, and the per-frame reference in u64 (numpy, int64 arithmetic)."""
        rng = np.random.default_rng(seed)
        bufs, views = [], []
        for s in range(2):
            total = GUARD + self.off[s] + self.span(s) + GUARD + 16
            buf = np.full(total, 0 if s == 0 else 255, np.uint8)
            # (what lies between the rows and frames keeps the guard value too)
            bufs.append(buf)
            base = GUARD + self.off[s]
            v = np.lib.stride_tricks.as_strided(buf[base:], shape=(self.n, self.h, 3 * self.w),
                                                strides=(self.frame_pitch(s), self.row_pitch(s), 1), writeable=True)
            views.append(v)
        a, b = views
        if self.content == "extreme":
            a[...] = 0
            b[...] = 255
        elif self.content == "count":
            x = rng.integers(0, 250, (self.n, self.h, 3 * self.w), dtype=np.uint8)
            a[...] = x
            y = x.reshape(self.n, -1).copy()
            for k in range(self.n):
                d = count_terms(k + 1, y.shape[1])
                y[k, :len(d)] += np.array(d, np.uint8)
            b[...] = y.reshape(x.shape)
        else:
            a[...] = rng.integers(0, 256, a.shape, dtype=np.uint8)
            b[...] = rng.integers(0, 256, b.shape, dtype=np.uint8)
        d = a.astype(np.int64) - b.astype(np.int64)
        ref = (d * d).reshape(self.n, -1).sum(axis=1).astype(np.uint64)
        return bufs[0], bufs[1], ref


def count_terms(total: int, slots: int) -> list:
    """Differences of 1 (as many as fit), else 2 and 3, whose squares sum to `total` in at most `slots` bytes."""
    terms, rem = [], total
    for d in (3, 2):
        while rem >= d * d and rem > slots - len(terms):
            terms.append(d)
            rem -= d * d
    terms += [1] * rem
    assert len(terms) <= slots and sum(t * t for t in terms) == total
    return terms


def _flat_width(vb: int, largest: bool) -> int:
    """A width w with h = 1 whose 3w bytes take exactly `vb` virtual blocks: the largest such w, or the smallest."""
    if largest:
        return (16 * PER_VB * vb - 15) // 3            # floor((3w + 30) / 16) <= PER_VB * vb
    return -(-(16 * PER_VB * (vb - 1) - 14) // 3)      # floor((3w + 30) / 16) >= PER_VB * (vb - 1) + 1


def cases() -> list:
    out = [Case("1x1x1", 1, 1, 1)]
    # every residue of 3w mod 16, flat and by rows (pitched against packed, packed against pitched, both with other pitches)
    for w in range(1, 18):
        out.append(Case(f"w{w}-flat", w, 3, 2, off=(0, 0)))
        out.append(Case(f"w{w}-pitched-a", w, 3, 2, row_pad=(7, 0), frame_pad=(5, 0)))
        out.append(Case(f"w{w}-pitched-b", w, 3, 2, row_pad=(0, 9), frame_pad=(0, 3)))
        out.append(Case(f"w{w}-pitched-both", w, 3, 2, row_pad=(13, 6), frame_pad=(1, 34)))
    # base pointers at every byte offset
    for k in range(16):
        out.append(Case(f"a+{k}", 23, 5, 3, off=(k, 5)))
        out.append(Case(f"b+{k}", 23, 5, 3, off=(3, k)))
        out.append(Case(f"a+{k}-rows", 23, 5, 3, off=(k, 5), row_pad=(2, 11)))
        out.append(Case(f"b+{k}-rows", 23, 5, 3, off=(3, k), row_pad=(11, 2)))
    # frames cannot be swapped or merged
    out.append(Case("300-frames", 5, 3, 300, content="count"))
    out.append(Case("300-frames-cap7", 5, 3, 300, content="count", cap=7))
    out.append(Case("300-frames-rows", 5, 3, 300, content="count", row_pad=(3, 0)))
    # a frame's sum past 32 bits
    out.append(Case("frame-sum-2^32", 160, 140, 2, content="extreme"))
    out.append(Case("frame-sum-2^32-rows", 160, 140, 2, content="extreme", row_pad=(0, 4), off=(1, 2)))
    # several virtual blocks per frame, several trips
    out.append(Case("multi-vb", 211, 97, 3, off=(9, 2), cap=2))
    out.append(Case("multi-vb-rows", 211, 97, 3, off=(9, 2), row_pad=(5, 0), cap=2))
    # the per-lane fold: one workgroup takes a whole frame of maximal terms
    side = 1
    while 3 * side * side <= (FLUSH * 16 + 4) * BLOCK:     # 2400 for 256 lanes: bytes > 66 052 * lanes
        side += 1
    side = -(-side // 100) * 100
    out.append(Case(f"fold-{side}sq-cap1", side, side, 1, content="extreme", cap=1))
    out.append(Case(f"fold-{side}sq-cap3", side, side, 1, content="extreme", cap=3))
    # a stride of the grid that is whole frames plus some segments (7 workgroups over frames of 3 virtual blocks)
    out.append(Case("stride-frames-and-segments", 211, 150, 9, off=(4, 11), cap=7))
    out.append(Case("stride-frames-and-segments-rows", 211, 150, 9, off=(4, 11), row_pad=(0, 7), cap=7))
    # the fold limit itself under one workgroup: a frame of one virtual block less than a lane may hold, of exactly as many
    # (every block as full as it gets), of one window more (base at the last byte of a line, so that the window exists), and
    # of one whole virtual block more: without the fold nearly every lane would hold FLUSH + VPL whole maximal windows there
    out.append(Case("fold-limit-below", _flat_width(FLUSH_VB - 1, True), 1, 1, content="extreme", cap=1))
    out.append(Case("fold-limit-at", _flat_width(FLUSH_VB, True), 1, 1, content="extreme", cap=1))
    out.append(Case("fold-limit-past", _flat_width(FLUSH_VB + 1, False), 1, 1, off=(15, 0), content="extreme", cap=1))
    out.append(Case("fold-limit-past-whole-block", _flat_width(FLUSH_VB + 1, True), 1, 1, content="extreme", cap=1))
    return out
