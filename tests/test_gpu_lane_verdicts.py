"""One damaged payload, one verdict: the four lane decoders of split.hip (every block, every block of wide symbols, the blocks
of a frame range, the blocks of a preview) run one chain (the frame-range decoder a copy of it), so the same damage in a
block all of them read must be
refused by all of them with the same error code and the same message, and a refused partial decode must leave its output
alone.  Each decoder has its own test file; a clamp or an end check that drifted in one of them would pass there and show
here.

frames = 4, 16x16 pixels, lane length 64 (the smallest): a channel is 1024 symbols, a single block that every path plans.
32x32x16 is there for the plan that is a strict subset: four blocks per channel, of which frames [0, 1) and their preview
plan blocks 0 and 2.  The damage is every stream flip and lane-directory flip of test_gpu_split.corruption_cases over the
payload of channel 0 that falls into block 0: it holds the low-low quadrant of plane 0, so the whole decode, the range and
the preview all read it.  Versions 2 and 3.  Every case goes through the numpy restatement on the CPU first: what it
refuses every call must refuse, and the few flips that leave another valid stream behind every call must accept.

Nothing here is built to fault the device: every read of the lane decoders is clamped to its lane stream and every store
to its block or compact volume, so a damaged payload ends in a verdict.  The whole-chunk device decodes queue their
inverse before the verdict is read (their output on a refusal is unspecified), so for them only the bytes
around the output are held to the guard pattern; the range and the preview must not write a byte."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frames_ref as FR  # noqa: E402
import preview_ref as PR  # noqa: E402
import split_ref as R2  # noqa: E402
import wide_ref as R3  # noqa: E402
from test_gpu_frames import GUARD, Chunk, _channel_layout  # noqa: E402
from test_gpu_split import corruption_cases  # noqa: E402

pytestmark = pytest.mark.gpu

L = 64
KIND = FR.CDF53
T0, T1 = 0, 1
# header layout: 22 bytes of fixed fields, then 536 per channel, whose 256 u16 frequencies follow 24 bytes
# of fields (step, dead zone, num_symbols, n_blocks, payload_len)
FIXED_HEADER, CHANNEL_HEADER, CHANNEL_FIELDS = 22, 536, 24
VERDICTS = ("InvalidBitstream: stream 0: block or lane directory does not add up",
            "InvalidBitstream: stream 0: a lane failed its end check")


def _block0_cases(blob, seed):
    """(name, damaged container) for the flips of corruption_cases that fall into block 0 of channel 0"""
    lane_symbols, lay = _channel_layout(blob)
    pos, nb, offs, lens, plen, ns = lay[0]
    lo, hi = int(offs[0]), int(offs[0] + lens[0])
    out = []
    for name, bad in corruption_cases(blob[pos:pos + plen], ns, lane_symbols, seed):
        m = re.match(r"(stream|lane directory) flip \d+ at (\d+)$", name)
        if m and lo <= int(m.group(2)) < hi:
            assert len(bad) == plen
            out.append((name, blob[:pos] + bad + blob[pos + plen:]))
    return out


def _outcome(a, call):
    """(error code, message) of a refused call, None of one that went through"""
    try:
        call()
    except a.CodecError as e:
        return e.code, str(e)
    return None


@pytest.mark.parametrize("version", [2, 3])
@pytest.mark.parametrize("shape", [(16, 16, 4), (32, 32, 16)], ids=lambda s: "x".join(map(str, s)))
def test_one_damage_one_verdict(gpu_codec, shape, version):
    a = gpu_codec
    w, h, f = shape
    ch = Chunk(a, version, shape, KIND, q={2: 96, 3: 100}[version], seed=3, lane=L)
    plan, pplan = FR.frame_plan(KIND, w, h, f, L, T0, T1), PR.preview_plan(KIND, w, h, f, L, T0, T1)
    assert 0 in plan["planned"] and 0 in pplan["planned"]
    if shape == (32, 32, 16):
        assert plan["n_blocks"] == 4 and plan["planned"] == [0, 2] and list(pplan["planned"]) == [0, 2]
    else:
        assert plan["n_blocks"] == 1
    freq = np.frombuffer(ch.blob, "<u2", 256, FIXED_HEADER + 0 * CHANNEL_HEADER + CHANNEL_FIELDS).astype(np.uint16)   # channel 0
    ref_decode = R2.decode_channel if version == 2 else R3.decode_channel
    full_host = {2: a.decode_split, 3: a.decode_wide}[version]
    full_dev = {2: a.split_decode_device, 3: a.wide_decode_device}[version]
    out = ch.out.data_ptr() + GUARD
    n_full = f * ch.frame_bytes
    cases = _block0_cases(ch.blob, seed=7 + version)
    assert len(cases) >= 4, len(cases)
    _, lay = _channel_layout(ch.blob)
    pos, plen, ns = lay[0][0], lay[0][4], lay[0][5]
    refused = 0
    for name, bad in cases:
        # (a flip can leave another valid stream behind, a bit of an escape's residual for one: then nobody may refuse it)
        _, ref_ok = ref_decode(bad[pos:pos + plen], freq, L, ns)
        refused += not ref_ok
        ch.set_container(bad)
        ptr, size = ch.alc_view.data_ptr(), ch.alc_len
        got = {"decode": _outcome(a, lambda: full_host(bad)),
               "decode_frames": _outcome(a, lambda: a.decode_frames(bad, T0, T1 - T0)),
               "decode_preview": _outcome(a, lambda: a.decode_preview(bad, T0, T1 - T0))}
        for call in (a.frames_decode_device, a.preview_decode_device):
            ch.out.copy_(ch.pattern)
            got[call.__name__] = _outcome(a, lambda: call(ptr, size, T0, T1 - T0, out))
            assert ref_ok or ch.untouched(), (name, call.__name__, "a refused partial decode wrote to its output")
        ch.out.copy_(ch.pattern)
        got["decode_device"] = _outcome(a, lambda: full_dev(ptr, size, [size], out))
        torch.cuda.synchronize()
        assert torch.equal(ch.out[:GUARD], ch.pattern[:GUARD]) and torch.equal(ch.out[GUARD + n_full:], ch.pattern[GUARD + n_full:]), name
        verdict = None if ref_ok else (4, VERDICTS[0 if "lane directory" in name else 1])
        assert all(v == verdict for v in got.values()), (name, verdict, got)
    assert refused >= 4, refused
    # nothing of a refusal stays behind
    ch.set_container(ch.blob)
    assert torch.equal(ch.dev_frames(T0, T1), ch.want_dev(T0, T1))
