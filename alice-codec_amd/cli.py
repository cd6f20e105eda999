"""Command-line front end with the reference CLI's interface (src/bin/main.rs:34-196):
    python -m alice_codec_amd.cli encode INPUT -o OUT.alc -W 1920 -H 1080 -f 64 [-q 90] [-w cdf53|cdf97|haar]
    python -m alice_codec_amd.cli decode INPUT.alc -o OUT.rgb
    python -m alice_codec_amd.cli info INPUT.alc
`encode --format split [--lane-symbols N]` writes the split-stream container (.alc version 2);
`--format wide` the wide container (.alc version 3, section 11: the one whose video comes back at the top of the quality
scale); `--max-bytes` and `encode-chunks --kbps` work in v1 and split, and are still refused with `--format wide` here (the
library has the version 3 budget encode, `encode_wide_to_size`; this front end does not call it yet);
`--format reversible` the reversible container (.alc version 4, section 12: version 3 with the mirrored inverse, lossless at
quality 100), and `--lossless` is short for `--format reversible --quality 100`; version 4 has no byte budget, so
`--max-bytes` and `--kbps` are refused with it;
`--min-psnr DB` (encode and encode-chunks, `--format split` or `--format wide` only) codes each chunk at
the lowest quality in [--min-quality, --max-quality] whose measured PSNR reaches DB, and prints the chosen quality, the
measured dB and whether the floor was reached per chunk; it is refused for the default format, for `reversible` /
`--lossless`, and together with `--max-bytes` / `--kbps`;
`decode` and `info` pick the format from the version byte unless `--format` names one.  The default of every subcommand
is version 1.
`decode --frames A:B` (A alone: one frame) writes frames [A, B) of a version 2, 3 or 4 file from the blocks they need
(DESIGN.md section 14): the file is mapped, so only the header, the block-length tables and those blocks are read;
version 1 is refused with the library's message.
`decode --rect X,Y,W,H` (alone: every frame; or with `--frames`) writes the W x H pixels at (X, Y) as packed W x H frames,
from the blocks they need, through the same mapped file; with `--preview` it is refused.
`thumbnails IN [IN ...] -o OUT [--frame K | --every N]` writes preview frame K (default 0) of every input, or every N-th
frame of every input, back to back: one batched call per 1024 items over mapped files, such as the
PREFIX.NNNNN.alc files of `encode-chunks`; inputs whose preview sizes differ, and version 1 inputs, are refused.
`extract IN [IN ...] -o OUT [--rect X,Y,W,H] [--frame K | --every N]` is its full-resolution twin: whole frames, or the W x H
pixels at (X, Y), of frame K (default 0) or of every N-th frame of every input, back to back, one batched call per 1024
items over mapped files; inputs whose output sizes differ, and version 1 inputs, are refused.
`transcode IN -o OUT (--quality Q | --max-bytes N [--min-quality A --max-quality B]) [--lane-symbols L] [--to-version V]`
writes a version 2, 3 or 4 file again at a lower quality or under a byte budget, from its symbols alone (DESIGN.md section
19): no pixels, no transform.  A quality at or above the file's returns its bytes; `--to-version` 3 or 4 exchanges the two
wide versions; a version 4 result has no byte budget (ask for `--to-version 3`); version 1 is refused.
`--banded` (encode and encode-chunks, beside `--format split|wide|reversible` or `--lossless`) writes the banded container
(.alc version 5, DESIGN.md section 20: one frequency table per wavelet subband, the pixels of the named format in fewer bytes
at chunk sizes); it is refused with the default format, `--max-bytes`, `--kbps` and `--min-psnr`, which version 5 does not
have: encode the base format and `repack` it.
`repack IN -o OUT (--banded | --plain) [--lane-symbols L]` turns a version 2, 3 or 4 file into its version 5 twin or back,
byte for byte what the encoders write, from the symbols alone.  `decode --frames / --rect / --preview`, `thumbnails`,
`extract` and `transcode` refuse a version 5 file with the library's message: `repack --plain` it first.
Like the reference it treats the whole input file as ONE chunk (src/bin/main.rs:117-122).  `encode-chunks`
is the extension SURVEY.md section 8f asks for: it cuts a long raw-RGB file into 64-frame chunks
(DEFAULT_CHUNK_SIZE, src/lib.rs:110) and writes one .alc per chunk."""
from __future__ import annotations

import argparse
import sys

import numpy as np

from . import (DEFAULT_CHUNK_SIZE, PREVIEWS_MAX_ITEMS, RECTS_MAX_ITEMS, CodecError, EncodedChunk, FrameDecoder, FrameEncoder, WaveletType, budget_bytes_per_chunk,
               alc_version, banded_info, decode_banded, encode_banded, from_banded, to_banded, decode_frames, decode_preview, decode_previews, decode_rect, decode_rects, decode_reversible, decode_split, decode_wide, encode_many, encode_reversible, encode_split,
               encode_split_to_psnr, encode_split_to_size, encode_to_size, encode_wide, encode_wide_to_psnr, reversible_info,
               split_info, transcode, transcode_to_size, wide_info)

WAVELETS = {"cdf53": WaveletType.Cdf53, "cdf97": WaveletType.Cdf97, "haar": WaveletType.Haar}
WAVELET_NAMES = {WaveletType.Cdf53: "CDF 5/3", WaveletType.Cdf97: "CDF 9/7", WaveletType.Haar: "Haar"}


def parse_wavelet(s: str) -> WaveletType:
    if s not in WAVELETS:
        raise ValueError(f"unknown wavelet '{s}'; expected cdf53, cdf97, or haar")
    return WAVELETS[s]


FORMAT_VERSION = {"v1": 1, "split": 2, "wide": 3, "reversible": 4}
NO_WIDE_BUDGET = ("--format wide cannot be combined with {} on the command line yet: call encode_wide_to_size from the library for a "
                  "version 3 byte budget, or use --format split or v1 here")


NO_REVERSIBLE_BUDGET = ("--format reversible cannot be combined with {}: version 4 is the lossless container (quality 100 has no "
                        "quality to search, and a lossy version 4 is not recommended); use --format wide, split or v1 for a byte budget")
LOSSLESS_CONFLICT = "--lossless is --format reversible --quality 100: it cannot be combined with {}"
CONTAINER_INFO = {2: split_info, 3: wide_info, 4: reversible_info, 5: banded_info}
CONTAINER_DECODE = {2: decode_split, 3: decode_wide, 4: decode_reversible, 5: decode_banded}
CONTAINER_NAME = {2: "split-stream (version 2)", 3: "wide split-stream (version 3)", 4: "reversible split-stream (version 4)",
                  5: "banded split-stream (version 5)"}
NO_BANDED_V1 = ("--banded needs --format split, wide or reversible (or --lossless): version 5 keeps the symbols of one of them; "
                "an existing file of those formats becomes banded with `repack --banded`")
NO_BANDED_RATE = ("--banded cannot be combined with {}: version 5 has no size prediction, byte budget or PSNR floor; encode without "
                  "--banded and run `repack --banded` on the result")


def _check_banded(a, budget_flag: str, budget) -> None:
    """The refusals of --banded, before the input is read (a.format: after --lossless has been applied; --min-psnr is
    refused ahead of its own checks, by the callers)."""
    if not a.banded:
        return
    if a.format not in ("split", "wide", "reversible"):
        raise ValueError(NO_BANDED_V1)
    if budget is not None:
        raise ValueError(NO_BANDED_RATE.format(budget_flag))


def _apply_lossless(a) -> None:
    """--lossless: --format reversible --quality 100, refused together with another format or quality."""
    if not a.lossless:
        if a.quality is None:
            a.quality = 90
        return
    if a.format not in (None, "reversible"):
        raise ValueError(LOSSLESS_CONFLICT.format(f"--format {a.format}"))
    if a.quality not in (None, 100):
        raise ValueError(LOSSLESS_CONFLICT.format(f"--quality {a.quality}"))
    a.format, a.quality = "reversible", 100


NO_PSNR_FORMAT = ("--min-psnr needs --format split or --format wide: version 1 has no quality to control (its decoder desynchronises on "
                  "almost all content)")
NO_REVERSIBLE_PSNR = ("--min-psnr cannot be combined with {}: version 4 is the lossless container (quality 100 has no quality to "
                      "search, and a lossy version 4 is not recommended); use --format wide or split for a PSNR floor")
PSNR_AND_BUDGET = "--min-psnr and {} are two rate controls: give one of them"


def _check_min_psnr(a, budget_flag: str, budget) -> None:
    """The refusals of --min-psnr, before --lossless is applied and before the input is read."""
    if a.min_psnr is None:
        return
    if a.lossless:
        raise ValueError(NO_REVERSIBLE_PSNR.format("--lossless"))
    if a.format == "reversible":
        raise ValueError(NO_REVERSIBLE_PSNR.format("--format reversible"))
    if a.format not in ("split", "wide"):
        raise ValueError(NO_PSNR_FORMAT)
    if budget is not None:
        raise ValueError(PSNR_AND_BUDGET.format(budget_flag))
    if a.min_psnr != a.min_psnr or a.min_psnr < 0:
        raise ValueError("--min-psnr must be a number of dB >= 0 (inf for exact)")


def _encode_to_psnr(a, wt, rgb, frames):
    """One chunk under --min-psnr -> (bytes, the line that reports it)."""
    fn = encode_split_to_psnr if a.format == "split" else encode_wide_to_psnr
    data, quality, reached, db = fn(rgb, a.width, a.height, frames, a.min_psnr, wt, a.min_quality, a.max_quality, a.lane_symbols)
    line = f"chosen quality: {quality}, measured {db:.2f} dB, floor {a.min_psnr:g} dB {'reached' if reached else 'NOT reached'}"
    return data, quality, reached, line


def _container_version(a, data) -> int:
    """The version a decode / info run treats the file as: the version byte, or the one --format names."""
    return alc_version(data) if a.format == "auto" else FORMAT_VERSION[a.format]


def cmd_encode(a) -> None:
    wt = parse_wavelet(a.wavelet)
    if a.banded and a.min_psnr is not None:
        raise ValueError(NO_BANDED_RATE.format("--min-psnr"))
    _check_min_psnr(a, "--max-bytes", a.max_bytes)
    _apply_lossless(a)
    _check_banded(a, "--max-bytes", a.max_bytes)
    a.format = a.format or "v1"
    if a.format == "wide" and a.max_bytes is not None:
        raise ValueError(NO_WIDE_BUDGET.format("--max-bytes"))
    if a.format == "reversible" and a.max_bytes is not None:
        raise ValueError(NO_REVERSIBLE_BUDGET.format("--max-bytes"))
    rgb = np.fromfile(a.input, dtype=np.uint8)
    quality = a.quality
    if a.banded:
        data = encode_banded(FrameEncoder.with_wavelet(a.quality, wt), rgb, a.width, a.height, a.frames, a.lane_symbols, FORMAT_VERSION[a.format])
        with open(a.output, "wb") as f:
            f.write(data)
        ratio = 0.0 if rgb.size == 0 else len(data) / rgb.size
        print(f"encoded {a.width}x{a.height}x{a.frames} ({rgb.size} bytes) -> {len(data)} bytes "
              f"({ratio * 100:.1f}% ratio, quality={quality}, wavelet={a.wavelet}, format=banded {a.format})", file=sys.stderr)
        return
    if a.min_psnr is not None:
        data, quality, reached, line = _encode_to_psnr(a, wt, rgb, a.frames)
        print(line, file=sys.stderr)
        if not reached:
            print(f"warning: not even --max-quality {a.max_quality} reaches {a.min_psnr:g} dB; encoded at {quality}", file=sys.stderr)
        with open(a.output, "wb") as f:
            f.write(data)
        ratio = 0.0 if rgb.size == 0 else len(data) / rgb.size
        print(f"encoded {a.width}x{a.height}x{a.frames} ({rgb.size} bytes) -> {len(data)} bytes "
              f"({ratio * 100:.1f}% ratio, quality={quality}, wavelet={a.wavelet}, format={a.format})", file=sys.stderr)
        return
    if a.format in ("wide", "reversible"):
        encode_one = encode_reversible if a.format == "reversible" else encode_wide
        data = encode_one(FrameEncoder.with_wavelet(a.quality, wt), rgb, a.width, a.height, a.frames, a.lane_symbols)
        with open(a.output, "wb") as f:
            f.write(data)
        ratio = 0.0 if rgb.size == 0 else len(data) / rgb.size
        print(f"encoded {a.width}x{a.height}x{a.frames} ({rgb.size} bytes) -> {len(data)} bytes "
              f"({ratio * 100:.1f}% ratio, quality={quality}, wavelet={a.wavelet}, format={a.format})", file=sys.stderr)
        return
    if a.format == "split":
        if a.max_bytes is not None:
            data, quality, fits = encode_split_to_size(rgb, a.width, a.height, a.frames, a.max_bytes, wt, a.min_quality, a.max_quality,
                                                       a.lane_symbols)
            print(f"chosen quality: {quality}", file=sys.stderr)
            if not fits:
                print(f"warning: not even --min-quality {a.min_quality} is guaranteed to fit {a.max_bytes} bytes; "
                      f"encoded at {quality}", file=sys.stderr)
        else:
            data = encode_split(FrameEncoder.with_wavelet(a.quality, wt), rgb, a.width, a.height, a.frames, a.lane_symbols)
        with open(a.output, "wb") as f:
            f.write(data)
        ratio = 0.0 if rgb.size == 0 else len(data) / rgb.size
        print(f"encoded {a.width}x{a.height}x{a.frames} ({rgb.size} bytes) -> {len(data)} bytes "
              f"({ratio * 100:.1f}% ratio, quality={quality}, wavelet={a.wavelet}, format=split)", file=sys.stderr)
        return
    if a.max_bytes is not None:
        chunk, quality, fits = encode_to_size(rgb, a.width, a.height, a.frames, a.max_bytes, wt, a.min_quality, a.max_quality)
        print(f"chosen quality: {quality}", file=sys.stderr)
        if not fits:
            print(f"warning: not even --min-quality {a.min_quality} is guaranteed to fit {a.max_bytes} bytes; "
                  f"encoded at {quality}", file=sys.stderr)
    else:
        chunk = FrameEncoder.with_wavelet(a.quality, wt).encode(rgb, a.width, a.height, a.frames)
    data = chunk.to_bytes()
    with open(a.output, "wb") as f:
        f.write(data)
    ratio = 0.0 if rgb.size == 0 else len(data) / rgb.size
    print(f"encoded {a.width}x{a.height}x{a.frames} ({rgb.size} bytes) -> {len(data)} bytes "
          f"({ratio * 100:.1f}% ratio, quality={quality}, wavelet={a.wavelet})", file=sys.stderr)


def cmd_encode_chunks(a) -> None:
    wt = parse_wavelet(a.wavelet)
    if a.banded and a.min_psnr is not None:
        raise ValueError(NO_BANDED_RATE.format("--min-psnr"))
    _check_min_psnr(a, "--kbps", a.kbps)
    _apply_lossless(a)
    _check_banded(a, "--kbps", a.kbps)
    a.format = a.format or "v1"
    if a.format == "wide" and a.kbps is not None:
        raise ValueError(NO_WIDE_BUDGET.format("--kbps"))
    if a.format == "reversible" and a.kbps is not None:
        raise ValueError(NO_REVERSIBLE_BUDGET.format("--kbps"))
    frame_bytes = a.width * a.height * 3
    rgb = np.memmap(a.input, dtype=np.uint8, mode="r")
    if frame_bytes == 0 or rgb.size % frame_bytes:
        raise ValueError("input size is not a whole number of frames")
    n_frames = rgb.size // frame_bytes
    if a.kbps is not None:
        _encode_chunks_to_rate(a, wt, rgb, frame_bytes, n_frames)
        return
    enc = FrameEncoder.with_wavelet(a.quality, wt)
    starts = list(range(0, n_frames, a.chunk))
    if a.min_psnr is not None:   # one chunk uses the whole device: chunk after chunk
        for k, s0 in enumerate(starts):
            f = min(a.chunk, n_frames - s0)
            data, _, _, line = _encode_to_psnr(a, wt, np.ascontiguousarray(rgb[s0 * frame_bytes:(s0 + f) * frame_bytes]), f)
            with open(f"{a.output}.{k:05d}.alc", "wb") as out:
                out.write(data)
            print(f"chunk {k}: frames {s0}..{s0 + f - 1} -> {len(data)} bytes, {line}", file=sys.stderr)
        return
    if a.format in ("split", "wide", "reversible"):   # one chunk uses the whole device: chunk after chunk
        encode_one = {"split": encode_split, "wide": encode_wide, "reversible": encode_reversible}[a.format]
        if a.banded:
            base = FORMAT_VERSION[a.format]

            def encode_one(enc, part, width, height, f, lane_symbols):
                return encode_banded(enc, part, width, height, f, lane_symbols, base)
        for k, s0 in enumerate(starts):
            f = min(a.chunk, n_frames - s0)
            data = encode_one(enc, np.ascontiguousarray(rgb[s0 * frame_bytes:(s0 + f) * frame_bytes]), a.width, a.height, f,
                                a.lane_symbols)
            with open(f"{a.output}.{k:05d}.alc", "wb") as out:
                out.write(data)
            print(f"chunk {k}: frames {s0}..{s0 + f - 1} -> {len(data)} bytes", file=sys.stderr)
        return
    k = 0
    i = 0
    while i < len(starts):
        # whole chunks go through one call per group (their entropy chains run side by side); a short tail chunk alone
        group = [s0 for s0 in starts[i:i + a.in_flight] if n_frames - s0 >= a.chunk] or [starts[i]]
        f = min(a.chunk, n_frames - group[0])
        part = np.ascontiguousarray(rgb[group[0] * frame_bytes:(group[-1] + f) * frame_bytes])
        for start, chunk in zip(group, encode_many(enc, part, a.width, a.height, f)):
            data = chunk.to_bytes()
            with open(f"{a.output}.{k:05d}.alc", "wb") as out:
                out.write(data)
            print(f"chunk {k}: frames {start}..{start + f - 1} -> {len(data)} bytes", file=sys.stderr)
            k += 1
        i += len(group)


def _encode_chunks_to_rate(a, wt, rgb, frame_bytes, n_frames) -> None:
    """--kbps / --fps: every chunk gets floor(target_bits_per_frame * frames / 8) bytes (RateController's per-frame target),
    encoded by encode_to_size on --in-flight host threads, whose chains merge on the device.  --format split: chunk after
    chunk through encode_split_to_size (one chunk uses the whole device)."""
    from concurrent.futures import ThreadPoolExecutor
    starts = list(range(0, n_frames, a.chunk))

    def one(k):
        s0 = starts[k]
        f = min(a.chunk, n_frames - s0)
        budget = budget_bytes_per_chunk(a.kbps, a.fps, f)
        part = np.ascontiguousarray(rgb[s0 * frame_bytes:(s0 + f) * frame_bytes])
        if a.format == "split":
            data, q, fits = encode_split_to_size(part, a.width, a.height, f, budget, wt, a.min_quality, a.max_quality, a.lane_symbols)
        else:
            chunk, q, fits = encode_to_size(part, a.width, a.height, f, budget, wt, a.min_quality, a.max_quality)
            data = chunk.to_bytes()
        with open(f"{a.output}.{k:05d}.alc", "wb") as out:
            out.write(data)
        return s0, f, budget, q, fits, len(data)

    with ThreadPoolExecutor(max_workers=1 if a.format == "split" else max(1, a.in_flight)) as ex:
        for k, (s0, f, budget, q, fits, n) in enumerate(ex.map(one, range(len(starts)))):
            print(f"chunk {k}: frames {s0}..{s0 + f - 1} -> {n} bytes (budget {budget}), chosen quality: {q}", file=sys.stderr)
            if not fits:
                print(f"warning: chunk {k}: not even --min-quality {a.min_quality} is guaranteed to fit {budget} bytes",
                      file=sys.stderr)


def parse_frames(text: str):
    """'A' -> (A, A + 1), 'A:B' -> (A, B), half-open; ValueError otherwise."""
    parts = text.split(":")
    try:
        if len(parts) > 2 or not all(p.strip().isdigit() for p in parts):
            raise ValueError
        first = int(parts[0])
        end = int(parts[1]) if len(parts) == 2 else first + 1
        if end <= first or end > 0xFFFFFFFF:
            raise ValueError
    except ValueError:
        raise ValueError(f"--frames wants A or A:B with 0 <= A < B (half-open), got '{text}'") from None
    return first, end


def cmd_decode_frames(a) -> None:
    first, end = parse_frames(a.frames)
    data = np.memmap(a.input, dtype=np.uint8, mode="r")
    if a.format != "auto" and data.size > 4 and int(data[4]) != FORMAT_VERSION[a.format]:
        raise ValueError(f"--format {a.format} names version {FORMAT_VERSION[a.format]}, the file's version byte is {int(data[4])}")
    rgb = decode_frames(data, first, end - first)
    rgb.tofile(a.output)
    width, height, frames = (int(v) for v in np.frombuffer(bytes(data[6:18]), "<u4"))
    print(f"decoded frames [{first}, {end}) of {width}x{height}x{frames} -> {rgb.size} bytes (raw RGB)", file=sys.stderr)


def cmd_decode_preview(a) -> None:
    """--preview alone: every frame; with --frames A[:B]: that range.  Half resolution, from the low band alone."""
    data = np.memmap(a.input, dtype=np.uint8, mode="r")
    if a.format != "auto" and data.size > 4 and int(data[4]) != FORMAT_VERSION[a.format]:
        raise ValueError(f"--format {a.format} names version {FORMAT_VERSION[a.format]}, the file's version byte is {int(data[4])}")
    if data.size < 18:
        raise ValueError(f"{a.input}: too short for a container header")
    width, height, frames = (int(v) for v in np.frombuffer(bytes(data[6:18]), "<u4"))
    first, end = parse_frames(a.frames) if a.frames is not None else (0, frames)
    rgb = decode_preview(data, first, end - first)
    rgb.tofile(a.output)
    qw, qh = (width + 1) // 2, (height + 1) // 2
    print(f"decoded preview {qw}x{qh} of frames [{first}, {end}) of {width}x{height}x{frames} -> {rgb.size} bytes (raw RGB)", file=sys.stderr)


def cmd_thumbnails(a) -> None:
    """Preview frame K of every input (--frame K, default 0), or every N-th frame of every input (--every N), through the
    batched call in groups of at most PREVIEWS_MAX_ITEMS items, written back to back in input order."""
    if a.frame is not None and a.every is not None:
        raise ValueError("--frame and --every cannot be combined")
    if a.every is not None and a.every < 1:
        raise ValueError(f"--every wants N >= 1, got {a.every}")
    if a.frame is not None and a.frame < 0:
        raise ValueError(f"--frame wants K >= 0, got {a.frame}")
    files, items, size = [], [], None
    for path in a.inputs:
        data = np.memmap(path, dtype=np.uint8, mode="r")
        if data.size < 18 or bytes(data[:4]) != b"ALCC" or not 2 <= int(data[4]) <= 4:
            decode_previews([(data, 0, 1)])       # refused by the library, with its message (version 1: no random access)
            raise ValueError(f"{path}: not a version 2, 3 or 4 container")
        width, height, frames = (int(v) for v in np.frombuffer(bytes(data[6:18]), "<u4"))
        q = ((width + 1) // 2, (height + 1) // 2)
        if size is None:
            size, first_path = q, path
        elif q != size:
            raise ValueError(f"preview sizes differ: {first_path} gives {size[0]}x{size[1]}, {path} gives {q[0]}x{q[1]}")
        picks = range(0, frames, a.every) if a.every is not None else [a.frame or 0]
        for k in picks:
            if k >= frames:
                raise ValueError(f"{path}: frames [{k}, {k + 1}) are not a range of the chunk's {frames} frames")
            items.append((data, k, 1))
        files.append(data)
    written = 0
    try:
        with open(a.output, "wb") as out:
            for at in range(0, len(items), PREVIEWS_MAX_ITEMS):
                for rgb in decode_previews(items[at:at + PREVIEWS_MAX_ITEMS]):
                    rgb.tofile(out)
                    written += rgb.size
    except BaseException:
        import os
        if os.path.exists(a.output):
            os.remove(a.output)
        raise
    print(f"wrote {len(items)} preview frames {size[0]}x{size[1]} of {len(files)} files -> {written} bytes (raw RGB)", file=sys.stderr)


def parse_rect(text: str):
    """'X,Y,W,H' -> (X, Y, W, H); ValueError otherwise."""
    parts = text.split(",")
    try:
        if len(parts) != 4 or not all(p.strip().isdigit() for p in parts):
            raise ValueError
        x, y, w, h = (int(p) for p in parts)
        if w < 1 or h < 1 or max(x, y, w, h) > 0xFFFFFFFF:
            raise ValueError
    except ValueError:
        raise ValueError(f"--rect wants X,Y,W,H with W >= 1 and H >= 1, got '{text}'") from None
    return x, y, w, h


def cmd_extract(a) -> None:
    """Full-resolution frame K of every input (--frame K, default 0), or every N-th frame of every input (--every N): whole
    frames, or the rectangle of --rect, through the batched call in groups of at most RECTS_MAX_ITEMS items, written back to
    back in input order."""
    if a.frame is not None and a.every is not None:
        raise ValueError("--frame and --every cannot be combined")
    if a.every is not None and a.every < 1:
        raise ValueError(f"--every wants N >= 1, got {a.every}")
    if a.frame is not None and a.frame < 0:
        raise ValueError(f"--frame wants K >= 0, got {a.frame}")
    rect = parse_rect(a.rect) if a.rect is not None else None
    files, items, size = [], [], None
    for path in a.inputs:
        data = np.memmap(path, dtype=np.uint8, mode="r")
        if data.size < 18 or bytes(data[:4]) != b"ALCC" or not 2 <= int(data[4]) <= 4:
            decode_rects([(data, 0, 1)])          # refused by the library, with its message (version 1: no random access)
            raise ValueError(f"{path}: not a version 2, 3 or 4 container")
        width, height, frames = (int(v) for v in np.frombuffer(bytes(data[6:18]), "<u4"))
        if rect is not None and (rect[0] + rect[2] > width or rect[1] + rect[3] > height):
            raise ValueError(f"{path}: rectangle {rect[2]}x{rect[3]} at ({rect[0]}, {rect[1]}) does not lie inside the {width}x{height} frame")
        out_size = (rect[2], rect[3]) if rect is not None else (width, height)
        if size is None:
            size, first_path = out_size, path
        elif out_size != size:
            raise ValueError(f"output sizes differ: {first_path} gives {size[0]}x{size[1]}, {path} gives {out_size[0]}x{out_size[1]}")
        picks = range(0, frames, a.every) if a.every is not None else [a.frame or 0]
        for k in picks:
            if k >= frames:
                raise ValueError(f"{path}: frames [{k}, {k + 1}) are not a range of the chunk's {frames} frames")
            items.append((data, k, 1) if rect is None else (data, k, 1, *rect))
        files.append(data)
    written = 0
    try:
        with open(a.output, "wb") as out:
            for at in range(0, len(items), RECTS_MAX_ITEMS):
                for rgb in decode_rects(items[at:at + RECTS_MAX_ITEMS]):
                    rgb.tofile(out)
                    written += rgb.size
    except BaseException:
        import os
        if os.path.exists(a.output):
            os.remove(a.output)
        raise
    what = "frames" if rect is None else f"rectangles at ({rect[0]}, {rect[1]})"
    print(f"wrote {len(items)} {what} {size[0]}x{size[1]} of {len(files)} files -> {written} bytes (raw RGB)", file=sys.stderr)


def cmd_decode_rect(a) -> None:
    """--rect alone: the rectangle of every frame; with --frames A[:B]: of that range.  Packed W x H frames."""
    x, y, w, h = parse_rect(a.rect)
    data = np.memmap(a.input, dtype=np.uint8, mode="r")
    if a.format != "auto" and data.size > 4 and int(data[4]) != FORMAT_VERSION[a.format]:
        raise ValueError(f"--format {a.format} names version {FORMAT_VERSION[a.format]}, the file's version byte is {int(data[4])}")
    if data.size < 18:
        raise ValueError(f"{a.input}: too short for a container header")
    width, height, frames = (int(v) for v in np.frombuffer(bytes(data[6:18]), "<u4"))
    first, end = parse_frames(a.frames) if a.frames is not None else (0, frames)
    rgb = decode_rect(data, first, end - first, x, y, w, h)
    rgb.tofile(a.output)
    print(f"decoded rectangle {w}x{h} at ({x}, {y}) of frames [{first}, {end}) of {width}x{height}x{frames} -> {rgb.size} bytes (raw RGB)",
          file=sys.stderr)


def cmd_decode(a) -> None:
    if a.rect is not None:
        if a.preview:
            raise ValueError("--rect and --preview cannot be combined: there is no rectangle of a preview (decode the preview and crop it)")
        cmd_decode_rect(a)
        return
    if a.preview:
        cmd_decode_preview(a)
        return
    if a.frames is not None:
        cmd_decode_frames(a)
        return
    data = np.fromfile(a.input, dtype=np.uint8)
    version = _container_version(a, data)
    if version in CONTAINER_INFO:
        i = CONTAINER_INFO[version](data)
        rgb = CONTAINER_DECODE[version](data)
        rgb.tofile(a.output)
        print(f"decoded {i.width}x{i.height}x{i.frames} -> {rgb.size} bytes (raw RGB)", file=sys.stderr)
        return
    chunk = EncodedChunk.from_bytes(data)
    rgb = FrameDecoder().decode(chunk)
    rgb.tofile(a.output)
    print(f"decoded {chunk.width}x{chunk.height}x{chunk.frames} -> {rgb.size} bytes (raw RGB)", file=sys.stderr)


def cmd_transcode(a) -> None:
    """IN at --quality Q, or under --max-bytes N at the best quality in [--min-quality, --max-quality], from its symbols."""
    if (a.quality is None) == (a.max_bytes is None):
        raise ValueError("transcode wants exactly one of --quality Q and --max-bytes N")
    if a.max_bytes is not None and a.max_bytes < 0:
        raise ValueError(f"--max-bytes wants a byte count >= 0, got {a.max_bytes}")
    data = np.fromfile(a.input, dtype=np.uint8)
    if a.max_bytes is None:
        out = transcode(data, a.quality, a.lane_symbols, a.to_version)
        line = f"quality {a.quality}"
    else:
        out, quality, fits = transcode_to_size(data, a.max_bytes, a.min_quality, a.max_quality, a.lane_symbols, a.to_version)
        line = f"chosen quality: {quality}, budget {a.max_bytes} bytes {'met' if fits else 'NOT met'}"
    with open(a.output, "wb") as f:
        f.write(out)
    info = CONTAINER_INFO[out[4]](out)
    print(f"transcoded {data.size} -> {len(out)} bytes ({CONTAINER_NAME[out[4]]}, {line}, quantiser steps {list(info.quant_step)}, "
          f"lane_symbols {info.lane_symbols})", file=sys.stderr)


def cmd_repack(a) -> None:
    """IN as its version 5 twin (--banded) or a version 5 IN as its base version (--plain), from the symbols alone."""
    if a.banded == a.plain:
        raise ValueError("repack wants exactly one of --banded and --plain")
    data = np.fromfile(a.input, dtype=np.uint8)
    out = to_banded(data, a.lane_symbols) if a.banded else from_banded(data, a.lane_symbols)
    with open(a.output, "wb") as f:
        f.write(out)
    info = CONTAINER_INFO[out[4]](out)
    print(f"repacked {data.size} -> {len(out)} bytes ({CONTAINER_NAME[out[4]]}, lane_symbols {info.lane_symbols})", file=sys.stderr)


def cmd_info(a) -> None:
    data = np.fromfile(a.input, dtype=np.uint8)
    version = _container_version(a, data)
    if version in CONTAINER_INFO:
        i = CONTAINER_INFO[version](data)
        raw = i.width * i.height * i.frames * 3
        payload = sum(i.payload_len)
        print("ALICE-Codec Bitstream Info")
        print(f"  File:        {a.input}")
        print(f"  File size:   {data.size} bytes")
        print("  Format:      " + CONTAINER_NAME[version])
        print(f"  Width:       {i.width}")
        print(f"  Height:      {i.height}")
        print(f"  Frames:      {i.frames}")
        print(f"  Wavelet:     {WAVELET_NAMES[i.wavelet_type]}")
        print(f"  Lane length: {i.lane_symbols} symbols, {sum(i.n_blocks)} blocks")
        if version == 5:
            print(f"  Base:        version {i.base}")
            for c, name in enumerate(("Y", "Co", "Cg")):
                print(f"  Bands {name + ':':4s}   " + " ".join(str(v) for v in i.payload_len[8 * c:8 * c + 8]) + " bytes")
        print(f"  Payload:     {payload} bytes")
        print(f"  Raw size:    {raw} bytes (uncompressed RGB)")
        print(f"  Ratio:       {0.0 if raw == 0 else payload / raw * 100:.1f}%")
        return
    chunk = EncodedChunk.from_bytes(data)
    raw = chunk.width * chunk.height * chunk.frames * 3
    ratio = 0.0 if raw == 0 else chunk.compressed_size() / raw
    print("ALICE-Codec Bitstream Info")
    print(f"  File:        {a.input}")
    print(f"  File size:   {data.size} bytes")
    print(f"  Width:       {chunk.width}")
    print(f"  Height:      {chunk.height}")
    print(f"  Frames:      {chunk.frames}")
    print(f"  Wavelet:     {WAVELET_NAMES[chunk.wavelet_type]}")
    print(f"  Payload:     {chunk.compressed_size()} bytes")
    print(f"  Raw size:    {raw} bytes (uncompressed RGB)")
    print(f"  Ratio:       {ratio * 100:.1f}%")


def _u8(text: str) -> int:
    """clap parses `quality: u8` (src/bin/main.rs:44-46): 300 or -1 is a usage error, not quality 44 or 255."""
    v = int(text)
    if not 0 <= v <= 255:
        raise argparse.ArgumentTypeError(f"{text} is not in 0..255")
    return v


def main(argv=None) -> int:
    p = argparse.ArgumentParser(prog="alice-codec", description="ALICE-Codec: 3D wavelet video codec (MI355X path)")
    sub = p.add_subparsers(dest="command", required=True)
    for name in ("encode", "encode-chunks"):
        e = sub.add_parser(name)
        e.add_argument("input")
        e.add_argument("-o", "--output", required=True)
        e.add_argument("-W", "--width", type=int, required=True)
        e.add_argument("-H", "--height", type=int, required=True)
        if name == "encode":
            e.add_argument("-f", "--frames", type=int, default=1)
        else:
            e.add_argument("-c", "--chunk", type=int, default=DEFAULT_CHUNK_SIZE)
            e.add_argument("--in-flight", type=int, default=16, help="chunks encoded per call (GPU memory: about 2.4x the raw size of a chunk each)")
        e.add_argument("-q", "--quality", type=_u8, default=None, help="0..100 (default 90; 100 with --lossless)")
        e.add_argument("-w", "--wavelet", default="cdf53")
        if name == "encode":
            e.add_argument("--max-bytes", type=int, default=None, help="encode at the highest quality that fits this many bytes")
        else:
            e.add_argument("--kbps", type=int, default=None, help="target bitrate: a byte budget per chunk (with --fps)")
            e.add_argument("--fps", type=float, default=30.0)
        e.add_argument("--min-psnr", type=float, default=None, metavar="DB",
                       help="--format split / wide: the lowest quality in [--min-quality, --max-quality] whose measured PSNR is at least DB")
        e.add_argument("--format", choices=("v1", "split", "wide", "reversible"), default=None,
                       help="v1 (default): the reference's bitstream; split: .alc version 2; wide: .alc version 3 (untruncated symbols, for "
                            "the top qualities); reversible: .alc version 4 (version 3 with the mirrored inverse: lossless at quality 100)")
        e.add_argument("--lossless", action="store_true", help="short for --format reversible --quality 100")
        e.add_argument("--banded", action="store_true",
                       help="with --format split / wide / reversible or --lossless: .alc version 5 of that format (one frequency table per "
                            "wavelet subband; for chunks, not thumbnails)")
        e.add_argument("--lane-symbols", type=int, default=0,
                       help="--format split / wide / reversible: symbols per lane (power of two in 64..16384, wide and reversible: 64..8192; 0 = default)")
        e.add_argument("--min-quality", type=_u8, default=10)
        e.add_argument("--max-quality", type=_u8, default=95)
    d = sub.add_parser("decode")
    d.add_argument("input")
    d.add_argument("-o", "--output", required=True)
    d.add_argument("--frames", default=None, metavar="A[:B]",
                   help="write frames [A, B) only (A alone: one frame), decoded from the blocks they need; versions 2, 3 and 4")
    d.add_argument("--preview", action="store_true",
                   help="write half-resolution frames (ceil(W/2) x ceil(H/2)) decoded from the low band alone: all frames, or those of "
                        "--frames; versions 2, 3 and 4")
    d.add_argument("--rect", default=None, metavar="X,Y,W,H",
                   help="write the W x H pixels at (X, Y) only, as packed W x H frames decoded from the blocks they need: all frames, or "
                        "those of --frames; versions 2, 3 and 4; not with --preview")
    t = sub.add_parser("thumbnails", help="one call for many small previews: a contact sheet or a scrub bar")
    t.add_argument("inputs", nargs="+", metavar="IN", help="version 2, 3 or 4 containers, such as the PREFIX.NNNNN.alc files of encode-chunks")
    t.add_argument("-o", "--output", required=True)
    t.add_argument("--frame", type=int, default=None, metavar="K", help="preview frame K of every input (default 0)")
    t.add_argument("--every", type=int, default=None, metavar="N", help="every N-th frame of every input instead")
    x = sub.add_parser("extract", help="one call for many full-resolution frames or crops: frame K, or every N-th frame, of every input")
    x.add_argument("inputs", nargs="+", metavar="IN", help="version 2, 3 or 4 containers, such as the PREFIX.NNNNN.alc files of encode-chunks")
    x.add_argument("-o", "--output", required=True)
    x.add_argument("--rect", default=None, metavar="X,Y,W,H", help="the W x H pixels at (X, Y) of every picked frame instead of the whole frame")
    x.add_argument("--frame", type=int, default=None, metavar="K", help="frame K of every input (default 0)")
    x.add_argument("--every", type=int, default=None, metavar="N", help="every N-th frame of every input instead")
    tr = sub.add_parser("transcode", help="a version 2, 3 or 4 file at a lower quality or under a byte budget, from its symbols alone")
    tr.add_argument("input")
    tr.add_argument("-o", "--output", required=True)
    tr.add_argument("-q", "--quality", type=_u8, default=None, help="target quality 0..100; at or above the file's: its bytes come back")
    tr.add_argument("--max-bytes", type=int, default=None, help="instead of --quality: the highest quality that fits this many bytes")
    tr.add_argument("--min-quality", type=_u8, default=10)
    tr.add_argument("--max-quality", type=_u8, default=95)
    tr.add_argument("--lane-symbols", type=int, default=0, help="lane the chunk again (power of two in the version's range; 0 = keep)")
    tr.add_argument("--to-version", type=_u8, default=0, metavar="V", help="3 or 4 for a version 3 or 4 file (0 = keep)")
    rp = sub.add_parser("repack", help="a version 2, 3 or 4 file as its banded (version 5) twin, or back, from its symbols alone")
    rp.add_argument("input")
    rp.add_argument("-o", "--output", required=True)
    rp.add_argument("--banded", action="store_true", help="version 2, 3 or 4 -> version 5 of that base")
    rp.add_argument("--plain", action="store_true", help="version 5 -> its base version, byte for byte")
    rp.add_argument("--lane-symbols", type=int, default=0, help="lane the chunk again (power of two in the base's range; 0 = keep)")
    i = sub.add_parser("info")
    i.add_argument("input")
    for x in (d, i):
        x.add_argument("--format", choices=("auto", "v1", "split", "wide", "reversible"), default="auto",
                       help="auto: from the file's version byte; otherwise the file must be of that format")
    a = p.parse_args(argv)
    try:
        {"encode": cmd_encode, "encode-chunks": cmd_encode_chunks, "decode": cmd_decode, "info": cmd_info,
         "thumbnails": cmd_thumbnails, "extract": cmd_extract, "transcode": cmd_transcode, "repack": cmd_repack}[a.command](a)
    except (CodecError, ValueError, OSError) as e:
        print(f"error: {e}", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
