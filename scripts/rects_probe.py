"""Times many frame ranges and rectangles in one call (alice_codec_dev_decode_rects) against a loop of
the existing single calls (alice_codec_dev_decode_rect, alice_codec_dev_decode_frames), alternating in one run.

Device-resident 1920x1080x64 chunks of the benchmark's content (bench.py, synth_chunk, one seed per chunk), CDF 9/7, lane
length 512; even chunks are version 2 at q = 80, odd chunks version 3 at q = 95.  Rows:
  * one 256x256 crop of frame 31 of N = 1, 8, 32 distinct chunks;
  * the whole frame 31 of N = 1, 8, 32 distinct chunks;
  * 16 crops of one chunk at 16 different frames;
  * a 4x4 mosaic: sixteen 480x270 crops of frame 31 of 16 chunks pasted into one 1920x1080 surface.
Every alternative sits between HIP events (each call ends in its own synchronise), the alternatives of a row rotate inside
every repetition; 2 warm-up rounds, `--reps` timed ones (6 by default); median, minimum, maximum.  Every batched result is
compared, in this run, with the bytes the single calls wrote.

  python scripts/rects_probe.py --out profiles/r24_rects_probe_1080p64.json

Kernel-only times, from kernel traces in runs of their own (ten rounds of one kind after the encodes, no counters):

  rocprofv3 --kernel-trace --stats --output-format csv -d DIR/batched_32 -- python scripts/rects_probe.py --trace-run batched
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR/loop_32 -- python scripts/rects_probe.py --trace-run loop
  python scripts/rects_probe.py --trace-parse DIR --out profiles/r24_rects_kernel_trace.json
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import alice_codec_amd as a  # noqa: E402
from frames_probe import F, H, W  # noqa: E402
from previews_probe import CONTAINERS, ENCODE_KERNELS, FRAME, N_CHUNKS, ROWS_N, TRACE_ROUNDS, encode_chunks, timed_row  # noqa: E402

CROP = (832, 412, 256, 256)                 # x, y, w, h: the middle of the frame
TILE = (480, 270)                           # the mosaic's crops: 4 x 4 of them fill 1920 x 1080
TRACE_KERNELS = ("rans_tables_from_arrays_kernel", "rans_table_from_arrays_kernel", "split_scan_kernel", "split_box_decode_kernel",
                 "split_frames_decode_kernel", "inv_t_win_many_kernel", "inv_t_wide_win_many_kernel", "inv_xy_many_kernel",
                 "rgb_rect_paste_many_kernel", "inv_t_win_kernel", "inv_t_wide_win_kernel", "inv_xy_kernel", "rgb_rect_paste_kernel")


def crop_items(chunks, d_out, n):
    x, y, w, h = CROP
    return [(c.data_ptr(), m, FRAME, 1, x, y, w, h, d_out.data_ptr() + i * w * h * 3, 0, 0) for i, (c, m) in enumerate(chunks[:n])]


def single(it):
    alc, m, first, count, x, y, w, h, out, rp, fp = it
    if w == 0:
        a.frames_decode_device(alc, m, first, count, out)
    else:
        a.rect_decode_device(alc, m, first, count, x, y, w, h, out, rp, fp)


def trace_run(what):
    """the encodes, then TRACE_ROUNDS rounds of the 32-crop row, batched or as the loop: what a kernel trace sees"""
    a.set_device(0)
    dev = torch.device("cuda", 0)
    chunks = encode_chunks(dev, N_CHUNKS)
    d_out = torch.empty(N_CHUNKS * CROP[2] * CROP[3] * 3, dtype=torch.uint8, device=dev)
    items = crop_items(chunks, d_out, N_CHUNKS)
    for _ in range(TRACE_ROUNDS):
        if what == "batched":
            a.rects_decode_device(items)
        else:
            for it in items:
                single(it)
    torch.cuda.synchronize()
    print(f"{what}: {TRACE_ROUNDS} rounds of {N_CHUNKS} crops")
    return 0


def trace_parse(trace_dir, out):
    """DIR/<run>/**/*_kernel_trace.csv -> per run and kernel: launches, total, average, minimum and maximum microseconds"""
    import csv
    import glob
    res = {"what": f"rocprofv3 --kernel-trace --stats, a run of its own per entry and no counters, {TRACE_ROUNDS} rounds after the "
                   f"encodes: one {CROP[2]}x{CROP[3]} crop of frame {FRAME} of {N_CHUNKS} distinct 1920x1080x64 CDF 9/7 chunks (lane "
                   "length 512, versions 2 and 3 alternating) through one batched call per round (batched_32) and through a loop of "
                   "single calls per round (loop_32); kernel time per launch in microseconds, and per round in total",
           "runs": {}}
    for run in sorted(os.listdir(trace_dir)):
        rows = {}
        for path in sorted(glob.glob(os.path.join(trace_dir, run, "**", "*_kernel_trace.csv"), recursive=True)):
            trace = list(csv.DictReader(open(path)))
            # the encodes build tables and scan too: only what starts after the last encode kernel is a round's
            encoded = max([int(r["End_Timestamp"]) for r in trace if any(k in r["Kernel_Name"] for k in ENCODE_KERNELS)], default=0)
            for r in trace:
                key = next((k for k in TRACE_KERNELS if k in r["Kernel_Name"]), None)
                if key and int(r["Start_Timestamp"]) > encoded:
                    rows.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        if rows:
            res["runs"][run] = {k: {"launches": len(v), "launches_per_round": round(len(v) / TRACE_ROUNDS, 1),
                                    "total_us_per_round": round(sum(v) / TRACE_ROUNDS, 1), "average_us": round(sum(v) / len(v), 1),
                                    "min_us": round(min(v), 1), "max_us": round(max(v), 1)} for k, v in rows.items()}
            res["runs"][run]["kernel_us_per_round"] = round(sum(sum(v) for v in rows.values()) / TRACE_ROUNDS, 1)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res["runs"]))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-run", choices=("batched", "loop"), default=None)
    ap.add_argument("--trace-parse", metavar="DIR", default=None)
    args = ap.parse_args()
    if args.trace_run:
        return trace_run(args.trace_run)
    if args.trace_parse:
        return trace_parse(args.trace_parse, args.out)
    a.set_device(0)
    dev = torch.device("cuda", 0)
    chunks = encode_chunks(dev, N_CHUNKS)
    fb = W * H * 3
    d_batched = torch.empty(N_CHUNKS * fb, dtype=torch.uint8, device=dev)
    d_single = torch.empty(N_CHUNKS * fb, dtype=torch.uint8, device=dev)
    res = {"device": torch.cuda.get_device_name(0), "chunk": [W, H, F], "crop": list(CROP), "mosaic_tile": list(TILE), "wavelet": "cdf97",
           "lane_symbols": 512,
           "containers": {f"chunk {i} mod 2 = {i}": {"format": name, "quality": q} for i, (name, q) in enumerate(CONTAINERS)},
           "container_bytes": [n for _, n in chunks], "reps": args.reps, "warmup": args.warmup,
           "timing": "HIP events around each alternative (a batched call; a loop of single calls); the alternatives of a row rotate inside "
                     "every repetition",
           "stats_columns": ["items", "distinct containers", "table launches", "lane launches", "batched finish launches",
                             "items finished through the per-item path", "stream drains", "blocks decoded", "payload bytes uploaded",
                             "symbols stored", "frames written"],
           "rows": {}}
    ok = True

    def row(name, make_items, n_bytes):
        """make_items(output tensor) -> the items; n_bytes: what they cover of it"""
        nonlocal ok
        items_batched, items_single = make_items(d_batched), make_items(d_single)
        alternatives = {
            "batched": lambda: a.rects_decode_device(items_batched),
            "loop_of_single_calls": lambda: [single(it) for it in items_single],
        }
        r = timed_row(alternatives, args.warmup, args.reps)
        d_batched[:n_bytes].zero_()
        d_single[:n_bytes].zero_()
        alternatives["batched"]()
        stats = a._test_last_rects_stats()
        alternatives["loop_of_single_calls"]()
        torch.cuda.synchronize()
        same = bool(torch.equal(d_batched[:n_bytes], d_single[:n_bytes])) and bool(d_batched[:n_bytes].any())
        ok = ok and same
        b, lp = r["batched"], r["loop_of_single_calls"]
        loop_spread = lp["max_ms"] - lp["min_ms"]
        r.update(items=len(items_batched), batched_equals_single_calls=same, stats=list(stats),
                 batched_over_loop=round(b["median_ms"] / lp["median_ms"], 4), loop_spread_ms=round(loop_spread, 4),
                 batched_faster_than_loop_by_more_than_its_spread=bool(lp["median_ms"] - b["median_ms"] > loop_spread),
                 batched_not_slower_than_loop_by_more_than_its_spread=bool(b["median_ms"] - lp["median_ms"] <= loop_spread))
        res["rows"][name] = r
        print(f"{name}: batched {b['median_ms']:.3f} ms [{b['min_ms']:.3f}, {b['max_ms']:.3f}], loop {lp['median_ms']:.3f} ms "
              f"[{lp['min_ms']:.3f}, {lp['max_ms']:.3f}], ratio {r['batched_over_loop']:.3f}; stats {stats}; "
              f"{'equal' if same else 'DIFFERENT'} bytes", flush=True)
        return r

    x, y, cw, ch = CROP
    for n in ROWS_N:
        row(f"{n} distinct chunks, one {cw}x{ch} crop of frame {FRAME} of each", lambda d, n=n: crop_items(chunks, d, n), n * cw * ch * 3)
    for n in ROWS_N:
        row(f"{n} distinct chunks, the whole frame {FRAME} of each",
            lambda d, n=n: [(c.data_ptr(), m, FRAME, 1, 0, 0, 0, 0, d.data_ptr() + i * fb, 0, 0) for i, (c, m) in enumerate(chunks[:n])], n * fb)
    for ci in (0, 1):
        c, m = chunks[ci]
        row(f"16 {cw}x{ch} crops of chunk {ci} ({CONTAINERS[ci][0]}) at frames 0, 4, .., 60",
            lambda d: [(c.data_ptr(), m, 4 * k, 1, x, y, cw, ch, d.data_ptr() + k * cw * ch * 3, 0, 0) for k in range(16)], 16 * cw * ch * 3)
    tw, th = TILE
    row(f"4x4 mosaic: sixteen {tw}x{th} crops of frame {FRAME} of 16 chunks pasted into one {W}x{H} surface",
        lambda d: [(chunks[k][0].data_ptr(), chunks[k][1], FRAME, 1, (k % 4) * tw, (k // 4) * th, tw, th,
                    d.data_ptr() + ((k // 4) * th * W + (k % 4) * tw) * 3, 3 * W, fb) for k in range(16)], fb)
    res["all_batched_results_equal_the_single_calls"] = ok
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
