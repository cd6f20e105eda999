"""Times the rectangle decode (alice_codec_dev_decode_rect) against the frame-range decode of the same
frames and the full decode of the chunk, in one run.

One 1920x1080x64 chunk of the benchmark's content (bench.py, synth_chunk), CDF 9/7, lane length 512, in three containers:
version 2 at q = 80, version 3 at q = 95 and version 4 at q = 100 (the chunk of sections 14.6 and 15.7).  Rectangles: 256 x 256
at the centre, the top strip of 1920 x 270, the column of 640 x 1080 at x = 640, and the whole frame; frame ranges [31, 32),
[24, 40) and [0, 64).  Every repetition times the rectangle call, dev_decode_frames of the same range and the full device
decode, each between HIP events around one call (each call ends in its own verdict synchronise), in rotating order, so that
no call always runs behind the same other one.  The median, the minimum and the maximum are reported with the planned blocks
and stored symbols of alice_codec_test_last_rect_stats / _last_frames_stats.  Every rectangle is compared, in this run, with
the crop of the full decode.

  python scripts/rect_probe.py --out profiles/r19_rect_probe_1080p64.json
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import alice_codec_amd as a  # noqa: E402
from frames_probe import spread, synth_chunk  # noqa: E402

W, H, F = 1920, 1080, 64
LANE = 512
RECTS = [("256x256 centre", (832, 412, 256, 256)), ("1920x270 top strip", (0, 0, 1920, 270)), ("640x1080 column", (640, 0, 640, 1080)),
         ("whole frame", (0, 0, 1920, 1080))]
RANGES = [(31, 32), (24, 40), (0, 64)]
CONTAINERS = [("v2", 80), ("v3", 95), ("v4", 100)]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    w, h, f = W, H, F
    a.set_device(0)
    dev = torch.device("cuda", 0)
    wt = a.WaveletType.Cdf97
    rgb = synth_chunk(dev, w, h, f).contiguous()
    fb = w * h * 3
    stride = (a.SPLIT_HEADER_BYTES + 3 * a.wide_stream_bound(w * h * f, LANE) + 255) & ~255
    d_alc = torch.empty(stride, dtype=torch.uint8, device=dev)
    d_full = torch.empty(f * fb, dtype=torch.uint8, device=dev)
    d_frames = torch.empty(f * fb, dtype=torch.uint8, device=dev)
    d_rect = torch.empty(f * fb, dtype=torch.uint8, device=dev)
    res = {"device": torch.cuda.get_device_name(0), "chunk": [w, h, f], "wavelet": "cdf97", "lane_symbols": LANE, "reps": args.reps,
           "warmup": args.warmup,
           "timing": "HIP events around one call; rectangle, frame range and full decode alternate inside every repetition, in rotating order",
           "containers": {}}
    enc = {"v2": a.split_encode_device, "v3": a.wide_encode_device, "v4": a.reversible_encode_device}
    dec = {"v2": a.split_decode_device, "v3": a.wide_decode_device, "v4": a.reversible_decode_device}
    ok = True
    for name, q in CONTAINERS:
        sizes = enc[name](rgb.data_ptr(), w, h, f, 1, wt, q, d_alc.data_ptr(), stride, lane_symbols=LANE)
        n = int(sizes[0])
        out = {"quality": q, "container_bytes": n, "n_blocks_per_channel": -(-(w * h * f) // (64 * LANE)), "cases": {}}
        dec[name](d_alc.data_ptr(), stride, sizes, d_full.data_ptr())
        full4 = d_full.view(f, h, w, 3)
        for t0, t1 in RANGES:
            for label, (x, y, rw, rh) in RECTS:
                calls = {
                    "rect": lambda: a.rect_decode_device(d_alc.data_ptr(), n, t0, t1 - t0, x, y, rw, rh, d_rect.data_ptr()),
                    "frames": lambda: a.frames_decode_device(d_alc.data_ptr(), n, t0, t1 - t0, d_frames.data_ptr()),
                    "full": lambda: dec[name](d_alc.data_ptr(), stride, sizes, d_full.data_ptr()),
                }
                order = list(calls)
                for _ in range(args.warmup):
                    for k in order:
                        calls[k]()
                samples = {k: [] for k in order}
                for rep in range(args.reps):
                    for k in order[rep % 3:] + order[:rep % 3]:
                        samples[k].append(timed(calls[k]))
                r = {k: spread(v) for k, v in samples.items()}
                calls["frames"]()
                fst = a._test_last_frames_stats()
                d_rect.zero_()
                calls["rect"]()
                st = a._test_last_rect_stats()
                got = d_rect[:(t1 - t0) * rh * rw * 3].view(t1 - t0, rh, rw, 3)
                same = bool(torch.equal(got, full4[t0:t1, y:y + rh, x:x + rw]))
                ok = ok and same
                r.update(windows={"t": [st[0], st[1]], "x": [st[2], st[3]], "y": [st[4], st[5]]}, rect_blocks_decoded=st[6],
                         frames_blocks_decoded=fst[2], blocks_of_chunk=3 * out["n_blocks_per_channel"], symbols_stored=st[9],
                         equals_crop_of_full_decode=same,
                         rect_over_frames=round(r["rect"]["median_ms"] / r["frames"]["median_ms"], 4),
                         rect_over_full=round(r["rect"]["median_ms"] / r["full"]["median_ms"], 4))
                out["cases"][f"[{t0}, {t1}) {label}"] = r
                print(f"{name} q={q} [{t0}, {t1}) {label}: rect {r['rect']['median_ms']:.3f} ms ({st[6]} blocks), frames "
                      f"{r['frames']['median_ms']:.3f} ms ({fst[2]} blocks), full {r['full']['median_ms']:.3f} ms; "
                      f"{'equals' if same else 'DIFFERS FROM'} the crop", flush=True)
        res["containers"][name] = out
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    print("every rectangle equals the crop of the full decode" if ok else "MISMATCH")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
