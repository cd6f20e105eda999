"""Times frame-range decodes (alice_codec_dev_decode_frames / alice_codec_decode_frames) against the
full decode of the same chunk, in one run.

One 1920x1080x64 chunk of the benchmark's content (bench.py, synth_chunk: moving sinusoids plus integer noise), CDF 9/7,
lane length 512, in three containers: version 2 at q = 80, version 3 at q = 95 and version 4 at q = 100.  For each:
  full        the device-resident decode of the whole chunk (split / wide / reversible_decode_device)
  [31, 32)    one middle frame        [0, 1)   the first frame
  [24, 40)    sixteen frames          [0, 64)  every frame through the window instances (what they cost when nothing is skipped)
Device-resident calls are timed between HIP events around one call (each call ends in its own verdict synchronise), after
warm-up, `--reps` times: the median, the minimum and the maximum are reported.  The two host calls (decode_split / _wide /
_reversible and decode_frames for [31, 32)) are timed by the wall clock.  Every range is compared with the full decode's
frames, and the planned blocks and uploaded bytes of each call are reported from alice_codec_test_last_frames_stats.

  python scripts/frames_probe.py --out profiles/r16_frames_probe_1080p64.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import alice_codec_amd as a  # noqa: E402

W, H, F = 1920, 1080, 64
LANE = 512
RANGES = [(31, 32), (0, 1), (24, 40), (0, 64)]
CONTAINERS = [("v2", 80), ("v3", 95), ("v4", 100)]


def synth_chunk(dev, w, h, f, idx=0):
    """bench.py's synth_chunk at a shape of the caller's choice."""
    g = torch.Generator(device=dev)
    g.manual_seed(1234 + idx)
    t = torch.arange(f, device=dev, dtype=torch.float32).view(f, 1, 1, 1)
    y = torch.arange(h, device=dev, dtype=torch.float32).view(1, h, 1, 1)
    x = torch.arange(w, device=dev, dtype=torch.float32).view(1, 1, w, 1)
    s = torch.tensor([23.0, 31.0, 17.0], device=dev).view(1, 1, 1, 3)
    ph = torch.tensor([0.0, 1.0, 2.0], device=dev).view(1, 1, 1, 3)
    base = 128 + 90 * torch.sin((x + 2 * t + 5 * idx) / s + ph) * torch.cos((y - t) / (0.7 * s))
    noise = torch.randint(-4, 5, (f, h, w, 3), device=dev, generator=g)
    return (base + noise).round().clamp(0, 255).to(torch.uint8)


def spread(samples):
    return {"median_ms": round(statistics.median(samples), 4), "min_ms": round(min(samples), 4), "max_ms": round(max(samples), 4),
            "samples_ms": [round(s, 4) for s in samples]}


def device_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return spread(out)


def wall_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return spread(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=W)
    ap.add_argument("--height", type=int, default=H)
    ap.add_argument("--frames", type=int, default=F)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    w, h, f = args.width, args.height, args.frames
    a.set_device(0)
    dev = torch.device("cuda", 0)
    wt = a.WaveletType.Cdf97
    rgb = synth_chunk(dev, w, h, f).contiguous()
    fb = w * h * 3
    pw, ph, pf = w + (w & 1), h + (h & 1), 2 if f == 1 else f + (f & 1)
    stride = (a.SPLIT_HEADER_BYTES + 3 * a.wide_stream_bound(pw * ph * pf, LANE) + 255) & ~255
    d_alc = torch.empty(stride, dtype=torch.uint8, device=dev)
    d_full = torch.empty(f * fb, dtype=torch.uint8, device=dev)
    d_part = torch.empty(f * fb, dtype=torch.uint8, device=dev)
    ranges = [(min(t0, f - 1), min(t1, f)) for t0, t1 in RANGES] if f != F else RANGES
    res = {"device": torch.cuda.get_device_name(0), "chunk": [w, h, f], "wavelet": "cdf97", "lane_symbols": LANE, "reps": args.reps,
           "warmup": args.warmup, "timing": "HIP events around one call (device-resident); wall clock (host calls)", "containers": {}}
    enc = {"v2": a.split_encode_device, "v3": a.wide_encode_device, "v4": a.reversible_encode_device}
    dec = {"v2": a.split_decode_device, "v3": a.wide_decode_device, "v4": a.reversible_decode_device}
    host_dec = {"v2": a.decode_split, "v3": a.decode_wide, "v4": a.decode_reversible}
    for name, q in CONTAINERS:
        sizes = enc[name](rgb.data_ptr(), w, h, f, 1, wt, q, d_alc.data_ptr(), stride, lane_symbols=LANE)
        n = int(sizes[0])
        out = {"quality": q, "container_bytes": n, "n_blocks_per_channel": -(-(pw * ph * pf) // (64 * LANE))}
        out["full_dev_decode"] = device_ms(lambda: dec[name](d_alc.data_ptr(), stride, sizes, d_full.data_ptr()), args.warmup, args.reps)
        full_ms = out["full_dev_decode"]["median_ms"]
        out["ranges"] = {}
        for t0, t1 in ranges:
            d_part.zero_()
            r = device_ms(lambda: a.frames_decode_device(d_alc.data_ptr(), n, t0, t1 - t0, d_part.data_ptr()), args.warmup, args.reps)
            st = a._test_last_frames_stats()
            r.update(window=[st[0], st[1]], blocks_decoded=st[2], blocks_of_chunk=3 * out["n_blocks_per_channel"], frames_spatial=st[4],
                     equals_full_decode=bool(torch.equal(d_part[:(t1 - t0) * fb], d_full[t0 * fb:t1 * fb])),
                     share_of_full=round(r["median_ms"] / full_ms, 4))
            out["ranges"][f"[{t0}, {t1})"] = r
        blob = d_alc[:n].cpu().numpy()
        t0, t1 = ranges[0]
        out["host_full_decode"] = wall_ms(lambda: host_dec[name](blob), 1, args.reps)
        hr = wall_ms(lambda: a.decode_frames(blob, t0, t1 - t0), 1, args.reps)
        st = a._test_last_frames_stats()
        hr.update(range=[t0, t1], uploaded_payload_bytes=st[3], blocks_decoded=st[2], downloaded_bytes=(t1 - t0) * fb,
                  equals_full_decode=bool(np.array_equal(np.asarray(a.decode_frames(blob, t0, t1 - t0)), d_full[t0 * fb:t1 * fb].cpu().numpy())))
        out["host_decode_frames"] = hr
        res["containers"][name] = out
        line = ", ".join(f"{k} {v['median_ms']:.3f} ms ({v['share_of_full']:.2f}x)" for k, v in out["ranges"].items())
        print(f"{name} q={q}: full {full_ms:.3f} ms; {line}; host full {out['host_full_decode']['median_ms']:.1f} ms, host "
              f"[{t0}, {t1}) {hr['median_ms']:.1f} ms ({hr['uploaded_payload_bytes']} payload bytes up)", flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    ok = all(r["equals_full_decode"] for c in res["containers"].values() for r in list(c["ranges"].values()) + [c["host_decode_frames"]])
    print("all ranges equal the full decode" if ok else "MISMATCH")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
