"""Times the half-resolution preview (alice_codec_dev_decode_preview) against the frame-range decode of
the same range and the full decode of the same chunk, alternating in one run.

One 1920x1080x64 chunk of the benchmark's content (bench.py, synth_chunk), CDF 9/7, lane length 512, in three containers:
version 2 at q = 80, version 3 at q = 95 and version 4 at q = 100.  For each range -- [31, 32), [24, 40), [0, 64) -- every
repetition times the preview, dev_decode_frames of the same range and the full device decode, each between HIP events around
one call (each call ends in its own synchronise), in an order that rotates from one repetition to the next (what ran before
a call decides what it finds in the cache); 2 warm-up rounds, `--reps` timed ones (6 by default: two of each order); median,
minimum, maximum.
Every preview is compared, in this run, with tests/preview_ref.py on a crop of 64 x 128 quadrant pixels: the numpy oracle's
forward transform of the 144 x 264 full-resolution pixels the crop's low-low coefficients depend on (a margin of 8 pixels
keeps the crop's own boundary extension out of them), quantised as the encoder quantises, through the contract.

  python scripts/preview_probe.py --out profiles/r17_preview_probe_1080p64.json

Kernel-only times, from kernel traces in runs of their own (ten calls of one kind after the encode):

  rocprofv3 --kernel-trace --stats --output-format csv -d DIR/v3_preview -- python scripts/preview_probe.py --trace-run v3 preview
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR/v3_frames -- python scripts/preview_probe.py --trace-run v3 frames
  python scripts/preview_probe.py --trace-parse DIR --out profiles/r17_preview_kernel_trace.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import alice_codec_amd as a  # noqa: E402
import oracle.alice_oracle_np as o  # noqa: E402
import preview_ref as PR  # noqa: E402
import wide_ref as R3  # noqa: E402
from frames_probe import CONTAINERS, F, H, LANE, W, spread, synth_chunk  # noqa: E402

RANGES = [(31, 32), (24, 40), (0, 64)]
CROP_X0, CROP_W, CROP_H, MARGIN = 400, 64, 128, 8      # quadrant pixels [0, 128) x [400, 464)


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def crop_coefficients(rgb, w, h, f, kind):
    """[Y, Co, Cg] low-low coefficients (pf, CROP_H, CROP_W) of the crop, unquantised, from the numpy oracle's forward"""
    c0, c1 = 2 * CROP_X0 - MARGIN, 2 * (CROP_X0 + CROP_W) + MARGIN
    r1 = 2 * CROP_H + MARGIN
    assert c0 >= 0 and c1 <= w and r1 <= h and c0 % 2 == 0
    part = np.ascontiguousarray(rgb.reshape(f, h, w, 3)[:, :r1, c0:c1])
    cw, ch = c1 - c0, r1
    out = []
    for chan in o.rgb_to_ycocg_r(part.reshape(-1)):
        v, pw, ph, pf = o._pad(chan, cw, ch, f)
        coef = np.asarray(o.wavelet3d(kind, v, pw, ph, pf)).reshape(pf, ph, pw)
        out.append(coef[:, :CROP_H, MARGIN // 2:MARGIN // 2 + CROP_W].copy())
    return out


def crop_reference(coefs, f, kind, step, version, t0, t1):
    """preview_ref.preview of a volume whose low-low quadrant is the crop's symbols"""
    pf = coefs[0].shape[0]
    dims = (2 * CROP_W, 2 * CROP_H, pf)
    syms = []
    for c in coefs:
        q = np.asarray(o.quantize(c, step, step), np.int64)
        vol = np.zeros((pf, 2 * CROP_H, 2 * CROP_W), np.uint8 if version == 2 else np.uint16)
        vol[:, :CROP_H, :CROP_W] = o.to_symbols(q) if version == 2 else R3.wide_symbols(q).reshape(q.shape)
        syms.append(vol.reshape(-1))
    return PR.preview(syms, dims, f, kind, (step,) * 3, version, t0, t1).reshape(t1 - t0, CROP_H, CROP_W, 3)


TRACE_RANGE = (31, 32)
TRACE_CALLS = 10
TRACE_KERNELS = ("rans_table_from_arrays_kernel", "split_scan_kernel", "split_box_decode_kernel", "split_frames_decode_kernel",
                 "preview_inv_kernel", "inv_t_win_kernel", "inv_t_wide_win_kernel", "inv_xy_kernel")


def trace_run(name, what):
    """the encode, then TRACE_CALLS calls of the preview or of the frame-range decode of TRACE_RANGE: what a kernel trace sees"""
    w, h, f = W, H, F
    a.set_device(0)
    dev = torch.device("cuda", 0)
    rgb = synth_chunk(dev, w, h, f).contiguous()
    stride = (a.SPLIT_HEADER_BYTES + 3 * a.wide_stream_bound(w * h * f, LANE) + 255) & ~255
    d_alc = torch.empty(stride, dtype=torch.uint8, device=dev)
    d_out = torch.empty(w * h * 3, dtype=torch.uint8, device=dev)
    enc = {"v2": a.split_encode_device, "v3": a.wide_encode_device, "v4": a.reversible_encode_device}[name]
    n = int(enc(rgb.data_ptr(), w, h, f, 1, a.WaveletType.Cdf97, dict(CONTAINERS)[name], d_alc.data_ptr(), stride, lane_symbols=LANE)[0])
    call = a.preview_decode_device if what == "preview" else a.frames_decode_device
    t0, t1 = TRACE_RANGE
    for _ in range(TRACE_CALLS):
        call(d_alc.data_ptr(), n, t0, t1 - t0, d_out.data_ptr())
    torch.cuda.synchronize()
    print(f"{name} {what}: {TRACE_CALLS} calls of [{t0}, {t1})")
    return 0


def trace_parse(trace_dir, out):
    """DIR/<run>/**/*_kernel_trace.csv -> per run and kernel: launches, average, minimum and maximum microseconds"""
    import csv
    import glob
    res = {"what": f"rocprofv3 --kernel-trace --stats, a run of its own per entry, {TRACE_CALLS} calls after the encode: the preview "
                   f"against alice_codec_dev_decode_frames for frames [{TRACE_RANGE[0]}, {TRACE_RANGE[1]}) of one 1920x1080x64 CDF 9/7 "
                   "chunk at lane length 512; kernel time per launch in microseconds", "runs": {}}
    for run in sorted(os.listdir(trace_dir)):
        rows = {}
        for path in sorted(glob.glob(os.path.join(trace_dir, run, "**", "*_kernel_trace.csv"), recursive=True)):
            for r in csv.DictReader(open(path)):
                key = next((k for k in TRACE_KERNELS if k in r["Kernel_Name"]), None)
                if key:
                    rows.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        if rows:
            res["runs"][run] = {k: {"calls": len(v), "average_us": round(sum(v) / len(v), 1), "min_us": round(min(v), 1),
                                    "max_us": round(max(v), 1)} for k, v in rows.items()}
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res["runs"]))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-run", nargs=2, metavar=("CONTAINER", "KIND"), default=None, help="v2 | v3 | v4 and preview | frames")
    ap.add_argument("--trace-parse", metavar="DIR", default=None)
    args = ap.parse_args()
    if args.trace_run:
        return trace_run(*args.trace_run)
    if args.trace_parse:
        return trace_parse(args.trace_parse, args.out)
    w, h, f = W, H, F
    a.set_device(0)
    dev = torch.device("cuda", 0)
    wt = a.WaveletType.Cdf97
    rgb = synth_chunk(dev, w, h, f).contiguous()
    fb = w * h * 3
    qw, qh = a.preview_dims(w, h)
    qb = qw * qh * 3
    n_sym = w * h * f
    stride = (a.SPLIT_HEADER_BYTES + 3 * a.wide_stream_bound(n_sym, LANE) + 255) & ~255
    d_alc = torch.empty(stride, dtype=torch.uint8, device=dev)
    d_full = torch.empty(f * fb, dtype=torch.uint8, device=dev)
    d_part = torch.empty(f * fb, dtype=torch.uint8, device=dev)
    d_prev = torch.empty(f * qb, dtype=torch.uint8, device=dev)
    coefs = crop_coefficients(rgb.cpu().numpy(), w, h, f, int(wt))
    res = {"device": torch.cuda.get_device_name(0), "chunk": [w, h, f], "preview": [qw, qh], "wavelet": "cdf97", "lane_symbols": LANE,
           "reps": args.reps, "warmup": args.warmup,
           "timing": "HIP events around one call; preview, frame range and full decode alternate inside every repetition, in rotating order",
           "crop": {"quadrant_rows": [0, CROP_H], "quadrant_columns": [CROP_X0, CROP_X0 + CROP_W]}, "containers": {}}
    enc = {"v2": a.split_encode_device, "v3": a.wide_encode_device, "v4": a.reversible_encode_device}
    dec = {"v2": a.split_decode_device, "v3": a.wide_decode_device, "v4": a.reversible_decode_device}
    ok = True
    for name, q in CONTAINERS:
        version = int(name[1])
        sizes = enc[name](rgb.data_ptr(), w, h, f, 1, wt, q, d_alc.data_ptr(), stride, lane_symbols=LANE)
        n = int(sizes[0])
        step = o.quality_to_step(q)
        out = {"quality": q, "step": step, "container_bytes": n, "n_blocks_per_channel": -(-n_sym // (64 * LANE)), "ranges": {}}
        for t0, t1 in RANGES:
            calls = {
                "preview": lambda: a.preview_decode_device(d_alc.data_ptr(), n, t0, t1 - t0, d_prev.data_ptr()),
                "frames": lambda: a.frames_decode_device(d_alc.data_ptr(), n, t0, t1 - t0, d_part.data_ptr()),
                "full": lambda: dec[name](d_alc.data_ptr(), stride, sizes, d_full.data_ptr()),
            }
            samples = {k: [] for k in calls}
            order = list(calls)
            for rep in range(args.warmup + args.reps):
                for k in order[rep % 3:] + order[:rep % 3]:      # every call follows each of the other two in turn
                    ms = event_ms(calls[k])
                    if rep >= args.warmup:
                        samples[k].append(ms)
            calls["preview"]()
            st = a._test_last_preview_stats()
            calls["frames"]()
            fst = a._test_last_frames_stats()
            got = d_prev[:(t1 - t0) * qb].cpu().numpy().reshape(t1 - t0, qh, qw, 3)[:, :CROP_H, CROP_X0:CROP_X0 + CROP_W]
            same = bool(np.array_equal(got, crop_reference(coefs, f, int(wt), step, version, t0, t1)))
            ok = ok and same
            r = {k: spread(v) for k, v in samples.items()}
            r.update(window=[st[0], st[1]], preview_blocks_decoded=st[2], frames_blocks_decoded=fst[2],
                     blocks_of_chunk=3 * out["n_blocks_per_channel"], symbols_stored=st[5], crop_equals_preview_ref=same,
                     preview_over_frames=round(r["preview"]["median_ms"] / r["frames"]["median_ms"], 4),
                     preview_over_full=round(r["preview"]["median_ms"] / r["full"]["median_ms"], 4))
            out["ranges"][f"[{t0}, {t1})"] = r
            print(f"{name} q={q} [{t0}, {t1}): preview {r['preview']['median_ms']:.3f} ms, frames {r['frames']['median_ms']:.3f} ms, "
                  f"full {r['full']['median_ms']:.3f} ms; blocks {st[2]} / {fst[2]} / {3 * out['n_blocks_per_channel']}; "
                  f"crop {'equals' if same else 'DIFFERS FROM'} preview_ref", flush=True)
        res["containers"][name] = out
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    print("every preview crop equals preview_ref" if ok else "MISMATCH")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
