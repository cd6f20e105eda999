"""Times the device segmentation calls (alice_codec_dev_segment_motion / _chroma_rgb) on 1920x1080x64 frames.

For each config: radius 2/1 (the default) and 300/300, one shared reference or one per frame, with and without the u8 mask
output.  Wall time per call comes from HIP events around synchronised calls after warm-up (each call returns after its
work has drained, so this includes the host side of the call).  Kernel times come from a separate
`rocprofv3 --kernel-trace --stats` run of this script with --config NAME.  Achieved bandwidth uses byte counts from the
shapes: the current frames (1 B/px), per-frame references (1 B/px, a shared one stays in cache) and the mask (1 B/px).

  python scripts/segment_probe.py --out profiles/segment_probe.json
  rocprofv3 --kernel-trace --stats -d DIR -o seg -- python scripts/segment_probe.py --config r2_shared_mask --reps 20
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import alice_codec_amd as a  # noqa: E402

W, H, N = 1920, 1080, 64
COPY_TBPS = 6.29   # MI355X_MICROARCH.md: float4 copy, measured


def configs():
    for rd, re in ((2, 1), (300, 300)):
        for shared in (True, False):
            for mask in (True, False):
                yield f"r{rd}_{'shared' if shared else 'perframe'}_{'mask' if mask else 'stats'}", rd, re, shared, mask


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    a.set_device(0)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    ref = torch.randint(0, 256, (N, H, W), dtype=torch.uint8, device=dev, generator=g)
    cur = ref.clone()
    cur[:, 300:800, 700:1200] ^= 0x80          # a moving region, about 12% of each frame
    for f in range(N):
        cur[f, 300:800, 700 + 4 * f:1200 + 4 * f] ^= 0x40
    mask = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
    stats = torch.empty(N * 5, dtype=torch.int32, device=dev)
    rows = []
    for name, rd, re, shared, with_mask in configs():
        if args.config and name != args.config:
            continue
        cfg = a.SegmentConfig(25, 100, rd, re)

        def call():
            a.segment_motion_device(cur.data_ptr(), ref.data_ptr(), 0 if shared else W * H, W, H, N, stats.data_ptr(),
                                    mask.data_ptr() if with_mask else None, cfg)

        for _ in range(args.warmup):
            call()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            call()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1000.0 / args.reps
        px = W * H * N
        nbytes = px * (1 + (0 if shared else 1) + (1 if with_mask else 0))
        rows.append({"config": name, "dilate_radius": rd, "erode_radius": re, "shared_reference": shared, "mask_output": with_mask,
                     "frames": N, "width": W, "height": H, "us_per_call_wall": round(us, 2), "bytes_from_shapes": nbytes,
                     "floor_us_at_copy_rate": round(nbytes / (COPY_TBPS * 1e12) * 1e6, 2),
                     "achieved_TBps_wall": round(nbytes / (us * 1e-6) / 1e12, 3)})
        print(json.dumps(rows[-1]), flush=True)
    # chroma from RGB, default radii
    if not args.config or args.config == "chroma_rgb_mask":
        rgb = torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, device=dev, generator=g)
        for _ in range(args.warmup):
            a.segment_chroma_rgb_device(rgb.data_ptr(), W, H, N, 30, stats.data_ptr(), mask.data_ptr())
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            a.segment_chroma_rgb_device(rgb.data_ptr(), W, H, N, 30, stats.data_ptr(), mask.data_ptr())
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1000.0 / args.reps
        nbytes = W * H * N * 4
        rows.append({"config": "chroma_rgb_mask", "us_per_call_wall": round(us, 2), "bytes_from_shapes": nbytes,
                     "floor_us_at_copy_rate": round(nbytes / (COPY_TBPS * 1e12) * 1e6, 2),
                     "achieved_TBps_wall": round(nbytes / (us * 1e-6) / 1e12, 3)})
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
