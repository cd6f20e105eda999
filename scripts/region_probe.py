"""Times region encode / decode (Batch.encode_regions / decode_regions) on 1920x1080 frames against the alternatives.

One 640x720 region of 64 frames per chunk, N chunks (default 32), Cdf53 q=90, the same synthetic frames for every route:
  region      Batch.encode_regions + encode_finish, Batch.decode_regions (into full frames) + decode_finish: the transforms
              read / write the rectangles of the full frames in place.  Per-stage device times (stage_ms) and the wall time
              of encode + finish and decode + finish between HIP events after warm-up.
  contiguous  the same crops, already in a packed device buffer of their own (made beforehand, not timed), through
              Batch.encode / decode: the device-resident path without regions.
  host        what the hybrid flow did before: frames to the host, crop_to_bbox per frame, FrameEncoder.encode (host
              memory), FrameDecoder.decode, paste_from_bbox per frame.  Timed on --host-chunks chunks (default 2) and
              scaled per chunk.
The .alc of every route is compared with the others (all must be byte-identical).

  python scripts/region_probe.py --out profiles/r05_region_probe_1080p64.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import alice_codec_amd as a  # noqa: E402

W, H, F = 1920, 1080, 64
RW, RH = 640, 720
Q = 90


def alcs_of(bt, sizes):
    packed = torch.empty(int(sizes.sum()), dtype=torch.uint8, device="cuda")
    bt.pack_alc(sizes, packed.data_ptr(), packed.numel())
    torch.cuda.synchronize()
    host = packed.cpu().numpy()
    ends = np.cumsum(sizes.astype(np.int64))
    return [host[e - int(s):e].tobytes() for e, s in zip(ends, sizes)]


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-chunks", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = args.chunks
    a.set_device(0)
    dev = torch.device("cuda", 0)
    # smooth moving gradients plus noise: compressible like camera frames, different in every chunk (made chunk by chunk)
    frames = torch.empty((n * F, H, W, 3), dtype=torch.uint8, device=dev)
    y = torch.arange(H, device=dev, dtype=torch.int32)[None, :, None]
    x = torch.arange(W, device=dev, dtype=torch.int32)[None, None, :]
    g = torch.Generator(device=dev).manual_seed(5)
    for i in range(n):
        t = torch.arange(i * F, (i + 1) * F, device=dev, dtype=torch.int32)[:, None, None]
        base = (x // 3 + y // 2 + t * 3) % 256
        rgb = torch.stack([base, 255 - base, (base * 5) % 256], dim=3)
        rgb += torch.randint(-6, 7, rgb.shape, device=dev, dtype=torch.int32, generator=g)
        frames[i * F:(i + 1) * F] = rgb.clamp_(0, 255).to(torch.uint8)
    del rgb, base
    origins = [((64 * i) % (W - RW) // 4 * 4 + (i % 4), (16 * i) % (H - RH)) for i in range(n)]   # all four x0 % 4
    crops = torch.stack([frames[i * F:(i + 1) * F, y0:y0 + RH, x0:x0 + RW] for i, (x0, y0) in enumerate(origins)]).contiguous()
    out_frames = torch.zeros_like(frames)
    out_crops = torch.empty_like(crops)
    px = n * F * RW * RH
    res = {"device": torch.cuda.get_device_name(0), "frame": [W, H], "region": [RW, RH], "frames_per_chunk": F, "chunks": n,
           "quality": Q, "wavelet": "cdf53", "origins": origins, "reps": args.reps, "warmup": args.warmup}

    # region route
    bt = a.Batch(RW, RH, F, n, Q)
    enc = lambda: (bt.encode_regions(frames.data_ptr(), W, H, origins), bt.encode_finish())  # noqa: E731
    for _ in range(args.warmup):
        enc()
    enc_ms = timed(enc, args.reps)
    stage_enc = bt.stage_ms()
    sizes = bt.encode_finish()
    region_alc = alcs_of(bt, sizes)
    dec = lambda: (bt.decode_regions(bt.alc_ptr(0), bt.alc_stride, out_frames.data_ptr(), W, H, origins), bt.decode_finish())  # noqa: E731
    for _ in range(args.warmup):
        dec()
    dec_ms = timed(dec, args.reps)
    stage_dec = bt.stage_ms()
    res["region"] = {"encode_ms": round(enc_ms, 2), "decode_ms": round(dec_ms, 2), "mpix_s_encode_plus_decode": round(px / ((enc_ms + dec_ms) * 1e3), 1),
                     "stage_ms": {"forward_transform": round(stage_enc["forward_transform"], 3), "rans_encode": round(stage_enc["rans_encode"], 3),
                                  "rans_decode": round(stage_dec["rans_decode"], 3), "inverse_transform": round(stage_dec["inverse_transform"], 3)},
                     "alc_bytes": int(sizes.sum())}
    print(json.dumps({"region": res["region"]}), flush=True)
    del bt

    # contiguous route: the same crops from a packed buffer
    bt = a.Batch(RW, RH, F, n, Q)
    enc = lambda: (bt.encode(crops.data_ptr()), bt.encode_finish())  # noqa: E731
    for _ in range(args.warmup):
        enc()
    enc_ms = timed(enc, args.reps)
    stage_enc = bt.stage_ms()
    contiguous_alc = alcs_of(bt, bt.encode_finish())
    dec = lambda: (bt.decode(bt.alc_ptr(0), bt.alc_stride, out_crops.data_ptr()), bt.decode_finish())  # noqa: E731
    for _ in range(args.warmup):
        dec()
    dec_ms = timed(dec, args.reps)
    stage_dec = bt.stage_ms()
    res["contiguous"] = {"encode_ms": round(enc_ms, 2), "decode_ms": round(dec_ms, 2), "mpix_s_encode_plus_decode": round(px / ((enc_ms + dec_ms) * 1e3), 1),
                         "stage_ms": {"forward_transform": round(stage_enc["forward_transform"], 3), "rans_encode": round(stage_enc["rans_encode"], 3),
                                      "rans_decode": round(stage_dec["rans_decode"], 3), "inverse_transform": round(stage_dec["inverse_transform"], 3)}}
    print(json.dumps({"contiguous": res["contiguous"]}), flush=True)
    del bt
    same_alc = region_alc == contiguous_alc
    oc = out_crops.cpu().numpy()
    of = out_frames.cpu().numpy()
    same_pixels = all(np.array_equal(of[i * F:(i + 1) * F, y0:y0 + RH, x0:x0 + RW], oc[i]) for i, (x0, y0) in enumerate(origins))

    # host route on a few chunks
    k = min(args.host_chunks, n)
    fe, fd = a.FrameEncoder(Q), a.FrameDecoder()
    bg = np.zeros((F, H, W, 3), np.uint8)
    t_d2h = t_crop = t_enc = t_dec = t_paste = 0.0
    host_alc = []
    for i in range(k):
        x0, y0 = origins[i]
        bbox = [x0 * 3, y0, RW * 3, RH]
        s = time.perf_counter()
        host = frames[i * F:(i + 1) * F].cpu().numpy()
        t_d2h += time.perf_counter() - s
        s = time.perf_counter()
        crop = np.frombuffer(b"".join(a.crop_to_bbox(host[f].reshape(-1), W * 3, bbox) for f in range(F)), np.uint8)
        t_crop += time.perf_counter() - s
        s = time.perf_counter()
        chunk = fe.encode(crop, RW, RH, F)
        t_enc += time.perf_counter() - s
        host_alc.append(chunk.to_bytes())
        s = time.perf_counter()
        decd = fd.decode(chunk)
        t_dec += time.perf_counter() - s
        s = time.perf_counter()
        per = RW * RH * 3
        for f in range(F):
            a.paste_from_bbox(bg[f], W * 3, decd[f * per:(f + 1) * per], bbox)
        t_paste += time.perf_counter() - s
    per_chunk = {"d2h_frames": t_d2h / k, "crop_to_bbox": t_crop / k, "frame_encoder_encode": t_enc / k,
                 "frame_decoder_decode": t_dec / k, "paste_from_bbox": t_paste / k}
    tot = sum(per_chunk.values())
    res["host"] = {"chunks_timed": k, "ms_per_chunk": {kk: round(v * 1e3, 1) for kk, v in per_chunk.items()},
                   "ms_per_chunk_total": round(tot * 1e3, 1), "ms_for_all_chunks_scaled": round(tot * 1e3 * n, 1),
                   "mpix_s_encode_plus_decode": round(F * RW * RH / (tot * 1e6), 1)}
    res["all_routes_byte_identical"] = bool(same_alc and host_alc == region_alc[:k] and same_pixels)
    print(json.dumps({"host": res["host"], "all_routes_byte_identical": res["all_routes_byte_identical"]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    if not res["all_routes_byte_identical"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
