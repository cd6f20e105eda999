"""The split-stream format (.alc v2) on 1920x1080x64 CDF 9/7 chunks of the benchmark's content, next to v1 on the same chunk.

* device-resident v2 encode / decode of one chunk and of --many chunks in one call: HIP events around the calls (they
  return after their work has drained, so the host side and the one size read-back are inside); every chunk of the
  many-chunk call is compared, bytes and pixels, with the one-chunk route;
* the same chunk through v1: a Batch of one chunk (HIP events) and the host calls (wall);
* the v2 host calls (wall);
* lane length sweep: time and size per lane_symbols;
* v2 bytes against v1 bytes at q = 50, 80, 95.

  python scripts/split_probe.py --out profiles/r07_split_probe_1080p64.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import alice_codec_amd as a  # noqa: E402
import bench  # noqa: E402

W, H, F = 1920, 1080, 64
PX = W * H * F


def events(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_split_probe_1080p64.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--many", type=int, default=32)
    ap.add_argument("--quick", action="store_true", help="v2 device calls at the default lane length only (for a kernel trace)")
    args = ap.parse_args()
    a.set_device(0)
    dev = torch.device("cuda:0")
    wt = a.WaveletType.Cdf97
    rgb = bench.synth_chunk(dev, 0).reshape(-1).contiguous()
    back = torch.empty_like(rgb)
    cap = a.SPLIT_HEADER_BYTES + 3 * a.split_stream_bound(PX, 64)
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    res = {"what": "split-stream .alc v2 against v1, 1920x1080x64 CDF 9/7 (bench.synth_chunk content), MI355X", "reps": args.reps}

    def v2(q, L, n=1, src=rgb, dst=out, stride=cap, bk=back):
        size = [None]

        def enc():
            size[0] = a.split_encode_device(src.data_ptr(), W, H, F, n, wt, q, dst.data_ptr(), stride, lane_symbols=L)

        e = events(enc, args.reps)
        d = events(lambda: a.split_decode_device(dst.data_ptr(), stride, size[0], bk.data_ptr()), args.reps)
        return e, d, size[0]

    def many_chunks(n):
        many = torch.stack([bench.synth_chunk(dev, i).reshape(-1) for i in range(n)]).contiguous()
        stride = (a.SPLIT_HEADER_BYTES + 3 * a.split_stream_bound(PX, a.SPLIT_DEFAULT_LANE_SYMBOLS) + 255) // 256 * 256
        mout = torch.empty(n * stride, dtype=torch.uint8, device=dev)
        mback = torch.empty_like(many)
        e, d, sizes = v2(80, 0, n, many, mout, stride, mback)
        # every chunk of the many-chunk call against the one-chunk route: the same bytes, the same pixels
        for i in range(n):
            s1 = a.split_encode_device(many[i].data_ptr(), W, H, F, 1, wt, 80, out.data_ptr(), cap)
            a.split_decode_device(out.data_ptr(), cap, s1, back.data_ptr())
            assert int(s1[0]) == int(sizes[i]), (i, s1, sizes[i])
            assert torch.equal(out[:int(s1[0])], mout[i * stride:i * stride + int(s1[0])]), i
            assert torch.equal(back, mback[i]), i
        return {"chunks": n, "every_chunk_equals_the_one_chunk_route": True, "encode_ms_per_chunk": round(e / n, 3), "decode_ms_per_chunk": round(d / n, 3),
                "encode_mpix_s": round(n * PX / e / 1e3, 1), "decode_mpix_s": round(n * PX / d / 1e3, 1)}

    e, d, size = v2(80, 0)
    res["v2_device_one_chunk_q80"] = {"lane_symbols": a.SPLIT_DEFAULT_LANE_SYMBOLS, "encode_ms": round(e, 3), "decode_ms": round(d, 3),
                                      "bytes": int(size[0]), "encode_mpix_s": round(PX / e / 1e3, 1), "decode_mpix_s": round(PX / d / 1e3, 1)}
    if args.quick:
        if args.many > 1:
            res["v2_device_many_chunks_q80"] = many_chunks(args.many)
        print(json.dumps(res))
        return
    sweep = []
    for L in (256, 512, 1024, 2048, 4096):
        e, d, size = v2(80, L)
        lanes = 3 * ((PX + 64 * L - 1) // (64 * L)) * 64
        sweep.append({"lane_symbols": L, "encode_ms": round(e, 3), "decode_ms": round(d, 3), "bytes": int(size[0]),
                      "lane_overhead_bytes": lanes * 6 + lanes // 64 * 4})
    res["lane_sweep_q80"] = sweep

    host = rgb.cpu().numpy()
    sizes = {}
    v1_chunk = None
    for q in (50, 80, 95):
        _, _, s2 = v2(q, 0)
        t = time.perf_counter()
        chunk = a.FrameEncoder.with_wavelet(q, wt).encode(host, W, H, F)
        t_enc = time.perf_counter() - t
        n1 = len(chunk.to_bytes())
        sizes[str(q)] = {"v2_bytes": int(s2[0]), "v1_bytes": n1, "v2_over_v1": round(int(s2[0]) / n1, 5)}
        if q == 80:
            v1_chunk = chunk
            t = time.perf_counter()
            dec1 = a.FrameDecoder().decode(chunk)
            t_dec = time.perf_counter() - t
            res["v1_host_one_chunk_q80"] = {"encode_s": round(t_enc, 3), "decode_s": round(t_dec, 3),
                                            "psnr_db": round(a.psnr(dec1, host), 2)}
    res["bytes_v2_vs_v1"] = sizes

    enc = a.FrameEncoder.with_wavelet(80, wt)
    a.encode_split(enc, host, W, H, F)
    t = time.perf_counter()
    b2 = a.encode_split(enc, host, W, H, F)
    t_enc = time.perf_counter() - t
    t = time.perf_counter()
    dec2 = a.decode_split(b2)
    t_dec = time.perf_counter() - t
    res["v2_host_one_chunk_q80"] = {"encode_s": round(t_enc, 3), "decode_s": round(t_dec, 3), "psnr_db": round(a.psnr(dec2, host), 2),
                                    "encode_mpix_s": round(PX / t_enc / 1e6, 1), "decode_mpix_s": round(PX / t_dec / 1e6, 1)}

    batch = a.Batch(W, H, F, 1, 80, wt)

    def v1_enc():
        batch.encode(rgb.data_ptr())
        return batch.encode_finish()

    e1 = events(v1_enc, 2)

    def v1_dec():
        batch.decode(batch.alc_ptr(0), batch.alc_stride, back.data_ptr())
        batch.decode_finish()

    d1 = events(v1_dec, 2)
    res["v1_device_batch_of_one_q80"] = {"encode_ms": round(e1, 1), "decode_ms": round(d1, 1)}
    del batch

    res["v2_device_many_chunks_q80"] = many_chunks(args.many)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
