"""Rate prediction on 1920x1080x64 chunks (CDF 9/7, the benchmark's synthetic content): what it costs and how tight it is.

* prediction ms per chunk: HIP events around alice_codec_dev_predict_sizes on a batch of chunks after warm-up (the call
  returns after its work has drained, so this includes its host side and its one small device-to-host copy), next to
  the forward transform pair of an encode (alice_codec_test_transform_ms);
* the relative bracket width (hi - lo) / hi at q = 50, 80, 95;
* the bracket against the actual .alc lengths of GPU encodes at those qualities;
* encode_to_size of one chunk for a few budgets: chosen quality, size, budget.

  python scripts/rate_probe.py --out profiles/r06_rate_probe_1080p64.json

--format split: the same for the split-stream container (.alc version 2) at --lane-symbols: the v2
prediction timed next to the v1 prediction in the same run (they differ by the cost kernel only), the bracket against
encode_split at q = 50 / 80 / 95, and encode_split_to_size at the three budgets with its refinement trials and wall time.

  python scripts/rate_probe.py --format split --out profiles/r08_split_rate_probe_1080p64.json

--format wide: the same for the wide container (.alc version 3): the v3 prediction timed next to the v2
prediction in the same run (they differ by the fold and the cost kernel only), the bracket against encode_wide at
q = 90 / 95 / 100, and encode_wide_to_size at those three sizes with its refinement trials and wall time.

  python scripts/rate_probe.py --format wide --chunks 1 --out profiles/r11_wide_rate_probe_1080p64.json
"""
import argparse
import ctypes as C
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


def _timed_prediction(call, reps, chunks):
    call()   # warm-up
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        p = call()
    t1.record()
    torch.cuda.synchronize()
    return p, t0.elapsed_time(t1) / (reps * chunks)


def split_probe(args, lib, rgb, wt):
    L = args.lane_symbols
    n = args.chunks
    _, v1_ms = _timed_prediction(lambda: a.predict_sizes_device(rgb.data_ptr(), W, H, F, n, wt), args.reps, n)
    p, v2_ms = _timed_prediction(lambda: a.predict_split_sizes_device(rgb.data_ptr(), W, H, F, n, wt, L), args.reps, n)
    _, v1_ms_again = _timed_prediction(lambda: a.predict_sizes_device(rgb.data_ptr(), W, H, F, n, wt), args.reps, n)
    host = rgb[0].cpu().numpy()
    actual = {}
    for q in (50, 80, 95):
        size = len(a.encode_split(a.FrameEncoder.with_wavelet(q, wt), host, W, H, F, L))
        lo, hi = int(p.lo[0][q]), int(p.hi[0][q])
        actual[q] = {"lo": lo, "actual": size, "hi": hi, "rel_width": (hi - lo) / hi, "inside": lo <= size <= hi}
    trials = np.zeros(1, np.uint32)
    rows = []
    for budget in (actual[50]["hi"] // 2, actual[80]["hi"], actual[95]["hi"] + 1, actual[80]["actual"]):
        a.encode_split_to_size(host, W, H, F, budget, wt, 10, 95, L)   # warm-up of the pool for this size
        t = time.perf_counter()
        data, q, fits = a.encode_split_to_size(host, W, H, F, budget, wt, 10, 95, L)
        ms = (time.perf_counter() - t) * 1e3
        lib.alice_codec_test_last_split_trials(trials.ctypes.data_as(C.POINTER(C.c_uint32)), 1)
        rows.append({"budget": budget, "chosen_quality": q, "fits": fits, "bytes": len(data), "trials": int(trials[0]),
                     "host_call_ms": round(ms, 2)})
    res = {
        "what": "version 2 rate prediction of 1920x1080x64 CDF 9/7 chunks (bench.synth_chunk content), MI355X",
        "lane_symbols": L,
        "predict_ms_per_chunk": {"v2": round(v2_ms, 3), "v1_before": round(v1_ms, 3), "v1_after": round(v1_ms_again, 3)},
        "chunks_per_call": n, "reps": args.reps,
        "bracket_vs_actual": {str(k): v for k, v in actual.items()},
        "encode_split_to_size": rows,
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


def wide_probe(args, lib, rgb, wt):
    L = args.lane_symbols
    n = args.chunks
    _, v2_ms = _timed_prediction(lambda: a.predict_split_sizes_device(rgb.data_ptr(), W, H, F, n, wt, L), args.reps, n)
    p, v3_ms = _timed_prediction(lambda: a.predict_wide_sizes_device(rgb.data_ptr(), W, H, F, n, wt, L), args.reps, n)
    _, v2_ms_again = _timed_prediction(lambda: a.predict_split_sizes_device(rgb.data_ptr(), W, H, F, n, wt, L), args.reps, n)
    host = rgb[0].cpu().numpy()
    actual = {}
    for q in (90, 95, 100):
        size = len(a.encode_wide(a.FrameEncoder.with_wavelet(q, wt), host, W, H, F, L))
        lo, hi = int(p.lo[0][q]), int(p.hi[0][q])
        actual[q] = {"lo": lo, "actual": size, "hi": hi, "rel_width": (hi - lo) / hi, "inside": lo <= size <= hi}
    trials = np.zeros(1, np.uint32)
    rows = []
    for q in (90, 95, 100):
        budget = actual[q]["actual"]
        a.encode_wide_to_size(host, W, H, F, budget, wt, 10, 100, L)   # warm-up of the pool for this size
        t = time.perf_counter()
        data, cq, fits = a.encode_wide_to_size(host, W, H, F, budget, wt, 10, 100, L)
        ms = (time.perf_counter() - t) * 1e3
        lib.alice_codec_test_last_split_trials(trials.ctypes.data_as(C.POINTER(C.c_uint32)), 1)
        rows.append({"budget": budget, "budget_is_the_size_at_quality": q, "chosen_quality": cq, "fits": fits, "bytes": len(data),
                     "trials": int(trials[0]), "host_call_ms": round(ms, 2)})
    res = {
        "what": "version 3 rate prediction of 1920x1080x64 CDF 9/7 chunks (bench.synth_chunk content), MI355X",
        "lane_symbols": L,
        "predict_ms_per_chunk": {"v3": round(v3_ms, 3), "v2_before": round(v2_ms, 3), "v2_after": round(v2_ms_again, 3)},
        "chunks_per_call": n, "reps": args.reps,
        "bracket_vs_actual": {str(k): v for k, v in actual.items()},
        "encode_wide_to_size": rows,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r06_rate_probe_1080p64.json"))
    ap.add_argument("--chunks", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--predict-only", action="store_true", help="time the prediction only (replica sweeps of the bin layout)")
    ap.add_argument("--format", choices=("v1", "split", "wide"), default="v1")
    ap.add_argument("--lane-symbols", type=int, default=512)
    args = ap.parse_args()
    a.set_device(0)
    lib = a.load_library()
    dev = torch.device("cuda:0")
    px = W * H * F
    rgb = torch.stack([bench.synth_chunk(dev, i).reshape(-1) for i in range(args.chunks)]).contiguous()
    wt = a.WaveletType.Cdf97
    if args.format == "split":
        return split_probe(args, lib, rgb, wt)
    if args.format == "wide":
        return wide_probe(args, lib, rgb, wt)
    a.predict_sizes_device(rgb.data_ptr(), W, H, F, args.chunks, wt)   # warm-up
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(args.reps):
        p = a.predict_sizes_device(rgb.data_ptr(), W, H, F, args.chunks, wt)
    t1.record()
    torch.cuda.synchronize()
    predict_ms = t0.elapsed_time(t1) / (args.reps * args.chunks)
    if args.predict_only:
        print(json.dumps({"predict_ms_per_chunk": round(predict_ms, 3), "chunks_per_call": args.chunks, "reps": args.reps}))
        return

    sym = torch.empty((args.chunks, 3 * px), dtype=torch.uint8, device=dev)
    out = torch.empty_like(rgb)
    ms = (C.c_float * 2)()
    st = torch.cuda.current_stream().cuda_stream
    assert lib.alice_codec_test_transform_ms(rgb.data_ptr(), sym.data_ptr(), out.data_ptr(), args.chunks, W, H, F, int(wt), 80,
                                             args.chunks, args.reps, 0, ms, st) == 0
    forward_ms = float(ms[0])

    host = rgb[0].cpu().numpy()
    actual = {}
    for q in (50, 80, 95):
        n = len(a.FrameEncoder.with_wavelet(q, wt).encode(host, W, H, F).to_bytes())
        actual[q] = {"lo": int(p.lo[0][q]), "actual": n, "hi": int(p.hi[0][q]), "status": int(p.status[0][q]),
                     "rel_width": (int(p.hi[0][q]) - int(p.lo[0][q])) / int(p.hi[0][q]),
                     "inside": int(p.lo[0][q]) <= n <= int(p.hi[0][q])}
    budget_rows = []
    for budget in (actual[50]["hi"] // 2, actual[80]["hi"], actual[95]["hi"] + 1):
        chunk, q, fits = a.encode_to_size(host, W, H, F, budget, wt, 10, 95)
        budget_rows.append({"budget": budget, "chosen_quality": q, "fits": fits, "bytes": len(chunk.to_bytes())})
    res = {
        "what": "rate prediction of 1920x1080x64 CDF 9/7 chunks (bench.synth_chunk content), MI355X",
        "predict_ms_per_chunk": round(predict_ms, 3),
        "forward_transform_pair_ms_per_chunk": round(forward_ms, 3),
        "chunks_per_call": args.chunks, "reps": args.reps,
        "bracket_vs_actual": {str(k): v for k, v in actual.items()},
        "status_counts": {s: int((p.status == i).sum()) for i, s in enumerate(("bounded", "unbounded", "diverges"))},
        "encode_to_size": budget_rows,
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
