"""Times many previews in one call (alice_codec_dev_decode_previews) against a loop of the existing
single calls (alice_codec_dev_decode_preview), alternating in one run.

Device-resident 1920x1080x64 chunks of the benchmark's content (bench.py, synth_chunk, one seed per chunk), CDF 9/7, lane
length 512; even chunks are version 2 at q = 80, odd chunks version 3 at q = 95.  Rows:
  * N = 1, 8, 32 one-frame previews [31, 32) of N distinct chunks: the batched call against a loop of N single calls;
  * 64 one-frame previews of one chunk: the batched call against the loop of 64 single calls and against the single
    preview of [0, 64).
Every alternative sits between HIP events (each call ends in its own synchronise), the alternatives of a row rotate inside
every repetition; 2 warm-up rounds, `--reps` timed ones (6 by default); median, minimum, maximum.  Every batched result is
compared, in this run, with the bytes the single calls wrote.

  python scripts/previews_probe.py --out profiles/r22_previews_probe_1080p64.json

Kernel-only times, from kernel traces in runs of their own (ten rounds of one kind after the encodes, no counters):

  rocprofv3 --kernel-trace --stats --output-format csv -d DIR/batched_32 -- python scripts/previews_probe.py --trace-run batched
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR/loop_32 -- python scripts/previews_probe.py --trace-run loop
  python scripts/previews_probe.py --trace-parse DIR --out profiles/r22_previews_kernel_trace.json
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
from frames_probe import F, H, LANE, W, spread, synth_chunk  # noqa: E402

N_CHUNKS = 32
ROWS_N = (1, 8, 32)
FRAME = 31
CONTAINERS = (("v2", 80), ("v3", 95))       # chunk i is CONTAINERS[i % 2]
TRACE_ROUNDS = 10
TRACE_KERNELS = ("rans_tables_from_arrays_kernel", "rans_table_from_arrays_kernel", "split_scan_kernel", "split_box_decode_kernel",
                 "preview_inv_many_kernel", "preview_inv_kernel")
ENCODE_KERNELS = ("encode_kernel", "split_header_kernel", "split_version_kernel", "fwd_")


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def encode_chunks(dev, n_chunks):
    """-> [(device tensor holding exactly the container, its length)], chunk i of synth_chunk(idx = i)"""
    enc = {"v2": a.split_encode_device, "v3": a.wide_encode_device}
    stride = (a.SPLIT_HEADER_BYTES + 3 * a.wide_stream_bound(W * H * F, LANE) + 255) & ~255
    d_alc = torch.empty(stride, dtype=torch.uint8, device=dev)
    out = []
    for i in range(n_chunks):
        name, q = CONTAINERS[i % 2]
        rgb = synth_chunk(dev, W, H, F, idx=i).contiguous()
        n = int(enc[name](rgb.data_ptr(), W, H, F, 1, a.WaveletType.Cdf97, q, d_alc.data_ptr(), stride, lane_symbols=LANE)[0])
        out.append((d_alc[:n].clone(), n))
        del rgb
    return out


def timed_row(alternatives, warmup, reps):
    """{name: spread} of the alternatives, rotating their order from one repetition to the next"""
    samples = {k: [] for k in alternatives}
    order = list(alternatives)
    for rep in range(warmup + reps):
        r = rep % len(order)
        for k in order[r:] + order[:r]:
            ms = event_ms(alternatives[k])
            if rep >= warmup:
                samples[k].append(ms)
    return {k: spread(v) for k, v in samples.items()}


def trace_run(what):
    """the encodes, then TRACE_ROUNDS rounds of the 32-chunk row, batched or as the loop: what a kernel trace sees"""
    a.set_device(0)
    dev = torch.device("cuda", 0)
    chunks = encode_chunks(dev, N_CHUNKS)
    qw, qh = a.preview_dims(W, H)
    qb = qw * qh * 3
    d_out = torch.empty(N_CHUNKS * qb, dtype=torch.uint8, device=dev)
    items = [(c.data_ptr(), n, FRAME, 1, d_out.data_ptr() + i * qb) for i, (c, n) in enumerate(chunks)]
    for _ in range(TRACE_ROUNDS):
        if what == "batched":
            a.previews_decode_device(items)
        else:
            for it in items:
                a.preview_decode_device(*it)
    torch.cuda.synchronize()
    print(f"{what}: {TRACE_ROUNDS} rounds of {N_CHUNKS} one-frame previews")
    return 0


def trace_parse(trace_dir, out):
    """DIR/<run>/**/*_kernel_trace.csv -> per run and kernel: launches, total, average, minimum and maximum microseconds"""
    import csv
    import glob
    res = {"what": f"rocprofv3 --kernel-trace --stats, a run of its own per entry and no counters, {TRACE_ROUNDS} rounds after the "
                   f"encodes: {N_CHUNKS} one-frame previews [{FRAME}, {FRAME + 1}) of {N_CHUNKS} distinct 1920x1080x64 CDF 9/7 chunks "
                   "(lane length 512, versions 2 and 3 alternating) through one batched call per round (batched_32) and through a "
                   "loop of single calls per round (loop_32); kernel time per launch in microseconds, and per round in total",
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
    qw, qh = a.preview_dims(W, H)
    qb = qw * qh * 3
    d_batched = torch.empty(F * qb, dtype=torch.uint8, device=dev)
    d_single = torch.empty(F * qb, dtype=torch.uint8, device=dev)
    d_whole = torch.empty(F * qb, dtype=torch.uint8, device=dev)
    res = {"device": torch.cuda.get_device_name(0), "chunk": [W, H, F], "preview": [qw, qh], "wavelet": "cdf97", "lane_symbols": LANE,
           "containers": {f"chunk {i} mod 2 = {i}": {"format": name, "quality": q} for i, (name, q) in enumerate(CONTAINERS)},
           "container_bytes": [n for _, n in chunks], "reps": args.reps, "warmup": args.warmup,
           "timing": "HIP events around each alternative (a batched call; a loop of single calls); the alternatives of a row rotate inside "
                     "every repetition",
           "stats_columns": ["items", "distinct containers", "table launches", "lane launches", "finish launches", "stream drains",
                             "blocks decoded", "payload bytes uploaded", "symbols stored"],
           "rows": {}}
    ok = True

    def row(name, items_batched, items_single, extra=None):
        nonlocal ok
        alternatives = {
            "batched": lambda: a.previews_decode_device(items_batched),
            "loop_of_single_calls": lambda: [a.preview_decode_device(*it) for it in items_single],
        }
        if extra:
            alternatives.update(extra)
        r = timed_row(alternatives, args.warmup, args.reps)
        d_batched.zero_()
        d_single.zero_()
        alternatives["batched"]()
        stats = a._test_last_previews_stats()
        alternatives["loop_of_single_calls"]()
        torch.cuda.synchronize()
        n_bytes = len(items_batched) * qb
        same = bool(torch.equal(d_batched[:n_bytes], d_single[:n_bytes])) and bool(d_batched[:n_bytes].any())
        ok = ok and same
        b, lp = r["batched"], r["loop_of_single_calls"]
        r.update(items=len(items_batched), batched_equals_single_calls=same, stats=list(stats),
                 batched_over_loop=round(b["median_ms"] / lp["median_ms"], 4),
                 batched_inside_loop_spread=bool(b["median_ms"] <= lp["max_ms"]), batched_faster_than_loop=bool(b["max_ms"] < lp["min_ms"]))
        res["rows"][name] = r
        print(f"{name}: batched {b['median_ms']:.3f} ms [{b['min_ms']:.3f}, {b['max_ms']:.3f}], loop {lp['median_ms']:.3f} ms "
              f"[{lp['min_ms']:.3f}, {lp['max_ms']:.3f}], ratio {r['batched_over_loop']:.3f}; stats {stats}; "
              f"{'equal' if same else 'DIFFERENT'} bytes", flush=True)
        return r

    for n in ROWS_N:
        row(f"{n} distinct chunks, frame [{FRAME}, {FRAME + 1}) of each",
            [(c.data_ptr(), m, FRAME, 1, d_batched.data_ptr() + i * qb) for i, (c, m) in enumerate(chunks[:n])],
            [(c.data_ptr(), m, FRAME, 1, d_single.data_ptr() + i * qb) for i, (c, m) in enumerate(chunks[:n])])
    for ci in (0, 1):
        c, m = chunks[ci]
        r = row(f"64 one-frame previews of chunk {ci} ({CONTAINERS[ci][0]})",
                [(c.data_ptr(), m, t, 1, d_batched.data_ptr() + t * qb) for t in range(F)],
                [(c.data_ptr(), m, t, 1, d_single.data_ptr() + t * qb) for t in range(F)],
                {"single_preview_of_the_whole_chunk": lambda: a.preview_decode_device(c.data_ptr(), m, 0, F, d_whole.data_ptr())})
        same = bool(torch.equal(d_whole, d_batched))
        r["whole_chunk_preview_equals_batched"] = same
        ok = ok and same
    res["all_batched_results_equal_the_single_calls"] = ok
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
