"""Developer probe on a GPU box: what one window refill costs the rANS decode chains where they run, in the batch.

    python scripts/refill_cost_fit.py chunks [out.json]          (ALICE_DEC_TILE selects the tile, as everywhere)

One Batch encode + decode at the benchmark's shape (1920x1080x64, CDF 9/7, q = 80) of `chunks` chunks made by
bench.synth_chunk(dev, i), so that the byte counts differ from chain to chain.  Every chain decodes the same number of symbols
and refills its window once per four stream bytes; the decoder's own cycle stamps (ALICE_CODEC_DEBUG: "decode chain i:
consumed ... bytes, ... Mcycles") give, by least squares over all chains,

    cycles = a * symbols + b * (bytes / 4)

a: shader cycles per symbol without refills, b: shader cycles per refill.  Prints a, b, the residual and the per-channel
medians (chain i belongs to channel i % 3: Y, Co, Cg) as one JSON line.  The stamps have a resolution of 1024 cycles against
some 10^10 per chain.  Not the bench; see bench.py."""
import json
import os
import re
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["ALICE_CODEC_DEBUG"] = "1"
import numpy as np  # noqa: E402
import torch  # noqa: E402
import alice_codec_amd as a  # noqa: E402
import bench  # noqa: E402

B = int(sys.argv[1])
W, H, F = bench.W, bench.H, bench.F
dev = torch.device("cuda:0")
rgb = torch.empty((B, F, H, W, 3), dtype=torch.uint8, device=dev)
for i in range(B):
    rgb[i] = bench.synth_chunk(dev, i)
torch.cuda.synchronize()
torch.cuda.empty_cache()   # the generator's temporaries: the batch needs the memory
st =torch.cuda.current_stream().cuda_stream
bt = a.Batch(W, H, F, B, bench.QUALITY, a.WaveletType.Cdf97)
log = tempfile.TemporaryFile(mode="w+")
sys.stderr.flush()
saved = os.dup(2)
os.dup2(log.fileno(), 2)
try:
    for _ in range(2):                      # the second pass is the one that counts: clocks and code objects are warm
        log.seek(0)
        log.truncate()
        bt.encode(rgb.data_ptr(), st)
        bt.encode_finish()
        bt.decode(bt.alc_ptr(0), bt.alc_stride, None, st)
        bt.decode_finish()
        ms = bt.stage_ms()
finally:
    os.dup2(saved, 2)
    os.close(saved)
log.seek(0)
rows = {}
for line in log.read().splitlines():
    m = re.search(r"decode chain (\d+): consumed (\d+) bytes, fast tiles (\d+), slow tiles (\d+), ([0-9.]+) Mcycles", line)
    if m:
        rows[int(m.group(1))] = (int(m.group(2)), float(m.group(5)) * 1e6, int(m.group(4)))
assert sorted(rows) == list(range(3 * B)), f"{len(rows)} decode chain lines for {3 * B} chains"
nbytes = np.array([rows[i][0] for i in range(3 * B)], np.float64)
cycles = np.array([rows[i][1] for i in range(3 * B)], np.float64)
symbols = np.full(3 * B, float(W * H * F))
A = np.stack([symbols, nbytes / 4], axis=1)
(ca, cb), *_ = np.linalg.lstsq(A, cycles, rcond=None)
resid = cycles - A @ np.array([ca, cb])
chan = {}
for c, name in enumerate(("Y", "Co", "Cg")):
    chan[name] = {"bits_per_symbol": round(float(np.median(nbytes[c::3])) * 8 / (W * H * F), 4),
                  "symbols_per_refill": round(4 * W * H * F / float(np.median(nbytes[c::3])), 3),
                  "cycles_per_symbol": round(float(np.median(cycles[c::3])) / (W * H * F), 3)}
slow = int(np.argmax(cycles))
result = {"tile": os.environ.get("ALICE_DEC_TILE", "default"), "chunks": B, "chains": 3 * B,
          "a_cycles_per_symbol": round(float(ca), 3), "b_cycles_per_refill": round(float(cb), 2),
          "residual_rms_cycles_per_symbol": round(float(np.sqrt(np.mean(resid ** 2))) / (W * H * F), 4),
          "residual_max_cycles_per_symbol": round(float(np.abs(resid).max()) / (W * H * F), 4),
          "median_per_channel": chan,
          "slowest_chain": {"chain": slow, "channel": ("Y", "Co", "Cg")[slow % 3], "cycles_per_symbol": round(float(cycles[slow]) / (W * H * F), 3),
                            "refills_per_block": round(float(nbytes[slow]) / 4 / (W * H * F / 64), 3)},
          "chains_with_slow_tiles": int(sum(1 for i in rows if rows[i][2])),
          "rans_decode_ms": round(float(ms["rans_decode"]), 1)}
print(json.dumps(result), flush=True)
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
