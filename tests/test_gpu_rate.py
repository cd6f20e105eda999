"""Rate prediction and budget encodes on the MI355X, against the oracle: the step histograms the GPU derives from one
coefficient histogram per channel must be the headers' histograms of oracle.encode at every step, the brackets must be
rate_ref's integers, real encodes must fall inside them, and encode_to_size must give the oracle's bytes at the quality
the budget rule picks."""
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rate_ref as R  # noqa: E402

import torch  # noqa: E402

pytestmark = pytest.mark.gpu


def _source(seed, w, h, f, noise=8):
    """smooth gradients plus noise, packed RGB of f frames"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = ((x[None] * 3 + y[None] * 2 + np.arange(f)[:, None, None] * 5) % 256).astype(np.int16)
    rgb = np.stack([base, 255 - base, (base * 7) % 256], axis=3) + rng.integers(-noise, noise + 1, (f, h, w, 3))
    return np.clip(rgb, 0, 255).astype(np.uint8).reshape(-1)


@pytest.fixture(scope="module")
def table(gpu_codec):
    return R.log_table(gpu_codec)


def _device_prediction(codec, rgb, w, h, f, wavelet, n_chunks=1):
    d = torch.from_numpy(np.ascontiguousarray(rgb)).to("cuda:0")
    hist = torch.zeros(n_chunks * 64 * 3 * 256, dtype=torch.int32, device="cuda:0")
    p = codec.predict_sizes_device(d.data_ptr(), w, h, f, n_chunks, wavelet, hist.data_ptr())
    torch.cuda.synchronize()
    return p, hist.cpu().numpy().view(np.uint32).reshape(n_chunks, 64, 3, 256)


CASES = [   # (w, h, f, noise): odd shapes, f = 1, a tile-path shape, generic-path shapes (a padded side < 6)
    (13, 9, 3, 8), (16, 12, 1, 40), (70, 50, 6, 8), (3, 40, 4, 8), (33, 3, 2, 60),
]


@pytest.mark.parametrize("wavelet", [0, 1, 2])
@pytest.mark.parametrize("case", CASES)
def test_step_histograms_and_cost_are_exact(gpu_codec, oracle_mod, table, case, wavelet):
    w, h, f, noise = case
    rgb = _source(w * 7 + h + f, w, h, f, noise)
    p, hist = _device_prediction(gpu_codec, rgb, w, h, f, wavelet)
    want = R.oracle_step_hists(oracle_mod, rgb, w, h, f, wavelet)
    assert np.array_equal(hist[0], want)
    lo, hi, st = R.chunk_prediction(oracle_mod, want, table)
    assert np.array_equal(p.lo[0], lo) and np.array_equal(p.hi[0], hi) and np.array_equal(p.status[0], st)
    hp = gpu_codec.predict_sizes(rgb, w, h, f, wavelet)
    assert np.array_equal(hp.lo, lo) and np.array_equal(hp.hi, hi) and np.array_equal(hp.status, st)
    for q in range(101):   # real encodes fall inside the bracket
        n = len(oracle_mod.encode(rgb, w, h, f, q, wavelet))
        if st[q] == R.BOUNDED:
            assert lo[q] <= n <= hi[q], (q, lo[q], n, hi[q])


def test_banded_chunk_and_shrunk_radius(gpu_codec, oracle_mod, table):
    lib = gpu_codec.load_library()
    w, h, f = 96, 200, 4
    rgb = _source(11, w, h, f, 30)
    try:
        lib.alice_codec_test_set_tuning(16)           # several bands of a few tile rows each
        for wavelet in (0, 1):
            p, hist = _device_prediction(gpu_codec, rgb, w, h, f, wavelet)
            want = R.oracle_step_hists(oracle_mod, rgb, w, h, f, wavelet)
            assert np.array_equal(hist[0], want)
            lo, hi, st = R.chunk_prediction(oracle_mod, want, table)
            assert np.array_equal(p.lo[0], lo) and np.array_equal(p.hi[0], hi) and np.array_equal(p.status[0], st)
        lib.alice_codec_test_set_tuning(1024 * 1024)
        lib.alice_codec_test_set_value_table_radius(24)   # coefficients outside [-24, 24): the per-step fallback
        for (ww, hh, ff) in ((w, h, f), (5, 20, 3)):
            r = _source(3, ww, hh, ff, 30)
            p, hist = _device_prediction(gpu_codec, r, ww, hh, ff, 1)
            want = R.oracle_step_hists(oracle_mod, r, ww, hh, ff, 1)
            assert np.array_equal(hist[0], want)
            lo, hi, st = R.chunk_prediction(oracle_mod, want, table)
            assert np.array_equal(p.lo[0], lo) and np.array_equal(p.hi[0], hi)
    finally:
        lib.alice_codec_test_set_tuning(1024 * 1024)
        lib.alice_codec_test_set_value_table_radius(2048)


def test_many_chunks_in_one_device_call(gpu_codec, oracle_mod, table):
    w, h, f, n = 24, 16, 4, 3
    rgb = np.concatenate([_source(40 + i, w, h, f, 4 + 30 * i) for i in range(n)])
    p, hist = _device_prediction(gpu_codec, rgb, w, h, f, 0, n)
    for i in range(n):
        chunk = rgb[i * w * h * f * 3:(i + 1) * w * h * f * 3]
        want = R.oracle_step_hists(oracle_mod, chunk, w, h, f, 0)
        assert np.array_equal(hist[i], want)
        lo, hi, st = R.chunk_prediction(oracle_mod, want, table)
        assert np.array_equal(p.lo[i], lo) and np.array_equal(p.hi[i], hi) and np.array_equal(p.status[i], st)


def test_bracket_on_a_1080p64_chunk(gpu_codec, oracle_mod, table):
    w, h, f = 1920, 1080, 64
    rgb = _source(1080, w, h, f, 6)
    p = gpu_codec.predict_sizes(rgb, w, h, f, gpu_codec.WaveletType.Cdf53)
    for q in (30, 80, 95):
        got = gpu_codec.FrameEncoder.with_wavelet(q, gpu_codec.WaveletType.Cdf53).encode(rgb, w, h, f).to_bytes()
        assert got == oracle_mod.encode(rgb, w, h, f, q, 0, three_threads=True)
        # the prediction at q is rate_ref's model of the encoded header's own histograms
        st = [R.channel_cost(oracle_mod, hh, table) for hh in R.header_hists(got)]
        worst = max(c[0] for c in st)
        assert p.status[q] == worst == R.BOUNDED
        assert p.lo[q] == R.HEADER + sum(c[1] for c in st) and p.hi[q] == R.HEADER + sum(c[2] for c in st)
        assert p.lo[q] <= len(got) <= p.hi[q], (q, p.lo[q], len(got), p.hi[q])


def _budget_cases():
    shapes = [(24, 16, 4), (13, 9, 3), (70, 50, 6)]
    out = []
    for i, (w, h, f) in enumerate(shapes):
        rgb = _source(100 + i, w, h, f, 20)
        out.append((rgb, w, h, f))
    return out


def test_encode_to_size_matches_oracle_and_threads(gpu_codec, oracle_mod):
    cases = _budget_cases()
    jobs = []
    for rgb, w, h, f in cases:
        p = gpu_codec.predict_sizes(rgb, w, h, f, 1)
        for budget in (0, int(p.hi[50]), int(p.hi[95]) + 10, 10**12):   # none fits, mid, max_q fits, anything fits
            jobs.append((rgb, w, h, f, budget, p))
    single = []
    for rgb, w, h, f, budget, p in jobs:
        chunk, q, fits = gpu_codec.encode_to_size(rgb, w, h, f, budget, 1, 10, 95)
        assert (q, fits) == R.choose(p.hi, p.status, budget, 10, 95)
        got = chunk.to_bytes()
        assert got == oracle_mod.encode(rgb, w, h, f, q, 1)
        if fits:
            assert len(got) <= budget
        single.append((q, fits, got))
    assert any(not s[1] for s in single) and any(s[0] == 95 for s in single)
    results = [None] * len(jobs)

    def run(k):
        for i in range(k, len(jobs), 8):
            rgb, w, h, f, budget, _ = jobs[i]
            chunk, q, fits = gpu_codec.encode_to_size(rgb, w, h, f, budget, 1, 10, 95)
            results[i] = (q, fits, chunk.to_bytes())

    threads = [threading.Thread(target=run, args=(k,)) for k in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert results == single


# ---- batches: per-chunk qualities and budget encodes ----

def _batch_alcs(bt, sizes):
    packed = torch.empty(int(sizes.sum()), dtype=torch.uint8, device="cuda:0")
    bt.pack_alc(sizes, packed.data_ptr(), packed.numel())
    torch.cuda.synchronize()
    host = packed.cpu().numpy()
    ends = np.cumsum(sizes.astype(np.int64))
    return [host[e - int(s):e].tobytes() for e, s in zip(ends, sizes)]


def test_budget_batch(gpu_codec, oracle_mod):
    a = gpu_codec
    w, h, f, n = 40, 24, 4, 6
    chunks = [_source(200 + i, w, h, f, 2 + 12 * i) for i in range(n)]
    rgb = np.concatenate(chunks)
    d = torch.from_numpy(rgb).to("cuda:0")
    bt = a.Batch(w, h, f, n, 80, a.WaveletType.Cdf97)
    p = bt.predict_sizes(d.data_ptr())
    for i in range(n):   # the batch's prediction is the one-chunk call's
        one = a.predict_sizes(chunks[i], w, h, f, a.WaveletType.Cdf97)
        assert np.array_equal(p.hi[i], one.hi) and np.array_equal(p.lo[i], one.lo) and np.array_equal(p.status[i], one.status)
    budgets = [0, int(p.hi[1][95]) + 5, int(p.hi[2][40]), int(p.hi[3][70]) + 100, int(p.hi[4][20]), 10**12]
    chosen, fits = bt.encode_to_budget(d.data_ptr(), budgets, 10, 95)
    for i in range(n):
        assert (int(chosen[i]), bool(fits[i])) == R.choose(p.hi[i], p.status[i], budgets[i], 10, 95)
    assert not fits[0] and chosen[1] == 95 and fits[1]
    got = _batch_alcs(bt, bt.encode_finish())
    for i in range(n):
        assert got[i] == oracle_mod.encode(chunks[i], w, h, f, int(chosen[i]), 1), i
        if fits[i]:
            assert len(got[i]) <= budgets[i]
    out = torch.empty_like(d)
    bt.decode(bt.alc_ptr(0), bt.alc_stride, out.data_ptr())
    bt.decode_finish()
    dec = out.cpu().numpy()
    for i in range(n):
        assert np.array_equal(dec[i * w * h * f * 3:(i + 1) * w * h * f * 3], oracle_mod.decode(got[i])), i


def test_per_chunk_qualities(gpu_codec, oracle_mod):
    a = gpu_codec
    w, h, f, n = 24, 16, 4, 4
    chunks = [_source(300 + i, w, h, f, 10) for i in range(n)]
    d = torch.from_numpy(np.concatenate(chunks)).to("cuda:0")
    bt = a.Batch(w, h, f, n, 75, a.WaveletType.Cdf53)
    bt.encode(d.data_ptr())
    plain = _batch_alcs(bt, bt.encode_finish())
    qs = [5, 100, 75, 42]
    bt.set_qualities(qs)
    bt.encode(d.data_ptr())
    mixed = _batch_alcs(bt, bt.encode_finish())
    for i in range(n):
        assert mixed[i] == oracle_mod.encode(chunks[i], w, h, f, qs[i], 0), i
    out = torch.empty_like(d)   # a mixed-quality batch decodes: each chunk's steps come from its own header
    bt.decode(bt.alc_ptr(0), bt.alc_stride, out.data_ptr())
    bt.decode_finish()
    dec = out.cpu().numpy()
    for i in range(n):
        assert np.array_equal(dec[i * w * h * f * 3:(i + 1) * w * h * f * 3], oracle_mod.decode(mixed[i])), i
    bt.set_qualities(None)
    bt.encode(d.data_ptr())
    assert _batch_alcs(bt, bt.encode_finish()) == plain
    # regions of larger frames, each at its own quality
    W, H = 64, 40
    frames = np.stack([_source(400 + i, W, H, f, 10).reshape(f, H, W, 3) for i in range(n)]).reshape(-1)
    origins = [(0, 0), (5, 7), (40, 24), (17, 3)]
    df = torch.from_numpy(frames).to("cuda:0")
    bt.set_qualities(qs)
    bt.encode_regions(df.data_ptr(), W, H, origins)
    got = _batch_alcs(bt, bt.encode_finish())
    fr = frames.reshape(n * f, H, W, 3)
    for i, (x0, y0) in enumerate(origins):
        crop = np.ascontiguousarray(fr[i * f:(i + 1) * f, y0:y0 + h, x0:x0 + w]).reshape(-1)
        assert got[i] == oracle_mod.encode(crop, w, h, f, qs[i], 0), i


# ---- command line ----

def test_cli_budget_options(gpu_codec, oracle_mod, tmp_path):
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    w, h, f = 32, 24, 4
    rgb = _source(500, w, h, f, 12)
    raw = tmp_path / "in.rgb"
    rgb.tofile(raw)
    p = gpu_codec.predict_sizes(rgb, w, h, f, 0)
    budget = int(p.hi[60])
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cli = [sys.executable, "-c", "import sys, alice_codec_amd.cli as c; sys.exit(c.main())"]
    out = subprocess.run(cli + ["encode", str(raw), "-o", str(tmp_path / "a.alc"), "-W", str(w), "-H", str(h), "-f", str(f),
                                "--max-bytes", str(budget)], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stderr
    q, fits = R.choose(p.hi, p.status, budget, 10, 95)
    assert fits and f"chosen quality: {q}" in out.stderr
    data = (tmp_path / "a.alc").read_bytes()
    assert len(data) <= budget and data == oracle_mod.encode(rgb, w, h, f, q, 0)
    assert oracle_mod.decode(data).size == rgb.size
    out = subprocess.run(cli + ["encode", str(raw), "-o", str(tmp_path / "b.alc"), "-W", str(w), "-H", str(h), "-f", str(f),
                                "--max-bytes", "10"], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0 and "warning" in out.stderr and (tmp_path / "b.alc").exists()
    # encode-chunks at a bitrate: 3 chunks of 4 frames, each within floor(target_bits_per_frame * 4 / 8) bytes
    long = np.concatenate([_source(600 + i, w, h, 4, 12) for i in range(3)])
    long.tofile(tmp_path / "long.rgb")
    kbps, fps = 2000, 30.0
    out = subprocess.run(cli + ["encode-chunks", str(tmp_path / "long.rgb"), "-o", str(tmp_path / "c"), "-W", str(w), "-H", str(h),
                                "-c", "4", "--kbps", str(kbps), "--fps", str(fps), "--in-flight", "3"],
                         capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stderr
    budget = gpu_codec.budget_bytes_per_chunk(kbps, fps, 4)
    for k in range(3):
        data = (tmp_path / f"c.{k:05d}.alc").read_bytes()
        part = long[k * w * h * 4 * 3:(k + 1) * w * h * 4 * 3]
        pk = gpu_codec.predict_sizes(part, w, h, 4, 0)
        qk, fk = R.choose(pk.hi, pk.status, budget, 10, 95)
        assert f"chunk {k}:" in out.stderr and f"chosen quality: {qk}" in out.stderr
        assert data == oracle_mod.encode(part, w, h, 4, qk, 0)
        if fk:
            assert len(data) <= budget
        assert oracle_mod.decode(data).size == part.size
