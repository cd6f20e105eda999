"""All four instances of rans_decode_kernel (alice-codec_amd/csrc/rans.hip: one chain per SIMD or plain placement, vector or
classic tile) on the case list of tests/decode_chain_cases.py, in merged launches through alice_codec_test_decode_chains_ex.

Per process two launches: run A, the list once (at most 1024 chains: the exclusive instance), and run B, the list cycled to
at least 1100 chains (the plain instance), each repeat with the stream and output misalignments rotated by one.  Histogram
and array tables, fresh and resumed chains, chains that report through their descriptor and chains that report into
results[chain] share every launch; every chain's output lies between 16 guard bytes of 0xEE.  The parent process runs the
vector tile; a fresh child with ALICE_DEC_TILE=classic runs the same two launches and dumps its arrays.  Symbols, len and
final state must be the oracle's, the path mask and the tile counts the model's, for every chain of every run.

A Batch of 342 chunks (1026 chains: the smallest that leaves the exclusive instance) checks the plain instance end to end.

Run as a program (the child): python tests/test_gpu_decode_chain_fuzz.py OUT.npz"""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (os.path.dirname(os.path.abspath(__file__)), ROOT) if p not in sys.path]   # the child has neither
import decode_chain_cases as D  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 16
MIN_CHAINS_B = 1100
RUNS = [("vector", "A"), ("vector", "B"), ("classic", "A"), ("classic", "B")]
OUTPUTS = ("len", "final_state", "paths", "fast_tiles", "slow_tiles", "flags")


@functools.lru_cache(maxsize=None)
def _plan(run):
    """[(case, stream misalignment, output misalignment, own RansResult)] per chain"""
    cases = D.cases()
    reps = 1 if run == "A" else -(-MIN_CHAINS_B // len(cases))
    plan = [(c, (c.in_mis + r) % 4, (c.out_mis + r) % 4, k % 3 != 1) for r in range(reps) for k, c in enumerate(cases)]
    assert len(plan) <= 1024 if run == "A" else len(plan) >= MIN_CHAINS_B
    return plan


def _round16(v):
    return (v + 15) // 16 * 16


@functools.lru_cache(maxsize=None)
def _layout(run):
    """(stream offsets, output offsets, size of the stream buffer, size of the output buffer): chain c's stream starts at
    in_at[c], its symbols at out_at[c], each at its misalignment behind a 16-byte boundary, the symbols between two guards"""
    in_at, out_at, i, o = [], [], 0, 0
    for case, in_mis, out_mis, _ in _plan(run):
        in_at.append(i + in_mis)
        i += _round16(in_mis + len(case.data) + 1)
        out_at.append(o + GUARD + out_mis)
        o += _round16(GUARD + out_mis + case.n + GUARD)
    return in_at, out_at, i + 16, o + 16


def _launch(lib, run):
    import torch
    plan = _plan(run)
    in_at, out_at, in_size, out_size = _layout(run)
    k = len(plan)
    h_in = np.zeros(in_size, np.uint8)
    hists, cums, freqs = np.ones((k, 256), np.uint32), np.zeros((k, 256), np.uint16), np.full((k, 256), 16, np.uint16)
    cums[:] = 16 * np.arange(256)
    from_arrays, resume, x0, own = (np.zeros(k, np.uint32) for _ in range(4))
    pos0, lens, ns = (np.zeros(k, np.uint64) for _ in range(3))
    for c, (case, _, _, mine) in enumerate(plan):
        h_in[in_at[c]: in_at[c] + len(case.data)] = np.frombuffer(case.data, np.uint8)
        if case.hist is not None:
            hists[c] = case.hist
        else:
            cums[c], freqs[c], from_arrays[c] = case.cum, case.freq, 1
        resume[c], x0[c], pos0[c] = D.start_of(case)
        own[c], lens[c], ns[c] = mine, len(case.data), case.n
    d_in = torch.from_numpy(h_in).cuda()
    d_out = torch.full((out_size,), 0xEE, dtype=torch.uint8, device="cuda")
    assert d_in.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    vp = C.c_void_p
    streams, outs = (vp * k)(), (vp * k)()
    for c in range(k):
        streams[c], outs[c] = d_in.data_ptr() + in_at[c], d_out.data_ptr() + out_at[c]
    res = np.zeros((k, 6), np.uint32)
    u16p, u32p, u64p = C.POINTER(C.c_uint16), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    p32 = lambda a: a.ctypes.data_as(u32p)   # noqa: E731
    rc = lib.alice_codec_test_decode_chains_ex(k, streams, lens.ctypes.data_as(u64p), outs, ns.ctypes.data_as(u64p), p32(hists),
                                               cums.ctypes.data_as(u16p), freqs.ctypes.data_as(u16p), p32(from_arrays), p32(resume), p32(x0),
                                               pos0.ctypes.data_as(u64p), p32(own), p32(res), None)
    assert rc == 0, (run, rc)
    return d_out.cpu().numpy(), res


def _launch_both(lib):
    got = {}
    for run in ("A", "B"):
        got["out" + run], got["res" + run] = _launch(lib, run)
    return got


@pytest.fixture(scope="module")
def runs(gpu_codec, tmp_path_factory):
    """{(tile, run): (output buffer, six outputs per chain)}: this process with the vector tile, then a fresh child with the
    classic one (two processes with the GPU open at most)"""
    assert os.environ.get("ALICE_DEC_TILE") != "classic"
    mine = _launch_both(gpu_codec.load_library())
    dump = str(tmp_path_factory.mktemp("decode_chain_fuzz") / "classic.npz")
    flags = ["-s"] if sys.flags.no_user_site else []
    subprocess.run([sys.executable, *flags, os.path.abspath(__file__), dump], env=dict(os.environ, ALICE_DEC_TILE="classic"), check=True,
                   timeout=300)
    with np.load(dump) as z:
        theirs = {name: z[name] for name in z.files}
    return {(tile, run): (got["out" + run], got["res" + run]) for tile, got in (("vector", mine), ("classic", theirs)) for run in "AB"}


@functools.lru_cache(maxsize=None)
def _expected(case):
    return D.expected(case)


@functools.lru_cache(maxsize=None)
def _predicted(case, in_mis, out_mis):
    p = D.predict(case, in_mis, out_mis)
    return p["paths"], p["fast_tiles"], p["slow_tiles"]


def _name(run, c):
    case, in_mis, out_mis, mine = _plan(run)[c]
    return f"run {run} chain {c}: {case}, here in+{in_mis} out+{out_mis}, {'own' if mine else 'shared'} result"


@pytest.mark.parametrize("tile,run", RUNS)
def test_symbols_len_and_final_state_are_the_oracles(runs, oracle_mod, tile, run):
    out, res = runs[tile, run]
    out_at = _layout(run)[1]
    for c, (case, _, _, _) in enumerate(_plan(run)):
        sym, length, state = _expected(case)
        got = out[out_at[c]: out_at[c] + case.n]
        assert np.array_equal(got, sym), (tile, _name(run, c), "first difference at", int(np.argmax(got != sym)))
        assert (int(res[c, 0]), int(res[c, 1])) == (length, state), (tile, _name(run, c))


@pytest.mark.parametrize("tile,run", RUNS)
def test_guards_are_intact_and_flags_are_zero(runs, tile, run):
    out, res = runs[tile, run]
    out_at = _layout(run)[1]
    outside = np.ones(out.size, bool)
    for c, (case, _, _, _) in enumerate(_plan(run)):
        assert (out[out_at[c] - GUARD: out_at[c]] == 0xEE).all() and (out[out_at[c] + case.n: out_at[c] + case.n + GUARD] == 0xEE).all(), \
            (tile, _name(run, c))
        outside[out_at[c]: out_at[c] + case.n] = False
        assert int(res[c, 5]) == 0, (tile, _name(run, c), hex(int(res[c, 5])))
    assert (out[outside] == 0xEE).all()      # nothing between the chains either


@pytest.mark.parametrize("tile,run", RUNS)
def test_paths_and_tile_counts_are_the_models(runs, oracle_mod, tile, run):
    _, res = runs[tile, run]
    for c, (case, in_mis, out_mis, _) in enumerate(_plan(run)):
        paths, n_fast, n_slow = _predicted(case, in_mis, out_mis)
        got = (int(res[c, 2]), int(res[c, 3]), int(res[c, 4]))
        assert got == (paths, n_fast, n_slow), (tile, _name(run, c), "kernel", D.path_names(got[0]), got[1:], "model", D.path_names(paths),
                                                (n_fast, n_slow))


@pytest.mark.parametrize("tile,run", RUNS)
def test_every_branch_of_the_tile_loop_ran(runs, tile, run):
    seen = int(np.bitwise_or.reduce(runs[tile, run][1][:, 2]))
    missing = [name for bit, name in D.PATHS.items() if not seen & bit]
    assert not missing, f"{tile} tile, run {run}: branches never taken: {missing} (mask {seen:#x})"


@pytest.mark.parametrize("tile", ["vector", "classic"])
def test_plain_instance_repeats_the_exclusive_one(runs, tile):
    """chains 0 .. len(cases) - 1 of run B are the chains of run A"""
    (out_a, res_a), (out_b, res_b) = runs[tile, "A"], runs[tile, "B"]
    k = len(D.cases())
    assert _plan("B")[:k] == _plan("A") and _layout("B")[1][:k] == _layout("A")[1]
    for j, name in enumerate(OUTPUTS):
        bad = np.flatnonzero(res_a[:, j] != res_b[:k, j])
        assert bad.size == 0, (tile, name, _name("A", int(bad[0])))
    size = _layout("A")[3] - 16
    bad = np.flatnonzero(out_a[:size] != out_b[:size])
    assert bad.size == 0, (tile, "first differing output byte", int(bad[0]))


@pytest.mark.parametrize("run", ["A", "B"])
def test_classic_tile_gives_what_the_vector_tile_gives(runs, run):
    (out_v, res_v), (out_c, res_c) = runs["vector", run], runs["classic", run]
    for j, name in enumerate(OUTPUTS):
        bad = np.flatnonzero(res_v[:, j] != res_c[:, j])
        assert bad.size == 0, (name, _name(run, int(bad[0])))
    assert np.array_equal(out_v, out_c)


def _pixels(w, h, f, seed):
    """a moving gradient with a little noise: symbols of several values in every channel"""
    rng = np.random.default_rng(seed)
    t, y, x = np.meshgrid(np.arange(f), np.arange(h), np.arange(w), indexing="ij")
    rgb = np.stack([(9 * x + 5 * y + 7 * t + seed) % 256, (3 * x + 11 * y + seed // 3) % 256, (x * y + 13 * t) % 256], axis=-1)
    return ((rgb + rng.integers(-3, 4, rgb.shape)) % 256).astype(np.uint8).reshape(-1)


@pytest.mark.parametrize("wavelet", ["Cdf53", "Cdf97"])
def test_batch_of_342_chunks_decodes_on_the_plain_instance(gpu_codec, oracle_mod, wavelet):
    """3 * 342 = 1026 chains in the one launch_rans_decode of Batch decode: more than 1024"""
    import torch
    w, h, f, B, q = 16, 16, 2, 342, 80
    wt = gpu_codec.WaveletType[wavelet]
    chunks = [_pixels(w, h, f, 1000 + i) for i in range(B)]
    rgb = torch.from_numpy(np.stack(chunks)).cuda()
    out = torch.full_like(rgb, 0xEE)
    bt = gpu_codec.Batch(w, h, f, B, q, wt)
    st = torch.cuda.current_stream().cuda_stream
    bt.encode(rgb.data_ptr(), st)
    sizes = bt.encode_finish()
    stride = bt.alc_stride
    alc = torch.empty(B * stride, dtype=torch.uint8, device="cuda")
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(alc.data_ptr(), bt.alc_ptr(0), B * stride, 3) == 0   # device to device
    alc = alc.cpu().numpy()
    refs = [oracle_mod.encode(chunks[i], w, h, f, q, int(wt)) for i in range(B)]
    for i in range(B):
        assert alc[i * stride: i * stride + int(sizes[i])].tobytes() == refs[i], i
    bt.decode(bt.alc_ptr(0), stride, out.data_ptr(), st)
    bt.decode_finish()
    got = out.cpu().numpy()
    for i in range(B):
        assert np.array_equal(got[i], oracle_mod.decode(refs[i])), i


if __name__ == "__main__":
    import alice_codec_amd
    assert alice_codec_amd.device_count() >= 1
    alice_codec_amd.set_device(0)
    np.savez(sys.argv[1], **_launch_both(alice_codec_amd.load_library()))
