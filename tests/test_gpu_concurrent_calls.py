"""Every entry-point family beside every other one (many threads may call at once).  The families share one
device pool whose blocks go back after draining only the stream they were tagged with, three short streams and the hub's
merged chain launches, the caller-stream scope and a dozen thread-local records; a block that reaches a second thread too
early, a record that is not per thread or a stage chain mishandled inside a merged launch shows only when calls of different
kinds overlap.  The jobs and their expected values are tests/concurrent_cases.py's: every comparison is bit-exact against the
CPU references.  Eight threads, each with a fixed list that it runs once; the first mismatch fails the test.

JOIN_LIMIT holds, per test, ten times the run time measured on an MI355X and at least 60 s; nothing asserts on speed."""
import ctypes as C
import os
import sys
import threading
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import concurrent_cases as CC  # noqa: E402

pytestmark = pytest.mark.gpu

THREADS = 8
# seconds; measured on an MI355X: each_job_alone 1.39 (no threads), side_by_side 0.06, stage_chains 0.12, caller_streams 0.67,
# refusals 0.08, per_thread_records 0.11 -- ten times each is below the floor of 60
JOIN_LIMIT = {"side_by_side": 60, "stage_chains": 60, "caller_streams": 60, "refusals": 60, "records": 60}


def run_threads(fns, limit, on_error=None):
    """every fn on a thread of its own; -> the exceptions.  Fails if a thread is still alive `limit` seconds after the start."""
    errs = []

    def guard(fn):
        try:
            fn()
        except BaseException as e:   # noqa: BLE001
            errs.append(e)
            if on_error is not None:
                on_error()
    th = [threading.Thread(target=guard, args=(fn,), daemon=True) for fn in fns]
    deadline = time.monotonic() + limit
    [t.start() for t in th]
    for t in th:
        t.join(max(0.0, deadline - time.monotonic()))
    alive = [i for i, t in enumerate(th) if t.is_alive()]
    assert not alive, f"threads {alive} still run after {limit} s"
    return errs


def _message(a) -> str:
    return (a.load_library().alice_codec_last_error_message() or b"").decode()


# ---- the thread-local records ----
def _decode_stats(a):
    out = (C.c_uint32 * 4)()
    a.load_library().alice_codec_test_last_decode_stats(out)
    return tuple(int(v) for v in out)


def _split_trials(a):
    out = np.zeros(1, np.uint32)
    got = a.load_library().alice_codec_test_last_split_trials(out.ctypes.data_as(C.POINTER(C.c_uint32)), 1)
    return int(got), int(out[0])


def _record_jobs():
    """[(job, reader of the record the job leaves in its thread)]"""
    fams = CC.by_family()
    out = [(j, lambda a: a._test_last_frames_stats()) for j in fams["frames"]]
    out += [(j, lambda a: a._test_last_preview_stats()) for j in fams["preview"]]
    out += [(j, lambda a: a._test_last_rect_stats()) for j in fams["rect"]]
    out += [(j, lambda a: a._test_last_previews_stats()) for j in fams["previews"]]
    out += [(j, _decode_stats) for j in fams["stage"] if "RansDecoder decode_n" in j.name]
    out += [(j, _split_trials) for j in fams["rate"] if "to_size" in j.name]
    return out


_alone = {}


def _alone_records(a):
    """the record every record job leaves when it runs alone (plan figures: deterministic)"""
    if not _alone:
        for job, read in _record_jobs():
            CC.check(job, a)
            _alone[job.name] = read(a)
    return _alone


def test_each_job_alone(gpu_codec):
    """A failure here is a kernel or a reference matter, not one of concurrency: the other tests' messages rely on this one."""
    a = gpu_codec
    t0 = time.monotonic()
    for job in CC.jobs():
        CC.check(job, a)
    stream = torch.cuda.Stream(device=CC.DEV)
    for job in CC.device_jobs():
        CC.check_device(job, a, stream)
    records = _alone_records(a)
    # the records are the plans', not just repeatable
    import frames_ref as FR
    import preview_ref as PR
    import rect_ref as RF
    for (case, f0, f1), job in zip(CC.FRAMES_CASES, CC.by_family()["frames"]):
        plan = FR.frame_plan(case[1], *case[0], CC.LANE, f0, f1)
        assert records[job.name][:3] == (plan["a"], plan["b"], 3 * plan["n_planned"]) and records[job.name][4] == f1 - f0, job.name
    for (case, f0, f1), job in zip(CC.PREVIEW_CASES, CC.by_family()["preview"]):
        plan = PR.preview_plan(case[1], *case[0], CC.LANE, f0, f1)
        assert records[job.name][:3] == (plan["a"], plan["b"], 3 * plan["n_planned"]) and records[job.name][5] == plan["stored"], job.name
    for (case, f0, f1, rect), job in zip(CC.RECT_CASES, CC.by_family()["rect"]):
        plan = RF.rect_plan(case[1], *case[0], CC.LANE, f0, f1, rect, classes=False)
        assert records[job.name][:7] == (plan["ta"], plan["tb"], plan["xa"], plan["xb"], plan["ya"], plan["yb"], 3 * plan["n_planned"]), job.name
    for job in CC.by_family()["previews"]:
        assert records[job.name][0] in (3, 5) and records[job.name][2] == 1, job.name
    assert records["rate/encode_split_to_size (33, 17, 5) wavelet 1"] == (1, CC.budget_choice((33, 17, 5), CC.CDF97, False)[3])
    assert records["rate/encode_wide_to_size (40, 24, 1) wavelet 2"] == (1, CC.budget_choice((40, 24, 1), CC.HAAR, True)[3])
    print(f"each_job_alone: {time.monotonic() - t0:.2f} s for {len(CC.jobs())} host and {len(CC.device_jobs())} device jobs")


def _outcome(job, a, stream=None):
    """check(), reduced to what can be compared again after the join"""
    got = CC.check(job, a, stream)
    return ("error", got.code) if CC.is_refusal(job.expected) else got


def test_host_calls_of_every_family_side_by_side(gpu_codec):
    a = gpu_codec
    fams = CC.by_family()
    names = list(CC.FAMILIES)
    n, k, rounds = len(names), 5, 3
    assert {(t + r * k) % n for t in range(THREADS) for r in range(rounds)} == set(range(n)), "every family takes a turn"
    barrier = threading.Barrier(THREADS)
    results, spans = {}, []
    t_start = time.monotonic()

    def work(t):
        for r in range(rounds):
            fam = names[(t + r * k) % n]
            barrier.wait(JOIN_LIMIT["side_by_side"])
            for job in fams[fam]:
                t0 = time.monotonic()
                got = _outcome(job, a)
                spans.append((fam, t0, time.monotonic()))
                results[(r, t, job.name)] = (job, got)
    errs = run_threads([lambda t=t: work(t) for t in range(THREADS)], JOIN_LIMIT["side_by_side"], barrier.abort)
    assert errs == [], errs[:3]
    print(f"side_by_side: {time.monotonic() - t_start:.2f} s for {len(results)} calls")
    assert len(results) == sum(len(fams[names[(t + r * k) % n]]) for t in range(THREADS) for r in range(rounds))
    for (r, t, name), (job, got) in results.items():
        assert CC.same(got, job.expected), (r, t, name, "differs after the join")
    # a run whose calls happened to serialise must not pass emptily
    for fam in names:
        mine = [(s, e) for f, s, e in spans if f == fam]
        others = [(s, e) for f, s, e in spans if f != fam]
        assert any(s < e2 and s2 < e for s, e in mine for s2, e2 in others), f"no call of {fam} overlapped a call of another family"


def test_stage_chains_ride_with_chunk_chains(gpu_codec, oracle_mod):
    """Six threads drive the stage-level objects while two encode and decode version 1 chunks of 128x64x8 throughout: the stage
    chains, resumed and kept open ones among them, leave in the hub's merged launches together with chunk chains."""
    a = gpu_codec
    stage = CC.by_family()["stage"]
    chains = [j for j in stage if "Rans" in j.name]
    w, h, f, q, kind = 128, 64, 8, 80, CC.CDF97
    rgbs = [CC.source((w, h, f), seed=900 + i) for i in range(2)]
    refs = [oracle_mod.encode(r, w, h, f, q, kind) for r in rgbs]
    wants = [np.asarray(oracle_mod.decode(r)) for r in refs]
    left = [6]
    lock = threading.Lock()
    all_done = threading.Event()
    chunk_calls = [0, 0]
    t_start = time.monotonic()

    def finished():
        with lock:
            left[0] -= 1
            if left[0] == 0:
                all_done.set()

    def stage_worker(jobs):
        try:
            for job in jobs:
                CC.check(job, a)
        finally:
            finished()

    def two_decoders():
        try:
            want_x, want_y = CC.decoder_expected(7, 30000), CC.decoder_expected(8, 23000)
            x, y = CC.decoder_steps(a, 7, 30000), CC.decoder_steps(a, 8, 23000)
            for i in range(len(CC.DECODER_CALLS)):      # one object per sequence, the calls of the two interleaved
                assert CC.same(next(x), want_x[i]), ("decoder of stream 7, call", i)
                assert CC.same(next(y), want_y[i]), ("decoder of stream 8, call", i)
            for seed, n in ((7, 30000), (8, 23000)):
                assert CC.single_symbols(a, seed, n) == CC.single_symbols_expected(seed, n), ("decode() one symbol at a time", seed)
            for job in chains[::-1]:
                CC.check(job, a)
        finally:
            finished()

    def chunks(i):
        enc = a.FrameEncoder.with_wavelet(q, a.WaveletType(kind))
        while True:       # throughout: as long as a stage thread runs, twice at least, 200 times at most
            assert enc.encode(rgbs[i], w, h, f).to_bytes() == refs[i], ("chunk encode", i, chunk_calls[i])
            assert np.array_equal(np.asarray(a.FrameDecoder().decode(a.EncodedChunk.from_bytes(refs[i]))), wants[i]), ("chunk decode", i)
            chunk_calls[i] += 1
            if (all_done.is_set() and chunk_calls[i] >= 2) or chunk_calls[i] >= 200:
                return
    fns = [lambda k=k: stage_worker(stage[k::4] + chains[k::2]) for k in range(4)] + [two_decoders, lambda: stage_worker(chains + stage[::3])]
    fns += [lambda i=i: chunks(i) for i in range(2)]
    assert len(fns) == THREADS
    errs = run_threads(fns, JOIN_LIMIT["stage_chains"], all_done.set)
    assert errs == [], errs[:3]
    assert min(chunk_calls) >= 2
    print(f"stage_chains: {time.monotonic() - t_start:.2f} s, chunk calls beside the stage jobs: {chunk_calls}")


def test_device_calls_on_caller_streams(gpu_codec):
    """Every thread owns a torch.cuda.Stream and hands it to the device-pointer calls; inputs arrive by a non-blocking copy on
    that stream right before the call, outputs start as 0xEE and are read after stream.synchronize() (concurrent_cases.OnStream)."""
    a = gpu_codec
    jobs = CC.device_jobs()
    results = {}
    t_start = time.monotonic()

    def work(t):
        stream = torch.cuda.Stream(device=CC.DEV)
        for i in range(len(jobs)):
            job = jobs[(3 * t + i) % len(jobs)]
            results[(t, job.name)] = (job, CC.check_device(job, a, stream))
    errs = run_threads([lambda t=t: work(t) for t in range(THREADS)], JOIN_LIMIT["caller_streams"])
    assert errs == [], errs[:3]
    print(f"caller_streams: {time.monotonic() - t_start:.2f} s for {len(results)} calls")
    assert len(results) == THREADS * len(jobs)
    for (t, name), (job, got) in results.items():
        if not CC.is_strided(job.expected):
            assert CC.same(got, job.expected), (t, name, "differs after the join")
        else:
            assert got[0] == len(job.expected[1]) and got[1][:got[0]].tobytes() == job.expected[1] and (got[1][got[0]:] == CC.FILL).all(), (t, name)


# ---- refusals ----
def _device_refusals(a, stream, t):
    """the device forms: each must raise its kind, name this thread's failure and leave its output 0xEE"""
    c = CC.REFUSAL_FRAMES_CASE
    w, h, f = c[0]
    blob = CC.container(*c)
    rows_bad = CC.previews_with_damage(1)
    sizes = [CC.preview_expected(cc, p0, p1).size for cc, p0, p1 in CC.PREVIEWS_ITEMS]
    offs = [64 + sum(sizes[:i]) + 64 * i for i in range(len(sizes))]       # the items' outputs do not overlap
    with CC.OnStream(stream) as s:
        out = s.out(max(offs[-1] + sizes[-1] + 64, w * h * 3))
        d_good, d_dir, d_v1 = s.up_bytes(blob), s.up_bytes(CC.directory_damaged(c)), s.up_bytes(CC.v1_blob())
        cases = [
            (lambda: a.frames_decode_device(d_good.data_ptr(), len(blob), f + t, 1, out.data_ptr(), s.cs), 2, f"frames [{f + t}, {f + t + 1})"),
            (lambda: a.rect_decode_device(d_good.data_ptr(), len(blob), 0, 1, w - 1 - t, 0, 2 + t, 1, out.data_ptr(), 0, 0, s.cs), 2,
             f"rectangle {2 + t}x1 at ({w - 1 - t}, 0)"),
            (lambda: a.frames_decode_device(d_dir.data_ptr(), len(blob), 0, 1, out.data_ptr(), s.cs), 4, "directory"),
            (lambda: a.frames_decode_device(d_v1.data_ptr(), len(CC.v1_blob()), 0, 1, out.data_ptr(), s.cs), 4, "version 1 has no random access"),
        ]
        for call, code, text in cases:
            with pytest.raises(a.CodecError) as e:
                call()
            assert e.value.code == code and text in _message(a), (t, code, text, _message(a))
        devs = [s.up_bytes(b) for b, _, _ in rows_bad]
        rows = [(d.data_ptr(), len(b), first, count, out.data_ptr() + offs[i]) for i, (d, (b, first, count)) in enumerate(zip(devs, rows_bad))]
        with pytest.raises(a.CodecError) as e:
            a.previews_decode_device(rows, s.cs)
        assert e.value.code == 4 and e.value.bad_item == 1 and _message(a).startswith("item 1: "), (t, _message(a))
        assert (s.back(out) == CC.FILL).all(), "a refused device call wrote to its output"


def test_refusals_beside_good_calls(gpu_codec):
    a = gpu_codec
    lib = a.load_library()
    fams = CC.by_family()
    refusals = fams["refusal"]
    good = [j for fam in ("frames", "preview", "rect", "previews", "v2", "v3", "v4") for j in fams[fam]]
    t_start = time.monotonic()
    counts = [0] * THREADS

    def refusing(t):
        stream = torch.cuda.Stream(device=CC.DEV)
        f = CC.REFUSAL_FRAMES_CASE[0][2]
        for i in range(len(refusals)):
            job = refusals[(t * 3 + i) % len(refusals)]
            e = CC.check(job, a)
            msg = _message(a)
            assert msg and msg in str(e), (t, job.name, msg, str(e))
            if "end check" in job.name:
                assert "end check" in msg, (job.name, msg)
            if "directory" in job.name:
                assert "directory" in msg or "block" in msg, (job.name, msg)
            if "item 1" in job.name:
                assert msg.startswith("item 1: ") and e.bad_item == 1, (job.name, msg)
            if t == 0:
                lib.alice_codec_trim()
            counts[t] += 1
        # this thread's own range in the message, not a neighbour's
        with pytest.raises(a.CodecError) as e:
            a.decode_frames(CC.container(*CC.REFUSAL_FRAMES_CASE), f + t, 1)
        assert e.value.code == 2 and f"frames [{f + t}, {f + t + 1})" in _message(a), (t, _message(a))
        _device_refusals(a, stream, t)

    def neighbour(t):
        for i in range(len(good)):
            job = good[(t * 5 + i) % len(good)]
            CC.check(job, a)
            assert _message(a) == "", (t, job.name, "a good call's thread holds an error message", _message(a))
            counts[t] += 1
    fns = [lambda t=t: refusing(t) for t in range(4)] + [lambda t=t: neighbour(t) for t in range(4, THREADS)]
    errs = run_threads(fns, JOIN_LIMIT["refusals"])
    assert errs == [], errs[:3]
    assert counts == [len(refusals)] * 4 + [len(good)] * 4
    print(f"refusals: {time.monotonic() - t_start:.2f} s")


def test_per_thread_records(gpu_codec):
    """Inside the mixed traffic every thread reads, after its own call, the record the call left: the figures must be the ones
    the same call gave when it ran alone."""
    a = gpu_codec
    alone = dict(_alone_records(a))
    record_jobs = _record_jobs()
    fams = CC.by_family()
    traffic = fams["v2"] + fams["v3"] + fams["quality"] + fams["segment"][:4] + fams["v1"][:2]
    seen = {}
    t_start = time.monotonic()

    def work(t):
        for i in range(len(record_jobs)):
            job, read = record_jobs[(2 * t + i) % len(record_jobs)]
            CC.check(job, a)
            got = read(a)
            assert got == alone[job.name], (t, job.name, "record", got, "alone", alone[job.name])
            seen[(t, job.name)] = got
            CC.check(traffic[(t + i) % len(traffic)], a)      # a call that leaves none of the records just read
    errs = run_threads([lambda t=t: work(t) for t in range(THREADS)], JOIN_LIMIT["records"])
    assert errs == [], errs[:3]
    assert len(seen) == THREADS * len(record_jobs)
    assert len({v for (_, name), v in seen.items() if "frames" in name}) >= 3, "the jobs' records differ, so a shared one would show"
    print(f"per_thread_records: {time.monotonic() - t_start:.2f} s for {len(seen)} records")
