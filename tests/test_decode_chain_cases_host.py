"""The conditions tests/test_gpu_decode_chain_fuzz.py rests on, checked on the CPU: the tile-loop model of
tests/decode_chain_cases.py changes decisions, not results (its symbols, len and final state are the oracle's plain decode for
every case), and the case list reaches every branch of the tile loop, every kind of table, every misalignment and enough
resume points.  Prints the number of cases per class and per path bit."""
import collections
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_chain_cases as D  # noqa: E402


@pytest.fixture(scope="module")
def predicted(oracle_mod):
    return [(c, D.predict(c), D.expected(c)) for c in D.cases()]


def test_model_gives_the_oracles_results(predicted):
    for k, (c, p, (sym, length, state)) in enumerate(predicted):
        assert len(p["symbols"]) == c.n == len(sym), (k, str(c))
        assert np.array_equal(p["symbols"], sym), (k, str(c), int(np.argmax(p["symbols"] != sym)))
        assert (p["len"], p["state"]) == (length, state), (k, str(c))
        # every symbol belongs to exactly one tile; only the exact loop may cut one short
        assert p["fast_tiles"] * D.TILE <= c.n and p["fast_tiles"] + p["slow_tiles"] >= -(-c.n // D.TILE), (k, str(c))


def test_model_does_not_depend_on_alignment_for_results(predicted):
    """the misalignments move the window base and the output path, never a symbol (run B of the GPU test rotates them)"""
    for k, (c, p, _) in enumerate(predicted[::7]):
        q = D.predict(c, (c.in_mis + 1) % 4, (c.out_mis + 1) % 4)
        assert np.array_equal(q["symbols"], p["symbols"]) and (q["len"], q["state"]) == (p["len"], p["state"]), (k, str(c))


def test_every_path_bit_is_predicted(predicted, capsys):
    count = {bit: sum(1 for _, p, _ in predicted if p["paths"] & bit) for bit in D.PATHS}
    with capsys.disabled():      # part of the test's output whether it passes or not
        print()
        for bit, name in D.PATHS.items():
            print(f"  path bit {bit:5d} {name:36s} {count[bit]:4d} cases")
    short = [name for bit, name in D.PATHS.items() if count[bit] < 3]
    assert not short, f"fewer than 3 cases predicted for: {short}"


def test_coverage_conditions(predicted, capsys):
    per_class = collections.Counter(c.cls for c, _, _ in predicted)
    with capsys.disabled():
        print()
        for cls, k in per_class.items():
            print(f"  class {cls:28s} {k:4d} cases")
    assert len(predicted) >= 200
    assert len({(c.data, c.n, c.n1, c.in_mis, c.out_mis) for c, _, _ in predicted}) == len(predicted)   # distinct
    assert all(per_class[cls] >= 3 for cls in D.HIST_CLASSES + D.TABLE_CLASSES), per_class
    exact_tables = [c for c, p, _ in predicted if D.oracle_of(c).exact_only]
    assert len(exact_tables) >= 3
    assert all(p["fast_tiles"] == 0 for c, p, _ in predicted if D.oracle_of(c).exact_only)
    assert sum(1 for c, _, _ in predicted if c.n1 is not None) >= 24
    fast = [(c, p) for c, p, _ in predicted if p["paths"] & (D.WHOLE | D.SPEC_KEPT)]
    assert {c.in_mis for c, _ in fast} == {0, 1, 2, 3} and {c.out_mis for c, _ in fast} == {0, 1, 2, 3}
    tails = {c.n % D.TILE for c, _, _ in predicted if c.n > D.TILE}
    assert {0, *D.TAILS} <= tails
    assert {0, 1} <= {c.n for c, _, _ in predicted}
    assert all(c.n in (0, 1) or 3 * D.TILE <= c.n < 6 * D.TILE for c, _, _ in predicted)


def test_hook_refuses_bad_arguments_before_any_device_work(codec):
    """alice_codec_test_decode_chains_ex: missing arrays, and a resume position behind the end of its stream (no decoder
    object has one, and the kernel's window arithmetic relies on that)"""
    import ctypes as C
    lib = codec.load_library()
    vp = C.c_void_p
    streams, outs = (vp * 1)(0x1000), (vp * 1)(0x2000)     # never dereferenced: every check comes before the device is touched
    one = lambda t, v: (t * 1)(v)   # noqa: E731
    lens, ns, out = one(C.c_uint64, 100), one(C.c_uint64, 10), (C.c_uint32 * 6)()
    hist = (C.c_uint32 * 256)(*([1] * 256))
    arr = (C.c_uint16 * 256)(*([16] * 256))
    fn = lib.alice_codec_test_decode_chains_ex
    NULL_ARG, BUFFER_SIZE = 9, 1
    assert fn(1, streams, lens, outs, ns, None, None, None, None, None, None, None, None, out, None) == NULL_ARG      # no table
    assert fn(1, streams, lens, outs, ns, None, arr, None, None, None, None, None, None, out, None) == NULL_ARG       # half the arrays
    assert fn(1, streams, lens, outs, ns, hist, None, None, one(C.c_uint32, 1), None, None, None, None, out, None) == NULL_ARG   # a choice of one
    assert fn(1, streams, lens, outs, ns, hist, None, None, None, one(C.c_uint32, 1), None, None, None, out, None) == NULL_ARG   # resume without a state
    assert fn(0, streams, lens, outs, ns, hist, None, None, None, None, None, None, None, out, None) == NULL_ARG
    assert fn(1, streams, lens, (vp * 1)(None), ns, hist, None, None, None, None, None, None, None, out, None) == NULL_ARG
    assert lib.alice_codec_last_error() == NULL_ARG
    rc = fn(1, streams, lens, outs, ns, hist, None, None, None, one(C.c_uint32, 1), one(C.c_uint32, 1 << 23), one(C.c_uint64, 101), None, out, None)
    assert rc == BUFFER_SIZE and lib.alice_codec_last_error() == BUFFER_SIZE


def test_resume_points(predicted):
    """pos0 at every residue mod 4 against every stream misalignment; at the head of a stream misaligned by 3; on the dry
    stream; inside the last window"""
    res = [(c, *D.start_of(c)[1:]) for c, _, _ in predicted if c.n1 is not None]
    assert {(c.in_mis, pos0 % 4) for c, _, pos0 in res} == {(m, r) for m in range(4) for r in range(4)}
    assert {pos0 for c, _, pos0 in res if c.in_mis == 3 and c.n1 in (0, 1)} & {4, 5}
    assert sum(1 for c, _, pos0 in res if pos0 == len(c.data)) >= 3
    assert sum(1 for c, _, pos0 in res if len(c.data) - D.WINDOW < pos0 < len(c.data)) >= 3
    assert all(pos0 <= len(c.data) for c, _, pos0 in res)
