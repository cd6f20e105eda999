"""The shadow decode tile (alice-codec_amd/csrc/rans_decode_tile_sh.inc: the record in the stall behind the lane read, the
window shifts in the wait-state slots, the state alternating between two SGPR shift pairs) on the MI355X.

The 228 chains of tests/decode_chain_cases.py run in ONE alice_codec_test_decode_chains_ex launch with the default tile,
laid out and launched by tests/test_gpu_decode_chain_fuzz.py's run A, and once more in a fresh child process with
ALICE_DEC_TILE=vector.  Symbols, len and final state must be the oracle's, the path mask and the tile counts the model's, and
the two processes must agree on every byte of the output buffer and on all six outputs per chain.  (The chain fuzz itself
sets the default tile against the classic one; this file keeps the vector tile covered.)

Run as a program (the child): python tests/test_gpu_decode_tile_shadow.py OUT.npz"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (os.path.dirname(os.path.abspath(__file__)), ROOT) if p not in sys.path]   # the child has neither
import decode_chain_cases as D  # noqa: E402
import test_gpu_decode_chain_fuzz as F  # noqa: E402

pytestmark = pytest.mark.gpu

TILES = ("default", "vector")


@pytest.fixture(scope="module")
def runs(gpu_codec, tmp_path_factory):
    """{tile: (output buffer, six outputs per chain)}: this process with the default tile, then a fresh child with the
    vector tile (two processes with the GPU open at most)"""
    assert os.environ.get("ALICE_DEC_TILE") is None
    assert len(F._plan("A")) == len(D.cases()) == 228
    mine = F._launch(gpu_codec.load_library(), "A")
    dump = str(tmp_path_factory.mktemp("decode_tile_shadow") / "vector.npz")
    flags = ["-s"] if sys.flags.no_user_site else []
    subprocess.run([sys.executable, *flags, os.path.abspath(__file__), dump], env=dict(os.environ, ALICE_DEC_TILE="vector"), check=True,
                   timeout=300)
    with np.load(dump) as z:
        theirs = (z["out"], z["res"])
    return {"default": mine, "vector": theirs}


@pytest.mark.parametrize("tile", TILES)
def test_symbols_len_and_final_state_are_the_oracles(runs, oracle_mod, tile):
    out, res = runs[tile]
    out_at = F._layout("A")[1]
    for c, (case, _, _, _) in enumerate(F._plan("A")):
        sym, length, state = F._expected(case)
        got = out[out_at[c]: out_at[c] + case.n]
        assert np.array_equal(got, sym), (tile, F._name("A", c), "first difference at", int(np.argmax(got != sym)))
        assert (int(res[c, 0]), int(res[c, 1])) == (length, state), (tile, F._name("A", c))
        assert int(res[c, 5]) == 0, (tile, F._name("A", c), hex(int(res[c, 5])))


@pytest.mark.parametrize("tile", TILES)
def test_paths_and_tile_counts_are_the_models(runs, oracle_mod, tile):
    _, res = runs[tile]
    full_tiles = 0
    for c, (case, in_mis, out_mis, _) in enumerate(F._plan("A")):
        paths, n_fast, n_slow = F._predicted(case, in_mis, out_mis)
        got = (int(res[c, 2]), int(res[c, 3]), int(res[c, 4]))
        assert got == (paths, n_fast, n_slow), (tile, F._name("A", c), "kernel", D.path_names(got[0]), got[1:], "model", D.path_names(paths),
                                                (n_fast, n_slow))
        full_tiles += n_fast
    assert full_tiles >= 100          # the fast tile is what this launch is about


def test_vector_tile_gives_what_the_default_tile_gives(runs):
    (out_d, res_d), (out_v, res_v) = runs["default"], runs["vector"]
    for j, name in enumerate(F.OUTPUTS):
        bad = np.flatnonzero(res_d[:, j] != res_v[:, j])
        assert bad.size == 0, (name, F._name("A", int(bad[0])))
    assert np.array_equal(out_d, out_v)     # guards and gaps included


if __name__ == "__main__":
    import alice_codec_amd
    assert alice_codec_amd.device_count() >= 1
    alice_codec_amd.set_device(0)
    child_out, child_res = F._launch(alice_codec_amd.load_library(), "A")
    np.savez(sys.argv[1], out=child_out, res=child_res)
