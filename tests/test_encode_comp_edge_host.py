"""The block edge of a run of complement blocks in the rANS encode chain (alice-codec_amd/csrc/rans.hip, ripple64_comp_run),
modelled by hand in 32-bit wrap-around arithmetic: the statement's instruction list is macro text, not data, so the functions
below restate it and name the macro lines they mirror.

  ALICE_RUN_REST, the four fillers behind the s_waitcnt (block b prepares block b + 1):
      v_mov_b32_dpp ccp, cc  wave_ror:1      lane 0 <- C[63] of block b
      v_mov_b32_dpp ccp, C'  wave_shr:1      lanes 1..63 <- C'[lane - 1]; lane 0 keeps what it has
      v_add_u32     tm1', -1, xmax'          T' - 1
      v_sub_u32     kc', tm1', ccp
  ALICE_RUN_NEXT, step 0 (the edge):  v_add_u32_dpp u', z, kc' wave_ror:1     lane 0 <- z[63] + kc'[0]
  ALICE_RUN_NEXT, steps 0..5 (block b - 1's byte): sign of its u into VCC, ~u, mbcnt on tw, span1 - off, tw += popcount

The edge is compared with the reference step (src/rans.rs:269-284) for every incoming frequency of the big class, and a
three-block run of the model with the oracle encoder's states and bytes.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_encode_comp_step_host import (L, X_END, _pushed, comp_step, entries, reference_step, sext, u32,  # noqa: E402
                                        v_add_u32, v_sub_u32)

MINUS_1 = np.uint64(0xFFFFFFFF)


def wave_ror1(src):
    return np.roll(src, 1)


def wave_shr1(old, src):
    """bound_ctrl off: lane 0 has no source lane and keeps the destination's old value"""
    out = np.array(old, np.uint64)
    out[1:] = src[:-1]
    return out


def next_kc(cur_c, nxt):
    """the four ALICE_RUN_REST fillers: kc of block b + 1, lane 0 against block b's last lane"""
    ccp = wave_ror1(cur_c)
    ccp = wave_shr1(ccp, nxt["C"])
    tm1 = v_add_u32(nxt["T"], MINUS_1)
    return v_sub_u32(tm1, ccp)


def test_edge_instruction_for_every_incoming_frequency():
    """z[63] + kc'[0] = T'[0] - 1 - x' (mod 2^32), x' the reference's state after block b's last symbol"""
    rng = np.random.default_rng(20261020)
    f = np.arange(17, 4097, dtype=np.int64)[:, None]
    t = f << 19
    edges = [t - 1, t, t + 1, np.full_like(t, (1 << 31) - 1), np.full_like(t, 1 << 31), np.full_like(t, L),
             np.full_like(t, X_END - 1)]
    x = np.concatenate(edges + [rng.integers(L, X_END, (len(f), 300))], axis=1)
    assert ((x >= L) & (x < X_END)).all()
    cum = rng.integers(0, 4097 - f, x.shape)
    cum[:, 0], cum[:, 1] = 0, (4096 - f)[:, 0]
    e = entries(np.broadcast_to(f, x.shape), cum)
    _, _, z = comp_step(v_sub_u32(e["tm1"], x), e)                 # lane 63 of block b: its u is T - 1 - x
    want, _, _ = reference_step(x, f, cum)
    assert ((want >= L) & (want < X_END)).all()
    out_f = np.concatenate([[17, 18, 4095, 4096], rng.integers(17, 4097, 300)])
    # (native uint32 arrays from here on: their sums and differences wrap as v_add_u32 / v_sub_u32 do)
    z32, c32, want32 = z.astype(np.uint32), e["C"].astype(np.uint32), want.astype(np.uint32)
    for fo in out_f:
        t_o = int(fo) << 19
        tm1_o = np.uint32(t_o - 1)                                 # v_add_u32 tm1', -1, xmax'
        kc0 = tm1_o - c32                                          # v_sub_u32 kc', tm1', ccp with ccp[0] = C[63]
        u_next = z32 + kc0                                         # v_add_u32_dpp ... wave_ror:1, lane 0
        assert np.array_equal(u_next, tm1_o - want32), int(fo)
        # ... which is what the first step of block b + 1 takes as its complement: it wraps exactly when x' >= T'
        assert np.array_equal(u_next.view(np.int32) < 0, want >= t_o), int(fo)


def run_of_blocks(x0, blocks):
    """ripple64_comp_run on a list of blocks' table entries (64 lanes each): -> per block (u, z), the bytes in the order
    the tile's byte counter places them, the plain state after the run"""
    rng = np.random.default_rng(9)
    u = rng.integers(0, 1 << 32, 64, dtype=np.uint64)             # registers hold anything on entry
    z = rng.integers(0, 1 << 32, 64, dtype=np.uint64)
    tile_bytes, tw, per_block = {}, 0, []

    def emit(up):                                                  # ALICE_RUN_NEXT steps 0..5, and the caller's last block
        nonlocal tw
        vcc = sext(up, 32) < 0                                     # v_cmp_gt_i32 vcc, 0, up
        byt = ~up & np.uint64(0xFF)                                # v_not_b32 (the store takes the low byte)
        off = tw + np.cumsum(vcc) - vcc                            # mbcnt_lo / mbcnt_hi on tw
        for lane in np.flatnonzero(vcc):                           # span1 - off: byte i of the tile at base[span - 1 - i]
            assert int(off[lane]) not in tile_bytes
            tile_bytes[int(off[lane])] = int(byt[lane])
        tw += int(vcc.sum())                                       # s_bcnt1 + v_add_u32 tw

    e = blocks[0]
    kc = v_sub_u32(e["tm1"], np.roll(e["C"], 1))                   # kc_of in the kernel; lane 0's is never used
    u[0] = v_sub_u32(e["tm1"][0], x0)                              # the first block enters with the plain state
    for b, e in enumerate(blocks):
        if b:
            kc = next_kc(blocks[b - 1]["C"], e)
            up = u.copy()
            u = v_add_u32(wave_ror1(z), kc)                        # step 0: every lane written, lane 0's is the edge
            _, _, z = comp_step(u, e, one_mad=True)
            steps = 63
        else:
            steps = 64
        for step in range(steps):
            u[1:] = v_add_u32(z[:-1], kc[1:])                      # wave_shr:1
            _, _, z = comp_step(u, e, one_mad=True)
            if b and step == 4:
                emit(up)                                           # the saved u is not touched by the chain
        per_block.append((u.copy(), z.copy()))
    emit(u)
    x_after = int(v_sub_u32(blocks[-1]["C"][63], z[63]))
    return per_block, bytes(tile_bytes[i] for i in range(tw)), x_after


@pytest.mark.parametrize("seed", range(6))
def test_run_of_three_blocks_against_the_oracle(oracle_mod, seed):
    o = oracle_mod
    rng = np.random.default_rng(200 + seed)
    hist = np.zeros(256, np.uint32)
    if seed % 2:                                                   # the extremes 17 and 4079
        hist[[3, 250]] = [4079, 17]
    else:
        hist[rng.choice(256, 30, replace=False)] = rng.integers(20, 200, 30)
    table = o.FrequencyTable(hist)
    freq, cum = table.freq.astype(np.int64), table.cum_freq.astype(np.int64)
    alphabet = np.flatnonzero((freq >= 17) & (freq <= 4096))
    assert len(alphabet) >= 2
    p = freq[alphabet] / freq[alphabet].sum()
    prefix = rng.choice(alphabet, int(rng.integers(0, 300)), p=p)
    run = rng.choice(alphabet, 192, p=p)
    if seed == 1:
        run[63], run[64], run[127], run[128] = 250, 250, 3, 250    # both frequencies on either side of an edge
    enc = o.RansEncoder()
    for s in prefix:
        enc.encode(int(cum[s]), int(freq[s]))
    x0, states = enc.state, []
    for s in run:
        enc.encode(int(cum[s]), int(freq[s]))
        states.append(enc.state)
    assert L <= x0 < X_END
    blocks = [entries(freq[run[i: i + 64]], cum[run[i: i + 64]]) for i in (0, 64, 128)]
    per_block, got_bytes, x_after = run_of_blocks(x0, blocks)
    before = np.concatenate([[x0], states[:-1]]).astype(np.uint64)
    for b, (e, (u, z)) in enumerate(zip(blocks, per_block)):
        assert np.array_equal(v_sub_u32(e["C"], z), np.array(states[64 * b: 64 * b + 64], np.uint64)), b
        assert np.array_equal(v_sub_u32(e["tm1"], u), before[64 * b: 64 * b + 64]), b
    assert x_after == states[-1]
    n_before = len(_pushed(o, prefix, cum, freq))
    assert got_bytes == _pushed(o, np.concatenate([prefix, run]), cum, freq)[n_before:]
