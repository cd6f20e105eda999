"""Frequency tables for the rANS fuzz tests (decoder and encoder) that no histogram produces."""
import numpy as np


def custom_oracle_table(oracle_mod, cum, freq):
    """The oracle's table struct filled by hand the way FrequencyTable::from_histogram fills cum_to_sym
    (src/rans.rs:135-144: zeroed, then symbol by symbol over [cum, min(cum + freq, 4096)), later symbols overwrite)."""
    t = oracle_mod.FrequencyTable(np.ones(256, np.uint32))
    c2s = np.zeros(4096, np.uint8)
    for s in range(256):
        t._t.cum_freq[s] = int(cum[s])
        t._t.freq[s] = int(freq[s])
        lo, hi = int(cum[s]), min(int(cum[s]) + int(freq[s]), 4096)
        if lo < hi:
            c2s[lo:hi] = s
    for k in range(4096):
        t._t.cum_to_sym[k] = int(c2s[k])
    return t
