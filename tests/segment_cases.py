"""The case tables and pattern builders of tests/test_gpu_segment_geometry.py, apart from it so that
tests/test_segment_host.py can hold the tables to the classes of segment_ref.segment_geometry, and the patterns to the
literal restatement, without a GPU.

Patterns are bool arrays of the pixels over threshold *before* the cleanup.  An erosion is given the complement of a
pattern (a single hole instead of a single pixel), so its result shows the clipped window as exactly as a dilation's."""
import numpy as np

BIG = 2 ** 32 - 1

# ---- (a) column geometry: 64-row steps, blocks of B = min(2r+1, h) rows, the carry between steps ----

COLUMN_HEIGHTS = [3, 5, 63, 64, 65, 127, 128, 129, 191, 257]
COLUMN_WIDTHS = [1, 65]
_COLUMN_RADII = [1, 2, 8, 15, 31, 32, 33, 63, 64, 95, 127, 128]


def column_radii(h):
    return sorted({r for r in _COLUMN_RADII + [(h - 1) // 2, (h - 1) // 2 + 1, h - 2, h - 1, h, BIG] if r >= 1})


def pixel_rows(h, r):
    """rows of the single set pixel: the frame's edges, the step edge, and the rows whose window just reaches an edge"""
    return sorted({y for y in (0, r, r + 1, 63, 64, h - 1 - r, h - 1) if 0 <= y < h})


def column_cases(h):
    """-> dicts: w, h, n (frames), rd, re, mode, row (of the single pixel), shared (reference stride 0), stats_only"""
    cases = []
    radii = column_radii(h)
    for w in COLUMN_WIDTHS:
        for i, r in enumerate(radii):
            other = radii[(i + 1) % len(radii)]
            for mode, rd, re in (("dilate", r, 0), ("erode", 0, r), ("both", r, other)):
                for j, row in enumerate(pixel_rows(h, r)):
                    k = len(cases)
                    cases.append(dict(w=w, h=h, n=2 if k % 3 == 2 else 3, rd=rd, re=re, mode=mode, row=row, shared=j % 2 == 0,
                                      stats_only=k % 3 == 0))
    return cases


def column_pattern(case, rng):
    """bool [n, h, w]: one set pixel; a frame at 0.5 % density; with three frames, one at 50 % in between"""
    w, h, n = case["w"], case["h"], case["n"]
    m = np.zeros((n, h, w), bool)
    m[0, case["row"], (case["row"] * 7 + case["rd"] + case["re"]) % w] = True
    m[n - 1] = rng.random((h, w)) < 0.005
    if n == 3:
        m[1] = rng.random((h, w)) < 0.5
    # an erosion alone sees the complement; dilate-then-erode takes the pattern and its complement in turn
    if case["mode"] == "erode" or (case["mode"] == "both" and case["row"] % 2 == 1):
        m = ~m
    return m


# ---- (b) row geometry: words of 64 pixels, chunks of 64 words ----

ROW_HEIGHTS = [2, 5]
ROW_WIDTHS = [4032, 4033, 4095, 4096, 4097, 8191, 8192, 8193]
ROW_RADII = [1, 62, 63, 64, 65, 4031, 4096, BIG]


def row_positions(w):
    return sorted({p for p in (0, 63, 64, 4095, 4096, 8191, w - 1) if p < w})


def row_pairs(w, r):
    """(p, q), p < q, on the two sides of a chunk edge (a word edge where the row has one chunk), q - p = r-1, r, r+1"""
    edges = [e for e in (4096, 8192) if e < w] or [64, 4032]
    out = []
    for e in edges:
        for d in (r - 1, r, r + 1):
            q = e + d // 2
            p = q - d
            if d >= 1 and 0 <= p < e <= q < w:
                out.append((p, q))
    return out


def row_pattern(w, h, r):
    """bool [n, h, w]: frame f holds one pattern on row f % h and nothing else, the last frame nothing at all"""
    rows = [[p] for p in row_positions(w)] + [list(pq) for pq in row_pairs(w, r)] + [[]]
    m = np.zeros((len(rows), h, w), bool)
    for f, xs in enumerate(rows):
        m[f, f % h, xs] = True
    return m


def row_cases(w):
    """-> dicts: w, h, n, rd, re, mode"""
    cases = []
    for h in ROW_HEIGHTS:
        for r in ROW_RADII:
            n = len(row_positions(w)) + len(row_pairs(w, r)) + 1
            cases.append(dict(w=w, h=h, n=n, rd=r, re=0, mode="dilate"))
            cases.append(dict(w=w, h=h, n=n, rd=0, re=r, mode="erode"))
    return cases


# ---- (c) grids past the cap of 2^20 workgroups: the loop bodies run a second time ----

GRID_SHAPES = [(1, 1, 4_300_000), (5, 6, 530_000)]
GRID_RADII = [(1, 1), (0, 0)]


def grid_cases():
    return [dict(w=w, h=h, n=n, rd=rd, re=re) for (w, h, n) in GRID_SHAPES for (rd, re) in GRID_RADII]


def all_segment_calls():
    """every (w, h, n_frames, dilate, erode) of (a), (b) and (c)"""
    calls = [c for h in COLUMN_HEIGHTS for c in column_cases(h)] + [c for w in ROW_WIDTHS for c in row_cases(w)] + grid_cases()
    return [(c["w"], c["h"], c["n"], c["rd"], c["re"]) for c in calls]


def reached_classes(calls):
    import segment_ref as R
    out = set()
    for key in set(calls):
        out |= R.geometry_classes(R.segment_geometry(*key))
    return out
