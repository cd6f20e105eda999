"""The size tables of tests/test_gpu_generic_geometry.py, apart from it so that tests/test_generic_cases_host.py can hold them
to the launch caps of csrc/generic.hip and csrc/rate.hip without a GPU.

Every kernel of the family is a grid-stride loop under a host-side cap on the grid, so what a size exercises is the number of
trips the loop takes and whether the last one is full.  A table is a list of (items, items_per_trip) pairs, one per launch;
trip_classes() names what it reaches and REQUIRED is what every table must reach.

The caps, restated from the launch code:
* grid_for(): one workgroup per 256 items, at most 65535 * 4 workgroups -- or the test hook's cap (1 and 3 here);
* launch_histogram / _wide, launch_sq_diff_sum, launch_sum_i32: grid_for() clamped to 2048 workgroups;
* launch_coef_hist: at most 1024 workgroups;
* the region colour kernels: one workgroup per row, at most 65536, and 256 threads across the row."""

DEFAULT_CAP = 65535 * 4
HOOK_CAPS = (1, 3)
REDUCE_TRIP = 2048 * 256          # items per trip of the launches clamped to 2048 workgroups
HIST_VEC = 16                     # bytes per item of histogram_kernel's vector loop
COEF_TRIP = 1024 * 256
REGION_ROWS = 65536
REGION_X = 256

REQUIRED = {"one_partial", "one_full", "two_full", "partial_last"}


def per_trip(cap: int) -> int:
    return (cap or DEFAULT_CAP) * 256


def trips(items: int, items_per_trip: int) -> int:
    """trips of a grid-stride loop over `items` whose grid covers `items_per_trip` of them at a time"""
    return -(-items // items_per_trip)


def trip_classes(pairs) -> set:
    out = set()
    for items, ipt in pairs:
        full, rest = divmod(items, ipt)
        if full == 0 and rest:
            out.add("one_partial")
        if rest == 0 and full in (1, 2):
            out.add("one_full" if full == 1 else "two_full")
        if full >= 1 and rest:
            out.add("partial_last")
    return out


# ---- element-wise kernels under the hook ----

def elementwise_sizes(cap: int) -> list:
    t = cap * 256
    return sorted({t - 1, t, t + 1, 2 * t, 2 * t + 77, 5000})


def elementwise_pairs():
    return [(n, per_trip(c)) for c in HOOK_CAPS for n in elementwise_sizes(c)]


# ---- launch_wavelet_axis under the hook ----
# Shapes the tile kernels do not take (an odd side, or a side below 6; every 1-D signal).  The lift kernels run n / 2 items per
# line and the shuffle / copy kernels n; a line along the fastest axis is walked along the line (line_fast = 0), any other
# across the lines (line_fast = 1).  Chosen so that at 256 and at 768 items per trip both kinds of launch, in both orderings,
# need one trip, exactly one, exactly two, and two-and-a-bit.
WAVELET_1D = [2, 3, 255, 256, 512, 513, 600, 768, 1024, 1100, 1536, 1700, 3072, 3300]
WAVELET_2D = [(4, 2), (5, 3), (5, 103), (4, 64), (4, 128), (4, 150), (4, 192), (4, 256), (4, 300), (4, 384), (4, 450), (4, 768),
              (4, 900), (3, 171)]
WAVELET_3D = [(5, 3, 7), (3, 40, 4), (4, 4, 40), (7, 9, 11), (2, 2, 130), (6, 4, 3)]


def wavelet_shapes():
    return [(n,) for n in WAVELET_1D] + WAVELET_2D + WAVELET_3D


def tile_eligible(shape) -> bool:
    """stage_tiles_eligible of csrc/transform.hip for the sizes used here"""
    if len(shape) < 2:
        return False
    w, h = shape[0], shape[1]
    d = shape[2] if len(shape) > 2 else 1
    if w % 2 or h % 2 or w < 6 or h < 6:
        return False
    return not (len(shape) == 3 and d > 1 and d % 2)


def axis_launches(shape) -> list:
    """(n, lines, line_fast) of each launch_wavelet_axis call of a forward or inverse transform of this shape"""
    dims = list(shape) + [1] * (3 - len(shape))
    w, h, d = dims
    out = [(w, h * d, 0)]
    if len(shape) >= 2:
        out.append((h, w * d, 1))
    if len(shape) >= 3:
        out.append((d, w * h, 1))
    return [a for a in out if a[0] >= 2]       # a line of one element is left alone


def wavelet_pairs(kind: str, line_fast: int):
    """kind: 'lift' (n / 2 items per line) or 'shuffle' (n items per line; the copy launch has the same grid)"""
    out = []
    for cap in HOOK_CAPS:
        for shape in wavelet_shapes():
            for n, lines, lf in axis_launches(shape):
                if lf == line_fast:
                    out.append(((n // 2 if kind == "lift" else n) * lines, per_trip(cap)))
    return out


# ---- pad / strip and the whole generic pipeline under the hook ----
# (w, h, f): a padded side below 6 or more than 64 frames.  The first four are odd in one way each; the others make the padded
# volume (and, all sides being even, the pixel count) exactly one and two trips at 256 and at 768 items.
PIPELINE_SHAPES = [(5, 3, 7), (3, 40, 4), (20, 12, 66), (1, 300, 4), (4, 4, 16), (4, 4, 32), (4, 4, 48), (4, 4, 96)]


def padded_dims(w, h, f):
    return w + (w & 1), h + (h & 1), 2 if f == 1 else f + (f & 1)


def pipeline_pairs(kind: str):
    out = []
    for cap in HOOK_CAPS:
        for (w, h, f) in PIPELINE_SHAPES:
            pw, ph, pf = padded_dims(w, h, f)
            out.append((pw * ph * pf if kind == "pad" else w * h * f, per_trip(cap)))
    return out


# ---- ssim / ms_ssim under the hook: (width, height, caps) ----
SSIM_CASES = [(256, 256, (3, 1, 0)), (250, 131, (3, 1, 0)), (64, 64, (1, 0)),
              # blocks: exactly two trips at cap 1, exactly one and two at cap 3 (256 x 256 at cap 1 has a half scale of one)
              (128, 256, (1,)), (256, 192, (3,)), (256, 384, (3,)),
              # half-scale pixels: exactly one and two trips at cap 1 and at cap 3
              (32, 32, (1,)), (64, 32, (1,)), (64, 48, (3,)), (64, 96, (3, 0))]


def ssim_pairs(kind: str):
    """kind: 'blocks' (8 x 8 blocks of every scale ms_ssim visits) or 'downsample' (pixels of every half-scale image)"""
    out = []
    for w, h, caps in SSIM_CASES:
        for cap in caps:
            if not cap:
                continue
            cw, ch = w, h
            for _ in range(3):
                if kind == "blocks" and (cw // 8) * (ch // 8):
                    out.append(((cw // 8) * (ch // 8), per_trip(cap)))
                cw, ch = cw // 2, ch // 2
                if cw < 8 or ch < 8:
                    break
                if kind == "downsample":
                    out.append((cw * ch, per_trip(cap)))
    return out


# ---- the real caps ----
HIST_SMALL = sorted({16 * k + d for k in (0, 1, 2, 3, 17) for d in (-1, 0, 1) if 16 * k + d >= 0})
HIST_SIZES = HIST_SMALL + [100_000, REDUCE_TRIP, 2 * REDUCE_TRIP, HIST_VEC * REDUCE_TRIP, HIST_VEC * REDUCE_TRIP + 16 * 300 + 5,
                           2 * HIST_VEC * REDUCE_TRIP]
HIST_OFFSETS = [0, 1, 4, 15]      # bytes into a 16-byte aligned allocation: only 0 takes the vector loop
HIST_BIG = 9_000_000              # sizes above this (the two full trips of the vector loop, 16 MiB) run at offsets 0 and 1 only
HIST_ALL_CONTENTS = 1_000_000     # sizes above this run on the random and the one-non-zero-byte content only


def hist_offsets(n: int) -> list:
    return HIST_OFFSETS if n <= HIST_BIG else [0, 1]


def hist_pairs(kind: str):
    """kind: 'vector' (16-byte items of an aligned pointer) or 'scalar' (the bytes of an unaligned one)"""
    out = []
    for n in HIST_SIZES:
        for off in hist_offsets(n):
            if kind == "vector" and off == 0 and n // HIST_VEC:
                out.append((n // HIST_VEC, REDUCE_TRIP))
            if kind == "scalar" and off != 0 and n:
                out.append((n, REDUCE_TRIP))
    return out


WIDE_HIST_SIZES = [1000, REDUCE_TRIP, REDUCE_TRIP + 1, 600_001, 2 * REDUCE_TRIP]
PSNR_SIZES = [100_003, REDUCE_TRIP - 1, REDUCE_TRIP, REDUCE_TRIP + 1, 600_001, 2 * REDUCE_TRIP]
RDO_SIZES = [1000, REDUCE_TRIP, REDUCE_TRIP + 1, 600_001, 2 * REDUCE_TRIP]

# generic-path chunks (w, h, f) for the size prediction and the region calls: padded volumes of one partial, one full, one
# full and a bit, and two full trips of coef_hist_kernel; h * f rows of the same classes for the region kernels
RATE_SHAPES = [(4, 4, 2), (4, 1024, 64), (4, 1100, 64), (4, 2048, 64)]
RATE_FULL = (4, 1100, 64)         # the shape that gets all three containers and the shrunk value table

# (frame width, frame height, w, h, f, origins): rows above 65536, and widths above 256
REGION_CASES = [
    (9, 1103, 4, 1100, 64, [(4, 3), (1, 0)]),
    (9, 1024, 4, 1024, 64, [(5, 0)]),
    (9, 2050, 4, 2048, 64, [(0, 2)]),
    (320, 10, 300, 4, 3, [(0, 0), (1, 6), (20, 3), (17, 1)]),
    (320, 10, 256, 4, 3, [(4, 5), (61, 0)]),
    (530, 7, 512, 4, 3, [(8, 3), (17, 0)]),
    (40, 30, 37, 4, 3, [(3, 26)]),
]


def rate_pairs():
    out = []
    for (w, h, f) in RATE_SHAPES:
        pw, ph, pf = padded_dims(w, h, f)
        out.append((pw * ph * pf, COEF_TRIP))
    return out


def region_pairs(kind: str):
    return [(h * f if kind == "rows" else w, REGION_ROWS if kind == "rows" else REGION_X) for (_, _, w, h, f, _) in REGION_CASES]


def families() -> dict:
    """name -> (items, items_per_trip) pairs of every launch the GPU file makes for that family"""
    return {
        "elementwise": elementwise_pairs(),
        "axis_lift_along": wavelet_pairs("lift", 0), "axis_lift_across": wavelet_pairs("lift", 1),
        "axis_shuffle_along": wavelet_pairs("shuffle", 0), "axis_shuffle_across": wavelet_pairs("shuffle", 1),
        "pad_channel": pipeline_pairs("pad"), "strip_channel": pipeline_pairs("strip"),
        "ssim_blocks": ssim_pairs("blocks"), "downsample2": ssim_pairs("downsample"),
        "histogram_vector": hist_pairs("vector"), "histogram_scalar": hist_pairs("scalar"),
        "histogram_wide": [(n, REDUCE_TRIP) for n in WIDE_HIST_SIZES],
        "sq_diff_sum": [(n, REDUCE_TRIP) for n in PSNR_SIZES],
        "sum_i32": [(n, REDUCE_TRIP) for n in RDO_SIZES],
        "coef_hist": rate_pairs(),
        "region_rows": region_pairs("rows"), "region_x": region_pairs("x"),
    }
