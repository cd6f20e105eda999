"""Two independent restatements of the reference's person segmentation (src/segment.rs), written from reading it.

(a) `lit_*`: the reference's own loops -- the distance scans of dilate_mask_separable (:313-373), the complement trick of
    erode_mask_separable (:378-390), the row scan of compute_bbox_fast (:400-441), the run loop of rle_encode_mask
    (:131-154).  Python integers, so the radii never wrap.  Slow: small frames only.
(b) `vec_*`: numpy on a different formulation -- a box maximum over the window clipped to the frame, taken from cumulative
    sums along each axis (a pixel is set iff its clipped window holds a set pixel); erosion as a box minimum with pixels
    outside the frame counted as foreground; RLE from run boundaries.  Fast enough for 1920x1080x8.
"""
import numpy as np

U16_MAX = 65535


# ---------------------------------------------------------------------------------------------------------------------
# (a) literal
# ---------------------------------------------------------------------------------------------------------------------

def lit_dilate(mask, w, h, r):
    """dilate_mask_separable, :313-373"""
    temp = [0] * (w * h)
    for y in range(h):
        off = y * w
        dist = r + 1
        for x in range(w):
            if mask[off + x] != 0:
                dist = 0
            if dist <= r:
                temp[off + x] = 1
            dist += 1
        dist = r + 1
        for x in reversed(range(w)):
            if mask[off + x] != 0:
                dist = 0
            if dist <= r:
                temp[off + x] = 1
            dist += 1
    out = [0] * (w * h)
    for x in range(w):
        dist = r + 1
        for y in range(h):
            if temp[y * w + x] != 0:
                dist = 0
            if dist <= r:
                out[y * w + x] = 1
            dist += 1
        dist = r + 1
        for y in reversed(range(h)):
            if temp[y * w + x] != 0:
                dist = 0
            if dist <= r:
                out[y * w + x] = 1
            dist += 1
    return out


def lit_erode(mask, w, h, r):
    """erode_mask_separable, :378-390: complement, dilate, complement"""
    return [v ^ 1 for v in lit_dilate([v ^ 1 for v in mask], w, h, r)]


def lit_bbox(mask, w, h):
    """compute_bbox_fast, :400-441"""
    min_x, min_y, max_x, max_y, count = w, h, 0, 0, 0
    for y in range(h):
        row = mask[y * w:(y + 1) * w]
        rc = sum(row)
        if rc == 0:
            continue
        count += rc
        min_y = min(min_y, y)
        max_y = y
        first = row.index(1)
        last = w - 1 - row[::-1].index(1)
        min_x = min(min_x, first)
        max_x = max(max_x, last)
    if count == 0:
        return [0, 0, 0, 0], 0
    return [min_x, min_y, max_x - min_x + 1, max_y - min_y + 1], count


def lit_cleanup(mask, w, h, dilate, erode):
    """:213-218: dilate first, then erode; a radius of 0 skips its step"""
    if dilate > 0:
        mask = lit_dilate(mask, w, h, dilate)
    if erode > 0:
        mask = lit_erode(mask, w, h, erode)
    return mask


def lit_motion(cur, ref, w, h, threshold, dilate, erode):
    """segment_by_motion, :172-230 -> (mask list, bbox, count)"""
    total = w * h
    mask = [1 if abs(int(cur[i]) - int(ref[i])) > threshold else 0 for i in range(total)]
    mask = lit_cleanup(mask, w, h, dilate, erode)
    bbox, count = lit_bbox(mask, w, h)
    return mask, bbox, count


def lit_chroma(cg, w, h, green_threshold):
    """segment_by_chroma, :234-265"""
    mask = [1 if int(v) <= green_threshold else 0 for v in list(cg)[:w * h]]
    mask = lit_erode(lit_dilate(mask, w, h, 2), w, h, 1)
    bbox, count = lit_bbox(mask, w, h)
    return mask, bbox, count


def lit_rle(mask):
    """rle_encode_mask, :131-154"""
    out = bytearray()
    n, pos = len(mask), 0
    while pos < n:
        val = mask[pos] & 1
        start = pos
        while pos < n and (mask[pos] & 1) == val and (pos - start) < U16_MAX:
            pos += 1
        run = pos - start
        out += bytes([run & 0xFF, run >> 8, val])
    return bytes(out)


def lit_extract(mask, width, bbox, rgb):
    """extract_person_rgb, :107-125"""
    bx, by, bw, bh = bbox
    out = bytearray()
    for row in range(by, by + bh):
        for col in range(bx, bx + bw):
            mi = row * width + col
            if mi < len(mask) and mask[mi] == 1:
                ri = mi * 3
                if ri + 2 < len(rgb):
                    out += bytes(rgb[ri:ri + 3])
    return bytes(out)


def lit_crop(frame, frame_width, bbox):
    """crop_to_bbox, :269-281"""
    bx, by, bw, bh = bbox
    out = bytearray()
    for row in range(by, by + bh):
        start = row * frame_width + bx
        end = start + bw
        if end <= len(frame):
            out += bytes(frame[start:end])
    return bytes(out)


def lit_paste(frame, frame_width, person, bbox):
    """paste_from_bbox, :284-298 (returns a new bytearray)"""
    frame = bytearray(frame)
    bx, by, bw, bh = bbox
    src = 0
    for row in range(by, by + bh):
        d0 = row * frame_width + bx
        d1 = d0 + bw
        if d1 <= len(frame) and src + bw <= len(person):
            frame[d0:d1] = person[src:src + bw]
        src += bw
    return frame


# ---------------------------------------------------------------------------------------------------------------------
# (b) vectorised: clipped box windows from cumulative sums
# ---------------------------------------------------------------------------------------------------------------------

def _box_any(m, r, axis):
    """out[i] = any(m[max(0, i-r) .. min(n-1, i+r)]) along axis (m: bool array [..., h, w])"""
    n = m.shape[axis]
    if n == 0:
        return m.copy()
    c = np.cumsum(m, axis=axis, dtype=np.int64)
    zero_shape = list(m.shape)
    zero_shape[axis] = 1
    c = np.concatenate([np.zeros(zero_shape, np.int64), c], axis=axis)   # c[k] = sum of m[0 .. k-1]
    i = np.arange(n, dtype=np.int64)
    r = int(r)
    hi = np.minimum(i + r + 1, n) if r < n else np.full(n, n, np.int64)
    lo = np.maximum(i - r, 0) if r < n else np.zeros(n, np.int64)
    return (np.take(c, hi, axis=axis) - np.take(c, lo, axis=axis)) > 0


def vec_dilate(m, r):
    """box maximum of radius r, pixels outside the frame = 0 (m: bool [..., h, w])"""
    return _box_any(_box_any(m, r, -1), r, -2)


def vec_erode(m, r):
    """box minimum of radius r, pixels outside the frame = 1"""
    return ~vec_dilate(~m, r)


def vec_cleanup(m, dilate, erode):
    if dilate > 0:
        m = vec_dilate(m, dilate)
    if erode > 0:
        m = vec_erode(m, erode)
    return m


def vec_bbox(m):
    """m: bool [h, w] -> ([x, y, w, h], count)"""
    count = int(m.sum())
    if count == 0:
        return [0, 0, 0, 0], 0
    rows = np.flatnonzero(m.any(axis=1))
    cols = np.flatnonzero(m.any(axis=0))
    return [int(cols[0]), int(rows[0]), int(cols[-1] - cols[0] + 1), int(rows[-1] - rows[0] + 1)], count


def vec_stats(m):
    """m: bool [n, h, w] -> int64 [n, 5] = x, y, w, h, count per frame (vec_bbox without the loop over frames)"""
    m = np.asarray(m, bool)
    n, h, w = m.shape
    count = m.reshape(n, -1).sum(axis=1, dtype=np.int64)
    rows, cols = m.any(axis=2), m.any(axis=1)
    y0, y1 = rows.argmax(axis=1), h - 1 - rows[:, ::-1].argmax(axis=1)
    x0, x1 = cols.argmax(axis=1), w - 1 - cols[:, ::-1].argmax(axis=1)
    st = np.stack([x0, y0, x1 - x0 + 1, y1 - y0 + 1, count], axis=1).astype(np.int64)
    st[count == 0] = 0
    return st


def vec_motion_batch(cur, ref, threshold, dilate, erode):
    """vec_motion with vec_stats: for batches of many small frames"""
    m = np.abs(np.asarray(cur, np.int16) - np.asarray(ref, np.int16)) > int(threshold)
    m = vec_cleanup(m, dilate, erode)
    return m.astype(np.uint8), vec_stats(m)


def vec_motion(cur, ref, threshold, dilate, erode):
    """cur, ref: uint8 [f, h, w] (ref broadcastable) -> (mask uint8 [f, h, w], stats int64 [f, 5] = x, y, w, h, count)"""
    cur = np.asarray(cur, np.int16)
    ref = np.asarray(ref, np.int16)
    m = np.abs(cur - ref) > int(threshold)
    m = vec_cleanup(m, dilate, erode)
    stats = np.array([vec_bbox(fr)[0] + [vec_bbox(fr)[1]] for fr in m], np.int64).reshape(len(m), 5)
    return m.astype(np.uint8), stats


def vec_cg_of_rgb(rgb):
    """Cg of interleaved RGB (src/color.rs:225-228): rgb uint8 [..., 3] -> int16"""
    r, g, b = (rgb[..., k].astype(np.int32) for k in range(3))
    co = r - b
    t = b + (co >> 1)
    return (g - t).astype(np.int16)


def vec_chroma(cg, green_threshold):
    """cg: int16 [f, h, w] -> (mask uint8, stats [f, 5])"""
    m = np.asarray(cg, np.int16) <= int(green_threshold)
    m = vec_erode(vec_dilate(m, 2), 1)
    stats = np.array([vec_bbox(fr)[0] + [vec_bbox(fr)[1]] for fr in m], np.int64).reshape(len(m), 5)
    return m.astype(np.uint8), stats


def vec_rle(mask):
    m = np.asarray(mask, np.uint8).reshape(-1) & 1
    n = m.size
    if n == 0:
        return b""
    starts = np.concatenate([[0], np.flatnonzero(m[1:] != m[:-1]) + 1])
    lens = np.diff(np.concatenate([starts, [n]]))
    pieces = (lens + U16_MAX - 1) // U16_MAX
    run_of_piece = np.repeat(np.arange(starts.size), pieces)
    first_piece = np.repeat(np.cumsum(pieces) - pieces, pieces)
    k = np.arange(run_of_piece.size) - first_piece
    plen = np.minimum(U16_MAX, lens[run_of_piece] - k * U16_MAX)
    out = np.empty((plen.size, 3), np.uint8)
    out[:, 0] = plen & 0xFF
    out[:, 1] = plen >> 8
    out[:, 2] = m[starts[run_of_piece]]
    return out.tobytes()


def _u8(a):
    if isinstance(a, (bytes, bytearray)):
        return np.frombuffer(bytes(a), np.uint8)
    return np.asarray(a, np.uint8).reshape(-1)


def vec_extract(mask, width, bbox, rgb):
    mask, rgb = _u8(mask), _u8(rgb)
    bx, by, bw, bh = (int(v) for v in bbox)
    rows = np.arange(by, by + bh, dtype=np.int64)
    cols = np.arange(bx, bx + bw, dtype=np.int64)
    mi = (rows[:, None] * int(width) + cols[None, :]).reshape(-1)
    ok = mi < mask.size
    ok[ok] = mask[mi[ok]] == 1
    ok &= mi * 3 + 2 < rgb.size
    sel = mi[ok]
    return rgb[(sel[:, None] * 3 + np.arange(3)[None, :]).reshape(-1)].tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# (c) the launch geometry of csrc/segment.hip, restated from its conditions
# ---------------------------------------------------------------------------------------------------------------------

GRID_CAP = 1 << 20   # grid_cap, segment.hip:328

# every class a case table has to reach; the text before " @" is the key of segment_geometry that reports it
ALL_CLASSES = frozenset([
    "chunks_per_row=1", "chunks_per_row>1", "row_of_64_words",
    "block<64", "block>64", "block==64", "block==h-1", "block==h", "block>h clamped",   # (64 only through the clamp: 2r+1 is odd)
    "block_starts_on_lane0", "block_starts_on_lane63", "block_ends_on_lane0",
    "pick=0", "pick=1", "pick=2",
    "last_step_partial", "last_step_full",
    "smear<63", "smear>=63",
    "row_grid_loops", "row_grid_loops_with_partial_group", "column_grid_loops"])


def segment_geometry(w, h, n_frames, dilate, erode):
    """What one segmentation call of w x h x n_frames with these radii reaches in csrc/segment.hip.  Keys are
    "<name> @<line of segment.hip>"; `geometry_classes` flattens the result into members of ALL_CLASSES."""
    w, h, n, radii = int(w), int(h), int(n_frames), [int(r) for r in (dilate, erode) if int(r)]
    W64 = (w + 63) // 64
    nch = (W64 + 63) // 64
    g = {
        "words_per_row @133": W64,
        "chunks_per_row @133": nch,
        # a radius takes :215 (one chunk) or :220 (two sweeps with ncarry); the final stage always takes :213
        "row_path @213-220": ({"one_chunk" if nch == 1 else "many_chunks"} if radii else set()) | {"plain"},
        "row_of_64_words @215": bool(radii) and W64 == 64,
        "smear @90": {">=63" if r >= 63 else "<63" for r in radii},
        "block @505": {}, "pick @146": set(),
        "block_starts_on_lane0 @292": False, "block_starts_on_lane63 @294": False, "block_ends_on_lane0 @308": False,
        "last_step_partial @286": None if not radii else h % 64 != 0,
        "row_grid_loops @135": ((h + 3) // 4) * n > GRID_CAP,
        "row_group_partial @138": h % 4 != 0,
        "column_grid_loops @281": bool(radii) and (n * W64 + 3) // 4 > GRID_CAP,
    }
    for r in radii:
        full = 2 * r + 1
        B = full if full < h else h                                    # :505
        cls = {"<64" if B < 64 else ("==64" if B == 64 else ">64")}   # block_of, :110
        if full > h:
            cls.add("clamped")
        if full == h:
            cls.add("==h")
        if full == h - 1:
            cls.add("==h-1")
        g["block @505"][r] = (B, cls)
        for y0 in range(B, h, B):                                      # first row of every block but the first
            g["block_starts_on_lane0 @292"] |= y0 % 64 == 0             # the carry of the step before must be dropped
            g["block_starts_on_lane63 @294"] |= y0 % 64 == 63           # the carry out is a block of one row
            g["block_ends_on_lane0 @308"] |= y0 % 64 == 1               # the same for the reverse pass
        for y in range(h):                                             # :144-146
            lo = y - r if y > r else 0
            hi = y + r if h - 1 - y > r else h - 1
            g["pick @146"].add(0 if lo // B != hi // B else (1 if lo % B == 0 else 2))
    return g


def geometry_classes(g):
    """the members of ALL_CLASSES that a segment_geometry result holds"""
    out = {"chunks_per_row=1" if g["chunks_per_row @133"] == 1 else "chunks_per_row>1"}
    if g["row_of_64_words @215"]:
        out.add("row_of_64_words")
    out |= {"smear" + s for s in g["smear @90"]}
    for B, cls in g["block @505"].values():
        for c in cls:
            out.add({"clamped": "block>h clamped"}.get(c, "block" + c))
    for k in ("block_starts_on_lane0 @292", "block_starts_on_lane63 @294", "block_ends_on_lane0 @308", "row_grid_loops @135",
              "column_grid_loops @281"):
        if g[k]:
            out.add(k.split(" @")[0])
    if g["row_grid_loops @135"] and g["row_group_partial @138"]:
        out.add("row_grid_loops_with_partial_group")
    out |= {"pick=%d" % p for p in g["pick @146"]}
    if g["last_step_partial @286"] is not None:
        out.add("last_step_partial" if g["last_step_partial @286"] else "last_step_full")
    return out
