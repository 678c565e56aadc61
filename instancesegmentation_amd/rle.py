"""COCO run-length encoding of binary masks (numpy only: no torch, no GPU).

This module is the CPU statement of the contracts that csrc/mask_rle.hip (`encode`),
csrc/mask_rle_decode.hip (`decode_canvas`) and csrc/mask_rle_string.hip (`compress`,
`summarize`, `parse_total`) implement, and the codec between the kernels' `counts` and the
strings COCO tools read.

Binarisation: a pixel is set when mask >= 128 (the threshold of the mask-NMS).
Counts: the binarised H x W mask flattened column-major (pixel (x, y) at position
x*H + y); `counts` are the lengths of the alternating runs, the first always of zeros
(counts[0] == 0 when pixel 0 is set). An all-zero mask is [H*W], a full one [0, H*W].
String: the `counts` field of a compressed COCO RLE: count i (for i > 2 its difference
to count i-2, signed) in groups of five bits, least significant first, bit 0x20 flagging
that more groups follow, each group offset by 48 into printable ASCII.
"""
import glob
import json
import os

import numpy as np

THRESHOLD = 128


def encode(mask):
    """uint32 counts of a [H,W] mask (uint8: set where >= 128; bool: as is)."""
    m = np.asarray(mask)
    if m.ndim != 2:
        raise ValueError(f"mask must be [H,W], got shape {m.shape}")
    if m.size >= 2 ** 31:
        raise ValueError("H*W must be below 2^31")
    bits = (m if m.dtype == np.bool_ else m >= THRESHOLD).T.reshape(-1)  # column-major
    # positions whose bit differs from the predecessor's (a virtual zero before position 0)
    t = np.flatnonzero(np.diff(np.concatenate([[False], bits]).astype(np.int8)))
    return np.diff(np.concatenate([[0], t, [bits.size]])).astype(np.uint32)


def decode(counts, H, W):
    """bool [H,W] mask of `counts`."""
    c = np.asarray(counts, np.int64).reshape(-1)
    if c.sum() != H * W:
        raise ValueError(f"counts sum to {int(c.sum())}, not H*W = {H * W}")
    vals = (np.arange(len(c)) & 1).astype(bool)
    return np.repeat(vals, c).reshape(W, H).T.copy()


def decode_canvas(counts, H, W):
    """(uint8 [H,W] canvas of 0 / 255, total) of `counts`: the CPU statement of the contract
    csrc/mask_rle_decode.hip implements. Total, where `decode` is strict: with ends =
    cumsum(counts), position p = x*H + y belongs to run i = the number of ends <= p (so
    zero-length runs are stepped over) and is 255 when i is odd and i < len(counts).
    Positions at or past the sum are background, runs past H*W are ignored; `total` is the
    unclipped sum (the mask is well-formed when total == H*W). Empty counts: all zero, 0."""
    c = np.asarray(counts).reshape(-1)
    if c.size and (c.dtype.kind not in "iu" or c.min() < 0 or c.max() >= 2 ** 32):
        raise ValueError("counts must be integers in [0, 2^32)")
    ends = np.cumsum(c.astype(np.int64))
    i = np.searchsorted(ends, np.arange(H * W, dtype=np.int64), side="right")
    bits = ((i & 1) == 1) & (i < len(c))
    canvas = np.ascontiguousarray(bits.reshape(W, H).T).astype(np.uint8) * np.uint8(255)
    return canvas, int(ends[-1]) if len(c) else 0


def to_string(counts):
    """The ASCII `counts` field of a compressed COCO RLE."""
    x = np.array(counts, dtype=np.int64).reshape(-1)
    x[3:] -= x[1:-2].copy()  # count i > 2 as its (signed) difference to count i - 2
    # groups of five bits, least significant first; a value takes the fewest groups n whose
    # 5n bits hold it as a signed number (the decoder sign-extends from the last group)
    k = np.arange(7)
    half = np.int64(1) << (5 * k[1:] - 1)
    n = 7 - ((x[:, None] >= -half) & (x[:, None] < half)).sum(1)
    g = (x[:, None] >> (5 * k)) & 0x1f
    g |= (k < n[:, None] - 1) << 5  # more groups follow
    return (g[k < n[:, None]] + 48).astype(np.uint8).tobytes().decode("ascii")


def from_string(s):
    """uint32 counts of a compressed COCO RLE `counts` string (str or bytes)."""
    b = s.encode("ascii") if isinstance(s, str) else bytes(s)
    counts = []
    p = 0
    while p < len(b):
        x, k, more = 0, 0, True
        while more:
            if p >= len(b):
                raise ValueError("truncated RLE string")
            g = b[p] - 48
            x |= (g & 0x1f) << (5 * k)
            more = bool(g & 0x20)
            p += 1
            k += 1
            if not more and (g & 0x10):
                x |= -1 << (5 * k)  # sign-extend
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return np.asarray(counts, np.int64).astype(np.uint32)


def area(counts):
    """Number of set pixels: the sum of the odd-indexed runs."""
    return int(np.asarray(counts, np.int64).reshape(-1)[1::2].sum())


def to_bbox(counts, H, W):
    """[x, y, w, h] of the tight box around the set pixels ([0,0,0,0] when empty)."""
    c = np.asarray(counts, np.int64).reshape(-1)
    ends = np.cumsum(c)
    s, e = (ends - c)[1::2], ends[1::2]  # set runs [s, e) in column-major positions
    keep = e > s
    s, e = s[keep], e[keep] - 1
    if not len(s):
        return [0, 0, 0, 0]
    x0, x1 = int(s[0] // H), int(e[-1] // H)
    # a run that crosses a column seam covers the bottom row and the top row
    if np.any(s // H != e // H):
        y0, y1 = 0, H - 1
    else:
        y0, y1 = int((s % H).min()), int((e % H).max())
    return [x0, y0, x1 - x0 + 1, y1 - y0 + 1]


# ---- the total contracts of csrc/mask_rle_string.hip --------------------------------------
TRUNCATED, BAD_CHAR, TOO_LONG, RANGE = 1, 2, 4, 8  # parse_total's status bits
STATUS_WORDS = ((TRUNCATED, "truncated RLE string"),
                (BAD_CHAR, "a character outside '0'..'o'"),
                (TOO_LONG, "a count of more than 7 groups"),
                (RANGE, "a count outside [0, 2^32)"))


def status_text(status):
    """The reasons a nonzero parse_total status stands for, TRUNCATED in from_string's words."""
    return ", ".join(text for bit, text in STATUS_WORDS if status & bit)


def summarize(counts, H, W):
    """([x, y, w, h], area) of the canvas `decode_canvas(counts, H, W)` gives: the tight box
    around its set pixels ([0,0,0,0] when there is none) and their number; the CPU statement
    of the boxes / areas of isg_rle_compress. Total: with ends = cumsum(counts) in 64 bits,
    the set runs are [min(ends[i-1], H*W), min(ends[i], H*W)) for odd i (runs are clipped at
    H*W, zero-length runs are stepped over), empty counts give [0,0,0,0], 0. A set run that
    crosses a column seam covers the bottom row and the top row, so y spans 0..H-1. Where the
    counts sum to H*W this is (to_bbox, area)."""
    c = np.asarray(counts).reshape(-1)
    if c.size and (c.dtype.kind not in "iu" or c.min() < 0 or c.max() >= 2 ** 32):
        raise ValueError("counts must be integers in [0, 2^32)")
    hw = H * W
    ends = np.minimum(np.cumsum(c.astype(np.uint64)), np.uint64(hw)).astype(np.int64)
    e = ends[1::2]
    s = np.concatenate([[0], ends])[1:len(ends):2]  # the end of the run before each odd run
    keep = e > s
    s, e = s[keep], e[keep] - 1  # first and last position of every non-empty set run
    if not len(s):
        return [0, 0, 0, 0], 0
    x0, x1 = int((s // H).min()), int((e // H).max())
    if np.any(s // H != e // H):
        y0, y1 = 0, H - 1
    else:
        y0, y1 = int((s % H).min()), int((e % H).max())
    return [x0, y0, x1 - x0 + 1, y1 - y0 + 1], int((e - s + 1).sum())


def compress(counts):
    """bytes of the `counts` string, `to_string` stated per count (the CPU statement of the
    characters of isg_rle_compress). Count i is written as v_i = c_i for i <= 2 and
    v_i = c_i - c_{i-2} (signed, 64 bits) for i >= 3, in n_i groups: the fewest n in 1..7 with
    -2^(5n-1) <= v < 2^(5n-1) (seven always suffice for uint32 counts: |v| < 2^32). Group k
    is ((v >> 5k) & 31) | (32 if k < n - 1 else 0), plus 48; count i starts at the sum of
    the n before it."""
    c = np.asarray(counts).reshape(-1)
    if c.size and (c.dtype.kind not in "iu" or c.min() < 0 or c.max() >= 2 ** 32):
        raise ValueError("counts must be integers in [0, 2^32)")
    c = c.astype(np.int64)
    v = c.copy()
    v[3:] = c[3:] - c[1:-2]
    x = v ^ (v >> 63)  # v for v >= 0, -v - 1 below: x < 2^(5n-1) is the range test
    n = np.ones(len(v), np.int64)
    for k in range(1, 7):
        n += x >= (np.int64(1) << (5 * k - 1))
    start = np.cumsum(n) - n
    out = np.zeros(int(n.sum()), np.uint8)
    for k in range(7):
        m = k < n
        out[start[m] + k] = (((v[m] >> (5 * k)) & 31) | ((k < n[m] - 1) << 5)) + 48
    return out.tobytes()


def parse_total(b):
    """(uint32 counts, status) of the bytes of a `counts` string: the total form of
    `from_string` and the CPU statement of isg_rle_parse. Every byte is read as
    g = (byte - 48) & 0x3f; a byte with g & 0x20 == 0 ends a count, so there are as many
    counts as terminators. A count of k groups takes the value of its last min(k, 7) groups:
    the sum of (g & 31) << 5m over them, lowest first, sign-extended from bit 5 min(k, 7)
    when the terminator has g & 0x10 (for k <= 7 that is from_string's value; a TOO_LONG
    count so keeps a definite value, that of its last seven groups). The stride-2 delta is
    undone in wrapping int64 arithmetic, c_i = v_i + c_{i-2} for i >= 3, and the low 32 bits
    are stored. status is the OR of
      TRUNCATED  the last byte continues (its dangling groups yield no count),
      BAD_CHAR   a byte outside 48..111,
      TOO_LONG   a count of more than 7 groups,
      RANGE      a count outside [0, 2^32) after the delta is undone.
    Every string `compress` emits parses with status 0 to the counts it was made from."""
    a = np.frombuffer(b.encode("latin-1") if isinstance(b, str) else bytes(b), np.uint8)
    g = (a.astype(np.int64) - 48) & 0x3f
    term = (g & 0x20) == 0
    status = 0
    if a.size and not term[-1]:
        status |= TRUNCATED
    if np.any((a < 48) | (a > 111)):
        status |= BAD_CHAR
    t = np.flatnonzero(term)
    if not len(t):
        return np.zeros(0, np.uint32), status
    k = t - np.concatenate([[-1], t[:-1]])  # groups of each count
    if np.any(k > 7):
        status |= TOO_LONG
    n = np.minimum(k, 7)
    v = np.zeros(len(t), np.int64)
    for m in range(7):
        use = m < n
        v[use] |= (g[t[use] - n[use] + 1 + m] & 31) << (5 * m)
    neg = (g[t] & 0x10) != 0
    v[neg] |= np.int64(-1) << (5 * n[neg])
    c = v.copy()
    c[1::2] = np.cumsum(v[1::2])
    c[2::2] = np.cumsum(v[2::2])
    if np.any((c < 0) | (c >= 2 ** 32)):
        status |= RANGE
    return (c & 0xffffffff).astype(np.uint32), status


def image_id_of(basename):
    """COCO file names are the zero-padded image id; anything else keeps its name."""
    return int(basename) if basename.isdigit() else basename


def assemble_results(out_dir):
    """COCO results list from the per-image `<name>.json` files of a --format coco run:
    one {"image_id", "category_id": 1, "segmentation", "bbox", "score"} per kept instance.
    `results.json` itself and JSONs without a "segmentation" field are not per-image files."""
    results = []
    for path in sorted(glob.glob(os.path.join(out_dir, "*.json"))):
        name = os.path.splitext(os.path.basename(path))[0]
        if name == "results":
            continue
        with open(path) as f:
            res = json.load(f)
        if not isinstance(res, dict) or "segmentation" not in res:
            continue
        for k, seg, box in zip(res["keep"], res["segmentation"], res["bbox"]):
            results.append({"image_id": image_id_of(name), "category_id": 1,
                            "segmentation": seg, "bbox": box,
                            "score": float(res["scores"][k])})
    return results


def write_results(out_dir):
    """Assemble and write `<out_dir>/results.json`; returns the list."""
    results = assemble_results(out_dir)
    with open(os.path.join(out_dir, "results.json"), "w") as f:
        json.dump(results, f)
    return results
