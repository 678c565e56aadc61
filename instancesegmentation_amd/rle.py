"""COCO run-length encoding of binary masks (numpy only: no torch, no GPU).

This module is the CPU statement of the contracts that csrc/mask_rle.hip (`encode`) and
csrc/mask_rle_decode.hip (`decode_canvas`) implement, and the codec between the kernels'
`counts` and the strings COCO tools read.

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
