"""What tests/test_gpu_kp_stem_forms.py feeds the keypoint stem (isg_kp_stem_fwd / _wgrad,
isg_kp_pool; csrc/kp_stem.hip) and the fp64 expectations it compares them with. numpy and torch
on the CPU only: tests/test_kp_stem_cases_cpu.py proves, without a GPU, that the references
agree with torch autograd over cat(image, heatmaps), that no heatmap pixel sits on the
threshold, and that every row's keypoints reach the code paths the row is there for.

ROWS is the geometry table. A case is a row in one operand form (FWD_FORMS for the forward,
WG_FORMS for the weight gradient): what a form changes is how the operands are presented, and
the forms of one data kind (KIND) share their inputs, which is what lets the GPU test ask them
for the same bits.

The heatmaps are oracle.heatmaps_oracle.keypoint2heatmaps's fp32 values, widened to fp64
exactly; every other input is an fp32 array widened the same way."""
import functools
import math
from typing import NamedTuple

import numpy as np
import torch
import torch.nn.functional as F

from oracle.heatmaps_oracle import keypoint2heatmaps
from tests.conv_cases import make_seg

THRESHOLD = 0.01
TILE = 16          # kp_fwd_kernel: one workgroup per 16 x 16 output tile
WG_PIX = 256       # kp_wgrad_kernel: output pixels per staged chunk
WG_BANDS = 4       # kp_wgrad_kernel: row bands (gridDim.y)
WIDE = 3           # channels by which a BatchNorm layer is wider than the dy segment reading it
TIE_MARGIN = 1e-9  # |e - threshold| every window pixel keeps (asserted on the CPU)


class Row(NamedTuple):
    id: str
    Co: int
    c_kp0: int
    parts: int
    H: int
    W: int
    k: tuple
    s: tuple
    p: tuple
    d: tuple
    sigma: float
    note: str = ""

    @property
    def Ci(self):
        return self.c_kp0 + self.parts

    @property
    def KK(self):
        return self.k[0] * self.k[1]

    @property
    def OH(self):
        return (self.H + 2 * self.p[0] - self.d[0] * (self.k[0] - 1) - 1) // self.s[0] + 1

    @property
    def OW(self):
        return (self.W + 2 * self.p[1] - self.d[1] * (self.k[1] - 1) - 1) // self.s[1] + 1

    @property
    def foot(self):
        """Input footprint of a 16 x 16 output tile (kp_args FH, FW)."""
        return tuple(self.s[i] * (TILE - 1) + self.d[i] * (self.k[i] - 1) + 1 for i in (0, 1))

    @property
    def r(self):
        return math.sqrt(math.log(THRESHOLD) * -(self.sigma ** 2))

    @property
    def T(self):
        """fp32 terms one output pixel's accumulator can see (every part active)."""
        return self.parts * self.KK


def _r(id, Co, c_kp0, parts, H, W, k, s, p, d, sigma, note=""):
    return Row(id, Co, c_kp0, parts, H, W, k, s, p, d, float(sigma), note)


ROWS = [
    _r("stem", 16, 3, 17, 72, 88, (5, 5), (2, 2), (2, 2), (1, 1), 10),
    _r("k3", 5, 0, 1, 40, 56, (3, 3), (1, 1), (1, 1), (1, 1), 3,
       note="one part: no tile can be reached by two windows, and its three keypoint slots hold "
            "the border, the invisible and the origin keypoint only"),
    _r("k1s3", 16, 2, 4, 51, 47, (1, 1), (3, 3), (0, 0), (1, 1), 3,
       note="51 rows, not 50: a window's first row is never past H - 2, so with H - 1 = 49 every "
            "window holds a row that is a multiple of the stride; with H - 1 = 50 the one-row "
            "window [49, 50) reaches no output pixel, which is what the row is there for"),
    _r("asym", 7, 1, 6, 44, 60, (3, 5), (1, 2), (1, 2), (2, 1), 4),
    _r("k7", 10, 0, 10, 36, 36, (7, 7), (1, 1), (3, 3), (1, 1), 3),
    _r("p32", 16, 3, 32, 48, 64, (3, 3), (2, 2), (1, 1), (1, 1), 3),
    _r("chunks", 8, 2, 3, 66, 80, (3, 3), (1, 1), (1, 1), (1, 1), 10,
       note="66 rows, not 64: 64 x 80 outputs are whole 16 x 16 tiles only, and every row keeps a "
            "partial tile; three parts leave no slot for the wholly-outside-by-x keypoint in "
            "image 0, it sits in image 2"),
]
ROW = {r.id: r for r in ROWS}

FWD_FORMS = ("fwd-base", "fwd-nostats", "fwd-off1", "fwd-n1")
WG_FORMS = ("wgrad-plain", "wgrad-bn_train", "wgrad-coef", "wgrad-nrep1", "wgrad-n1")
KIND = {"fwd-base": "fwd", "fwd-nostats": "fwd", "fwd-off1": "fwd", "fwd-n1": "fwd-n1",
        "wgrad-plain": "wg", "wgrad-nrep1": "wg", "wgrad-bn_train": "wg-bn_train",
        "wgrad-coef": "wg-coef", "wgrad-n1": "wg-n1"}
FWD_CASES = [(r.id, f) for r in ROWS for f in FWD_FORMS]
WG_CASES = [(r.id, f) for r in ROWS for f in WG_FORMS]


# ---- keypoints ------------------------------------------------------------------------------
def drawn(q):
    """Whether keypoint q = (x, y, visible) draws a map. The reference raises on a non-finite
    coordinate (int()) and on +-1e300 (numpy.arange over a bound beyond int64); the kernels
    treat such a part as not visible (common.h kp_coord), and so does the expectation."""
    return bool(q[2] > 0 and np.isfinite(q[0]) and np.isfinite(q[1]) and abs(q[0]) < 1e12 and abs(q[1]) < 1e12)


def corner(row):
    """A keypoint exactly on a 16 x 16 output-tile corner, mapped back through stride and pad
    (output column 8 where the row has one tile column only)."""
    ox = TILE if row.OW > TILE else TILE // 2
    return (float(ox * row.s[1] - row.p[1]), float(TILE * row.s[0] - row.p[0]))


@functools.lru_cache(maxsize=None)
def keypoints(rid):
    """[3, parts, 3] fp64, read-only. Image 0: near the right / bottom border, on a tile
    corner, a second window over the same tile, wholly outside, then anywhere. Image 1 draws
    nothing: invisible, NaN, infinite and +-1e300 parts in turn. Image 2 keeps to its top-left
    third, so its bottom-right tile is reached by no window: about (-r + 1.5, -r + 1.5), a one-row
    window [H - 2, H - 1), then fillers."""
    row = ROW[rid]
    rng = np.random.default_rng(4099 * ROWS.index(row) + 17)
    H, W, r, n = row.H, row.W, row.r, row.parts
    kp = np.zeros((3, n, 3), np.float64)
    kp[0, :, 0] = rng.uniform(-r, W + r, n)
    kp[0, :, 1] = rng.uniform(-r, H + r, n)
    kp[0, :, 2] = rng.uniform(size=n) < 0.8
    cx, cy = corner(row)
    outside = (W + r + 3.5, 0.5 * H, 1.0)
    first = [(W - 0.45 * r, H - 0.55 * r, 1.0), (cx, cy, 1.0), (cx + 0.37 * r, cy - 0.41 * r, 1.0), outside]
    for j, q in enumerate(first[:n]):
        kp[0, j] = q
    dead = [(0.4 * W, 0.6 * H, 0.0), (np.nan, 0.5 * H, 1.0), (0.5 * W, -1e300, 1.0), (np.inf, 0.3 * H, 1.0),
            (1e300, 0.5 * H, 1.0), (0.5 * W, -np.inf, 1.0), (0.5 * W, 0.5 * H, -1.0)]
    for j in range(n):
        kp[1, j] = dead[j % len(dead)]
    kp[2, :, 0] = rng.uniform(-r, W / 3.0, n)
    kp[2, :, 1] = rng.uniform(-r, H / 3.0, n)
    kp[2, :, 2] = rng.uniform(size=n) < 0.8
    kp[2, 0] = (-r + 1.5, -r + 1.5, 1.0)
    if n >= 4:
        kp[2, 1] = (0.25 * W, (H - 2) + r + 0.5, 1.0)
    elif n >= 2:
        kp[2, n - 1] = outside
    kp.setflags(write=False)
    return kp


def window(row, q):
    """(x0, x1, y0, y1) of a drawn keypoint's window as the reference computes it: python int()
    truncates toward zero, and the last row / column of the image is never inside."""
    r = row.r
    return (max(0, int(q[0] - r)), min(row.W - 1, int(q[0] + r + 1)),
            max(0, int(q[1] - r)), min(row.H - 1, int(q[1] + r + 1)))


def out_range(row, win):
    """(oy_lo, oy_hi, ox_lo, ox_hi), inclusive: the output pixels with a tap inside the window
    (kp_wgrad_kernel's arithmetic; python // floors)."""
    x0, x1, y0, y1 = win
    (KH, KW), (SH, SW), (PH, PW), (DH, DW) = row.k, row.s, row.p, row.d
    return (max(0, -(-(y0 + PH - DH * (KH - 1)) // SH)), min(row.OH - 1, (y1 - 1 + PH) // SH),
            max(0, -(-(x0 + PW - DW * (KW - 1)) // SW)), min(row.OW - 1, (x1 - 1 + PW) // SW))


def windows(row, kp):
    """[(n, j, window, raw)] of every drawn keypoint; raw = (int(x - r), int(y - r)) unclipped."""
    out = []
    for n in range(kp.shape[0]):
        for j in range(kp.shape[1]):
            if drawn(kp[n, j]):
                raw = (int(kp[n, j, 0] - row.r), int(kp[n, j, 1] - row.r))
                out.append((n, j, window(row, kp[n, j]), raw))
    return out


def tile_hits(row, kp):
    """[N, tiles_y, tiles_x]: how many non-empty windows meet each output tile's input
    footprint (kp_fwd_kernel's `hit`)."""
    ty, tx = -(-row.OH // TILE), -(-row.OW // TILE)
    hits = np.zeros((kp.shape[0], ty, tx), np.int64)
    FH, FW = row.foot
    for n, _, (x0, x1, y0, y1), _ in windows(row, kp):
        if x1 <= x0 or y1 <= y0:
            continue
        for a in range(ty):
            for b in range(tx):
                iy0, ix0 = a * TILE * row.s[0] - row.p[0], b * TILE * row.s[1] - row.p[1]
                hits[n, a, b] += y0 < iy0 + FH and y1 > iy0 and x0 < ix0 + FW and x1 > ix0
    return hits


def wg_blocks(row, kp):
    """[(n, j, band, rows in the band, ncol)] of every kp_wgrad_kernel workgroup that stages
    anything: band = ceil(nrow / 4) rows of the window's output rows per blockIdx.y."""
    out = []
    for n, j, win, _ in windows(row, kp):
        if win[1] <= win[0] or win[3] <= win[2]:
            continue
        oy_lo, oy_hi, ox_lo, ox_hi = out_range(row, win)
        if oy_hi < oy_lo or ox_hi < ox_lo:
            continue
        nrow, ncol = oy_hi - oy_lo + 1, ox_hi - ox_lo + 1
        band = -(-nrow // WG_BANDS)
        for b in range(WG_BANDS):
            rows = min(oy_hi + 1, oy_lo + (b + 1) * band) - (oy_lo + b * band)
            if rows > 0:
                out.append((n, j, b, rows, ncol))
    return out


def reach(row, kp):
    """P: the most output pixels one part's window reaches in one image."""
    best = 0
    for _, _, win, _ in windows(row, kp):
        if win[1] > win[0] and win[3] > win[2]:
            oy_lo, oy_hi, ox_lo, ox_hi = out_range(row, win)
            best = max(best, max(0, oy_hi - oy_lo + 1) * max(0, ox_hi - ox_lo + 1))
    return best


def replicas_of(case, nrep):
    """(may, must), each [nrep, parts] bool: the weight-gradient replicas a workgroup of part j
    adds into, (blockIdx.x + 7 * blockIdx.y) % nrep with blockIdx.x = n * parts + j, and those
    among them whose workgroup's band taps a non-zero heatmap pixel. Every replica outside `may`
    must keep the bits of that part's channel; every replica in `must` receives a sum of
    products with dy that is zero only by accident."""
    row, kp, maps = case["row"], case["kp"], case["maps"]
    (KH, KW), (SH, SW), (PH, PW), (DH, DW) = row.k, row.s, row.p, row.d
    may, must = np.zeros((nrep, row.parts), bool), np.zeros((nrep, row.parts), bool)
    for n, j, b, rows, _ in wg_blocks(row, kp):
        rep = (n * row.parts + j + 7 * b) % nrep
        may[rep, j] = True
        oy_lo, oy_hi, ox_lo, ox_hi = out_range(row, window(row, kp[n, j]))
        r_lo = oy_lo + b * -(-(oy_hi - oy_lo + 1) // WG_BANDS)
        iy, ix = np.nonzero(maps[n, j])
        ok_y, ok_x = np.zeros(iy.shape, bool), np.zeros(ix.shape, bool)
        for kh in range(KH):  # pixel row iy is tap kh of output row (iy + PH - kh*DH) / SH
            t = iy + PH - kh * DH
            ok_y |= (t % SH == 0) & (t // SH >= r_lo) & (t // SH < r_lo + rows)
        for kw in range(KW):
            t = ix + PW - kw * DW
            ok_x |= (t % SW == 0) & (t // SW >= ox_lo) & (t // SW <= ox_hi)
        must[rep, j] |= bool((ok_y & ok_x).any())
    return may, must


def maps_of(row, kp):
    """[N, parts, H, W] fp32: the oracle's heatmaps of the drawn keypoints."""
    out = np.zeros((kp.shape[0], row.parts, row.H, row.W), np.float32)
    for n in range(kp.shape[0]):
        pts = {j: (kp[n, j, 0], kp[n, j, 1]) for j in range(row.parts) if drawn(kp[n, j])}
        out[n] = np.stack(keypoint2heatmaps(pts, (row.H, row.W), sigma=row.sigma, threshold=THRESHOLD,
                                            n_parts=row.parts))
    return out


@functools.lru_cache(maxsize=None)
def row_maps(rid):
    m = maps_of(ROW[rid], keypoints(rid))
    m.setflags(write=False)
    return m


def tie_distance(row, kp):
    """min |e - threshold| over every pixel of every drawn window, e the double of the
    oracle's own expression."""
    best = np.inf
    for n, j, (x0, x1, y0, y1), _ in windows(row, kp):
        if x1 <= x0 or y1 <= y0:
            continue
        x, y = kp[n, j, 0], kp[n, j, 1]
        xs, ys = np.arange(x0, x1), np.arange(y0, y1)[:, None]
        e = np.exp(-((xs - x) ** 2 + (ys - y) ** 2) / row.sigma ** 2)
        best = min(best, float(np.abs(e - THRESHOLD).min()))
    return best


# ---- references -----------------------------------------------------------------------------
def conv_kw(row):
    return dict(stride=row.s, padding=row.p, dilation=row.d)


def _seed(row, kind):
    return 7919 * ROWS.index(row) + 101 * sorted(set(KIND.values())).index(kind) + 3


def abs_dy(sg):
    """An elementwise bound of |dy| through the arithmetic that forms it: |p| for a plain
    segment, |A||g| + |B||y - mean| + |C| for BatchNorm backward (common.h bwd_coef_of)."""
    if sg["xf"] == "plain":
        return np.abs(sg["v"])
    C, bnC, M = sg["C"], sg["bnC"], sg["count"]
    if sg["bn"] == "coef":
        A, B, mean, Cc = (sg["coef_bwd"][:, i].astype(np.float64) for i in range(4))
    else:
        gam, rstd, mean, st = sg["gamma"].astype(np.float64), sg["rstd"], sg["mean"], sg["stats"]
        A = gam * rstd
        B = -gam * rstd * rstd * (rstd * st[3 * bnC:] / M)
        Cc = -gam * rstd * (st[2 * bnC:3 * bnC] / M)
    b = lambda a: np.abs(a)[None, :C, None, None]
    return (b(A) * np.abs(sg["p"].astype(np.float64))
            + b(B) * np.abs(sg["y"].astype(np.float64) - mean[None, :C, None, None]) + b(Cc))


def _freeze(case):
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def _data(rid, kind):
    row = ROW[rid]
    rng = np.random.default_rng(_seed(row, kind))
    N = 1 if kind.endswith("n1") else 3
    kp = keypoints(rid)[:N]
    maps = torch.from_numpy(row_maps(rid)[:N].astype(np.float64))
    case = {"row": row, "N": N, "kp": kp, "maps": row_maps(rid)[:N], "P": reach(row, keypoints(rid))}
    if kind.startswith("fwd"):
        fan = row.Ci * row.KK
        w = (rng.normal(0.0, 1.0, (row.Co, row.Ci, *row.k)) * (2.0 / fan) ** 0.5).astype(np.float32)
        v = rng.normal(0.0, 1.0, (N, row.Co, row.OH, row.OW)).astype(np.float32)
        v[v == 0] = 0.5  # -0.0 + 0 would become +0.0: the untouched pixels are compared bitwise
        wk = torch.from_numpy(w[:, row.c_kp0:].astype(np.float64))
        sums = rng.uniform(1.0, 50.0, 4 * row.Co) * rng.choice([-1.0, 1.0], 4 * row.Co)
        case.update(w=w, v=v, delta=F.conv2d(maps, wk, None, **conv_kw(row)).numpy(),
                    mag=F.conv2d(maps, wk.abs(), None, **conv_kw(row)).numpy(), stats0=sums)
        return _freeze(case)
    xf, bn = {"wg-bn_train": ("bn_bwd", "train"), "wg-coef": ("bn_bwd", "coef")}.get(kind, ("plain", "eval"))
    sg = make_seg(rng, N, row.Co, row.OH, row.OW, xf, bn=bn, bnC=row.Co + WIDE)
    shape = (row.Co, row.parts, *row.k)
    wgrad = lambda dy: torch.nn.grad.conv2d_weight(maps, shape, torch.from_numpy(dy), **conv_kw(row)).numpy()
    case.update(dy=sg, dw=wgrad(sg["v"]), mag_w=wgrad(abs_dy(sg)))
    return _freeze(case)


def make_case(rid, form):
    """Inputs and fp64 expectations of row `rid` in operand form `form` — cached, read-only,
    shared by the forms of one data kind.
      forward: kp, w [Co][Ci][KH][KW], v (the dense part already in y), delta and mag (the fp64
        conv of the heatmaps with w and |w| over the heatmap channels), stats0 (4*Co sums);
      weight gradient: kp, dy (a conv_cases.make_seg segment), dw and mag_w ([Co][parts][KH][KW],
        the fp64 weight gradient of the heatmap channels with dy and with abs_dy), P."""
    return dict(_data(rid, KIND[form]), form=form)


# ---- refusals (include/isg.h, isg_kp_stem) --------------------------------------------------
INVALID, UNSUPPORTED = -1, -2
ALL3, CONV = ("fwd", "wgrad", "pool"), ("fwd", "wgrad")
REF_GEOM = dict(N=2, Ci=20, H=32, W=48, Co=16, OH=16, OW=24, KH=5, KW=5, SH=2, SW=2, PH=2, PW=2,
                DH=1, DW=1, groups=1)
REF_PARTS, REF_CKP0 = 17, 3

# (what, entry points, overrides, code): a "g" override updates the geometry, "dy" names a
# malformed gradient vtensor, None clears a pointer
REFUSED = [
    ("no parts", ALL3, dict(nparts=0), INVALID),
    ("33 parts", ALL3, dict(nparts=33), INVALID),
    ("sigma 0", ALL3, dict(sigma=0.0), INVALID),
    ("threshold 0", ALL3, dict(threshold=0.0), INVALID),
    ("threshold 1", ALL3, dict(threshold=1.0), INVALID),
    ("NULL kp", ALL3, dict(kp=None), INVALID),
    ("N 0", ALL3, dict(g=dict(N=0)), INVALID),
    ("H 0", ALL3, dict(g=dict(H=0)), INVALID),
    ("W 0", ALL3, dict(g=dict(W=0)), INVALID),
    ("NULL w", ("fwd",), dict(w=None), INVALID),
    ("NULL y", ("fwd",), dict(y=None), INVALID),
    ("NULL dw", ("wgrad",), dict(dw=None), INVALID),
    ("dy of two segments", ("wgrad",), dict(dy="two"), INVALID),
    ("dy narrower than Co", ("wgrad",), dict(dy="narrow"), INVALID),
    ("no replicas", ("wgrad",), dict(nrep=0), INVALID),
    ("two replicas without a stride", ("wgrad",), dict(nrep=2, rep_stride=0), INVALID),
    ("NULL out", ("pool",), dict(out=None), INVALID),
    ("pool window 0", ("pool",), dict(k=0), INVALID),
    ("pool window not dividing H", ("pool",), dict(k=3), INVALID),
    ("radius 128.8", ALL3, dict(sigma=60.0), UNSUPPORTED),
    ("groups 2", CONV, dict(g=dict(groups=2)), UNSUPPORTED),
    ("Co 17", CONV, dict(g=dict(Co=17)), UNSUPPORTED),
    ("an 8x8 kernel", CONV, dict(g=dict(KH=8, KW=8)), UNSUPPORTED),
    ("c_kp0 + nparts != Ci", CONV, dict(c_kp0=4), UNSUPPORTED),
    ("a tile footprint of 65", CONV, dict(g=dict(SH=4, SW=4)), UNSUPPORTED),
    ("17 parts x 49 taps", ("fwd",), dict(g=dict(KH=7, KW=7, PH=3, PW=3)), UNSUPPORTED),
    ("Co x taps = 560", ("wgrad",), dict(nparts=8, g=dict(Ci=11, KH=7, KW=5)), UNSUPPORTED),
    ("a residual-form dy", ("wgrad",), dict(dy="residual"), UNSUPPORTED),
    # dilation in the weight gradient's staging bound: the host once took both
    ("286 output columns per window", ("wgrad",),
     dict(sigma=55.0, g=dict(KH=1, KW=2, SH=1, SW=1, PH=0, PW=0, DW=48)), UNSUPPORTED),
    ("a dilated window footprint of 52 x 110", ("wgrad",),
     dict(sigma=3.0, g=dict(KH=2, KW=2, SH=1, SW=1, PH=0, PW=0, DH=48, DW=48)), UNSUPPORTED),
]


def refusal_spec(over, ptrs, nrep):
    """The isg_kp_stem field dictionary of a refused call. ptrs: kp, w, y, stats, dw, out and p
    (the gradient segment), valid device addresses on the GPU and any non-zero number on the
    CPU, where the host checks return before anything is read."""
    g = dict(REF_GEOM, **over.get("g", {}))
    Co, hw = REF_GEOM["Co"], REF_GEOM["OH"] * REF_GEOM["OW"]
    seg = lambda C, **kw: dict({"p": ptrs["p"], "n_stride": Co * hw, "C": C, "xform": 0}, **kw)
    segs = {"one": [seg(Co)], "two": [seg(9), seg(7)], "narrow": [seg(Co - 1)],
            "residual": [seg(Co, xform=1, y=ptrs["p"], y_n_stride=Co * hw)]}[over.get("dy", "one")]
    spec = {"kp": ptrs["kp"], "nparts": REF_PARTS, "c_kp0": REF_CKP0, "sigma": 10.0, "threshold": THRESHOLD,
            "w": ptrs["w"], "y": ptrs["y"], "y_n_stride": Co * hw, "stats": ptrs["stats"],
            "dy": {"s": segs, "nseg": len(segs), "N": g["N"], "H": REF_GEOM["OH"], "W": REF_GEOM["OW"]},
            "dw": ptrs["dw"], "rep_stride": Co * REF_GEOM["Ci"] * 25 + 7, "nrep": nrep, "k": 4,
            "out": ptrs["out"], "out_n_stride": REF_PARTS * (REF_GEOM["H"] // 4) * (REF_GEOM["W"] // 4)}
    spec.update({k: v for k, v in over.items() if k not in ("g", "dy")})
    spec["g"] = g
    return spec
