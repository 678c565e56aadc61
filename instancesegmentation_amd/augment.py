"""Random augmentation of training samples: the numpy statement of isg_train_crop_aug
(csrc/train_crop.hip, include/isg.h). CPU only; the kernel matches `augment_sample` bit for bit.

The reference's loader lists five random augmentations and has all of them commented out
(train_instance.py:153-155, :186-191): rotation +/-25 degrees, a jitter of every side of the
crop by up to 20 % of the box, LinearContrast(0.75, 1.5), AdditiveGaussianNoise(0, (0,
0.05*255), per_channel=0.5) and Multiply((0.8, 1.2), per_channel=0.2), each but the jitter
under Sometimes(0.6). `Augment` holds those numbers, `draw_augment` draws one record per
sample on the host, and the kernel (or `augment_sample`) applies a record: the device takes
parameters, never probabilities. The one random thing left to the device is the per-pixel
noise, a counter-based generator (`philox4x32_10`) addressed by (seed, sample ordinal, pixel).

Two deliberate differences from imgaug: the photometric steps act on the resampled crop, not
on the source image before the resize (that would be a second pass over memory); and the noise
is the centred sum of four uniform bytes (Irwin-Hall, cut at +/-3.46 sigma) scaled to the drawn
standard deviation, which is integer arithmetic both sides compute identically.
"""
import dataclasses
import math

import numpy as np

from .data import (N_PARTS, ORDER_PART_NAMES, TRAIN_PAD, blend_taps, crop_resample, instance_box,
                   round_u8)

JITTER_ONE = 1024                 # a jitter integer j moves a side by floor(j * a / 1024)
JITTER_DIV = 5                    # a = box extent // 5
NOISE_SIGMA = math.sqrt(4 * (256 ** 2 - 1) / 12)  # of the sum of four uniform bytes: 147.80
VALUE_MAX = 65536.0               # isg.h ISG_TRAIN_AUG_MAX

# isg.h isg_train_aug, field for field (64 bytes)
AUG_DTYPE = np.dtype([("rot_cos", "<f8"), ("rot_sin", "<f8"), ("jitter", "<i4", (4,)),
                      ("flip", "<i4"), ("noise_per_channel", "<i4"), ("contrast", "<f4"),
                      ("noise", "<f4"), ("mult", "<f4", (3,)), ("pad_", "<i4")])


def _mirror_rows():
    """Row of ORDER_PART_NAMES holding the other side's part (the nose is its own)."""
    swap = {"left": "right", "right": "left"}
    out = []
    for name in ORDER_PART_NAMES:
        side, _, part = name.partition("_")
        out.append(ORDER_PART_NAMES.index(swap[side] + "_" + part) if side in swap else
                   ORDER_PART_NAMES.index(name))
    return np.array(out, np.int64)


MIRROR_PART = _mirror_rows()


@dataclasses.dataclass
class Augment:
    """Probabilities and ranges; the defaults are the reference's commented-out list. The flip
    is not in the reference, so it is off."""
    jitter: float = 1.0 / JITTER_DIV      # each side moves by up to this fraction of the box (<= 1/5)
    flip_p: float = 0.0
    rotate_p: float = 0.6
    rotate_deg: float = 25.0
    contrast_p: float = 0.6
    contrast: tuple = (0.75, 1.5)
    noise_p: float = 0.6
    noise_scale: tuple = (0.0, 0.05 * 255)  # standard deviation, in grey levels
    noise_per_channel_p: float = 0.5
    multiply_p: float = 0.6
    multiply: tuple = (0.8, 1.2)
    multiply_per_channel_p: float = 0.2

    def __post_init__(self):
        if not 0.0 <= self.jitter <= 1.0 / JITTER_DIV:
            raise ValueError(f"Augment: jitter {self.jitter} outside [0, 1/{JITTER_DIV}]")
        for name in ("flip_p", "rotate_p", "contrast_p", "noise_p", "noise_per_channel_p",
                     "multiply_p", "multiply_per_channel_p"):
            if not 0.0 <= getattr(self, name) <= 1.0:
                raise ValueError(f"Augment: {name} = {getattr(self, name)} is not a probability")
        for name in ("contrast", "noise_scale", "multiply"):
            lo, hi = getattr(self, name)
            if not 0.0 <= lo <= hi <= VALUE_MAX:
                raise ValueError(f"Augment: {name} = {(lo, hi)}")

    @classmethod
    def off(cls):
        """Every draw is the identity record."""
        return cls(jitter=0.0, flip_p=0.0, rotate_p=0.0, contrast_p=0.0, noise_p=0.0, multiply_p=0.0)


def identity_records(n):
    t = np.zeros(n, AUG_DTYPE)
    t["rot_cos"] = 1.0
    t["contrast"] = 1.0
    t["mult"] = 1.0
    return t


def draw_augment(rng, n, cfg):
    """n records (AUG_DTYPE) from a numpy.random.Generator. The stream is consumed in a fixed
    order whatever cfg says, so a change of one probability leaves the other draws alone:

        J = rng.integers(-jm, jm + 1, size=(n, 4))    jm = round(1024 * 5 * cfg.jitter)
        U = rng.random((n, 13))                        float64 in [0, 1)

    and of sample i: jitter = J[i]; flip = U[i,0] < flip_p; rotation fires if U[i,1] < rotate_p,
    its angle (2 U[i,2] - 1) * rotate_deg; contrast fires if U[i,3] < contrast_p, alpha from
    U[i,4]; noise fires if U[i,5] < noise_p, its standard deviation from U[i,6], per channel if
    U[i,7] < noise_per_channel_p; multiply fires if U[i,8] < multiply_p, per channel if U[i,9] <
    multiply_per_channel_p, the multipliers from U[i,10:13] (all U[i,10] unless per channel).
    A range (lo, hi) is sampled as lo + U (hi - lo)."""
    jm = int(round(JITTER_ONE * JITTER_DIV * cfg.jitter))
    J = rng.integers(-jm, jm + 1, size=(n, 4))
    U = rng.random((n, 13))
    t = identity_records(n)
    t["jitter"] = J
    t["flip"] = U[:, 0] < cfg.flip_p
    ang = np.deg2rad((2.0 * U[:, 2] - 1.0) * cfg.rotate_deg)
    fire = U[:, 1] < cfg.rotate_p
    t["rot_cos"] = np.where(fire, np.cos(ang), 1.0)
    t["rot_sin"] = np.where(fire, np.sin(ang), 0.0)

    def span(r, u):
        return r[0] + u * (r[1] - r[0])

    t["contrast"] = np.where(U[:, 3] < cfg.contrast_p, span(cfg.contrast, U[:, 4]), 1.0)
    fire = U[:, 5] < cfg.noise_p
    t["noise"] = np.where(fire, span(cfg.noise_scale, U[:, 6]) / NOISE_SIGMA, 0.0)
    t["noise_per_channel"] = fire & (U[:, 7] < cfg.noise_per_channel_p)
    fire = U[:, 8] < cfg.multiply_p
    per = (U[:, 9] < cfg.multiply_per_channel_p)[:, None]
    m = span(cfg.multiply, np.where(per, U[:, 10:13], U[:, 10:11]))
    t["mult"] = np.where(fire[:, None], m, 1.0)
    return t


_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11; the Random123 constants), vectorised: counter is
    four and key two integers or arrays of them (taken mod 2^32, broadcast together); returns
    the four output words, uint32, stacked on a new first axis."""
    c = [np.asarray(v).astype(np.uint64) & _M32 for v in counter]
    k = [np.asarray(v).astype(np.uint64) & _M32 for v in key]
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    w0, w1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    sh = np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]            # 32 x 32 -> 64 bits, exact in uint64
        c = [(p1 >> sh) ^ c[1] ^ k[0], p1 & _M32, (p0 >> sh) ^ c[3] ^ k[1], p0 & _M32]
        k = [(k[0] + w0) & _M32, (k[1] + w1) & _M32]
    return np.stack(np.broadcast_arrays(*c)).astype(np.uint32)


def noise_sums(S, seed, ordinal):
    """s - 510 for every output pixel and Philox output word of one sample: int64 [4, S, S],
    s the sum of the word's four bytes. Key (seed lo, seed hi), counter (pixel lo, pixel hi,
    ordinal lo, ordinal hi), pixel = v * S + u."""
    seed, ordinal = int(seed) % 2 ** 64, int(ordinal) % 2 ** 64
    pix = np.arange(S * S, dtype=np.uint64)
    w = philox4x32_10((pix, pix >> np.uint64(32), ordinal & 0xFFFFFFFF, ordinal >> 32),
                      (seed & 0xFFFFFFFF, seed >> 32)).astype(np.int64)
    s = (w & 255) + ((w >> 8) & 255) + ((w >> 16) & 255) + (w >> 24)
    return (s - 510).reshape(4, S, S)


def augment_window(mask, valid, jitter):
    """instance_window's box with the three-way fallback, each side jittered, then +/- 16."""
    bx0, by0, bx1, by1 = instance_box(mask, valid)
    ax, ay = (bx1 - bx0) // JITTER_DIV, (by1 - by0) // JITTER_DIV
    j = [int(v) for v in jitter]
    return (bx0 - TRAIN_PAD + (j[0] * ax) // JITTER_ONE, by0 - TRAIN_PAD + (j[1] * ay) // JITTER_ONE,
            bx1 + TRAIN_PAD + (j[2] * ax) // JITTER_ONE, by1 + TRAIN_PAD + (j[3] * ay) // JITTER_ONE)


def rot_resample(img, window, valid, size, cos, sin):
    """crop_resample on a grid rotated about the crop's centre. Output (u, v) samples the crop
    at p = R (u + 0.5 - S/2, v + 0.5 - S/2) + S/2, R = [[cos, -sin], [sin, cos]] in float32, and
    p maps into the image like an output centre: ((p * scale) - 0.5) + lo. Taps at floor and
    floor + 1, not clamped into the window; a tap outside `valid` or the image counts as 0."""
    f32 = np.float32
    x0, y0, x1, y1 = (int(v) for v in window)
    c, s, half = f32(cos), f32(sin), f32(size) * f32(0.5)
    d = (np.arange(size).astype(f32) + f32(0.5)) - half
    du, dv = d[None, :], d[:, None]
    px = ((c * du) - (s * dv)) + half
    py = ((s * du) + (c * dv)) + half
    fx = ((px * (f32(x1 - x0) / f32(size))) - f32(0.5)) + f32(x0)
    fy = ((py * (f32(y1 - y0) / f32(size))) - f32(0.5)) + f32(y0)
    flx, fly = np.floor(fx), np.floor(fy)
    ix, iy = flx.astype(np.int64), fly.astype(np.int64)
    return blend_taps(img, valid, (iy, iy + 1), (ix, ix + 1), fy - fly, fx - flx)


def colour(q, params, seed, ordinal):
    """The photometric steps on a quantised crop q (uint8 [S, S, 3]), each re-quantised:
    contrast ((float)(q - 127) * alpha) + 127; noise (float)q + ((float)(s - 510) * k), only
    when k != 0; multiply (float)q * m_c. Returns uint8 [S, S, 3]."""
    f32 = np.float32
    S = q.shape[0]
    q = q.astype(np.int64)
    q = round_u8(((q - 127).astype(f32) * f32(params["contrast"])) + f32(127.0))
    k = f32(params["noise"])
    if k != 0:
        s = noise_sums(S, seed, ordinal)
        words = [0, 1, 2] if int(params["noise_per_channel"]) else [0, 0, 0]
        s = np.stack([s[w] for w in words], -1)
        q = round_u8(q.astype(f32) + (s.astype(f32) * k))
    q = round_u8(q.astype(f32) * np.asarray(params["mult"], f32)[None, None, :])
    return q.astype(np.uint8)


def augment_keypoints(kp, window, S, params):
    """[17, 3] float64 image coordinates -> crop coordinates: projected through the window;
    then, if rotated, R^T about (S/2, S/2) (the inverse of the pixels' map, so a keypoint stays
    on the pixel it marked); then, if flipped, x -> S - x and the left and right rows of
    ORDER_PART_NAMES exchanged, visibility included."""
    kp = np.array(kp, np.float64)
    x0, y0, x1, y1 = window
    kp[:, 0] = (kp[:, 0] - x0) * S / (x1 - x0)
    kp[:, 1] = (kp[:, 1] - y0) * S / (y1 - y0)
    kp[:, 2] = (kp[:, 2] > 0).astype(np.float64)
    c, s = np.float64(params["rot_cos"]), np.float64(params["rot_sin"])
    if not (c == 1.0 and s == 0.0):
        h = np.float64(S) * 0.5
        dx, dy = kp[:, 0] - h, kp[:, 1] - h
        kp[:, 0] = ((c * dx) + (s * dy)) + h
        kp[:, 1] = ((c * dy) - (s * dx)) + h
    if int(params["flip"]):
        kp = kp[MIRROR_PART]
        kp[:, 0] = np.float64(S) - kp[:, 0]
    return kp


def augment_crops(image, mask, valid, params, S, seed=0, ordinal=0):
    """The quantised crops of one sample: (window, image uint8 [S,S,3], mask uint8 [S,S])."""
    win = augment_window(mask, valid, params["jitter"])
    c, s = float(params["rot_cos"]), float(params["rot_sin"])
    if c == 1.0 and s == 0.0:
        img_c = crop_resample(image, win, valid, S)
        mask_c = crop_resample(mask, win, valid, S)
        if int(params["flip"]):
            img_c, mask_c = img_c[:, ::-1], mask_c[:, ::-1]
    else:
        u = np.arange(S)[::-1] if int(params["flip"]) else np.arange(S)
        img_c = rot_resample(image, win, valid, S, c, s)[:, u]
        mask_c = rot_resample(mask, win, valid, S, c, s)[:, u]
    return win, colour(img_c, params, seed, ordinal), np.ascontiguousarray(mask_c[:, :, 0])


def augment_sample(image, mask, valid, keypoints, params, S, seed=0, ordinal=0):
    """What isg_train_crop_aug computes for one decoded sample (image uint8 [H,W,3], mask uint8
    [H,W], valid, keypoints [17,3] in image coordinates) and one record `params` (a row of
    AUG_DTYPE). `ordinal` counts the samples augmented so far in the run: with `seed` it
    addresses the noise, so no two samples of a run share it. Returns (x float32 [3,S,S],
    mask float32 [1,S,S], keypoints float64 [17,3], window): with the identity record,
    InstanceCommonDataset.__getitem__'s tensors bit for bit."""
    f32 = np.float32
    win, img_c, mask_c = augment_crops(image, mask, valid, params, S, seed, ordinal)
    x = ((img_c.astype(f32) / f32(255.0) - f32(0.5)) / f32(0.5)).transpose(2, 0, 1).copy()
    m = (mask_c.astype(f32) / f32(255.0))[None]
    return x, m, augment_keypoints(keypoints, win, S, params), win


def augment_batch(raw, table, S, seed=0, ordinal0=0):
    """augment_sample over a list of raw samples: (x [n,3,S,S], mask [n,1,S,S], keypoints
    [n,17,3], windows int32 [n,4]); sample i has ordinal ordinal0 + i."""
    out = [augment_sample(im, mk, va, kp, table[i], S, seed, ordinal0 + i)
           for i, (im, mk, va, kp) in enumerate(raw)]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]),
            np.stack([o[2] for o in out]), np.array([o[3] for o in out], np.int32))


assert AUG_DTYPE.itemsize == 64 and len(MIRROR_PART) == N_PARTS
