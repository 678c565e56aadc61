"""The augmentation contract in numpy (instancesegmentation_amd/augment.py), the flags and
the host-side argument checks of isg_train_crop_aug. No GPU."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

from instancesegmentation_amd import _lib as L
from instancesegmentation_amd import augment as A
from instancesegmentation_amd import data as D

# the five odd-sized samples of the train-crop tests (W, H), batch a of tests/test_gpu_train_crop.py
SIZES = [(61, 83), (200, 150), (97, 97), (300, 260), (33, 47)]
BOXES = [(3, 5, 58, 78), (0, 0, 90, 80), (40, 30, 96, 95), (200, 150, 300, 260), (-10, -12, 45, 60)]
S = 37


def _masks(rng):
    m = [np.zeros((h, w), np.uint8) for w, h in SIZES]
    m[0][12:70, 10:50] = rng.choice(np.array([0, 1, 255], np.uint8), (58, 40))  # interior blob
    m[1][0:80, 0:90] = 255                                  # touches the left and top borders
    m[2][5:60, 8:70] = rng.choice(np.array([3, 128], np.uint8), (55, 62))  # cut by valid
    m[3][10:40, 20:70] = 200                                # wholly outside valid: fallback box
    return m                                                # (sample 4: all zero, box = image)


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    from PIL import Image
    rng = np.random.default_rng(21)
    root = str(tmp_path_factory.mktemp("aug"))
    for d in ("data", "image", "instance_mask"):
        os.makedirs(os.path.join(root, d))
    for i, ((w, h), m, box) in enumerate(zip(SIZES, _masks(rng), BOXES)):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(
            os.path.join(root, "image", f"{i}.png"))
        Image.fromarray(m).save(os.path.join(root, "instance_mask", f"{i}.png"))
        kp = {name + "|sub_dict": {
            "status|keypoint_status": "invis" if j % 4 == 0 else "vis",
            "point|point_xy": [-30.5 + j * (w + 60) / 17 + 0.3 * i, h + 25.25 - j * (h + 50) / 16]}
            for j, name in enumerate(D.ORDER_PART_NAMES)}
        obj = {"box|box_xyxy": list(box), "class|class": "person",
               "instance_mask|mask_path": f"instance_mask/{i}.png", "body_keypoint|sub_dict": kp}
        with open(os.path.join(root, "data", f"{i}.json"), "w") as f:
            json.dump({"image|image_path": f"image/{i}.png", "object|sub_list": [obj]}, f)
    return root


@functools.lru_cache(maxsize=None)
def _raw(root):
    ds = D.InstanceCommonDataset(root, raw=True)
    assert len(ds) == len(SIZES)
    return [ds[i] for i in range(len(ds))]


@functools.lru_cache(maxsize=None)
def _plain(root):
    """InstanceCommonDataset.__getitem__ at S: (x, mask, keypoints) per sample, computed once."""
    ds = D.InstanceCommonDataset(root, with_heatmaps=False)
    ds.out_size = (S, S)
    got = [ds[i] for i in range(len(ds))]
    return [(g[0].numpy(), g[1].numpy(), g[2]["keypoints"].numpy()) for g in got]


def rec(**kw):
    r = A.identity_records(1)
    for k, v in kw.items():
        r[k] = v
    return r[0]


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(
        a.view(np.int64 if a.dtype == np.float64 else np.int32), b.view(
            np.int64 if b.dtype == np.float64 else np.int32))


# ---- Philox and the noise -------------------------------------------------------------
@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     "d16cfe09 94fdcceb 5001e420 24126ea1")])
def test_philox_known_answers(counter, key, want):
    out = A.philox4x32_10(counter, key)
    assert out.dtype == np.uint32 and " ".join(f"{int(w):08x}" for w in out) == want
    # vectorised: the same answer at one position of an array of counters
    c0 = np.array([5, counter[0], 7], np.uint64)
    out = A.philox4x32_10((c0, counter[1], counter[2], counter[3]), key)
    assert out.shape == (4, 3) and " ".join(f"{int(w):08x}" for w in out[:, 1]) == want


def test_noise_statistics():
    s = A.noise_sums(1024, seed=11, ordinal=3)  # 2^20 pixels, four words each
    assert s.shape == (4, 1024, 1024) and s.min() >= -510 and s.max() <= 510
    for w in range(4):
        assert abs(s[w].mean()) < 1.0
        assert abs(s[w].std() / 147.80 - 1.0) < 0.01
    assert abs(A.NOISE_SIGMA - 147.80) < 0.01


# ---- draw_augment ---------------------------------------------------------------------
def test_draw_augment_is_reproducible_and_in_range():
    cfg = A.Augment(flip_p=0.5)
    t = A.draw_augment(np.random.Generator(np.random.PCG64(5)), 10000, cfg)
    t2 = A.draw_augment(np.random.Generator(np.random.PCG64(5)), 10000, cfg)
    assert t.dtype == A.AUG_DTYPE and t.tobytes() == t2.tobytes()
    assert t.tobytes() != A.draw_augment(np.random.Generator(np.random.PCG64(6)), 10000, cfg).tobytes()
    assert t["jitter"].min() >= -1024 and t["jitter"].max() <= 1024 and t["jitter"].std() > 500
    assert np.abs(t["rot_cos"] ** 2 + t["rot_sin"] ** 2 - 1).max() < 1e-12
    ang = np.degrees(np.arctan2(t["rot_sin"], t["rot_cos"]))
    assert np.abs(ang).max() <= 25.0 + 1e-9 and ang.min() < -20 and ang.max() > 20
    rot = ~((t["rot_cos"] == 1.0) & (t["rot_sin"] == 0.0))
    con, noi, mul = t["contrast"] != 1, t["noise"] != 0, (t["mult"] != 1).any(1)
    for fired in (rot, con, noi, mul):  # Sometimes(0.6)
        assert abs(fired.mean() - 0.6) <= 0.03
    assert abs(t["flip"].mean() - 0.5) <= 0.03 and set(np.unique(t["flip"])) == {0, 1}
    assert t["contrast"].dtype == np.float32 and t["contrast"][con].min() >= 0.75
    assert t["contrast"][con].max() <= 1.5
    k_max = np.float32(0.05 * 255 / A.NOISE_SIGMA)
    assert t["noise"].min() >= 0 and t["noise"].max() <= k_max and (t["noise"][~noi] == 0).all()
    assert (t["noise_per_channel"][~noi] == 0).all()
    assert abs(t["noise_per_channel"][noi].mean() - 0.5) <= 0.03
    assert t["mult"][mul].min() >= np.float32(0.8) and t["mult"][mul].max() <= np.float32(1.2)
    per = (t["mult"][:, 0] != t["mult"][:, 1]) | (t["mult"][:, 0] != t["mult"][:, 2])
    assert abs(per[mul].mean() - 0.2) <= 0.03 and not per[~mul].any()
    assert (t["pad_"] == 0).all()


def test_augment_off_draws_identity_records():
    t = A.draw_augment(np.random.Generator(np.random.PCG64(1)), 64, A.Augment.off())
    assert t.tobytes() == A.identity_records(64).tobytes()
    assert ctypes.sizeof(L.TrainAug) == A.AUG_DTYPE.itemsize == 64
    for name, _ in L.TrainAug._fields_:  # the numpy record is the C struct, field for field
        assert getattr(L.TrainAug, name).offset == A.AUG_DTYPE.fields[name][1], name
    with pytest.raises(ValueError):
        A.Augment(jitter=0.3)
    with pytest.raises(ValueError):
        A.Augment(rotate_p=1.5)


# ---- augment_sample -------------------------------------------------------------------
def test_identity_equals_the_loader(root):
    for i, (raw, ref) in enumerate(zip(_raw(root), _plain(root))):
        x, m, kp, win = A.augment_sample(*raw, rec(), S, seed=9, ordinal=i)
        assert win == D.instance_window(raw[1], raw[2])
        assert same_bits(x, ref[0]) and same_bits(m, ref[1]) and same_bits(kp, ref[2]), i


def test_flip_only(root):
    for raw, ref in zip(_raw(root), _plain(root)):
        x, m, kp, _ = A.augment_sample(*raw, rec(flip=1), S)
        assert same_bits(x, np.ascontiguousarray(np.flip(ref[0], axis=-1)))
        assert same_bits(m, np.ascontiguousarray(np.flip(ref[1], axis=-1)))
        want = ref[2][A.MIRROR_PART].copy()
        want[:, 0] = S - want[:, 0]
        assert same_bits(kp, want)
    names = D.ORDER_PART_NAMES
    for j, o in enumerate(A.MIRROR_PART):
        assert A.MIRROR_PART[o] == j
        assert names[o] == (names[j].replace("left", "right") if "left" in names[j]
                            else names[j].replace("right", "left"))
    assert A.MIRROR_PART[names.index("nose")] == names.index("nose")
    # flipping twice is the identity: of the pixels exactly, of the rows and x = S - (S - x)
    kp = np.array(_plain(root)[0][2])
    kp[:, 0] = np.round(kp[:, 0] * 8) / 8  # dyadic, so that S - (S - x) is exact
    twice = kp[A.MIRROR_PART][A.MIRROR_PART]
    twice[:, 0] = S - (S - twice[:, 0])
    assert same_bits(twice, kp)
    x = _plain(root)[0][0]
    assert np.array_equal(np.flip(np.flip(x, -1), -1), x)


@pytest.mark.parametrize("side", range(4))
@pytest.mark.parametrize("j", [-1024, 0, 1024])
def test_jitter_only(root, side, j):
    jit = [0, 0, 0, 0]
    jit[side] = j
    for i, raw in enumerate(_raw(root)):
        image, mask, valid, kp = raw
        b = np.array(D.instance_window(mask, valid, pad=0))  # the box before the pad
        if i == 4:
            assert b.tolist() == [0, 0, 33, 47]              # all-zero mask: the image
        a = (b[2] - b[0]) // 5 if side % 2 == 0 else (b[3] - b[1]) // 5
        win = np.array(D.instance_window(mask, valid))
        win[side] += (j * a) // 1024
        assert abs(int((j * a) // 1024)) == (a if j else 0)
        x, m, k, got = A.augment_sample(image, mask, valid, kp, rec(jitter=jit), S)
        assert got == tuple(win) and got[2] > got[0] and got[3] > got[1]
        f32 = np.float32
        img_c = D.crop_resample(image, got, valid, S)
        assert same_bits(x, ((img_c.astype(f32) / f32(255) - f32(0.5)) / f32(0.5)).transpose(2, 0, 1).copy())
        assert same_bits(m, (D.crop_resample(mask, got, valid, S)[:, :, 0].astype(f32) / f32(255))[None])
        want = np.array(kp)
        want[:, 0] = (want[:, 0] - got[0]) * S / (got[2] - got[0])
        want[:, 1] = (want[:, 1] - got[1]) * S / (got[3] - got[1])
        want[:, 2] = want[:, 2] > 0
        assert same_bits(k, want)


def test_jitter_floor_division_of_negative_products():
    mask = np.zeros((40, 50), np.uint8)
    mask[5:28, 7:30] = 1                                      # box 23 x 23: a = 4
    win = A.augment_window(mask, (0, 0, 50, 40), [-1, 1, -513, 1023])
    assert win == (7 - 16 - 1, 5 - 16 + 0, 30 + 16 - 3, 28 + 16 + 3)  # floor, not truncation


def test_rotation_by_a_quarter_turn_is_rot90():
    """Scale 1 (an S x S window) inside valid: every output pixel is one source pixel."""
    rng = np.random.default_rng(2)
    S0 = 40
    image = rng.integers(0, 256, (60, 70, 3), dtype=np.uint8)
    mask = np.zeros((60, 70), np.uint8)
    mask[26:34, 31:39] = rng.choice(np.array([1, 255], np.uint8), (8, 8))
    mask[26, 31] = mask[33, 38] = 255                         # box (31,26,39,34): window 40 x 40
    valid = (0, 0, 70, 60)
    kp = np.zeros((17, 3))
    kp[:, 0] = 15 + 2.5 * np.arange(17)
    kp[:, 1] = 50 - 2.25 * np.arange(17)
    kp[:, 2] = np.arange(17) % 3 > 0
    px, pm, pk, win = A.augment_sample(image, mask, valid, kp, rec(), S0)
    assert win == (15, 10, 55, 50)
    rx, rm, rk, _ = A.augment_sample(image, mask, valid, kp, rec(rot_cos=0.0, rot_sin=1.0), S0)
    turns = [k for k in (1, 3) if np.array_equal(rx, np.rot90(px, k, axes=(1, 2)))]
    assert len(turns) == 1
    k = turns[0]
    assert np.array_equal(rm, np.rot90(pm, k, axes=(1, 2))) and pm.any()
    # np.rot90 with k = 1 takes the pixel at (x, y) to (y, S - x), with k = 3 to (S - y, x)
    want = np.stack([pk[:, 1], S0 - pk[:, 0]], 1) if k == 1 else np.stack([S0 - pk[:, 1], pk[:, 0]], 1)
    assert np.array_equal(rk[:, :2], want) and np.array_equal(rk[:, 2], pk[:, 2])


@pytest.mark.parametrize("deg", [25.0, -25.0])
@pytest.mark.parametrize("second_blob", [False, True])
def test_rotation_moves_pixels_and_keypoints_together(deg, second_blob):
    """A single 5 x 5 blob with a keypoint at its centre: after a rotation by 25 degrees the
    blob's centroid lies within 1 px of the keypoint. Alone, the blob sits at the centre of its
    own window, where a rotation moves nothing; with a second blob that widens the window it is
    off-centre, and pixel and keypoint have to travel together."""
    S0 = 64
    image = np.zeros((120, 140, 3), np.uint8)
    mask = np.zeros((120, 140), np.uint8)
    mask[30:35, 90:95] = 255
    if second_blob:
        mask[80:85, 30:35] = 255
    valid = (0, 0, 140, 120)
    kp = np.zeros((17, 3))
    kp[:, :2] = (92.5, 32.5)                                  # the blob's centre
    kp[:, 2] = 1
    r = rec(rot_cos=np.cos(np.radians(deg)), rot_sin=np.sin(np.radians(deg)))
    _, m, k, win = A.augment_sample(image, mask, valid, kp, r, S0)
    _, _, k0, _ = A.augment_sample(image, mask, valid, kp, rec(), S0)
    assert win == ((14, 14, 111, 101) if second_blob else (74, 14, 111, 51))
    ys, xs = np.nonzero(m[0] > 0)
    near = (xs + 0.5 - k[0, 0]) ** 2 + (ys + 0.5 - k[0, 1]) ** 2 < 8 ** 2  # the blob at the keypoint
    assert near.sum() >= 4 and (near.all() or second_blob)
    w = m[0][ys[near], xs[near]]
    cx, cy = ((xs[near] + 0.5) * w).sum() / w.sum(), ((ys[near] + 0.5) * w).sum() / w.sum()
    assert abs(cx - k[0, 0]) < 1.0 and abs(cy - k[0, 1]) < 1.0, (cx, cy, k[0])
    moved = np.hypot(*(k0[0, :2] - k[0, :2]))
    assert moved > 5.0 if second_blob else moved < 1e-9


def test_colour_steps(root):
    image, mask, valid, kp = _raw(root)[1]
    win, q0, _ = A.augment_crops(image, mask, valid, rec(), S)
    assert q0.dtype == np.uint8 and q0.min() == 0 and q0.max() > 200
    f32 = np.float32

    def norm(q):
        return ((q.astype(f32) / f32(255) - f32(0.5)) / f32(0.5)).transpose(2, 0, 1)

    # contrast and multiply: integers 0..255 before the normalisation, by the stated formulas
    for r in (rec(contrast=1.5), rec(contrast=0.75), rec(mult=[1.2, 1.2, 1.2]), rec(mult=[0.8, 1.0, 1.2])):
        _, q, _ = A.augment_crops(image, mask, valid, r, S)
        qi = q0.astype(np.int64)
        step1 = np.clip((((qi - 127).astype(f32) * f32(r["contrast"])) + f32(127) + f32(0.5)).astype(np.int64), 0, 255)
        want = np.clip((step1.astype(f32) * np.asarray(r["mult"], f32) + f32(0.5)).astype(np.int64), 0, 255)
        assert q.dtype == np.uint8 and np.array_equal(q, want)
        assert (q != q0).any()
        x = A.augment_sample(image, mask, valid, kp, r, S)[0]
        assert same_bits(x, norm(q).copy())
    # the mask is left alone by every colour step
    r = rec(contrast=1.4, noise=0.05, mult=[0.9, 1.1, 1.0])
    assert same_bits(A.augment_sample(image, mask, valid, kp, r, S, 1, 2)[1],
                     A.augment_sample(image, mask, valid, kp, rec(), S)[1])
    # noise without the per-channel bit: one integer for the three planes where none clamps
    k = f32(0.05)
    _, q, _ = A.augment_crops(image, mask, valid, rec(noise=k), S, seed=4, ordinal=17)
    d = q.astype(np.int64) - q0
    s = A.noise_sums(S, 4, 17)[0]
    want = (q0.astype(f32) + (s.astype(f32) * k)[:, :, None] + f32(0.5)).astype(np.int64)
    free = ((want >= 0) & (want <= 255)).all(-1)
    assert free.sum() > S * S // 4 and np.array_equal(np.clip(want, 0, 255), q)
    assert (d[free] == d[free][:, :1]).all() and np.abs(d[free]).max() > 5
    # with it the planes differ
    _, qp, _ = A.augment_crops(image, mask, valid, rec(noise=k, noise_per_channel=1), S, seed=4, ordinal=17)
    dp = qp.astype(np.int64) - q0
    assert np.array_equal(dp[..., 0], d[..., 0]) and (dp[free][:, 1] != dp[free][:, 0]).any()
    # the same (seed, ordinal) reproduces; ordinal + 1, or another seed, does not
    again = A.augment_crops(image, mask, valid, rec(noise=k), S, seed=4, ordinal=17)[1]
    assert np.array_equal(again, q)
    assert not np.array_equal(A.augment_crops(image, mask, valid, rec(noise=k), S, seed=4, ordinal=18)[1], q)
    assert not np.array_equal(A.augment_crops(image, mask, valid, rec(noise=k), S, seed=5, ordinal=17)[1], q)
    # a 64-bit ordinal and seed address the high counter and key words
    hi = A.augment_crops(image, mask, valid, rec(noise=k), S, seed=4 + 2 ** 32, ordinal=17 + 2 ** 32)[1]
    assert not np.array_equal(hi, q)


# ---- flags and host validation ----------------------------------------------------------
def test_augment_flags_need_gpu_crop(capsys):
    from instancesegmentation_amd import train_loop as TL
    base = ["--train-dataset-dir", "a", "--val-dataset-dir", "b", "--checkpoint-dir", "c"]
    args = TL.parse_args(base)
    assert args.augment is False and args.flip is False and args.augment_seed is None
    assert TL.augment_config(args) is None
    assert TL.augment_config(TL.parse_args(base + ["--gpu-crop"])) is None
    for extra in (["--augment"], ["--flip"], ["--augment-seed", "3"]):
        with pytest.raises(SystemExit) as e:
            TL.parse_args(base + extra)
        assert e.value.code != 0 and "--gpu-crop" in capsys.readouterr().err
    args = TL.parse_args(base + ["--gpu-crop", "--augment", "--flip", "--augment-seed", "3"])
    cfg = TL.augment_config(args)
    assert args.augment_seed == 3 and cfg.flip_p == 0.5 and cfg.rotate_p == 0.6 and cfg.jitter == 0.2
    assert TL.augment_config(TL.parse_args(base + ["--gpu-crop", "--augment"])) == A.Augment()
    only_flip = TL.augment_config(TL.parse_args(base + ["--gpu-crop", "--flip"]))
    assert only_flip == dataclass_replace(A.Augment.off(), flip_p=0.5)


def dataclass_replace(obj, **kw):
    import dataclasses
    return dataclasses.replace(obj, **kw)


def test_train_crop_aug_rejects_bad_arguments_before_any_hip_call():
    """isg_train_crop_aug's checks are host code over host records: they answer without a
    device (the pointers are never dereferenced)."""
    lib = L.lib()
    assert lib.isg_abi_version() == 14
    assert ctypes.sizeof(L.TrainAug) == lib.isg_record_size(21) == 64
    p = 0x1000  # any non-NULL value

    def call(arena=p, nbytes=4 * 6 * 5, sample=(0, 90, 6, 5), aug=None, no_aug=False, kp=p, n=1,
             B=1, S=8, work=p, x=p, mask=p, kpo=p, win=p):
        s = (L.TrainSample * 1)()
        s[0].img_off, s[0].mask_off, s[0].H, s[0].W = sample
        a = (L.TrainAug * 1)()
        a[0].rot_cos, a[0].contrast = 1.0, 1.0
        a[0].mult[:] = [1.0, 1.0, 1.0]
        for name, v in (aug or {}).items():
            if name in ("jitter", "mult"):
                getattr(a[0], name)[:] = v
            else:
                setattr(a[0], name, v)
        return lib.isg_train_crop_aug(arena, nbytes, s, None if no_aug else a, 7, 0, kp, n, B, S,
                                      work, x, mask, kpo, win, None)

    nan, inf = float("nan"), float("inf")
    bad_records = [dict(jitter=[1025, 0, 0, 0]), dict(jitter=[0, -1025, 0, 0]), dict(jitter=[0, 0, 0, 4096]),
                   dict(rot_cos=1.0, rot_sin=0.01), dict(rot_cos=0.0, rot_sin=0.0),
                   dict(rot_cos=nan), dict(rot_sin=inf), dict(contrast=-0.5), dict(contrast=nan),
                   dict(contrast=inf), dict(noise=-1e-3), dict(noise=nan), dict(noise=inf),
                   dict(mult=[1.0, -1.0, 1.0]), dict(mult=[1.0, 1.0, nan]), dict(mult=[inf, 1.0, 1.0]),
                   dict(flip=2), dict(noise_per_channel=-1)]
    for r in bad_records:
        assert call(aug=r) == -1, r  # ISG_ERR_INVALID
        assert b"train_crop_aug: record 0" in lib.isg_last_error(), r
    for kw in [dict(no_aug=True), dict(arena=None), dict(kp=None), dict(work=None), dict(x=None),
               dict(mask=None), dict(kpo=None), dict(win=None), dict(S=0), dict(S=-3), dict(n=2, B=1),
               dict(n=-1), dict(sample=(0, 90, 0, 5)), dict(sample=(0, 90, 6, -1)),
               dict(sample=(31, 90, 6, 5)), dict(sample=(0, 91, 6, 5)), dict(sample=(-1, 90, 6, 5)),
               dict(nbytes=119), dict(sample=(0, 90, 30000, 30000))]:
        assert call(**kw) == -1, kw
        assert b"train_crop_aug" in lib.isg_last_error(), kw
    assert call(n=0) == 0  # nothing to do: no launch, no error
    assert call(n=0, aug=dict(jitter=[9999, 0, 0, 0])) == 0  # records past n are not read
