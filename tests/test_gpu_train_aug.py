"""isg_train_crop_aug on the MI355X (csrc/train_crop.hip; gpu_batch.GpuBatcher(augment=...);
train_loop --gpu-crop --augment --flip) against its numpy statement augment.augment_sample, bit
for bit: both sides do the same single IEEE operations and the same integer Philox, so every
comparison is np.array_equal, rotations included."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from instancesegmentation_amd import _lib as L
from instancesegmentation_amd import augment as A
from instancesegmentation_amd import data as D
from instancesegmentation_amd.gpu_batch import aug_table

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

# the two five-sample batches of tests/test_gpu_train_crop.py, (W, H): odd sizes and offsets
SIZES = [(61, 83), (200, 150), (97, 97), (300, 260), (33, 47)]


def _masks_a(rng):
    m = [np.zeros((h, w), np.uint8) for w, h in SIZES]
    m[0][12:70, 10:50] = rng.choice(np.array([0, 1, 255], np.uint8), (58, 40))  # interior, valid = image
    m[1][0:80, 0:90] = 255                  # touches two borders: the window leaves the image
    m[2][5:60, 8:70] = rng.choice(np.array([3, 128], np.uint8), (55, 62))  # cut by valid
    m[3][10:40, 20:70] = 200                # wholly outside valid: the whole-mask fallback
    boxes = [(3, 5, 58, 78), (0, 0, 90, 80), (40, 30, 96, 95), (200, 150, 300, 260),
             (-10, -12, 45, 60)]            # (sample 4: all zero, the window is the image +/- 16)
    return m, boxes


def _masks_b(rng):
    m = [np.zeros((h, w), np.uint8) for w, h in SIZES]
    m[0][2:15, 1:12] = 9                    # outside valid = (17,21,61,83)
    m[1][40:110, 60:140] = rng.choice(np.array([0, 1, 255], np.uint8), (70, 80))
    m[3][0, 0] = 1                          # two corner pixels: the box needs stage A's reduction
    m[3][259, 299] = 255                    # across workgroups (sample 2: all zero)
    m[4][30:47, 20:33] = 200
    boxes = [(20, 30, 75, 95), (50, 30, 150, 120), (10, 10, 80, 90), (0, 0, 300, 260),
             (-5, -5, 50, 60)]
    return m, boxes


def _write(root, rng, masks, boxes):
    from PIL import Image
    for d in ("data", "image", "instance_mask"):
        os.makedirs(os.path.join(root, d))
    for i, ((w, h), m, box) in enumerate(zip(SIZES, masks, boxes)):
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


@pytest.fixture(scope="module")
def roots(tmp_path_factory):
    out = {}
    for name, fn, seed in (("a", _masks_a, 21), ("b", _masks_b, 22)):
        rng = np.random.default_rng(seed)
        masks, boxes = fn(rng)
        out[name] = str(tmp_path_factory.mktemp("aug_" + name))
        _write(out[name], rng, masks, boxes)
    return out


@functools.lru_cache(maxsize=None)
def _raw(root):
    ds = D.InstanceCommonDataset(root, raw=True)
    assert len(ds) == len(SIZES)
    return [ds[i] for i in range(len(ds))]


def records(n, **kw):
    t = A.identity_records(n)
    for k, v in kw.items():
        t[k] = v
    return t


def rot(deg=None, rad=None):
    a = np.radians(deg) if rad is None else rad
    return dict(rot_cos=np.cos(a), rot_sin=np.sin(a))


K_NOISE = np.float32(0.05 * 255 / A.NOISE_SIGMA)  # the largest gain draw_augment gives
CASES = {
    "jitter_out": dict(jitter=[-1024, -1024, 1024, 1024]),
    "jitter_in": dict(jitter=[1024, 1024, -1024, -1024]),
    "jitter_mixed": dict(jitter=[-1024, 1024, -1024, 1024]),
    "flip": dict(flip=1),
    "rot_25": rot(25.0),
    "rot_m25": rot(-25.0),
    "rot_90": dict(rot_cos=0.0, rot_sin=1.0),
    "rot_1e-3": rot(rad=1e-3),
    "rot_25_flip": dict(flip=1, **rot(25.0)),
    "contrast": dict(contrast=1.5),
    "noise": dict(noise=K_NOISE),
    "noise_per_channel": dict(noise=K_NOISE, noise_per_channel=1),
    "multiply": dict(mult=[0.8, 1.0, 1.2]),
    "all": dict(jitter=[700, -1024, 1024, -300], flip=1, contrast=0.75, noise=K_NOISE,
                noise_per_channel=1, mult=[1.2, 0.9, 1.1], **rot(-25.0)),
}


def _pack(raw, lead=1):
    """Arena bytes and the sample table: `lead` filler bytes, then per sample the mask and then
    the image, so images too start at odd offsets."""
    parts, off = [np.full(lead, 0xEE, np.uint8)], lead
    tab = (L.TrainSample * len(raw))()
    for s, (image, mask, valid, _) in zip(tab, raw):
        h, w = mask.shape
        s.mask_off, s.img_off, s.H, s.W = off, off + h * w, h, w
        s.valid[:] = [int(v) for v in valid]
        parts += [mask.reshape(-1), image.reshape(-1)]
        off += 4 * h * w
    return np.concatenate(parts), tab


class Buffers:
    """Outputs of one call with `guard` elements of a fill pattern on either side of each."""
    FILL = {"x": 7.5, "mask": -3.25, "kp": -123.0, "win": -77}

    def __init__(self, B, S, guard=64):
        self.B, self.S, self.g = B, S, guard
        shapes = {"x": ((B, 3, S, S), torch.float32), "mask": ((B, 1, S, S), torch.float32),
                  "kp": ((B, 17, 3), torch.float64), "win": ((B, 4), torch.int32)}
        self.flat, self.view = {}, {}
        for k, (shape, dt) in shapes.items():
            n = int(np.prod(shape))
            self.flat[k] = torch.full((n + 2 * guard,), self.FILL[k], dtype=dt, device=DEV)
            self.view[k] = self.flat[k][guard:guard + n].view(shape)
        self.work = torch.full((L.lib().isg_train_crop_workspace(B),), 0xFF, dtype=torch.uint8,
                               device=DEV)

    def run(self, raw, n, table=None, seed=0, ordinal0=0, lead=1):
        """table None: the plain isg_train_crop."""
        arena_np, tab = _pack(raw, lead)
        arena = torch.from_numpy(arena_np).to(DEV)
        kp = torch.from_numpy(np.stack([r[3] for r in raw])).to(DEV)
        v, lib = self.view, L.lib()
        tail = (kp.data_ptr(), n, self.B, self.S, self.work.data_ptr(), v["x"].data_ptr(),
                v["mask"].data_ptr(), v["kp"].data_ptr(), v["win"].data_ptr(), L.stream_ptr(DEV))
        if table is None:
            rc = lib.isg_train_crop(arena.data_ptr(), arena.numel(), tab, *tail)
        else:
            rc = lib.isg_train_crop_aug(arena.data_ptr(), arena.numel(), tab, aug_table(table),
                                        seed, ordinal0, *tail)
        torch.cuda.synchronize(DEV)
        assert rc == 0, lib.isg_last_error()

    def got(self):
        return tuple(self.view[k].cpu().numpy() for k in ("x", "mask", "kp", "win"))

    def check(self, ref, n):
        """Rows [0, n) equal ref = (x, mask, keypoints, windows) bit for bit; rows [n, B) and the
        guards keep their fill."""
        for k, r, got in zip(("x", "mask", "kp", "win"), ref, self.got()):
            if k == "kp":  # float64 compared as bits
                bad = (got[:n].view(np.int64) != r[:n].view(np.int64)).any(axis=(1, 2))
            else:
                assert got.dtype == r.dtype
                bad = (got[:n] != r[:n]).reshape(n, -1).any(axis=1)
            assert not bad.any(), f"{k}: samples {np.nonzero(bad)[0].tolist()} differ"
            assert (got[n:] == self.FILL[k]).all(), f"{k}: rows past n were written"
            flat, g = self.flat[k].cpu().numpy(), self.g
            assert (flat[:g] == self.FILL[k]).all() and (flat[len(flat) - g:] == self.FILL[k]).all(), \
                f"{k}: guard region written"


# S = 37: the 4-byte-store kernel (S % 4 != 0); S = 40: the 16-byte-store kernel
@pytest.mark.parametrize("S", [37, 40])
def test_identity_records_equal_the_plain_crop(roots, S):
    for name, lead in (("a", 1), ("b", 3)):
        raw = _raw(roots[name])
        plain, aug = Buffers(5, S), Buffers(5, S)
        plain.run(raw, 5, lead=lead)
        aug.run(raw, 5, records(5), seed=5, ordinal0=1 << 40, lead=lead)
        aug.check(plain.got(), 5)
        aug.check(A.augment_batch(raw, records(5), S), 5)


@pytest.mark.parametrize("S", [37, 40])
@pytest.mark.parametrize("case", sorted(CASES))
def test_each_augmentation_against_numpy(roots, S, case):
    """Every sample of both batches with the same record: rotated corners that leave valid and
    the image (a2-a4, b0), windows outside the image, the all-zero and the fallback masks."""
    seed, ordinal0 = 0x123456789, (1 << 32) - 2  # the ordinal's low word wraps inside the batch
    buf = Buffers(5, S)
    for name, lead in (("a", 1), ("b", 2)):
        raw = _raw(roots[name])
        table = records(5, **CASES[case])
        buf.run(raw, 5, table, seed, ordinal0, lead)
        buf.check(A.augment_batch(raw, table, S, seed, ordinal0), 5)


def _seventeen(roots):
    a, b = _raw(roots["a"]), _raw(roots["b"])
    raw = a + b + a + b[:2]
    table = A.draw_augment(np.random.Generator(np.random.PCG64(3)), 17, A.Augment(flip_p=0.5))
    for i, case in enumerate(sorted(CASES)):  # and every hand-made case once, 14 of them
        for k, v in CASES[case].items():
            table[i + 2][k] = v
    assert len({t.tobytes() for t in table}) == 17  # a different record each
    return raw, table


@pytest.mark.parametrize("S", [37, 40])
def test_seventeen_samples_cross_the_chunk(roots, S):
    """More samples than one launch takes (16): sample 16 reads record 16, not record 0."""
    raw, table = _seventeen(roots)
    buf = Buffers(17, S)
    buf.run(raw, 17, table, seed=9, ordinal0=100)
    ref = A.augment_batch(raw, table, S, 9, 100)
    buf.check(ref, 17)
    assert not np.array_equal(ref[0][16], A.augment_sample(*raw[16], table[0], S, 9, 116)[0])
    part = Buffers(20, S)  # n < B: rows 17..19 are left alone
    part.run(raw, 17, table, seed=9, ordinal0=100)
    part.check(ref, 17)
    few = Buffers(5, S)
    few.run(raw[:5], 3, table[:5], seed=9, ordinal0=100)
    few.check(ref, 3)


def test_misaligned_outputs_take_the_narrow_kernel(roots):
    """S = 40 with x and mask 20 bytes off 16-byte alignment: 4-byte stores, the same bits."""
    raw, table = _seventeen(roots)
    raw, table = raw[3:8], table[3:8]
    buf = Buffers(5, 40, guard=5)
    assert buf.view["x"].data_ptr() % 16 != 0 and buf.view["mask"].data_ptr() % 16 != 0
    buf.run(raw, 5, table, seed=2, ordinal0=7)
    buf.check(A.augment_batch(raw, table, 40, 2, 7), 5)


# ---- GpuBatcher and fit on the three-sample dataset of the existing fit test ----------------
@pytest.fixture(scope="module")
def small_root(tmp_path_factory):
    from tests.test_train_crop_cpu import write_dataset
    root = tmp_path_factory.mktemp("aug_ds")
    write_dataset(root, np.random.default_rng(31))
    return str(root)


def test_gpu_batcher_draws_and_counts(small_root):
    from instancesegmentation_amd.gpu_batch import GpuBatcher
    from instancesegmentation_amd.train_loop import _gpu_batches
    raw_ds = D.InstanceCommonDataset(small_root, raw=True)
    S, cfg = 40, A.Augment(flip_p=0.5)
    gb, plain = GpuBatcher(2, S, DEV, augment=cfg, seed=7), GpuBatcher(2, S, DEV)
    rng = np.random.Generator(np.random.PCG64(7))
    ordinal = 0
    for idx in ([0, 1], [2], [1, 0]):  # consecutive calls: the draws and the ordinal go on
        samples = [raw_ds[i] for i in idx]
        batch = D.raw_collate_fn(samples)
        x, kp, mask, n = gb.prepare(batch)
        table = A.draw_augment(rng, n, cfg)
        ref = A.augment_batch(samples, table, S, 7, ordinal)
        ordinal += n
        assert gb.ordinal == ordinal and gb.last_table.tobytes() == table.tobytes()
        assert np.array_equal(x.cpu().numpy(), ref[0]) and np.array_equal(mask.cpu().numpy(), ref[1])
        assert np.array_equal(kp.cpu().numpy().view(np.int64), ref[2].view(np.int64))
        assert np.array_equal(gb.windows[:n].cpu().numpy(), ref[3])
        # augment=False: the plain crop, no draw, the ordinal stays
        want = [t.clone() for t in plain.prepare(batch)[:3]]
        got = gb.prepare(batch, augment=False)
        assert gb.ordinal == ordinal
        for g, w in zip(got[:3], want):
            assert torch.equal(g, w)
    # the validation form of the loop's generator never augments
    loader = [D.raw_collate_fn([raw_ds[0], raw_ds[2]])]
    (xs, vmask, _), = list(_gpu_batches(loader, gb))
    want = plain.prepare(loader[0])
    assert torch.equal(xs[0], want[0]) and torch.equal(xs[1], want[1]) and torch.equal(vmask, want[2])
    assert gb.ordinal == ordinal
    # without an Augment the object is the old one; an Augment on the call overrides that
    assert plain.ordinal == 0
    plain.prepare(loader[0], augment=cfg)
    assert plain.ordinal == 2


def test_fit_with_augment_is_reproducible_and_differs(small_root, tmp_path):
    from instancesegmentation_amd import train_loop as TL

    def run(tag, *extra):
        torch.manual_seed(0)
        args = TL.parse_args(["--train-dataset-dir", small_root, "--val-dataset-dir", small_root,
                              "--checkpoint-dir", str(tmp_path / tag), "--batch-size", "2",
                              "--epoch", "4", "--val-iter", "2", "--show-iter", "1", "--cpu-num",
                              "0", "--max-steps", "3", "--gpu-crop", *extra])
        tr, _ = TL.fit(args, device=DEV)
        torch.cuda.synchronize(DEV)
        assert int(tr.step_dev.item()) == 3 and np.isfinite(tr.loss())
        return {k: v.detach().cpu().clone() for k, v in tr.model.state_dict().items()}

    aug = ("--augment", "--flip", "--augment-seed", "3")
    one, two, plain = run("aug1", *aug), run("aug2", *aug), run("plain")
    assert one.keys() == two.keys() == plain.keys()
    assert not [k for k in one if not torch.equal(one[k], two[k])]
    assert [k for k in one if not torch.equal(one[k], plain[k])]
