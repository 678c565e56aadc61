"""What tests/test_gpu_train_crop.py and tests/test_gpu_train_aug.py share: two five-sample
datasets that between them hold every window case, their raw samples, an arena packed by hand,
and the guard-banded output buffers of one isg_train_crop / isg_train_crop_aug call."""
import functools
import json
import os

import numpy as np
import torch

from instancesegmentation_amd import _lib as L
from instancesegmentation_amd import data as D
from instancesegmentation_amd.gpu_batch import aug_table

DEV = torch.device("cuda", 0)

# (W, H) of the five samples: odd sizes, so masks and images start at odd byte offsets
SIZES = [(61, 83), (200, 150), (97, 97), (300, 260), (33, 47)]


def _masks_a(rng):
    """One case per sample (the boxes put `valid` where the case needs it)."""
    m = [np.zeros((h, w), np.uint8) for w, h in SIZES]
    # (a) interior blob mixing 0, 1 and 255: non-zero is the rule, not >= 128; valid = image
    m[0][12:70, 10:50] = rng.choice(np.array([0, 1, 255], np.uint8), (58, 40))
    # (b) blob touching the left and top borders: the window reaches outside the image
    m[1][0:80, 0:90] = 255
    # (c) box centre far off-centre: valid = (19,14,97,97) cuts the blob
    m[2][5:60, 8:70] = rng.choice(np.array([3, 128], np.uint8), (55, 62))
    # (d) blob wholly outside valid = (100,75,300,260): the whole-mask box is the fallback
    m[3][10:40, 20:70] = 200
    # (e) all-zero mask: the window is the image +/- 16
    boxes = [(3, 5, 58, 78), (0, 0, 90, 80), (40, 30, 96, 95), (200, 150, 300, 260),
             (-10, -12, 45, 60)]
    return m, boxes


def _masks_b(rng):
    """A second batch on the same images. The 300 x 260 sample has exactly two set pixels at
    opposite corners: they lie in different workgroups of stage A, so its box exists only
    after the reduction across workgroups."""
    m = [np.zeros((h, w), np.uint8) for w, h in SIZES]
    m[0][2:15, 1:12] = 9                   # outside valid = (17,21,61,83)
    m[1][40:110, 60:140] = rng.choice(np.array([0, 1, 255], np.uint8), (70, 80))
    m[3][0, 0] = 1                         # (sample 2: all zero)
    m[3][259, 299] = 255
    m[4][30:47, 20:33] = 200               # touches the right and bottom borders
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
        kp = {}  # parts with visible = 0 and coordinates outside the window are projected too
        for j, name in enumerate(D.ORDER_PART_NAMES):
            kp[name + "|sub_dict"] = {
                "status|keypoint_status": "invis" if j % 4 == 0 else "vis",
                "point|point_xy": [-30.5 + j * (w + 60) / 17 + 0.3 * i, h + 25.25 - j * (h + 50) / 16]}
        obj = {"box|box_xyxy": list(box), "class|class": "person",
               "instance_mask|mask_path": f"instance_mask/{i}.png", "body_keypoint|sub_dict": kp}
        with open(os.path.join(root, "data", f"{i}.json"), "w") as f:
            json.dump({"image|image_path": f"image/{i}.png", "object|sub_list": [obj]}, f)


def make_roots(tmp_path_factory, prefix):
    """{"a": dir, "b": dir}: the two datasets written under fresh temporary directories."""
    out = {}
    for name, fn, seed in (("a", _masks_a, 21), ("b", _masks_b, 22)):
        rng = np.random.default_rng(seed)
        masks, boxes = fn(rng)
        out[name] = str(tmp_path_factory.mktemp(prefix + name))
        _write(out[name], rng, masks, boxes)
    return out


@functools.lru_cache(maxsize=None)
def _raw(root):
    ds = D.InstanceCommonDataset(root, raw=True)
    assert len(ds) == len(SIZES)
    return [ds[i] for i in range(len(ds))]


def _pack(raw, lead=1):
    """Arena bytes and the sample table, packed by hand: `lead` filler bytes, then per sample
    the mask and then the image, so images too start at odd offsets."""
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
        # 0xFF everywhere: the call must initialise its workspace itself
        self.work = torch.full((L.lib().isg_train_crop_workspace(B),), 0xFF, dtype=torch.uint8,
                               device=DEV)

    def run(self, raw, n, table=None, seed=0, ordinal0=0, lead=1):
        """table None: the plain isg_train_crop. Returns the call's code, which is 0."""
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
        return rc

    def got(self):
        return tuple(self.view[k].cpu().numpy() for k in ("x", "mask", "kp", "win"))

    def check(self, ref, n):
        """Rows [0, n) equal ref = (x, mask, keypoints, windows) bit for bit; rows [n, B) and the
        guards keep their fill."""
        for k, r, got in zip(("x", "mask", "kp", "win"), ref, self.got()):
            if k == "kp":  # float64 compared as bits
                bad = got[:n].view(np.int64) != r[:n].view(np.int64)
            else:
                assert got.dtype == r.dtype
                bad = got[:n] != r[:n]
            bad = bad.any(axis=tuple(range(1, bad.ndim)))
            assert not bad.any(), f"{k}: samples {np.nonzero(bad)[0].tolist()} differ"
            assert (got[n:] == self.FILL[k]).all(), f"{k}: rows past n were written"
            flat, g = self.flat[k].cpu().numpy(), self.g
            assert (flat[:g] == self.FILL[k]).all() and (flat[len(flat) - g:] == self.FILL[k]).all(), \
                f"{k}: guard region written"
