"""Host side of the GPU batch path (no GPU): data.instance_window (the CPU statement of
stage A of isg_train_crop), the unchanged default sample, the raw dataset mode with
raw_collate_fn, and the argument checks that return before any HIP call."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from instancesegmentation_amd import _lib as L
from instancesegmentation_amd import data as D


def _blob(h, w, x0, y0, x1, y1, value=255):
    m = np.zeros((h, w), np.uint8)
    m[y0:y1, x0:x1] = value
    return m


WINDOW_CASES = {
    # name: (mask, valid, expected box before the pad)
    "interior": (_blob(60, 80, 20, 10, 50, 40), (0, 0, 80, 60), (20, 10, 50, 40)),
    "cut_by_valid": (_blob(60, 80, 20, 10, 50, 40), (30, 15, 80, 60), (30, 15, 50, 40)),
    "outside_valid": (_blob(60, 80, 2, 3, 12, 9), (30, 15, 80, 60), (2, 3, 12, 9)),
    "all_zero": (np.zeros((60, 80), np.uint8), (5, 5, 70, 50), (0, 0, 80, 60)),
    "pixel_at_origin": (_blob(60, 80, 0, 0, 1, 1, 1), (0, 0, 80, 60), (0, 0, 1, 1)),
    "pixel_at_far_corner": (_blob(60, 80, 79, 59, 80, 60, 7), (0, 0, 80, 60), (79, 59, 80, 60)),
}


@pytest.mark.parametrize("name", sorted(WINDOW_CASES))
def test_instance_window(name):
    mask, valid, box = WINDOW_CASES[name]
    assert D.instance_window(mask, valid) == (box[0] - 16, box[1] - 16, box[2] + 16, box[3] + 16)
    assert D.instance_window(mask, valid, pad=3) == (box[0] - 3, box[1] - 3, box[2] + 3, box[3] + 3)


def write_dataset(root, rng, sizes=((90, 120), (75, 101), (64, 83))):
    """A common-format dataset of len(sizes) images with one kept person each: image i is
    sizes[i] = (H, W), its box is off-centre (so `valid` is not the whole image), its mask
    mixes the values 1 and 255, and some keypoints are invisible or outside the window."""
    from PIL import Image
    os.makedirs(root / "data")
    os.makedirs(root / "image")
    os.makedirs(root / "instance_mask")
    for i, (H, W) in enumerate(sizes):
        Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(
            root / "image" / f"{i}.png")
        box = (2 + i, 1, W - 20 - 3 * i, H - 8)  # centre left of and above the image centre
        m = np.zeros((H, W), np.uint8)
        m[box[1] + 3:box[3] - 2, box[0]:box[2] - 4] = rng.choice(
            np.array([0, 1, 255], np.uint8), (box[3] - box[1] - 5, box[2] - box[0] - 4))
        Image.fromarray(m).save(root / "instance_mask" / f"{i}.png")
        kp = {}
        for j, name in enumerate(D.ORDER_PART_NAMES):
            st = "vis" if j % 3 else ("missing" if j > 12 else "invis")
            kp[name + "|sub_dict"] = {"status|keypoint_status": st,
                                      "point|point_xy": [7.25 * j - 20.0, H - 5.5 * j + 0.125 * i]}
        obj = {"box|box_xyxy": list(box), "class|class": "person",
               "instance_mask|mask_path": f"instance_mask/{i}.png", "body_keypoint|sub_dict": kp}
        with open(root / "data" / f"{i}.json", "w") as f:
            json.dump({"image|image_path": f"image/{i}.png", "object|sub_list": [obj]}, f)
    return sizes


def test_default_sample_is_unchanged(tmp_path):
    """ds[i] after the instance_window refactor: the tensors of the window re-derived inline,
    the way __getitem__ did it before (and test_common_dataset_reader does)."""
    from PIL import Image
    sizes = write_dataset(tmp_path, np.random.default_rng(3))
    ds = D.InstanceCommonDataset(str(tmp_path), with_heatmaps=False)
    assert len(ds) == len(sizes)
    for i, (H, W) in enumerate(sizes):
        image = np.asarray(Image.open(tmp_path / "image" / f"{i}.png").convert("RGB"))
        mask = np.asarray(Image.open(tmp_path / "instance_mask" / f"{i}.png").convert("L"))
        r = ds.results[i]
        valid = D.centring_valid([float(v) for v in D.ckey(r, "box")[:4]], H, W)
        assert valid != (0, 0, W, H)
        m = np.zeros_like(mask)
        m[valid[1]:valid[3], valid[0]:valid[2]] = mask[valid[1]:valid[3], valid[0]:valid[2]]
        ib = D.mask_box(m) or D.mask_box(mask) or (0, 0, W, H)
        win = (ib[0] - 16, ib[1] - 16, ib[2] + 16, ib[3] + 16)
        assert D.instance_window(mask, valid) == win
        img_c = D.crop_resample(image, win, valid, 480)
        mask_c = D.crop_resample(mask, win, valid, 480)[:, :, 0]
        x = ((img_c.astype(np.float32) / np.float32(255.0) - np.float32(0.5)) / np.float32(0.5))
        kp = D._keypoint_table(D.ckey(r, "body_keypoint"))
        kp[:, 0] = (kp[:, 0] - win[0]) * 480 / (win[2] - win[0])
        kp[:, 1] = (kp[:, 1] - win[1]) * 480 / (win[3] - win[1])
        kp[:, 2] = (kp[:, 2] > 0).astype(np.float64)
        img_t, mask_t, out = ds[i]
        assert np.array_equal(img_t.numpy(), x.transpose(2, 0, 1))
        assert np.array_equal(mask_t.numpy(), (mask_c.astype(np.float32) / np.float32(255.0))[None])
        assert np.array_equal(out["keypoints"].numpy().view(np.int64), kp.view(np.int64))
        assert np.array_equal(out["image"], img_c) and np.array_equal(out["mask"], mask_c)
        assert 0 < out["keypoints"][:, 2].sum() < 17


def test_raw_samples_and_collate_round_trip(tmp_path):
    from PIL import Image
    sizes = write_dataset(tmp_path, np.random.default_rng(4))
    ds = D.InstanceCommonDataset(str(tmp_path), raw=True)
    samples = [ds[i] for i in range(len(ds))]
    arena, desc, kp = D.raw_collate_fn(samples)
    assert arena.dtype == torch.uint8 and arena.dim() == 1
    assert desc.dtype == torch.int64 and tuple(desc.shape) == (len(sizes), len(D.RAW_DESC_COLS))
    assert kp.dtype == torch.float64 and tuple(kp.shape) == (len(sizes), 17, 3)
    assert arena.numel() == sum(4 * h * w for h, w in sizes)  # packed with no padding
    a = arena.numpy()
    end = 0
    for i, (H, W) in enumerate(sizes):
        image, mask, valid, k = samples[i]
        assert image.dtype == np.uint8 and image.shape == (H, W, 3)
        assert mask.dtype == np.uint8 and mask.shape == (H, W)
        assert np.array_equal(image, np.asarray(Image.open(tmp_path / "image" / f"{i}.png").convert("RGB")))
        assert np.array_equal(mask, np.asarray(Image.open(tmp_path / "instance_mask" / f"{i}.png")))
        r = ds.results[i]
        assert tuple(valid) == D.centring_valid([float(v) for v in D.ckey(r, "box")[:4]], H, W)
        assert np.array_equal(k, D._keypoint_table(D.ckey(r, "body_keypoint")))  # image coordinates
        io, mo, h, w = (int(v) for v in desc[i, :4])
        assert (io, mo, h, w) == (end, end + 3 * H * W, H, W)
        end = mo + H * W
        assert np.array_equal(a[io:io + 3 * H * W].reshape(H, W, 3), image)
        assert np.array_equal(a[mo:mo + H * W].reshape(H, W), mask)
        assert desc[i, 4:].tolist() == [int(v) for v in valid]
        assert np.array_equal(kp[i].numpy().view(np.int64), k.view(np.int64))
    assert any(int(o) % 4 for o in desc[:, :2].reshape(-1))  # offsets are not all aligned
    one = D.raw_collate_fn(samples[1:2])
    assert one[1][0, :2].tolist() == [0, 3 * sizes[1][0] * sizes[1][1]]


def test_gpu_batcher_needs_a_gpu():
    from instancesegmentation_amd.gpu_batch import GpuBatcher
    with pytest.raises(RuntimeError):
        GpuBatcher(2, 480, device="cpu")


def test_gpu_crop_flag_is_opt_in():
    from instancesegmentation_amd import train_loop as TL
    base = ["--train-dataset-dir", "a", "--val-dataset-dir", "b", "--checkpoint-dir", "c"]
    assert TL.parse_args(base).gpu_crop is False
    assert TL.parse_args(base + ["--gpu-crop"]).gpu_crop is True


def test_train_crop_rejects_bad_arguments_before_any_hip_call():
    """isg_train_crop's checks are host code over host descriptors: they answer without a
    device (the pointers are never dereferenced)."""
    lib = L.lib()
    assert lib.isg_train_crop_workspace(0) == 0 and lib.isg_train_crop_workspace(5) == 5 * 2048
    assert ctypes.sizeof(L.TrainSample) == lib.isg_record_size(20) == 40
    p = 0x1000  # any non-NULL value

    def call(arena=p, nbytes=4 * 6 * 5, sample=(0, 90, 6, 5), kp=p, n=1, B=1, S=8, work=p, x=p,
             mask=p, kpo=p, win=p):
        s = (L.TrainSample * 1)()
        s[0].img_off, s[0].mask_off, s[0].H, s[0].W = sample
        return lib.isg_train_crop(arena, nbytes, s, kp, n, B, S, work, x, mask, kpo, win, None)

    for kw in [dict(arena=None), dict(kp=None), dict(work=None), dict(x=None), dict(mask=None),
               dict(kpo=None), dict(win=None), dict(S=0), dict(S=-3), dict(n=2, B=1), dict(n=-1),
               dict(sample=(0, 90, 0, 5)), dict(sample=(0, 90, 6, -1)),
               dict(sample=(31, 90, 6, 5)),       # the image ends past the arena's end
               dict(sample=(0, 91, 6, 5)), dict(sample=(-1, 90, 6, 5)), dict(nbytes=119),
               dict(sample=(0, 90, 30000, 30000))]:
        assert call(**kw) == -1, kw  # ISG_ERR_INVALID
        assert b"train_crop" in lib.isg_last_error(), kw
    assert lib.isg_train_crop(p, 0, None, p, 0, 1, 8, p, p, p, p, p, None) == -1  # NULL samples
    assert call(n=0) == 0  # nothing to do: no launch, no error
