"""Training batches prepared on the MI355X (csrc/train_crop.hip, isg_train_crop; gpu_batch.py;
train_loop --gpu-crop) against the loader's CPU path, bit for bit: the window is
data.instance_window's, the tensors and keypoints InstanceCommonDataset.__getitem__'s. Both
sides do the same single IEEE operations, so every comparison is np.array_equal."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

from instancesegmentation_amd import _lib as L
from instancesegmentation_amd import data as D

pytestmark = pytest.mark.gpu
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


@pytest.fixture(scope="module")
def roots(tmp_path_factory):
    out = {}
    for name, fn, seed in (("a", _masks_a, 21), ("b", _masks_b, 22)):
        rng = np.random.default_rng(seed)
        masks, boxes = fn(rng)
        out[name] = str(tmp_path_factory.mktemp("crop_" + name))
        _write(out[name], rng, masks, boxes)
    return out


@functools.lru_cache(maxsize=None)
def _raw(root):
    ds = D.InstanceCommonDataset(root, raw=True)
    assert len(ds) == len(SIZES)
    return [ds[i] for i in range(len(ds))]


@functools.lru_cache(maxsize=None)
def _reference(root, S):
    """The CPU path, computed once per (batch, S): windows [5,4], x [5,3,S,S], mask
    [5,1,S,S], keypoints [5,17,3] from __getitem__ and instance_window."""
    ds = D.InstanceCommonDataset(root, with_heatmaps=False)
    ds.out_size = (S, S)
    got = [ds[i] for i in range(len(ds))]
    win = np.array([D.instance_window(mask, valid) for _, mask, valid, _ in _raw(root)], np.int32)
    return (win, np.stack([g[0].numpy() for g in got]), np.stack([g[1].numpy() for g in got]),
            np.stack([g[2]["keypoints"].numpy() for g in got]))


def test_reference_cases_are_the_intended_ones(roots):
    wa = _reference(roots["a"], 37)[0].tolist()
    assert wa[0] == [10 - 16, 12 - 16, 50 + 16, 70 + 16]
    assert wa[1] == [-16, -16, 90 + 16, 80 + 16]
    assert wa[2] == [19 - 16, 14 - 16, 70 + 16, 60 + 16]
    assert wa[3] == [20 - 16, 10 - 16, 70 + 16, 40 + 16]
    assert wa[4] == [-16, -16, 33 + 16, 47 + 16]
    wb = _reference(roots["b"], 37)[0].tolist()
    assert wb[0] == [1 - 16, 2 - 16, 12 + 16, 15 + 16]
    assert wb[2] == [-16, -16, 97 + 16, 97 + 16]
    assert wb[3] == [-16, -16, 300 + 16, 260 + 16]
    assert wb[4] == [20 - 16, 30 - 16, 33 + 16, 47 + 16]


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

    def __init__(self, B, S, guard):
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

    def run(self, raw, n, lead=1):
        arena_np, tab = _pack(raw, lead)
        arena = torch.from_numpy(arena_np).to(DEV)
        kp = torch.from_numpy(np.stack([r[3] for r in raw])).to(DEV)
        v = self.view
        rc = L.lib().isg_train_crop(arena.data_ptr(), arena.numel(), tab, kp.data_ptr(), n, self.B,
                                    self.S, self.work.data_ptr(), v["x"].data_ptr(),
                                    v["mask"].data_ptr(), v["kp"].data_ptr(), v["win"].data_ptr(),
                                    L.stream_ptr(DEV))
        torch.cuda.synchronize(DEV)
        return rc

    def check(self, ref, n):
        """Rows [0, n) equal the reference, rows [n, B) and the guards keep their fill."""
        for k, r in zip(("win", "x", "mask", "kp"), ref):
            got = self.view[k].cpu().numpy()
            if k == "kp":  # float64 compared as bits
                assert np.array_equal(got[:n].view(np.int64), r[:n].view(np.int64)), k
            else:
                assert got.dtype == r.dtype and np.array_equal(got[:n], r[:n]), k
            assert (got[n:] == self.FILL[k]).all(), f"{k}: rows past n were written"
            flat, g = self.flat[k].cpu().numpy(), self.g
            assert (flat[:g] == self.FILL[k]).all() and (flat[len(flat) - g:] == self.FILL[k]).all(), \
                f"{k}: guard region written"


# S = 480 and 37 with 16-byte aligned outputs (the 16-byte-store kernel and, S % 4 != 0, the
# 4-byte one); S = 36 with outputs 20 bytes off alignment (the 4-byte kernel by alignment)
@pytest.mark.parametrize("S,guard", [(480, 64), (37, 64), (36, 5)])
def test_train_crop_bit_exact(roots, S, guard):
    buf = Buffers(5, S, guard)
    assert buf.run(_raw(roots["a"]), 5) == 0, L.lib().isg_last_error()
    buf.check(_reference(roots["a"], S), 5)
    # the same buffers and workspace again with another batch: nothing is left of the first
    assert buf.run(_raw(roots["b"]), 5, lead=3) == 0, L.lib().isg_last_error()
    buf.check(_reference(roots["b"], S), 5)
    assert buf.run(_raw(roots["a"]), 5, lead=0) == 0, L.lib().isg_last_error()
    buf.check(_reference(roots["a"], S), 5)


def test_train_crop_partial_batch_leaves_the_rest(roots):
    buf = Buffers(5, 37, 64)
    assert buf.run(_raw(roots["a"]), 3) == 0, L.lib().isg_last_error()
    buf.check(_reference(roots["a"], 37), 3)


def test_train_crop_empty_batch_and_bad_arguments(roots):
    lib = L.lib()
    buf = Buffers(5, 37, 64)
    assert buf.run(_raw(roots["a"]), 0) == 0
    buf.check(_reference(roots["a"], 37), 0)  # nothing written anywhere
    assert (buf.work.cpu() == 0xFF).all()      # not even the workspace: nothing was launched
    arena_np, tab = _pack(_raw(roots["a"]))
    arena = torch.from_numpy(arena_np).to(DEV)
    kp = torch.from_numpy(np.stack([r[3] for r in _raw(roots["a"])])).to(DEV)
    v = buf.view
    good = dict(arena=arena.data_ptr(), nbytes=arena.numel(), tab=tab, kp=kp.data_ptr(), n=5, B=5,
                S=37, work=buf.work.data_ptr(), x=v["x"].data_ptr(), mask=v["mask"].data_ptr(),
                kpo=v["kp"].data_ptr(), win=v["win"].data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        return lib.isg_train_crop(a["arena"], a["nbytes"], a["tab"], a["kp"], a["n"], a["B"], a["S"],
                                  a["work"], a["x"], a["mask"], a["kpo"], a["win"], L.stream_ptr(DEV))

    bad_h = (L.TrainSample * 5)(*tab)
    bad_h[2].H = 0
    bad_w = (L.TrainSample * 5)(*tab)
    bad_w[4].W = -4
    past = (L.TrainSample * 5)(*tab)
    past[4].img_off += 1  # the last image now ends one byte past the arena
    for kw in [dict(arena=None), dict(tab=None), dict(kp=None), dict(work=None), dict(x=None),
               dict(mask=None), dict(kpo=None), dict(win=None), dict(S=0), dict(n=6), dict(n=-1),
               dict(tab=bad_h), dict(tab=bad_w), dict(tab=past), dict(nbytes=arena.numel() - 1)]:
        assert call(**kw) == -1, kw  # ISG_ERR_INVALID
        assert b"train_crop" in lib.isg_last_error(), kw
    torch.cuda.synchronize(DEV)
    buf.check(_reference(roots["a"], 37), 0)  # the refused calls wrote nothing
    assert call() == 0
    torch.cuda.synchronize(DEV)
    buf.check(_reference(roots["a"], 37), 5)


# ---- GpuBatcher and fit(--gpu-crop) on a three-sample dataset ---------------------------
@pytest.fixture(scope="module")
def small_root(tmp_path_factory):
    from tests.test_train_crop_cpu import write_dataset
    root = tmp_path_factory.mktemp("crop_ds")
    write_dataset(root, np.random.default_rng(31))
    return str(root)


def test_gpu_batcher_prepare(small_root):
    """Batch size 2 over three samples: one full and one partial batch, into the batcher's
    own tensors and into destination tensors, against the collated CPU batch."""
    from instancesegmentation_amd.gpu_batch import GpuBatcher
    cpu = D.InstanceCommonDataset(small_root, with_heatmaps=False)
    raw = D.InstanceCommonDataset(small_root, raw=True)
    S = cpu.out_size[0]
    gb = GpuBatcher(2, S, DEV)
    dst = [torch.full((2, 3, S, S), 9.0, device=DEV), torch.full((2, 17, 3), 9.0, dtype=torch.float64, device=DEV),
           torch.full((2, 1, S, S), 9.0, device=DEV)]
    for idx in ([0, 1], [2]):
        img_ts, mask_ts, outs = D.collate_fn([cpu[i] for i in idx])
        kp_ref = torch.stack([o["keypoints"] for o in outs])
        batch = D.raw_collate_fn([raw[i] for i in idx])
        x, kp, mask, n = gb.prepare(batch)
        assert n == len(idx) and x.shape[0] == kp.shape[0] == mask.shape[0] == n
        assert x.data_ptr() == gb.x.data_ptr() and mask.data_ptr() == gb.mask.data_ptr()
        assert torch.equal(x.cpu(), img_ts) and torch.equal(mask.cpu(), mask_ts)
        assert torch.equal(kp.cpu().view(torch.int64), kp_ref.view(torch.int64))
        x2, kp2, mask2, n2 = gb.prepare(batch, *dst)
        assert n2 == n
        for view, d in zip((x2, kp2, mask2), dst):  # the returned views alias the destinations
            assert view.data_ptr() == d.data_ptr() and view.shape[1:] == d.shape[1:]
        assert torch.equal(dst[0][:n].cpu(), img_ts) and torch.equal(dst[2][:n].cpu(), mask_ts)
        assert torch.equal(dst[1][:n].cpu().view(torch.int64), kp_ref.view(torch.int64))
    # the partial batch left row 1 of the destinations as the full batch wrote it
    img_ts, mask_ts, _ = D.collate_fn([cpu[1]])
    assert torch.equal(dst[0][1:].cpu(), img_ts) and torch.equal(dst[2][1:].cpu(), mask_ts)
    with pytest.raises(ValueError):
        gb.prepare(batch, dst[0][:1])  # not a full [batch_size, ...] buffer
    with pytest.raises(ValueError):
        gb.prepare(D.raw_collate_fn([raw[i] for i in (0, 1, 2)]))


def test_fit_with_gpu_crop_trains_the_same_model(small_root, tmp_path):
    """Three steps of fit() at batch size 2 from the same seed: the model after --gpu-crop
    equals the model after the default loader bit for bit (the step is bitwise
    reproducible and the two loaders feed bit-equal batches)."""
    from instancesegmentation_amd import train_loop as TL

    def run(tag, *extra):
        torch.manual_seed(0)
        args = TL.parse_args(["--train-dataset-dir", small_root, "--val-dataset-dir", small_root,
                              "--checkpoint-dir", str(tmp_path / tag), "--batch-size", "2",
                              "--epoch", "4", "--val-iter", "2", "--show-iter", "1", "--cpu-num",
                              "0", "--max-steps", "3", *extra])
        tr, history = TL.fit(args, device=DEV)
        torch.cuda.synchronize(DEV)
        assert int(tr.step_dev.item()) == 3 and np.isfinite(tr.loss())
        return {k: v.detach().cpu().clone() for k, v in tr.model.state_dict().items()}, history

    ref, h_ref = run("cpu")
    got, h_got = run("gpu", "--gpu-crop")
    assert h_got == h_ref and len(h_ref) >= 1
    assert ref.keys() == got.keys()
    diff = [k for k in ref if not torch.equal(ref[k], got[k])]
    assert not diff, diff
