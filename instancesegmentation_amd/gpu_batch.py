"""Training batches prepared on the GPU (csrc/train_crop.hip, isg_train_crop).

The loader's workers only decode (`InstanceCommonDataset(raw=True)`) and pack
(`data.raw_collate_fn`); a `GpuBatcher` uploads the packed uint8 pixels once per batch and
runs the mask box, the crop of image and mask and the keypoint projection on the device,
writing the normalised tensors where the caller wants them — the `Trainer`'s static input
buffers, so that `trainer.step()` follows without a copy:

    batcher = GpuBatcher(batch_size, 480, device)
    for raw in DataLoader(InstanceCommonDataset(d, raw=True), collate_fn=raw_collate_fn, ...):
        batcher.prepare(raw, trainer.inputs[0], trainer.inputs[1], trainer.target)
        loss = trainer.step()

The results equal `InstanceCommonDataset.__getitem__`'s bit for bit (tests/test_gpu_train_crop.py).
This path is eager: the arena grows with the largest batch seen, so it is not for capture.

With an `augment.Augment` the batcher draws one record per sample on the host
(`augment.draw_augment`, from its own `Generator(PCG64(seed))`) and calls isg_train_crop_aug:
jitter, flip, rotation and colour happen in the same kernel, bit for bit `augment.augment_sample`
(tests/test_gpu_train_aug.py). Without one, or with `prepare(..., augment=False)`, it is the
plain isg_train_crop.
"""
import ctypes

import numpy as np
import torch

from . import _lib as L
from .augment import AUG_DTYPE, draw_augment
from .data import N_PARTS


def sample_table(desc):
    """The isg_train_sample array (host memory) of a raw_collate_fn descriptor table."""
    rows = desc.tolist()
    tab = (L.TrainSample * len(rows))()
    for s, r in zip(tab, rows):
        s.img_off, s.mask_off, s.H, s.W = r[0], r[1], r[2], r[3]
        s.valid[:] = r[4:8]
    return tab


def aug_table(table):
    """The isg_train_aug array (host memory) of an augment.AUG_DTYPE table, copied."""
    table = np.ascontiguousarray(table, AUG_DTYPE)
    tab = (L.TrainAug * len(table))()
    ctypes.memmove(tab, table.ctypes.data, table.nbytes)
    return tab


class GpuBatcher:
    """Owns the device arena, the workspace and default output tensors of isg_train_crop for
    batches of up to `batch_size` samples at crop size `size`."""

    def __init__(self, batch_size, size=480, device="cuda", augment=None, seed=0):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("GpuBatcher runs on the MI355X only (no CPU path)")
        if batch_size <= 0 or size <= 0:
            raise ValueError(f"GpuBatcher: batch_size {batch_size}, size {size}")
        self.B, self.S = int(batch_size), int(size)
        dev, B, S = self.device, self.B, self.S
        self.arena = torch.empty(0, dtype=torch.uint8, device=dev)
        self.kp_in = torch.empty(B, N_PARTS, 3, dtype=torch.float64, device=dev)
        self.work = torch.empty(L.lib().isg_train_crop_workspace(B), dtype=torch.uint8, device=dev)
        self.windows = torch.empty(B, 4, dtype=torch.int32, device=dev)
        self.x = torch.empty(B, 3, S, S, dtype=torch.float32, device=dev)
        self.keypoints = torch.empty(B, N_PARTS, 3, dtype=torch.float64, device=dev)
        self.mask = torch.empty(B, 1, S, S, dtype=torch.float32, device=dev)
        # augmentation: the config, the seed (draws and noise key) and the count of samples
        # augmented so far (the noise counter's high half: no two samples of a run share noise)
        self.augment, self.seed, self.ordinal = augment, int(seed) % 2 ** 64, 0
        self.rng = np.random.Generator(np.random.PCG64(self.seed))

    def _dest(self, t, own, what):
        if t is None:
            return own
        if (t.shape != own.shape or t.dtype != own.dtype or t.device != own.device
                or not t.is_contiguous()):
            raise ValueError(f"GpuBatcher.prepare: {what} must be a contiguous {own.dtype} "
                             f"{tuple(own.shape)} tensor on {own.device}")
        return t

    def prepare(self, raw_batch, x=None, keypoints=None, mask=None, augment=None):
        """raw_batch: raw_collate_fn's (arena, desc, keypoints). Launches on the current
        stream and returns (x [n,3,S,S], keypoints [n,17,3], mask [n,1,S,S], n): views of the
        first n rows of the given tensors (each a full [batch_size, ...] buffer), or of this
        object's own, which the next prepare() overwrites. Rows past n are left alone.
        augment: None applies the constructor's Augment if there is one; False forces the plain
        crop (no draw, the ordinal stays); an Augment overrides the constructor's for this call."""
        arena, desc, kp = raw_batch
        n = int(desc.shape[0])
        if n > self.B:
            raise ValueError(f"GpuBatcher.prepare: {n} samples, batch_size {self.B}")
        x = self._dest(x, self.x, "x")
        keypoints = self._dest(keypoints, self.keypoints, "keypoints")
        mask = self._dest(mask, self.mask, "mask")
        if n == 0:
            return x[:0], keypoints[:0], mask[:0], 0
        cfg = self.augment if augment is None else (augment or None)
        nbytes = int(arena.numel())
        if nbytes > self.arena.numel():  # grow: the old arena's pending reads are stream-ordered
            self.arena = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            self.arena[:nbytes].copy_(arena, non_blocking=True)
            self.kp_in[:n].copy_(kp, non_blocking=True)
            if cfg is None:
                L.check(L.lib().isg_train_crop(
                    self.arena.data_ptr(), nbytes, sample_table(desc), self.kp_in.data_ptr(), n,
                    self.B, self.S, self.work.data_ptr(), x.data_ptr(), mask.data_ptr(),
                    keypoints.data_ptr(), self.windows.data_ptr(), L.stream_ptr(self.device)),
                    "train_crop")
            else:
                self.last_table = draw_augment(self.rng, n, cfg)
                L.check(L.lib().isg_train_crop_aug(
                    self.arena.data_ptr(), nbytes, sample_table(desc), aug_table(self.last_table),
                    self.seed, self.ordinal, self.kp_in.data_ptr(), n, self.B, self.S,
                    self.work.data_ptr(), x.data_ptr(), mask.data_ptr(), keypoints.data_ptr(),
                    self.windows.data_ptr(), L.stream_ptr(self.device)), "train_crop_aug")
                self.ordinal += n
        return x[:n], keypoints[:n], mask[:n], n
