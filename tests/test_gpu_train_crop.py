"""Training batches prepared on the MI355X (csrc/train_crop.hip, isg_train_crop; gpu_batch.py;
train_loop --gpu-crop) against the loader's CPU path, bit for bit: the window is
data.instance_window's, the tensors and keypoints InstanceCommonDataset.__getitem__'s. Both
sides do the same single IEEE operations, so every comparison is np.array_equal."""
import functools

import numpy as np
import pytest
import torch

from instancesegmentation_amd import _lib as L
from instancesegmentation_amd import data as D
from tests.train_crop_cases import DEV, Buffers, _pack, _raw, make_roots

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def roots(tmp_path_factory):
    return make_roots(tmp_path_factory, "crop_")


@functools.lru_cache(maxsize=None)
def _reference(root, S):
    """The CPU path, computed once per (batch, S), in Buffers.check's order: x [5,3,S,S], mask
    [5,1,S,S], keypoints [5,17,3] from __getitem__ and windows [5,4] from instance_window."""
    ds = D.InstanceCommonDataset(root, with_heatmaps=False)
    ds.out_size = (S, S)
    got = [ds[i] for i in range(len(ds))]
    win = np.array([D.instance_window(mask, valid) for _, mask, valid, _ in _raw(root)], np.int32)
    return (np.stack([g[0].numpy() for g in got]), np.stack([g[1].numpy() for g in got]),
            np.stack([g[2]["keypoints"].numpy() for g in got]), win)


def test_reference_cases_are_the_intended_ones(roots):
    wa = _reference(roots["a"], 37)[3].tolist()
    assert wa[0] == [10 - 16, 12 - 16, 50 + 16, 70 + 16]
    assert wa[1] == [-16, -16, 90 + 16, 80 + 16]
    assert wa[2] == [19 - 16, 14 - 16, 70 + 16, 60 + 16]
    assert wa[3] == [20 - 16, 10 - 16, 70 + 16, 40 + 16]
    assert wa[4] == [-16, -16, 33 + 16, 47 + 16]
    wb = _reference(roots["b"], 37)[3].tolist()
    assert wb[0] == [1 - 16, 2 - 16, 12 + 16, 15 + 16]
    assert wb[2] == [-16, -16, 97 + 16, 97 + 16]
    assert wb[3] == [-16, -16, 300 + 16, 260 + 16]
    assert wb[4] == [20 - 16, 30 - 16, 33 + 16, 47 + 16]


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
