"""isg_train_crop_aug on the MI355X (csrc/train_crop.hip; gpu_batch.GpuBatcher(augment=...);
train_loop --gpu-crop --augment --flip) against its numpy statement augment.augment_sample, bit
for bit: both sides do the same single IEEE operations and the same integer Philox, so every
comparison is np.array_equal, rotations included."""
import numpy as np
import pytest
import torch

from instancesegmentation_amd import augment as A
from instancesegmentation_amd import data as D
from tests.train_crop_cases import DEV, Buffers, _raw, make_roots

pytestmark = pytest.mark.gpu


# the two five-sample batches of tests/test_gpu_train_crop.py
@pytest.fixture(scope="module")
def roots(tmp_path_factory):
    return make_roots(tmp_path_factory, "aug_")


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
