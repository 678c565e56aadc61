"""What preparing a training batch costs on the GPU and on the host (gpu_batch.GpuBatcher,
isg_train_crop) at batch 8, S = 480, 640 x 480 sources (JPEG image + PNG mask, written to a
temporary common-format dataset from a seed).

    python tools/batch_bench.py [--rounds 20] [--reps 10] [--cpu-num 2] [--fit-steps 30]
        (i)   GpuBatcher.prepare per batch, device events: the whole call (upload + kernels)
              and the kernels alone on an arena already uploaded;
        (iii) Trainer.step at the same batch in the same process, rounds alternating;
        (iv)  host cost per batch of the two loaders, wall clock: __getitem__ + collate_fn
              against raw decode + raw_collate_fn + the upload;
        (v)   samples/s of a short fit() with and without --gpu-crop at the same --cpu-num
              (host clock after each synchronised step, the first two left out).
    python tools/batch_bench.py --replay 200
        only repeats the kernels: the command to put under `rocprofv3 --kernel-trace --stats`
        (with `--output-format csv`) for stage A and stage B separately;
    python tools/batch_bench.py --summarise DIR
        (i, ii) reads that trace: train_box_kernel (stage A) and train_crop_kernel (stage B)
        time per launch, and stage B's write rate (4 planes x S^2 x 4 B x B) over the
        6.29 TB/s HBM streaming rate measured on this part (8.0 TB/s spec). Needs no GPU.

    python tools/batch_bench.py --augment [--rounds 20] [--reps 10] [--fit-steps 30]
        isg_train_crop_aug beside isg_train_crop in one run, rounds alternating: the kernels
        of the plain call, of the augmented call with identity records and with every
        augmentation on (jitter, flip, rotation, contrast, per-channel noise, multiply), by
        device events; then fit --gpu-crop, fit --gpu-crop --augment --flip and fit --gpu-crop
        again at the same --cpu-num (the two plain legs give the run-to-run spread).
        With --replay N it repeats each of the three N times in that order, and --summarise
        then splits train_crop_aug_kernel's launches into the identity and the full half.

Prints one JSON line per mode.
"""
import argparse
import csv
import glob
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12
B, S, SRC_W, SRC_H = 8, 480, 640, 480


def write_dataset(root, n, seed=0):
    """n images of SRC_W x SRC_H with one person each: an elliptical mask, a box round it,
    17 keypoints inside it."""
    from PIL import Image

    from instancesegmentation_amd.data import ORDER_PART_NAMES
    rng = np.random.default_rng(seed)
    for d in ("data", "image", "instance_mask"):
        os.makedirs(os.path.join(root, d))
    yy, xx = np.mgrid[0:SRC_H, 0:SRC_W]
    for i in range(n):
        # smooth content: a JPEG of noise would time the entropy decoder, not a photograph
        low = rng.integers(0, 256, (SRC_H // 16, SRC_W // 16, 3), dtype=np.uint8)
        img = Image.fromarray(low).resize((SRC_W, SRC_H), Image.BILINEAR)
        img.save(os.path.join(root, "image", f"{i}.jpg"), quality=90)
        cx, cy = rng.uniform(0.3, 0.7) * SRC_W, rng.uniform(0.35, 0.65) * SRC_H
        ax, ay = rng.uniform(0.12, 0.25) * SRC_W, rng.uniform(0.25, 0.4) * SRC_H
        m = ((((xx - cx) / ax) ** 2 + ((yy - cy) / ay) ** 2) <= 1.0).astype(np.uint8) * 255
        Image.fromarray(m).save(os.path.join(root, "instance_mask", f"{i}.png"))
        kp = {name + "|sub_dict": {"status|keypoint_status": "vis" if rng.uniform() < 0.8 else "invis",
                                   "point|point_xy": [cx + rng.uniform(-0.8, 0.8) * ax,
                                                      cy + rng.uniform(-0.8, 0.8) * ay]}
              for name in ORDER_PART_NAMES}
        box = [int(cx - ax), int(cy - ay), int(cx + ax) + 1, int(cy + ay) + 1]
        obj = {"box|box_xyxy": box, "class|class": "person",
               "instance_mask|mask_path": f"instance_mask/{i}.png", "body_keypoint|sub_dict": kp}
        with open(os.path.join(root, "data", f"{i}.json"), "w") as f:
            json.dump({"image|image_path": f"image/{i}.jpg", "object|sub_list": [obj]}, f)


def stats(xs):
    xs = np.asarray(xs, np.float64)
    return {"median": round(float(np.median(xs)), 4), "min": round(float(xs.min()), 4),
            "max": round(float(xs.max()), 4)}


def event_ms(fn, reps, inner=10):
    """Median over reps of the device time per call, `inner` calls enqueued back to back
    between the two events: a single call between events on an idle queue times the host's
    launch latency as much as the kernels."""
    t = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        t.append(e0.elapsed_time(e1) / inner)
    return float(np.median(t))


def kernels_only(gb, batch):
    """A closure that runs isg_train_crop on the arena gb.prepare(batch) has uploaded."""
    from instancesegmentation_amd import _lib as L
    from instancesegmentation_amd.gpu_batch import sample_table
    arena, desc, _ = batch
    gb.prepare(batch)
    tab, n, nbytes = sample_table(desc), int(desc.shape[0]), int(arena.numel())
    lib, st = L.lib(), L.stream_ptr(gb.device)

    def run():
        L.check(lib.isg_train_crop(gb.arena.data_ptr(), nbytes, tab, gb.kp_in.data_ptr(), n, gb.B,
                                   gb.S, gb.work.data_ptr(), gb.x.data_ptr(), gb.mask.data_ptr(),
                                   gb.keypoints.data_ptr(), gb.windows.data_ptr(), st))
    return run


def full_records(n):
    """Every augmentation on, a different record per sample."""
    from instancesegmentation_amd import augment as A
    cfg = A.Augment(flip_p=1.0, rotate_p=1.0, contrast_p=1.0, noise_p=1.0, noise_per_channel_p=1.0,
                    multiply_p=1.0, multiply_per_channel_p=1.0, noise_scale=(6.0, 12.75))
    return A.draw_augment(np.random.Generator(np.random.PCG64(0)), n, cfg)


def kernels_only_aug(gb, batch, table):
    """kernels_only for isg_train_crop_aug with the records `table`."""
    from instancesegmentation_amd import _lib as L
    from instancesegmentation_amd.gpu_batch import aug_table, sample_table
    arena, desc, _ = batch
    gb.prepare(batch)
    tab, n, nbytes = sample_table(desc), int(desc.shape[0]), int(arena.numel())
    recs = aug_table(table)
    lib, st = L.lib(), L.stream_ptr(gb.device)

    def run():
        L.check(lib.isg_train_crop_aug(gb.arena.data_ptr(), nbytes, tab, recs, 1, 0,
                                       gb.kp_in.data_ptr(), n, gb.B, gb.S, gb.work.data_ptr(),
                                       gb.x.data_ptr(), gb.mask.data_ptr(), gb.keypoints.data_ptr(),
                                       gb.windows.data_ptr(), st))
    return run


def summarise(d):
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {d}")
    per = {"train_box_kernel": [], "train_crop_kernel": [], "train_crop_aug_kernel": []}
    with open(files[0]) as fh:
        for r in sorted(csv.DictReader(fh), key=lambda r: int(r["Start_Timestamp"])):
            for k in per:
                if k in r["Kernel_Name"]:
                    per[k].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    out = {"trace": files[0]}
    aug = per.pop("train_crop_aug_kernel")
    if aug:  # --replay N --augment: N launches with identity records, then N with all on
        half = len(aug) // 2
        for name, t in (("stage_b_aug_identity_us", aug[:half]), ("stage_b_aug_full_us", aug[half:])):
            t = t[len(t) // 4:]
            out[name] = dict(stats(t), launches=len(t))
    for k, name in (("train_box_kernel", "stage_a_us"), ("train_crop_kernel", "stage_b_us")):
        t = per[k][len(per[k]) // 4:]  # the first quarter is warm-up
        if not t:
            raise SystemExit(f"no {k} launches in {files[0]}")
        out[name] = dict(stats(t), launches=len(t))
    nbytes = 4 * S * S * 4 * B
    rate = nbytes / (out["stage_b_us"]["median"] * 1e-6)
    out["stage_b_write_bytes"] = nbytes
    out["stage_b_write_TBps"] = round(rate / 1e12, 3)
    out["stage_b_share_of_measured_hbm"] = round(rate / HBM_MEASURED, 3)
    out["stage_b_share_of_spec_hbm"] = round(rate / HBM_SPEC, 3)
    print(json.dumps(out), flush=True)


def fit_rate(root, cpu_num, steps, gpu_crop, dev, extra=()):
    """samples/s of fit() between step 3 and the last step (the first two absorb the
    workers' start-up), by the host clock after each synchronised Trainer.step: overall, and
    from the median interval between steps (which leaves out the validation at an epoch's
    first step and the workers' restart between epochs)."""
    from instancesegmentation_amd import train as TR
    from instancesegmentation_amd import train_loop as TL
    stamps = []
    orig = TR.Trainer.step

    def step(self, *a, **k):
        out = orig(self, *a, **k)
        torch.cuda.synchronize(self.device)
        stamps.append(time.perf_counter())
        return out
    TR.Trainer.step = step
    try:
        with tempfile.TemporaryDirectory() as ck:
            args = TL.parse_args(["--train-dataset-dir", root, "--val-dataset-dir", root,
                                  "--checkpoint-dir", ck, "--batch-size", str(B), "--epoch", "1000",
                                  "--val-iter", "1000000", "--show-iter", "1000000", "--cpu-num",
                                  str(cpu_num), "--max-steps", str(steps)]
                                 + (["--gpu-crop"] if gpu_crop else []) + list(extra))
            torch.manual_seed(0)
            TL.fit(args, device=dev)
    finally:
        TR.Trainer.step = orig
    gaps = np.diff(stamps[2:])
    return {"overall": round((len(stamps) - 3) * B / (stamps[-1] - stamps[2]), 2),
            "by_median_step_interval": round(B / float(np.median(gaps)), 2),
            "step_interval_ms": stats(gaps * 1e3)}


def augment_legs(args, root, gb, runs, ref, dev):
    """--augment: the three kernel legs by events, rounds alternating, then the three fits."""
    runs[1]()  # identity records: the loader's answer again
    torch.cuda.synchronize(dev)
    assert torch.equal(gb.x.cpu(), ref[0]) and torch.equal(gb.mask.cpu(), ref[1])
    names = ("kernels_plain_ms", "kernels_aug_identity_ms", "kernels_aug_full_ms")
    for run in runs:
        for _ in range(5):
            run()
    torch.cuda.synchronize(dev)
    t = {k: [] for k in names}
    for _ in range(args.rounds):
        for k, run in zip(names, runs):
            t[k].append(event_ms(run, args.reps))
    out = {"batch": B, "S": S, "source": [SRC_W, SRC_H], "rounds": args.rounds, "reps": args.reps}
    out.update({k: stats(v) for k, v in t.items()})
    print(json.dumps(out), flush=True)
    if args.fit_steps:
        out = {"cpu_num": args.cpu_num, "fit_steps": args.fit_steps}
        for name, extra in (("fit_samples_per_s_gpu_crop", ()),
                            ("fit_samples_per_s_gpu_crop_augment", ("--augment", "--flip")),
                            ("fit_samples_per_s_gpu_crop_again", ())):
            out[name] = fit_rate(root, args.cpu_num, args.fit_steps, True, dev, extra)
            print(json.dumps(out), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--replay", type=int, default=0)
    ap.add_argument("--summarise", default="")
    ap.add_argument("--cpu-num", type=int, default=2)
    ap.add_argument("--fit-steps", type=int, default=30, help="0: skip (v)")
    ap.add_argument("--augment", action="store_true", help="isg_train_crop_aug beside the plain call")
    ap.add_argument("--images", type=int, default=256, help="dataset size: 32 steps an epoch")
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise)
    if not torch.cuda.is_available():
        raise SystemExit("batch_bench: no GPU (there is no CPU fallback to time)")
    from instancesegmentation_amd import data as D
    from instancesegmentation_amd.gpu_batch import GpuBatcher
    dev = torch.device("cuda", 0)
    with tempfile.TemporaryDirectory() as root:
        write_dataset(root, args.images)
        cpu_ds = D.InstanceCommonDataset(root, with_heatmaps=False)
        raw_ds = D.InstanceCommonDataset(root, raw=True)
        batches = [D.raw_collate_fn([raw_ds[(r * B + i) % len(raw_ds)] for i in range(B)])
                   for r in range(4)]
        gb = GpuBatcher(B, S, dev)
        runs = [kernels_only(gb, b) for b in batches[:1]]
        if args.augment:
            from instancesegmentation_amd import augment as A
            runs.append(kernels_only_aug(gb, batches[0], A.identity_records(B)))
            runs.append(kernels_only_aug(gb, batches[0], full_records(B)))
        if args.replay:
            for run in runs:
                for _ in range(args.replay):
                    run()
            torch.cuda.synchronize(dev)
            print(json.dumps({"replayed": args.replay}), flush=True)
            return 0
        # the answer being timed is the loader's
        x, kp, mask, n = gb.prepare(batches[0])
        ref = D.collate_fn([cpu_ds[i] for i in range(B)])
        assert torch.equal(x.cpu(), ref[0]) and torch.equal(mask.cpu(), ref[1])
        assert torch.equal(kp.cpu(), torch.stack([o["keypoints"] for o in ref[2]]))
        if args.augment:
            return augment_legs(args, root, gb, runs, ref, dev)

        from instancesegmentation_amd.model.segment import Segment
        from instancesegmentation_amd.train import Trainer
        torch.manual_seed(0)
        tr = Trainer(Segment(20), B, [(B, 3, S, S), (B, 17, 3)], device=dev).capture()
        gb.prepare(batches[0], tr.inputs[0], tr.inputs[1], tr.target)
        for _ in range(5):
            tr.step(loss=False)
            gb.prepare(batches[1])
            runs[0]()
        torch.cuda.synchronize(dev)
        t_prep, t_kern, t_step = [], [], []
        for r in range(args.rounds):  # alternating: drift and other tenants hit all alike
            b = batches[r % len(batches)]
            t_prep.append(event_ms(lambda: gb.prepare(b), args.reps))
            t_kern.append(event_ms(runs[0], args.reps))
            t_step.append(event_ms(lambda: tr.step(loss=False), args.reps))
        out = {"batch": B, "S": S, "source": [SRC_W, SRC_H], "rounds": args.rounds, "reps": args.reps,
               "prepare_ms": stats(t_prep), "prepare_kernels_ms": stats(t_kern),
               "trainer_step_ms": stats(t_step),
               "upload_bytes": int(batches[0][0].numel()), "output_bytes": 4 * S * S * 4 * B}
        print(json.dumps(out), flush=True)
        del tr

        # (iv) host cost per batch, one process, wall clock
        h_cpu, h_raw = [], []
        for r in range(max(3, args.rounds // 4)):
            idx = [(r * B + i) % len(cpu_ds) for i in range(B)]
            t0 = time.perf_counter()
            D.collate_fn([cpu_ds[i] for i in idx])
            h_cpu.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            a, _, k = D.raw_collate_fn([raw_ds[i] for i in idx])
            t1 = time.perf_counter()
            a.to(dev)
            k.to(dev)
            torch.cuda.synchronize(dev)
            h_raw.append(((t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3))
        out = {"host_ms_per_batch_default": stats(h_cpu),
               "host_ms_per_batch_raw_decode_pack": stats([a for a, _ in h_raw]),
               "host_ms_per_batch_raw_upload": stats([b for _, b in h_raw])}
        print(json.dumps(out), flush=True)

        if args.fit_steps:
            out = {"cpu_num": args.cpu_num, "fit_steps": args.fit_steps}
            for name, flag in (("fit_samples_per_s_default", False), ("fit_samples_per_s_gpu_crop", True)):
                out[name] = fit_rate(root, args.cpu_num, args.fit_steps, flag, dev)
                print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
