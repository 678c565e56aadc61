"""What the GPU run-length encoder costs and saves, at the bench's inference configuration
(K = 16 instances, 1024 x 1024, bench.py's crowded scene and calibrated model).

    python tools/rle_bench.py [--rounds 30] [--reps 20]
        (a) eng.run() of an rle=True and an rle=False engine, alternating in one process:
            median and min of the per-round medians, device events around each replay;
        (c) result_rle() against result() followed by masks.cpu(), host wall clock, and the
            bytes each moves device -> host.
    python tools/rle_bench.py --replay 50
        only replays the rle=True graph: the command to put under
        `rocprofv3 --kernel-trace --stats` for (b), the rle_*_kernel times beside
        paste_pack_kernel's in the same run.

    python tools/rle_bench.py --strings [--rounds 30] [--reps 20]
        the `counts` strings on the device (rle_strings=True) against the host codec, both
        engines of this commit alternating in one process:
        (d) eng.run() with rle=True alone and with rle_strings=True, device events;
        (e) result_rle() followed by the box loop infer's command line ran before the device
            strings (rle.to_bbox(rle.from_string(counts)) per kept mask) against
            result_coco(), host wall clock after a finished run;
        (f) isg_rle_compress alone, 20 calls back to back between device events;
        and the characters per count of the scene.

Prints one JSON line. The end-to-end gain of (c) depends on the host link of the machine.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def engines(dev, K=16, H=1024, W=1024, configs=None):
    """bench.py infer_bench's scene and model (BatchNorm calibrated on the scene, head bias
    +3), one engine with the encoder and one without."""
    import bench
    from instancesegmentation_amd.infer import InstanceSegmenter
    from instancesegmentation_amd.model.segment import Segment
    torch.manual_seed(99)
    model = Segment(20)
    img, boxes, kps = bench.infer_scene(H, W, 8, 8)
    calib = InstanceSegmenter(model, (H, W), max_instances=K, device=dev, capture=False)
    calib.load(img, boxes, kps)
    calib.run()
    model = model.to(dev).train()
    bns = [m for m in model.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    for b in bns:
        b.momentum = 1.0
    with torch.no_grad():
        model(calib.x[:len(boxes)].contiguous(), calib.keypoints[:len(boxes)].contiguous())
    for b in bns:
        b.momentum = 0.1
    with torch.no_grad():
        model.bottle6_2.bias.add_(3.0)
    model.eval()
    del calib
    out = []
    for kw in (configs or (dict(rle=False), dict(rle=True))):
        eng = InstanceSegmenter(model, (H, W), max_instances=K, iou_thr=0.5, device=dev, **kw)
        eng.load(img, boxes, kps)
        for _ in range(3):
            eng.run()
        out.append(eng)
    torch.cuda.synchronize(dev)
    return out


def run_ms(eng, reps):
    t = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        eng.run()
        e1.record()
        e1.synchronize()
        t.append(e0.elapsed_time(e1))
    return float(np.median(t))


def stats(xs):
    return {"median": round(float(np.median(xs)), 4), "min": round(float(np.min(xs)), 4),
            "max": round(float(np.max(xs)), 4)}


def strings_bench(dev, rounds, reps):
    from instancesegmentation_amd import _lib as L
    from instancesegmentation_amd import rle as R
    host, strs = engines(dev, configs=(dict(rle=True), dict(rle=True, rle_strings=True)))
    H, W = host.H, host.W
    t_host, t_strs = [], []
    for _ in range(rounds):  # alternating: drift and other tenants hit both alike
        t_host.append(run_ms(host, reps))
        t_strs.append(run_ms(strs, reps))

    def host_path():  # what infer --format coco did per image before the device strings
        segs, keep, scores = host.result_rle()
        return segs, [R.to_bbox(R.from_string(sg["counts"]), H, W) for sg in segs], keep

    def device_path():
        segs, boxes, _, keep, scores = strs.result_coco()
        return segs, boxes, keep

    host.run()
    strs.run()
    torch.cuda.synchronize(dev)
    assert host_path() == device_path()  # the timed answers are equal
    w_host, w_strs, w_rle = [], [], []
    for _ in range(rounds):
        for fn, ts in ((host_path, w_host), (device_path, w_strs), (host.result_rle, w_rle)):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
    lib, st = L.lib(), L.stream_ptr(dev)

    def compress():
        L.check(lib.isg_rle_compress(strs.rle_runs.data_ptr(), strs.rle_capacity,
                                     strs.rle_offsets.data_ptr(), strs.K, H, W,
                                     strs.rle_chars.data_ptr(), strs.rle_chars_capacity,
                                     strs.rle_char_offsets.data_ptr(), strs.rle_boxes.data_ptr(),
                                     strs.rle_areas.data_ptr(), strs.rle_string_work.data_ptr(), st))
    k_ms = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            compress()
        e1.record()
        e1.synchronize()
        k_ms.append(e0.elapsed_time(e1) / 20)
    counts = int(strs.rle_offsets[-1].item())
    chars = int(strs.rle_char_offsets[-1].item())
    print(json.dumps({
        "bench": "rle_strings", "device": torch.cuda.get_device_name(0),
        "run_ms_rle": stats(t_host), "run_ms_rle_strings": stats(t_strs),
        "result_rle_then_box_loop_ms": stats(w_host), "result_coco_ms": stats(w_strs),
        "result_rle_ms": stats(w_rle), "rle_compress_ms": stats(k_ms),
        "counts": counts, "chars": chars, "chars_per_count": round(chars / max(counts, 1), 4),
        "kept": len(device_path()[2]), "rle_capacity": strs.rle_capacity,
        "rle_chars_capacity": strs.rle_chars_capacity, "rounds": rounds, "reps": reps}))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--strings", action="store_true")
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--replay", type=int, default=0)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    if args.strings:
        return strings_bench(dev, args.rounds, args.reps)
    plain, rle = engines(dev)
    if args.replay:
        for _ in range(args.replay):
            rle.run()
        torch.cuda.synchronize(dev)
        print(json.dumps({"replayed": args.replay}))
        return 0
    t_plain, t_rle = [], []
    for _ in range(args.rounds):  # alternating: drift and other tenants hit both alike
        t_plain.append(run_ms(plain, args.reps))
        t_rle.append(run_ms(rle, args.reps))
    # the download paths, each after a finished run
    w_rle, w_png = [], []
    for _ in range(args.rounds):
        rle.run()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        segs, keep, _ = rle.result_rle()
        w_rle.append((time.perf_counter() - t0) * 1e3)
        plain.run()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        masks, keep_p, _ = plain.result()
        host = masks.cpu()
        w_png.append((time.perf_counter() - t0) * 1e3)
    assert keep == keep_p
    total = int(rle.rle_offsets[-1].item())
    from instancesegmentation_amd import rle as R
    for seg, i in zip(segs, keep):  # the timed answer is the right one
        assert np.array_equal(R.decode(R.from_string(seg["counts"]), *seg["size"]),
                              host[i].numpy() >= 128)
    K = rle.K
    meta = 4 * (2 * (K + 1) + K + 1 + K)  # result_rle(): offsets, keep, nkeep, scores
    small = 4 + 4 * int(plain.nkeep.item()) + 4 * plain.n  # result(): nkeep, keep, scores
    print(json.dumps({
        "run_ms_rle_off": {"median": round(float(np.median(t_plain)), 4),
                           "min": round(float(np.min(t_plain)), 4)},
        "run_ms_rle_on": {"median": round(float(np.median(t_rle)), 4),
                          "min": round(float(np.min(t_rle)), 4)},
        "result_rle_ms": {"median": round(float(np.median(w_rle)), 4),
                          "min": round(float(np.min(w_rle)), 4)},
        "result_masks_cpu_ms": {"median": round(float(np.median(w_png)), 4),
                                "min": round(float(np.min(w_png)), 4)},
        "bytes_rle": 4 * total + meta, "bytes_masks": int(host.numel()) + small,
        "counts": total, "kept": len(keep), "rle_capacity": rle.rle_capacity,
        "rounds": args.rounds, "reps": args.reps}))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
