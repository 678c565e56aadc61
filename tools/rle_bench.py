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


def engines(dev, K=16, H=1024, W=1024):
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
    for rle in (False, True):
        eng = InstanceSegmenter(model, (H, W), max_instances=K, iou_thr=0.5, device=dev, rle=rle)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--replay", type=int, default=0)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
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
