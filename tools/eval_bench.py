"""What scoring costs on the host and on the GPU (instancesegmentation_amd/evaluate.py,
csrc/mask_eval.hip), at the sizes the project runs:

    python tools/eval_bench.py [--rounds 10] [--reps 10]
        (i)  validation IoU of one batch, B = 8, 480 x 480 (train_loop's --val-iter):
             the host path train_loop.tensors_mean_iou (2 B synchronising copies, numpy),
             wall clock around a call that ends synchronised; the device path
             crop_iou_counts + one read-back + mean_iou_from_counts the same way; and the
             kernel alone by device events, in probability and in logit mode, with its read
             rate (2 x B x S^2 x 4 B) over the 6.29 TB/s HBM streaming rate measured on this
             part (8.0 TB/s spec);
        (ii) detections x ground truth at K = G = 16, 1024 x 1024 (the bench's inference
             configuration): iou_matrix_cpu on the host against MaskMatcher.iou from device
             canvases (kernels + the one copy), wall clock; isg_mask_iou_matrix alone by
             device events;
        (iii) COCO RLE back onto canvases, n = 16 masks of 1024 x 1024 (the detections of
             (ii), run-length encoded): rle.decode per mask, stacked and uploaded, against
             RleDecoder.decode (packing, upload, kernels, the totals' copy back), wall clock;
             isg_mask_rle_decode alone by device events, with its share of the HBM rate for
             the canvas bytes it writes; and, on its own, rle.from_string over the same
             masks' strings, and that parse followed by RleDecoder.decode against
             RleDecoder.decode_strings (the strings parsed on the device, isg_rle_parse),
             wall clock, with isg_rle_parse alone by device events.
    Rounds alternate the legs; every leg is warmed up first; the two answers of each pair
    are compared before anything is timed. Prints one JSON line. Needs the GPU: there is
    no fallback.
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

HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12
B, S = 8, 480
K, G, H, W = 16, 16, 1024, 1024


def stats(xs):
    xs = np.asarray(xs, np.float64)
    return {"median": round(float(np.median(xs)), 4), "min": round(float(xs.min()), 4),
            "max": round(float(xs.max()), 4)}


def wall_ms(fn, reps):
    """Host clock per call of a function that ends synchronised (it returns host values)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def event_ms(fn, reps, inner=20):
    """Device time per call, `inner` calls enqueued back to back between two events (one call
    between events on an idle queue times the launch latency as much as the kernel)."""
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


def ellipses(rng, n, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    out = np.zeros((n, h, w), np.uint8)
    for i in range(n):
        cx, cy = rng.uniform(0.3, 0.7) * w, rng.uniform(0.3, 0.7) * h
        ax, ay = rng.uniform(0.1, 0.3) * w, rng.uniform(0.2, 0.4) * h
        out[i] = ((((xx - cx) / ax) ** 2 + ((yy - cy) / ay) ** 2) <= 1.0) * 255
    return out


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--rounds", type=int, default=10)
    p.add_argument("--reps", type=int, default=10)
    args = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench.py measures on the GPU; none found")
    from instancesegmentation_amd import evaluate as E
    from instancesegmentation_amd import train_loop as TL
    dev = torch.device("cuda")
    rng = np.random.default_rng(0)
    out = {"bench": "eval", "device": torch.cuda.get_device_name(0)}

    # (i) validation IoU of one batch
    target = torch.from_numpy((ellipses(rng, B, S, S) / 255.0).astype(np.float32)[:, None]).to(dev)
    logits = (target * 6.0 - 3.0 + torch.randn(B, 1, S, S, device=dev)).contiguous()
    prob = torch.sigmoid(logits)
    table = torch.empty((B, 2), dtype=torch.int64, device=dev)

    def host_iou():
        return TL.tensors_mean_iou(prob, target)

    def device_iou():
        E.crop_iou_counts(prob, target, out=table)
        return E.mean_iou_from_counts(table.cpu().numpy())

    assert host_iou() == device_iou()
    legs = {"host_ms": host_iou, "device_ms": device_iou}
    times = {k: [] for k in legs}
    for fn in legs.values():
        wall_ms(fn, 3)
    for _ in range(args.rounds):
        for k, fn in legs.items():
            times[k].append(wall_ms(fn, args.reps))
    klegs = {"kernel_prob_ms": lambda: E.crop_iou_counts(prob, target, out=table),
             "kernel_logits_ms": lambda: E.crop_iou_counts(logits, target, from_logits=True,
                                                           out=table)}
    ktimes = {k: [] for k in klegs}
    for fn in klegs.values():
        event_ms(fn, 2)
    for _ in range(args.rounds):
        for k, fn in klegs.items():
            ktimes[k].append(event_ms(fn, args.reps))
    nbytes = 2 * B * S * S * 4
    val = {k: stats(v) for k, v in {**times, **ktimes}.items()}
    val["speedup_host_over_device"] = round(val["host_ms"]["median"] / val["device_ms"]["median"], 2)
    val["kernel_read_bytes"] = nbytes
    val["kernel_prob_share_of_measured_hbm"] = round(
        nbytes / (val["kernel_prob_ms"]["median"] * 1e-3) / HBM_MEASURED, 4)
    out["val_iou_b8_480"] = val

    # (ii) detections x ground truth
    det_h, gt_h = ellipses(rng, K, H, W), ellipses(rng, G, H, W)
    det_d, gt_d = torch.from_numpy(det_h).to(dev), torch.from_numpy(gt_h).to(dev)
    matcher = E.MaskMatcher((H, W), K, G, dev)

    def host_matrix():
        return E.iou_from_counts(*E.iou_matrix_cpu(det_h, gt_h))

    def device_matrix():
        return matcher.iou(det_d, gt_d)[0]

    assert np.array_equal(host_matrix(), device_matrix())
    from instancesegmentation_amd import _lib as L
    base = matcher.out.data_ptr()

    def kernels():
        L.check(L.lib().isg_mask_iou_matrix(det_d.data_ptr(), K, gt_d.data_ptr(), G, H, W,
                                            matcher.work.data_ptr(), base, base + 4 * K * G,
                                            base + 4 * (K * G + K), L.stream_ptr(dev)))

    legs = {"host_ms": host_matrix, "device_ms": device_matrix}
    times = {k: [] for k in legs}
    wall_ms(host_matrix, 1)
    wall_ms(device_matrix, 3)
    event_ms(kernels, 2)
    ktime = []
    for _ in range(args.rounds):
        times["host_ms"].append(wall_ms(host_matrix, 1))
        times["device_ms"].append(wall_ms(device_matrix, args.reps))
        ktime.append(event_ms(kernels, args.reps))
    mat = {k: stats(v) for k, v in times.items()}
    mat["kernels_ms"] = stats(ktime)
    mat["speedup_host_over_device"] = round(mat["host_ms"]["median"] / mat["device_ms"]["median"], 2)
    mat["read_bytes"] = (K + G) * H * W
    out["iou_matrix_k16_g16_1024"] = mat

    # (iii) COCO RLE back onto canvases: the detections of (ii), run-length encoded
    from instancesegmentation_amd import rle as R
    counts = [R.encode(m) for m in det_h]
    strings = [R.to_string(c) for c in counts]
    total = sum(len(c) for c in counts)
    decoder = E.RleDecoder((H, W), K, total, dev)

    def host_decode():
        stack = np.stack([R.decode(c, H, W) for c in counts]).astype(np.uint8) * np.uint8(255)
        return torch.from_numpy(stack).to(dev)

    def device_decode():
        return decoder.decode(counts)

    def parse_strings():
        return [R.from_string(s) for s in strings]

    assert torch.equal(host_decode(), device_decode()) and torch.equal(device_decode(), det_d)
    assert all(np.array_equal(a, b) for a, b in zip(parse_strings(), counts))

    def decode_kernels():  # on what device_decode() uploaded
        L.check(L.lib().isg_mask_rle_decode(decoder.runs.data_ptr(), total,
                                            decoder.offsets.data_ptr(), K, H, W,
                                            decoder.masks.data_ptr(), decoder.totals.data_ptr(),
                                            decoder.work.data_ptr(), L.stream_ptr(dev)))

    def host_parse_device_decode():  # the offline scorer's path before decode_strings
        return decoder.decode(parse_strings())

    def device_parse_decode():
        return decoder.decode_strings(strings)

    assert torch.equal(device_parse_decode(), det_d)
    nbytes = sum(len(s) for s in strings)

    def parse_kernels():  # on what device_parse_decode() uploaded
        L.check(L.lib().isg_rle_parse(decoder._chars.data_ptr(), nbytes,
                                      decoder._char_offsets.data_ptr(), K, decoder.runs.data_ptr(),
                                      decoder.max_counts, decoder.offsets.data_ptr(),
                                      decoder._status.data_ptr(), decoder._parse_work.data_ptr(),
                                      L.stream_ptr(dev)))

    times = {"host_ms": [], "device_ms": [], "from_string_ms": [],
             "from_string_then_decode_ms": [], "decode_strings_ms": []}
    wall_ms(host_decode, 1)
    wall_ms(device_decode, 3)
    wall_ms(host_parse_device_decode, 1)
    wall_ms(device_parse_decode, 3)
    event_ms(decode_kernels, 2)
    event_ms(parse_kernels, 2)
    ktime, ptime = [], []
    for _ in range(args.rounds):
        times["host_ms"].append(wall_ms(host_decode, 1))
        times["device_ms"].append(wall_ms(device_decode, args.reps))
        times["from_string_ms"].append(wall_ms(parse_strings, 1))
        times["from_string_then_decode_ms"].append(wall_ms(host_parse_device_decode, 1))
        times["decode_strings_ms"].append(wall_ms(device_parse_decode, args.reps))
        ktime.append(event_ms(decode_kernels, args.reps))
        ptime.append(event_ms(parse_kernels, args.reps))
    dec = {k: stats(v) for k, v in times.items()}
    dec["kernels_ms"] = stats(ktime)
    dec["parse_kernels_ms"] = stats(ptime)
    dec["speedup_host_parse_over_decode_strings"] = round(
        dec["from_string_then_decode_ms"]["median"] / dec["decode_strings_ms"]["median"], 2)
    dec["speedup_host_over_device"] = round(dec["host_ms"]["median"] / dec["device_ms"]["median"], 2)
    dec["counts"] = total
    dec["string_bytes"] = sum(len(s) for s in strings)
    dec["written_bytes"] = K * H * W
    dec["kernels_share_of_measured_hbm"] = round(
        K * H * W / (dec["kernels_ms"]["median"] * 1e-3) / HBM_MEASURED, 4)
    out["rle_decode_n16_1024"] = dec
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
