"""COCO RLE on the MI355X (csrc/mask_rle.hip, isg_mask_rle) against its CPU statement
(instancesegmentation_amd/rle.py `encode`), bit-exact:

  * every shape x pattern below, K = 3 masks per launch: 1x1, single rows and columns, odd
    sizes (byte path, partial row segment, several workgroups per mask), W % 4 == 0 (dword
    path), more rows per segment than one batch of loads (300 x 8), more workgroups per
    mask than one round of the scan kernel (2 x 8197), an unaligned canvas pointer;
  * selection (permuted subset with a duplicate, *nsel == 0, sel == NULL, indices -1 and K,
    offsets constant past the last slot), overflow (true offsets, correct prefix, guard
    intact), poisoned workspace / outputs and repeated calls;
  * InstanceSegmenter(rle=True): every kept mask decodes to its binarised canvas, graph
    replay equals an eager engine, a tiny rle_capacity gives the same answer through the
    CPU fallback, rle=False is unchanged and result_rle() raises;
  * infer.main --format coco against a --format png run, and --continue-test."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

from instancesegmentation_amd import _lib as L
from instancesegmentation_amd import rle as R
from instancesegmentation_amd.model.segment import Segment
from oracle.seeding import synth_params

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64


def gpu_rle(masks, sel=None, nsel=None, max_sel=None, cap=None, calls=1, byte_offset=0):
    """isg_mask_rle on masks [K,H,W] with every buffer poisoned (0xFF) beforehand.
    Returns (runs uint32 [cap + GUARD], offsets int64 [max_sel + 1])."""
    K, H, W = masks.shape
    flat = torch.zeros(masks.size + 8, dtype=torch.uint8, device=DEV)
    M = flat[byte_offset:byte_offset + masks.size]
    M.copy_(torch.from_numpy(np.ascontiguousarray(masks).reshape(-1)))
    max_sel = K if max_sel is None else max_sel
    cap = K * (H * W + 1) if cap is None else cap
    runs = torch.full((cap + GUARD,), -1, dtype=torch.int32, device=DEV)
    offsets = torch.full((max_sel + 1,), -1, dtype=torch.int64, device=DEV)
    work = torch.full((L.lib().isg_mask_rle_workspace(K, H, W),), 0xFF, dtype=torch.uint8,
                      device=DEV)
    S = None if sel is None else torch.tensor(sel, dtype=torch.int32, device=DEV)
    N = None if nsel is None else torch.tensor([nsel], dtype=torch.int32, device=DEV)
    for _ in range(calls):
        L.check(L.lib().isg_mask_rle(M.data_ptr(), K, H, W, S.data_ptr() if S is not None else None,
                                     N.data_ptr() if N is not None else None, max_sel,
                                     runs.data_ptr(), cap, offsets.data_ptr(), work.data_ptr(),
                                     L.stream_ptr()), "mask_rle")
    torch.cuda.synchronize()
    return runs.cpu().numpy().view(np.uint32), offsets.cpu().numpy()


def expected(masks, slots, max_sel):
    """(runs, offsets) a large enough buffer receives for the source indices `slots`."""
    K, H, W = masks.shape
    per = [R.encode(masks[i]) if 0 <= i < K else np.array([H * W], np.uint32) for i in slots]
    off = np.zeros(max_sel + 1, np.int64)
    ends = np.cumsum([len(c) for c in per]) if per else np.zeros(0, np.int64)
    off[1:len(per) + 1] = ends
    off[len(per) + 1:] = ends[-1] if len(per) else 0
    runs = np.concatenate(per) if per else np.zeros(0, np.uint32)
    return runs, off


def check(masks, **kw):
    K = masks.shape[0]
    runs, off = gpu_rle(masks, **kw)
    e_runs, e_off = expected(masks, range(K), K)
    assert np.array_equal(off, e_off), (off, e_off)
    assert np.array_equal(runs[:len(e_runs)], e_runs)
    assert np.all(runs[len(e_runs):] == 0xFFFFFFFF)  # nothing written past the total


def patterns(H, W, seed):
    """name -> uint8 [H,W]: the cases of the contract that a walk down columns can get wrong."""
    rng = np.random.Generator(np.random.PCG64(seed))
    yy, xx = np.mgrid[0:H, 0:W]
    z = np.zeros((H, W), np.uint8)
    p = {"zero": z.copy(), "full": np.full((H, W), 255, np.uint8)}
    p["first"] = z.copy()
    p["first"][0, 0] = 255
    p["last"] = z.copy()
    p["last"][H - 1, W - 1] = 128
    # alternating along the scan order (position x*H + y; for odd H the 2-D checkerboard):
    # every position is a transition
    p["checker0"] = (((xx * H + yy) & 1) * 255).astype(np.uint8)      # pixel 0 clear: H*W counts
    p["checker1"] = (((xx * H + yy + 1) & 1) * 255).astype(np.uint8)  # pixel 0 set: H*W + 1
    p["checker2d"] = (((xx + yy) & 1) * 255).astype(np.uint8)  # even H: runs of 2 across seams
    p["threshold"] = rng.integers(126, 130, (H, W), dtype=np.uint8)
    p["vstripes"] = (((xx // 3) & 1) * 200).astype(np.uint8)
    p["hstripes"] = (((yy // 2) & 1) * 200).astype(np.uint8)
    cy, cx, ry, rx = (H - 1) / 2.0, (W - 1) / 2.0, max(H / 3.0, 0.6), max(W / 2.5, 0.6)
    p["ellipse"] = ((((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0) * 255).astype(np.uint8)
    # column seams: the run continues from the bottom of column x into the top of column x+1
    x = min(W // 2, max(W - 2, 0))
    both = z.copy()
    both[H - 1, x] = 255
    both[0, min(x + 1, W - 1)] = 255
    p["seam_both"] = both
    p["seam_bottom"] = z.copy()
    p["seam_bottom"][H - 1, x] = 255
    p["seam_top"] = z.copy()
    p["seam_top"][0, min(x + 1, W - 1)] = 255
    return p


SHAPES = [(1, 1), (1, 7), (7, 1), (5, 3), (67, 129), (64, 256), (130, 64), (131, 64), (300, 8),
          (2, 8197)]


@pytest.mark.parametrize("shape", SHAPES)
def test_bit_exact_shapes_and_patterns(shape):
    H, W = shape
    p = patterns(H, W, 11 * H + W)
    assert len(R.encode(p["checker0"])) == H * W
    assert len(R.encode(p["checker1"])) == H * W + 1  # the maximum number of counts
    names = sorted(p)
    names += names[:(-len(names)) % 3]
    for k in range(0, len(names), 3):
        check(np.stack([p[n] for n in names[k:k + 3]]))


def test_unaligned_canvas_takes_the_byte_path():
    p = patterns(64, 256, 3)
    check(np.stack([p["threshold"], p["ellipse"], p["checker1"]]), byte_offset=1)


def _three(H=67, W=129):
    p = patterns(H, W, 5)
    return np.stack([p["ellipse"], p["threshold"], p["vstripes"]])


def test_selection():
    masks = _three()
    K, H, W = masks.shape
    # a permuted subset with a duplicate
    runs, off = gpu_rle(masks, sel=[2, 0, 2], nsel=3)
    e_runs, e_off = expected(masks, [2, 0, 2], 3)
    assert np.array_equal(off, e_off) and np.array_equal(runs[:len(e_runs)], e_runs)
    # fewer slots than max_sel: offsets constant past the last slot
    runs, off = gpu_rle(masks, sel=[1, 2, 0], nsel=1)
    e_runs, e_off = expected(masks, [1], 3)
    assert np.array_equal(off, e_off) and off[1] == off[2] == off[3]
    assert np.array_equal(runs[:len(e_runs)], e_runs) and np.all(runs[len(e_runs):] == 0xFFFFFFFF)
    # *nsel above max_sel is clamped
    runs, off = gpu_rle(masks, sel=[1, 2, 0], nsel=7, max_sel=2)
    e_runs, e_off = expected(masks, [1, 2], 2)
    assert np.array_equal(off, e_off) and np.array_equal(runs[:len(e_runs)], e_runs)
    # *nsel == 0
    runs, off = gpu_rle(masks, sel=[0, 1, 2], nsel=0)
    assert np.array_equal(off, np.zeros(4, np.int64)) and np.all(runs == 0xFFFFFFFF)
    # sel == NULL, with and without nsel
    runs, off = gpu_rle(masks, sel=None, nsel=None)
    e_runs, e_off = expected(masks, [0, 1, 2], 3)
    assert np.array_equal(off, e_off) and np.array_equal(runs[:len(e_runs)], e_runs)
    runs, off = gpu_rle(masks, sel=None, nsel=2)
    e_runs, e_off = expected(masks, [0, 1], 3)
    assert np.array_equal(off, e_off) and np.array_equal(runs[:len(e_runs)], e_runs)
    # indices outside [0, K): the all-zero mask
    runs, off = gpu_rle(masks, sel=[-1, 1, K], nsel=3)
    e_runs, e_off = expected(masks, [-1, 1, K], 3)
    assert runs[0] == H * W and runs[off[2]] == H * W and off[3] - off[2] == 1
    assert np.array_equal(off, e_off) and np.array_equal(runs[:len(e_runs)], e_runs)


@pytest.mark.parametrize("shape", [(67, 129), (64, 256)])
def test_overflow_keeps_true_offsets_and_guard(shape):
    masks = _three(*shape)
    e_runs, e_off = expected(masks, [0, 1, 2], 3)
    for cap in (0, 1, int(e_off[1]) + 5, len(e_runs) - 1):
        runs, off = gpu_rle(masks, cap=cap)
        assert np.array_equal(off, e_off) and off[-1] > cap
        assert np.array_equal(runs[:cap], e_runs[:cap])
        assert len(runs) == cap + GUARD and np.all(runs[cap:] == 0xFFFFFFFF)
    # runs == NULL with runs_cap == 0: the offsets alone
    K, H, W = masks.shape
    M = torch.from_numpy(masks).to(DEV)
    offsets = torch.full((K + 1,), -1, dtype=torch.int64, device=DEV)
    work = torch.full((L.lib().isg_mask_rle_workspace(K, H, W),), 0xFF, dtype=torch.uint8,
                      device=DEV)
    L.check(L.lib().isg_mask_rle(M.data_ptr(), K, H, W, None, None, K, None, 0,
                                 offsets.data_ptr(), work.data_ptr(), L.stream_ptr()), "mask_rle")
    torch.cuda.synchronize()
    assert np.array_equal(offsets.cpu().numpy(), e_off)


def test_poisoned_workspace_and_repeated_calls():
    masks = _three(64, 256)
    once = gpu_rle(masks, sel=[2, 1, 0], nsel=3, calls=1)
    twice = gpu_rle(masks, sel=[2, 1, 0], nsel=3, calls=2)
    e_runs, e_off = expected(masks, [2, 1, 0], 3)
    for runs, off in (once, twice):
        assert np.array_equal(off, e_off) and np.array_equal(runs[:len(e_runs)], e_runs)
    assert np.array_equal(once[0], twice[0]) and np.array_equal(once[1], twice[1])


def test_argument_errors():
    lib = L.lib()
    buf = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    p = buf.data_ptr()
    st = L.stream_ptr()
    bad = [
        (p, 0, 4, 4, None, None, 0, p, 16, p, p),          # K
        (p, 1, 0, 4, None, None, 1, p, 16, p, p),          # H
        (p, 1, 4, -1, None, None, 1, p, 16, p, p),         # W
        (p, 1, 65536, 32768, None, None, 1, p, 16, p, p),  # H*W == 2^31
        (p, 1, 4, 4, None, None, -1, p, 16, p, p),         # max_sel < 0
        (p, 1, 4, 4, None, None, 2, p, 16, p, p),          # max_sel > K with sel == NULL
        (p, 1, 4, 4, None, None, 1, p, -1, p, p),          # runs_cap < 0
        (None, 1, 4, 4, None, None, 1, p, 16, p, p),       # masks
        (p, 1, 4, 4, None, None, 1, p, 16, None, p),       # offsets
        (p, 1, 4, 4, None, None, 1, p, 16, p, None),       # work
        (p, 1, 4, 4, None, None, 1, None, 16, p, p),       # runs NULL with runs_cap > 0
    ]
    for args in bad:
        assert lib.isg_mask_rle(*args, st) == -1, args  # ISG_ERR_INVALID
        assert lib.isg_last_error()
    assert lib.isg_mask_rle_workspace(16, 1024, 1024) > 0


# ---- the pipeline (the synthetic-scene recipe of test_gpu_infer.py, restated) -------------
def _calibrated(model_cin=20, seed=41):
    m = Segment(model_cin)
    shapes = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    params = synth_params(shapes, seed)
    sd = m.state_dict()
    m.load_state_dict({k: torch.as_tensor(v).to(sd[k].dtype) for k, v in params.items()})
    return m


def _scene(rng, H, W, n, dup):
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    boxes, kps = [], []
    for i in range(n):
        cx, cy = rng.uniform(0.3, 0.7) * W, rng.uniform(0.3, 0.7) * H
        bw, bh = rng.uniform(0.15, 0.3) * W, rng.uniform(0.3, 0.5) * H
        b = [int(cx - bw / 2), int(cy - bh / 2), int(cx + bw / 2), int(cy + bh / 2)]
        kp = np.zeros((17, 3))
        kp[:, 0] = rng.uniform(b[0], b[2], 17)
        kp[:, 1] = rng.uniform(b[1], b[3], 17)
        kp[:, 2] = rng.uniform(size=17) < 0.8
        boxes.append(b)
        kps.append(kp)
    for i in range(dup):
        j = i % n
        boxes.append([v + int(rng.integers(-3, 4)) for v in boxes[j]])
        kps.append(kps[j] + np.array([rng.uniform(-2, 2), rng.uniform(-2, 2), 0.0]))
    return img, np.asarray(boxes, np.int64), np.asarray(kps)


def _decode(seg):
    return R.decode(R.from_string(seg["counts"]), *seg["size"])


def test_instance_segmenter_rle():
    from instancesegmentation_amd.infer import InstanceSegmenter
    rng = np.random.Generator(np.random.PCG64(23))
    H, W = 192, 256
    m = _calibrated()
    img, boxes, kps = _scene(rng, H, W, 4, 3)
    eng = InstanceSegmenter(m, (H, W), max_instances=8, iou_thr=0.5, rle=True)
    masks, keep, scores = eng(img, boxes, kps)
    segs, keep_r, scores_r = eng.result_rle()
    assert keep_r == keep and len(segs) == len(keep) and len(keep) > 0
    assert np.array_equal(scores_r, scores)
    host = masks.cpu().numpy()
    assert any((host[i] >= 128).any() for i in keep)  # the scene is not all empty masks
    for seg, i in zip(segs, keep):
        assert seg["size"] == [H, W] and isinstance(seg["counts"], str)
        assert np.array_equal(_decode(seg), host[i] >= 128), i
    # a second image through the replayed graph equals a fresh eager engine
    img2, boxes2, kps2 = _scene(rng, H, W, 5, 2)
    eng.load(img2, boxes2, kps2)
    eng.run()
    segs2, keep2, scores2 = eng.result_rle()
    masks2 = eng.masks[:eng.n].clone()
    eager = InstanceSegmenter(m, (H, W), max_instances=8, iou_thr=0.5, capture=False, rle=True)
    eager.load(img2, boxes2, kps2)
    eager.run()
    segs3, keep3, _ = eager.result_rle()
    assert keep2 == keep3 and segs2 == segs3 and len(segs2) > 0
    # a deliberately tiny capacity: the first kept mask fits, the rest take the CPU fallback
    tiny_cap = len(R.from_string(segs2[0]["counts"])) + 3
    tiny = InstanceSegmenter(m, (H, W), max_instances=8, iou_thr=0.5, capture=False, rle=True,
                             rle_capacity=tiny_cap)
    tiny.load(img2, boxes2, kps2)
    tiny.run()
    with pytest.warns(RuntimeWarning, match="rle_capacity"):
        segs4, keep4, _ = tiny.result_rle()
    assert keep4 == keep2 and segs4 == segs2
    with warnings.catch_warnings():  # it warns once
        warnings.simplefilter("error")
        assert tiny.result_rle()[0] == segs2
    # rle=False: what it returns today, nothing allocated, result_rle() raises
    plain = InstanceSegmenter(m, (H, W), max_instances=8, iou_thr=0.5, capture=False)
    masks_p, keep_p, scores_p = plain(img2, boxes2, kps2)
    assert keep_p == keep2 and torch.equal(masks_p, masks2) and np.array_equal(scores_p, scores2)
    assert not hasattr(plain, "rle_runs") and not hasattr(plain, "rle_work")
    with pytest.raises(RuntimeError):
        plain.result_rle()


def test_infer_main_coco_format(tmp_path):
    from PIL import Image

    from instancesegmentation_amd import infer as I
    from instancesegmentation_amd.data import ORDER_PART_NAMES
    rng = np.random.Generator(np.random.PCG64(31))
    H, W = 192, 256
    m = _calibrated()
    d = tmp_path / "images"
    d.mkdir()
    for name in ("000000000042", "b"):
        img, boxes, kps = _scene(rng, H, W, 3, 1)
        Image.fromarray(img).save(d / f"{name}.png")
        objs = [{"box": [int(v) for v in b],
                 "body_keypoint": {ORDER_PART_NAMES[j]: {"status": "vis" if k[j, 2] > 0 else "missing",
                                                         "point": [float(k[j, 0]), float(k[j, 1])]}
                                   for j in range(17)}} for b, k in zip(boxes, kps)]
        with open(d / f"{name}.json", "w") as f:
            json.dump({"object": objs}, f)
    ck = tmp_path / "m.pth"
    torch.save({"state_dict": {k: v.cpu() for k, v in m.state_dict().items()}}, ck)
    common = ["-i", str(d), "--checkpoint", str(ck), "--max-instances", "4"]
    png, coco = tmp_path / "png", tmp_path / "coco"
    assert I.main(common + ["-o", str(png)]) == 0
    assert I.main(common + ["-o", str(coco), "--format", "coco"]) == 0
    results = json.load(open(coco / "results.json"))
    assert {r["image_id"] for r in results} == {42, "b"}
    n = 0
    for name, image_id in (("000000000042", 42), ("b", "b")):
        ref = json.load(open(png / f"{name}.json"))
        res = json.load(open(coco / f"{name}.json"))
        assert res["keep"] == ref["keep"] and res["scores"] == ref["scores"]
        assert not (coco / name).exists()  # no PNGs
        mine = [r for r in results if r["image_id"] == image_id]
        assert len(mine) == len(ref["keep"]) > 0
        for r, i in zip(mine, ref["keep"]):
            mask = np.asarray(Image.open(png / name / f"{i}.png")) >= 128
            assert r["category_id"] == 1 and r["score"] == ref["scores"][i]
            assert np.array_equal(_decode(r["segmentation"]), mask)
            ys, xs = np.nonzero(mask)
            box = [0, 0, 0, 0] if not len(xs) else [int(xs.min()), int(ys.min()),
                                                    int(xs.max() - xs.min() + 1),
                                                    int(ys.max() - ys.min() + 1)]
            assert r["bbox"] == box
            n += 1
    assert n == len(results)
    # a half-finished output directory: --continue-test completes results.json
    os.remove(coco / "b.json")
    os.remove(coco / "results.json")
    kept = os.stat(coco / "000000000042.json").st_mtime_ns
    assert I.main(common + ["-o", str(coco), "--format", "coco", "--continue-test"]) == 0
    assert os.stat(coco / "000000000042.json").st_mtime_ns == kept  # skipped, not redone
    assert json.load(open(coco / "results.json")) == results
