"""Scoring on the MI355X (csrc/mask_eval.hip) against its CPU statements
(instancesegmentation_amd/evaluate.py), exact — the counts are integers:

  * isg_mask_iou_crops against crop_iou_counts_cpu: B = 3, sample sizes from one float to
    480^2 (scalar only, the quad tail, several workgroups per sample), both operands one
    float past a 16-B boundary, the operands misaligned to each other, the threshold
    128/255 and its two fp32 neighbours, NaN and infinities, counts written into the middle
    of a poisoned table, two calls (no accumulation), and from_logits against the
    probability mode fed from isg_sigmoid_fwd (GPU against GPU);
  * isg_mask_iou_matrix against iou_matrix_cpu: empty stacks, odd sizes, more groups than
    one round of the packing kernel, patterns, unaligned stacks, a poisoned workspace reused
    by a second call with other inputs;
  * MaskMatcher on the canvases of a real InstanceSegmenter, the graph replay unaffected;
  * infer.main --evaluate (both formats) against MaskAP fed from iou_matrix_cpu over the
    PNGs of the run;
  * train_loop.fit: --gpu-iou gives the history of the host path, with --val-batches 0 too,
    and never calls Trainer.probabilities."""
import json

import numpy as np
import pytest
import torch

from instancesegmentation_amd import _lib as L
from instancesegmentation_amd import evaluate as E

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
EDGE = F(128.0) / F(255.0)
POISON = -7


def _off(values, floats):
    """A device copy of `values` (fp32, flat) that starts `floats` floats past a 16-B boundary."""
    buf = torch.zeros(values.size + 8, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[floats:floats + values.size]
    view.copy_(torch.from_numpy(values.reshape(-1)))
    assert view.data_ptr() % 16 == 4 * floats
    return view


def _count(pred, target, B, from_logits, calls=2):
    """isg_mask_iou_crops into rows 2 .. 2 + B of a poisoned table; the guard rows checked."""
    table = torch.full((B + 4, 2), POISON, dtype=torch.int64, device=DEV)
    for _ in range(calls):  # a second call overwrites, it does not accumulate
        out = E.crop_iou_counts(pred.view(B, -1), target.view(B, -1), from_logits=from_logits,
                                out=table[2:2 + B])
    assert out.data_ptr() == table.data_ptr() + 32
    host = table.cpu().numpy()
    assert np.all(host[:2] == POISON) and np.all(host[2 + B:] == POISON)
    return host[2:2 + B]


def _crop_values(rng, B, hw, logits):
    special = ([0.0, np.nan, np.inf, -np.inf, 1.0, -1.0, 0.015686, 0.0157] if logits else
               [0.0, 1.0, np.nan, EDGE, np.nextafter(EDGE, F(0)), np.nextafter(EDGE, F(1))])
    v = (rng.normal(0, 3, (B, hw)) if logits else rng.uniform(0, 1, (B, hw))).astype(F)
    for b in range(B):
        # the special values at the head, inside the quads and at the tail of each sample
        for k, s in enumerate(special):
            for pos in (k + b, hw // 2 + k, hw - 1 - k - b):
                if 0 <= pos < hw:
                    v[b, pos] = s
    return v


@pytest.mark.parametrize("hw", [1, 5, 255, 256, 257, 1027, 70001, 480 * 480])
def test_crop_counts_exact(hw):
    rng = np.random.default_rng(hw)
    B = 3
    p = _crop_values(rng, B, hw, False)
    t = (rng.uniform(0, 1, (B, hw)) < 0.5).astype(F)
    t[:, -1] = [EDGE, np.nextafter(EDGE, F(0)), np.nan]  # the threshold on the target side too
    t[2] = 0 if hw > 1 else t[2]                         # an empty target
    want = E.crop_iou_counts_cpu(p, t)
    got = _count(_off(p, 1), _off(t, 1), B, False)
    print(f"hw {hw}: counts {got.tolist()}")
    assert np.array_equal(got, want)
    if hw > 16:
        assert want[:, 0].min() >= 0 and want[:2, 0].min() > 0  # the case counts something
    # logits: the kernel's own sigmoid against the probabilities isg_sigmoid_fwd stores
    x = _crop_values(rng, B, hw, True)
    xd, td = _off(x, 1), _off(t, 1)
    prob = _off(np.zeros(B * hw, F), 1)
    L.check(L.lib().isg_sigmoid_fwd(xd.data_ptr(), prob.data_ptr(), B * hw, L.stream_ptr()), "sigmoid")
    from_prob = _count(prob, td, B, False)
    from_logits = _count(xd, td, B, True)
    assert np.array_equal(from_logits, from_prob)
    # and both are the CPU statement of the probabilities the GPU stored
    assert np.array_equal(from_prob, E.crop_iou_counts_cpu(prob.cpu().numpy().reshape(B, hw), t))


@pytest.mark.parametrize("offsets", [(0, 0), (1, 2), (3, 0), (2, 2)])
def test_crop_counts_operands_at_any_4_byte_offset(offsets):
    """hw = 1027 is odd, so the samples of one call sit at three different offsets from a
    16-B boundary; with different offsets for the two operands there is no common aligned
    middle and the sample is read one float at a time."""
    rng = np.random.default_rng(7)
    B, hw = 3, 1027
    p = _crop_values(rng, B, hw, False)
    t = (rng.uniform(0, 1, (B, hw)) < 0.5).astype(F)
    got = _count(_off(p, offsets[0]), _off(t, offsets[1]), B, False)
    assert np.array_equal(got, E.crop_iou_counts_cpu(p, t))


def test_crop_counts_wrapper():
    rng = np.random.default_rng(3)
    p = torch.from_numpy(rng.uniform(0, 1, (2, 1, 24, 24)).astype(F)).to(DEV)
    t = torch.from_numpy((rng.uniform(0, 1, (2, 1, 24, 24)) < 0.5).astype(F)).to(DEV)
    out = E.crop_iou_counts(p, t)
    assert out.dtype == torch.int64 and tuple(out.shape) == (2, 2) and out.is_cuda
    assert np.array_equal(out.cpu().numpy(), E.crop_iou_counts_cpu(p.cpu().numpy(), t.cpu().numpy()))
    from instancesegmentation_amd import train_loop as TL
    assert E.mean_iou_from_counts(out.cpu().numpy()) == TL.tensors_mean_iou(p, t)
    with pytest.raises(ValueError):
        E.crop_iou_counts(p, t[:1])
    with pytest.raises(ValueError):
        E.crop_iou_counts(p, t, out=torch.empty((3, 2), dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError):
        E.crop_iou_counts(p.cpu(), t.cpu())


# ---- the IoU matrix ------------------------------------------------------------------------
def _stack(rng, n, H, W, first=None):
    """n masks cycling through the patterns; `first` (a mask) replaces mask 0."""
    out = np.zeros((n, H, W), np.uint8)
    for i in range(n):
        kind = i % 5
        if kind == 0:
            out[i] = rng.integers(0, 256, (H, W), dtype=np.uint8)
        elif kind == 1:
            out[i] = rng.integers(127, 129, (H, W), dtype=np.uint8)  # 127 / 128 only
        elif kind == 2:
            out[i] = 255
        elif kind == 3:
            out[i] = 0
        else:
            out[i] = (rng.uniform(size=(H, W)) < 0.1) * 200
    if first is not None and n:
        out[0] = first
    return out


def _bytes_at(values, offset):
    buf = torch.zeros(values.size + 8, dtype=torch.uint8, device=DEV)
    view = buf[offset:offset + values.size]
    view.copy_(torch.from_numpy(np.ascontiguousarray(values).reshape(-1)))
    return view


def _matrix(det, gt, work, offsets):
    K, G = len(det), len(gt)
    H, W = det.shape[1:]
    d, g = _bytes_at(det, offsets[0]), _bytes_at(gt, offsets[1])
    inter = torch.full((K * G + 2,), POISON, dtype=torch.int32, device=DEV)
    ad = torch.full((K + 2,), POISON, dtype=torch.int32, device=DEV)
    ag = torch.full((G + 2,), POISON, dtype=torch.int32, device=DEV)
    L.check(L.lib().isg_mask_iou_matrix(d.data_ptr(), K, g.data_ptr(), G, H, W, work.data_ptr(),
                                        inter.data_ptr() + 4, ad.data_ptr() + 4, ag.data_ptr() + 4,
                                        L.stream_ptr()), "mask_iou_matrix")
    torch.cuda.synchronize()
    inter, ad, ag = inter.cpu().numpy(), ad.cpu().numpy(), ag.cpu().numpy()
    for a in (inter, ad, ag):  # nothing written outside the outputs
        assert a[0] == POISON and a[-1] == POISON
    return inter[1:-1].reshape(K, G), ad[1:-1], ag[1:-1]


@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (16, 16), (17, 31), (64, 64), (300, 8),
                                   (2, 8197)])
def test_iou_matrix_exact(shape):
    H, W = shape
    rng = np.random.default_rng(100 * H + W)
    for K, G in ((0, 3), (3, 0), (1, 1), (3, 5), (17, 2)):
        ws = L.lib().isg_mask_iou_matrix_workspace(K, G, H, W)
        assert ws == (K + G) * ((H * W + 255) // 256) * 32
        work = torch.full((ws,), 0xFF, dtype=torch.uint8, device=DEV)
        for call in range(2):  # the second call: other inputs through the used workspace
            det = _stack(rng, K, H, W)
            gt = _stack(rng, G, H, W, first=det[0] if K else None)  # gt 0 identical to det 0
            # first neither stack 4-B aligned, then both (the 4-B loads of the packing)
            got = _matrix(det, gt, work, ((1, 3), (0, 4))[call])
            want = E.iou_matrix_cpu(det, gt)
            for a, b, name in zip(got, want, ("inter", "area_det", "area_gt")):
                assert np.array_equal(a, b), (K, G, call, name)
            if K and G:
                assert got[0][0, 0] == got[1][0] == got[2][0]  # the identical pair


# ---- MaskMatcher on a real engine ---------------------------------------------------------
def test_mask_matcher_on_engine_canvases():
    from instancesegmentation_amd.infer import InstanceSegmenter
    from tests.test_gpu_rle import _calibrated, _scene
    rng = np.random.Generator(np.random.PCG64(23))
    H, W = 192, 256
    m = _calibrated()
    img, boxes, kps = _scene(rng, H, W, 3, 1)
    eng = InstanceSegmenter(m, (H, W), max_instances=4, iou_thr=0.5)
    masks, keep, scores = eng(img, boxes, kps)
    host = masks.cpu().numpy()
    assert any((host[i] >= 128).any() for i in keep)
    # ground truth: perturbed copies of the engine's own canvases (shifted, eroded, cleared)
    gt = np.stack([np.roll(host[0], 5, axis=1), host[1], np.where(host[2] > 200, host[2], 0),
                   np.zeros_like(host[0]), np.roll(host[3], -7, axis=0)]).astype(np.uint8)
    matcher = E.MaskMatcher((H, W), max_det=4, max_gt=8, device=DEV)
    matcher.work.fill_(0xFF)
    matcher.out.fill_(POISON)
    iou, inter, ad, ag = matcher.iou(masks, gt)  # device canvases against a numpy stack
    w_inter, w_ad, w_ag = E.iou_matrix_cpu(host, gt)
    assert np.array_equal(inter, w_inter) and np.array_equal(ad, w_ad) and np.array_equal(ag, w_ag)
    assert iou.dtype == np.float64 and np.array_equal(iou, E.iou_from_counts(w_inter, w_ad, w_ag))
    if ad[1] > 0:
        assert iou[1, 1] == 1.0
    assert np.all(iou[:, 3] == 0.0)  # an empty ground truth: union > 0 or 0 by definition
    # the kept canvases only, indexed on the device, against a device stack
    idx = torch.as_tensor(keep, dtype=torch.long, device=DEV)
    iou_k = matcher.iou(masks[idx], torch.from_numpy(gt).to(DEV))[0]
    assert np.array_equal(iou_k, iou[keep])
    assert matcher.iou(masks[:0], gt)[0].shape == (0, 5)
    assert matcher.iou(masks, gt[:0])[0].shape == (4, 0)
    with pytest.raises(ValueError):
        matcher.iou(np.zeros((5, H, W), np.uint8), gt)  # over max_det
    # the graph replay is unaffected: the same image again gives the same canvases
    eng.load(img, boxes, kps)
    eng.run()
    masks2, keep2, scores2 = eng.result()
    assert keep2 == keep and np.array_equal(scores2, scores) and np.array_equal(masks2.cpu().numpy(), host)


# ---- infer.main --evaluate ------------------------------------------------------------------
def test_infer_main_evaluate(tmp_path):
    from PIL import Image

    from instancesegmentation_amd import infer as I
    from instancesegmentation_amd.data import ORDER_PART_NAMES
    from tests.test_gpu_rle import _calibrated, _scene
    rng = np.random.Generator(np.random.PCG64(31))
    H, W = 192, 256
    m = _calibrated()
    d = tmp_path / "images"
    (d / "gt").mkdir(parents=True)
    names = ("000000000042", "b")
    scenes = {}
    for name in names:
        img, boxes, kps = _scene(rng, H, W, 3, 1)
        Image.fromarray(img).save(d / f"{name}.png")
        scenes[name] = boxes
        objs = [{"box": [int(v) for v in b],
                 "body_keypoint": {ORDER_PART_NAMES[j]: {"status": "vis" if k[j, 2] > 0 else "missing",
                                                         "point": [float(k[j, 0]), float(k[j, 1])]}
                                   for j in range(17)}} for b, k in zip(boxes, kps)]
        with open(d / f"{name}.json", "w") as f:
            json.dump({"object": objs}, f)
    ck = tmp_path / "m.pth"
    torch.save({"state_dict": {k: v.cpu() for k, v in m.state_dict().items()}}, ck)
    plain_args = ["-i", str(d), "--checkpoint", str(ck), "--max-instances", "4"]
    # a run without --evaluate: what it writes today, and the masks the ground truth is cut from
    plain = tmp_path / "plain"
    assert I.main(plain_args + ["-o", str(plain)]) == 0
    assert not (plain / "eval.json").exists()
    gts = {}
    for name in names:
        res = json.load(open(plain / f"{name}.json"))
        ann = json.load(open(d / f"{name}.json"))
        gts[name] = []
        for i, (obj, b) in enumerate(zip(ann["object"], scenes[name])):
            if i == 1:  # object 1 has no mask: it is not ground truth
                continue
            if i in res["keep"] and i % 2 == 0:  # the model's own mask, moved 3 px: a near match
                g = np.roll(np.asarray(Image.open(plain / name / f"{i}.png")), 3, axis=1)
            else:                                # its box, filled: a poor match or none
                g = np.zeros((H, W), np.uint8)
                g[max(b[1], 0):b[3], max(b[0], 0):b[2]] = 255
            Image.fromarray(g).save(d / "gt" / f"{name}_{i}.png")
            obj["instance_mask"] = f"gt/{name}_{i}.png"
            gts[name].append(i)
        with open(d / f"{name}.json", "w") as f:
            json.dump(ann, f)
    common = plain_args + ["--evaluate"]
    png, coco = tmp_path / "png", tmp_path / "coco"
    assert I.main(common + ["-o", str(png)]) == 0
    assert I.main(common + ["-o", str(coco), "--format", "coco", "--mask-root", str(d)]) == 0
    got = json.load(open(png / "eval.json"))
    # the expectation: MaskAP fed from iou_matrix_cpu over the PNGs of the png run
    ap, images = E.MaskAP(), []
    for name in names:
        res = json.load(open(png / f"{name}.json"))
        det = np.stack([np.asarray(Image.open(png / name / f"{i}.png")) for i in res["keep"]])
        gt = np.stack([np.asarray(Image.open(d / "gt" / f"{name}_{i}.png")) for i in gts[name]])
        iou = E.iou_from_counts(*E.iou_matrix_cpu(det, gt))
        mm = ap.add_image([res["scores"][i] for i in res["keep"]], iou)
        images.append({"image": f"{name}.png", "keep": res["keep"],
                       "matched_gt@0.5": [gts[name][j] if j >= 0 else -1 for j in mm["matched_gt@0.5"]],
                       "iou@0.5": mm["iou@0.5"]})
    want = ap.summary()
    print("eval summary:", want)
    assert want["detections"] > 0 and want["ground_truth"] == 6 and want["images"] == 2
    assert 0.0 < want["AP"] < 1.0 and want["mean_matched_iou@0.5"] > 0.5  # something matched
    assert got == {"summary": want, "skipped": 0, "images": images}
    got_coco = json.load(open(coco / "eval.json"))
    assert got_coco == got
    # --continue-test: nothing left to process, nothing scored, and eval.json says so
    assert I.main(common + ["-o", str(png), "--continue-test"]) == 0
    again = json.load(open(png / "eval.json"))
    assert again["skipped"] == 2 and again["images"] == [] and again["summary"]["images"] == 0
    # --evaluate changed nothing of what the run writes otherwise
    for name in names:
        assert json.load(open(plain / f"{name}.json")) == json.load(open(png / f"{name}.json"))


# ---- train_loop.fit -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_root(tmp_path_factory):
    from tests.test_train_crop_cpu import write_dataset
    root = tmp_path_factory.mktemp("eval_ds")
    write_dataset(root, np.random.default_rng(31))
    return str(root)


def _fit(root, out, *extra):
    from instancesegmentation_amd import train_loop as TL
    torch.manual_seed(0)
    args = TL.parse_args(["--train-dataset-dir", root, "--val-dataset-dir", root,
                          "--checkpoint-dir", str(out), "--batch-size", "2", "--epoch", "4",
                          "--val-iter", "1", "--show-iter", "1", "--cpu-num", "0",
                          "--max-steps", "2", *extra])
    _, history = TL.fit(args, device=DEV)
    torch.cuda.synchronize(DEV)
    assert len(history) == 2
    return history


@pytest.mark.parametrize("extra", [(), ("--val-batches", "0")], ids=["one_batch", "whole_set"])
def test_fit_gpu_iou_gives_the_host_history(small_root, tmp_path, monkeypatch, extra):
    """Same seed, same data order: `history` is a list of identical Python floats. With
    --gpu-iou the probabilities tensor is never made."""
    from instancesegmentation_amd.train import Trainer
    h_host = _fit(small_root, tmp_path / "host", *extra)

    def boom(self):
        raise AssertionError("--gpu-iou must not call Trainer.probabilities")

    monkeypatch.setattr(Trainer, "probabilities", boom)
    h_gpu = _fit(small_root, tmp_path / "gpu", "--gpu-iou", *extra)
    print("history:", h_host)
    assert h_gpu == h_host
    assert all(0.0 <= t <= 1.0 and 0.0 <= v <= 1.0 for _, _, t, v in h_host)
