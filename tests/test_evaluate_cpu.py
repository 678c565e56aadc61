"""Host side of the scoring path (no GPU): argument checks of isg_mask_iou_crops and
isg_mask_iou_matrix (they answer before any HIP call), the numpy statements of the two
kernels, mean_iou_from_counts against train_loop.tensors_mean_iou, the MaskAP accumulator
on hand-worked cases, and the new command-line flags."""
import numpy as np
import pytest
import torch

from instancesegmentation_amd import _lib as L
from instancesegmentation_amd import evaluate as E
from instancesegmentation_amd import infer as I
from instancesegmentation_amd import train_loop as TL

P = 0x1000  # any non-NULL, 16-B aligned value: nothing may dereference it


def test_crops_rejects_bad_arguments_before_any_hip_call():
    lib = L.lib()
    assert lib.isg_abi_version() == 14  # additive symbols: the ABI version stays
    ok = dict(pred=P, target=P, B=2, hw=16, logits=0, counts=P)
    for kw, text in ((dict(B=-1), b"bad sizes"), (dict(hw=0), b"bad sizes"),
                     (dict(hw=-5), b"bad sizes"), (dict(pred=None), b"NULL"),
                     (dict(target=None), b"NULL"), (dict(counts=None), b"NULL"),
                     (dict(pred=P + 2), b"alignment"), (dict(counts=P + 4), b"alignment")):
        a = dict(ok, **kw)
        rc = lib.isg_mask_iou_crops(a["pred"], a["target"], a["B"], a["hw"], a["logits"],
                                    a["counts"], None)
        assert rc == -1, kw
        msg = lib.isg_last_error()
        assert b"mask_iou_crops" in msg and text in msg, (kw, msg)
    # B == 0 is valid and touches nothing, NULL pointers included
    assert lib.isg_mask_iou_crops(None, None, 0, 16, 0, None, None) == 0


def test_matrix_rejects_bad_arguments_before_any_hip_call():
    lib = L.lib()
    ok = dict(det=P, K=2, gt=P, G=3, H=8, W=8, work=P, inter=P, ad=P, ag=P)
    cases = ((dict(K=-1), -1, b"bad sizes"), (dict(G=-1), -1, b"bad sizes"),
             (dict(H=0), -1, b"bad sizes"), (dict(W=-3), -1, b"bad sizes"),
             (dict(H=1 << 16, W=1 << 15), -1, b"2^31"), (dict(H=46341, W=46341), -1, b"2^31"),
             (dict(K=65535, G=1), -2, b"K + G"),
             (dict(det=None), -1, b"NULL"), (dict(gt=None), -1, b"NULL"),
             (dict(work=None), -1, b"NULL"), (dict(inter=None), -1, b"NULL"),
             (dict(ad=None), -1, b"NULL"), (dict(ag=None), -1, b"NULL"),
             (dict(work=P + 4), -1, b"alignment"))
    for kw, code, text in cases:
        a = dict(ok, **kw)
        rc = lib.isg_mask_iou_matrix(a["det"], a["K"], a["gt"], a["G"], a["H"], a["W"], a["work"],
                                     a["inter"], a["ad"], a["ag"], None)
        assert rc == code, kw
        msg = lib.isg_last_error()
        assert b"mask_iou_matrix" in msg and text in msg, (kw, msg)
    # K = G = 0: valid, nothing to do, nothing dereferenced
    assert lib.isg_mask_iou_matrix(None, 0, None, 0, 8, 8, None, None, None, None, None) == 0
    # the workspace: (K + G) rows of 4 words per 256-pixel group
    assert lib.isg_mask_iou_matrix_workspace(0, 0, 8, 8) == 0
    assert lib.isg_mask_iou_matrix_workspace(2, 3, 8, 8) == 5 * 4 * 8
    assert lib.isg_mask_iou_matrix_workspace(1, 1, 17, 31) == 2 * 3 * 4 * 8
    assert lib.isg_mask_iou_matrix_workspace(-1, 1, 8, 8) == -1
    assert lib.isg_mask_iou_matrix_workspace(1, 1, 0, 8) == -1


def test_crop_counts_statement_and_threshold():
    f = np.float32
    edge = f(128.0) / f(255.0)
    below, above = np.nextafter(edge, f(0)), np.nextafter(edge, f(1))
    # which of the three neighbours pass is decided by the fp32 product, not by the real one
    vals = np.array([0.0, 1.0, np.nan, np.inf, -np.inf, below, edge, above, 0.5, 0.50196], f)
    fg = (vals * f(255)) >= f(128)
    assert fg.tolist()[:5] == [False, True, False, True, False] and fg[7] and not fg[8]
    pred = np.stack([vals, vals])
    target = np.stack([np.ones_like(vals), np.zeros_like(vals)])
    c = E.crop_iou_counts_cpu(pred, target)
    assert c.dtype == np.int64 and c.tolist() == [[int(fg.sum()), len(vals)], [0, int(fg.sum())]]
    # on [0,1] it is tensor2mask followed by >= 128
    rng = np.random.default_rng(0)
    p = rng.uniform(0, 1, (3, 1, 9, 7)).astype(f)
    t = (rng.uniform(0, 1, (3, 1, 9, 7)) < 0.5).astype(f)
    want = [[int(((TL.tensor2mask(torch.from_numpy(a)) >= 128) & (TL.tensor2mask(torch.from_numpy(b)) >= 128)).sum()),
             int(((TL.tensor2mask(torch.from_numpy(a)) >= 128) | (TL.tensor2mask(torch.from_numpy(b)) >= 128)).sum())]
            for a, b in zip(p, t)]
    assert E.crop_iou_counts_cpu(p, t).tolist() == want


def test_mean_iou_from_counts_equals_tensors_mean_iou():
    rng = np.random.default_rng(5)
    for B, S in ((1, 5), (8, 33), (3, 16)):
        p = rng.uniform(0, 1, (B, 1, S, S)).astype(np.float32)
        t = (rng.uniform(0, 1, (B, 1, S, S)) < 0.4).astype(np.float32)
        p[0] *= 0.3  # an all-empty pair: IoU 1.0 by definition
        t[0] = 0
        if B > 2:
            t[2] = 0  # empty target, non-empty prediction: IoU 0
        want = TL.tensors_mean_iou(torch.from_numpy(p), torch.from_numpy(t))
        counts = E.crop_iou_counts_cpu(p, t)
        assert counts[0].tolist() == [0, 0]
        assert E.mean_iou_from_counts(counts) == want  # ==, not approx


def test_iou_matrix_cpu_on_hand_made_masks():
    z = np.zeros((4, 4), np.uint8)
    a = z.copy()
    a[0:2, 0:2] = 255          # 4 px
    b = z.copy()
    b[1:3, 1:3] = 128          # 4 px, 1 shared with a
    c = z.copy()
    c[:, :] = 127              # just under the threshold: empty
    d = np.full((4, 4), 200, np.uint8)  # full
    inter, ad, ag = E.iou_matrix_cpu(np.stack([a, c, d]), np.stack([b, a, c, d]))
    assert inter.dtype == ad.dtype == ag.dtype == np.int32
    assert ad.tolist() == [4, 0, 16] and ag.tolist() == [4, 4, 0, 16]
    assert inter.tolist() == [[1, 4, 0, 4], [0, 0, 0, 0], [4, 4, 0, 16]]
    iou = E.iou_from_counts(inter, ad, ag)
    assert iou.dtype == np.float64
    assert iou.tolist() == [[1 / 7, 1.0, 0.0, 0.25], [0.0, 0.0, 0.0, 0.0], [0.25, 0.25, 0.0, 1.0]]
    e = E.iou_matrix_cpu(np.zeros((0, 4, 4), np.uint8), np.stack([a]))
    assert e[0].shape == (0, 1) and e[1].shape == (0,) and e[2].tolist() == [4]
    with pytest.raises(ValueError):
        E.iou_matrix_cpu(np.zeros((1, 4, 4), np.uint8), np.zeros((1, 4, 5), np.uint8))


# ---- MaskAP (build-defined: parity unpinned) -------------------------------------------
def test_ap_perfect_detections():
    ap = E.MaskAP()
    ap.add_image([0.9, 0.8], np.eye(2))
    ap.add_image([0.7], np.ones((1, 1)))
    s = ap.summary()
    assert s["AP"] == 1.0 and s["AP50"] == 1.0 and s["AP75"] == 1.0 and s["AR"] == 1.0
    assert s["mean_matched_iou@0.5"] == 1.0
    assert (s["images"], s["detections"], s["ground_truth"]) == (2, 3, 3)


def test_ap_one_detection_at_iou_062():
    """IoU 0.62 passes t = 0.5, 0.55, 0.6 and fails the other seven: AP_t is 1 three times
    (precision 1 at every recall) and 0 seven times."""
    ap = E.MaskAP()
    m = ap.add_image([0.5], [[0.62]])
    assert m == {"matched_gt@0.5": [0], "iou@0.5": [0.62]}
    s = ap.summary()
    # (the eps of the definition, np.spacing(1) = 2.2e-16, makes 1 / (1 + eps) the double
    # below 1: the hand values hold to a few eps, 1e-12 is far above that and far below 1/101)
    assert s["AP"] == pytest.approx(0.3, abs=1e-12) and s["AP75"] == 0.0
    assert s["AP50"] == pytest.approx(1.0, abs=1e-12)
    assert s["AR"] == pytest.approx(0.3, abs=1e-12) and s["mean_matched_iou@0.5"] == 0.62


def test_ap_false_positive_ahead_of_true_positives():
    """Two ground truths; detections by score: A 0.9 (overlaps nothing), B 0.8 (IoU 1.0 with
    gt 0), C 0.7 (IoU 0.82 with gt 1), given out of score order.
    t <= 0.8 (seven thresholds): TP cumulated (0,1,2), FP (1,1,1): recall (0, .5, 1),
      precision (0, 1/2, 2/3), envelope 2/3 everywhere: AP_t = 2/3, final recall 1.
    t >= 0.85 (three): C is a false positive: TP (0,1,1), FP (1,1,2): recall (0, .5, .5),
      precision (0, 1/2, 1/3), envelope (1/2, 1/2, 1/3); the 51 recalls 0 .. 0.5 sample
      1/2, the 50 above find no recall and sample 0: AP_t = 25.5/101, final recall 0.5."""
    ap = E.MaskAP()
    m = ap.add_image([0.7, 0.9, 0.8], [[0.0, 0.82], [0.0, 0.0], [1.0, 0.1]])
    assert m["matched_gt@0.5"] == [1, -1, 0] and m["iou@0.5"] == [0.82, 0.0, 1.0]
    s = ap.summary()
    assert s["AP"] == pytest.approx((7 * (2 / 3) + 3 * (25.5 / 101)) / 10, abs=1e-12)
    assert s["AP50"] == pytest.approx(2 / 3, abs=1e-12) and s["AP75"] == pytest.approx(2 / 3, abs=1e-12)
    assert s["AR"] == pytest.approx((7 * 1.0 + 3 * 0.5) / 10, abs=1e-12)
    assert s["mean_matched_iou@0.5"] == pytest.approx(0.91, abs=1e-12)
    assert (s["images"], s["detections"], s["ground_truth"]) == (1, 3, 2)


def test_ap_equal_ious_match_the_lowest_index_and_a_taken_gt_is_not_reused():
    ap = E.MaskAP()
    m = ap.add_image([0.9, 0.8, 0.7], [[0.7, 0.7, 0.7], [0.7, 0.7, 0.7], [0.9, 0.6, 0.0]])
    # detection 0 takes gt 0 (the lowest of equals), detection 1 the next, detection 2 finds
    # its best (gt 0) and second best (gt 1) taken and gt 2 below the threshold
    assert m["matched_gt@0.5"] == [0, 1, -1]
    assert m["iou@0.5"] == [0.7, 0.7, 0.0]


def test_ap_truncates_to_100_detections_per_image():
    n = 130
    scores = np.linspace(0.1, 0.9, n)  # ascending: the last 100 are the kept ones
    ap = E.MaskAP()
    m = ap.add_image(scores, np.eye(n))
    assert m["matched_gt@0.5"][:30] == [-1] * 30  # cut before matching
    assert m["matched_gt@0.5"][30:] == list(range(30, n))
    s = ap.summary()
    assert s["detections"] == 100 and s["ground_truth"] == n
    assert s["AR"] == pytest.approx(100 / n, abs=1e-12)
    # precision 1 up to recall 100/130, nothing beyond: the recalls 0 .. 0.76 sample 1
    assert s["AP"] == pytest.approx(77 / 101, abs=1e-12)


def test_ap_without_ground_truth_and_without_detections():
    ap = E.MaskAP()
    m = ap.add_image([0.9], np.zeros((1, 0)))
    assert m == {"matched_gt@0.5": [-1], "iou@0.5": [0.0]}
    s = ap.summary()
    assert s["AP"] == -1.0 and s["AR"] == -1.0 and s["detections"] == 1 and s["ground_truth"] == 0
    assert E.MaskAP().summary()["AP"] == -1.0
    ap = E.MaskAP()
    ap.add_image([], np.zeros((0, 2)))
    s = ap.summary()
    assert s["AP"] == 0.0 and s["AP50"] == 0.0 and s["AR"] == 0.0
    assert (s["images"], s["detections"], s["ground_truth"]) == (1, 0, 2)
    assert "parity unpinned" in E.MaskAP.__doc__


def test_ap_pools_images_by_score():
    """Image 1 holds a confident false positive, image 2 a less confident true positive: the
    pooled order puts the false positive first, as in the single-image case."""
    ap = E.MaskAP()
    ap.add_image([0.9], [[0.0]])
    ap.add_image([0.8], [[1.0]])
    s = ap.summary()
    # TP (0,1), FP (1,1), nGT 2: recall (0, .5), precision (0, .5), envelope .5; the 51
    # recalls up to 0.5 sample 0.5
    assert s["AP"] == pytest.approx(25.5 / 101, abs=1e-12) and s["AR"] == 0.5


# ---- command lines -----------------------------------------------------------------------
def test_new_flags_and_defaults():
    base = ["--train-dataset-dir", "t", "--val-dataset-dir", "v", "--checkpoint-dir", "c"]
    a = TL.parse_args(base)
    assert a.val_batches == 1 and a.gpu_iou is False
    a = TL.parse_args(base + ["--val-batches", "0", "--gpu-iou"])
    assert a.val_batches == 0 and a.gpu_iou is True
    assert TL.parse_args(base + ["--val-batches", "5"]).val_batches == 5
    with pytest.raises(SystemExit):
        TL.parse_args(base + ["--val-batches", "-1"])
    assert "--val-batches" in TL.__doc__ and "--gpu-iou" in TL.__doc__
    a = I.parse_args(["-i", "in", "-o", "out"])
    assert a.evaluate is False and a.mask_root is None
    a = I.parse_args(["-i", "in", "-o", "out", "--evaluate", "--mask-root", "m", "--format", "coco"])
    assert a.evaluate is True and a.mask_root == "m" and a.format == "coco"


def test_read_instance_masks_follows_read_instances(tmp_path):
    from instancesegmentation_amd import data as D
    from tests.test_infer_cpu import _write_dataset
    _write_dataset(tmp_path, np.random.default_rng(2))
    path = str(tmp_path / "data" / "a.json")
    boxes, _ = D.read_instances(path)
    masks = D.read_instance_masks(path)
    assert len(masks) == len(boxes) == 3
    assert masks == [f"instance_mask/a/{i}.png" for i in range(3)]
    assert D.read_instance_masks(str(tmp_path / "missing.json")) == []
