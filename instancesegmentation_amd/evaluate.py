"""Scoring: validation IoU, detections x ground-truth IoU and COCO-style mask AP.

The counting runs on the GPU (csrc/mask_eval.hip); this module holds

  * the CPU statements of the two kernels' contracts, `crop_iou_counts_cpu` and
    `iou_matrix_cpu` (numpy; the kernels are tested bit-exact against them);
  * their wrappers `crop_iou_counts` (device tensors in, a device table out, no sync) and
    `MaskMatcher` (owns workspace and outputs, one device-to-host copy per call);
  * `mean_iou_from_counts`, train_loop.tensors_mean_iou from the integer counts;
  * `MaskAP`, a numpy accumulator of mask average precision on top of the IoU matrix;
  * `RleDecoder`, COCO RLE counts back onto device canvases (csrc/mask_rle_decode.hip; its
    CPU statement is rle.decode_canvas), and on top of it the offline scorer of an existing
    results file:

        python -m instancesegmentation_amd.evaluate --results OUT/results.json -i IMAGES
            [--mask-root DIR] [-o eval.json]

    It walks the images as `infer` does, decodes each image's detections on the GPU,
    matches them against the sidecar `instance_mask` ground truth and writes what
    `infer --evaluate` would have written for a complete run (default: eval.json next to
    the results file).

Foreground is `>= 128` everywhere: on a crop that is tensor2mask (p * 255 truncated to
uint8, train_instance.py:398-399) followed by the build's mask_iou threshold, on a canvas
it is the mask-NMS contract's threshold. torch and libisg.so are imported by the wrappers
and the scorer only: everything else here is numpy.
"""
import numpy as np

THRESHOLD = 128


# ---- CPU statements of the kernel contracts -------------------------------------------
def crop_iou_counts_cpu(pred, target):
    """int64 [B,2] = (|P and T|, |P or T|) per sample of pred, target [B,...] (probabilities
    and masks in [0,1]): X = fp32(x * 255) >= 128, one fp32 multiply; NaN is background.
    The statement of isg_mask_iou_crops with from_logits = 0 (its logit mode is this on
    the device's own sigmoid, 1/(1 + expf(-x)) as isg_sigmoid_fwd computes it)."""
    p = np.asarray(pred, np.float32)
    t = np.asarray(target, np.float32)
    if p.shape != t.shape or p.ndim < 1:
        raise ValueError(f"pred {p.shape} and target {t.shape} must have one shape [B,...]")
    B, hw = p.shape[0], int(np.prod(p.shape[1:]))
    with np.errstate(invalid="ignore", over="ignore"):
        P = (p.reshape(B, hw) * np.float32(255.0)) >= np.float32(THRESHOLD)
        T = (t.reshape(B, hw) * np.float32(255.0)) >= np.float32(THRESHOLD)
    return np.stack([(P & T).sum(1), (P | T).sum(1)], 1).astype(np.int64).reshape(B, 2)


def iou_matrix_cpu(det, gt):
    """(inter int32 [K,G], area_det int32 [K], area_gt int32 [G]) of uint8 stacks det
    [K,H,W] and gt [G,H,W], foreground >= 128: the statement of isg_mask_iou_matrix."""
    d = np.asarray(det)
    g = np.asarray(gt)
    if d.ndim != 3 or g.ndim != 3 or d.shape[1:] != g.shape[1:]:
        raise ValueError(f"det {d.shape} and gt {g.shape} must be [K,H,W] and [G,H,W]")
    hw = d.shape[1] * d.shape[2]
    D = (d >= THRESHOLD).reshape(d.shape[0], hw)
    G = (g >= THRESHOLD).reshape(g.shape[0], hw)
    inter = D.astype(np.int32) @ G.astype(np.int32).T
    return (inter.astype(np.int32).reshape(len(D), len(G)), D.sum(1).astype(np.int32),
            G.sum(1).astype(np.int32))


def iou_from_counts(inter, area_det, area_gt):
    """float64 [K,G] = inter / (area_det + area_gt - inter), 0 where the union is 0."""
    inter = np.asarray(inter, np.int64)
    union = np.asarray(area_det, np.int64)[:, None] + np.asarray(area_gt, np.int64)[None, :] - inter
    out = np.zeros(inter.shape, np.float64)
    np.divide(inter, union, out=out, where=union > 0)
    return out


def mean_iou_from_counts(counts):
    """train_loop.tensors_mean_iou from [n,2] (inter, union) counts: per sample 1.0 for an
    empty union, else float(inter) / float(union); then train_loop.mean's sum / len. Equal
    to the host path with ==, not approximately: the same Python float operations."""
    ious = [1.0 if int(u) == 0 else float(int(i)) / float(int(u))
            for i, u in np.asarray(counts).reshape(-1, 2)]
    return sum(ious) / len(ious)


# ---- the kernels ----------------------------------------------------------------------
def crop_iou_counts(pred, target, from_logits=False, out=None):
    """isg_mask_iou_crops on device tensors pred, target [B,1,S,S] or [B,S,S] (fp32,
    contiguous): int64 [B,2] (inter, union) per sample on the device, nothing synchronised.
    from_logits: pred holds logits (the sigmoid is applied in the kernel, nothing stored).
    out: an int64 [B,2] contiguous device tensor to fill, e.g. rows of a larger table that
    one validation pass reads back once."""
    import torch

    from . import _lib as L
    if pred.device.type != "cuda" or target.device != pred.device:
        raise RuntimeError("crop_iou_counts runs on the MI355X only (crop_iou_counts_cpu is "
                           "the CPU statement)")
    if pred.dtype != torch.float32 or target.dtype != torch.float32:
        raise ValueError(f"pred {pred.dtype} and target {target.dtype} must be float32")
    if pred.shape != target.shape or pred.dim() < 2:
        raise ValueError(f"pred {tuple(pred.shape)} and target {tuple(target.shape)} must "
                         "have one shape [B,...]")
    if not (pred.is_contiguous() and target.is_contiguous()):
        raise ValueError("pred and target must be contiguous")
    B = pred.shape[0]
    if out is None:
        out = torch.empty((B, 2), dtype=torch.int64, device=pred.device)
    elif (out.dtype != torch.int64 or tuple(out.shape) != (B, 2) or not out.is_contiguous()
          or out.device != pred.device):
        raise ValueError(f"out must be a contiguous int64 [{B},2] tensor on {pred.device}")
    if B:
        L.check(L.lib().isg_mask_iou_crops(pred.data_ptr(), target.data_ptr(), B,
                                           pred.numel() // B, 1 if from_logits else 0,
                                           out.data_ptr(), L.stream_ptr(pred.device)),
                "mask_iou_crops")
    return out


class MaskMatcher:
    """isg_mask_iou_matrix for images of one size: owns the workspace and the output buffer
    for up to max_det detections against up to max_gt ground-truth masks."""

    def __init__(self, image_hw, max_det, max_gt, device=None):
        import torch

        from . import _lib as L
        self.device = torch.device(device or "cuda")
        if self.device.type != "cuda":
            raise RuntimeError("MaskMatcher runs on the MI355X only (iou_matrix_cpu is the CPU "
                               "statement)")
        self.H, self.W = int(image_hw[0]), int(image_hw[1])
        self.max_det, self.max_gt = int(max_det), int(max_gt)
        ws = L.lib().isg_mask_iou_matrix_workspace(self.max_det, self.max_gt, self.H, self.W)
        if ws < 0:
            raise ValueError(f"MaskMatcher: bad sizes {image_hw} {max_det} {max_gt}")
        self.work = torch.empty(max(ws, 8), dtype=torch.uint8, device=self.device)
        # inter [n][g], area_det [n], area_gt [g] back to back: one copy brings all three
        self.out = torch.empty(self.max_det * self.max_gt + self.max_det + self.max_gt + 1,
                               dtype=torch.int32, device=self.device)

    def _stack(self, m, limit, what):
        import torch
        if isinstance(m, np.ndarray):
            m = torch.from_numpy(np.ascontiguousarray(m))
        if m.dtype != torch.uint8 or m.dim() != 3 or tuple(m.shape[1:]) != (self.H, self.W):
            raise ValueError(f"{what} must be uint8 [n,{self.H},{self.W}], got "
                             f"{tuple(m.shape)} {m.dtype}")
        if m.shape[0] > limit:
            raise ValueError(f"{m.shape[0]} {what} masks > capacity {limit}")
        return m.to(self.device).contiguous()

    def iou(self, det, gt):
        """det uint8 [n,H,W], gt uint8 [g,H,W] (device tensors or numpy arrays) ->
        (iou float64 [n,g], inter int32 [n,g], area_det int32 [n], area_gt int32 [g]),
        iou = inter / (area_det + area_gt - inter), 0 where the union is 0."""
        from . import _lib as L
        det = self._stack(det, self.max_det, "det")
        gt = self._stack(gt, self.max_gt, "gt")
        n, g = det.shape[0], gt.shape[0]
        base = self.out.data_ptr()
        L.check(L.lib().isg_mask_iou_matrix(det.data_ptr(), n, gt.data_ptr(), g, self.H, self.W,
                                            self.work.data_ptr(), base, base + 4 * n * g,
                                            base + 4 * (n * g + n), L.stream_ptr(self.device)),
                "mask_iou_matrix")
        host = self.out[:n * g + n + g].cpu().numpy()  # the one copy (it synchronises)
        inter = host[:n * g].reshape(n, g).copy()
        area_det, area_gt = host[n * g:n * g + n].copy(), host[n * g + n:].copy()
        return iou_from_counts(inter, area_det, area_gt), inter, area_det, area_gt


# ---- mask average precision -----------------------------------------------------------
class MaskAP:
    """COCOeval's `segm` procedure for one category, no crowd regions, area range "all",
    maxDets 100 — parity unpinned: pycocotools is not available to this project, so this
    class is a build-defined contract, restated from the published
    procedure and pinned only by the hand-worked cases of tests/test_evaluate_cpu.py.

    Thresholds t = np.linspace(.5, .95, 10). Per image (`add_image`): detections in
    descending score order (stable sort), the first 100; at each t a detection takes the
    still unmatched ground truth of highest IoU >= t. Equal IoUs go to the LOWEST
    ground-truth index — a deliberate choice (COCOeval's loop keeps the last of equals
    with its `<` test; with one category and no crowd the counts of true positives are
    the same, the index is only reported). `summary`: all detections pooled and
    stable-sorted by descending score; TP and FP cumulated; recall = TP / nGT, precision =
    TP / (TP + FP + eps); the precision envelope made monotone from the right and
    sampled at the 101 recalls linspace(0, 1, 101) with searchsorted(side="left"), 0
    beyond the last recall; AP_t the mean of the 101 samples."""

    IOU_THRS = np.linspace(.5, .95, 10)
    REC_THRS = np.linspace(0, 1, 101)
    MAX_DETS = 100

    def __init__(self):
        self.images = 0
        self.ground_truth = 0
        self._scores = []   # per image: float64 [n] in matching order
        self._tp = []       # per image: bool [10, n]
        self._matched_iou = []  # IoU of every match at t = 0.5

    def add_image(self, scores, iou):
        """scores [n] and iou [n,g] (rows: detections, columns: ground truth) of one image.
        Returns {"matched_gt@0.5": [n], "iou@0.5": [n]} in the INPUT order of the
        detections: the ground-truth index matched at t = 0.5 (-1: none, or beyond the
        first 100) and the IoU of that match (0.0 where unmatched)."""
        scores = np.asarray(scores, np.float64).reshape(-1)
        n = len(scores)
        iou = np.asarray(iou, np.float64)
        if iou.ndim != 2 or iou.shape[0] != n:
            raise ValueError(f"iou must be [{n},g] for {n} scores, got {iou.shape}")
        g = iou.shape[1]
        order = np.argsort(-scores, kind="stable")[:self.MAX_DETS]
        tp = np.zeros((len(self.IOU_THRS), len(order)), bool)
        match = np.full((len(self.IOU_THRS), len(order)), -1, np.int64)
        if g:
            for ti, t in enumerate(self.IOU_THRS):
                taken = np.zeros(g, bool)
                for di, d in enumerate(order):
                    row = np.where(taken, -1.0, iou[d])
                    j = int(np.argmax(row))  # the first of equal maxima: the lowest index
                    if row[j] >= t:
                        taken[j] = True
                        tp[ti, di] = True
                        match[ti, di] = j
        self.images += 1
        self.ground_truth += g
        self._scores.append(scores[order])
        self._tp.append(tp)
        matched = np.full(n, -1, np.int64)
        matched_iou = np.zeros(n, np.float64)
        for di, d in enumerate(order):
            j = match[0, di]
            if j >= 0:
                matched[d] = j
                matched_iou[d] = iou[d, j]
                self._matched_iou.append(float(iou[d, j]))
        return {"matched_gt@0.5": [int(v) for v in matched],
                "iou@0.5": [float(v) for v in matched_iou]}

    def summary(self):
        """{"AP", "AP50", "AP75", "AR", "mean_matched_iou@0.5", "images", "detections",
        "ground_truth"}. AP is the mean of AP_t over the ten thresholds, AR the mean over t
        of the final recall; both -1.0 without ground truth (as are AP50 and AP75). No
        detections give 0. mean_matched_iou@0.5: the mean IoU of the matches at t = 0.5,
        0.0 when there is none."""
        scores = np.concatenate(self._scores) if self._scores else np.zeros(0)
        tp_all = (np.concatenate(self._tp, 1) if self._tp
                  else np.zeros((len(self.IOU_THRS), 0), bool))
        out = {"AP": -1.0, "AP50": -1.0, "AP75": -1.0, "AR": -1.0,
               "mean_matched_iou@0.5": (sum(self._matched_iou) / len(self._matched_iou)
                                        if self._matched_iou else 0.0),
               "images": self.images, "detections": int(len(scores)),
               "ground_truth": int(self.ground_truth)}
        if self.ground_truth == 0:
            return out
        order = np.argsort(-scores, kind="stable")
        ap, ar = [], []
        for ti in range(len(self.IOU_THRS)):
            tps = tp_all[ti, order]
            tp = np.cumsum(tps).astype(np.float64)
            fp = np.cumsum(~tps).astype(np.float64)
            rc = tp / self.ground_truth
            pr = tp / (tp + fp + np.spacing(1))
            for i in range(len(pr) - 1, 0, -1):  # the envelope, monotone from the right
                if pr[i] > pr[i - 1]:
                    pr[i - 1] = pr[i]
            idx = np.searchsorted(rc, self.REC_THRS, side="left")
            q = np.zeros(len(self.REC_THRS))
            ok = idx < len(pr)
            q[ok] = pr[idx[ok]]
            ap.append(float(q.mean()))
            ar.append(float(rc[-1]) if len(rc) else 0.0)
        out["AP"] = float(np.mean(ap))
        out["AP50"] = ap[0]
        out["AP75"] = ap[5]
        out["AR"] = float(np.mean(ar))
        return out


# ---- COCO RLE back onto canvases --------------------------------------------------------
def _counts_u32(counts):
    """One mask's counts as a contiguous uint32 array (ValueError outside [0, 2^32))."""
    c = np.asarray(counts).reshape(-1)
    if not c.size:
        return np.zeros(0, np.uint32)
    if c.dtype.kind not in "iu" or c.min() < 0 or c.max() >= 2 ** 32:
        raise ValueError("counts must be integers in [0, 2^32)")
    return np.ascontiguousarray(c.astype(np.uint32))


class RleStringError(ValueError):
    """A `counts` string isg_rle_parse flagged: `mask` is its index in the call, `reason`
    the words of rle.status_text."""

    def __init__(self, mask, reason):
        super().__init__(f"mask {mask}: {reason}")
        self.mask, self.reason = mask, reason


class RleDecoder:
    """isg_mask_rle_decode for images of one size: owns the runs, offsets, totals, workspace
    and canvas buffers for up to max_masks masks of max_counts counts together (rle.py
    `decode_canvas` is the CPU statement). decode_strings takes the `counts` strings
    themselves and parses them on the device too (isg_rle_parse, rle.py `parse_total`)."""

    def __init__(self, image_hw, max_masks, max_counts, device=None):
        import torch

        from . import _lib as L
        self.device = torch.device(device or "cuda")
        if self.device.type != "cuda":
            raise RuntimeError("RleDecoder runs on the MI355X only (rle.decode_canvas is the CPU "
                               "statement)")
        self.H, self.W = int(image_hw[0]), int(image_hw[1])
        self.max_masks, self.max_counts = int(max_masks), int(max_counts)
        ws = L.lib().isg_mask_rle_decode_workspace(self.max_masks, self.H, self.W, self.max_counts)
        if ws < 0:
            raise ValueError(f"RleDecoder: bad sizes {image_hw} {max_masks} {max_counts}")
        dev = self.device
        self.runs = torch.empty(max(self.max_counts, 1), dtype=torch.int32, device=dev)  # uint32 bits
        self.offsets = torch.empty(self.max_masks + 1, dtype=torch.int64, device=dev)
        self.totals = torch.empty(max(self.max_masks, 1), dtype=torch.int64, device=dev)
        self.work = torch.empty(ws // 8, dtype=torch.int64, device=dev)
        self.masks = torch.empty((self.max_masks, self.H, self.W), dtype=torch.uint8, device=dev)

    def decode(self, counts, strict=True):
        """counts: a list of uint32 count arrays, one per mask -> the uint8 [n,H,W] device
        view of their canvases (0 / 255; valid until the next call), ready for
        MaskMatcher.iou. strict: a mask whose counts do not sum to H*W raises ValueError;
        strict=False returns (canvases, totals int64 [n]) and leaves the judgement to the
        caller (the canvas of such a mask is rle.decode_canvas's)."""
        import torch

        from . import _lib as L
        per = [_counts_u32(c) for c in counts]
        n = len(per)
        if n > self.max_masks:
            raise ValueError(f"{n} masks > capacity {self.max_masks}")
        off = np.zeros(n + 1, np.int64)
        off[1:] = np.cumsum([len(c) for c in per])
        total = int(off[-1])
        if total > self.max_counts:
            raise ValueError(f"{total} counts > capacity {self.max_counts}")
        if n == 0:
            empty = np.zeros(0, np.int64)
            return self.masks[:0] if strict else (self.masks[:0], empty)
        if total:
            self.runs[:total].copy_(torch.from_numpy(np.concatenate(per).view(np.int32)))
        self.offsets[:n + 1].copy_(torch.from_numpy(off))
        L.check(L.lib().isg_mask_rle_decode(self.runs.data_ptr(), total, self.offsets.data_ptr(), n,
                                            self.H, self.W, self.masks.data_ptr(),
                                            self.totals.data_ptr(), self.work.data_ptr(),
                                            L.stream_ptr(self.device)), "mask_rle_decode")
        totals = self.totals[:n].cpu().numpy()  # the one copy back (it synchronises)
        if not strict:
            return self.masks[:n], totals
        for j in np.flatnonzero(totals != self.H * self.W):
            raise ValueError(f"mask {int(j)}: counts sum to {int(totals[j])}, not H*W = "
                             f"{self.H * self.W}")
        return self.masks[:n]

    def decode_strings(self, strings, strict=True):
        """strings: a list of COCO `counts` strings (str or bytes), one per mask -> what
        `decode` returns for their counts, without a host codec: the concatenated bytes and
        their offsets go up, isg_rle_parse fills the decoder's own runs / offsets,
        isg_mask_rle_decode reads them, and one copy brings totals and status back. A
        string the parser flags raises RleStringError (a ValueError) naming the mask and the
        reason, a truncated one in rle.from_string's words."""
        import torch

        from . import _lib as L
        from .rle import status_text
        per = [np.frombuffer(s.encode("latin-1") if isinstance(s, str) else bytes(s), np.uint8)
               for s in strings]
        n = len(per)
        if n > self.max_masks:
            raise ValueError(f"{n} masks > capacity {self.max_masks}")
        off = np.zeros(n + 1, np.int64)
        off[1:] = np.cumsum([len(b) for b in per])
        nbytes = int(off[-1])
        flat = np.concatenate(per) if nbytes else np.zeros(0, np.uint8)
        # a mask has at most as many counts as bytes; only past that bound are they counted
        if nbytes > self.max_counts:
            total = int(np.count_nonzero(((flat - np.uint8(48)) & np.uint8(0x20)) == 0))
            if total > self.max_counts:
                raise ValueError(f"{total} counts > capacity {self.max_counts}")
        if n == 0:
            empty = np.zeros(0, np.int64)
            return self.masks[:0] if strict else (self.masks[:0], empty)
        if nbytes >= 2 ** 31:
            raise ValueError(f"{nbytes} characters in one call (max 2^31 - 1)")
        lib, dev, st = L.lib(), self.device, L.stream_ptr(self.device)
        if getattr(self, "_chars", None) is None or self._chars.numel() < nbytes:
            self._chars = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        if getattr(self, "_char_offsets", None) is None:  # first use: the parser's buffers
            self._char_offsets = torch.empty(self.max_masks + 1, dtype=torch.int64, device=dev)
            self._parse_work = torch.empty(max(self.max_masks, 1), dtype=torch.int64, device=dev)
            self._status = torch.empty(max(self.max_masks, 1), dtype=torch.int32, device=dev)
        if nbytes:
            self._chars[:nbytes].copy_(torch.from_numpy(flat.copy()))
        self._char_offsets[:n + 1].copy_(torch.from_numpy(off))
        L.check(lib.isg_rle_parse(self._chars.data_ptr(), nbytes, self._char_offsets.data_ptr(), n,
                                  self.runs.data_ptr(), self.max_counts, self.offsets.data_ptr(),
                                  self._status.data_ptr(), self._parse_work.data_ptr(), st),
                "rle_parse")
        L.check(lib.isg_mask_rle_decode(self.runs.data_ptr(), self.max_counts,
                                        self.offsets.data_ptr(), n, self.H, self.W,
                                        self.masks.data_ptr(), self.totals.data_ptr(),
                                        self.work.data_ptr(), st), "mask_rle_decode")
        back = torch.cat([self.totals[:n].view(torch.int32), self._status[:n]]).cpu().numpy()
        totals, status = back[:2 * n].view(np.int64).copy(), back[2 * n:]
        for j in np.flatnonzero(status):
            raise RleStringError(int(j), status_text(int(status[j])))
        if not strict:
            return self.masks[:n], totals
        for j in np.flatnonzero(totals != self.H * self.W):
            raise ValueError(f"mask {int(j)}: counts sum to {int(totals[j])}, not H*W = "
                             f"{self.H * self.W}")
        return self.masks[:n]


# ---- scoring an existing results.json ---------------------------------------------------
def group_detections(results, image_paths):
    """The COCO results list grouped by image: {path: [result, ...]} with every path of
    `image_paths` present (images without detections score their ground truth) and the
    detections of an image in file order. File names map to ids through rle.image_id_of.
    Raises ValueError for two images with one id and for an id that matches no image."""
    import os

    from .rle import image_id_of
    by_id, groups = {}, {}
    for path in image_paths:
        image_id = image_id_of(os.path.splitext(os.path.basename(path))[0])
        if image_id in by_id:
            raise ValueError(f"{by_id[image_id]} and {path} both map to image_id {image_id!r}")
        by_id[image_id] = path
        groups[path] = []
    for k, r in enumerate(results):
        image_id = r["image_id"]
        # JSON keeps 42 and "42" apart; so does image_id_of (digits are always the int)
        if isinstance(image_id, bool) or image_id not in by_id:
            raise ValueError(f"result {k}: image_id {image_id!r} matches no image")
        groups[by_id[image_id]].append(r)
    return groups


def segmentation_counts(seg, H, W):
    """uint32 counts of one result's `segmentation` for an H x W image: a COCO RLE whose
    counts are the compressed string (rle.from_string) or the uncompressed list. Raises
    ValueError for a polygon list and for a `size` that is not the image's."""
    from .rle import from_string
    if not isinstance(seg, dict) or "counts" not in seg or "size" not in seg:
        raise ValueError("segmentation must be a COCO RLE {\"size\", \"counts\"}; polygons are "
                         "not supported")
    if [int(v) for v in seg["size"]] != [H, W]:
        raise ValueError(f"segmentation size {seg['size']} is not the image's {[H, W]}")
    c = seg["counts"]
    return from_string(c) if isinstance(c, (str, bytes)) else _counts_u32(c)


def segmentation_source(seg, H, W):
    """As segmentation_counts, with a compressed `counts` string left as it is (bytes) for
    RleDecoder.decode_strings: its length bounds its number of counts."""
    c = seg.get("counts") if isinstance(seg, dict) else None
    if isinstance(c, (str, bytes)) and "size" in seg and [int(v) for v in seg["size"]] == [H, W]:
        return c.encode("latin-1") if isinstance(c, str) else bytes(c)
    return segmentation_counts(seg, H, W)


DECODE_MASKS = 16  # masks one decode / match round holds (the matcher's max_det)


def score_results(results_path, image_dir, mask_root=None, device=None):
    """Score a COCO results file against the sidecar ground truth of `image_dir`, as
    `infer --evaluate` scores a run: returns the eval.json dictionary."""
    import json
    import os

    import torch
    from PIL import Image

    from .infer import RLE_CAPACITY_FACTOR, list_images, load_ground_truth
    dev = torch.device(device or "cuda")
    with open(results_path) as f:
        results = json.load(f)
    if not isinstance(results, list):
        raise ValueError(f"{results_path}: a COCO results file is a list")
    paths = list_images(image_dir)
    groups = group_detections(results, paths)
    mask_root = mask_root or image_dir
    ap, images, decoders, matchers = MaskAP(), [], {}, {}
    for path in paths:
        with Image.open(path) as im:
            W, H = im.size
        dets = groups[path]
        counts = [segmentation_source(r["segmentation"], H, W) for r in dets]
        gt, gt_index = load_ground_truth(os.path.splitext(path)[0] + ".json", mask_root, H, W)
        matcher = matchers.get((H, W))
        if matcher is None or matcher.max_gt < len(gt):
            matcher = matchers[(H, W)] = MaskMatcher((H, W), DECODE_MASKS, max(len(gt), 1), dev)
        gt_dev = torch.from_numpy(gt).to(dev)
        need = max([len(c) for c in counts], default=0)
        dec = decoders.get((H, W))
        if dec is None or dec.max_counts < need:
            dec = decoders[(H, W)] = RleDecoder(
                (H, W), DECODE_MASKS, max(RLE_CAPACITY_FACTOR * DECODE_MASKS * (H + W), need), dev)
        rows, k = [], 0
        while k < len(counts):  # a chunk: up to DECODE_MASKS masks that fit the runs buffer
            e, used = k, 0
            while (e < len(counts) and e - k < dec.max_masks
                   and (e == k or used + len(counts[e]) <= dec.max_counts)):
                used += len(counts[e])
                e += 1
            name = os.path.basename(path)
            if all(isinstance(c, bytes) for c in counts[k:e]):  # parsed on the device
                try:
                    canvases, totals = dec.decode_strings(counts[k:e], strict=False)
                except RleStringError as err:
                    raise ValueError(f"{name}, detection {k + err.mask}: {err.reason}") from None
            else:
                for d in range(k, e):
                    if isinstance(counts[d], bytes):
                        try:
                            counts[d] = segmentation_counts(dets[d]["segmentation"], H, W)
                        except ValueError as err:
                            raise ValueError(f"{name}, detection {d}: {err}") from None
                canvases, totals = dec.decode(counts[k:e], strict=False)
            for j in np.flatnonzero(totals != H * W):
                raise ValueError(f"{os.path.basename(path)}, detection {k + int(j)}: counts sum to "
                                 f"{int(totals[j])}, not H*W = {H * W}")
            rows.append(matcher.iou(canvases, gt_dev)[0])
            k = e
        iou = np.concatenate(rows) if rows else np.zeros((0, len(gt)))
        m = ap.add_image([float(r["score"]) for r in dets], iou)
        images.append({"image": os.path.basename(path), "detections": len(dets),
                       "matched_gt@0.5": [gt_index[j] if j >= 0 else -1
                                          for j in m["matched_gt@0.5"]],
                       "iou@0.5": m["iou@0.5"]})
    return {"summary": ap.summary(), "results": results_path, "images": images}


def parse_args(argv=None):
    import argparse
    parser = argparse.ArgumentParser(
        prog="python -m instancesegmentation_amd.evaluate",
        description="score an existing COCO results.json (mask AP) against the sidecar "
                    "instance_mask ground truth")
    parser.add_argument("--results", required=True, help="results.json of infer --format coco")
    parser.add_argument("-i", "--test-image-dir", required=True, help="image test dir")
    parser.add_argument("--mask-root", default=None,
                        help="directory the instance_mask paths are relative to (default: the "
                             "image directory)")
    parser.add_argument("-o", "--output", default=None,
                        help="where eval.json goes (default: next to the results file)")
    return parser.parse_args(argv)


def main(argv=None):
    import json
    import os
    args = parse_args(argv)
    out = score_results(args.results, args.test_image_dir, args.mask_root)
    path = args.output or os.path.join(os.path.dirname(os.path.abspath(args.results)), "eval.json")
    with open(path, "w") as f:
        json.dump(out, f)
    print("eval: " + " ".join(f"{k} {v:.4f}" if isinstance(v, float) else f"{k} {v}"
                              for k, v in out["summary"].items()))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
