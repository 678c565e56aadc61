"""The infer.py product path: person instances of one image -> masks.

The reference's `infer.py` (:12-36) parses `-i/--test-image-dir -o/--output-dir
--continue-test`, globs the images and stops (a stub: no model, no output). This module
keeps that command line and supplies the missing path, built from the reference's own
per-instance input path (train_instance.py:139-202, test branch) and model:

  per instance k (box + 17 keypoints, the reference's training annotation):
    window   = box +/- 16 px                                  (train_instance.py:166-171)
    valid    = image minus what the centring translation drops (:141-149)
    crop     = window resampled to 480x480, normalised [-1,1] (:175-181, :80-85)
    heatmaps = keypoint2heatmaps of the projected keypoints   (:33-68, :200-202), made
               inside the stem kernels from the keypoints (never in HBM)
  logits   = Segment(20) in eval mode with every BatchNorm folded into its conv
             (Conv.fuseforward, segment.py:47-48)
  prob     = sigmoid                                           (segment.py:534)
  masks    = paste back through the window onto the image canvas (A13), uint8 by
             truncation of p*255 (tensor2mask, train_instance.py:398-399)
  keep     = greedy mask-NMS, IoU 0.5 (A14)
  rle      = (rle=True) the kept masks run-length encoded on the GPU, COCO order
             (csrc/mask_rle.hip, rle.py): a few KB leave the device instead of the canvases
  strings  = (rle_strings=True) their COCO `counts` strings, boxes and areas, written on the
             GPU as well (csrc/mask_rle_string.hip): the host slices bytes, no codec runs

Everything after the host copy of the image runs on the GPU (csrc/infer_ops.hip,
maskops.hip, the Segment plan) and is captured into one HIP graph per (image size,
instance capacity). Instance counts below the capacity are padded with empty windows,
which produce empty masks, score 0, and never suppress anything; their indices are
dropped from `keep`.

    python -m instancesegmentation_amd.infer -i IMAGES -o OUT [--continue-test]
        [--checkpoint best.pth] [--max-instances 16] [--format {png,coco}]
        [--evaluate [--mask-root DIR]]

Instances come from a sidecar annotation next to each image (`<name>.json`, the common
dataset format of dataset/transfer_coco.py:125-227: {"object": [{"box": [x0,y0,x1,y1],
"body_keypoint": {part: {"status": "vis", "point": [x, y]}}}]}; keys may carry ymlib
`key_combine` suffixes, see data.py). Output per image: `<out>/<name>/<i>.png` for each
kept instance and `<out>/<name>.json` with the kept indices and scores. With
`--format coco` no PNG is written: `<out>/<name>.json` also carries one COCO RLE
("segmentation") and one box ("bbox", [x, y, w, h]) per kept index, and
`<out>/results.json` is the COCO results list assembled from every per-image JSON in
the output directory (so `--continue-test` completes it).

`--evaluate` scores the kept masks against the ground truth next to the images: each
sidecar object's `instance_mask` PNG (a path relative to `--mask-root`, default the image
directory; objects without one are not ground truth). The kept canvases are matched on the
GPU while they are still there (evaluate.MaskMatcher, csrc/mask_eval.hip) and accumulated
into evaluate.MaskAP; `<out>/eval.json` carries the summary (AP, AP50, AP75, AR, ...), per
image {image, keep, matched_gt@0.5, iou@0.5}, and how many images `--continue-test`
skipped (only the images processed in this run are scored). Works with either --format.
"""
import argparse
import ctypes
import glob
import json
import os
import warnings

import numpy as np
import torch

from . import _lib as L
from . import rle as R
from .engine import S_ACT, S_IN, S_OUT, S_STATS, S_TENSOR0, Plan

CROP = 480   # train_instance.py:77
PAD = 16     # train_instance.py:167
N_PARTS = 17
NMS_MAX = 256  # masks one isg_mask_nms launch can rank (include/isg.h)
# default capacity of the RLE buffer, in uint32 counts: RLE_CAPACITY_FACTOR * K * (H + W).
# A mask has one count per boundary crossing of a column, so a convex blob that fills the
# frame has about 2 W of them and a person (limbs, holes) a small multiple of that (a
# 1024^2 ellipse: 1,199 counts against the 32,768 a slot gets here). Noise can still
# exceed any fixed capacity (a checkerboard has H*W + 1 counts): result_rle() then
# falls back to the CPU encoder for the slots that did not fit.
RLE_CAPACITY_FACTOR = 16


class InstanceSegmenter:
    """Segment(20) inference over the instances of one image, as one HIP graph.

    model: a Segment(20) whose weights are loaded (it is deep-copied and fused);
    image_hw: (H, W) of the images this instance serves; max_instances: capacity K.
    rle=True appends the COCO run-length encoding of the kept masks to the pipeline
    (result_rle()); rle_capacity: uint32 counts the device buffer holds for all kept masks
    of one image (default RLE_CAPACITY_FACTOR * K * (H + W)).
    rle_strings=True (needs rle=True) appends the `counts` strings, boxes and areas of those
    encodings (result_coco(); result_rle() then slices the strings instead of building
    them); rle_chars_capacity: bytes the device buffer holds for all strings of one image
    (default 2 * rle_capacity: a person's mask takes about one character per count, the
    worst case is seven)."""

    def __init__(self, model, image_hw, max_instances=16, iou_thr=0.5, device=None,
                 capture=True, rle=False, rle_capacity=None, rle_strings=False,
                 rle_chars_capacity=None):
        import copy
        self.device = torch.device(device or "cuda")
        if self.device.type != "cuda":
            raise RuntimeError("InstanceSegmenter runs on the MI355X only (no CPU path)")
        dev = self.device
        self.model = copy.deepcopy(model).to(dev).fuse()
        self.H, self.W = int(image_hw[0]), int(image_hw[1])
        self.K = int(max_instances)
        self.iou_thr = float(iou_thr)
        K, S, H, W = self.K, CROP, self.H, self.W
        cin = self.model.init_conv.layer1.conv.in_channels
        if cin != 3 + N_PARTS:
            raise ValueError(f"InstanceSegmenter needs Segment(20) (RGB + 17 heatmaps), got {cin}")
        # the heatmaps are synthesised inside the stem from the projected keypoints
        # (engine.Keypoints): they are never written to HBM
        self.plan = Plan(self.model, [(K, 3, S, S), (K, N_PARTS, 3)], False, False,
                         (False, False))
        self.image = torch.zeros((H, W, 3), dtype=torch.uint8, device=dev)
        self.windows = torch.zeros((K, 4), dtype=torch.int32, device=dev)
        self.valid = torch.zeros((K, 4), dtype=torch.int32, device=dev)
        self.keypoints = torch.zeros((K, N_PARTS, 3), dtype=torch.float64, device=dev)
        self.x = torch.empty((K, 3, S, S), dtype=torch.float32, device=dev)
        self.logits = torch.empty(self.plan.out_shapes[0], dtype=torch.float32, device=dev)
        self.prob = torch.empty_like(self.logits)
        self.masks = torch.empty((K, H, W), dtype=torch.uint8, device=dev)
        self.work = torch.empty(L.lib().isg_mask_nms_workspace(K, H, W), dtype=torch.uint8,
                                device=dev)
        self.scores = torch.empty(K, dtype=torch.float32, device=dev)
        self.keep = torch.empty(K, dtype=torch.int32, device=dev)
        self.nkeep = torch.zeros(1, dtype=torch.int32, device=dev)
        self.rle = bool(rle)
        if self.rle:
            cap = RLE_CAPACITY_FACTOR * K * (H + W) if rle_capacity is None else int(rle_capacity)
            if cap < 0:
                raise ValueError(f"rle_capacity {cap} < 0")
            self.rle_capacity = cap
            self.rle_runs = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)  # uint32 bits
            self.rle_offsets = torch.empty(K + 1, dtype=torch.int64, device=dev)
            self.rle_work = torch.empty(L.lib().isg_mask_rle_workspace(K, H, W),
                                        dtype=torch.uint8, device=dev)
            self._rle_warned = False
        self.rle_strings = bool(rle_strings)
        if self.rle_strings:
            if not self.rle:
                raise ValueError("rle_strings=True needs rle=True")
            ccap = 2 * self.rle_capacity if rle_chars_capacity is None else int(rle_chars_capacity)
            if ccap < 0:
                raise ValueError(f"rle_chars_capacity {ccap} < 0")
            self.rle_chars_capacity = ccap
            self.rle_chars = torch.empty(max(ccap, 1), dtype=torch.uint8, device=dev)
            # character offsets [K+1] and areas [K] (int64), boxes [K,4] (int32), back to
            # back so that one copy brings them
            self.rle_meta = torch.empty(2 * (K + 1) + 2 * K + 4 * K, dtype=torch.int32, device=dev)
            self.rle_char_offsets = self.rle_meta[:2 * K + 2].view(torch.int64)
            self.rle_areas = self.rle_meta[2 * K + 2:4 * K + 2].view(torch.int64)
            self.rle_boxes = self.rle_meta[4 * K + 2:].view(K, 4)
            self.rle_string_work = torch.empty(
                L.lib().isg_rle_compress_workspace(K, self.rle_capacity) // 8, dtype=torch.int64,
                device=dev)
        self.act = torch.empty(max(self.plan.act_size, 1), dtype=torch.float32, device=dev)
        self.stats = torch.empty(self.plan.stats_size, dtype=torch.float64, device=dev)
        g = self.plan.graph
        tab = (ctypes.c_void_p * (S_TENSOR0 + len(g.tensor_names)))()
        tab[S_ACT] = self.act.data_ptr()
        tab[S_STATS] = self.stats.data_ptr()
        tab[S_IN[0]] = self.x.data_ptr()
        tab[S_IN[1]] = self.keypoints.data_ptr()
        tab[S_OUT[0]] = self.logits.data_ptr()
        tensors = [p for _, p in self.model.named_parameters()] + \
                  [b for _, b in self.model.named_buffers()]
        for j, t in enumerate(tensors):
            tab[S_TENSOR0 + j] = t.data_ptr()
        self.table = tab
        self.graph = None
        if capture:
            self._run()  # first-use initialisation outside the capture
            torch.cuda.synchronize(dev)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self._run()

    def _run(self):
        lib = L.lib()
        st = L.stream_ptr(self.device)
        K, S = self.K, CROP
        L.check(lib.isg_instance_crop(self.image.data_ptr(), self.H, self.W,
                                      self.windows.data_ptr(), self.valid.data_ptr(), K, S,
                                      self.x.data_ptr(), st), "instance_crop")
        self.plan.fwd.run(self.table, st)
        L.check(lib.isg_sigmoid_fwd(self.logits.data_ptr(), self.prob.data_ptr(),
                                    self.prob.numel(), st), "sigmoid")
        # paste-back and the NMS bit-packing in one pass over the canvases (A13 + A14)
        L.check(lib.isg_mask_paste_nms(self.prob.data_ptr(), K, S, self.windows.data_ptr(),
                                       self.H, self.W, self.iou_thr, self.masks.data_ptr(),
                                       self.work.data_ptr(), self.scores.data_ptr(),
                                       self.keep.data_ptr(), self.nkeep.data_ptr(), st),
                "mask_paste_nms")
        if self.rle:  # the kept masks, in keep order
            L.check(lib.isg_mask_rle(self.masks.data_ptr(), K, self.H, self.W,
                                     self.keep.data_ptr(), self.nkeep.data_ptr(), K,
                                     self.rle_runs.data_ptr(), self.rle_capacity,
                                     self.rle_offsets.data_ptr(), self.rle_work.data_ptr(), st),
                    "mask_rle")
        if self.rle_strings:  # slots past *nkeep are empty ranges: no characters
            L.check(lib.isg_rle_compress(self.rle_runs.data_ptr(), self.rle_capacity,
                                         self.rle_offsets.data_ptr(), K, self.H, self.W,
                                         self.rle_chars.data_ptr(), self.rle_chars_capacity,
                                         self.rle_char_offsets.data_ptr(),
                                         self.rle_boxes.data_ptr(), self.rle_areas.data_ptr(),
                                         self.rle_string_work.data_ptr(), st), "rle_compress")

    def load(self, image, boxes, keypoints):
        """Copy one image's inputs into the static buffers (no launch).
        image: uint8 [H,W,3] (numpy or tensor); boxes: [n,4] (x0,y0,x1,y1);
        keypoints: [n,17,3] (x, y, visible) in image coordinates."""
        img = torch.as_tensor(np.ascontiguousarray(image) if isinstance(image, np.ndarray) else image)
        if tuple(img.shape) != (self.H, self.W, 3) or img.dtype != torch.uint8:
            raise ValueError(f"image must be uint8 [{self.H},{self.W},3], got "
                             f"{tuple(img.shape)} {img.dtype}")
        boxes = np.asarray(boxes, np.int64).reshape(-1, 4)
        n = len(boxes)
        if n > self.K:
            raise ValueError(f"{n} instances > capacity {self.K}")
        kp = np.zeros((self.K, N_PARTS, 3), np.float64)
        win = np.zeros((self.K, 4), np.int32)  # padding: empty windows
        val = np.zeros((self.K, 4), np.int32)
        if n:
            w = instance_windows(boxes)
            win[:n] = w
            val[:n] = valid_rects(boxes, self.H, self.W)
            kp[:n] = crop_keypoints(np.asarray(keypoints, np.float64).reshape(n, N_PARTS, 3), w)
        self.n = n
        self.image.copy_(img, non_blocking=False)
        self.windows.copy_(torch.from_numpy(win))
        self.valid.copy_(torch.from_numpy(val))
        self.keypoints.copy_(torch.from_numpy(kp))

    def run(self):
        """Launch the pipeline on the loaded inputs (asynchronous)."""
        if self.graph is not None:
            self.graph.replay()
        else:
            self._run()

    def result(self):
        """(masks uint8 [n,H,W] device view, keep list, scores [n]) of the last run."""
        torch.cuda.synchronize(self.device)
        nk = int(self.nkeep.item())
        keep = [int(i) for i in self.keep[:nk].cpu().tolist() if i < self.n]
        return self.masks[:self.n], keep, self.scores[:self.n].cpu().numpy()

    def result_rle(self):
        """(segmentations, keep list, scores [n]) of the last run: segmentations[i] is the
        COCO RLE {"size": [H, W], "counts": str} of mask keep[i]. Only the offsets and the
        counts themselves leave the device. If the counts of an image exceed rle_capacity,
        the masks that did not fit are encoded on the CPU from their canvases (same
        answer, one warning)."""
        if not self.rle:
            raise RuntimeError("result_rle() needs InstanceSegmenter(rle=True)")
        if self.rle_strings:
            segs, _, _, keep, scores = self._result_strings()
            return segs, keep, scores
        K = self.K
        torch.cuda.synchronize(self.device)  # as result() does, before anything reads
        # the small results in one copy: offsets, keep, nkeep, scores
        meta = torch.cat([self.rle_offsets.view(torch.int32), self.keep, self.nkeep,
                          self.scores.view(torch.int32)]).cpu().numpy()
        off = meta[:2 * K + 2].view(np.int64)
        slots = meta[2 * K + 2:3 * K + 2][:int(meta[3 * K + 2])].tolist()
        scores = meta[3 * K + 3:].view(np.float32)[:self.n].copy()
        total, cap = int(off[-1]), self.rle_capacity
        runs = self.rle_runs[:min(total, cap)].cpu().numpy().view(np.uint32)
        if total > cap and not self._rle_warned:
            self._rle_warned = True
            warnings.warn(f"RLE buffer overflow: {total} counts > rle_capacity {cap}; the "
                          "masks that did not fit are encoded on the CPU", RuntimeWarning)
        segs, keep = [], []
        for j, i in enumerate(slots):
            if i >= self.n:  # padded slot
                continue
            if off[j + 1] <= cap:
                counts = runs[off[j]:off[j + 1]]
            else:
                counts = R.encode(self.masks[i].cpu().numpy())
            segs.append({"size": [self.H, self.W], "counts": R.to_string(counts)})
            keep.append(int(i))
        return segs, keep, scores

    def result_coco(self):
        """(segmentations, boxes, areas, keep list, scores [n]) of the last run:
        segmentations and keep as result_rle(), boxes[i] = [x, y, w, h] (ints, as
        rle.to_bbox) and areas[i] the set pixels of mask keep[i]. Everything was written on
        the device; two copies bring it. Masks whose counts or characters did not fit their
        buffers take the CPU path (same answer, one warning)."""
        if not self.rle_strings:
            raise RuntimeError("result_coco() needs InstanceSegmenter(rle=True, rle_strings=True)")
        return self._result_strings()

    def _result_strings(self):
        K, H, W = self.K, self.H, self.W
        torch.cuda.synchronize(self.device)
        # one copy: count offsets, character offsets, areas, boxes, keep, nkeep, scores
        meta = torch.cat([self.rle_offsets.view(torch.int32), self.rle_meta, self.keep,
                          self.nkeep, self.scores.view(torch.int32)]).cpu().numpy()
        off = meta[:2 * K + 2].view(np.int64)
        coff = meta[2 * K + 2:4 * K + 4].view(np.int64)
        areas = meta[4 * K + 4:6 * K + 4].view(np.int64)
        boxes = meta[6 * K + 4:10 * K + 4].reshape(K, 4)
        slots = meta[10 * K + 4:11 * K + 4][:int(meta[11 * K + 4])].tolist()
        scores = meta[11 * K + 5:].view(np.float32)[:self.n].copy()
        total, cap = int(off[-1]), self.rle_capacity
        ctotal, ccap = int(coff[-1]), self.rle_chars_capacity
        chars = self.rle_chars[:min(ctotal, ccap)].cpu().numpy().tobytes()  # the second copy
        if (total > cap or ctotal > ccap) and not self._rle_warned:
            self._rle_warned = True
            what = (f"{total} counts > rle_capacity {cap}" if total > cap
                    else f"{ctotal} characters > rle_chars_capacity {ccap}")
            warnings.warn(f"RLE buffer overflow: {what}; the masks that did not fit are encoded "
                          "on the CPU", RuntimeWarning)
        segs, out_boxes, out_areas, keep = [], [], [], []
        for j, i in enumerate(slots):
            if i >= self.n:  # padded slot
                continue
            if off[j + 1] <= cap and coff[j + 1] <= ccap:
                counts = chars[coff[j]:coff[j + 1]].decode("ascii")
                box, area = [int(v) for v in boxes[j]], int(areas[j])
            else:
                if off[j + 1] <= cap:
                    c = self.rle_runs[int(off[j]):int(off[j + 1])].cpu().numpy().view(np.uint32)
                else:
                    c = R.encode(self.masks[i].cpu().numpy())
                counts = R.to_string(c)
                box, area = R.summarize(c, H, W)
            segs.append({"size": [H, W], "counts": counts})
            out_boxes.append(box)
            out_areas.append(area)
            keep.append(int(i))
        return segs, out_boxes, out_areas, keep, scores

    def __call__(self, image, boxes, keypoints):
        self.load(image, boxes, keypoints)
        self.run()
        return self.result()


def instance_windows(boxes, pad=PAD):
    """Crop window of each instance: its box +/- 16 px (train_instance.py:166-171)."""
    b = np.asarray(boxes, np.int64).reshape(-1, 4)
    return np.stack([b[:, 0] - pad, b[:, 1] - pad, b[:, 2] + pad, b[:, 3] + pad],
                    1).astype(np.int32)


def valid_rects(boxes, height, width):
    """The image minus what the reference's centring translation (tx, ty) =
    (int(W/2 - cx), int(H/2 - cy)) pushes out of the frame (train_instance.py:141-149)."""
    out = np.zeros((len(boxes), 4), np.int32)
    for i, (x0, y0, x1, y1) in enumerate(np.asarray(boxes, np.float64).reshape(-1, 4)):
        tx = int(width / 2 - (x0 + x1) / 2)
        ty = int(height / 2 - (y0 + y1) / 2)
        out[i] = (max(0, -tx), max(0, -ty), min(width, width - tx), min(height, height - ty))
    return out


def crop_keypoints(keypoints, windows, size=CROP):
    """Keypoints (x, y, visible) in image coordinates -> crop coordinates: the window
    offset, then imgaug's resize projection x * new/old (train_instance.py:176-181)."""
    kp = np.array(keypoints, dtype=np.float64, copy=True)
    for k, (x0, y0, x1, y1) in enumerate(np.asarray(windows, np.int64)):
        if x1 <= x0 or y1 <= y0:
            kp[k, :, 2] = 0.0
            continue
        kp[k, :, 0] = (kp[k, :, 0] - float(x0)) * float(size) / float(x1 - x0)
        kp[k, :, 1] = (kp[k, :, 1] - float(y0)) * float(size) / float(y1 - y0)
    return kp


# ---- command line (infer.py:12-36) ------------------------------------------------------
def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="inference image")
    parser.add_argument("-i", "--test-image-dir", help="image test dir", required=True)
    parser.add_argument("-o", "--output-dir", help="image save dir", required=True)
    parser.add_argument("--continue-test", action="store_true", help="skip existing file.")
    parser.add_argument("--checkpoint", default=None,
                        help="checkpoint with 'state_dict' (train_instance.py:497-503) or a "
                             "bare state_dict; default: the model's own initialisation")
    parser.add_argument("--max-instances", type=int, default=16)
    parser.add_argument("--iou", type=float, default=0.5, help="mask-NMS IoU threshold")
    parser.add_argument("--format", choices=("png", "coco"), default="png",
                        help="png: one PNG per kept instance; coco: COCO RLE results "
                             "(per-image JSON + results.json), no PNGs")
    parser.add_argument("--evaluate", action="store_true",
                        help="score the kept masks against the sidecar objects' instance_mask "
                             "PNGs (mask AP, evaluate.py); writes OUT/eval.json")
    parser.add_argument("--mask-root", default=None,
                        help="with --evaluate: directory the instance_mask paths are relative "
                             "to (default: the image directory)")
    return parser.parse_args(argv)


def path_decompose(path):
    """infer.py:24-29."""
    basename = os.path.basename(path)
    dirname = os.path.dirname(path)
    ext = os.path.splitext(path)[-1][1:]
    basename = os.path.splitext(basename)[0]
    return dirname, basename, ext


def list_images(d):
    """The reference globs "*[jpg,png,jpgerr]" (a character class, infer.py:35); the
    intent — jpg / png files — is what is listed here."""
    return sorted(p for p in glob.glob(os.path.join(d, "*"))
                  if os.path.splitext(p)[1].lower() in (".jpg", ".jpeg", ".png"))


def load_model(checkpoint):
    from .model.segment import Segment
    m = Segment(3 + N_PARTS)
    if checkpoint:
        ck = torch.load(checkpoint, map_location="cpu", weights_only=True)
        m.load_state_dict(ck["state_dict"] if isinstance(ck, dict) and "state_dict" in ck else ck)
    return m


def load_ground_truth(json_path, mask_root, H, W):
    """(gt uint8 [g,H,W], object indices [g]) of one image for --evaluate: the instance_mask
    PNG of every sidecar object that has one, in read_instances order."""
    from PIL import Image

    from .data import read_instance_masks
    masks, index = [], []
    for i, rel in enumerate(read_instance_masks(json_path)):
        if not rel:
            continue
        m = np.asarray(Image.open(os.path.join(mask_root, rel)).convert("L"))
        if m.shape != (H, W):
            raise ValueError(f"{rel}: instance mask is {m.shape}, the image {(H, W)}")
        masks.append(m)
        index.append(i)
    gt = np.stack(masks) if masks else np.zeros((0, H, W), np.uint8)
    return np.ascontiguousarray(gt, np.uint8), index


def main(argv=None):
    from PIL import Image

    from .data import read_instances
    args = parse_args(argv)
    if args.evaluate:
        from .evaluate import MaskAP, MaskMatcher
        ap, matchers, eval_images, skipped = MaskAP(), {}, [], 0
        mask_root = args.mask_root or args.test_image_dir
    os.makedirs(args.output_dir, exist_ok=True)
    model = load_model(args.checkpoint)
    coco = args.format == "coco"
    engines = {}
    for filepath in list_images(args.test_image_dir):
        dirname, basename, ext = path_decompose(filepath)
        out_json = os.path.join(args.output_dir, basename + ".json")
        if args.continue_test and os.path.exists(out_json):
            if args.evaluate:
                skipped += 1
            continue
        img = np.asarray(Image.open(filepath).convert("RGB"))
        boxes, kps = read_instances(os.path.join(dirname, basename + ".json"))
        H, W = img.shape[:2]
        # one greedy NMS over ALL instances of the image: the capacity grows (doubling
        # from --max-instances, one captured engine per capacity) up to the NMS kernel's
        # limit of NMS_MAX masks; only beyond that is the image split into chunks, each
        # with its own NMS (duplicates in different chunks are then not suppressed; the
        # output JSON says so)
        cap = max(1, args.max_instances)
        while cap < min(len(boxes), NMS_MAX):
            cap *= 2
        cap = min(cap, NMS_MAX) if len(boxes) > args.max_instances else cap
        eng = engines.get((H, W, cap))
        if eng is None:
            eng = engines[(H, W, cap)] = InstanceSegmenter(model, (H, W), cap, args.iou,
                                                           rle=coco, rle_strings=coco)
        res = {"image": os.path.basename(filepath), "instances": len(boxes), "keep": [],
               "scores": []}
        if coco:
            res["segmentation"], res["bbox"] = [], []
        if len(boxes) > eng.K:
            print(f"warning: {basename}: {len(boxes)} instances > {eng.K}: mask-NMS runs per "
                  f"chunk of {eng.K}")
            res["nms"] = f"per chunk of {eng.K}"
        if args.evaluate:
            gt, gt_index = load_ground_truth(os.path.join(dirname, basename + ".json"),
                                             mask_root, H, W)
            matcher = matchers.get((H, W))
            if matcher is None or matcher.max_det < eng.K or matcher.max_gt < len(gt):
                matcher = matchers[(H, W)] = MaskMatcher((H, W), eng.K, max(len(gt), 1),
                                                         eng.device)
            gt_dev = torch.from_numpy(gt).to(eng.device)
            rows, det_scores = [], []

        def match(keep, scores):
            # the chunk's kept canvases, still on the device, against the image's ground truth
            det = eng.masks[:eng.n][torch.as_tensor(keep, dtype=torch.long, device=eng.device)]
            rows.append(matcher.iou(det, gt_dev)[0])
            det_scores.extend(float(scores[i]) for i in keep)
        if len(boxes):
            for b0 in range(0, len(boxes), eng.K):
                if coco:
                    eng.load(img, boxes[b0:b0 + eng.K], kps[b0:b0 + eng.K])
                    eng.run()
                    if eng.rle_strings:  # strings and boxes as the device wrote them
                        segs, bbox, _, keep, scores = eng.result_coco()
                    else:
                        segs, keep, scores = eng.result_rle()
                        bbox = [R.to_bbox(R.from_string(sg["counts"]), H, W) for sg in segs]
                    res["keep"] += [b0 + i for i in keep]
                    res["scores"] += [float(s) for s in scores]
                    res["segmentation"] += segs
                    res["bbox"] += bbox
                    if args.evaluate:
                        match(keep, scores)
                    continue
                masks, keep, scores = eng(img, boxes[b0:b0 + eng.K], kps[b0:b0 + eng.K])
                odir = os.path.join(args.output_dir, basename)
                os.makedirs(odir, exist_ok=True)
                host = masks.cpu().numpy()
                for i in keep:
                    Image.fromarray(host[i]).save(os.path.join(odir, f"{b0 + i}.png"))
                res["keep"] += [b0 + i for i in keep]
                res["scores"] += [float(s) for s in scores]
                if args.evaluate:
                    match(keep, scores)
        with open(out_json, "w") as f:
            json.dump(res, f)
        if args.evaluate:
            # every chunk's matrix on its own, the rows concatenated before matching
            iou = np.concatenate(rows) if rows else np.zeros((0, len(gt)))
            m = ap.add_image(det_scores, iou)
            eval_images.append({"image": res["image"], "keep": res["keep"],
                                "matched_gt@0.5": [gt_index[j] if j >= 0 else -1
                                                   for j in m["matched_gt@0.5"]],
                                "iou@0.5": m["iou@0.5"]})
    if coco:
        R.write_results(args.output_dir)
    if args.evaluate:
        summary = ap.summary()
        with open(os.path.join(args.output_dir, "eval.json"), "w") as f:
            json.dump({"summary": summary, "skipped": skipped, "images": eval_images}, f)
        print("eval: " + " ".join(f"{k} {v:.4f}" if isinstance(v, float) else f"{k} {v}"
                                  for k, v in summary.items())
              + (f" (skipped {skipped})" if skipped else ""))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
