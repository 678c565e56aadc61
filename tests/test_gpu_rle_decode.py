"""COCO RLE decoding on the MI355X (csrc/mask_rle_decode.hip, isg_mask_rle_decode) against
its CPU statement (instancesegmentation_amd/rle.py `decode_canvas`), bit-exact:

  * every shape x pattern below, n = 3 slots per launch: 1x1, single rows and columns, an odd
    size (byte path, partial row segments), W % 4 == 0 (dword path), ten rows per row
    segment (300 x 8), more tiles per canvas and more runs than one chunk of the
    scan (2 x 8197), an unaligned canvas pointer; canvases, totals and workspace poisoned
    (0xFF) before every call, every launch made twice, guard bytes around the canvases;
  * slots: empty, reversed, below 0, past runs_cap, a short and a long sum between intact
    neighbours, overlapping ranges, n == 0, runs_cap == 0;
  * the round trip on the device, isg_mask_rle's runs / offsets fed straight back;
  * one captured graph holding the decode alone, replayed on refilled inputs;
  * evaluate.RleDecoder on the strings of a real InstanceSegmenter, into MaskMatcher;
  * python -m instancesegmentation_amd.evaluate on the results.json of an
    infer --format coco --evaluate run: the same eval as the online one."""
import json

import numpy as np
import pytest
import torch

from instancesegmentation_amd import _lib as L
from instancesegmentation_amd import evaluate as E
from instancesegmentation_amd import rle as R
from tests.test_gpu_rle import _calibrated, _scene, patterns

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64


def _launch(runs_d, cap, off_d, n, H, W, flat, byte_offset, totals, work):
    L.check(L.lib().isg_mask_rle_decode(runs_d.data_ptr() if runs_d is not None else None, cap,
                                        off_d.data_ptr(), n, H, W,
                                        flat.data_ptr() + byte_offset, totals.data_ptr() + 8,
                                        work.data_ptr(), L.stream_ptr()), "mask_rle_decode")


def gpu_decode(runs, offsets, H, W, cap=None, byte_offset=0):
    """isg_mask_rle_decode of the slots `offsets` [n+1] of `runs`, twice, canvases, totals
    and workspace poisoned (0xFF) before each call and the guards around the outputs checked
    after it. Returns (canvases uint8 [n,H,W], totals int64 [n]) of the second call, equal
    to the first's."""
    runs = np.asarray(runs, np.uint32)
    offsets = np.asarray(offsets, np.int64)
    n = len(offsets) - 1
    cap = len(runs) if cap is None else cap
    runs_d = torch.from_numpy(np.concatenate([runs, np.full(GUARD, 0xFFFFFFFF, np.uint32)])
                              .view(np.int32)).to(DEV)
    off_d = torch.from_numpy(offsets).to(DEV)
    ws = L.lib().isg_mask_rle_decode_workspace(n, H, W, cap)
    assert ws >= 8
    nbytes = n * H * W
    got = []
    for _ in range(2):
        flat = torch.full((GUARD + nbytes + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
        totals = torch.full((n + 2,), -1, dtype=torch.int64, device=DEV)
        work = torch.full((ws // 8,), -1, dtype=torch.int64, device=DEV)
        _launch(runs_d, cap, off_d, n, H, W, flat, GUARD + byte_offset, totals, work)
        torch.cuda.synchronize()
        f, t = flat.cpu().numpy(), totals.cpu().numpy()
        lo, hi = GUARD + byte_offset, GUARD + byte_offset + nbytes
        assert np.all(f[:lo] == 0xFF) and np.all(f[hi:] == 0xFF)  # the guards are intact
        assert t[0] == -1 and t[-1] == -1
        got.append((f[lo:hi].reshape(n, H, W), t[1:-1]))
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
    return got[1]


def expected(runs, offsets, H, W, cap=None):
    runs = np.asarray(runs, np.uint32)
    cap = len(runs) if cap is None else cap
    canvases, totals = [], []
    for a, b in zip(offsets[:-1], offsets[1:]):
        ok = 0 <= a < b <= cap
        c, t = R.decode_canvas(runs[a:b] if ok else [], H, W)
        canvases.append(c)
        totals.append(t)
    return np.stack(canvases), np.asarray(totals, np.int64)


def check(per_slot, H, W, **kw):
    """The slots packed back to back, as the encoder packs them."""
    runs = np.concatenate([np.asarray(c, np.uint32) for c in per_slot])
    offsets = np.concatenate([[0], np.cumsum([len(c) for c in per_slot])]).astype(np.int64)
    canvases, totals = gpu_decode(runs, offsets, H, W, **kw)
    e_canvases, e_totals = expected(runs, offsets, H, W)
    assert np.array_equal(totals, e_totals), (totals, e_totals)
    for j in range(len(per_slot)):
        assert np.array_equal(canvases[j], e_canvases[j]), j
    return canvases, totals


def blobs(rng, H, W):
    """Random blobs: a few random ellipses, one of them cut out again."""
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.zeros((H, W), bool)
    for k in range(4):
        cy, cx = rng.uniform(0, H), rng.uniform(0, W)
        ry, rx = rng.uniform(0.1, 0.4) * H + 0.6, rng.uniform(0.1, 0.4) * W + 0.6
        e = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
        m = m & ~e if k == 3 else m | e
    return (m * 255).astype(np.uint8)


def with_zero_runs(rng, counts):
    """A valid counts array (the same sum) with zero-length runs inserted at random places,
    some of them next to each other, at both ends too."""
    c = np.asarray(counts, np.uint32)
    at = np.sort(rng.integers(0, len(c) + 1, max(3, len(c) // 4)))
    at = np.concatenate([at, [0, 0, len(c)], at[:2]])
    return np.insert(c, np.sort(at), 0).astype(np.uint32)


def count_sets(H, W, seed):
    """name -> counts: the cases of the contract that a walk down columns can get wrong."""
    rng = np.random.Generator(np.random.PCG64(seed))
    p = patterns(H, W, seed)
    # zero / full: a single run over every column, lanes never meet an end; the two
    # checkerboards: H*W and H*W + 1 counts, every position its own run; vstripes: ends
    # exactly on column seams
    names = ["zero", "full", "first", "last", "checker0", "checker1", "vstripes", "hstripes"]
    out = {k: R.encode(p[k]) for k in names}
    assert len(out["checker0"]) == H * W and len(out["checker1"]) == H * W + 1
    out["blobs"] = R.encode(blobs(rng, H, W))
    out["blobs_zero_runs"] = with_zero_runs(rng, R.encode(blobs(rng, H, W)))
    out["threshold_zero_runs"] = with_zero_runs(rng, R.encode(p["threshold"]))
    assert int(out["blobs_zero_runs"].astype(np.int64).sum()) == H * W
    return out


SHAPES = [(1, 1), (1, 67), (67, 1), (37, 53), (64, 128), (300, 8), (2, 8197)]


@pytest.mark.parametrize("shape", SHAPES)
def test_bit_exact_shapes_and_patterns(shape):
    H, W = shape
    sets = count_sets(H, W, 11 * H + W)
    names = sorted(sets)
    names += names[:(-len(names)) % 3]
    for k in range(0, len(names), 3):
        _, totals = check([sets[n] for n in names[k:k + 3]], H, W)
        assert np.all(totals == H * W)


def test_unaligned_canvas_takes_the_byte_path():
    H, W = 37, 53
    sets = count_sets(H, W, 3)
    check([sets["blobs_zero_runs"], sets["checker1"], sets["vstripes"]], H, W, byte_offset=1)
    # W % 4 == 0 but the canvases one byte past a dword
    sets = count_sets(64, 128, 4)
    check([sets["blobs"], sets["full"], sets["hstripes"]], 64, 128, byte_offset=3)


@pytest.mark.parametrize("shape", [(37, 53), (64, 128)])
def test_slots(shape):
    H, W = shape
    hw = H * W
    sets = count_sets(H, W, 5)
    A, B, C = sets["blobs"], sets["vstripes"], sets["blobs_zero_runs"]
    la, lb, lc = len(A), len(B), len(C)
    runs = np.concatenate([A, B, C])
    cap = len(runs)
    full = [0, la, la + lb, cap]

    def run(offsets, cap=cap):
        got = gpu_decode(runs, offsets, H, W, cap=cap)
        want = expected(runs, offsets, H, W, cap=cap)
        assert np.array_equal(got[1], want[1]), (offsets, got[1], want[1])
        assert np.array_equal(got[0], want[0]), offsets
        return got

    _, t = run(full)
    assert t.tolist() == [hw, hw, hw]
    # an empty range between two good ones
    c, t = run([0, la, la, la + lb])
    assert t.tolist() == [hw, 0, hw] and not c[1].any() and c[0].any() and c[2].any()
    # a reversed range; the slot after it starts where the reversed one "ends"
    c, t = run([la, 0, la, la + lb])
    assert t.tolist() == [0, hw, hw] and not c[0].any()
    # a range that starts below 0, one that reaches past runs_cap, one that starts past it
    c, t = run([-3, la, la + lb, cap + 5, cap + 9])
    assert t.tolist() == [0, hw, 0, 0] and not c[0].any() and not c[2].any() and not c[3].any()
    # runs_cap below the buffer's content: the slots that reach past it are empty and the
    # prefix sum stops at the last run a valid slot owns
    c, t = run(full, cap=la + lb)
    assert t.tolist() == [hw, hw, 0]
    c, t = run(full, cap=la + lb - 1)
    assert t.tolist() == [hw, 0, 0]
    # a short sum and a long sum between intact neighbours: slot 1 loses B's last two
    # counts, slot 2 is those two and all of C
    c, t = run([0, la, la + lb - 2, cap])
    tail = int(B[-2:].astype(np.int64).sum())
    assert t.tolist() == [hw, hw - tail, hw + tail] and tail > 0
    # overlapping and repeated ranges: every slot reads its own
    c, t = run([0, la + lb, la, cap, 0, la])
    assert t.tolist() == [2 * hw, 0, 2 * hw, 0, hw]
    assert np.array_equal(c[4], R.decode_canvas(A, H, W)[0])
    # counts whose sum passes 2^32: the total is the true sum
    big = np.array([hw // 2, 0xFFFFFFFF, 0xFFFFFFFF, 7], np.uint32)
    c, t = gpu_decode(big, [0, 4], H, W)
    assert t.tolist() == [hw // 2 + 2 * 0xFFFFFFFF + 7]
    assert np.array_equal(c[0], R.decode_canvas(big, H, W)[0])


def test_nothing_to_decode():
    H, W = 37, 53
    # n == 0: nothing is touched
    flat = torch.full((GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
    totals = torch.full((3,), -1, dtype=torch.int64, device=DEV)
    work = torch.full((8,), -1, dtype=torch.int64, device=DEV)
    off_d = torch.zeros(1, dtype=torch.int64, device=DEV)
    _launch(None, 0, off_d, 0, H, W, flat, 0, totals, work)
    torch.cuda.synchronize()
    assert torch.all(flat == 0xFF) and torch.all(totals == -1) and torch.all(work == -1)
    # runs_cap == 0 with runs == NULL: every slot is the zero canvas
    flat = torch.full((2 * H * W + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
    off_d = torch.tensor([0, 0, 5], dtype=torch.int64, device=DEV)
    _launch(None, 0, off_d, 2, H, W, flat, 0, totals, work)
    torch.cuda.synchronize()
    assert not flat[:2 * H * W].any() and torch.all(flat[2 * H * W:] == 0xFF)
    assert totals.tolist() == [-1, 0, 0]


@pytest.mark.parametrize("shape", [(37, 53), (64, 128)])
def test_round_trip_on_the_device(shape):
    """isg_mask_rle's runs and offsets, still on the device, straight into the decoder."""
    H, W = shape
    p = patterns(H, W, 9)
    masks = np.stack([p["threshold"], p["ellipse"], p["checker1"], p["seam_both"]])
    K, sel = len(masks), [2, 0, 3, 1]
    M = torch.from_numpy(masks).to(DEV)
    S = torch.tensor(sel, dtype=torch.int32, device=DEV)
    N = torch.tensor([K], dtype=torch.int32, device=DEV)
    cap = K * (H * W + 1)
    runs = torch.full((cap,), -1, dtype=torch.int32, device=DEV)
    offsets = torch.full((K + 1,), -1, dtype=torch.int64, device=DEV)
    work = torch.empty(L.lib().isg_mask_rle_workspace(K, H, W), dtype=torch.uint8, device=DEV)
    L.check(L.lib().isg_mask_rle(M.data_ptr(), K, H, W, S.data_ptr(), N.data_ptr(), K,
                                 runs.data_ptr(), cap, offsets.data_ptr(), work.data_ptr(),
                                 L.stream_ptr()), "mask_rle")
    out = torch.full((K, H, W), 0xFF, dtype=torch.uint8, device=DEV)
    totals = torch.full((K,), -1, dtype=torch.int64, device=DEV)
    dwork = torch.full((L.lib().isg_mask_rle_decode_workspace(K, H, W, cap) // 8,), -1,
                       dtype=torch.int64, device=DEV)
    L.check(L.lib().isg_mask_rle_decode(runs.data_ptr(), cap, offsets.data_ptr(), K, H, W,
                                        out.data_ptr(), totals.data_ptr(), dwork.data_ptr(),
                                        L.stream_ptr()), "mask_rle_decode")
    torch.cuda.synchronize()
    assert totals.tolist() == [H * W] * K
    assert np.array_equal(out.cpu().numpy(), (masks[sel] >= 128).astype(np.uint8) * 255)


def test_captured_decode_replays_on_refilled_inputs():
    H, W = 64, 128
    sets = count_sets(H, W, 21)
    first = [sets["blobs"], sets["checker0"], sets["vstripes"]]
    second = [sets["hstripes"], sets["blobs_zero_runs"], sets["last"]]
    n, cap = 3, 3 * (H * W + 1)
    runs = torch.zeros(cap, dtype=torch.int32, device=DEV)
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    out = torch.full((n, H, W), 0xFF, dtype=torch.uint8, device=DEV)
    totals = torch.full((n,), -1, dtype=torch.int64, device=DEV)
    work = torch.full((L.lib().isg_mask_rle_decode_workspace(n, H, W, cap) // 8,), -1,
                      dtype=torch.int64, device=DEV)

    def fill(per):
        flat = np.concatenate(per)
        runs[:len(flat)].copy_(torch.from_numpy(flat.view(np.int32)))
        offsets.copy_(torch.from_numpy(np.concatenate([[0], np.cumsum([len(c) for c in per])])
                                       .astype(np.int64)))

    def decode():
        L.check(L.lib().isg_mask_rle_decode(runs.data_ptr(), cap, offsets.data_ptr(), n, H, W,
                                            out.data_ptr(), totals.data_ptr(), work.data_ptr(),
                                            L.stream_ptr()), "mask_rle_decode")

    fill(first)
    decode()  # first use outside the capture
    torch.cuda.synchronize()
    eager_first = out.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        decode()
    fill(second)
    out.fill_(0xFF)
    totals.fill_(-1)
    graph.replay()
    torch.cuda.synchronize()
    replayed, replayed_totals = out.clone(), totals.clone()
    out.fill_(0xFF)
    decode()  # eager, the same inputs
    torch.cuda.synchronize()
    assert torch.equal(replayed, out) and torch.equal(replayed_totals, totals)
    assert not torch.equal(replayed, eager_first)
    want = np.stack([R.decode_canvas(c, H, W)[0] for c in second])
    assert np.array_equal(replayed.cpu().numpy(), want) and totals.tolist() == [H * W] * n


# ---- RleDecoder ----------------------------------------------------------------------------
def test_rle_decoder_on_engine_strings():
    from instancesegmentation_amd.infer import InstanceSegmenter
    rng = np.random.Generator(np.random.PCG64(23))
    H, W = 192, 256
    img, boxes, kps = _scene(rng, H, W, 4, 3)
    eng = InstanceSegmenter(_calibrated(), (H, W), max_instances=8, iou_thr=0.5, rle=True)
    masks, keep, _ = eng(img, boxes, kps)
    segs, keep_r, _ = eng.result_rle()
    assert keep_r == keep and len(keep) > 0
    host = masks.cpu().numpy()
    assert any((host[i] >= 128).any() for i in keep)
    counts = [R.from_string(s["counts"]) for s in segs]
    dec = E.RleDecoder((H, W), max_masks=8, max_counts=2 * sum(len(c) for c in counts), device=DEV)
    dec.masks.fill_(0x5A)
    dec.work.fill_(-1)
    out = dec.decode(counts)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (len(keep), H, W) and out.is_cuda
    assert np.array_equal(out.cpu().numpy() >= 128, host[keep] >= 128)
    assert np.array_equal(out.cpu().numpy(), (host[keep] >= 128).astype(np.uint8) * 255)
    # into the matcher: the decoded canvases score as the engine's own
    gt = np.stack([np.roll(host[keep[0]], 5, axis=1), host[keep[-1]],
                   np.zeros_like(host[0])]).astype(np.uint8)
    matcher = E.MaskMatcher((H, W), max_det=8, max_gt=4, device=DEV)
    idx = torch.as_tensor(keep, dtype=torch.long, device=DEV)
    want = matcher.iou(masks[idx], gt)
    got = matcher.iou(out, gt)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    # strict: a bad slot raises and is named; without it the totals come back
    bad = [counts[0], counts[0][:-1], np.zeros(0, np.uint32)]
    with pytest.raises(ValueError, match="mask 1: counts sum to"):
        dec.decode(bad)
    canvases, totals = dec.decode(bad, strict=False)
    assert totals.tolist() == [H * W, H * W - int(counts[0][-1]), 0]
    assert np.array_equal(canvases[1].cpu().numpy(), R.decode_canvas(counts[0][:-1], H, W)[0])
    assert not canvases[2].any()
    assert tuple(dec.decode([]).shape) == (0, H, W)
    # the capacities
    with pytest.raises(ValueError, match="masks > capacity"):
        dec.decode([counts[0]] * 9)
    small = E.RleDecoder((H, W), max_masks=2, max_counts=len(counts[0]), device=DEV)
    assert np.array_equal(small.decode([counts[0]]).cpu().numpy(), out[:1].cpu().numpy())
    with pytest.raises(ValueError, match="counts > capacity"):
        small.decode([counts[0], np.array([H * W], np.uint32)])
    with pytest.raises(ValueError):
        E.RleDecoder((0, W), 2, 16, device=DEV)


# ---- python -m instancesegmentation_amd.evaluate -------------------------------------------
def test_offline_scorer_equals_the_online_evaluation(tmp_path, capsys):
    from PIL import Image

    from instancesegmentation_amd import infer as I
    from instancesegmentation_amd.data import ORDER_PART_NAMES
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
    plain = tmp_path / "plain"  # the masks the ground truth is cut from
    assert I.main(plain_args + ["-o", str(plain)]) == 0
    for name in names:
        res = json.load(open(plain / f"{name}.json"))
        ann = json.load(open(d / f"{name}.json"))
        for i, (obj, b) in enumerate(zip(ann["object"], scenes[name])):
            if i == 1:  # object 1 has no mask: it is not ground truth
                continue
            if i in res["keep"] and i % 2 == 0:  # the model's own mask, moved 3 px
                g = np.roll(np.asarray(Image.open(plain / name / f"{i}.png")), 3, axis=1)
            else:                                # its box, filled
                g = np.zeros((H, W), np.uint8)
                g[max(b[1], 0):b[3], max(b[0], 0):b[2]] = 255
            Image.fromarray(g).save(d / "gt" / f"{name}_{i}.png")
            obj["instance_mask"] = f"gt/{name}_{i}.png"
        with open(d / f"{name}.json", "w") as f:
            json.dump(ann, f)
    coco = tmp_path / "coco"
    assert I.main(plain_args + ["-o", str(coco), "--format", "coco", "--evaluate",
                                "--mask-root", str(d)]) == 0
    online = json.load(open(coco / "eval.json"))
    capsys.readouterr()
    offline_path = tmp_path / "offline_eval.json"
    assert E.main(["--results", str(coco / "results.json"), "-i", str(d), "--mask-root", str(d),
                   "-o", str(offline_path)]) == 0
    printed = capsys.readouterr().out
    offline = json.load(open(offline_path))
    print("offline summary:", offline["summary"])
    assert set(offline) == {"summary", "results", "images"}
    assert offline["results"] == str(coco / "results.json")
    assert offline["summary"] == online["summary"]
    assert offline["summary"]["detections"] > 0 and offline["summary"]["ground_truth"] == 6
    assert 0.0 < offline["summary"]["AP"] < 1.0
    assert printed.startswith("eval: AP ") and f"ground_truth {6}" in printed
    assert len(offline["images"]) == len(online["images"]) == 2
    for off, on in zip(offline["images"], online["images"]):
        assert set(off) == {"image", "detections", "matched_gt@0.5", "iou@0.5"}
        assert off["image"] == on["image"] and off["detections"] == len(on["keep"])
        assert off["matched_gt@0.5"] == on["matched_gt@0.5"] and off["iou@0.5"] == on["iou@0.5"]
    assert any(j >= 0 for im in offline["images"] for j in im["matched_gt@0.5"])
    # the default output: eval.json next to the results file
    assert E.main(["--results", str(coco / "results.json"), "-i", str(d)]) == 0
    assert json.load(open(coco / "eval.json")) == offline
    # uncompressed counts score the same
    results = json.load(open(coco / "results.json"))
    loose = [dict(r, segmentation={"size": r["segmentation"]["size"],
                                   "counts": [int(c) for c in
                                              R.from_string(r["segmentation"]["counts"])]})
             for r in results]
    with open(tmp_path / "loose.json", "w") as f:
        json.dump(loose, f)
    assert E.score_results(str(tmp_path / "loose.json"), str(d))["summary"] == offline["summary"]
    # one image's detections removed: its ground truth still counts, so the recall drops
    matched = [im["image"] for im in offline["images"] if any(j >= 0 for j in im["matched_gt@0.5"])]
    gone = R.image_id_of(matched[0][:-len(".png")])
    with open(tmp_path / "part.json", "w") as f:
        json.dump([r for r in results if r["image_id"] != gone], f)
    part = E.score_results(str(tmp_path / "part.json"), str(d))
    assert part["summary"]["images"] == 2 and part["summary"]["ground_truth"] == 6
    assert part["summary"]["detections"] < offline["summary"]["detections"]
    assert part["summary"]["AR"] < offline["summary"]["AR"]
    assert [im["detections"] for im in part["images"] if im["image"] == matched[0]] == [0]
    # a counts array that does not fill the image is refused, the detection named
    broken = [dict(r) for r in results]
    c = R.from_string(broken[1]["segmentation"]["counts"])
    broken[1]["segmentation"] = {"size": [H, W], "counts": [int(v) for v in c[:-1]]}
    with open(tmp_path / "broken.json", "w") as f:
        json.dump(broken, f)
    with pytest.raises(ValueError, match="counts sum to"):
        E.score_results(str(tmp_path / "broken.json"), str(d))
