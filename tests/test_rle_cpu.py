"""instancesegmentation_amd/rle.py: the COCO RLE contract on the CPU (numpy only).

The vectors were computed by an independent implementation of the COCO string format
(the first four also by hand); `pycocotools` is not a dependency."""
import json

import numpy as np
import pytest

from instancesegmentation_amd import rle

VECTORS = [
    ([3, 2, 4], "324"),
    ([3, 2, 4, 5], "3243"),
    ([3, 5, 4, 2], "354M"),
    ([16], "`0"),
    ([0, 12], "0<"),
    ([1048576], "PPPP1"),
    ([0, 1048576], "0PPPP1"),
    ([5, 1024, 7, 1000, 40000, 3], "5PP17XOiQW1kPO"),
]

EXAMPLE = np.array([[0, 128, 0], [255, 0, 0], [255, 0, 200], [0, 0, 127]], np.uint8)


@pytest.mark.parametrize("counts,string", VECTORS)
def test_string_vectors_both_directions(counts, string):
    assert rle.to_string(counts) == string
    got = rle.from_string(string)
    assert got.dtype == np.uint32 and got.tolist() == counts
    assert rle.from_string(string.encode("ascii")).tolist() == counts


def test_string_round_trip_random_counts():
    rng = np.random.Generator(np.random.PCG64(5))
    for n in (1, 2, 3, 4, 5, 17, 200):
        for hi in (1, 2, 33, 1 << 10, 1 << 20, 1 << 31):
            c = rng.integers(0, hi, n, dtype=np.int64)
            c[rng.uniform(size=n) < 0.2] = 0
            c[rng.uniform(size=n) < 0.1] = 2 ** 31 - 1
            s = rle.to_string(c)
            assert all(48 <= ord(ch) < 48 + 64 for ch in s)
            assert rle.from_string(s).tolist() == c.tolist(), (n, hi)
    edge = [0, 2 ** 31 - 1, 0, 0, 2 ** 31 - 1, 2 ** 31 - 1, 0, 1, 15, 16, 31, 32]
    assert rle.from_string(rle.to_string(edge)).tolist() == edge


def test_encode_example():
    c = rle.encode(EXAMPLE)
    assert c.dtype == np.uint32 and c.tolist() == [1, 2, 1, 1, 5, 1, 1]
    assert rle.to_string(c) == "121O40L"
    assert rle.encode(np.zeros((4, 3), np.uint8)).tolist() == [12]
    assert rle.encode(np.full((4, 3), 255, np.uint8)).tolist() == [0, 12]
    assert rle.encode(EXAMPLE >= 128).tolist() == c.tolist()  # bool masks pass as they are


SHAPES = [(1, 1), (1, 9), (9, 1), (4, 3), (5, 8), (33, 17), (64, 40)]


@pytest.mark.parametrize("shape", SHAPES)
def test_decode_inverts_encode_and_area_bbox(shape):
    rng = np.random.Generator(np.random.PCG64(shape[0] * 131 + shape[1]))
    H, W = shape
    masks = [rng.integers(0, 256, shape, dtype=np.uint8),
             rng.integers(126, 130, shape, dtype=np.uint8),
             np.zeros(shape, np.uint8), np.full(shape, 255, np.uint8)]
    blob = np.zeros(shape, np.uint8)
    blob[H // 3:H // 3 + max(1, H // 2), W // 4:W // 4 + max(1, W // 3)] = 200
    masks.append(blob)
    col = np.zeros(shape, np.uint8)  # a set run that crosses a column seam
    col[H - 1, 0] = 255
    col[0, W - 1] = 255
    masks.append(col)
    for m in masks:
        c = rle.encode(m)
        assert 1 <= len(c) <= H * W + 1 and int(c.astype(np.int64).sum()) == H * W
        d = rle.decode(c, H, W)
        ref = m >= 128
        assert d.dtype == np.bool_ and np.array_equal(d, ref)
        assert np.array_equal(rle.decode(rle.from_string(rle.to_string(c)), H, W), ref)
        assert rle.area(c) == int(ref.sum())
        ys, xs = np.nonzero(ref)
        box = [0, 0, 0, 0] if not len(xs) else [int(xs.min()), int(ys.min()),
                                                int(xs.max() - xs.min() + 1),
                                                int(ys.max() - ys.min() + 1)]
        assert rle.to_bbox(c, H, W) == box


def test_decode_rejects_wrong_size():
    with pytest.raises(ValueError):
        rle.decode([3, 2, 4], 2, 2)


def test_results_assembly(tmp_path):
    seg = lambda m: {"size": list(m.shape), "counts": rle.to_string(rle.encode(m))}  # noqa: E731
    a = {"image": "000000000139.jpg", "instances": 3, "keep": [2, 0],
         "scores": [0.5, 0.25, 0.75], "segmentation": [seg(EXAMPLE), seg(EXAMPLE.T)],
         "bbox": [[0, 0, 3, 3], [0, 0, 3, 3]]}
    b = {"image": "street.png", "instances": 1, "keep": [0], "scores": [0.125],
         "segmentation": [seg(EXAMPLE)], "bbox": [[0, 0, 3, 3]]}
    empty = {"image": "7.jpg", "instances": 0, "keep": [], "scores": [], "segmentation": [],
             "bbox": []}
    png_run = {"image": "old.png", "instances": 1, "keep": [0], "scores": [0.5]}
    for name, res in (("000000000139", a), ("street", b), ("7", empty), ("old", png_run)):
        with open(tmp_path / f"{name}.json", "w") as f:
            json.dump(res, f)
    with open(tmp_path / "results.json", "w") as f:  # a stale file is not an input
        json.dump([{"image_id": 1}], f)
    got = rle.write_results(str(tmp_path))
    assert got == json.load(open(tmp_path / "results.json"))
    assert [(r["image_id"], r["score"]) for r in got] == [(139, 0.75), (139, 0.5),
                                                          ("street", 0.125)]
    for r in got:
        assert r["category_id"] == 1 and set(r) == {"image_id", "category_id", "segmentation",
                                                    "bbox", "score"}
    assert got[0]["segmentation"] == seg(EXAMPLE) and got[1]["segmentation"] == seg(EXAMPLE.T)
    # running it again (a --continue-test run) gives the same file
    assert rle.write_results(str(tmp_path)) == got
