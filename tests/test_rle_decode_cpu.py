"""Host side of the RLE decode path (no GPU): rle.decode_canvas, the CPU statement of
csrc/mask_rle_decode.hip, on the encoder's pattern set and on hand-worked cases; the argument
checks of isg_mask_rle_decode (they answer before any HIP call); and the host half of the
offline scorer (image ids, grouping, the refusals of a results file)."""
import numpy as np
import pytest

from instancesegmentation_amd import _lib as L
from instancesegmentation_amd import evaluate as E
from instancesegmentation_amd import rle as R
from tests.test_gpu_rle import patterns

P = 0x1000  # any non-NULL, 16-B aligned value: nothing may dereference it


# ---- the CPU statement --------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1), (5, 3), (37, 53), (64, 128)])
def test_decode_canvas_inverts_encode(shape):
    H, W = shape
    for name, m in patterns(H, W, 11 * H + W).items():
        counts = R.encode(m)
        canvas, total = R.decode_canvas(counts, H, W)
        assert canvas.dtype == np.uint8 and canvas.shape == (H, W) and canvas.flags.c_contiguous
        assert total == H * W, name
        assert np.array_equal(canvas, (m >= 128).astype(np.uint8) * 255), name
        assert np.array_equal(canvas == 255, R.decode(counts, H, W)), name  # where decode is defined


def test_decode_canvas_hand_worked():
    H, W = 3, 4
    z = [0, 0, 0, 0]
    # zero-length runs in the middle: ends [3,3,5,9,9,9,12]; positions 5..8 are run 3 (odd),
    # positions 3..4 run 2 and 9..11 run 6 (even)
    canvas, total = R.decode_canvas([3, 0, 2, 4, 0, 0, 3], H, W)
    assert total == 12
    assert canvas.tolist() == [[0, 0, 255, 0], [0, 0, 255, 0], [0, 255, 255, 0]]
    assert np.array_equal(canvas == 255, R.decode([3, 0, 2, 4, 0, 0, 3], H, W))
    # a short sum: positions 2..4 set, everything from 5 on is background
    canvas, total = R.decode_canvas([2, 3], H, W)
    assert total == 5
    assert canvas.tolist() == [[0, 255, 0, 0], [0, 255, 0, 0], [255, 0, 0, 0]]
    # a short sum that ends inside a set run's successor: the tail after an even run too
    canvas, total = R.decode_canvas([2, 3, 1], H, W)
    assert total == 6 and canvas.tolist() == [[0, 255, 0, 0], [0, 255, 0, 0], [255, 0, 0, 0]]
    # a long sum: the set run [10, 15) is clipped at 12, the run after it ignored
    canvas, total = R.decode_canvas([10, 5, 4], H, W)
    assert total == 19
    assert canvas.tolist() == [z, [0, 0, 0, 255], [0, 0, 0, 255]]
    canvas, total = R.decode_canvas([0, 20, 7], H, W)
    assert total == 27 and np.all(canvas == 255)
    # a run that ends exactly on a column seam: column 1, whole
    canvas, total = R.decode_canvas([3, 3, 6], H, W)
    assert total == 12
    assert canvas.tolist() == [[0, 255, 0, 0]] * 3
    # empty counts
    canvas, total = R.decode_canvas([], H, W)
    assert total == 0 and canvas.shape == (H, W) and not canvas.any()
    canvas, total = R.decode_canvas(np.zeros(0, np.uint32), H, W)
    assert total == 0 and not canvas.any()
    # only zero-length runs; uint32 counts whose sum passes 2^32
    canvas, total = R.decode_canvas([0, 0, 0], H, W)
    assert total == 0 and not canvas.any()
    big = np.array([5, 0xFFFFFFFF, 0xFFFFFFFF], np.uint32)
    canvas, total = R.decode_canvas(big, H, W)
    assert total == 5 + 2 * 0xFFFFFFFF and canvas.T.reshape(-1).tolist() == [0] * 5 + [255] * 7
    with pytest.raises(ValueError):
        R.decode_canvas([3, -1, 10], H, W)
    # decode stays strict
    with pytest.raises(ValueError):
        R.decode([2, 3], H, W)


# ---- the library, without a GPU -----------------------------------------------------------
def test_symbols_present_and_abi_unchanged():
    lib = L.lib()
    assert hasattr(lib, "isg_mask_rle_decode") and hasattr(lib, "isg_mask_rle_decode_workspace")
    assert "isg_mask_rle_decode" in L.SIGNATURES and "isg_mask_rle_decode_workspace" in L.SIGNATURES
    assert lib.isg_abi_version() == 14 == L.ABI_VERSION  # additive symbols: the version stays


def test_decode_rejects_bad_arguments_before_any_hip_call():
    lib = L.lib()
    ok = dict(runs=P, cap=64, offsets=P, n=2, H=8, W=8, masks=P, totals=P, work=P)
    cases = ((dict(n=-1), b"bad sizes"), (dict(H=0), b"bad sizes"), (dict(H=-2), b"bad sizes"),
             (dict(W=0), b"bad sizes"), (dict(W=-3), b"bad sizes"), (dict(cap=-1), b"bad sizes"),
             (dict(H=1 << 16, W=1 << 15), b"2^31"), (dict(H=46341, W=46341), b"2^31"),
             (dict(runs=None), b"NULL"), (dict(offsets=None), b"NULL"),
             (dict(masks=None), b"NULL"), (dict(totals=None), b"NULL"), (dict(work=None), b"NULL"),
             (dict(offsets=P + 4), b"alignment"), (dict(totals=P + 4), b"alignment"),
             (dict(work=P + 4), b"alignment"), (dict(runs=P + 2), b"alignment"),
             (dict(runs=P + 1), b"alignment"))
    for kw, text in cases:
        a = dict(ok, **kw)
        rc = lib.isg_mask_rle_decode(a["runs"], a["cap"], a["offsets"], a["n"], a["H"], a["W"],
                                     a["masks"], a["totals"], a["work"], None)
        assert rc == -1, kw  # ISG_ERR_INVALID
        msg = lib.isg_last_error()
        assert b"mask_rle_decode" in msg and text in msg, (kw, msg)
    # a canvas pointer at any byte is not an error: nothing here may refuse it (n == 0 so
    # that nothing is launched)
    assert lib.isg_mask_rle_decode(P, 64, P, 0, 8, 8, P + 1, P, P, None) == 0
    # n == 0 is valid and touches nothing, NULL pointers included
    assert lib.isg_mask_rle_decode(None, 0, None, 0, 8, 8, None, None, None, None) == 0
    assert lib.isg_mask_rle_decode(None, 64, None, 0, 8, 8, None, None, None, None) == 0
    # but its sizes are still checked
    assert lib.isg_mask_rle_decode(None, 0, None, 0, 0, 8, None, None, None, None) == -1
    # more runs than a slot-relative index of 32 bits holds: unsupported, not invalid
    assert lib.isg_mask_rle_decode(P, 1 << 31, P, 1, 8, 8, P, P, P, None) == -2


def test_decode_workspace():
    ws = L.lib().isg_mask_rle_decode_workspace
    # the 64-bit prefix sums P[0 .. runs_cap] and one sum per chunk of 2048 runs
    assert ws(3, 8, 8, 0) == 8
    assert ws(3, 8, 8, 1) == 8 * (2 + 1)
    assert ws(3, 8, 8, 2048) == 8 * (2049 + 1)
    assert ws(16, 1024, 1024, 2049) == 8 * (2050 + 2)
    assert ws(0, 8, 8, 16) == 8 * (17 + 1)
    for bad in ((-1, 8, 8, 16), (1, 0, 8, 16), (1, 8, -1, 16), (1, 8, 8, -1),
                (1, 1 << 16, 1 << 15, 16), (1, 8, 8, 1 << 31)):
        assert ws(*bad) == -1, bad


# ---- the scorer's host half ---------------------------------------------------------------
def _rle(H, W, counts):
    return {"size": [H, W], "counts": counts}


def test_image_ids_and_grouping_keep_file_order():
    assert R.image_id_of("000000000042") == 42 and R.image_id_of("b") == "b"
    paths = ["/d/000000000042.png", "/d/b.jpg", "/d/c.png"]
    results = [{"image_id": "b", "score": 0.1, "k": 0}, {"image_id": 42, "score": 0.9, "k": 1},
               {"image_id": "b", "score": 0.7, "k": 2}, {"image_id": 42, "score": 0.2, "k": 3},
               {"image_id": "b", "score": 0.7, "k": 4}]
    groups = E.group_detections(results, paths)
    assert list(groups) == paths  # every image, in list order, the one without detections too
    assert [r["k"] for r in groups[paths[0]]] == [1, 3]
    assert [r["k"] for r in groups[paths[1]]] == [0, 2, 4]  # file order, not score order
    assert groups[paths[2]] == []
    assert E.group_detections([], paths) == {p: [] for p in paths}


def test_scorer_refusals():
    paths = ["/d/000000000042.png", "/d/b.png"]
    with pytest.raises(ValueError, match="matches no image"):
        E.group_detections([{"image_id": 43}], paths)
    with pytest.raises(ValueError, match="matches no image"):
        E.group_detections([{"image_id": "42"}], paths)  # the id of that file is the int
    with pytest.raises(ValueError, match="both map to image_id 42"):
        E.group_detections([], paths + ["/d/42.jpg"])
    with pytest.raises(ValueError, match="both map to image_id 'b'"):
        E.group_detections([], paths + ["/d/b.jpg"])
    with pytest.raises(ValueError, match="polygon"):
        E.segmentation_counts([[1.0, 2.0, 3.0, 4.0, 5.0, 6.0]], 4, 6)
    with pytest.raises(ValueError, match="size"):
        E.segmentation_counts(_rle(6, 4, [24]), 4, 6)
    with pytest.raises(ValueError):
        E.segmentation_counts(_rle(4, 6, [30, -6]), 4, 6)


def test_segmentation_counts_reads_both_forms():
    m = patterns(5, 3, 1)["ellipse"]
    counts = R.encode(m)
    for form in (R.to_string(counts), [int(c) for c in counts]):
        got = E.segmentation_counts(_rle(5, 3, form), 5, 3)
        assert got.dtype == np.uint32 and np.array_equal(got, counts)
    assert len(E.segmentation_counts(_rle(5, 3, []), 5, 3)) == 0


def test_scorer_command_line():
    a = E.parse_args(["--results", "out/results.json", "-i", "images"])
    assert (a.results, a.test_image_dir, a.mask_root, a.output) == ("out/results.json", "images",
                                                                   None, None)
    a = E.parse_args(["--results", "r.json", "-i", "d", "--mask-root", "m", "-o", "e.json"])
    assert (a.mask_root, a.output) == ("m", "e.json")
    with pytest.raises(RuntimeError, match="decode_canvas"):
        E.RleDecoder((8, 8), 2, 64, device="cpu")
