"""The CPU statements of the `counts` string codec (no GPU): rle.compress against
rle.to_string, rle.parse_total against rle.from_string and a plain big-integer reading of the
format, rle.summarize against rle.to_bbox / rle.area and against the box and area taken from
rle.decode_canvas's canvas; the host refusals of isg_rle_compress / isg_rle_parse (they answer
before any HIP call)."""
import numpy as np
import pytest

from instancesegmentation_amd import _lib as L
from instancesegmentation_amd import rle as R
from tests.rle_string_cases import CHUNK, SIZES, byte_strings, count_lists

P = 0x1000  # any non-NULL, 16-B aligned value: nothing may dereference it


def reference_parse(b):
    """(exact integer counts, status, from_string's answer or None where it raises): the
    format read byte by byte with Python integers, nothing wraps."""
    vals, status, acc, k = [], 0, [], 0
    for byte in b:
        if byte < 48 or byte > 111:
            status |= R.BAD_CHAR
        g = (byte - 48) & 0x3f
        acc.append(g)
        if not g & 0x20:
            if len(acc) > 7:
                status |= R.TOO_LONG
            last = acc[-7:]
            x = sum((q & 31) << (5 * m) for m, q in enumerate(last))
            if g & 0x10:
                x -= 1 << (5 * len(last))
            vals.append(x)
            acc = []
    if acc:
        status |= R.TRUNCATED
    counts = []
    for i, v in enumerate(vals):
        counts.append(v + counts[i - 2] if i >= 3 else v)
    if any(c < 0 or c >= 2 ** 32 for c in counts):
        status |= R.RANGE
    try:
        theirs = R.from_string(b)
    except ValueError as e:
        assert "truncated RLE string" in str(e)
        theirs = None
    except OverflowError:  # a count past 64 bits
        theirs = "overflow"
    return counts, status, theirs


@pytest.mark.parametrize("shape", SIZES)
def test_compress_is_to_string(shape):
    for name, c in count_lists(*shape).items():
        b = R.compress(c)
        assert isinstance(b, bytes) and b == R.to_string(c).encode(), name
    assert R.compress([]) == b"" and R.compress(np.zeros(0, np.uint32)) == b""


def test_compress_is_to_string_on_random_lists():
    rng = np.random.Generator(np.random.PCG64(7))
    for t in range(200):
        n = int(rng.integers(0, 40))
        bits = int(rng.integers(1, 33))  # every magnitude, so every group count
        c = rng.integers(0, 2 ** bits, n, dtype=np.uint64).astype(np.uint32)
        b = R.compress(c)
        assert b == R.to_string(c).encode(), c
        got, status = R.parse_total(b)
        assert status == 0 and got.dtype == np.uint32 and np.array_equal(got, c)
    with pytest.raises(ValueError):
        R.compress([1, -1])
    with pytest.raises(ValueError):
        R.compress([2 ** 32])


@pytest.mark.parametrize("shape", SIZES)
def test_parse_total_inverts_compress(shape):
    for name, c in count_lists(*shape).items():
        got, status = R.parse_total(R.compress(c))
        assert status == 0 and np.array_equal(got, c), name
        assert np.array_equal(R.from_string(R.compress(c)), c), name
        got, status = R.parse_total(R.to_string(c))  # str as well as bytes
        assert status == 0 and np.array_equal(got, c), name


def test_parse_total_flags_exactly_what_from_string_cannot_read():
    H, W = SIZES[0]
    seen = 0
    for name, b in byte_strings(H, W).items():
        counts, want, theirs = reference_parse(b)
        got, status = R.parse_total(b)
        assert status == want, (name, status, want)
        assert got.dtype == np.uint32 and got.tolist() == [c & 0xffffffff for c in counts], name
        # from_string raises exactly on the truncated ones, in these words
        assert (theirs is None) == bool(status & R.TRUNCATED), name
        if status == 0:  # well-formed: its answer
            assert np.array_equal(theirs, got), name
        elif not status & (R.TRUNCATED | R.BAD_CHAR) and not isinstance(theirs, str):
            # it read the string but could not hold a count: what it returns has wrapped
            # (RANGE), or comes from more groups than a count may have (TOO_LONG)
            exact = [int(v) for v in theirs.astype(np.int64)]
            assert status & R.TOO_LONG or exact != counts, name
        seen |= status
    assert seen == R.TRUNCATED | R.BAD_CHAR | R.TOO_LONG | R.RANGE
    assert R.status_text(R.TRUNCATED) == "truncated RLE string"
    assert R.status_text(0) == "" and "7 groups" in R.status_text(R.TOO_LONG | R.RANGE)


def test_parse_total_hand_worked():
    got, status = R.parse_total(b"")
    assert status == 0 and got.dtype == np.uint32 and len(got) == 0
    got, status = R.parse_total(b"5/3")  # '/' reads as a continuation of 31
    assert status == R.BAD_CHAR and got.tolist() == [5, 31 | (3 << 5)]
    got, status = R.parse_total(b"5p3")  # 'p' reads as the terminator 0
    assert status == R.BAD_CHAR and got.tolist() == [5, 0, 3]
    got, status = R.parse_total(b"1o")
    assert status == R.TRUNCATED and got.tolist() == [1]
    # eight groups: the first is dropped, the last seven are 1,1,1,1,1,1,1
    got, status = R.parse_total(bytes([99] + [81] * 6 + [49]))
    assert status == R.TOO_LONG and got.tolist() == [sum(1 << (5 * m) for m in range(7))]
    got, status = R.parse_total(bytes([81] * 6 + [49]))  # seven: a count like any other
    assert status == 0 and got.tolist() == [sum(1 << (5 * m) for m in range(7))]


@pytest.mark.parametrize("shape", SIZES)
def test_summarize(shape):
    H, W = shape
    n_full = 0
    for name, c in count_lists(H, W).items():
        box, area = R.summarize(c, H, W)
        assert all(type(v) is int for v in box) and type(area) is int, name
        canvas, total = R.decode_canvas(c, H, W)
        ys, xs = np.nonzero(canvas)
        want = ([0, 0, 0, 0] if not len(xs) else
                [int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1),
                 int(ys.max() - ys.min() + 1)])
        assert box == want and area == len(xs), (name, box, want)
        if total == H * W:
            n_full += 1
            assert box == R.to_bbox(c, H, W) and area == R.area(c), name
    assert n_full >= 4  # all_clear, all_set, borders, interior at the least
    assert R.summarize([], H, W) == ([0, 0, 0, 0], 0)
    with pytest.raises(ValueError):
        R.summarize([3, -1], H, W)


def test_summarize_hand_worked():
    H, W = 3, 4
    assert R.summarize([3, 3, 6], H, W) == ([1, 0, 1, 3], 3)      # column 1, whole
    assert R.summarize([2, 2, 8], H, W) == ([0, 0, 2, 3], 2)      # across the seam: y 0..2
    assert R.summarize([4, 1, 2, 1, 4], H, W) == ([1, 1, 2, 1], 2)
    assert R.summarize([10, 5, 4], H, W) == ([3, 1, 1, 2], 2)     # clipped at H*W
    assert R.summarize([0, 20, 7], H, W) == ([0, 0, 4, 3], 12)
    assert R.summarize([12, 5], H, W) == ([0, 0, 0, 0], 0)        # set past the canvas
    assert R.summarize([5, 0, 2, 0], H, W) == ([0, 0, 0, 0], 0)   # only empty set runs


# ---- the library, without a GPU -----------------------------------------------------------
def test_symbols_and_chunk():
    lib = L.lib()
    for name in ("isg_rle_compress", "isg_rle_compress_workspace", "isg_rle_parse",
                 "isg_rle_parse_workspace", "isg_rle_string_chunk"):
        assert hasattr(lib, name) and name in L.SIGNATURES
    assert lib.isg_rle_string_chunk() == CHUNK == L.RLE_STRING_CHUNK


def _compress(lib, **kw):
    a = dict(runs=P, cap=64, offsets=P, n=2, H=8, W=8, chars=P + 1, ccap=64, coff=P, boxes=P,
             areas=P, work=P)
    a.update(kw)
    return lib.isg_rle_compress(a["runs"], a["cap"], a["offsets"], a["n"], a["H"], a["W"],
                                a["chars"], a["ccap"], a["coff"], a["boxes"], a["areas"],
                                a["work"], None)


def _parse(lib, **kw):
    a = dict(chars=P + 3, ccap=64, coff=P, n=2, runs=P, cap=64, offsets=P, status=P, work=P)
    a.update(kw)
    return lib.isg_rle_parse(a["chars"], a["ccap"], a["coff"], a["n"], a["runs"], a["cap"],
                             a["offsets"], a["status"], a["work"], None)


def test_entries_refuse_bad_arguments_before_any_hip_call():
    lib = L.lib()
    invalid = ((dict(n=-1), b"bad sizes"), (dict(cap=-1), b"bad sizes"),
               (dict(ccap=-1), b"bad sizes"), (dict(H=0), b"bad sizes"), (dict(W=-2), b"bad sizes"),
               (dict(H=1 << 16, W=1 << 15), b"2^31"), (dict(H=46341, W=46341), b"2^31"),
               (dict(runs=None), b"NULL"), (dict(offsets=None), b"NULL"),
               (dict(chars=None), b"NULL"), (dict(coff=None), b"NULL"), (dict(boxes=None), b"NULL"),
               (dict(areas=None), b"NULL"), (dict(work=None), b"NULL"),
               (dict(offsets=P + 4), b"alignment"), (dict(coff=P + 4), b"alignment"),
               (dict(areas=P + 4), b"alignment"), (dict(work=P + 4), b"alignment"),
               (dict(runs=P + 2), b"alignment"), (dict(boxes=P + 1), b"alignment"))
    for kw, text in invalid:
        assert _compress(lib, **kw) == -1, kw  # ISG_ERR_INVALID
        msg = lib.isg_last_error()
        assert b"rle_compress" in msg and text in msg, (kw, msg)
    assert _compress(lib, cap=1 << 31) == -2 and _compress(lib, ccap=1 << 31) == -2
    # n == 0 does nothing, NULL pointers included; its sizes are still checked
    assert lib.isg_rle_compress(None, 0, None, 0, 8, 8, None, 0, None, None, None, None, None) == 0
    assert lib.isg_rle_compress(None, 0, None, 0, 0, 8, None, 0, None, None, None, None, None) == -1
    invalid = ((dict(n=-1), b"bad sizes"), (dict(cap=-1), b"bad sizes"),
               (dict(ccap=-1), b"bad sizes"), (dict(chars=None), b"NULL"),
               (dict(coff=None), b"NULL"), (dict(runs=None), b"NULL"),
               (dict(offsets=None), b"NULL"), (dict(status=None), b"NULL"),
               (dict(work=None), b"NULL"), (dict(coff=P + 4), b"alignment"),
               (dict(offsets=P + 4), b"alignment"), (dict(work=P + 4), b"alignment"),
               (dict(runs=P + 2), b"alignment"), (dict(status=P + 2), b"alignment"))
    for kw, text in invalid:
        assert _parse(lib, **kw) == -1, kw
        msg = lib.isg_last_error()
        assert b"rle_parse" in msg and text in msg, (kw, msg)
    assert _parse(lib, cap=1 << 31) == -2 and _parse(lib, ccap=1 << 31) == -2
    assert lib.isg_rle_parse(None, 0, None, 0, None, 0, None, None, None, None) == 0


def test_workspaces():
    lib = L.lib()
    assert lib.isg_rle_compress_workspace(16, 1 << 20) == 16 * 8
    assert lib.isg_rle_parse_workspace(3, 100) == 3 * 8
    assert lib.isg_rle_compress_workspace(0, 0) == 8 and lib.isg_rle_parse_workspace(0, 0) == 8
    for ws in (lib.isg_rle_compress_workspace, lib.isg_rle_parse_workspace):
        for bad in ((-1, 16), (1, -1), (1, 1 << 31)):
            assert ws(*bad) == -1, bad


def test_segmenter_arguments_need_rle():
    import inspect

    from instancesegmentation_amd.infer import InstanceSegmenter
    sig = inspect.signature(InstanceSegmenter.__init__).parameters
    assert sig["rle_strings"].default is False and sig["rle_chars_capacity"].default is None
