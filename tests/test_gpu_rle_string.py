"""The `counts` string codec on the MI355X (csrc/mask_rle_string.hip: isg_rle_compress,
isg_rle_parse) against its CPU statements (rle.compress / summarize / parse_total), bit-exact
on the table of rle_string_cases.py, several slots per launch. Every output and workspace is
poisoned (0xFF) before every call, chars and runs sit between guard bytes, every launch is
made twice with equal results. Then void and overlapping slots, output overflow, an unaligned
chars pointer, the host refusals, the device round trip with the encoder and the decoder, a
captured graph, InstanceSegmenter(rle_strings=True), the infer CLI and the offline scorer."""
import json
import warnings

import numpy as np
import pytest
import torch

from instancesegmentation_amd import _lib as L
from instancesegmentation_amd import evaluate as E
from instancesegmentation_amd import rle as R
from tests.rle_string_cases import CHUNK, SIZES, byte_strings, count_lists
from tests.test_gpu_rle import _calibrated, _scene, patterns

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def gpu_compress(runs, offsets, H, W, cap=None, chars_cap=None, byte_offset=0):
    """isg_rle_compress on the slots `offsets` of `runs`, twice -> (chars uint8 [chars_cap],
    char_offsets [n+1], boxes [n,4], areas [n]) of the second call, equal to the first's."""
    runs = np.asarray(runs, np.uint32)
    offsets = np.asarray(offsets, np.int64)
    n = len(offsets) - 1
    cap = len(runs) if cap is None else cap
    chars_cap = 7 * max(len(runs), 1) * max(n, 1) if chars_cap is None else chars_cap
    runs_d = _dev(np.concatenate([runs, np.full(GUARD, 0xFFFFFFFF, np.uint32)]).view(np.int32))
    off_d = _dev(offsets)
    ws = L.lib().isg_rle_compress_workspace(n, cap)
    assert ws >= 8 and ws % 8 == 0
    got = []
    for _ in range(2):
        flat = torch.full((GUARD + byte_offset + chars_cap + GUARD,), 0xFF, dtype=torch.uint8,
                          device=DEV)
        coff = torch.full((n + 3,), -1, dtype=torch.int64, device=DEV)
        boxes = torch.full((n + 2, 4), -1, dtype=torch.int32, device=DEV)
        areas = torch.full((n + 2,), -1, dtype=torch.int64, device=DEV)
        work = torch.full((ws // 8,), -1, dtype=torch.int64, device=DEV)
        L.check(L.lib().isg_rle_compress(runs_d.data_ptr(), cap, off_d.data_ptr(), n, H, W,
                                         flat.data_ptr() + GUARD + byte_offset, chars_cap,
                                         coff.data_ptr() + 8, boxes.data_ptr() + 16,
                                         areas.data_ptr() + 8, work.data_ptr(), L.stream_ptr()),
                "rle_compress")
        torch.cuda.synchronize()
        f, co, bx, ar = (t.cpu().numpy() for t in (flat, coff, boxes, areas))
        lo = GUARD + byte_offset
        assert np.all(f[:lo] == 0xFF) and np.all(f[lo + chars_cap:] == 0xFF)  # guards intact
        assert co[0] == -1 and co[-1] == -1 and ar[0] == -1 and ar[-1] == -1
        assert np.all(bx[0] == -1) and np.all(bx[-1] == -1)
        got.append((f[lo:lo + chars_cap], co[1:-1], bx[1:-1], ar[1:-1]))
    for a, b in zip(*got):
        assert np.array_equal(a, b)
    return got[1]


def want_compress(runs, offsets, H, W, cap=None):
    runs = np.asarray(runs, np.uint32)
    cap = len(runs) if cap is None else cap
    strings, boxes, areas = [], [], []
    for a, b in zip(offsets[:-1], offsets[1:]):
        c = runs[a:b] if 0 <= a < b <= cap else np.zeros(0, np.uint32)
        strings.append(R.compress(c))
        box, area = R.summarize(c, H, W)
        boxes.append(box)
        areas.append(area)
    coff = np.concatenate([[0], np.cumsum([len(s) for s in strings])]).astype(np.int64)
    return b"".join(strings), coff, np.asarray(boxes, np.int32).reshape(-1, 4), \
        np.asarray(areas, np.int64)


def check_compress(runs, offsets, H, W, **kw):
    chars, coff, boxes, areas = gpu_compress(runs, offsets, H, W, **kw)
    w_chars, w_coff, w_boxes, w_areas = want_compress(runs, offsets, H, W, kw.get("cap"))
    assert np.array_equal(coff, w_coff), (coff, w_coff)
    assert np.array_equal(boxes, w_boxes), (boxes, w_boxes)
    assert np.array_equal(areas, w_areas), (areas, w_areas)
    k = min(len(w_chars), len(chars))
    assert chars[:k].tobytes() == w_chars[:k]
    assert np.all(chars[k:] == 0xFF)  # nothing written past the total
    return chars, coff, boxes, areas


def gpu_parse(chars, char_offsets, cap=None, runs_cap=None, byte_offset=0):
    """isg_rle_parse on the slots `char_offsets` of `chars`, twice -> (runs uint32 [runs_cap],
    offsets [n+1], status [n])."""
    chars = np.frombuffer(bytes(chars), np.uint8)
    char_offsets = np.asarray(char_offsets, np.int64)
    n = len(char_offsets) - 1
    cap = len(chars) if cap is None else cap
    runs_cap = max(len(chars), 1) * max(n, 1) if runs_cap is None else runs_cap
    buf = np.full(GUARD + byte_offset + len(chars) + GUARD, 0x30, np.uint8)  # '0's around it
    buf[GUARD + byte_offset:GUARD + byte_offset + len(chars)] = chars
    chars_d = _dev(buf)
    coff_d = _dev(char_offsets)
    ws = L.lib().isg_rle_parse_workspace(n, cap)
    assert ws >= 8 and ws % 8 == 0
    got = []
    for _ in range(2):
        runs = torch.full((GUARD + runs_cap + GUARD,), -1, dtype=torch.int32, device=DEV)
        off = torch.full((n + 3,), -1, dtype=torch.int64, device=DEV)
        status = torch.full((n + 2,), -1, dtype=torch.int32, device=DEV)
        work = torch.full((ws // 8,), -1, dtype=torch.int64, device=DEV)
        L.check(L.lib().isg_rle_parse(chars_d.data_ptr() + GUARD + byte_offset, cap,
                                      coff_d.data_ptr(), n, runs.data_ptr() + 4 * GUARD, runs_cap,
                                      off.data_ptr() + 8, status.data_ptr() + 4,
                                      work.data_ptr(), L.stream_ptr()), "rle_parse")
        torch.cuda.synchronize()
        r, o, s = runs.cpu().numpy().view(np.uint32), off.cpu().numpy(), status.cpu().numpy()
        assert np.all(r[:GUARD] == 0xFFFFFFFF) and np.all(r[GUARD + runs_cap:] == 0xFFFFFFFF)
        assert o[0] == -1 and o[-1] == -1 and s[0] == -1 and s[-1] == -1
        got.append((r[GUARD:GUARD + runs_cap], o[1:-1], s[1:-1]))
    for a, b in zip(*got):
        assert np.array_equal(a, b)
    return got[1]


def want_parse(chars, char_offsets, cap=None):
    chars = bytes(chars)
    cap = len(chars) if cap is None else cap
    per, status = [], []
    for a, b in zip(char_offsets[:-1], char_offsets[1:]):
        c, s = R.parse_total(chars[a:b] if 0 <= a < b <= cap else b"")
        per.append(c)
        status.append(s)
    off = np.concatenate([[0], np.cumsum([len(c) for c in per])]).astype(np.int64)
    runs = np.concatenate(per) if per else np.zeros(0, np.uint32)
    return runs.astype(np.uint32), off, np.asarray(status, np.int32)


def check_parse(chars, char_offsets, **kw):
    runs, off, status = gpu_parse(chars, char_offsets, **kw)
    w_runs, w_off, w_status = want_parse(chars, char_offsets, kw.get("cap"))
    assert np.array_equal(off, w_off), (off, w_off)
    assert np.array_equal(status, w_status), (status, w_status)
    k = min(len(w_runs), len(runs))
    assert np.array_equal(runs[:k], w_runs[:k])
    assert np.all(runs[k:] == 0xFFFFFFFF)
    return runs, off, status


def _packed(per):
    flat = np.concatenate([np.asarray(p) for p in per]) if per else np.zeros(0, np.uint32)
    off = np.concatenate([[0], np.cumsum([len(p) for p in per])]).astype(np.int64)
    return flat, off


# ---- bit-exact on the table --------------------------------------------------------------
@pytest.mark.parametrize("shape", SIZES)
def test_compress_table(shape):
    H, W = shape
    lists = count_lists(H, W)
    names = sorted(lists)
    for k in range(0, len(names), 12):  # a dozen slots per launch, len0 (void) among them
        runs, off = _packed([lists[n] for n in names[k:k + 12]])
        check_compress(runs, off, H, W)


def test_parse_table():
    H, W = SIZES[0]
    strings = byte_strings(H, W)
    names = sorted(strings)
    for k in range(0, len(names), 64):
        flat, off = _packed([np.frombuffer(strings[n], np.uint8) for n in names[k:k + 64]])
        check_parse(flat.astype(np.uint8).tobytes(), off)


def test_unaligned_chars_pointer():
    H, W = SIZES[0]
    lists = count_lists(H, W)
    per = [lists["chunk+1_wide"], lists["borders"], lists["raw7"], lists["2chunk+1"]]
    runs, off = _packed(per)
    for byte_offset in (1, 2, 3):
        check_compress(runs, off, H, W, byte_offset=byte_offset)
    strings = [R.compress(c) for c in per] + [byte_strings(H, W, cut=False)["straddle-3"]]
    flat, coff = _packed([np.frombuffer(s, np.uint8) for s in strings])
    for byte_offset in (1, 2, 3):
        check_parse(flat.astype(np.uint8).tobytes(), coff, byte_offset=byte_offset)


# ---- slots ---------------------------------------------------------------------------------
def test_void_and_overlapping_slots():
    H, W = SIZES[0]
    lists = count_lists(H, W)
    A, B, C = lists["borders"], lists["seam"], lists["chunk+1"]
    la, lb = len(A), len(B)
    runs = np.concatenate([A, B, C])
    cap = len(runs)
    for offsets, kw in (([0, la, la, la + lb], {}),                  # an empty range
                        ([la, 0, la, la + lb], {}),                  # a reversed one
                        ([-3, la, la + lb, cap + 5, cap + 9], {}),   # below 0, past the capacity
                        ([0, la, la + lb, cap], dict(cap=la + lb)),  # the capacity below the content
                        ([0, la, la + lb, cap], dict(cap=la + lb - 1)),
                        ([0, la + lb, la, cap, 0, la], {}),          # overlapping and repeated
                        ([cap, cap, cap], {})):                      # the slots past *nkeep
        _, coff, boxes, areas = check_compress(runs, np.asarray(offsets, np.int64), H, W, **kw)
    assert coff.tolist() == [0, 0, 0] and not boxes.any() and not areas.any()
    strings = [R.compress(c) for c in (A, B, C)]
    flat = b"".join(strings)
    sa, sb = len(strings[0]), len(strings[1])
    cap = len(flat)
    for offsets, kw in (([0, sa, sa, sa + sb], {}), ([sa, 0, sa, sa + sb], {}),
                        ([-3, sa, sa + sb, cap + 5, cap + 9], {}),
                        ([0, sa, sa + sb, cap], dict(cap=sa + sb)),
                        ([0, sa, sa + sb, cap], dict(cap=sa + sb - 1)),
                        ([0, sa + sb, sa, cap, 0, sa], {}),
                        ([1, sa, sa - 1, cap - 1], {}),  # ranges that start and end inside counts
                        ([cap, cap, cap], {})):
        _, off, status = check_parse(flat, np.asarray(offsets, np.int64), **kw)
    assert off.tolist() == [0, 0, 0] and status.tolist() == [0, 0]


def test_nothing_to_do():
    lib, st = L.lib(), L.stream_ptr()
    out = torch.full((64,), -1, dtype=torch.int64, device=DEV)
    p = out.data_ptr()
    # n == 0: nothing is touched
    assert lib.isg_rle_compress(None, 0, p, 0, 8, 8, None, 0, p, p, p, p, st) == 0
    assert lib.isg_rle_parse(None, 0, p, 0, None, 0, p, p, p, st) == 0
    torch.cuda.synchronize()
    assert torch.all(out == -1)
    # capacity 0 with NULL pointers: every slot is void, the outputs say so
    off = torch.tensor([0, 0, 5], dtype=torch.int64, device=DEV)
    coff = torch.full((3,), -1, dtype=torch.int64, device=DEV)
    boxes = torch.full((2, 4), -1, dtype=torch.int32, device=DEV)
    areas = torch.full((2,), -1, dtype=torch.int64, device=DEV)
    work = torch.full((2,), -1, dtype=torch.int64, device=DEV)
    L.check(lib.isg_rle_compress(None, 0, off.data_ptr(), 2, 8, 8, None, 0, coff.data_ptr(),
                                 boxes.data_ptr(), areas.data_ptr(), work.data_ptr(), st))
    status = torch.full((2,), -1, dtype=torch.int32, device=DEV)
    roff = torch.full((3,), -1, dtype=torch.int64, device=DEV)
    L.check(lib.isg_rle_parse(None, 0, off.data_ptr(), 2, None, 0, roff.data_ptr(),
                              status.data_ptr(), work.data_ptr(), st))
    torch.cuda.synchronize()
    assert coff.tolist() == [0, 0, 0] and not boxes.any() and not areas.any()
    assert roff.tolist() == [0, 0, 0] and status.tolist() == [0, 0]


def test_output_overflow_keeps_true_offsets():
    H, W = SIZES[0]
    lists = count_lists(H, W)
    per = [lists["borders"], lists["raw7"], lists["chunk+1_wide"], lists["interior"]]
    runs, off = _packed(per)
    w_chars, w_coff, _, _ = want_compress(runs, off, H, W)
    total = len(w_chars)
    # capacities that cut inside a slot, inside a count's groups (raw7's are 7 bytes each),
    # on a slot's edge, in the last dword
    for ccap in (0, 1, int(w_coff[1]) + 3, int(w_coff[1]) + 10, int(w_coff[2]),
                 int(w_coff[2]) + CHUNK + 5, total - 1, total - 5):
        chars, coff, _, _ = check_compress(runs, off, H, W, chars_cap=ccap)
        assert len(chars) == ccap and coff[-1] == total > ccap
        assert chars.tobytes() == w_chars[:ccap]
    strings = [R.compress(c) for c in per]
    flat, coff = _packed([np.frombuffer(s, np.uint8) for s in strings])
    flat = flat.astype(np.uint8).tobytes()
    w_runs, w_off, _ = want_parse(flat, coff)
    for rcap in (0, 1, int(w_off[1]) + 2, int(w_off[2]), int(w_off[2]) + CHUNK - 1,
                 len(w_runs) - 1):
        got, off_g, status = check_parse(flat, coff, runs_cap=rcap)
        assert len(got) == rcap and off_g[-1] == len(w_runs) > rcap and not status.any()
        assert np.array_equal(got, w_runs[:rcap])
    # status does not depend on the capacity either
    bad = byte_strings(H, W, cut=False)
    flat, coff = _packed([np.frombuffer(bad[k], np.uint8)
                          for k in ("to_2^32", "groups13", "straddle_truncated", "byte47")])
    _, _, status = check_parse(flat.astype(np.uint8).tobytes(), coff, runs_cap=3)
    assert status.tolist() == [R.RANGE, R.TOO_LONG, R.TRUNCATED, R.BAD_CHAR]


def test_host_refusals_touch_nothing():
    lib, st = L.lib(), L.stream_ptr()
    buf = torch.full((4096,), 0xFF, dtype=torch.uint8, device=DEV)
    p = buf.data_ptr()
    ok_c = [p, 64, p, 2, 8, 8, p, 64, p, p, p, p]
    ok_p = [p, 64, p, 2, p, 64, p, p, p]

    def bad(args, at, value):
        a = list(args)
        a[at] = value
        return a
    invalid_c = [(3, -1), (1, -1), (7, -1), (4, 0), (5, -1), (0, None), (2, None), (6, None),
                 (8, None), (9, None), (10, None), (11, None), (2, p + 4), (8, p + 4),
                 (10, p + 4), (11, p + 4), (0, p + 2), (9, p + 2)]
    for at, value in invalid_c:
        assert lib.isg_rle_compress(*bad(ok_c, at, value), st) == -1, (at, value)
        assert b"rle_compress" in lib.isg_last_error()
    assert lib.isg_rle_compress(*bad(bad(ok_c, 4, 1 << 16), 5, 1 << 15), st) == -1
    assert lib.isg_rle_compress(*bad(ok_c, 1, 1 << 31), st) == -2
    assert lib.isg_rle_compress(*bad(ok_c, 7, 1 << 31), st) == -2
    invalid_p = [(3, -1), (1, -1), (5, -1), (0, None), (2, None), (4, None), (6, None),
                 (7, None), (8, None), (2, p + 4), (6, p + 4), (8, p + 4), (4, p + 2), (7, p + 2)]
    for at, value in invalid_p:
        assert lib.isg_rle_parse(*bad(ok_p, at, value), st) == -1, (at, value)
        assert b"rle_parse" in lib.isg_last_error()
    assert lib.isg_rle_parse(*bad(ok_p, 1, 1 << 31), st) == -2
    assert lib.isg_rle_parse(*bad(ok_p, 5, 1 << 31), st) == -2
    assert lib.isg_rle_compress_workspace(2, 1 << 31) == -1
    assert lib.isg_rle_parse_workspace(-1, 8) == -1
    torch.cuda.synchronize()
    assert torch.all(buf == 0xFF)


# ---- with the encoder and the decoder ----------------------------------------------------------
class Codec:
    """isg_mask_rle -> isg_rle_compress -> isg_rle_parse -> isg_mask_rle_decode over static
    buffers, every hand-over on the device."""

    def __init__(self, K, H, W):
        lib = L.lib()
        self.K, self.H, self.W = K, H, W
        self.cap = K * (H * W + 1)
        self.ccap = 2 * self.cap
        i32, i64 = torch.int32, torch.int64
        self.masks = torch.zeros((K, H, W), dtype=torch.uint8, device=DEV)
        self.runs = torch.full((self.cap,), -1, dtype=i32, device=DEV)
        self.offsets = torch.full((K + 1,), -1, dtype=i64, device=DEV)
        self.work = torch.empty(lib.isg_mask_rle_workspace(K, H, W), dtype=torch.uint8, device=DEV)
        self.chars = torch.full((self.ccap,), 0xFF, dtype=torch.uint8, device=DEV)
        self.coff = torch.full((K + 1,), -1, dtype=i64, device=DEV)
        self.boxes = torch.full((K, 4), -1, dtype=i32, device=DEV)
        self.areas = torch.full((K,), -1, dtype=i64, device=DEV)
        self.cwork = torch.full((lib.isg_rle_compress_workspace(K, self.cap) // 8,), -1, dtype=i64,
                                device=DEV)
        self.runs2 = torch.full((self.cap,), -1, dtype=i32, device=DEV)
        self.offsets2 = torch.full((K + 1,), -1, dtype=i64, device=DEV)
        self.status = torch.full((K,), -1, dtype=i32, device=DEV)
        self.pwork = torch.full((lib.isg_rle_parse_workspace(K, self.ccap) // 8,), -1, dtype=i64,
                                device=DEV)
        self.out = torch.full((K, H, W), 0x5A, dtype=torch.uint8, device=DEV)
        self.totals = torch.full((K,), -1, dtype=i64, device=DEV)
        self.dwork = torch.full((lib.isg_mask_rle_decode_workspace(K, H, W, self.cap) // 8,), -1,
                                dtype=i64, device=DEV)

    def encode(self):
        L.check(L.lib().isg_mask_rle(self.masks.data_ptr(), self.K, self.H, self.W, None, None,
                                     self.K, self.runs.data_ptr(), self.cap,
                                     self.offsets.data_ptr(), self.work.data_ptr(),
                                     L.stream_ptr()), "mask_rle")

    def strings(self):
        lib, st, K = L.lib(), L.stream_ptr(), self.K
        L.check(lib.isg_rle_compress(self.runs.data_ptr(), self.cap, self.offsets.data_ptr(), K,
                                     self.H, self.W, self.chars.data_ptr(), self.ccap,
                                     self.coff.data_ptr(), self.boxes.data_ptr(),
                                     self.areas.data_ptr(), self.cwork.data_ptr(), st),
                "rle_compress")
        L.check(lib.isg_rle_parse(self.chars.data_ptr(), self.ccap, self.coff.data_ptr(), K,
                                  self.runs2.data_ptr(), self.cap, self.offsets2.data_ptr(),
                                  self.status.data_ptr(), self.pwork.data_ptr(), st), "rle_parse")

    def decode(self):
        L.check(L.lib().isg_mask_rle_decode(self.runs2.data_ptr(), self.cap,
                                            self.offsets2.data_ptr(), self.K, self.H, self.W,
                                            self.out.data_ptr(), self.totals.data_ptr(),
                                            self.dwork.data_ptr(), L.stream_ptr()),
                "mask_rle_decode")

    def check(self, masks):
        """Everything the chain left, against the host's codec on `masks`."""
        torch.cuda.synchronize()
        coff = self.coff.cpu().numpy()
        chars = self.chars.cpu().numpy().tobytes()
        for j, m in enumerate(masks):
            c = R.encode(m)
            assert chars[coff[j]:coff[j + 1]].decode() == R.to_string(c), j
            assert self.boxes[j].tolist() == R.to_bbox(c, self.H, self.W), j
            assert int(self.areas[j]) == R.area(c), j
        assert torch.equal(self.offsets2, self.offsets) and not self.status.any()
        total = int(self.offsets[-1])
        assert torch.equal(self.runs2[:total], self.runs[:total])
        assert self.totals.tolist() == [self.H * self.W] * self.K
        assert np.array_equal(self.out.cpu().numpy(), (masks >= 128).astype(np.uint8) * 255)


NAMES = ["threshold", "ellipse", "checker1", "seam_both", "zero", "full", "first", "last",
         "checker0", "checker2d", "vstripes", "hstripes", "seam_bottom", "seam_top"]


@pytest.mark.parametrize("shape", [(33, 29), (64, 128)])
def test_round_trip_on_the_device(shape):
    H, W = shape
    p = patterns(H, W, 9)
    masks = np.stack([p[k] for k in NAMES])
    codec = Codec(len(masks), H, W)
    codec.masks.copy_(_dev(masks))
    codec.encode()
    codec.strings()
    codec.decode()
    codec.check(masks)


def test_captured_codec_replays_on_refilled_inputs():
    H, W = 64, 128
    p = patterns(H, W, 21)
    first = np.stack([p["ellipse"], p["checker0"], p["vstripes"]])
    second = np.stack([p["hstripes"], p["threshold"], p["seam_both"]])
    codec = Codec(3, H, W)
    codec.masks.copy_(_dev(first))
    codec.encode()
    codec.strings()  # first use outside the capture
    torch.cuda.synchronize()
    first_chars = codec.chars.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        codec.strings()
    codec.masks.copy_(_dev(second))
    codec.encode()
    for t in (codec.chars, codec.runs2):
        t.fill_(-1 if t.dtype != torch.uint8 else 0xFF)
    for t in (codec.coff, codec.boxes, codec.areas, codec.cwork, codec.offsets2, codec.status,
              codec.pwork):
        t.fill_(-1)
    graph.replay()
    codec.decode()
    codec.check(second)
    assert not torch.equal(codec.chars, first_chars)


# ---- InstanceSegmenter ----------------------------------------------------------------------
def test_instance_segmenter_rle_strings():
    from instancesegmentation_amd.infer import InstanceSegmenter
    rng = np.random.Generator(np.random.PCG64(23))
    H, W = 192, 256
    m = _calibrated()
    img, boxes, kps = _scene(rng, H, W, 4, 3)
    img2, boxes2, kps2 = _scene(rng, H, W, 5, 2)
    host = InstanceSegmenter(m, (H, W), max_instances=8, iou_thr=0.5, rle=True)
    eng = InstanceSegmenter(m, (H, W), max_instances=8, iou_thr=0.5, rle=True, rle_strings=True)
    assert eng.rle_chars_capacity == 2 * eng.rle_capacity
    want = None
    for scene in ((img, boxes, kps), (img2, boxes2, kps2)):  # the second through the replay
        host(*scene)
        eng(*scene)
        want = host.result_rle()
        got = eng.result_rle()
        assert got[0] == want[0] and got[1] == want[1] and np.array_equal(got[2], want[2])
        segs, bxs, areas, keep, scores = eng.result_coco()
        assert segs == want[0] and keep == want[1] and np.array_equal(scores, want[2])
        assert len(keep) > 0 and any(areas)
        for sg, b, a in zip(segs, bxs, areas):
            c = R.from_string(sg["counts"])
            assert b == R.to_bbox(c, H, W) and all(type(v) is int for v in b)
            assert a == R.area(c) and type(a) is int
    # forced overflows of either capacity: the same answers, one warning
    n0 = len(R.from_string(want[0][0]["counts"]))
    for kw in (dict(rle_capacity=n0 + 3), dict(rle_chars_capacity=len(want[0][0]["counts"]) + 3)):
        tiny = InstanceSegmenter(m, (H, W), max_instances=8, iou_thr=0.5, capture=False, rle=True,
                                 rle_strings=True, **kw)
        tiny.load(img2, boxes2, kps2)
        tiny.run()
        with pytest.warns(RuntimeWarning, match="RLE buffer overflow") as rec:
            coco = tiny.result_coco()
        assert len(rec) == 1
        assert coco[0] == segs and coco[1] == bxs and coco[2] == areas and coco[3] == keep
        with warnings.catch_warnings():  # it warns once
            warnings.simplefilter("error")
            assert tiny.result_rle()[0] == segs
    with pytest.raises(ValueError, match="rle=True"):
        InstanceSegmenter(m, (H, W), max_instances=8, capture=False, rle_strings=True)
    with pytest.raises(RuntimeError, match="rle_strings"):
        host.result_coco()


# ---- the command lines -----------------------------------------------------------------------
def _dataset(tmp_path):
    """Two images with sidecars and ground truth (boxes, filled), a checkpoint."""
    from PIL import Image

    from instancesegmentation_amd.data import ORDER_PART_NAMES
    rng = np.random.Generator(np.random.PCG64(31))
    H, W = 192, 256
    m = _calibrated()
    d = tmp_path / "images"
    (d / "gt").mkdir(parents=True)
    for name in ("000000000042", "b"):
        img, boxes, kps = _scene(rng, H, W, 3, 1)
        Image.fromarray(img).save(d / f"{name}.png")
        objs = []
        for i, (b, k) in enumerate(zip(boxes, kps)):
            g = np.zeros((H, W), np.uint8)
            g[max(b[1], 0):b[3], max(b[0], 0):b[2]] = 255
            Image.fromarray(g).save(d / "gt" / f"{name}_{i}.png")
            objs.append({"box": [int(v) for v in b], "instance_mask": f"gt/{name}_{i}.png",
                         "body_keypoint": {ORDER_PART_NAMES[j]: {
                             "status": "vis" if k[j, 2] > 0 else "missing",
                             "point": [float(k[j, 0]), float(k[j, 1])]} for j in range(17)}})
        with open(d / f"{name}.json", "w") as f:
            json.dump({"object": objs}, f)
    ck = tmp_path / "m.pth"
    torch.save({"state_dict": {k: v.cpu() for k, v in m.state_dict().items()}}, ck)
    return d, ck


def test_command_lines_write_the_same_files(tmp_path, monkeypatch):
    from instancesegmentation_amd import infer as I
    d, ck = _dataset(tmp_path)
    argv = ["-i", str(d), "--checkpoint", str(ck), "--max-instances", "4", "--format", "coco",
            "--evaluate"]
    dev_out, host_out = tmp_path / "device", tmp_path / "host"
    made = []
    real = I.InstanceSegmenter

    def recording(*a, **kw):
        made.append(real(*a, **kw))
        return made[-1]
    monkeypatch.setattr(I, "InstanceSegmenter", recording)
    assert I.main(argv + ["-o", str(dev_out)]) == 0
    assert made and all(e.rle_strings for e in made)  # the CLI asks for the device strings
    # the host path, through the constructor argument
    monkeypatch.setattr(I, "InstanceSegmenter",
                        lambda *a, **kw: real(*a, **dict(kw, rle_strings=False)))
    assert I.main(argv + ["-o", str(host_out)]) == 0
    names = sorted(p.name for p in host_out.iterdir())
    assert names == sorted(p.name for p in dev_out.iterdir())
    assert names == ["000000000042.json", "b.json", "eval.json", "results.json"]
    for name in names:
        assert (dev_out / name).read_bytes() == (host_out / name).read_bytes(), name
    results = json.load(open(dev_out / "results.json"))
    assert len(results) > 0 and all(isinstance(r["segmentation"]["counts"], str) for r in results)
    # the offline scorer: decode_strings gives the eval.json that decode gives
    monkeypatch.undo()
    through_strings = tmp_path / "eval_strings.json"
    assert E.main(["--results", str(dev_out / "results.json"), "-i", str(d), "-o",
                   str(through_strings)]) == 0
    calls = []
    real_strings = E.RleDecoder.decode_strings
    monkeypatch.setattr(E.RleDecoder, "decode_strings",
                        lambda self, *a, **kw: calls.append(1) or real_strings(self, *a, **kw))
    assert E.score_results(str(dev_out / "results.json"), str(d)) == \
        json.load(open(through_strings))
    assert calls  # that was the device parser
    monkeypatch.undo()
    loose = [dict(r, segmentation={"size": r["segmentation"]["size"],
                                   "counts": [int(c) for c in
                                              R.from_string(r["segmentation"]["counts"])]})
             for r in results]
    with open(tmp_path / "loose.json", "w") as f:
        json.dump(loose, f)
    through_counts = E.score_results(str(tmp_path / "loose.json"), str(d))
    got = json.load(open(through_strings))
    assert got["summary"] == through_counts["summary"] and got["images"] == through_counts["images"]
    assert got["summary"]["detections"] == len(results) and got["summary"]["ground_truth"] == 8
    # a truncated string is refused, the detection named; so is one among uncompressed counts
    cut = [dict(r) for r in results]
    s = cut[1]["segmentation"]["counts"]
    while not (ord(s[-2]) - 48) & 0x20:  # cut inside a count
        s = s[:-1]
    cut[1]["segmentation"] = {"size": cut[1]["segmentation"]["size"], "counts": s[:-1]}
    with open(tmp_path / "cut.json", "w") as f:
        json.dump(cut, f)
    image = "000000000042.png" if cut[1]["image_id"] == 42 else "b.png"
    at = sum(r["image_id"] == cut[1]["image_id"] for r in cut[:1])  # its place in its image
    with pytest.raises(ValueError, match=f"{image}, detection {at}: truncated RLE string"):
        E.score_results(str(tmp_path / "cut.json"), str(d))
    cut[0] = loose[0]
    with open(tmp_path / "cut.json", "w") as f:
        json.dump(cut, f)
    with pytest.raises(ValueError, match=f"{image}, detection {at}: truncated RLE string"):
        E.score_results(str(tmp_path / "cut.json"), str(d))


def test_decode_strings():
    H, W = 64, 128
    p = patterns(H, W, 5)
    masks = np.stack([p["ellipse"], p["threshold"], p["seam_both"], p["zero"]])
    counts = [R.encode(m) for m in masks]
    strings = [R.to_string(c) for c in counts]
    dec = E.RleDecoder((H, W), max_masks=4, max_counts=sum(len(c) for c in counts), device=DEV)
    dec.masks.fill_(0x5A)
    # more bytes than max_counts, but not more counts: the terminators are counted
    assert sum(len(s) for s in strings) > dec.max_counts
    out = dec.decode_strings(strings)
    assert np.array_equal(out.cpu().numpy(), (masks >= 128).astype(np.uint8) * 255)
    assert torch.equal(out, dec.decode(counts).clone())
    out, totals = dec.decode_strings([s.encode() for s in strings[:2]], strict=False)
    assert totals.tolist() == [H * W] * 2 and tuple(out.shape) == (2, H, W)
    assert tuple(dec.decode_strings([]).shape) == (0, H, W)
    with pytest.raises(ValueError, match="mask 1: counts sum to"):
        dec.decode_strings([strings[0], R.to_string(counts[0][:-1])])
    with pytest.raises(ValueError, match="mask 2: truncated RLE string"):
        dec.decode_strings([strings[0], strings[1], "5o"])
    with pytest.raises(ValueError, match="mask 0: .*outside"):
        dec.decode_strings(["5/3"], strict=False)
    with pytest.raises(ValueError, match="masks > capacity"):
        dec.decode_strings(strings + ["1"])
    with pytest.raises(ValueError, match="counts > capacity"):
        dec.decode_strings(strings[:3] + ["1" * (len(counts[3]) + 1)])
