"""The case table of the `counts` string codec (rle.compress / summarize / parse_total and
csrc/mask_rle_string.hip), shared by test_rle_string_cpu.py and test_gpu_rle_string.py: the
inputs only, every expectation comes from the CPU statements (and, for those, from
rle.to_string / from_string / decode_canvas).

count_lists(H, W): name -> uint32 counts of one slot. byte_strings(H, W): name -> bytes of one
slot of the parser. CHUNK is what one workgroup takes per round; the lengths that cross it
are derived from it."""
import numpy as np

from instancesegmentation_amd import rle as R
from instancesegmentation_amd._lib import RLE_STRING_CHUNK as CHUNK

SIZES = [(33, 29), (1, 61), (61, 1)]  # the canvases the lists are summarised on
U32 = 2 ** 32 - 1


def _mask_counts(H, W, fn):
    m = np.zeros((H, W), np.uint8)
    fn(m)
    return R.encode(m)


def _frame(m):  # touches all four borders
    m[0] = m[-1] = 255
    m[:, 0] = m[:, -1] = 255


def _block(m):  # touches none (where the canvas has an interior)
    H, W = m.shape
    m[min(2, H - 1):max(H - 3, 1), min(3, W - 1):max(W - 2, 1)] = 255


def count_lists(H, W):
    hw = H * W
    rng = np.random.Generator(np.random.PCG64(1000 * H + W))
    c = {}
    # the delta rule starts at i = 3
    full = [5, 3, 2, 7, 1]
    for n in range(6):
        c[f"len{n}"] = full[:n]
    # every group boundary: the value just inside n groups and the first that needs n + 1,
    # as count 3's difference to count 1 in both signs, and as the raw counts 0..2
    for n in range(1, 7):
        b = 1 << (5 * n - 1)
        c[f"delta+{n}"] = [0, 0, 0, b - 1, 0, b]
        c[f"delta-{n}"] = [0, b, 0, 0, 0, 0, b + 1, 0, 0]
        c[f"raw{n}"] = [b - 1, b, b + 1]
    c["delta+7"] = [0, 0, 0, U32]
    c["delta-7"] = [0, U32, 0, 0]
    c["raw7"] = [U32, U32, U32, U32, 0, 0]
    c["zero_runs"] = [3, 0, 2, 4, 0, 0, 3]
    c["only_zero_runs"] = [0, 0, 0]
    c["all_clear"] = [hw]
    c["all_set"] = [0, hw]
    c["short_sum"] = [2, 3]
    c["short_sum_even"] = [2, 3, 1]
    c["long_sum"] = [max(hw - 2, 0), 5, 4]
    c["long_sum_first"] = [0, hw + 20, 7]
    c["past_2^32"] = [hw // 2, U32, U32, 7]
    c["checker_column"] = [1] * (2 * (H // 2) + 1) + [hw]
    c["checker"] = np.ones(hw, np.uint32)
    c["seam"] = [H - 1, 2, max(hw - H - 1, 0)] if W > 1 else [H - 1, 2]
    c["borders"] = _mask_counts(H, W, _frame)
    c["interior"] = _mask_counts(H, W, _block)
    # longer than one round of a workgroup by one, and by a round plus one: small counts (a
    # sum far past H*W), and 32-bit noise (7-group characters across the round's edge)
    c["chunk+1"] = rng.integers(0, 4, CHUNK + 1)
    c["2chunk+1"] = rng.integers(0, 3, 2 * CHUNK + 1)
    c["chunk+1_wide"] = rng.integers(0, 2 ** 32, CHUNK + 1, dtype=np.uint64)
    c["chunk_exact"] = rng.integers(0, 40, CHUNK)
    return {k: np.asarray(v, np.uint64).astype(np.uint32) for k, v in c.items()}


def write_values(values):
    """The bytes `compress` would write for the signed values themselves (no delta taken):
    how a string is made whose counts leave [0, 2^32)."""
    out = bytearray()
    for v in values:
        x = v if v >= 0 else -v - 1
        n = 1
        while x >= 1 << (5 * n - 1):
            n += 1
        for k in range(n):
            out.append((((v >> (5 * k)) & 31) | (32 if k < n - 1 else 0)) + 48)
    return bytes(out)


def byte_strings(H, W, cut=True):
    s = {}
    for name, c in count_lists(H, W).items():
        b = R.compress(c)
        s[name] = b
        if cut:  # cut after every one of its last 8 bytes (and before the first of them)
            for k in range(1, 9):
                if len(b) >= k:
                    s[f"{name}[:-{k}]"] = b[:len(b) - k]
    s["byte47"] = b"5/3"
    s["byte112"] = b"5p3"
    s["bytes_far"] = bytes([53, 0, 200, 255, 51])
    s["groups8"] = bytes([97] * 7 + [49])
    s["groups8_negative"] = bytes([97] * 7 + [49 + 16]) + b"3"
    s["groups13"] = b"2" + bytes([111] * 12 + [48]) + b"4"
    s["below0"] = write_values([5, 3, 2, -4, 1])
    s["below0_raw"] = write_values([5, -1])
    s["to_2^32"] = write_values([0, U32, 0, 1])
    s["just_inside"] = write_values([0, U32 - 1, 0, 1, 0, -U32])
    s["only_continuations"] = bytes([100] * 5)
    # a 7-group count at every alignment to the edge of a round: ending on it, straddling it
    # with 1..6 bytes before it, starting on it; a 13-group one across it
    for m in range(CHUNK - 7, CHUNK + 1):
        s[f"straddle{m - CHUNK}"] = b"1" * m + write_values([1 << 31, 1, -(1 << 31), 2])
    s["straddle_long"] = b"1" * (CHUNK - 5) + bytes([111] * 12 + [48]) + b"12"
    s["straddle_truncated"] = b"1" * (CHUNK - 3) + bytes([111] * 5)
    return s
