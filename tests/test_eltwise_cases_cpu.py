"""The inputs of tests/test_gpu_eltwise.py have the properties its comparisons rely on
(tests/eltwise_cases.py), checked without a GPU: the bit-exact max-pool routing condition in
EVERY window, the number and the nature of every planted window, the tails' distance from the
activation's kink, and the lengths / value ranges of the loss, sigmoid and Adam inputs."""
import collections

import numpy as np
import pytest

from tests import eltwise_cases as EC

POOL_ALL = [(s, False) for s in EC.POOL_SHAPES] + [(s, True) for s in EC.POOL_SMALL_SHAPES]


@pytest.mark.parametrize("shape,small", POOL_ALL)
def test_pool_routing_condition_holds_in_every_window(shape, small):
    case = EC.pool_case(*shape, small=small)
    gap, pre = EC.pool_margins(case)
    nwin = EC.N * case["C"] * (case["H"] // case["k"]) * (case["W"] // case["k"])
    print(f"pool {shape} small={small}: {nwin} windows, {len(case['plants'])} planted; smallest "
          f"top-two gap elsewhere {gap:.3e}, smallest |activation argument| {pre:.3e}")
    assert gap >= EC.MARGIN and pre >= EC.MARGIN
    # the values are O(1): 1e-3 is ~1000 fp32 roundings of them
    v = EC.pool_input64(case)
    assert np.nanmax(np.abs(np.where(np.isinf(v), 0.0, v))) <= 50.0


def test_pool_shapes_reach_the_paths_they_are_meant_to():
    outs = [(H // k) * (W // k) for H, W, k in EC.POOL_SHAPES]
    assert outs == [360, 90, 168] and outs[0] - 256 == 104  # a second workgroup, 104 live lanes
    assert [k for _, _, k in EC.POOL_SHAPES] == [2, 4, 3]
    assert [sg[2] for sg in EC.POOL_SEGS] == [3, 5, 4]
    for H, W, k in EC.POOL_SHAPES + EC.POOL_SMALL_SHAPES:
        assert H % k == 0 and W % k == 0 and (H * W) % 4 == 0  # channel slices stay 16-B aligned


@pytest.mark.parametrize("shape,small", POOL_ALL)
def test_pool_planted_windows(shape, small):
    case = EC.pool_case(*shape, small=small)
    k = case["k"]
    kk = k * k
    counts = collections.Counter(p[0] for p in case["plants"])
    want = {"dup": 4, "relu_zero": 2} if small else \
        {"dup": 6, "relu_zero": 2, "neg_inf": 2, "nan_then_larger": 2, "two_nan": 2}
    assert counts == want
    # every segment holds a duplicate; the specials sit in the PLAIN segment only
    for sg in case["segs"]:
        inside = [p for p in case["plants"] if sg["c0"] <= p[2] < sg["c0"] + sg["C"]]
        assert sum(p[0] == "dup" for p in inside) == 2
        if sg["kind"] != "plain":
            assert all(p[0] in ("dup", "relu_zero") for p in inside)
    win = EC._windows(EC.pool_input64(case), k)
    out, idx = EC.pool_forward_ref(case)
    out, idx = out.numpy(), idx.numpy()
    W = case["W"]
    for kind, n, c, oy, ox in case["plants"]:
        w = win[n, c, oy, ox]
        flat = int(idx[n, c, oy, ox])
        local = (flat // W - oy * k) * k + (flat % W - ox * k)  # position in the window
        if kind == "dup":
            assert w[1] == w[kk - 1] == w.max() and w[1].tobytes() == w[kk - 1].tobytes()
            assert abs(w[1] - EC.DUP_VALUE) < 1e-5  # the raw value is rounded to fp32
            assert np.sort(w)[-3] <= w.max() - EC.MARGIN
            assert local == 1, "the first of two equal maxima wins"
        elif kind == "relu_zero":
            assert (w == 0.0).all() and local == 0 and out[n, c, oy, ox] == 0.0
        elif kind == "neg_inf":
            assert np.isneginf(w).all() and local == 0 and np.isneginf(out[n, c, oy, ox])
        elif kind == "nan_then_larger":
            assert np.isnan(w).sum() == 1 and np.isnan(w[1]) and w[2] == 50.0
            assert w[2] > np.nanmax(np.delete(w, 2))
            assert local == 1 and np.isnan(out[n, c, oy, ox]), "a NaN is not displaced"
        else:
            assert np.isnan(w).sum() == 2 and np.isnan(w[0]) and np.isnan(w[kk - 2])
            assert local == kk - 2 and np.isnan(out[n, c, oy, ox]), "the last NaN wins"
    # a planted window in the second workgroup of the 360-output case
    if shape == (40, 36, 2) and not small:
        assert any(oy * 18 + ox >= 256 for _, _, _, oy, ox in case["plants"])


def test_pool_backward_reference_routes_to_one_pixel_per_window():
    case = EC.pool_case(*EC.POOL_SHAPES[0])
    OH, OW = 20, 18
    dout = np.random.default_rng(1).normal(0, 1, (EC.N, case["C"], OH, OW)).astype(np.float32)
    dx, hit = EC.pool_backward_ref(case, dout)
    assert dx.dtype == np.float32 and hit.sum() == dout.size
    assert (dx[~hit] == 0).all() and np.array_equal(np.sort(dx[hit]), np.sort(dout.ravel()))


TAIL_ALL = [(f, a, s) for f, acts in (("a", ("prelu", "relu", "none")), ("b", ("prelu", "relu", "none")),
                                      ("c", ("prelu", "relu", "none")), ("c_null", ("prelu",)),
                                      ("d", ("prelu",)))
            for a in acts for s in EC.TAIL_SHAPES]


@pytest.mark.parametrize("form,act,shape", TAIL_ALL)
def test_tail_sum_stays_away_from_the_kink(form, act, shape):
    case = EC.tail_case(form, act, *shape)
    ref = EC.tail_ref(case)
    if act != "none":
        assert np.abs(ref["pre"]).min() >= EC.MARGIN
        assert (ref["pre"] > 0).mean() > 0.2 and (ref["pre"] < 0).mean() > 0.2  # both branches
    if form == "a":  # two BatchNorm terms: each centred on a clearly different mean
        m0, m1 = (EC.seg_mean_scale(t)[0] for t in case["terms"])
        assert np.abs(m0 - m1).min() > 0.5
        assert not np.allclose(ref["gxsum"][0], ref["gxsum"][1], rtol=1e-2)


def test_tail_shapes_reach_both_forms():
    units = {(H, W): ((H // 2) * (W // 2), (H // 2) * (W // 4), H * W) for H, W in EC.TAIL_SHAPES}
    assert units[(40, 36)][0] == 360                       # quad form, two workgroups
    assert units[(128, 128)][2] == 16384                   # exactly the 2x4 threshold
    assert units[(126, 132)][1] == 2079 and 2079 % 256     # 2x4 form, partial last workgroup
    assert 128 * 124 < 16384 and 124 % 4 == 0              # below the threshold: quad form
    assert 130 * 130 >= 16384 and 130 % 4 == 2             # above it, W % 4 != 0: quad form
    for H, W in EC.TAIL_SHAPES:
        assert H % 2 == 0 and W % 2 == 0 and (H * W) % 4 == 0  # channel slices stay 16-B aligned
        if H * W >= 16384 and W % 4 == 0:  # 2x4 form: an upsampled term's planes 8-B aligned
            assert ((H // 2) * (W // 2)) % 2 == 0


@pytest.mark.parametrize("n", EC.BCE_VEC_N + EC.BCE_SCALAR_N)
def test_bce_inputs(n):
    x, t, planted = EC.bce_inputs(n)
    assert planted.sum() == min(n, 30) and planted[0] and planted[-1]
    if n >= 30:
        got = {(float(a), float(np.float32(b))) for a, b in zip(x[planted], t[planted])}
        assert got == {(v, float(np.float32(tt))) for v in EC.BCE_PLANTED for tt in EC.BCE_PLANT_T}
    assert (np.abs(x[~planted]) <= 12.0).all()
    assert not ((np.abs(x) > 16.0) & (np.abs(x) < 18.0)).any()
    assert (t >= 0).all() and (t <= 1).all()
    if n >= 8188:
        hard = np.isin(t, (0.0, 1.0))
        q = np.isin(t, (np.arange(256) / 255.0).astype(np.float32))
        assert hard.mean() > 0.3 and (q & ~hard).mean() > 0.25 and (~q).mean() > 0.25
    assert (n % 4 == 0) == (n in EC.BCE_VEC_N)


def test_bce_lengths_reach_the_paths_they_are_meant_to():
    per_wg = 256 * 8  # quads per workgroup of the vector kernel
    assert 8192 // 4 == per_wg and 8196 // 4 == per_wg + 1 and 8188 // 4 == per_wg - 1
    assert (3 * 8192 + 148) // 4 == 3 * per_wg + 37
    assert 262144 + 3 > 1024 * 256  # past the scalar kernel's grid cap: a second iteration


@pytest.mark.parametrize("n", EC.SIGMOID_N)
def test_sigmoid_inputs(n):
    x, planted = EC.sigmoid_inputs(n)
    assert (np.abs(x[~planted]) <= 80.0).all() and planted.sum() == (4 if n > 4 else 0)
    ref = EC.sigmoid_ref64(x)
    assert (ref[~planted] >= float(np.finfo(np.float32).tiny)).all(), "no subnormal result"
    if n > 4:
        assert ref[planted].astype(np.float32).tolist() == [1.0, 0.0, 1.0, 0.0]
    assert max(EC.SIGMOID_N) > 2048 * 256  # past the grid cap


def test_adam_inputs():
    assert max(EC.ADAM_N) > 2048 * 256
    p, g, m, v, live = EC.adam_inputs(max(EC.ADAM_N), 2, True)
    assert 0.05 < 1.0 - live.mean() < 0.15 and live[0] == 0 and live[-1] == 0
    assert (v > 0).all() and np.abs(m).max() > 0
    for n in EC.ADAM_N:  # the effective gradient stays clear of 0 with and without decay
        for step in (1, 2, 1000):
            pp, gg, _, _, _ = EC.adam_inputs(n, step, False)
            for wd in (0.0, EC.ADAM_WD):
                ge = gg.astype(np.float64) + wd * pp.astype(np.float64)
                assert np.abs(ge).min() >= EC.ADAM_MIN_GE
    _, _, m1, v1, none = EC.adam_inputs(257, 1, False)
    assert none is None and not m1.any() and not v1.any()
