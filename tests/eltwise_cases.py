"""What tests/test_gpu_eltwise.py feeds the element-wise kernels (max-pool, residual tails,
sigmoid + BCE, sigmoid, Adam) and the fp64 references it compares them with. numpy and torch
on the CPU only: tests/test_eltwise_cases_cpu.py proves, without a GPU, that the generated
inputs have the properties the GPU comparisons rely on.

Every input is an fp32 array; a reference converts it to fp64 (exactly) and evaluates the
documented formula there (include/isg.h)."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

EPS = float(np.float32(1e-5))  # BatchNorm eps as the kernels see it: the fp32 value, widened
N = 2

# Distance the generators keep (a) between the two largest values of a pooling window and
# (b) between an activation's argument and 0; the tests assert MARGIN of it survives the
# inversion to fp32 raw values. MARGIN is about a thousand times the fp32 error of the
# kernels' (x - mean) * gamma*rstd + beta on O(1) values (a few 2^-24).
GEN_MARGIN = 4e-3
MARGIN = 1e-3


def _act64(z, act, slope):
    if act == "relu":
        return np.maximum(z, 0.0)
    if act == "prelu":
        return np.where(z > 0, z, z * slope[None, :, None, None])
    return z


def _bn_params(rng, C):
    """gamma (either sign), beta, slope as fp32 and (mean, var) as fp64."""
    gamma = (rng.uniform(0.5, 1.5, C) * rng.choice([-1.0, 1.0], C)).astype(np.float32)
    beta = rng.uniform(-0.5, 0.5, C).astype(np.float32)
    slope = rng.uniform(0.05, 0.4, C).astype(np.float32)
    return gamma, beta, slope, rng.uniform(-1.0, 1.0, C), rng.uniform(0.5, 2.0, C)


def stats_block(mean, var, M):
    """[sum | sumsq | 0 | 0] (fp64, 4*C) of a layer whose batch mean and biased variance over
    M values per channel are (about) mean and var."""
    s = M * mean
    return np.concatenate([s, M * (var + mean * mean), np.zeros_like(s), np.zeros_like(s)])


def mean_rstd_of_stats(stats, C, M):
    """isg.h isg_bn, train: mean = sum/M, biased variance clamped at 0, rstd in fp64."""
    mean = stats[:C] / M
    var = np.maximum(stats[C:2 * C] / M - mean * mean, 0.0)
    return mean, 1.0 / np.sqrt(var + EPS)


def seg_mean_scale(sg):
    """(mean, gamma*rstd, beta) in fp64 of a BatchNorm segment, whatever carries them."""
    g, b = sg["gamma"].astype(np.float64), sg["beta"].astype(np.float64)
    if sg["kind"] == "bn_eval":
        mean = sg["rm"].astype(np.float64)
        rstd = 1.0 / np.sqrt(sg["rv"].astype(np.float64) + EPS)
    else:  # bn_train, coef: the statistics block
        mean, rstd = mean_rstd_of_stats(sg["stats"], sg["C"], sg["count"])
    return mean, g * rstd, b


def coef_block(sg):
    """The finalised forward coefficients of isg_bn.coef: [C][4] = (mean, gamma*rstd, beta, 0)
    as fp32 (rounded once from fp64, as isg_bn_finalize does)."""
    mean, scale, beta = seg_mean_scale(sg)
    return np.stack([mean, scale, beta, np.zeros_like(mean)], 1).astype(np.float32)


# ---- max-pool ------------------------------------------------------------------------------
POOL_SHAPES = [(40, 36, 2), (40, 36, 4), (36, 42, 3)]       # (H, W, k), segments 3 + 5 + 4
POOL_SMALL_SHAPES = [(12, 24, 2), (12, 24, 4), (12, 24, 3)]  # segments 2 + 3
POOL_SEGS = [("plain", "none", 3), ("bn_eval", "relu", 5), ("bn_train", "prelu", 4)]
POOL_SMALL_SEGS = [("act_only", "prelu", 2), ("coef", "relu", 3)]
DUP_VALUE = 6.0


def _windows(a, k):
    """[N, C, H, W] -> [N, C, OH, OW, k*k] in the kernels' visiting order (dy, then dx)."""
    n, c, h, w = a.shape
    return a.reshape(n, c, h // k, k, w // k, k).transpose(0, 1, 2, 4, 3, 5).reshape(
        n, c, h // k, w // k, k * k)


def _unwindows(wn, k):
    n, c, oh, ow, _ = wn.shape
    return wn.reshape(n, c, oh, ow, k, k).transpose(0, 1, 2, 4, 3, 5).reshape(n, c, oh * k, ow * k)


def top2_gap(v, k):
    """Per window the largest value minus the second largest ([N, C, OH, OW])."""
    s = np.sort(_windows(v, k), axis=-1)
    return s[..., -1] - s[..., -2]


def _draw_z(rng, shape, k, act, slope):
    """Activation arguments whose windows satisfy the routing condition with GEN_MARGIN."""
    def away(z):
        return z if act == "none" else np.where(np.abs(z) < GEN_MARGIN, 0.5, z)
    z = away(rng.normal(0.0, 1.0, shape))
    for _ in range(200):
        wn = _windows(z, k)
        bad = top2_gap(_act64(z, act, slope), k) < GEN_MARGIN
        if not bad.any():
            return z
        wn[bad] = rng.normal(0.0, 1.0, (int(bad.sum()), k * k))
        z = away(_unwindows(wn, k))
    raise AssertionError("the window redraw did not converge")


def _plant_list(H, W, k, segs):
    """(kind, n, global channel, oy, ox): windows of both images, of the first and the last
    workgroup in x, never the same window twice."""
    OH, OW = H // k, W // k
    plants, c0 = [], 0
    for kind, act, C in segs:
        plants += [("dup", 0, c0 + C - 1, OH - 1, OW - 2), ("dup", 1, c0, 0, 1)]
        if act == "relu":
            plants += [("relu_zero", 0, c0 + 1, 2, 3), ("relu_zero", 1, c0 + C - 1, OH - 1, OW - 1)]
        if kind == "plain":
            plants += [("neg_inf", 0, c0, 1, 1), ("neg_inf", 1, c0 + 1, OH - 1, 0),
                       ("nan_then_larger", 0, c0 + 1, 2, 2), ("nan_then_larger", 1, c0 + 2, OH - 2, OW - 1),
                       ("two_nan", 1, c0, 2, 5), ("two_nan", 0, c0, OH - 1, OW - 1)]
        c0 += C
    assert len({p[1:] for p in plants}) == len(plants)
    return plants


@functools.lru_cache(maxsize=None)
def pool_case(H, W, k, small=False):
    """{"segs": [...], "x": per-segment raw fp32 [N, C, H, W], "plants": [...]} — read-only."""
    spec = POOL_SMALL_SEGS if small else POOL_SEGS
    rng = np.random.default_rng(1000 * H + 10 * W + k + (7 if small else 0))
    M = float(N * H * W)
    segs, c0 = [], 0
    plants = _plant_list(H, W, k, spec)
    for kind, act, C in spec:
        gamma, beta, slope, mean, var = _bn_params(rng, C)
        sg = {"kind": kind, "act": act, "C": C, "c0": c0, "slope": slope, "count": M}
        if kind in ("bn_train", "coef"):
            sg.update(gamma=gamma, beta=beta, stats=stats_block(mean, var, M))
        elif kind == "bn_eval":
            sg.update(gamma=gamma, beta=beta, rm=mean.astype(np.float32), rv=var.astype(np.float32))
        z = _draw_z(rng, (N, C, H, W), k, act, slope.astype(np.float64))
        wz = _windows(z, k)
        for pk, n, c, oy, ox in plants:
            if not c0 <= c < c0 + C:
                continue
            if pk == "dup":          # the maximum at position 1 and again at the last position
                wz[n, c - c0, oy, ox, 1] = wz[n, c - c0, oy, ox, k * k - 1] = DUP_VALUE
            elif pk == "relu_zero":  # every pre-activation negative: an all-zero window
                wz[n, c - c0, oy, ox] = -np.abs(wz[n, c - c0, oy, ox])
        z = _unwindows(wz, k)
        if kind in ("plain", "act_only"):
            x = z.astype(np.float32)
        else:
            mu, scale, b = seg_mean_scale(sg)
            bc = lambda a: a[None, :, None, None]
            x = ((z - bc(b)) / bc(scale) + bc(mu)).astype(np.float32)
        wx = _windows(x, k)
        for pk, n, c, oy, ox in plants:
            if not c0 <= c < c0 + C:
                continue
            w_ = wx[n, c - c0, oy, ox]
            if pk == "dup":
                w_[k * k - 1] = w_[1]  # bit-equal raw values: bit-equal transformed values
            elif pk == "neg_inf":
                w_[:] = -np.inf
            elif pk == "nan_then_larger":
                w_[1], w_[2] = np.nan, 50.0
            elif pk == "two_nan":
                w_[0] = w_[k * k - 2] = np.nan
            wx[n, c - c0, oy, ox] = w_
        sg["x"] = np.ascontiguousarray(_unwindows(wx, k))
        sg["x"].setflags(write=False)
        segs.append(sg)
        c0 += C
    return {"H": H, "W": W, "k": k, "C": c0, "segs": segs, "plants": plants}


def seg_pre64(sg):
    """fp64 argument of the segment's activation (the raw values for a PLAIN segment)."""
    x = sg["x"].astype(np.float64)
    if sg["kind"] in ("plain", "act_only"):
        return x
    mu, scale, b = seg_mean_scale(sg)
    bc = lambda a: a[None, :, None, None]
    with np.errstate(invalid="ignore"):
        return (x - bc(mu)) * bc(scale) + bc(b)


def pool_input64(case):
    """The fp64-transformed input [N, C, H, W] the pool sees."""
    return np.concatenate([_act64(seg_pre64(sg), sg["act"], sg["slope"].astype(np.float64))
                           for sg in case["segs"]], 1)


def pool_planted_mask(case):
    m = np.zeros((N, case["C"], case["H"] // case["k"], case["W"] // case["k"]), bool)
    for _, n, c, oy, ox in case["plants"]:
        m[n, c, oy, ox] = True
    return m


def pool_margins(case):
    """(smallest top-two gap over EVERY window that holds no plant, smallest |activation
    argument| over every element of the activated segments)."""
    with np.errstate(invalid="ignore"):
        gap = top2_gap(pool_input64(case), case["k"])
    gap = np.where(pool_planted_mask(case), np.inf, gap)
    pre = [np.abs(seg_pre64(sg)).min() for sg in case["segs"] if sg["act"] != "none"]
    return float(gap.min()), float(min(pre)) if pre else float("inf")


def pool_forward_ref(case):
    """(F.max_pool2d of the fp64-transformed input, its flat argmax indices)."""
    v = torch.from_numpy(pool_input64(case))
    return F.max_pool2d(v, case["k"], case["k"], return_indices=True)


def pool_backward_ref(case, dout):
    """torch's CPU max_pool2d backward of the fp64-routed argmax: (dx as fp32 — every value
    is one fp32 dout value or 0, so the fp64 route is exact — and the argmax mask)."""
    v = torch.from_numpy(pool_input64(case)).requires_grad_(True)
    out, idx = F.max_pool2d(v, case["k"], case["k"], return_indices=True)
    out.backward(torch.from_numpy(dout).double())
    hit = torch.zeros(N, case["C"], case["H"] * case["W"], dtype=torch.bool)
    hit.scatter_(2, idx.reshape(N, case["C"], -1), True)
    return v.grad.float().numpy(), hit.reshape(N, case["C"], case["H"], case["W"]).numpy()


# ---- residual tails ------------------------------------------------------------------------
TAIL_C = 5
TAIL_SHAPES = [(40, 36), (128, 128), (126, 132), (128, 124), (130, 130)]
# form -> (term kinds, x2-upsampled?, dterm of each term: None / "store" / "accum")
TAIL_FORMS = {
    "a": (["bn_train", "bn_train"], [0, 0], [None, None]),
    "b": (["bn_eval", "plain"], [0, 0], [None, "store"]),
    "c": (["bn_train", "plain", "plain"], [0, 0, 1], [None, "accum", "store"]),
    "c_null": (["bn_train", "plain", "plain"], [0, 0, 1], [None, None, "store"]),
    "d": (["bn_train"], [0], [None]),
}


@functools.lru_cache(maxsize=None)
def tail_case(form, act, H, W):
    kinds, ups, dts = TAIL_FORMS[form]
    rng = np.random.default_rng(7919 * H + 31 * W + 5 * len(kinds) + len(act))
    C = TAIL_C
    terms = []
    for i, (kind, up) in enumerate(zip(kinds, ups)):
        h, w = (H // 2, W // 2) if up else (H, W)
        # BatchNorm'd terms with clearly different means and spreads (their own statistics)
        x = (rng.normal(0.0, 1.0 + 0.5 * i, (N, C, h, w)) + (0.2, -0.7, 0.6)[i]).astype(np.float32)
        tm = {"kind": kind, "up": up, "C": C, "x": x, "dterm": dts[i], "count": float(N * H * W)}
        if kind != "plain":
            gamma, beta, _, mean, var = _bn_params(rng, C)
            tm.update(gamma=gamma, beta=beta)
            if kind == "bn_train":  # the batch statistics of x itself
                x64 = x.astype(np.float64)
                s, sq = x64.sum((0, 2, 3)), (x64 * x64).sum((0, 2, 3))
                tm["stats"] = np.concatenate([s, sq, np.zeros(C), np.zeros(C)])
            else:
                tm.update(rm=(mean * 0.3 + 0.2).astype(np.float32), rv=var.astype(np.float32))
        if dts[i] == "accum":
            tm["old"] = rng.normal(0.0, 1.0, x.shape).astype(np.float32)
        terms.append(tm)
    case = {"form": form, "act": act, "H": H, "W": W, "C": C, "terms": terms,
            "slope": rng.uniform(0.05, 0.4, C).astype(np.float32),
            "dout": rng.normal(0.0, 1.0, (N, C, H, W)).astype(np.float32)}
    if act != "none":
        # keep the activation's argument away from 0: nudge term 0's raw value (always a
        # full-resolution BatchNorm term) where the sum comes close. The statistics block
        # is an input of its own and stays as it is.
        _, scale, _ = seg_mean_scale(terms[0])
        for _ in range(20):
            pre = tail_pre64(case)
            bad = np.abs(pre) < GEN_MARGIN
            if not bad.any():
                break
            step = (4 * GEN_MARGIN / scale)[None, :, None, None] * np.where(pre >= 0, 1.0, -1.0)
            terms[0]["x"] = np.where(bad, terms[0]["x"].astype(np.float64) + step,
                                     terms[0]["x"]).astype(np.float32)
        else:
            raise AssertionError("could not move the tail's sum away from 0")
    for tm in terms:
        tm["x"].setflags(write=False)
    return case


def _up2(a):
    return a.repeat(2, axis=2).repeat(2, axis=3)


def term_value64(tm):
    x = tm["x"].astype(np.float64)
    if tm["kind"] != "plain":
        mu, scale, b = seg_mean_scale(tm)
        bc = lambda a: a[None, :, None, None]
        x = _act64((x - bc(mu)) * bc(scale) + bc(b), tm.get("act", "none"), None)
    return _up2(x) if tm["up"] else x


def tail_pre64(case):
    return sum(term_value64(tm) for tm in case["terms"])


def tail_ref(case):
    """fp64: out, g = dL/d(sum), per term dterm (PLAIN, with its old value when it
    accumulates) or (gsum, gxsum) (BatchNorm, centred on the term's own mean), slope_grad."""
    pre = tail_pre64(case)
    sl = case["slope"].astype(np.float64)[None, :, None, None]
    d = case["dout"].astype(np.float64)
    act = case["act"]
    if act == "prelu":
        out, g = np.where(pre > 0, pre, pre * sl), np.where(pre > 0, d, d * sl)
    elif act == "relu":
        out, g = np.maximum(pre, 0.0), np.where(pre > 0, d, 0.0)
    else:
        out, g = pre, d
    ref = {"pre": pre, "out": out, "g": g, "dterm": [], "gsum": [], "gxsum": [],
           "slope_grad": np.where(pre > 0, 0.0, pre * d).sum((0, 2, 3))}
    for tm in case["terms"]:
        if tm["kind"] == "plain":
            dt = g
            if tm["up"]:
                n, c, h, w = g.shape
                dt = g.reshape(n, c, h // 2, 2, w // 2, 2).sum((3, 5))
            if tm["dterm"] == "accum":
                dt = dt + tm["old"].astype(np.float64)
            ref["dterm"].append(dt)
            ref["gsum"].append(None)
            ref["gxsum"].append(None)
        else:
            mu, _, _ = seg_mean_scale(tm)
            ref["dterm"].append(None)
            ref["gsum"].append(g.sum((0, 2, 3)))
            ref["gxsum"].append((g * (tm["x"].astype(np.float64) - mu[None, :, None, None])).sum((0, 2, 3)))
    return ref


# ---- sigmoid + BCE -------------------------------------------------------------------------
BCE_VEC_N = [4, 8188, 8192, 8196, 3 * 8192 + 148]
BCE_SCALAR_N = [8193, 262144 + 3]
BCE_PLANTED = [18.0, -18.0, 30.0, -30.0, 88.0, -88.0, 120.0, -120.0, np.inf, -np.inf]
BCE_PLANT_T = [0.0, 1.0, 0.3]


@functools.lru_cache(maxsize=None)
def bce_inputs(n):
    """(logits, target, planted mask), fp32. Every planted logit with every planted target
    when n >= 30 (else the first n pairs), spread from the first element to the last: the
    last quad and the last workgroup hold some."""
    rng = np.random.default_rng(4242 + n)
    x = np.clip(rng.normal(0.0, 3.0, n), -12.0, 12.0).astype(np.float32)
    kind = rng.integers(0, 3, n)
    t = np.where(kind == 0, rng.integers(0, 2, n).astype(np.float64),
                 np.where(kind == 1, rng.integers(0, 256, n) / 255.0, rng.uniform(0.0, 1.0, n)))
    t = t.astype(np.float32)
    pairs = [(v, tt) for v in BCE_PLANTED for tt in BCE_PLANT_T][:n]
    pos = np.unique(np.linspace(0, n - 1, len(pairs)).round().astype(np.int64))
    assert len(pos) == len(pairs)
    planted = np.zeros(n, bool)
    for p, (v, tt) in zip(pos, pairs):
        x[p], t[p], planted[p] = v, tt, True
    for a in (x, t, planted):
        a.setflags(write=False)
    return x, t, planted


def bce_ref(x, t, grad_scale):
    """torch CPU fp32 sigmoid -> binary_cross_entropy(reduction="none") with autograd:
    (fp64 sum of the per-element fp32 losses, dlogits fp32 for an upstream gradient of
    grad_scale per element)."""
    lt = torch.from_numpy(np.array(x)).requires_grad_(True)
    l = F.binary_cross_entropy(torch.sigmoid(lt), torch.from_numpy(np.array(t)), reduction="none")
    l.backward(torch.full_like(l, float(np.float32(grad_scale))))
    return float(l.detach().double().sum()), lt.grad.numpy()


# ---- sigmoid -------------------------------------------------------------------------------
SIGMOID_N = [1, 255, 256, 257, 2048 * 256 + 5]
SIGMOID_PLANTED = [120.0, -120.0, np.inf, -np.inf]


@functools.lru_cache(maxsize=None)
def sigmoid_inputs(n):
    """(x uniform in [-80, 80] with the planted values at the end when n > 4, planted mask)."""
    rng = np.random.default_rng(99 + n)
    x = rng.uniform(-80.0, 80.0, n).astype(np.float32)
    planted = np.zeros(n, bool)
    if n > 4:
        x[-4:] = SIGMOID_PLANTED
        planted[-4:] = True
    x.setflags(write=False)
    return x, planted


def sigmoid_ref64(x):
    x = x.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.where(x >= 0, 1.0 / (1.0 + np.exp(-x)), np.exp(x) / (1.0 + np.exp(x)))


def sigmoid_bwd_inputs(n):
    rng = np.random.default_rng(177 + n)
    y = rng.uniform(0.0, 1.0, n).astype(np.float32)
    dy = rng.normal(0.0, 1.0, n).astype(np.float32)
    if n > 4:
        y[:2] = 0.0, 1.0
    return y, dy


# ---- Adam ----------------------------------------------------------------------------------
ADAM_N = [1, 257, 2048 * 256 + 3]
ADAM_WD = 1e-2
# With L2 weight decay the gradient Adam sees is ge = g + wd*p, a sum that can cancel; fp32
# rounds it with an error up to d = 2^-23 (|g| + wd |p|), about 5e-9 here. At step 1 from a
# zero state the update is -lr * ge / (|ge| + eps), whose slope in ge is lr*eps / (|ge| + eps)^2:
# for the rounding to move the parameter by less than the bar's 1e-9 floor |ge| must exceed
# sqrt(lr*eps*d / 1e-9) = 7e-6. The inputs keep |ge| (and |g|) sixteen times that away from 0.
ADAM_MIN_GE = 1e-4


def adam_inputs(n, step, masked):
    """(param, grad, exp_avg, exp_avg_sq, live or None): optimizer state zero before step 1,
    otherwise that of a run in progress."""
    rng = np.random.default_rng(31 * n + step + (5 if masked else 0))
    p = rng.normal(0.0, 1.0, n).astype(np.float32)
    g = (rng.normal(0.0, 1.0, n) * 1e-2).astype(np.float32)
    for _ in range(8):  # always upwards: a value leaves each of the two windows for good
        bad = (np.abs(g) < 2 * ADAM_MIN_GE) | \
            (np.abs(g.astype(np.float64) + ADAM_WD * p.astype(np.float64)) < 2 * ADAM_MIN_GE)
        if not bad.any():
            break
        g = np.where(bad, g + np.float32(4 * ADAM_MIN_GE), g).astype(np.float32)
    if step == 1:
        m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    else:
        m = (rng.normal(0.0, 1.0, n) * 1e-2).astype(np.float32)
        v = (rng.uniform(0.1, 2.0, n) * 1e-4).astype(np.float32)
    live = None
    if masked:  # 10 % of the elements are skipped
        live = (rng.uniform(size=n) >= 0.1).astype(np.uint8)
        if n > 4:
            live[0], live[-1] = 0, 0
    return p, g, m, v, live
