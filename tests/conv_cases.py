"""What tests/test_gpu_conv_forms.py feeds the conv launchers (pw_gemm, tap_conv, down_conv,
thin_conv, halo_conv, conv_mfma, wgrad, tap_wgrad, dw_convt) and the fp64 expectations it
compares them with. numpy and torch on the CPU only: tests/test_conv_cases_cpu.py proves,
without a GPU, that the references agree with torch autograd and that no activation boundary
of a case is close to a tie.

ROWS is the kernel table: one row per (kernel, direction) at the smallest geometry the
launcher's host predicates still accept, with the launch name (isg_last_launch) the row must
reach. A case is a row in one operand form (FORMS): what changes is how the operands are
presented (segments, sinks, BatchNorm state), never the arithmetic.

Every input is an fp32 array; a reference widens it to fp64 (exactly) and evaluates the
documented formula there (include/isg.h)."""
import functools
from typing import NamedTuple

import numpy as np
import torch
import torch.nn.functional as F

from tests.eltwise_cases import EPS, coef_block, stats_block

GEN_MARGIN = 4e-3   # distance the generators keep between an activation's argument and 0
TIE_MARGIN = 1e-4   # what must survive, relative to max |z| (asserted on the CPU)
SIZE_CAP = 1 << 20  # N * max(Ci, Co) * H * W of a row


class Row(NamedTuple):
    id: str
    dirn: str            # "fwd", "dgrad", "wgrad" or "dwbwd" (isg_depthwise_bwd)
    Ci: int
    Co: int
    H: int
    W: int
    k: tuple             # (KH, KW)
    s: int
    p: tuple             # (PH, PW)
    d: int
    launch: str          # isg_last_launch of the base / slice / replicas / coef / n1 forms
    off4: tuple          # launch names allowed to take the off4 form
    multi: object = None  # sinks3 / segs3: names allowed (None: `launch`), or an error code
    groups: int = 1
    tol: float = 2e-5
    dbias: bool = True
    note: str = ""

    @property
    def OH(self):
        return (self.H + 2 * self.p[0] - self.d * (self.k[0] - 1) - 1) // self.s + 1

    @property
    def OW(self):
        return (self.W + 2 * self.p[1] - self.d * (self.k[1] - 1) - 1) // self.s + 1


def _r(id, dirn, Ci, Co, H, W, k, s, p, d, launch, off4=None, **kw):
    k = k if isinstance(k, tuple) else (k, k)
    p = p if isinstance(p, tuple) else (p, p)
    return Row(id, dirn, Ci, Co, H, W, k, s, p, d, launch, off4 or (launch,), **kw)


UNSUPPORTED = -2
PW, PWX, THINPW = "pw_kernel", "pwx_kernel", "thin_pw_kernel"
TAP, GEMM, HALO = "tap_conv_kernel", "gemm_conv_kernel", "halo_conv_kernel"
TAPW, WG = "tap_wgrad_kernel", "wgrad_kernel"

# The geometries start from the attributions in tests/test_gpu_kernels.py DENSE / DW_CFG, shrunk
# as far as each launcher's predicates allow. Where a row differs in kind, `note` says why.
ROWS = [
    # ---- forward ---------------------------------------------------------------------------
    _r("fwd-pw", "fwd", 80, 72, 6, 6, 1, 1, 0, 1, PW,
       note="no DENSE shape reaches pw_kernel (all are slab shapes): M > 64 with K > 64"),
    _r("fwd-pwx", "fwd", 48, 16, 6, 10, 1, 1, 0, 1, PWX, (PW,)),
    _r("fwd-thin_pw", "fwd", 4, 16, 6, 10, 1, 1, 0, 1, THINPW, (PW,)),
    _r("fwd-thin_conv", "fwd", 4, 4, 7, 10, 3, 1, 1, 1, "thin_conv_kernel"),
    _r("fwd-thin_conv3_x4", "fwd", 4, 1, 6, 8, 3, 1, 1, 1, "thin_conv3_x4_kernel", ("thin_conv_kernel",)),
    _r("fwd-down_conv", "fwd", 4, 16, 16, 24, 8, 4, 2, 1, "down_conv_kernel", (HALO,)),
    _r("fwd-s2k5", "fwd", 12, 8, 20, 72, 5, 2, 2, 1, "s2k5_fwd_kernel", (TAP,), tol=4e-6,
       note="DENSE calls s2k5_fwd opt-in; the chain tries it before tap_conv unconditionally"),
    _r("fwd-tap_s1", "fwd", 16, 20, 9, 13, 3, 1, 1, 1, TAP),
    _r("fwd-tap_s2", "fwd", 36, 16, 10, 12, 2, 2, 0, 1, TAP),
    _r("fwd-halo", "fwd", 16, 4, 24, 40, 8, 4, 2, 1, HALO, multi=(GEMM,),
       note="DENSE lists 16->4 k8 s4 under tap_conv; stride 4 is not tap_conv's (mx > 2)"),
    _r("fwd-gemm", "fwd", 8, 52, 7, 9, 3, 1, 1, 1, GEMM,
       note="more than 48 output channels: neither tap_conv nor halo_conv"),
    _r("fwd-dw_tile", "fwd", 8, 8, 10, 12, 3, 1, 1, 1, "dw_tile_kernel<fwd>", ("dw_kernel<fwd>",),
       multi=UNSUPPORTED, groups=8),
    _r("fwd-dw", "fwd", 8, 8, 9, 10, 3, 1, 2, 2, "dw_kernel<fwd>", multi=UNSUPPORTED, groups=8),
    # ---- input gradient --------------------------------------------------------------------
    _r("dgrad-pw", "dgrad", 80, 72, 6, 6, 1, 1, 0, 1, PW),
    _r("dgrad-pwx", "dgrad", 48, 16, 6, 10, 1, 1, 0, 1, PWX, (PW,)),
    _r("dgrad-thin_pw", "dgrad", 4, 16, 6, 10, 1, 1, 0, 1, THINPW, (PW,)),
    _r("dgrad-thin_conv", "dgrad", 4, 4, 7, 10, 3, 1, 1, 1, "thin_conv_kernel"),
    _r("dgrad-sub2", "dgrad", 8, 12, 12, 136, 5, 2, 2, 1, "sub2_dgrad_kernel", (TAP,),
       note="only the LDS-staged form launches under this name; the plain one is tap_conv's"),
    _r("dgrad-tap", "dgrad", 16, 20, 9, 13, 3, 1, 1, 1, TAP),
    _r("dgrad-gemm", "dgrad", 16, 4, 24, 40, 8, 4, 2, 1, GEMM),
    _r("dgrad-dw_tile", "dgrad", 8, 8, 10, 12, 3, 1, 1, 1, "dw_tile_kernel<dgrad>", ("dw_kernel<dgrad>",),
       multi=UNSUPPORTED, groups=8),
    # ---- weight gradient -------------------------------------------------------------------
    _r("wgrad-pwg", "wgrad", 48, 16, 6, 10, 1, 1, 0, 1, "pwg_kernel", (WG,)),
    _r("wgrad-wgrad", "wgrad", 8, 20, 7, 9, 3, 1, 1, 1, WG),
    _r("wgrad-tap", "wgrad", 16, 16, 9, 13, 3, 1, 1, 1, TAPW),
    _r("wgrad-tap_all", "wgrad", 20, 16, 16, 24, 5, 2, 2, 1, "tap_wgrad_all_kernel"),
    _r("wgrad-thin3_x4", "wgrad", 4, 1, 6, 8, 3, 1, 1, 1, "thin_wgrad3_x4_kernel", (TAPW, WG),
       multi=(TAPW, WG)),
    _r("wgrad-down", "wgrad", 4, 16, 16, 24, 8, 4, 2, 1, "down_wgrad_kernel", dbias=False,
       note="down_wgrad takes no bias gradient"),
    _r("wgrad-s2k5", "wgrad", 12, 8, 20, 72, 5, 2, 2, 1, "s2k5_wgrad_kernel", (TAPW,), tol=4e-6),
    _r("wgrad-dw_tile", "wgrad", 8, 8, 10, 12, 3, 1, 1, 1, "dw_wgrad_tile_kernel", ("dw_wgrad_kernel",),
       multi=UNSUPPORTED, groups=8),
    _r("wgrad-dw", "wgrad", 8, 8, 9, 10, 3, 1, 1, 1, "dw_wgrad_kernel", multi=UNSUPPORTED, groups=8),
    _r("dwbwd-fused", "dwbwd", 8, 8, 10, 12, 3, 1, 1, 1, "dw_bwd_tile_kernel", ("dw_wgrad_kernel",),
       multi=UNSUPPORTED, groups=8),
]
ROW = {r.id: r for r in ROWS}

FORMS = {"fwd": ("base", "slice", "off4", "replicas", "coef", "sinks3", "n1"),
         "dgrad": ("base", "slice", "off4", "replicas", "coef", "sinks3", "n1"),
         "wgrad": ("base", "slice", "off4", "replicas", "coef", "segs3", "n1"),
         "dwbwd": ("base", "slice", "off4", "replicas", "coef", "segs3", "n1")}
CASES = [(r.id, f) for r in ROWS for f in FORMS[r.dirn]]


def expected_launch(row, form):
    """The launch names allowed for (row, form), or the error code the form is refused with."""
    if form == "off4":
        return row.off4
    if form in ("sinks3", "segs3") and row.multi is not None:
        return row.multi
    return (row.launch,)


# ---- splitting channels -------------------------------------------------------------------
def split_sinks(C):
    """Up to three uneven parts whose boundaries are no multiple of 4: 1 / ... / 3 or so."""
    if C == 1:
        return [1]
    if C == 2:
        return [1, 1]
    b2 = next(b for b in (C - 3, C - 2, C - 1) if b > 1 and b % 4)
    return [1, b2 - 1, C - b2]


def split_segs(C):
    """Up to three segments of unequal width where C allows: 2 / ... / 3 or so."""
    if C < 5:
        return split_sinks(C)
    b2 = next(b for b in (C - 3, C - 2, C - 1) if b > 2 and b % 4)
    return [2, b2 - 2, C - b2]


# ---- segments -----------------------------------------------------------------------------
def _act64(z, act, slope):
    if act == "relu":
        return np.maximum(z, 0.0)
    if act == "prelu":
        return np.where(z > 0, z, z * slope[None, :, None, None])
    return z


def _bn_state(rng, C, bnC, bn, M):
    """A BatchNorm layer of bnC >= C channels in form `bn`: parameters as fp32, (mean, rstd)
    of its first C channels in fp64 as that form defines them."""
    st = {"bn": bn, "bnC": bnC, "count": float(M),
          "gamma": (rng.uniform(0.5, 1.5, bnC) * rng.choice([-1.0, 1.0], bnC)).astype(np.float32),
          "beta": rng.uniform(-0.5, 0.5, bnC).astype(np.float32),
          "slope": rng.uniform(0.05, 0.4, bnC).astype(np.float32)}
    mean, var = rng.uniform(-1.0, 1.0, bnC), rng.uniform(0.5, 2.0, bnC)
    if bn == "eval":
        st["rm"], st["rv"] = mean.astype(np.float32), var.astype(np.float32)
        mean = st["rm"].astype(np.float64)
        rstd = 1.0 / np.sqrt(st["rv"].astype(np.float64) + EPS)
    else:  # "train", "coef": the statistics block [sum | sumsq | gsum | gxsum]
        st["stats"] = stats_block(mean, var, M)
        mean = st["stats"][:bnC] / M
        rstd = 1.0 / np.sqrt(np.maximum(st["stats"][bnC:2 * bnC] / M - mean * mean, 0.0) + EPS)
    st["mean"], st["rstd"] = mean, rstd
    return st


def _fwd_coefs(st):
    """(mean, gamma*rstd, beta) of the layer's channels as the reference applies them: fp64,
    or for the coef form the fp32 values isg_bn_finalize stores (rounded once from fp64)."""
    if st["bn"] == "coef":
        blk = coef_block({"kind": "coef", "gamma": st["gamma"], "beta": st["beta"],
                          "stats": st["stats"], "C": st["bnC"], "count": st["count"]})
        st["coef_fwd"] = blk
        return tuple(blk[:, i].astype(np.float64) for i in range(3))
    return st["mean"], st["gamma"].astype(np.float64) * st["rstd"], st["beta"].astype(np.float64)


def _raw_for(rng, shape, mean, scale, beta):
    """fp32 raw values whose BatchNorm output keeps GEN_MARGIN from 0, and that output."""
    z = rng.normal(0.0, 1.0, shape)
    z = np.where(np.abs(z) < GEN_MARGIN, 0.5, z)
    b = lambda a: a[None, :, None, None]
    x = ((z - b(beta)) / b(scale) + b(mean)).astype(np.float32)
    return x, (x.astype(np.float64) - b(mean)) * b(scale) + b(beta)


def make_seg(rng, N, C, H, W, xf, act="none", bn="eval", bnC=None):
    """One channel segment: its raw operands, its BatchNorm state and its fp64 value `v`."""
    sg = {"C": C, "xf": xf, "act": act}
    if xf == "plain":
        sg["p"] = rng.normal(0.0, 1.0, (N, C, H, W)).astype(np.float32)
        sg["v"] = sg["p"].astype(np.float64)
        return sg
    bnC = bnC or C
    st = _bn_state(rng, C, bnC, bn, N * H * W)
    if xf == "bn_fwd":
        mean, scale, beta = (a[:C] for a in _fwd_coefs(st))
        sg.update(st)
        sg["p"], z = _raw_for(rng, (N, C, H, W), mean, scale, beta)
        sg["z"] = z
        sg["v"] = _act64(z, act, st["slope"][:C].astype(np.float64))
        return sg
    # bn_bwd: p = the gradient w.r.t. the BatchNorm output, y = the saved raw output;
    # dy = A*g + B*(y - mean) + C (common.h bwd_coef_of), gsum / gxsum of some earlier consumer
    assert bn in ("train", "coef")
    M = float(N * H * W)
    st["stats"][2 * bnC:3 * bnC] = rng.normal(0.0, np.sqrt(M), bnC)
    st["stats"][3 * bnC:] = rng.normal(0.0, np.sqrt(M), bnC)
    gam, rstd, mean = st["gamma"].astype(np.float64), st["rstd"], st["mean"]
    A = gam * rstd
    B = -gam * rstd * rstd * (rstd * st["stats"][3 * bnC:] / M)
    Cc = -gam * rstd * (st["stats"][2 * bnC:3 * bnC] / M)
    if bn == "coef":
        _fwd_coefs(st)
        blk = np.stack([A, B, mean, Cc], 1).astype(np.float32)
        st["coef_bwd"] = blk
        A, B, mean, Cc = (blk[:, i].astype(np.float64) for i in range(4))
    sg.update(st)
    sg["p"] = rng.normal(0.0, 1.0, (N, C, H, W)).astype(np.float32)
    sg["y"] = (rng.normal(0.0, 1.0, (N, C, H, W)) + 0.3).astype(np.float32)
    b = lambda a: a[None, :C, None, None]
    sg["v"] = b(A) * sg["p"].astype(np.float64) + b(B) * (sg["y"].astype(np.float64) - b(mean)) + b(Cc)
    return sg


def coef_of(sg):
    """The 8*bnC fp32 block of isg_bn.coef: the forward [bnC][4], then the backward [bnC][4]."""
    bnC = sg["bnC"]
    bwd = sg.get("coef_bwd", np.full((bnC, 4), np.nan, np.float32))
    return np.concatenate([sg["coef_fwd"].reshape(-1), bwd.reshape(-1)])


# ---- sinks --------------------------------------------------------------------------------
def make_sink(rng, N, c0, C, H, W, mode, v, bn="eval", act="prelu", bnC=None, bias=True):
    """A sink of rows [c0, c0 + C) receiving v (fp64 [N, C, H, W]) and what it must hold after."""
    sk = {"c0": c0, "C": C, "mode": mode}
    if mode == "store":
        sk["bias"] = rng.normal(0.0, 0.1, C).astype(np.float32) if bias else None
        out = v + (sk["bias"].astype(np.float64)[None, :, None, None] if bias else 0.0)
        sk.update(out=out, sum=out.sum((0, 2, 3)), sumsq=(out * out).sum((0, 2, 3)))
    elif mode == "accum":
        sk["old"] = rng.normal(0.0, 1.0, (N, C, H, W)).astype(np.float32)
        sk["out"] = sk["old"].astype(np.float64) + v
    elif mode == "actbwd":
        bnC = bnC or C
        st = _bn_state(rng, C, bnC, bn, N * H * W)
        mean, scale, beta = (a[:C] for a in _fwd_coefs(st))
        sk.update(st)
        sk["act"] = act
        sk["y"], z = _raw_for(rng, (N, C, H, W), mean, scale, beta)
        sl = st["slope"][:C].astype(np.float64)[None, :, None, None]
        g = {"prelu": np.where(z > 0, v, v * sl), "relu": np.where(z > 0, v, 0.0), "none": v}[act]
        yc = sk["y"].astype(np.float64) - mean[None, :, None, None]
        sk.update(z=z, out=g, gsum=g.sum((0, 2, 3)), gxsum=(g * yc).sum((0, 2, 3)),
                  slope_grad=np.where(z > 0, 0.0, z * v).sum((0, 2, 3)))
    return sk


# ---- references -----------------------------------------------------------------------------
def _conv_kw(row):
    return dict(stride=row.s, padding=row.p, dilation=row.d, groups=row.groups)


def wshape(row):
    return (row.Co, row.Ci // row.groups, row.k[0], row.k[1])


def cat_v(segs):
    return torch.from_numpy(np.concatenate([s["v"] for s in segs], 1))


def ref_fwd(row, x, w):
    return F.conv2d(x, w, None, **_conv_kw(row))


def ref_dgrad(row, N, dy, w):
    return torch.nn.grad.conv2d_input((N, row.Ci, row.H, row.W), w, dy, **_conv_kw(row))


def ref_wgrad(row, x, dy):
    return torch.nn.grad.conv2d_weight(x, wshape(row), dy, **_conv_kw(row))


def _seed(row, form):
    return 7919 * ROWS.index(row) + 101 * sorted({f for fs in FORMS.values() for f in fs}).index(form) + 5


def _src_segs(rng, row, form, N, C, H, W, side):
    """The gathered operand (forward: x, input gradient: dy; weight gradient: both) in `form`."""
    bn = {"replicas": "train", "coef": "coef"}.get(form, "eval")
    wide = 3 if form == "coef" else 0  # a layer wider than the segment that reads it
    multi = form in ("sinks3", "segs3")
    if side == "x":
        if multi:
            a, b, c = (split_segs(C) + [0, 0])[:3]
            segs = [make_seg(rng, N, a, H, W, "plain")]
            if b:
                segs.append(make_seg(rng, N, b, H, W, "bn_fwd", "prelu", "train"))
            if c:
                segs.append(make_seg(rng, N, c, H, W, "bn_fwd", "relu", "eval"))
            return segs
        if row.groups > 1 or row.dirn != "fwd":
            return [make_seg(rng, N, C, H, W, "bn_fwd", "prelu", bn, C + wide)]
        c1 = C // 2 if C > 1 else C  # as test_conv_fwd_dense: BatchNorm + PReLU | plain
        segs = [make_seg(rng, N, c1, H, W, "bn_fwd", "prelu", bn, c1 + wide)]
        if C - c1:
            segs.append(make_seg(rng, N, C - c1, H, W, "plain"))
        return segs
    bnb = "coef" if form == "coef" else "train"
    if multi and row.dirn == "dgrad":
        a, b, c = (split_segs(C) + [0, 0])[:3]
        segs = [make_seg(rng, N, a, H, W, "bn_bwd", bn="train")]
        if b:
            segs.append(make_seg(rng, N, b, H, W, "plain"))
        if c:
            segs.append(make_seg(rng, N, c, H, W, "bn_fwd", "relu", "eval"))
        return segs
    if multi and C > 1:  # the weight gradient's dy in two segments
        a = split_sinks(C)[0] if C < 4 else C - 3
        return [make_seg(rng, N, a, H, W, "bn_bwd", bn="train"), make_seg(rng, N, C - a, H, W, "plain")]
    return [make_seg(rng, N, C, H, W, "bn_bwd", bn=bnb, bnC=C + wide)]


@functools.lru_cache(maxsize=None)
def make_case(rid, form):
    """Inputs and fp64 expectations of row `rid` in operand form `form` — read-only."""
    row = ROW[rid]
    rng = np.random.default_rng(_seed(row, form))
    N = 1 if form == "n1" else 3
    OH, OW = row.OH, row.OW
    bn = {"replicas": "train", "coef": "coef"}.get(form, "eval")
    # (an ACTBWD sink's BatchNorm has the sink's own channels: isg.h isg_sink, bn.C == C)
    fan = (row.Ci // row.groups) * row.k[0] * row.k[1]
    w = (rng.normal(0.0, 1.0, wshape(row)) * (2.0 / fan) ** 0.5).astype(np.float32)
    case = {"row": row, "form": form, "N": N, "w": w}
    w64 = torch.from_numpy(w.astype(np.float64))
    if row.dirn in ("fwd", "dgrad"):
        fwd = row.dirn == "fwd"
        sC, sH, sW = (row.Ci, row.H, row.W) if fwd else (row.Co, OH, OW)
        oC, oH, oW = (row.Co, OH, OW) if fwd else (row.Ci, row.H, row.W)
        case["src"] = _src_segs(rng, row, form, N, sC, sH, sW, "x" if fwd else "dy")
        v = (ref_fwd(row, cat_v(case["src"]), w64) if fwd else ref_dgrad(row, N, cat_v(case["src"]), w64)).numpy()
        case["v"] = v
        last = "store" if fwd else "actbwd"
        if form == "sinks3":  # also what a one-sink launcher is asked and refuses
            parts = split_sinks(oC)
            modes = (["none", "accum", last])[-len(parts):]
        else:
            parts, modes = [oC], [last]
        case["sinks"], c0 = [], 0
        for C, mode in zip(parts, modes):
            case["sinks"].append(make_sink(rng, N, c0, C, oH, oW, mode, v[:, c0:c0 + C],
                                           bn="train" if form == "sinks3" else bn))
            c0 += C
    else:
        case["x"] = _src_segs(rng, row, form, N, row.Ci, row.H, row.W, "x")
        case["dy"] = _src_segs(rng, row, form, N, row.Co, OH, OW, "dy")
        x, dy = cat_v(case["x"]), cat_v(case["dy"])
        case["dw"] = ref_wgrad(row, x, dy).numpy()
        case["dbias"] = dy.sum((0, 2, 3)).numpy()
        if row.dirn == "dwbwd":
            v = ref_dgrad(row, N, dy, w64).numpy()
            case["v"] = v
            case["sinks"] = [make_sink(rng, N, 0, row.Ci, row.H, row.W, "actbwd", v, bn=bn)]
    return case


def ties(case):
    """(what, z) of every activation boundary the GPU evaluates in this case."""
    out = []
    for key in ("src", "x", "dy"):
        for i, sg in enumerate(case.get(key, [])):
            if sg["xf"] == "bn_fwd" and sg["act"] != "none":
                out.append((f"{key}[{i}]", sg["z"]))
    for i, sk in enumerate(case.get("sinks", [])):
        if sk["mode"] == "actbwd" and sk["act"] != "none":
            out.append((f"sink[{i}]", sk["z"]))
    return out
