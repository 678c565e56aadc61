"""What tests/test_gpu_mask_head.py feeds the fused mask head (isg_mask_head_fwd / _bwd / _fold,
csrc/mask_head.hip) and the fp64 expectations it compares them with. numpy and torch on the CPU
only: tests/test_head_cases_cpu.py proves, without a GPU, that the references agree with torch
autograd through the two unfused layers, that the loop shapes loop, and that the border
patterns put the 3x3 weight gradient's ring term where it cannot hide.

A case is a shape (SHAPES) with a dlogits pattern (PATTERNS) in an operand form (FORMS). What a
form changes is how the operands are presented; the data, and so the arithmetic, changes only
with the form's data kind (KIND): the forms of kind "plain" share one set of inputs, which is
what lets the GPU test ask them for the same bits.

Every input is an fp32 array; a reference widens it to fp64 (exactly) and evaluates the
documented formula there (include/isg.h)."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from tests.eltwise_cases import _bn_params, coef_block, seg_mean_scale, seg_pre64, stats_block

CI, CM = 16, 4       # convT input / intermediate channels
TY, TX = 32, 64      # the kernels' logit tile (mask_head.hip)
MAX_GROUPS = 256     # head_bwd_blocks: at most 256 two-tile workgroups

# id -> (N, Hi, Wi)
SHAPES = {
    "one_tile": (1, 5, 7),            # one partial tile, scalar path, half 1 never active
    "vec_partial": (2, 20, 44),       # Wi % 4 == 0; 80 x 176 ends inside a tile on both axes; 3 x 3 tiles
    "ragged": (2, 17, 33),
    "loop_even": (58, 24, 48),        # 522 tiles on 256 workgroups: workgroups 0-4 loop, both halves
    "loop_odd": (57, 24, 48),         # 513 tiles: workgroup 0's half 0 takes tile 512, its half 1 idles
    "loop_odd_scalar": (57, 23, 45),  # 513 tiles, partial tiles, Wi % 4 != 0
}
SMALL = ("one_tile", "vec_partial", "ragged")
LOOP = ("loop_even", "loop_odd", "loop_odd_scalar")
PATTERNS = ("dense", "border", "corners", "ones")

# form -> data kind
KIND = {"base": "plain", "slice": "plain", "off4": "plain", "replicas": "plain", "skip": "plain",
        "nobias": "nobias", "segs3": "segs3", "coef": "coef", "act_only": "act_only"}
FORMS = tuple(KIND)
SEGS3 = (("plain", "none", 5), ("bn_train", "prelu", 7), ("bn_eval", "relu", 4))
SINKS3 = (("none", 6), ("accum", 6), ("store", 4))  # does not split where the segments do
COEF_BNC = 19  # the coef form's layer is wider than the 16 channels the head reads

R_DW1, R_DB1, R_DW2, R_DB2 = 0, 4096, 4100, 4136  # offsets within one weight-gradient replica
R_LEN = 4137


def tiles(shape_id):
    """(tiles, workgroups) of the backward by the kernel's own formulas (head_bwd_blocks)."""
    N, Hi, Wi = SHAPES[shape_id]
    nt = -(-4 * Wi // TX) * -(-4 * Hi // TY) * N
    return nt, min((nt + 1) // 2, MAX_GROUPS)


def gpu_cases():
    """(shape, pattern, form) of every GPU comparison."""
    out = []
    for s in SMALL:
        for f in FORMS:
            if f == "off4" and SHAPES[s][2] % 4:
                continue  # off4 is about reaching the scalar kernel from a Wi % 4 == 0 shape
            out.append((s, "dense", f))
        for p in ("border", "corners"):
            out += [(s, p, f) for f in ("base", "segs3", "coef")]
    for s in LOOP:
        out += [(s, "dense", f) for f in ("base", "segs3", "coef")]
    out.append(("loop_odd", "ones", "base"))
    return out


def _seed(shape_id, pattern, kind):
    kinds = sorted(set(KIND.values()))
    return 10007 * list(SHAPES).index(shape_id) + 101 * PATTERNS.index(pattern) + 7 * kinds.index(kind) + 3


def _away(rng, C):
    """Per-channel beta with |beta| in [0.5, 1]: transform(0) != 0, so padding with the
    transform of zero instead of zero is wrong by an O(1) amount at every image edge."""
    return (rng.uniform(0.5, 1.0, C) * rng.choice([-1.0, 1.0], C)).astype(np.float32)


def _segment(rng, kind, act, C, c0, N, Hi, Wi):
    M = float(N * Hi * Wi)
    sg = {"kind": kind, "act": act, "C": C, "c0": c0, "count": M}
    z = rng.normal(0.0, 1.0, (N, C, Hi, Wi))
    if kind == "plain":
        sg["x"] = z.astype(np.float32)
        return sg
    bnC = COEF_BNC if kind == "coef" else C
    gamma, _, slope, mean, var = _bn_params(rng, bnC)
    sg["slope"] = slope[:C].copy()
    if kind == "act_only":
        sg["x"] = z.astype(np.float32)
        return sg
    beta = _away(rng, bnC)
    lay = {"kind": kind, "C": bnC, "count": M, "gamma": gamma, "beta": beta}
    if kind == "bn_eval":
        lay.update(rm=mean.astype(np.float32), rv=var.astype(np.float32))
    else:
        lay["stats"] = stats_block(mean, var, M)
    mu, scale, b = (a[:C] for a in seg_mean_scale(lay))
    if kind == "coef":  # the reference applies the fp32 values the layer's finalisation stored
        blk = coef_block(lay)
        sg["coef"] = np.concatenate([blk.reshape(-1), np.full(4 * bnC, np.nan, np.float32)])
        mu, scale, b = (blk[:C, i].astype(np.float64) for i in range(3))
    sg.update({k: v for k, v in lay.items() if k not in ("kind", "C")}, bnC=bnC)
    bc = lambda a: a[None, :, None, None]
    sg["x"] = ((z - bc(b)) / bc(scale) + bc(mu)).astype(np.float32)
    return sg


def seg_value64(sg):
    """isg.h isg_vseg in fp64: PLAIN v = p; BN_FWD v = act((p - mean) * gamma*rstd + beta)."""
    C = sg["C"]
    if sg["kind"] == "coef":
        c = sg["coef"][:4 * sg["bnC"]].reshape(-1, 4)[:C].astype(np.float64)
        bc = lambda a: a[None, :, None, None]
        pre = (sg["x"].astype(np.float64) - bc(c[:, 0])) * bc(c[:, 1]) + bc(c[:, 2])
    elif sg["kind"] in ("bn_train", "bn_eval"):
        lay = dict(sg, C=sg["bnC"])
        mu, scale, b = (a[:C] for a in seg_mean_scale(lay))
        bc = lambda a: a[None, :, None, None]
        pre = (sg["x"].astype(np.float64) - bc(mu)) * bc(scale) + bc(b)
    else:
        pre = seg_pre64(sg)
    if sg["act"] == "relu":
        return np.maximum(pre, 0.0)
    if sg["act"] == "prelu":
        return np.where(pre > 0, pre, pre * sg["slope"].astype(np.float64)[None, :, None, None])
    return pre


def _dlogits(rng, pattern, N, OH, OW):
    d = rng.normal(0.0, 1.0, (N, 1, OH, OW))
    if pattern == "ones":
        return np.ones((N, 1, OH, OW), np.float32)
    keep = np.zeros((OH, OW), bool)
    if pattern == "dense":
        keep[:] = True
    elif pattern == "border":
        keep[0], keep[-1], keep[:, 0], keep[:, -1] = True, True, True, True
    else:  # corners
        keep[0, 0] = keep[0, -1] = keep[-1, 0] = keep[-1, -1] = True
    return np.where(keep, d, 0.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _inputs(shape_id, pattern, kind):
    N, Hi, Wi = SHAPES[shape_id]
    rng = np.random.default_rng(_seed(shape_id, pattern, "plain" if kind == "nobias" else kind))
    spec = {"segs3": SEGS3, "coef": (("coef", "prelu", CI),), "act_only": (("act_only", "prelu", CI),)}.get(
        kind, (("plain", "none", CI),))
    segs, c0 = [], 0
    for k, act, C in spec:
        segs.append(_segment(rng, k, act, C, c0, N, Hi, Wi))
        c0 += C
    case = {"shape": shape_id, "pattern": pattern, "kind": kind, "N": N, "Hi": Hi, "Wi": Wi, "segs": segs,
            "w1": (rng.normal(0.0, 1.0, (CI, CM, 8, 8)) * 0.05).astype(np.float32),
            "w2": (rng.normal(0.0, 1.0, (1, CM, 3, 3)) * 0.3).astype(np.float32),
            "b2": (rng.normal(0.0, 1.0, 1) * 0.1).astype(np.float32)}
    if pattern in ("border", "corners"):  # |b1| ~ 1: b1 * sum(dlogits) matters in dW2
        case["b1"] = (rng.uniform(0.7, 1.3, CM) * rng.choice([-1.0, 1.0], CM)).astype(np.float32)
    else:
        case["b1"] = (rng.normal(0.0, 1.0, CM) * 0.1).astype(np.float32)
    case["dl"] = _dlogits(rng, pattern, N, 4 * Hi, 4 * Wi)
    case["preset"] = rng.normal(0.0, 1.0, (N, SINKS3[1][1], Hi, Wi)).astype(np.float32)
    if kind == "nobias":
        case["b1"] = case["b2"] = None
    for a in [case[k] for k in ("w1", "w2", "b1", "b2", "dl", "preset")] + [s["x"] for s in segs]:
        if a is not None:
            a.setflags(write=False)
    return case


def head_case(shape_id, form, pattern="dense"):
    """fp32 inputs of the case: raw x per segment with the segment descriptions ("segs"), w1,
    b1, w2, b2 (None in the nobias form), dlogits ("dl") and the ACCUM sink's preset values —
    read-only, shared by every form of the same data kind."""
    return _inputs(shape_id, pattern, KIND[form])


def ring_of(full, OH, OW):
    """The one-pixel ring outside the image of the un-cropped intermediate `full` (origin
    (-2, -2)): [N, 4, ISG_HEAD_RING] in isg.h's order — row -1, row OH (columns -1 .. OW), column
    -1, column OW (rows 0 .. OH - 1)."""
    return torch.cat([full[:, :, 1, 1:OW + 3], full[:, :, OH + 2, 1:OW + 3],
                      full[:, :, 2:OH + 2, 1], full[:, :, 2:OH + 2, OW + 2]], 2)


@functools.lru_cache(maxsize=None)
def _reference(shape_id, pattern, kind):
    case = _inputs(shape_id, pattern, kind)
    OH, OW = 4 * case["Hi"], 4 * case["Wi"]
    T = lambda a: None if a is None else torch.from_numpy(a.astype(np.float64))
    v = torch.from_numpy(np.concatenate([seg_value64(s) for s in case["segs"]], 1))
    P = {"v": v.clone(), "w1": T(case["w1"]), "b1": T(case["b1"]), "w2": T(case["w2"]), "b2": T(case["b2"])}
    for t in P.values():
        if t is not None:
            t.requires_grad_(True)
    dl = T(case["dl"])
    inter = F.conv_transpose2d(P["v"], P["w1"], P["b1"], stride=4, padding=2)
    y = F.conv2d(inter, P["w2"], P["b2"], padding=1)
    y.backward(dl)
    full = F.conv_transpose2d(v, P["w1"].detach(), None if P["b1"] is None else P["b1"].detach(), stride=4)
    assert full.shape[2] == OH + 4 and full.shape[3] == OW + 4
    ref = {"v": v, "logits": y.detach(), "ring": ring_of(full, OH, OW), "dx": P["v"].grad, "dw1": P["w1"].grad,
           "dw2": P["w2"].grad, "db1": None if P["b1"] is None else P["b1"].grad,
           "db2": None if P["b2"] is None else P["b2"].grad}
    # condition scales: the same sums over absolute values
    ia = inter.detach().abs().requires_grad_(True)
    wa = P["w2"].detach().abs().requires_grad_(True)
    F.conv2d(ia, wa, None, padding=1).backward(dl.abs())
    ref.update(dw2_scale=wa.grad, db1_scale=ia.grad.sum((0, 2, 3)), db2_scale=dl.abs().sum().reshape(1))
    # dW2 with the intermediate NOT cropped: the pairs whose intermediate pixel lies on the ring
    # outside the image included. ring_term = what the kernel's correction C must remove.
    wf = P["w2"].detach().clone().requires_grad_(True)
    F.conv2d(full[:, :, 1:OH + 3, 1:OW + 3], wf, None).backward(dl)
    ref["ring_term"] = wf.grad - ref["dw2"]
    return ref


def head_ref(shape_id, form, pattern="dense"):
    """The fp64 expectations of the case (cached, shared, read-only)."""
    return _reference(shape_id, pattern, KIND[form])
