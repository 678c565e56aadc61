"""Fused mask head (isg_mask_head_fwd / _bwd, csrc/mask_head.hip) against an fp64 torch
restatement of the reference's two layers (segment.py:435-438, 504-505:
ConvTranspose2d(16 -> 4, k8, s4, p2) then Conv2d(4 -> 1, 3x3, p1)), forward and backward
(input gradient through a STORE and an ACCUM sink, all four parameter gradients summed
over the weight-gradient replicas), on whole and partial tiles; then the case table of
tests/head_cases.py: every operand form on shapes that make the backward's persistent
workgroups loop, with the instantiation that ran asserted by name (isg_last_launch)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from instancesegmentation_amd import _lib as L
from tests import head_cases as HC
from tests.isg_helpers import (NAN, POISON, Slab, bits, bn_spec_eval, bn_spec_train, call, dev, ptr, rep_from,
                               rep_spread, same_bits, struct)

pytestmark = pytest.mark.gpu
DEV = "cuda"
_FAULT = []  # a GPU fault ends the module: nothing more is launched on a faulted device


def guarded(fn):
    """Run the test unless an earlier one of this module met a GPU fault; record one met here."""
    @functools.wraps(fn)
    def run(*a, **kw):
        if _FAULT:
            pytest.fail(f"not run: an earlier case met a GPU fault ({_FAULT[0]})")
        try:
            return fn(*a, **kw)
        except RuntimeError as e:
            if "(-3)" in str(e) or "HIP error" in str(e) or "hipError" in str(e):
                _FAULT.append(f"{fn.__name__} {a} {kw}: {e}"[:300])
            raise
    return run


def _case(N, Hi, Wi, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, 16, Hi, Wi, generator=g)
    w1 = torch.randn(16, 4, 8, 8, generator=g) * 0.05
    b1 = torch.randn(4, generator=g) * 0.1
    w2 = torch.randn(1, 4, 3, 3, generator=g) * 0.3
    b2 = torch.randn(1, generator=g) * 0.1
    dl = torch.randn(N, 1, 4 * Hi, 4 * Wi, generator=g)
    return x, w1, b1, w2, b2, dl


def _ref(x, w1, b1, w2, b2, dl):
    P = [t.double().requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    y = F.conv2d(F.conv_transpose2d(P[0], P[1], P[2], stride=4, padding=2), P[3], P[4], padding=1)
    y.backward(dl.double())
    return y.detach(), [p.grad for p in P]


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-12)


@pytest.mark.parametrize("N,Hi,Wi", [(2, 8, 16), (1, 5, 7), (2, 17, 33), (1, 64, 64)])
@guarded
def test_mask_head_fwd_bwd(N, Hi, Wi):
    x, w1, b1, w2, b2, dl = _case(N, Hi, Wi, Hi * 100 + Wi)
    ref_y, ref_g = _ref(x, w1, b1, w2, b2, dl)
    d = {k: v.to(DEV).contiguous() for k, v in dict(x=x, w1=w1, b1=b1, w2=w2, b2=b2, dl=dl).items()}
    OH, OW = 4 * Hi, 4 * Wi
    out = torch.full((N, 1, OH, OW), 7.0, device=DEV)
    # two input segments (channels 0-9, 10-15) exercise the vtensor segment split
    xa, xb = d["x"][:, :10].contiguous(), d["x"][:, 10:].contiguous()
    seg = lambda t, C: {"p": t.data_ptr(), "n_stride": C * Hi * Wi, "C": C, "xform": L.XF_PLAIN}
    ring = torch.full((N, L.head_ring_floats(Hi, Wi)), float("nan"), device=DEV)
    base = {"x": {"s": [seg(xa, 10), seg(xb, 6)], "nseg": 2, "N": N, "H": Hi, "W": Wi},
            "w1": d["w1"].data_ptr(), "b1": d["b1"].data_ptr(), "w2": d["w2"].data_ptr(),
            "b2": d["b2"].data_ptr(), "N": N, "Hi": Hi, "Wi": Wi, "ring": ring.data_ptr()}
    a = struct(L.MaskHead, dict(base, out=out.data_ptr(), out_n_stride=OH * OW))
    call("isg_mask_head_fwd", a, L.stream_ptr())
    e = _rel(out, ref_y)
    print(f"{N}x16x{Hi}x{Wi}: logits rel err {e:.2e}")
    assert e < 2e-6
    # the ring: the un-cropped intermediate one pixel outside the image (isg.h)
    full = F.conv_transpose2d(x.double(), w1.double(), b1.double(), stride=4)  # no crop: p = -2
    OHf = full.shape[2]
    rg = ring.view(N, 4, -1).double().cpu()
    exp = torch.cat([full[:, :, 1, 1:OW + 3], full[:, :, OH + 2, 1:OW + 3],
                     full[:, :, 2:OH + 2, 1], full[:, :, 2:OH + 2, OW + 2]], 2)
    assert OHf == OH + 4 and rg.shape == exp.shape
    er = (rg - exp).abs().max().item() / max(exp.abs().max().item(), 1e-12)
    print(f"ring rel err {er:.2e}")
    assert er < 2e-6
    # backward: dx of channels 0-9 STOREd, 10-15 ACCUMulated onto a preset value
    dxa = torch.full((N, 10, Hi, Wi), 5.0, device=DEV)
    pre = torch.randn(N, 6, Hi, Wi, device=DEV)
    dxb = pre.clone()
    R, nrep = 4096 + 4 + 36 + 1, L.WREP
    rep = torch.zeros(nrep * R, dtype=torch.float64, device=DEV)  # fp64 replicas (isg.h)
    rp = rep.data_ptr()
    sk = [{"p": dxa.data_ptr(), "n_stride": 10 * Hi * Wi, "c0": 0, "C": 10, "mode": L.SINK_STORE},
          {"p": dxb.data_ptr(), "n_stride": 6 * Hi * Wi, "c0": 10, "C": 6, "mode": L.SINK_ACCUM}]
    b = struct(L.MaskHead, dict(base, dout=d["dl"].data_ptr(), dout_n_stride=OH * OW,
                                dx={"s": sk, "nsink": 2}, dw1=rp, db1=rp + 8 * 4096,
                                dw2=rp + 8 * 4100, db2=rp + 8 * 4136, rep_stride=R, nrep=nrep))
    call("isg_mask_head_bwd", b, L.stream_ptr())
    tot = rep.view(nrep, R).sum(0).float().cpu()
    dx = torch.cat([dxa.cpu(), (dxb - pre).cpu()], 1)
    errs = {"dx": _rel(dx, ref_g[0]), "dw1": _rel(tot[:4096].view(16, 4, 8, 8), ref_g[1]),
            "db1": _rel(tot[4096:4100], ref_g[2]), "dw2": _rel(tot[4100:4136].view(1, 4, 3, 3), ref_g[3]),
            "db2": _rel(tot[4136:4137], ref_g[4])}
    print({k: f"{v:.1e}" for k, v in errs.items()})
    assert all(v < 2e-5 for v in errs.values()), errs


@pytest.mark.parametrize("N,Hi,Wi", [(2, 8, 16), (1, 17, 33), (2, 64, 64), HC.SHAPES["loop_odd"],
                                     HC.SHAPES["loop_even"]])
@guarded
def test_mask_head_bwd_slab_fold_matches_atomics(N, Hi, Wi):
    """The convT weight gradient through the per-workgroup slab (isg_mask_head.dw1_part)
    and the later fold (isg_mask_head_fold, the train plan's side-stream op) equals the
    in-kernel fp64 atomics bit for bit (both are exact fp64 sums of the same fp32
    partials), and every other output is unchanged. The two loop shapes fill the slab: 256
    rows carried across two tiles, folded in 16 chunks, one into every replica."""
    x, w1, b1, w2, b2, dl = _case(N, Hi, Wi, 7 * Hi + Wi)
    d = {k: v.to(DEV).contiguous() for k, v in dict(x=x, w1=w1, b1=b1, w2=w2, b2=b2, dl=dl).items()}
    OH, OW = 4 * Hi, 4 * Wi
    ring = torch.zeros(N, L.head_ring_floats(Hi, Wi), device=DEV)
    base = {"x": {"s": [{"p": d["x"].data_ptr(), "n_stride": 16 * Hi * Wi, "C": 16,
                         "xform": L.XF_PLAIN}], "nseg": 1, "N": N, "H": Hi, "W": Wi},
            "w1": d["w1"].data_ptr(), "b1": d["b1"].data_ptr(), "w2": d["w2"].data_ptr(),
            "b2": d["b2"].data_ptr(), "N": N, "Hi": Hi, "Wi": Wi, "ring": ring.data_ptr()}
    out = torch.zeros(N, 1, OH, OW, device=DEV)
    call("isg_mask_head_fwd", struct(L.MaskHead, dict(base, out=out.data_ptr(), out_n_stride=OH * OW)),
         L.stream_ptr())
    nslab = L.head_part_floats(N, Hi, Wi)
    assert nslab == L.lib().isg_mask_head_part_floats(N, Hi, Wi)
    R, nrep = 4096 + 4 + 36 + 1, L.WREP

    def run(slab):
        dx = torch.full((N, 16, Hi, Wi), float("nan"), device=DEV)
        rep = torch.zeros(nrep * R, dtype=torch.float64, device=DEV)
        part = torch.full((nslab,), float("nan"), device=DEV)
        rp = rep.data_ptr()
        sk = [{"p": dx.data_ptr(), "n_stride": 16 * Hi * Wi, "c0": 0, "C": 16, "mode": L.SINK_STORE}]
        b = struct(L.MaskHead, dict(base, dout=d["dl"].data_ptr(), dout_n_stride=OH * OW,
                                    dx={"s": sk, "nsink": 1}, dw1=rp, db1=rp + 8 * 4096,
                                    dw2=rp + 8 * 4100, db2=rp + 8 * 4136, rep_stride=R, nrep=nrep,
                                    dw1_part=part.data_ptr() if slab else None))
        call("isg_mask_head_bwd", b, L.stream_ptr())
        if slab:
            call("isg_mask_head_fold", b, L.stream_ptr())
        reps.append(rep.view(nrep, R).cpu())
        return dx, rep.view(nrep, R).sum(0)

    reps = []
    (dxa, ta), (dxb, tb) = run(True), run(False)
    if N >= 57:
        assert nslab == 256 * 4096 and (nslab // 4096 + 15) // 16 == nrep == 16
        assert all(r[:, :4096].abs().sum(1).min().item() > 0 for r in reps), "a replica received no chunk"
    assert torch.equal(dxa, dxb)
    assert torch.equal(ta, tb), (ta - tb).abs().max().item()
    ref_y, ref_g = _ref(x, w1, b1, w2, b2, dl)
    assert _rel(ta[:4096].float().view(16, 4, 8, 8), ref_g[1]) < 2e-5


# ---- the case table: tests/head_cases.py (proved on the CPU by tests/test_head_cases_cpu.py) ----
# One shape x dlogits pattern in every operand form:
#   base      one PLAIN segment, one STORE sink, contiguous and aligned
#   slice     every tensor operand a slice of a wider buffer (NaN around inputs, a poison value
#             around outputs, which must survive); logits and dlogits with an image-stride tail
#   off4      the same slices 4 bytes off a 16-B boundary, n_stride % 4 != 0: the scalar kernel
#   segs3     plain | BatchNorm(train) + PReLU | BatchNorm(eval) + ReLU into NONE / ACCUM / STORE
#   coef      finalised coefficients of a wider layer; gamma, beta, statistics are NaN
#   act_only  BN_FWD with PReLU and no statistics
#   nobias    b1 = b2 = NULL, db1 = db2 = NULL
#   replicas  produced replicas preloaded (nrep = ISG_WREP, and nrep = 1 without a stride);
#             consumed statistics spread over their replicas
#   skip      one run per output with that output NULL (and nsink = 0)
# Bars: logits and ring 2e-6 of the reference's max; dx and dW1 2e-5 of the tensor's max; dW2,
# db1, db2 elementwise 2e-5 of that element's condition scale (the same sum over absolute values).
T = torch.from_numpy
VEC, SCALAR = "head_bwd_kernel<vec>", "head_bwd_kernel<scalar>"
RSTRIDE = HC.R_LEN + 3  # a replica and three words that must stay zero
OUTPUTS = {"dw1": (HC.R_DW1, HC.R_DB1), "db1": (HC.R_DB1, HC.R_DW2), "dw2": (HC.R_DW2, HC.R_DB2),
           "db2": (HC.R_DB2, HC.R_LEN)}


def lay(form, C, H, W, image=False):
    """Where a [N, C, H, W] operand sits in its allocation (image: logits / dlogits)."""
    if form == "slice":
        return dict(pad=3, c0=2, tail=8 if image else 0)
    if form == "off4":
        return dict(pad=3, c0=2, off=1, tail=1 if ((C + 3) * H * W + 1) % 4 else 2)
    return dict(pad=0, c0=0)


class Flat:
    """A contiguous operand (a weight, the ring) inside a guarded allocation: 16 words of `fill`
    before and after, `off` more words before it (the 16-B alignment given away)."""

    def __init__(self, n, data=None, fill=NAN, off=0):
        self.n, self.o = n, 16 + off
        self.flat = torch.full((n + 32 + off,), fill, dtype=torch.float32, device=DEV)
        if data is not None:
            self.flat[self.o:self.o + n] = dev(np.asarray(data, np.float32).reshape(-1))
        self.ptr = self.flat[self.o:].data_ptr()
        self.before = self.flat.clone()

    def get(self):
        return self.flat[self.o:self.o + self.n]

    def outside_untouched(self, what, whole=False):
        changed = bits(self.flat) != bits(self.before)
        if not whole:
            changed[self.o:self.o + self.n] = False
        assert not changed.any(), f"{what}: {int(changed.sum())} words around it changed"


def preload(nrep):
    """Non-zero dyadic values in every word of every replica (as test_gpu_conv_forms.preload)."""
    r = torch.arange(nrep, dtype=torch.float64)[:, None]
    i = torch.arange(RSTRIDE, dtype=torch.float64)[None, :]
    return 0.25 * (r + 1) + 0.125 * (i % 5)


class Res:
    """What one forward + backward left behind, on the CPU."""


def run_head(case, form, skip=None, nrep=None, pre=False, spread=False):
    """Forward (with and without the ring) and backward of `case` presented in `form`;
    everything around the operands is verified untouched before the results are returned."""
    N, Hi, Wi = case["N"], case["Hi"], case["Wi"]
    OH, OW = 4 * Hi, 4 * Wi
    lf = form if form in ("slice", "off4") else "base"
    o1 = 1 if lf == "off4" else 0
    inputs, outputs, keep = [], [], []

    def slab(C, H, W, data, fill, out=False, image=False):
        sl = Slab(C, H, W, data=data, fill=fill, N=N, **lay(lf, C, H, W, image))
        (outputs if out else inputs).append(sl)
        return sl

    def flat(n, data, fill, off=0, out=False):
        fl = Flat(n, data, fill, off if lf != "base" else 0)
        (outputs if out else inputs).append(fl)
        return fl

    segs = []
    for sg in case["segs"]:
        sl = slab(sg["C"], Hi, Wi, sg["x"], NAN)
        s = {"p": sl.ptr, "n_stride": sl.n_stride, "C": sg["C"], "xform": L.XF_PLAIN}
        kind = sg["kind"]
        if kind != "plain":
            s.update(xform=L.XF_BN_FWD, act=L.ACT[sg["act"]])
            if sg["act"] == "prelu":
                SL = dev(sg["slope"])
                keep.append(SL)
                s["slope"] = ptr(SL)
            if kind == "act_only":
                s["bn"] = {"C": sg["C"], "train": 1, "count": 1.0, "eps": 1e-5}
            else:
                GA, BE = dev(sg["gamma"]), dev(sg["beta"])
                keep += [GA, BE]
                if kind == "bn_eval":
                    RM, RV = dev(sg["rm"]), dev(sg["rv"])
                    keep += [RM, RV]
                    s["bn"] = bn_spec_eval(GA, BE, RM, RV)
                elif kind == "bn_train":
                    ST = rep_spread(sg["stats"]) if spread else rep_from(T(sg["stats"]))
                    keep.append(ST)
                    s["bn"] = bn_spec_train(GA, BE, ST, sg["count"])
                else:  # finalised coefficients; gamma, beta and the statistics hold NaN
                    CO = dev(sg["coef"])
                    ST = torch.full((L.STAT_REP * 4 * sg["bnC"],), NAN, dtype=torch.float64, device=DEV)
                    GA.fill_(NAN)
                    BE.fill_(NAN)
                    keep += [CO, ST]
                    s["bn"] = dict(bn_spec_train(GA, BE, ST, sg["count"]), coef=ptr(CO))
        segs.append(s)
    W1 = flat(4096, case["w1"], NAN)  # the kernels read it with 16-B loads: always aligned
    W2 = flat(36, case["w2"], NAN, o1)
    B1 = flat(4, case["b1"], NAN, o1) if case["b1"] is not None else None
    B2 = flat(1, case["b2"], NAN, o1) if case["b2"] is not None else None
    RN = L.head_ring_floats(Hi, Wi)
    RING = flat(N * RN, None, POISON, o1, out=True)
    OUT = slab(1, OH, OW, None, POISON, out=True, image=True)
    base = {"x": {"s": segs, "nseg": len(segs), "N": N, "H": Hi, "W": Wi}, "w1": W1.ptr, "w2": W2.ptr,
            "b1": B1.ptr if B1 else None, "b2": B2.ptr if B2 else None, "N": N, "Hi": Hi, "Wi": Wi}
    lib = L.lib()
    call("isg_mask_head_fwd", struct(L.MaskHead, dict(base, ring=RING.ptr, out=OUT.ptr, out_n_stride=OUT.n_stride)),
         L.stream_ptr())
    assert lib.isg_last_launch() == b"head_fwd_kernel"
    r = Res()
    r.logits, r.ring = OUT.get().cpu(), RING.get().view(N, 4, -1).cpu()
    # the inference path: no ring, the same logits
    OUT2 = slab(1, OH, OW, None, POISON, out=True, image=True)
    call("isg_mask_head_fwd", struct(L.MaskHead, dict(base, out=OUT2.ptr, out_n_stride=OUT2.n_stride)),
         L.stream_ptr())
    same_bits(OUT2.get(), r.logits, "logits without the ring")

    DL = slab(1, OH, OW, case["dl"], NAN, image=True)
    sk, r.dx, none = [], [], []
    parts = HC.SINKS3 if case["kind"] == "segs3" else (("store", 16),)
    c0 = 0
    for mode, C in parts:
        if mode == "none":  # a real buffer that must stay as it is
            sl = slab(C, Hi, Wi, None, POISON)
            sk.append({"p": sl.ptr, "n_stride": sl.n_stride, "c0": c0, "C": C, "mode": L.SINK_NONE})
        else:
            sl = slab(C, Hi, Wi, case["preset"] if mode == "accum" else None, POISON, out=True)
            sk.append({"p": sl.ptr, "n_stride": sl.n_stride, "c0": c0, "C": C,
                       "mode": L.SINK_ACCUM if mode == "accum" else L.SINK_STORE})
            r.dx.append((mode, c0, C, sl))
        c0 += C
    if skip == "dx":
        sk, r.dx = [], []
    nrep = nrep or L.WREP
    P0 = preload(nrep) if pre else torch.zeros(nrep, RSTRIDE, dtype=torch.float64)
    REP = P0.to(DEV).reshape(-1).contiguous()
    rp = REP.data_ptr()
    nob = case["b1"] is None
    outp = {k: rp + 8 * a for k, (a, _) in OUTPUTS.items() if k != skip and not (nob and k in ("db1", "db2"))}
    b = struct(L.MaskHead, dict(base, ring=RING.ptr, dout=DL.ptr, dout_n_stride=DL.n_stride,
                                dx={"s": sk, "nsink": len(sk)}, rep_stride=RSTRIDE if nrep > 1 else 0,
                                nrep=nrep, **outp))
    call("isg_mask_head_bwd", b, L.stream_ptr())
    r.name = lib.isg_last_launch().decode()
    for x in inputs:
        x.outside_untouched("an input", whole=True)
    for x in outputs:
        x.outside_untouched("around an output")
    same_bits(RING.get().view(N, 4, -1), r.ring, "the backward changed the ring")
    got = REP.view(nrep, RSTRIDE).cpu()
    r.tot = (got - P0).sum(0)[:HC.R_LEN]
    assert torch.equal(got[:, HC.R_LEN:], P0[:, HC.R_LEN:]), "words past the replica changed"
    for k, (a, e) in OUTPUTS.items():
        if k not in outp:
            assert torch.equal(got[:, a:e], P0[:, a:e]), f"{k} is NULL and its replicas changed"
    r.dx = [(mode, c0, C, sl.get().cpu()) for mode, c0, C, sl in r.dx]
    return r


def check_ref(r, case, ref, what):
    """The run against the fp64 expectations at the module's bars; every figure is printed."""
    def rel(got, want, bar, name, scale=None):
        got, want = got.double(), want.double()
        sc = max(want.abs().max().item(), 1e-12) if scale is None else scale
        e = (got - want).abs().max().item() / sc
        print(f"{what}: {name} {e:.2e} (bar {bar:.0e})")
        assert e < bar, f"{what}: {name} rel err {e:.3e} >= {bar:.0e}"

    def elementwise(got, want, scale, name):
        q = ((got.double() - want).abs() / scale.clamp_min(1e-300)).max().item()
        print(f"{what}: {name} {q:.2e} of its condition scale (bar 2e-05)")
        assert q <= 2e-5, f"{what}: {name} off by {q:.3e} of its condition scale"

    rel(r.logits, ref["logits"], 2e-6, "logits")
    rel(r.ring, ref["ring"], 2e-6, "ring")
    dmax = max(ref["dx"].abs().max().item(), 1e-12)
    for mode, c0, C, got in r.dx:
        want = ref["dx"][:, c0:c0 + C]
        if mode == "accum":
            want = want + T(case["preset"]).double()
        rel(got, want, 2e-5, f"dx[{c0}:{c0 + C}] ({mode})", dmax)
    tot = r.tot
    rel(tot[:4096].view(16, 4, 8, 8), ref["dw1"], 2e-5, "dW1")
    elementwise(tot[HC.R_DW2:HC.R_DB2].view(1, 4, 3, 3), ref["dw2"], ref["dw2_scale"], "dW2")
    if case["b1"] is not None:
        elementwise(tot[HC.R_DB1:HC.R_DW2], ref["db1"], ref["db1_scale"], "db1")
        elementwise(tot[HC.R_DB2:], ref["db2"], ref["db2_scale"], "db2")


def expected_name(case, form):
    return VEC if case["Wi"] % 4 == 0 and form != "off4" else SCALAR


_BASE = {}


def base_run(sid, pattern):
    """The base form's results, run once per (shape, pattern): what the other plain forms must
    reproduce bit for bit."""
    if (sid, pattern) not in _BASE:
        _BASE[sid, pattern] = run_head(HC.head_case(sid, "base", pattern), "base")
    return _BASE[sid, pattern]


def same_as_base(r, b, what, but=None):
    same_bits(r.logits, b.logits, f"{what}: logits")
    same_bits(r.ring, b.ring, f"{what}: ring")
    if but != "dx":
        assert len(r.dx) == len(b.dx) == 1
        same_bits(r.dx[0][3], b.dx[0][3], f"{what}: dx")
    for k, (a, e) in OUTPUTS.items():
        if k != but:
            same_bits(r.tot[a:e], b.tot[a:e], f"{what}: {k} replica totals")


def run_case(sid, pattern, form):
    case, ref = HC.head_case(sid, form, pattern), HC.head_ref(sid, form, pattern)
    what = f"{sid}-{pattern}-{form}"
    want = expected_name(case, form)
    if form == "skip":
        b = base_run(sid, pattern)
        for out in ("dw1", "db1", "dw2", "db2", "dx"):
            r = run_head(case, "base", skip=out)
            assert r.name == want, (out, r.name)
            same_as_base(r, b, f"{what} without {out}", but=out)
            if out != "dx":
                a, e = OUTPUTS[out]
                assert not r.tot[a:e].any()
        return
    if form == "replicas":
        b = base_run(sid, pattern)
        r = run_head(case, "base", pre=True)
        assert r.name == want
        check_ref(r, case, ref, what + " preloaded")
        same_as_base(r, b, what + " preloaded")
        r = run_head(case, "base", pre=True, nrep=1)
        assert r.name == want
        same_as_base(r, b, what + " nrep 1")
        c3, ref3 = HC.head_case(sid, "segs3", pattern), HC.head_ref(sid, "segs3", pattern)
        r = run_head(c3, "segs3", spread=True, pre=True)
        assert r.name == want
        check_ref(r, c3, ref3, what + " spread statistics")
        return
    r = base_run(sid, pattern) if form == "base" else run_head(case, form)
    print(f"{what}: {r.name}")
    assert r.name == want, f"{what}: ran {r.name}, expected {want}"
    check_ref(r, case, ref, what)
    if form == "slice":
        same_as_base(r, base_run(sid, pattern), what)
    if form == "off4":  # another db2 summation order: to tolerance, not bitwise
        b = base_run(sid, pattern)
        same_bits(r.logits, b.logits, f"{what}: logits")
        d = (r.dx[0][3].double() - b.dx[0][3].double()).abs().max().item()
        assert d <= 2e-5 * ref["dx"].abs().max().item()
    if pattern == "ones":  # a tile skipped or counted twice shows as an integer
        assert r.tot[HC.R_DB2].item() == case["N"] * 16 * case["Hi"] * case["Wi"]


CASES = HC.gpu_cases()


@pytest.mark.parametrize("sid,pattern,form", CASES, ids=["-".join(c) for c in CASES])
@guarded
def test_mask_head_form(sid, pattern, form):
    run_case(sid, pattern, form)
