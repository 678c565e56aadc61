"""The conv launchers across operand forms, straight through the C-ABI, against the fp64
expectations of tests/conv_cases.py (proved on the CPU by tests/test_conv_cases_cpu.py), and
with the kernel that ran asserted by name (isg_last_launch).

One row per (kernel, direction) — conv_cases.ROWS — in every form of conv_cases.FORMS:
  base      contiguous, aligned operands, one sink: as tests/test_gpu_kernels.py runs them
  slice     every operand a channel slice of a wider buffer (NaN around inputs, a poison
            value around outputs, which must survive); the fast kernel still takes it
  off4      the same slices 4 bytes off a 16-B boundary with n_stride % 4 != 0: the call
            succeeds on a kernel the row allows, and the aligned-only kernel did not run
  replicas  consumed statistics spread over the replicas, produced accumulators preloaded
  coef      every BatchNorm as finalised coefficients of a layer wider than the segment;
            gamma, beta and the consumed statistics are NaN
  sinks3    three input segments with three transforms into NONE / ACCUM / STORE or ACTBWD
            sinks (segs3 for the weight gradients: x in three segments, dy in two); a
            launcher whose contract takes one segment and one sink refuses it
  n1        base at N = 1
The bars are tests/test_gpu_kernels.py's: 2e-5 of the reference's scale + 1e-6 (4e-6 on the
s2k5 rows), whatever the form."""
import numpy as np
import pytest
import torch

from instancesegmentation_amd import _lib as L
from tests import conv_cases as CC
from tests.isg_helpers import (NAN, POISON, Slab, bn_spec_eval, bn_spec_train, call, dev, geom, ptr,
                               rep_fold, rep_from, rep_spread, rep_zeros, same_bits, sinks, stream, vt)
from tests.test_gpu_kernels import close

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = torch.from_numpy
_FAULT = []  # a GPU fault ends the module: nothing more is launched on a faulted device


def lay(form, C, H, W):
    """Where a [N, C, H, W] operand sits in its allocation."""
    if form == "slice":
        return dict(pad=3, c0=2)
    if form == "off4":
        return dict(pad=3, c0=2, off=1, tail=1 if ((C + 3) * H * W + 1) % 4 else 2)
    return dict(pad=0, c0=0)


def preload(n):
    """Non-zero dyadic values in every replica of an accumulator of n values."""
    r = torch.arange(L.STAT_REP, dtype=torch.float64)[:, None]
    i = torch.arange(n, dtype=torch.float64)[None, :]
    return 0.25 * (r + 1) + 0.125 * (i % 5)


class Run:
    """The device operands of one case; everything stays alive until the results are read."""

    def __init__(self, case):
        self.case, self.form, self.N = case, case["form"], case["N"]
        self.keep, self.inputs, self.outputs, self.checks = [], [], [], []

    def slab(self, C, H, W, data, fill, out=False):
        sl = Slab(C, H, W, data=data, fill=fill, N=self.N, **lay(self.form, C, H, W))
        (self.outputs if out else self.inputs).append(sl)
        return sl

    def bn(self, st, accum=False):
        """(isg_bn spec, its statistics buffer, what its gsum / gxsum halves were preloaded with)."""
        bnC = st["bnC"]
        GA, BE = dev(st["gamma"]), dev(st["beta"])
        self.keep += [GA, BE]
        pre = torch.zeros(L.STAT_REP, 2 * bnC, dtype=torch.float64)
        if st["bn"] == "eval":
            RM, RV = dev(st["rm"]), dev(st["rv"])
            ST = rep_zeros(4 * bnC) if accum else None
            spec = dict(bn_spec_eval(GA, BE, RM, RV), stats=ptr(ST))
            self.keep += [RM, RV, ST]
            return spec, ST, pre
        if st["bn"] == "train":
            ST = rep_spread(st["stats"]) if self.form == "replicas" else rep_from(T(st["stats"]))
            spec = bn_spec_train(GA, BE, ST, st["count"])
        else:  # finalised coefficients; gamma, beta and the consumed statistics hold NaN
            CO = dev(CC.coef_of(st))
            ST = torch.full((L.STAT_REP * 4 * bnC,), NAN, dtype=torch.float64, device=DEV)
            GA.fill_(NAN)
            BE.fill_(NAN)
            if accum:
                ST.view(L.STAT_REP, 4 * bnC)[:, 2 * bnC:] = 0.0
            spec = dict(bn_spec_train(GA, BE, ST, st["count"]), coef=ptr(CO))
            self.keep.append(CO)
        if accum and self.form == "replicas":
            pre = preload(2 * bnC)
            ST.view(L.STAT_REP, 4 * bnC)[:, 2 * bnC:] += pre.to(DEV)
        self.keep.append(ST)
        return spec, ST, pre

    def seg(self, sg, H, W):
        sl = self.slab(sg["C"], H, W, sg["p"], NAN)
        s = {"p": sl.ptr, "n_stride": sl.n_stride, "C": sg["C"], "xform": L.XF_PLAIN}
        if sg["xf"] == "plain":
            return s
        s["bn"] = self.bn(sg)[0]
        if sg["xf"] == "bn_fwd":
            s.update(xform=L.XF_BN_FWD, act=L.ACT[sg["act"]])
            if sg["act"] == "prelu":
                SL = dev(sg["slope"])
                self.keep.append(SL)
                s["slope"] = ptr(SL)
            return s
        ysl = self.slab(sg["C"], H, W, sg["y"], NAN)
        s.update(xform=L.XF_BN_BWD, y=ysl.ptr, y_n_stride=ysl.n_stride)
        return s

    def vt(self, segs, H, W):
        return vt([self.seg(sg, H, W) for sg in segs], self.N, H, W)

    def sink(self, sk, H, W, tol):
        C, mode = sk["C"], sk["mode"]
        s = {"c0": sk["c0"], "C": C}
        if mode == "none":  # a real buffer that must stay as it is
            sl = self.slab(C, H, W, None, POISON)
            s.update(p=sl.ptr, n_stride=sl.n_stride, mode=L.SINK_NONE)
            return s
        sl = self.slab(C, H, W, sk.get("old"), POISON, out=True)
        s.update(p=sl.ptr, n_stride=sl.n_stride)
        self.checks.append(lambda: close(sl.get(), T(sk["out"]), tol, f"{mode} sink at row {sk['c0']}"))
        if mode == "accum":
            s["mode"] = L.SINK_ACCUM
        elif mode == "store":
            B, ST = dev(sk["bias"]), rep_zeros(4 * C)
            pre = preload(2 * C) if self.form == "replicas" else torch.zeros(L.STAT_REP, 2 * C, dtype=torch.float64)
            ST.view(L.STAT_REP, 4 * C)[:, :2 * C] += pre.to(DEV)
            self.keep += [B, ST]
            s.update(mode=L.SINK_STORE, bias=ptr(B), stats=ptr(ST))

            def stats():
                got = rep_fold(ST, 4 * C).cpu()
                assert not got[2 * C:].any(), "a STORE sink's gsum / gxsum halves changed"
                close(got[:C] - pre.sum(0)[:C], T(sk["sum"]), tol, "sum")
                close(got[C:2 * C] - pre.sum(0)[C:], T(sk["sumsq"]), tol, "sumsq")
            self.checks.append(stats)
        else:  # actbwd
            bnC = sk["bnC"]
            ysl = self.slab(C, H, W, sk["y"], NAN)
            spec, ST, pre = self.bn(sk, accum=True)
            SL, SG = dev(sk["slope"]), rep_zeros(C)
            spre = preload(C) if self.form == "replicas" else torch.zeros(L.STAT_REP, C, dtype=torch.float64)
            SG.view(L.STAT_REP, C)[:] += spre.to(DEV)
            self.keep += [SL, SG]
            s.update(mode=L.SINK_ACTBWD, act=L.ACT[sk["act"]], y=ysl.ptr, y_n_stride=ysl.n_stride,
                     slope=ptr(SL), slope_grad=ptr(SG), bn=spec)

            def sums():
                got = ST.view(L.STAT_REP, 4 * bnC)[:, 2 * bnC:].sum(0).cpu() - pre.sum(0)
                close(got[:C], T(sk["gsum"]), tol, "gsum")
                close(got[bnC:bnC + C], T(sk["gxsum"]), tol, "gxsum")
                assert not got[C:bnC].any() and not got[bnC + C:].any(), "sums outside the sink's channels"
                close(rep_fold(SG, C).cpu() - spre.sum(0), T(sk["slope_grad"]), tol, "slope gradient")
            self.checks.append(sums)
        return s

    def sinks(self, H, W, tol):
        return sinks([self.sink(sk, H, W, tol) for sk in self.case["sinks"]])

    def finish(self, refused):
        torch.cuda.synchronize()
        for sl in self.inputs:
            sl.outside_untouched("an input", whole=True)
        for sl in self.outputs:
            sl.outside_untouched("around an output slice", whole=refused)
        if not refused:
            for chk in self.checks:
                chk()


def launch_checked(row, form, fn):
    """Run fn (the call under test) and hold its launch name against the row's table entry.
    Returns True when the form is one the contract refuses (and it was refused as documented)."""
    want = CC.expected_launch(row, form)
    if isinstance(want, int):
        with pytest.raises(RuntimeError, match=rf"\({want}\)"):
            fn()
        return True
    fn()
    name = L.lib().isg_last_launch().decode()
    print(f"{row.id} {form}: {name}")
    assert any(name.startswith(w) for w in want), f"{row.id} {form}: ran {name}, the row allows {want}"
    if row.launch not in want:
        assert not name.startswith(row.launch)
    return False


def geom_of(row, N):
    return geom(N=N, Ci=row.Ci, H=row.H, W=row.W, Co=row.Co, OH=row.OH, OW=row.OW, KH=row.k[0],
                KW=row.k[1], SH=row.s, SW=row.s, PH=row.p[0], PW=row.p[1], DH=row.d, DW=row.d,
                groups=row.groups)


def run_case(rid, form):
    case = CC.make_case(rid, form)
    row, N = case["row"], case["N"]
    r = Run(case)
    W_ = dev(case["w"])
    ge = geom_of(row, N)
    if row.dirn in ("fwd", "dgrad"):
        fwd = row.dirn == "fwd"
        sH, sW, oH, oW = (row.H, row.W, row.OH, row.OW) if fwd else (row.OH, row.OW, row.H, row.W)
        src, out = r.vt(case["src"], sH, sW), r.sinks(oH, oW, row.tol)
        refused = launch_checked(row, form, lambda: call(
            "isg_conv_fwd" if fwd else "isg_conv_dgrad", ge, src, ptr(W_), out, stream()))
        r.finish(refused)
        return
    nw = int(np.prod(CC.wshape(row)))
    stride_ = nw + row.Co + 5  # replica stride: weight, bias, padding
    REP = torch.zeros(L.WREP * stride_, dtype=torch.float64, device=DEV)
    dbias = ptr(REP[nw:]) if row.dbias else None
    dy, x = r.vt(case["dy"], row.OH, row.OW), r.vt(case["x"], row.H, row.W)
    if row.dirn == "wgrad":
        fn = lambda: call("isg_conv_wgrad_rep", ge, dy, x, ptr(REP), dbias, stride_, L.WREP, stream())
    else:
        out = r.sinks(row.H, row.W, row.tol)
        fn = lambda: call("isg_depthwise_bwd", ge, dy, ptr(W_), out, x, ptr(REP), dbias, stride_,
                          L.WREP, stream())
    refused = launch_checked(row, form, fn)
    r.finish(refused)
    if refused:
        assert not REP.any(), "a refused weight gradient wrote its replicas"
        return
    OUT = torch.full((stride_,), NAN, device=DEV)
    call("isg_sum_replicas", ptr(OUT), ptr(REP), stride_, L.WREP, stride_, stream())
    torch.cuda.synchronize()
    close(OUT[:nw].view(CC.wshape(row)), T(case["dw"]), row.tol, "weight gradient")
    if row.dbias:
        close(OUT[nw:nw + row.Co], T(case["dbias"]), row.tol, "bias gradient")
    assert torch.all(OUT[nw + (row.Co if row.dbias else 0):] == 0), "words past the gradient changed"


@pytest.mark.parametrize("rid,form", CC.CASES, ids=[f"{r}-{f}" for r, f in CC.CASES])
def test_conv_form(rid, form):
    if _FAULT:
        pytest.fail(f"not run: an earlier case met a GPU fault ({_FAULT[0]})")
    try:
        run_case(rid, form)
    except RuntimeError as e:
        if "(-3)" in str(e) or "HIP error" in str(e) or "hipError" in str(e):
            _FAULT.append(f"{rid}-{form}: {e}"[:300])
        raise


def test_last_launch_names_the_latest_launch_of_this_thread():
    lib = L.lib()
    B = torch.zeros(8, dtype=torch.float64, device=DEV)
    call("isg_fill_f64", ptr(B), 8, 1.5, stream())
    assert lib.isg_last_launch() == b"fill_f64_kernel"
    O = torch.zeros(4, device=DEV)
    call("isg_sum_replicas", ptr(O), ptr(B), 4, 2, 4, stream())
    assert lib.isg_last_launch().startswith(b"sum_rep")
    same_bits(O, torch.full((4,), 3.0), "the probe changes nothing the launch computes")
