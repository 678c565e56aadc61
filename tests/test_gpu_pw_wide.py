"""The K-pipelined 1x1 kernel (pw_gemm.hip pwp_kernel) through the C-ABI against an fp64
convolution computed here on the CPU, across its chunk, row-block and pixel-block edges and the
operand forms the stacked 256 -> 128+48 pair needs.

Shapes: K in {64, 132, 176, 256} (one chunk, two chunks and a 4-channel rest, three chunks with
a 48-channel rest — which is both 3*64 - 16 and the pair's 176 — and four whole chunks) x M in
{16, 48, 80} (one row block, ragged against 64, more than one block) x 2 images of H*W in
{64, 100, 4096} (one pixel block per image; a quad-aligned plane that is no multiple of 64, so
a block crosses the image boundary and the last one is ragged; many blocks), plus the pair's
own channel counts at H*W = 256. The operand forms rotate over the shapes.

Layers with K <= 128 belong to the slab kernel; ISG_PW_KERNEL=pwp (read per call) hands them to
pwp. K > 128 must reach it with nothing set.

Bars, from the arithmetic and not from what the kernel gives:
  element    (K + 2) * 2^-24 * sum_k |w x|  (a K-term fp32 fma chain, and the transform's
             roundings of x) + one rounding of the stored value (bias add, accumulate, slope)
  statistic  (pixels + 8) * 2^-24 * sum |term|
  everything around the output slices keeps its poison."""
import numpy as np
import pytest
import torch

from instancesegmentation_amd import _lib as L
from tests import conv_cases as CC
from tests.isg_helpers import (NAN, POISON, Slab, bits, bn_spec_train, call, dev, geom, ptr, rep_fold,
                               rep_from, rep_zeros, same_bits, sinks, stream, struct)
from tests.test_gpu_conv_forms import Run

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
KS, MS, HWS = (64, 132, 176, 256), (16, 48, 80), ((8, 8), (10, 10), (64, 64))
FWD_FORMS = [(s, k) for s in ("plain", "bnfwd") for k in ("store1", "store2")]
DG_FORMS = ["actbwd_relu", "actbwd_prelu", "accum"]
SHAPES = [(K, M, hw) for K in KS for M in MS for hw in HWS]
FWD = [("fwd", K, M, hw) + FWD_FORMS[i % 4] for i, (K, M, hw) in enumerate(SHAPES)]
FWD += [("fwd", 256, 176, (16, 16), s, "store2") for s in ("plain", "bnfwd")]
DGRAD = [("dgrad", K, M, hw, "bnbwd2", DG_FORMS[i % 3]) for i, (K, M, hw) in enumerate(SHAPES)]
DGRAD += [("dgrad", 176, 256, (16, 16), "bnbwd2", k) for k in DG_FORMS]


def _id(c):
    return f"{c[0]}-K{c[1]}-M{c[2]}-hw{c[3][0] * c[3][1]}-{c[4]}-{c[5]}"


def build(dirn, K, M, hw, src, sink, seed):
    """fp32 operands, their fp64 values and what each sink must hold: K is the GEMM's reduction
    (forward Ci, input gradient Co), M its rows."""
    rng = np.random.default_rng(seed)
    N, (H, W) = 2, hw
    if src == "plain":
        segs = [CC.make_seg(rng, N, K, H, W, "plain")]
    elif src == "bnfwd":  # BatchNorm + PReLU, the coefficients taken from the statistics
        segs = [CC.make_seg(rng, N, K, H, W, "bn_fwd", "prelu", "train")]
    else:  # a stacked pair's two gradient segments, each rebuilt from its saved output
        k2 = 48 if K > 48 else 20
        segs = [CC.make_seg(rng, N, K - k2, H, W, "bn_bwd", bn="train"),
                CC.make_seg(rng, N, k2, H, W, "bn_bwd", bn="train")]
    fwd = dirn == "fwd"
    w = (rng.normal(0.0, 1.0, (M, K) if fwd else (K, M)) * (2.0 / K) ** 0.5).astype(np.float32)
    a = w.astype(np.float64) if fwd else w.astype(np.float64).T  # [M][K]
    x = np.concatenate([s["v"] for s in segs], 1).reshape(N, K, H * W)
    v = (a @ x).reshape(N, M, H, W)
    mag = (np.abs(a) @ np.abs(x)).reshape(N, M, H, W)
    if sink == "store2":  # split where no tile and no quad ends (the pair: 128 | 48)
        cut = 128 if M == 176 else M - 5
        parts = [(0, cut, "store"), (cut, M - cut, "store")]
    else:
        parts = [(0, M, {"store1": "store", "accum": "accum"}.get(sink, "actbwd"))]
    sks = [CC.make_sink(rng, N, c0, C, H, W, mode, v[:, c0:c0 + C], bn="train",
                        act=sink.split("_")[-1] if mode == "actbwd" else "none")
           for c0, C, mode in parts]
    return dict(form="slice", N=N, H=H, W=W, K=K, M=M, fwd=fwd, src=segs, w=w, sinks=sks,
                bar=(K + 2) * U * mag)


class Launch:
    """One case on the device: slices of wider buffers, NaN around inputs, poison around outputs."""

    def __init__(self, case, form="slice"):
        self.case = case
        self.r = Run(dict(case, form=form))
        N, H, W = case["N"], case["H"], case["W"]
        self.src = self.r.vt(case["src"], H, W)
        self.W_ = dev(case["w"])
        self.out, specs = [], []
        for sk in case["sinks"]:
            C = sk["C"]
            sl = Slab(C, H, W, data=sk.get("old"), fill=POISON, N=N)
            s = {"c0": sk["c0"], "C": C, "p": sl.ptr, "n_stride": sl.n_stride}
            o = {"sk": sk, "slab": sl}
            if sk["mode"] == "accum":
                s["mode"] = L.SINK_ACCUM
            elif sk["mode"] == "store":
                o["B"], o["ST"] = dev(sk["bias"]), rep_zeros(4 * C)
                s.update(mode=L.SINK_STORE, bias=ptr(o["B"]), stats=ptr(o["ST"]))
            else:
                o["y"] = Slab(C, H, W, data=sk["y"], fill=NAN, N=N)
                o["GA"], o["BE"], o["SL"] = dev(sk["gamma"]), dev(sk["beta"]), dev(sk["slope"])
                o["ST"], o["SG"] = rep_from(torch.from_numpy(sk["stats"])), rep_zeros(C)
                s.update(mode=L.SINK_ACTBWD, act=L.ACT[sk["act"]], y=o["y"].ptr, y_n_stride=o["y"].n_stride,
                         slope=ptr(o["SL"]), slope_grad=ptr(o["SG"]),
                         bn=bn_spec_train(o["GA"], o["BE"], o["ST"], sk["count"]))
            self.out.append(o)
            specs.append(s)
        self.sinks = sinks(specs)
        K, M = case["K"], case["M"]
        ci, co = (K, M) if case["fwd"] else (M, K)
        self.geom = geom(N=N, Ci=ci, H=H, W=W, Co=co, OH=H, OW=W, KH=1, KW=1, SH=1, SW=1, PH=0, PW=0,
                         DH=1, DW=1, groups=1)

    def run(self):
        call("isg_conv_fwd" if self.case["fwd"] else "isg_conv_dgrad", self.geom, self.src, ptr(self.W_),
             self.sinks, stream())
        return L.lib().isg_last_launch().decode()

    def check(self):
        case = self.case
        pixels = case["N"] * case["H"] * case["W"]
        for sl in self.r.inputs:
            sl.outside_untouched("an input", whole=True)
        for o in self.out:
            sk, sl, C, c0 = o["sk"], o["slab"], o["sk"]["C"], o["sk"]["c0"]
            sl.outside_untouched("around an output slice")
            bar = case["bar"][:, c0:c0 + C] + U * np.abs(sk["out"])
            err = np.abs(sl.get().double().cpu().numpy() - sk["out"])
            print(f"{sk['mode']} rows {c0}..{c0 + C}: max err / bar {np.max(err / bar):.3f}")
            assert np.all(err <= bar), f"{sk['mode']} sink at row {c0}: {np.max(err / bar):.3f} of the bar"

            def stat(got, terms, what):
                want, lim = terms.sum((0, 2, 3)), (pixels + 8) * U * np.abs(terms).sum((0, 2, 3))
                e = np.abs(got.cpu().numpy() - want)
                print(f"  {what}: max err / bar {np.max(e / np.maximum(lim, 1e-300)):.3f}")
                assert np.all(e <= lim), f"{what} of the sink at row {c0}"
            if sk["mode"] == "store":
                got = rep_fold(o["ST"], 4 * C)
                assert not got[2 * C:].any(), "a STORE sink's gsum / gxsum halves changed"
                stat(got[:C], sk["out"], "sum")
                stat(got[C:2 * C], sk["out"] ** 2, "sumsq")
            elif sk["mode"] == "actbwd":
                got = rep_fold(o["ST"], 4 * C).cpu() - torch.from_numpy(sk["stats"])
                assert not got[:2 * C].any(), "an ACTBWD sink's sum / sumsq halves changed"
                yc = sk["y"].astype(np.float64) - sk["mean"][None, :C, None, None]
                stat(got[2 * C:3 * C], sk["out"], "gsum")
                stat(got[3 * C:], sk["out"] * yc, "gxsum")
                v = case_v(case)[:, c0:c0 + C]
                stat(rep_fold(o["SG"], C), np.where(sk["z"] > 0, 0.0, sk["z"] * v) if sk["act"] == "prelu"
                     else np.zeros_like(v), "slope gradient")


def case_v(case):
    a = case["w"].astype(np.float64) if case["fwd"] else case["w"].astype(np.float64).T
    N, K, H, W = case["N"], case["K"], case["H"], case["W"]
    x = np.concatenate([s["v"] for s in case["src"]], 1).reshape(N, K, H * W)
    return (a @ x).reshape(N, case["M"], H, W)


def route(monkeypatch, K):
    """K > 128 reaches pwp by the launcher's own rule; narrower layers are handed to it."""
    if K > 128:
        monkeypatch.delenv("ISG_PW_KERNEL", raising=False)
    else:
        monkeypatch.setenv("ISG_PW_KERNEL", "pwp")


@pytest.mark.parametrize("c", FWD + DGRAD, ids=_id)
def test_pwp(c, monkeypatch):
    case = build(*c, seed=1000 + (FWD + DGRAD).index(c))
    route(monkeypatch, c[1])
    la = Launch(case)
    name = la.run()
    assert name.startswith("pwp_kernel"), f"ran {name}"
    la.check()


@pytest.mark.parametrize("c", [("fwd", 176, 48, (10, 10), "bnfwd", "store2"),
                               ("dgrad", 132, 48, (10, 10), "bnbwd2", "actbwd_prelu")], ids=_id)
def test_unaligned_twin_runs_the_chunked_kernel(c, monkeypatch):
    """The same numbers with every source row one float off a 16-B boundary: pw_kernel, same bar."""
    monkeypatch.delenv("ISG_PW_KERNEL", raising=False)
    case = build(*c, seed=77)
    la = Launch(case)
    assert la.run().startswith("pwp_kernel")
    la.check()
    tw = Launch(case, form="off4")
    name = tw.run()
    assert name.startswith("pw_kernel"), f"the unaligned twin ran {name}"
    tw.check()


def test_input_gradient_repeats_bitwise(monkeypatch):
    monkeypatch.delenv("ISG_PW_KERNEL", raising=False)
    case = build("dgrad", 176, 80, (10, 10), "bnbwd2", "actbwd_prelu", seed=5)
    got = []
    for _ in range(2):
        la = Launch(case)
        assert la.run().startswith("pwp_kernel")
        o = la.out[0]
        got.append((o["slab"].flat.clone(), o["ST"].clone(), o["SG"].clone()))
    for a, b, what in zip(got[0], got[1], ("the gradient", "gsum / gxsum", "the slope gradient")):
        same_bits(a, b, what)


@pytest.mark.parametrize("kind", ["res_sink", "mat", "rbn"])
def test_pwp_refuses_residual_forms(kind, monkeypatch):
    """Residual term, materialised input, residual BatchNorm: the slab kernel's, refused here."""
    monkeypatch.setenv("ISG_PW_KERNEL", "pwp")
    fwd = kind != "res_sink"
    case = build("fwd" if fwd else "dgrad", 132, 48, (8, 8), "bnfwd" if fwd else "bnbwd2",
                 "store1" if fwd else "actbwd_prelu", seed=9)
    la = Launch(case)
    N, H, W = case["N"], case["H"], case["W"]
    extra = Slab(132 if fwd else 48, H, W, data=None, fill=0.5, N=N)
    if kind == "res_sink":
        la.sinks.s[0].r, la.sinks.s[0].r_n_stride = extra.ptr, extra.n_stride
    elif kind == "mat":
        la.src.mat, la.src.mat_n_stride = extra.ptr, extra.n_stride
    else:
        sg = case["src"][0]
        GA, BE, ST = dev(sg["gamma"]), dev(sg["beta"]), rep_from(torch.from_numpy(sg["stats"]))
        la.src.rbn = struct(L.Bn, bn_spec_train(GA, BE, ST, sg["count"]))
        la.src.s[0].y, la.src.s[0].y_n_stride = extra.ptr, extra.n_stride
    with pytest.raises(RuntimeError, match=rf"\({CC.UNSUPPORTED}\)"):
        la.run()
    torch.cuda.synchronize()
    for sl in [o["slab"] for o in la.out] + [extra]:
        sl.outside_untouched("a refused launch", whole=True)


@pytest.mark.parametrize("c", [("fwd", 256, 176, (16, 16), "bnfwd", "store2"),
                               ("fwd", 132, 80, (10, 10), "plain", "store1"),
                               ("dgrad", 176, 256, (16, 16), "bnbwd2", "actbwd_prelu"),
                               ("dgrad", 176, 48, (10, 10), "bnbwd2", "accum")], ids=_id)
def test_pwp_keeps_the_chunked_kernels_bits(c, monkeypatch):
    """pwp reduces K in ascending order, as pw_kernel does, with the same tile-to-wave map: a
    layer moved from one to the other keeps every output and statistic bit for bit."""
    case = build(*c, seed=31)
    got = {}
    for kern, name in (("pwp", "pwp_kernel"), ("pw", "pw_kernel")):
        monkeypatch.setenv("ISG_PW_KERNEL", kern)
        la = Launch(case)
        assert la.run().startswith(name)
        got[kern] = [(o["slab"].flat.clone(), o.get("ST"), o.get("SG")) for o in la.out]
    for a, b in zip(got["pwp"], got["pw"]):
        for x, y, what in zip(a, b, ("the output", "the statistics", "the slope gradient")):
            if x is not None:
                same_bits(x, y, what)
