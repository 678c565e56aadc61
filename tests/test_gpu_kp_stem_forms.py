"""The keypoint stem kernels (csrc/kp_stem.hip: kp_fwd_kernel, kp_wgrad_kernel, kp_pool_kernel)
straight through the C-ABI, against the fp64 expectations of tests/kp_stem_cases.py (proved on
the CPU by tests/test_kp_stem_cases_cpu.py), with the kernel that ran asserted by name.

One row per geometry (kp_stem_cases.ROWS: the production stem, then kernels, strides, pads and
dilations that differ per axis, 1 to 32 parts, Co off a multiple of 4, 49 taps) in every form:
  forward          base (y a channel slice of a wider buffer with a tail after every image, the
                   statistics spread over their replicas), nostats (stats NULL), off1 (the
                   allocation one float off), n1 (one image)
  weight gradient  plain, bn_train (dy rebuilt from BatchNorm backward, statistics in spread
                   replicas of a layer wider than the segment), coef (finalised coefficients),
                   nrep1 (one replica, no stride), n1
The bars are derived from the kernels' fp32 arithmetic (U = 2^-24, the unit roundoff), next to
each constant; none was fitted to what the kernels return. They are orders of magnitude tighter
than the whole-network bars the kernels had until now (tests/test_gpu_kp_stem.py: logits within
1e-4, the heatmap weight gradient within 2e-3 of its maximum, running statistics rtol 1e-4)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from instancesegmentation_amd import _lib as L
from tests import kp_stem_cases as KC
from tests.isg_helpers import POISON, Slab, bits, call, dev, ptr, rep_spread, same_bits, stream, struct
from tests.test_gpu_conv_forms import Run

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
_FAULT = []  # a GPU fault ends the module: nothing more is launched on a faulted device


def guarded(fn):
    @functools.wraps(fn)
    def run(*a, **kw):
        if _FAULT:
            pytest.fail(f"not run: an earlier case met a GPU fault ({_FAULT[0]})")
        try:
            fn(*a, **kw)
        except RuntimeError as e:
            if "(-3)" in str(e) or "HIP error" in str(e) or "hipError" in str(e):
                _FAULT.append(str(e)[:300])
            raise
    return run


def launched(name):
    got = L.lib().isg_last_launch().decode()
    assert got == name, f"ran {got}, not {name}"


def geom_of(row, N):
    return dict(N=N, Ci=row.Ci, H=row.H, W=row.W, Co=row.Co, OH=row.OH, OW=row.OW, KH=row.k[0], KW=row.k[1],
                SH=row.s[0], SW=row.s[1], PH=row.p[0], PW=row.p[1], DH=row.d[0], DW=row.d[1], groups=1)


def kp_spec(row, N, K, **kw):
    return dict({"kp": ptr(K), "nparts": row.parts, "c_kp0": row.c_kp0, "sigma": row.sigma,
                 "threshold": KC.THRESHOLD, "g": geom_of(row, N)}, **kw)


# ---- forward --------------------------------------------------------------------------------
def fwd_once(case, stats, off):
    """One isg_kp_stem_fwd on fresh operands: (y slab, statistics before, after)."""
    row, N = case["row"], case["N"]
    K, Wt = dev(case["kp"]), dev(case["w"])
    Y = Slab(row.Co, row.OH, row.OW, data=case["v"], fill=POISON, pad=3, c0=2, off=off, N=N, tail=5)
    ST = rep_spread(case["stats0"]) if stats else None
    before = ST.clone() if stats else None
    a = struct(L.KpStem, kp_spec(row, N, K, w=ptr(Wt), y=Y.ptr, y_n_stride=Y.n_stride, stats=ptr(ST)))
    call("isg_kp_stem_fwd", a, stream())
    launched("kp_fwd_kernel")
    return Y, before, ST


@pytest.mark.parametrize("rid,form", KC.FWD_CASES, ids=[f"{r}-{f}" for r, f in KC.FWD_CASES])
@guarded
def test_kp_fwd_form(rid, form):
    case = KC.make_case(rid, form)
    row, Co = case["row"], case["row"].Co
    stats, off = form != "fwd-nostats", 1 if form == "fwd-off1" else 0
    Y, before, ST = fwd_once(case, stats, off)
    Y.outside_untouched(f"{rid} {form}")
    y = Y.get().cpu()
    v = torch.from_numpy(np.array(case["v"]))
    v64, delta, mag = v.double(), torch.from_numpy(np.array(case["delta"])), torch.from_numpy(np.array(case["mag"]))
    # The kernel adds at most T = parts * KK products w * h into one fp32 accumulator, one after the
    # other, from 0 (parts whose window misses the tile are skipped; h is the oracle's own fp32
    # value). Each term passes through at most T roundings (its product, unless fused, and the
    # additions after it): |acc - delta| <= g_T * mag, g_T = T U / (1 - T U) <= (T + 1/2) U for
    # T <= 512. Then y = fl(v + acc): U * |v + acc| <= U * (|v| + (1 + g_T) mag). Together
    # (g_T + U (1 + g_T)) mag + U |v| <= (T + 2) U (mag + |v|).
    err = (y.double() - (v64 + delta)).abs()
    bound = (row.T + 2) * U * (mag + v64.abs())
    worst = float((err / bound).max())
    print(f"{rid} {form}: forward error / bound {worst:.3f} (max error {float(err.max()):.3e})")
    assert worst <= 1.0, f"{rid} {form}: forward error {worst:.3f} of the bound"
    # a pixel no window's value reaches keeps its bits (every pixel of an image that draws nothing)
    quiet = mag == 0
    assert quiet.any() and int((bits(y)[quiet.numpy()] != bits(v)[quiet.numpy()]).sum()) == 0, \
        "pixels outside every window changed"
    Y2, _, ST2 = fwd_once(case, stats, off)
    same_bits(Y2.get(), y, "y of a second run on the same inputs")
    if not stats:
        Yb, _, _ = fwd_once(case, True, off)
        same_bits(Yb.get(), y, "y with and without the statistics block")
        return
    # statistics: the kernel adds sum(nv - v) and sum((nv - v)(nv + v)) of one 16 x 16 tile, summed
    # in fp32 (256 terms: 255 additions, and up to 3 roundings in a term), to one replica in fp64.
    # Against the same sums in fp64 over the values it stored: (256 + 8) U sum|term| per channel.
    # (The fp64 atomics and the replica fold add about 2^-52 of the preloaded sums, |s| <= 50,
    # per tile: 1e-13 against bars that are 1e-5 of sum|term|.)
    B, A = before.view(L.STAT_REP, 4 * Co).cpu(), ST.view(L.STAT_REP, 4 * Co).cpu()
    assert not torch.isnan(A).any()
    same_bits(A[:, 2 * Co:], B[:, 2 * Co:], "the gsum / gxsum quarters of the statistics block")
    assert (B != 0).all(), "every replica starts non-zero"
    got = (A - B).sum(0)
    y64 = y.double()
    for name, g, term in (("sum", got[:Co], y64 - v64), ("sumsq", got[Co:2 * Co], y64 * y64 - v64 * v64)):
        want, tol = term.sum((0, 2, 3)), (256 + 8) * U * term.abs().sum((0, 2, 3))
        assert (tol > 0).all()
        w = float(((g - want).abs() / tol).max())
        print(f"{rid} {form}: {name} correction error / bound {w:.3f}")
        assert w <= 1.0, f"{rid} {form}: {name} correction off by {w:.3f} of the bound: {g - want}"
    # the replica a tile adds into is (tile + 7 * image) % ISG_STAT_REP: more than one changed
    assert int((bits(A[:, :2 * Co]) != bits(B[:, :2 * Co])).any(1).sum()) >= 2


# ---- weight gradient ------------------------------------------------------------------------
def preload(nrep, n):
    """Non-zero dyadic values in every word of every replica, gap included."""
    r = torch.arange(nrep, dtype=torch.float64)[:, None]
    i = torch.arange(n, dtype=torch.float64)[None, :]
    return (0.25 * (r + 1) + 0.125 * (i % 5)).to(DEV)


@pytest.mark.parametrize("rid,form", KC.WG_CASES, ids=[f"{r}-{f}" for r, f in KC.WG_CASES])
@guarded
def test_kp_wgrad_form(rid, form):
    """dw_after - dw_before on the heatmap channels within (P + 8) * 2^-24 * mag_w of the fp64
    weight gradient, entry by entry (the whole-network test asks 2e-3 of the maximum)."""
    case = KC.make_case(rid, form)
    row, N, Co, c0 = case["row"], case["N"], case["row"].Co, case["row"].c_kp0
    nw = Co * row.Ci * row.KK
    nrep = 1 if form == "wgrad-nrep1" else L.WREP
    stride = nw + 11  # the gap after the weight shows stray writes
    r = Run({"form": {"wgrad-bn_train": "replicas", "wgrad-coef": "coef"}.get(form, "slice"), "N": N})
    dy = r.vt([case["dy"]], row.OH, row.OW)
    K = dev(case["kp"])
    DW = preload(nrep, stride)
    before = DW.clone()
    a = struct(L.KpStem, kp_spec(row, N, K, dy=dy, dw=ptr(DW), rep_stride=0 if nrep == 1 else stride, nrep=nrep))
    call("isg_kp_stem_wgrad", a, stream())
    launched("kp_wgrad_kernel")
    r.finish(False)
    A, B = DW.cpu(), before.cpu()
    same_bits(A[:, nw:], B[:, nw:], "the gap between the replicas")
    Aw, Bw = A[:, :nw].view(nrep, Co, row.Ci, row.KK), B[:, :nw].view(nrep, Co, row.Ci, row.KK)
    same_bits(Aw[:, :, :c0], Bw[:, :, :c0], "the image channels' entries")
    # One workgroup sums dy * h over the output pixels of its band, at most P of them, in fp32
    # (four partial sums, then the chunks) before its fp64 atomic: g_P * sum|dy||h|. dy itself is
    # exact for a plain segment; BatchNorm backward rebuilds it as A*g + B*(y - mean) + C in fp32
    # from coefficients rounded to fp32: at most 7 U of |A||g| + |B||y - mean| + |C| (4 operations,
    # the rounding of A, B and C; the rounding of the mean is U |B||mean|, which the same sum over a
    # window covers, |y - mean| averaging about 1 and |mean| <= 1), and the product's rounding 1 U.
    # Together (P + 8) U mag_w with mag_w the same sums over absolute values. (The fp64 atomics
    # on preloaded values of at most 4.5 add about 1e-15 per workgroup.)
    got = (Aw - Bw).sum(0)[:, c0:].reshape(Co, row.parts, *row.k)
    want, mag_w = torch.from_numpy(np.array(case["dw"])), torch.from_numpy(np.array(case["mag_w"]))
    tol = (case["P"] + 8) * U * mag_w
    err = (got - want).abs()
    assert (err[mag_w == 0] == 0).all(), "entries no tap reaches a map for changed"
    worst = float((err[mag_w > 0] / tol[mag_w > 0]).max())
    print(f"{rid} {form}: weight gradient error / bound {worst:.4f} (P {case['P']}, max error {float(err.max()):.3e}, "
          f"max |dw| {float(want.abs().max()):.3e})")
    assert worst <= 1.0, f"{rid} {form}: weight gradient off by {worst:.3f} of the bound"
    # which replica a workgroup adds into: (image * parts + part + 7 * band) % nrep
    may, must = KC.replicas_of(case, nrep)
    changed = (bits(Aw[:, :, c0:]) != bits(Bw[:, :, c0:])).any((1, 3))  # [nrep, parts]
    assert not (changed & ~may).any(), f"replicas no workgroup of the part owns changed: {np.argwhere(changed & ~may)}"
    assert not (must & ~changed).any(), f"replicas a workgroup adds into kept their bits: {np.argwhere(must & ~changed)}"
    if nrep == 1:
        assert changed[0].any() and (changed[0] == must[0]).all()


# ---- pool -----------------------------------------------------------------------------------
def pool_once(row, kp, maps, k):
    N, n = kp.shape[0], row.parts
    PH, PW = row.H // k, row.W // k
    C, c0 = n + 5, 2
    out = torch.full((N, C, PH, PW), 7.0, device=DEV)  # poisoned
    K = dev(kp)
    a = struct(L.KpStem, {"kp": ptr(K), "nparts": n, "sigma": row.sigma, "threshold": KC.THRESHOLD,
                          "g": {"N": N, "H": row.H, "W": row.W}, "k": k,
                          "out": out.data_ptr() + 4 * c0 * PH * PW, "out_n_stride": C * PH * PW})
    call("isg_kp_pool", a, stream())
    launched("kp_pool_kernel")
    got = out.cpu().numpy()
    ref = maps.reshape(N, n, PH, k, PW, k).max(axis=(3, 5))
    assert ref.any()
    np.testing.assert_array_equal(got[:, c0:c0 + n].view(np.int32), ref.view(np.int32))
    assert np.all(got[:, :c0] == 7.0) and np.all(got[:, c0 + n:] == 7.0), "channels outside [c0, c0 + parts) written"


@pytest.mark.parametrize("rid", ["k3", "asym"])
@guarded
def test_kp_pool_k1_is_the_oracle_map(rid):
    """With k = 1 the pooled output is the heatmap itself: bit for bit the oracle's."""
    pool_once(KC.ROW[rid], KC.keypoints(rid), KC.row_maps(rid), 1)


@pytest.mark.parametrize("k", [2, 8])
@guarded
def test_kp_pool_windows(k):
    """k = 2 and k = 8 on the 48 x 64 row's keypoints (32 parts, sigma 3): the reshaped maximum."""
    row = KC.ROW["p32"]
    assert (row.H, row.W) == (48, 64)
    pool_once(row, KC.keypoints("p32"), KC.row_maps("p32"), k)


# ---- refusals -------------------------------------------------------------------------------
@guarded
def test_kp_refusals_leave_every_output_alone():
    """Each refusal of include/isg.h's isg_kp_stem paragraph: its code, a message, no launch,
    and y, stats, dw and out bit for bit what they were. (tests/test_kp_stem_cases_cpu.py shows
    on the CPU, where a launch cannot succeed, that each returns on the host.)"""
    lib = L.lib()
    g = KC.REF_GEOM
    Co, hw = g["Co"], g["OH"] * g["OW"]
    pat = lambda n, dt: (torch.arange(n, device=DEV) % 13 + 1).to(dt)
    bufs = {"kp": torch.zeros(g["N"] * 33 * 3, dtype=torch.float64, device=DEV),
            "w": pat(17 * g["Ci"] * 64, torch.float32), "p": pat(g["N"] * 17 * hw, torch.float32),
            "y": pat(g["N"] * 17 * hw, torch.float32), "stats": pat(L.STAT_REP * 4 * 17, torch.float64),
            "dw": pat(L.WREP * (17 * g["Ci"] * 64 + 7), torch.float64),
            "out": pat(g["N"] * 33 * g["H"] * g["W"], torch.float32)}
    held = {k: t.clone() for k, t in bufs.items()}
    ptrs = {k: t.data_ptr() for k, t in bufs.items()}
    fn = {"fwd": lib.isg_kp_stem_fwd, "wgrad": lib.isg_kp_stem_wgrad, "pool": lib.isg_kp_pool}
    call("isg_fill_f64", ptrs["kp"], 8, 0.0, stream())
    mark = lib.isg_last_launch()
    for what, entries, over, code in KC.REFUSED:
        for e in entries:
            a = struct(L.KpStem, KC.refusal_spec(over, ptrs, L.WREP))
            rc = fn[e](ctypes.byref(a), stream())
            assert rc == code, (what, e, rc, lib.isg_last_error())
            assert lib.isg_last_error(), (what, e)
            assert lib.isg_last_launch() == mark, f"{what} ({e}) reached a launch"
    torch.cuda.synchronize()
    for k, t in bufs.items():
        same_bits(t, held[k], f"{k} after the refused calls")
