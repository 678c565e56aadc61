"""The cases of tests/head_cases.py, proved on the CPU: every fp64 expectation the GPU test
compares against agrees with torch autograd through an unfused ConvTranspose2d -> Conv2d on
the same transformed input, the loop shapes make the backward's persistent workgroups loop the
way the table claims, the border patterns put the ring term of dW2 where an error in it
cannot hide, and the host guards of isg_mask_head_* refuse what they document — without a
device (the pointers are never dereferenced)."""
import numpy as np
import pytest
import torch

from instancesegmentation_amd import _lib as L
from tests import head_cases as HC
from tests.isg_helpers import struct

P = 0x1000  # any non-NULL, 16-B aligned value: nothing may dereference it
SMALL_CASES = [c for c in HC.gpu_cases() if c[0] in HC.SMALL]
IDS = ["-".join(c) for c in SMALL_CASES]


def rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))


def test_loop_shapes_loop():
    """The kernel's own arithmetic: ceil(4Wi/64) * ceil(4Hi/32) * N tiles, one workgroup per two
    tiles and at most 256 (head_bwd_blocks, through its Python mirror)."""
    for sid, nt in (("loop_even", 522), ("loop_odd", 513), ("loop_odd_scalar", 513)):
        N, Hi, Wi = HC.SHAPES[sid]
        tiles = -(-4 * Wi // 64) * -(-4 * Hi // 32) * N
        groups = L.head_part_floats(N, Hi, Wi) // 4096
        assert (tiles, groups) == (nt, 256) == HC.tiles(sid)
        assert L.lib().isg_mask_head_part_floats(N, Hi, Wi) == 256 * 4096
        # workgroup g's half h runs tiles 2g + h, 2g + h + 512, ...: the second iteration
        second = [((t - 512) // 2, t % 2) for t in range(512, tiles)]
        if sid == "loop_even":  # workgroups 0-4, both halves
            assert second == [(g, h) for g in range(5) for h in (0, 1)]
        else:                   # workgroup 0's half 0 only: its half 1 sits the iteration out
            assert second == [(0, 0)]
    assert HC.SHAPES["loop_even"][2] % 4 == 0 and HC.SHAPES["loop_odd"][2] % 4 == 0
    assert HC.SHAPES["loop_odd_scalar"][2] % 4 and 4 * HC.SHAPES["loop_odd_scalar"][1] % 32
    for sid in HC.SMALL:
        assert HC.tiles(sid)[1] < 256 and HC.tiles(sid)[0] <= 2 * HC.tiles(sid)[1]
    N, Hi, Wi = HC.SHAPES["vec_partial"]
    assert Wi % 4 == 0 and (4 * Hi) % 32 and (4 * Wi) % 64 and HC.tiles("vec_partial")[0] == 9 * N
    assert HC.tiles("one_tile") == (1, 1)


def test_shapes_stay_small():
    """About a million input elements at most (the loop shapes need 513 tiles of 8 x 16 pixels)."""
    for sid, (N, Hi, Wi) in HC.SHAPES.items():
        assert N * HC.CI * Hi * Wi <= (1 << 20) * (1.02 if sid in HC.LOOP else 1.0), sid


def test_forms_present_what_they_claim():
    c = HC.head_case("ragged", "segs3")
    assert [(s["kind"], s["act"], s["C"]) for s in c["segs"]] == list(HC.SEGS3)
    assert sum(C for _, C in HC.SINKS3) == 16 and [m for m, _ in HC.SINKS3] == ["none", "accum", "store"]
    assert np.cumsum([C for _, C in HC.SINKS3])[0] != np.cumsum([s[2] for s in HC.SEGS3])[0]
    c = HC.head_case("ragged", "coef")
    (sg,) = c["segs"]
    assert sg["bnC"] == 19 > 16 and sg["coef"].shape == (8 * 19,) and np.isnan(sg["coef"][4 * 19:]).all()
    assert HC.head_case("ragged", "act_only")["segs"][0]["kind"] == "act_only"
    assert HC.head_case("ragged", "nobias")["b1"] is None and HC.head_case("ragged", "nobias")["b2"] is None
    for f in ("slice", "off4", "replicas", "skip"):  # the same inputs: the same bits are owed
        assert HC.head_case("vec_partial", f) is HC.head_case("vec_partial", "base")
    for form in ("segs3", "coef"):
        for sg in HC.head_case("one_tile", form)["segs"]:
            if sg["kind"] not in ("plain", "act_only"):
                assert np.abs(sg["beta"]).min() >= 0.5


@pytest.mark.parametrize("sid,pattern,form", SMALL_CASES, ids=IDS)
def test_references_agree_with_autograd(sid, pattern, form):
    case, ref = HC.head_case(sid, form, pattern), HC.head_ref(sid, form, pattern)
    N, Hi, Wi = HC.SHAPES[sid]
    T = lambda a: torch.from_numpy(a.astype(np.float64))
    ct = torch.nn.ConvTranspose2d(16, 4, 8, 4, 2, bias=case["b1"] is not None).double()
    cv = torch.nn.Conv2d(4, 1, 3, 1, 1, bias=case["b2"] is not None).double()
    with torch.no_grad():
        ct.weight.copy_(T(case["w1"]))
        cv.weight.copy_(T(case["w2"]))
        if case["b1"] is not None:
            ct.bias.copy_(T(case["b1"]))
            cv.bias.copy_(T(case["b2"]))
    v = ref["v"].clone().requires_grad_(True)
    y = cv(ct(v))
    y.backward(T(case["dl"]))
    assert rel(ref["logits"], y.detach()) <= 1e-12
    assert rel(ref["dx"], v.grad) <= 1e-12 and rel(ref["dw1"], ct.weight.grad) <= 1e-12
    assert (np.abs(ref["dw2"].numpy() - cv.weight.grad.numpy()) <= 1e-12 * ref["dw2_scale"].numpy()).all()
    if case["b1"] is not None:
        assert (np.abs(ref["db1"].numpy() - ct.bias.grad.numpy()) <= 1e-12 * ref["db1_scale"].numpy()).all()
        assert (np.abs(ref["db2"].numpy() - cv.bias.grad.numpy()) <= 1e-12 * ref["db2_scale"].numpy()).all()
    # the transformed input by the documented formula, from the segment's own description
    for sg in case["segs"]:
        x = sg["x"].astype(np.float64)
        got = ref["v"][:, sg["c0"]:sg["c0"] + sg["C"]].numpy()
        if sg["kind"] == "plain":
            assert np.array_equal(got, x)
            continue
        if sg["kind"] == "act_only":
            pre = x
        else:
            C, bnC, M = sg["C"], sg["bnC"], sg["count"]
            if sg["kind"] == "bn_eval":
                mean, var = sg["rm"].astype(np.float64), sg["rv"].astype(np.float64)
            else:
                mean = sg["stats"][:bnC] / M
                var = sg["stats"][bnC:2 * bnC] / M - mean * mean
            scale = sg["gamma"].astype(np.float64) / np.sqrt(var + float(np.float32(1e-5)))
            b = lambda a: a[None, :C, None, None]
            pre = (x - b(mean)) * b(scale) + b(sg["beta"].astype(np.float64))
        sl = sg["slope"].astype(np.float64)[None, :, None, None]
        want = np.maximum(pre, 0.0) if sg["act"] == "relu" else np.where(pre > 0, pre, pre * sl)
        assert rel(got, want) <= (1e-6 if sg["kind"] == "coef" else 1e-12)  # coef: rounded to fp32 once
    # scales are what they say: at least the value they bound
    assert (ref["dw2_scale"].numpy() >= np.abs(ref["dw2"].numpy()) * (1 - 1e-12)).all()
    assert ref["ring"].shape == (N, 4, 2 * (4 * Wi + 2) + 2 * 4 * Hi)
    assert L.head_ring_floats(Hi, Wi) == 4 * ref["ring"].shape[2]


@pytest.mark.parametrize("sid", HC.SMALL)
@pytest.mark.parametrize("pattern", ["border", "corners"])
def test_border_patterns_concentrate_the_ring_term(sid, pattern):
    """The pairs (p, tap) whose intermediate pixel lies outside the image — what the kernel's
    ring correction removes — are at least a quarter of |dW2| for some tap of every channel;
    with dense dlogits they are a perimeter / area share, which a 2e-5 bar cannot see."""
    for form in ("base", "segs3", "coef"):
        ref = HC.head_ref(sid, form, pattern)
        share = (ref["ring_term"].abs() / ref["dw2"].abs().clamp_min(1e-300)).reshape(4, 9)
        assert (share.max(1).values >= 0.25).all(), (form, share.max(1).values)
        dl = HC.head_case(sid, form, pattern)["dl"]
        inner = dl[:, :, 1:-1, 1:-1]
        assert not inner.any() and dl.any()
        if pattern == "corners":
            assert np.count_nonzero(dl) == 4 * dl.shape[0]
    dense = HC.head_ref("vec_partial", "base", "dense")
    assert (dense["ring_term"].abs() / dense["dw2_scale"]).max() < 0.25


# ---- host guards ---------------------------------------------------------------------------
def _head(**kw):
    """A mask-head record the launchers accept (1 x 16 x 8 x 12), with the overrides of kw."""
    N, Hi, Wi = 1, 8, 12
    seg = {"p": P, "n_stride": 16 * Hi * Wi, "C": 16, "xform": L.XF_PLAIN}
    sk = {"p": P, "n_stride": 16 * Hi * Wi, "c0": 0, "C": 16, "mode": L.SINK_STORE}
    spec = {"x": {"s": [seg], "nseg": 1, "N": N, "H": Hi, "W": Wi}, "w1": P, "b1": P, "w2": P, "b2": P,
            "N": N, "Hi": Hi, "Wi": Wi, "ring": P, "out": P, "out_n_stride": 16 * Hi * Wi, "dout": P,
            "dout_n_stride": 16 * Hi * Wi, "dx": {"s": [sk], "nsink": 1}, "dw1": P, "db1": P, "dw2": P,
            "db2": P, "rep_stride": 4137, "nrep": L.WREP}
    spec.update(kw)
    return struct(L.MaskHead, spec)


def _sk(c0, C, mode=L.SINK_STORE, **kw):
    return dict({"p": P, "n_stride": 16 * 8 * 12, "c0": c0, "C": C, "mode": mode}, **kw)


def _xs(*Cs, N=1):
    segs = [{"p": P, "n_stride": 16 * 8 * 12, "C": C, "xform": L.XF_PLAIN} for C in Cs]
    return {"s": segs, "nseg": len(segs), "N": N, "H": 8, "W": 12}


UNSUP, INVALID = -2, -1
REFUSED = [
    # (what, entry points, record overrides, error code)
    ("a segment without channels", ("fwd", "bwd"), dict(x=_xs(16, 0)), UNSUP),
    ("a segment with negative channels", ("fwd", "bwd"), dict(x=_xs(20, -4)), UNSUP),
    ("x.N != N", ("fwd", "bwd"), dict(x=_xs(16, N=2)), UNSUP),
    ("15 channels", ("fwd", "bwd"), dict(x=_xs(10, 5)), UNSUP),
    ("nseg above ISG_MAX_SEGS", ("fwd", "bwd"), dict(x=dict(_xs(6, 5, 5), nseg=4)), UNSUP),
    ("nsink above ISG_MAX_SEGS", ("bwd",), dict(dx={"s": [_sk(0, 6), _sk(6, 5), _sk(11, 5)], "nsink": 4}), UNSUP),
    ("negative nsink", ("bwd",), dict(dx={"s": [_sk(0, 16)], "nsink": -1}), UNSUP),
    ("two sinks that cover ten channels", ("bwd",), dict(dx={"s": [_sk(0, 4), _sk(4, 6)], "nsink": 2}), UNSUP),
    ("sinks that leave a gap", ("bwd",), dict(dx={"s": [_sk(0, 4), _sk(6, 10)], "nsink": 2}), UNSUP),
    ("sinks out of order", ("bwd",), dict(dx={"s": [_sk(8, 8), _sk(0, 8)], "nsink": 2}), UNSUP),
    ("sinks not starting at 0", ("bwd",), dict(dx={"s": [_sk(2, 14)], "nsink": 1}), UNSUP),
    ("sinks past 16", ("bwd",), dict(dx={"s": [_sk(0, 8), _sk(8, 12)], "nsink": 2}), UNSUP),
    ("an empty sink", ("bwd",), dict(dx={"s": [_sk(0, 16), _sk(16, 0)], "nsink": 2}), UNSUP),
    ("a sink bias", ("bwd",), dict(dx={"s": [_sk(0, 16, bias=P)], "nsink": 1}), UNSUP),
    ("a NONE sink's bias", ("bwd",), dict(dx={"s": [_sk(0, 16, L.SINK_NONE, bias=P)], "nsink": 1}), UNSUP),
    ("an ACTBWD sink", ("bwd",), dict(dx={"s": [_sk(0, 16, L.SINK_ACTBWD)], "nsink": 1}), UNSUP),
    ("sink statistics", ("bwd",), dict(dx={"s": [_sk(0, 16, stats=P)], "nsink": 1}), UNSUP),
    ("a STORE sink without a buffer", ("bwd",), dict(dx={"s": [_sk(0, 16, p=None)], "nsink": 1}), UNSUP),
    ("NULL ring", ("bwd",), dict(ring=None), INVALID),
    ("NULL dlogits", ("bwd",), dict(dout=None), INVALID),
    ("NULL output", ("fwd",), dict(out=None), INVALID),
    ("no replicas", ("bwd",), dict(nrep=0), INVALID),
    ("replicas without a stride", ("bwd",), dict(rep_stride=0), INVALID),
    ("fold without a slab", ("fold",), dict(), INVALID),
    ("fold without dw1", ("fold",), dict(dw1=None, dw1_part=P), INVALID),
]


@pytest.mark.parametrize("what,entries,kw,code", REFUSED, ids=[r[0].replace(" ", "_") for r in REFUSED])
def test_head_guards_refuse_before_any_launch(what, entries, kw, code):
    lib = L.lib()
    before = lib.isg_last_launch()
    for e in entries:
        rc = getattr(lib, "isg_mask_head_" + e)(_head(**kw), None)
        assert rc == code, (what, e, rc, lib.isg_last_error())
        assert lib.isg_last_error()
    assert lib.isg_last_launch() == before, "a refused call reached a launch"
