"""The cases of tests/conv_cases.py, proved on the CPU: every fp64 expectation the GPU tests
compare against agrees with torch autograd, the finalised-coefficient references agree with
the statistics they were rounded from, no activation boundary is near a tie, and every row
stays small."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import conv_cases as CC

IDS = [f"{r}-{f}" for r, f in CC.CASES]
T = torch.from_numpy


def rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))


def test_table_covers_the_launch_names():
    names = {r.launch for r in CC.ROWS}
    for n in ("pw_kernel", "pwx_kernel", "thin_pw_kernel", "thin_conv_kernel", "thin_conv3_x4_kernel",
              "down_conv_kernel", "s2k5_fwd_kernel", "tap_conv_kernel", "halo_conv_kernel",
              "gemm_conv_kernel", "dw_tile_kernel<fwd>", "dw_kernel<fwd>", "sub2_dgrad_kernel",
              "dw_tile_kernel<dgrad>", "pwg_kernel", "wgrad_kernel", "tap_wgrad_kernel",
              "tap_wgrad_all_kernel", "thin_wgrad3_x4_kernel", "down_wgrad_kernel", "s2k5_wgrad_kernel",
              "dw_wgrad_tile_kernel", "dw_wgrad_kernel", "dw_bwd_tile_kernel"):
        assert n in names, n
    by = {(r.dirn, r.launch, r.s) for r in CC.ROWS}
    assert ("fwd", "tap_conv_kernel", 1) in by and ("fwd", "tap_conv_kernel", 2) in by
    for n in ("pw_kernel", "pwx_kernel", "thin_pw_kernel", "thin_conv_kernel", "tap_conv_kernel",
              "gemm_conv_kernel"):
        assert any(r.dirn == "dgrad" and r.launch == n for r in CC.ROWS), n
    assert len({r.id for r in CC.ROWS}) == len(CC.ROWS)


@pytest.mark.parametrize("row", CC.ROWS, ids=[r.id for r in CC.ROWS])
def test_rows_stay_small(row):
    assert 3 * max(row.Ci, row.Co) * row.H * row.W <= CC.SIZE_CAP
    assert row.OH >= 1 and row.OW >= 1


def test_splits_avoid_vector_boundaries():
    for C in range(1, 130):
        for parts in (CC.split_sinks(C), CC.split_segs(C)):
            assert sum(parts) == C and all(p > 0 for p in parts) and len(parts) == min(C, 3)
            edges = np.cumsum(parts)[:-1]
            assert all(e % 4 for e in edges), (C, parts)


def _kw(row):
    return dict(stride=row.s, padding=row.p, dilation=row.d, groups=row.groups)


@pytest.mark.parametrize("rid,form", CC.CASES, ids=IDS)
def test_references_agree_with_autograd(rid, form):
    case = CC.make_case(rid, form)
    row, N = case["row"], case["N"]
    w = T(case["w"].astype(np.float64)).requires_grad_()
    if row.dirn == "fwd":
        out = F.conv2d(CC.cat_v(case["src"]), w, None, **_kw(row))
        assert rel(out.detach(), case["v"]) <= 1e-12
        for sk in case["sinks"]:
            v = out.detach()[:, sk["c0"]:sk["c0"] + sk["C"]]
            if sk["mode"] == "store":
                want = v + T(sk["bias"].astype(np.float64))[None, :, None, None]
                assert rel(sk["out"], want) <= 1e-12
                assert rel(sk["sum"], want.sum((0, 2, 3))) <= 1e-12
                assert rel(sk["sumsq"], (want * want).sum((0, 2, 3))) <= 1e-12
            elif sk["mode"] == "accum":
                assert rel(sk["out"], T(sk["old"].astype(np.float64)) + v) <= 1e-12
        return
    if row.dirn == "dgrad" or row.dirn == "dwbwd":
        # the conv's input as act(z) on the ACTBWD sink's rows, a free leaf elsewhere: one
        # backward gives the input gradient, g = dL/dz and the PReLU slope gradient
        dy = CC.cat_v(case["src"] if row.dirn == "dgrad" else case["dy"])
        u = torch.zeros(N, row.Ci, row.H, row.W, dtype=torch.float64, requires_grad=True)
        sk = case["sinks"][-1]
        assert sk["mode"] == "actbwd" and sk["c0"] + sk["C"] == row.Ci
        z = T(sk["z"]).requires_grad_()
        slope = T(sk["slope"][:sk["C"]].astype(np.float64)).requires_grad_()
        F.conv2d(torch.cat([u[:, :sk["c0"]], F.prelu(z, slope)], 1), w, None, **_kw(row)).backward(dy)
        if sk["c0"]:
            assert rel(case["v"][:, :sk["c0"]], u.grad[:, :sk["c0"]]) <= 1e-12
        assert rel(sk["out"], z.grad) <= 1e-12
        assert rel(sk["slope_grad"], slope.grad) <= 1e-10  # sums of either sign: cancellation
        mean = sk["mean"][:sk["C"]] if sk["bn"] != "coef" else sk["coef_fwd"][:sk["C"], 0].astype(np.float64)
        yc = sk["y"].astype(np.float64) - mean[None, :, None, None]
        assert rel(sk["gsum"], z.grad.sum((0, 2, 3))) <= 1e-12
        assert rel(sk["gxsum"], (z.grad * T(yc)).sum((0, 2, 3))) <= 1e-9
        for a in case["sinks"][:-1]:
            if a["mode"] == "accum":
                want = T(a["old"].astype(np.float64)) + u.grad[:, a["c0"]:a["c0"] + a["C"]]
                assert rel(a["out"], want) <= 1e-12
        if row.dirn == "dgrad":
            return
    x = CC.cat_v(case["x"])
    dy = CC.cat_v(case["dy"])
    w.grad = None
    F.conv2d(x, w, None, **_kw(row)).backward(dy)
    assert rel(case["dw"], w.grad) <= 1e-12
    assert rel(case["dbias"], dy.sum((0, 2, 3))) <= 1e-12


def _train_value(sg):
    """A segment's value from its statistics block in fp64 (isg.h isg_bn, train)."""
    C, bnC, M = sg["C"], sg["bnC"], sg["count"]
    st = sg["stats"]
    mean = st[:bnC] / M
    rstd = 1.0 / np.sqrt(st[bnC:2 * bnC] / M - mean * mean + CC.EPS)
    gam = sg["gamma"].astype(np.float64)
    b = lambda a: a[None, :C, None, None]
    p = sg["p"].astype(np.float64) if "p" in sg else None
    if sg.get("xf") == "bn_bwd":
        y = sg["y"].astype(np.float64)
        xhat = (y - b(mean)) * b(rstd)
        return b(gam * rstd) * (p - b(st[2 * bnC:3 * bnC]) / M - xhat * b(rstd * st[3 * bnC:]) / M)
    raw = p if p is not None else sg["y"].astype(np.float64)
    return (raw - b(mean)) * b(gam * rstd) + b(sg["beta"].astype(np.float64))


@pytest.mark.parametrize("rid,form", [c for c in CC.CASES if c[1] == "coef"],
                         ids=[i for i, c in zip(IDS, CC.CASES) if c[1] == "coef"])
def test_coef_reference_agrees_with_the_statistics(rid, form):
    case = CC.make_case(rid, form)
    seen = 0
    for key in ("src", "x", "dy"):
        for sg in case.get(key, []):
            if sg["xf"] == "plain":
                continue
            assert sg["bn"] == "coef" and sg["bnC"] > sg["C"]
            want = _train_value(sg)
            got = sg["z"] if sg["xf"] == "bn_fwd" else sg["v"]
            assert rel(got, want) <= 1e-6
            assert CC.coef_of(sg).shape == (8 * sg["bnC"],)
            seen += 1
    for sk in case.get("sinks", []):
        if sk["mode"] == "actbwd":
            assert sk["bn"] == "coef" and sk["bnC"] == sk["C"]  # isg.h isg_sink: bn.C == C
            assert rel(sk["z"], _train_value(sk)) <= 1e-6
            seen += 1
    assert seen


@pytest.mark.parametrize("rid,form", CC.CASES, ids=IDS)
def test_inputs_are_tie_free(rid, form):
    case = CC.make_case(rid, form)
    for what, z in CC.ties(case):
        a = np.abs(z)
        assert a.min() > CC.TIE_MARGIN * a.max(), (what, a.min(), a.max())
    assert CC.ties(case), "every case has an activation boundary and lists it"


def test_last_launch_is_empty_before_any_launch_of_a_thread():
    import threading

    from instancesegmentation_amd import _lib as L
    assert "isg_last_launch" in L.SIGNATURES
    got = []
    t = threading.Thread(target=lambda: got.append(L.lib().isg_last_launch()))
    t.start()
    t.join()
    assert got == [b""]


def test_forms_present_what_they_claim():
    c = CC.make_case("fwd-tap_s1", "sinks3")
    assert [s["xf"] for s in c["src"]] == ["plain", "bn_fwd", "bn_fwd"]
    assert [s["act"] for s in c["src"]] == ["none", "prelu", "relu"]
    assert len({s["C"] for s in c["src"]}) == 3
    assert [s["mode"] for s in c["sinks"]] == ["none", "accum", "store"]
    c = CC.make_case("dgrad-tap", "sinks3")
    assert [s["xf"] for s in c["src"]] == ["bn_bwd", "plain", "bn_fwd"]
    assert [s["mode"] for s in c["sinks"]] == ["none", "accum", "actbwd"]
    c = CC.make_case("wgrad-tap", "segs3")
    assert len(c["x"]) == 3 and len(c["dy"]) == 2
    assert CC.make_case("fwd-tap_s1", "n1")["N"] == 1 and CC.make_case("fwd-tap_s1", "base")["N"] == 3
    c = CC.make_case("dgrad-tap", "replicas")
    assert c["src"][0]["bn"] == "train" and c["sinks"][0]["bn"] == "train"
