"""The cases of tests/kp_stem_cases.py, proved on the CPU: the fp64 expectations agree with
torch autograd over cat(image, heatmaps), no heatmap pixel is near the threshold step, every
row's keypoints reach what the row is there for, every row fits the launchers' caps, and every
documented refusal returns on the host before a launch."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from instancesegmentation_amd import _lib as L
from tests import kp_stem_cases as KC
from tests.isg_helpers import struct

RIDS = [r.id for r in KC.ROWS]
T = lambda a: torch.from_numpy(np.array(a))  # a copy: the cases are read-only


def rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))


def test_table_is_the_issues():
    assert RIDS == ["stem", "k3", "k1s3", "asym", "k7", "p32", "chunks"]
    assert [(r.Co, r.c_kp0, r.parts, r.k, r.s, r.p, r.d, r.sigma) for r in KC.ROWS] == [
        (16, 3, 17, (5, 5), (2, 2), (2, 2), (1, 1), 10.0), (5, 0, 1, (3, 3), (1, 1), (1, 1), (1, 1), 3.0),
        (16, 2, 4, (1, 1), (3, 3), (0, 0), (1, 1), 3.0), (7, 1, 6, (3, 5), (1, 2), (1, 2), (2, 1), 4.0),
        (10, 0, 10, (7, 7), (1, 1), (3, 3), (1, 1), 3.0), (16, 3, 32, (3, 3), (2, 2), (1, 1), (1, 1), 3.0),
        (8, 2, 3, (3, 3), (1, 1), (1, 1), (1, 1), 10.0)]
    # the two rows moved from the issue's sizes say why
    assert all(KC.ROW[r].note for r in ("k1s3", "chunks", "k3"))
    assert (KC.ROW["stem"].OH, KC.ROW["stem"].OW) == (36, 44)
    a = KC.ROW["asym"]
    assert len({a.H, a.W}) == 2 and all(len(set(t)) == 2 for t in (a.k, a.s, a.p, a.d))


@pytest.mark.parametrize("rid", RIDS)
def test_row_caps(rid):
    row = KC.ROW[rid]
    assert 16 * row.parts * row.KK <= 8192  # forward: the active parts' weights in LDS
    assert row.Co * row.KK <= 512           # weight gradient: two accumulator slots of 256 threads
    assert all(f <= 64 for f in row.foot)
    assert 1 <= row.Co <= 16 and 1 <= row.parts <= 32 and row.KK <= 49 and row.r <= 120.0
    assert 3 * max(row.Ci, row.Co) * row.H * row.W <= 1 << 20
    if rid == "k7":
        assert row.KK == 49 and row.Co * row.KK > 256 and 16 * row.parts * row.KK == 7840
    if rid == "k3":
        assert row.KK % 5 == 4 and row.Co % 4


@pytest.mark.parametrize("rid", RIDS)
def test_autograd_agreement(rid):
    """delta and dw are what autograd gives for conv2d(cat(image, heatmaps), w), restricted to
    the heatmap channels."""
    row = KC.ROW[rid]
    rng = np.random.default_rng(5)
    for form in ("fwd-base", "fwd-n1"):
        c = KC.make_case(rid, form)
        maps = T(c["maps"].astype(np.float64))
        img = T(rng.normal(0.0, 1.0, (c["N"], row.c_kp0, row.H, row.W)))
        w = T(c["w"].astype(np.float64))
        full = F.conv2d(torch.cat([img, maps], 1), w, None, **KC.conv_kw(row))
        dense = F.conv2d(torch.cat([img, torch.zeros_like(maps)], 1), w, None, **KC.conv_kw(row))
        scale = max(np.abs(c["delta"]).max(), 1e-30)
        assert float((full - dense - T(c["delta"])).abs().max()) <= 1e-12 * max(scale, float(full.abs().max()))
        assert np.all(c["mag"] >= np.abs(c["delta"]) - 1e-15) and c["mag"].max() > 0
        assert c["delta"].shape == (c["N"], row.Co, row.OH, row.OW) and not (c["v"] == 0).any()
    for form in KC.WG_FORMS:
        c = KC.make_case(rid, form)
        maps = T(c["maps"].astype(np.float64))
        img = T(rng.normal(0.0, 1.0, (c["N"], row.c_kp0, row.H, row.W)))
        w = torch.zeros(row.Co, row.Ci, *row.k, dtype=torch.float64, requires_grad=True)
        F.conv2d(torch.cat([img, maps], 1), w, None, **KC.conv_kw(row)).backward(T(c["dy"]["v"]))
        assert rel(c["dw"], w.grad[:, row.c_kp0:]) <= 1e-12
        assert np.all(c["mag_w"] >= np.abs(c["dw"]) * (1 - 1e-12))
        assert np.all(KC.abs_dy(c["dy"]) >= np.abs(c["dy"]["v"]) * (1 - 1e-12))


def test_forms_present_what_they_claim():
    for rid in RIDS:
        base, nost, off1, n1 = (KC.make_case(rid, f) for f in KC.FWD_FORMS)
        assert base["w"] is nost["w"] is off1["w"] and base["v"] is off1["v"]  # one data kind
        assert base["N"] == 3 and n1["N"] == 1 and n1["kp"].shape[0] == 1
        plain, bnt, coef, nrep1, wn1 = (KC.make_case(rid, f) for f in KC.WG_FORMS)
        assert plain["dy"] is nrep1["dy"] and plain["dy"]["xf"] == "plain"
        Co = KC.ROW[rid].Co
        assert bnt["dy"]["xf"] == "bn_bwd" and bnt["dy"]["bn"] == "train" and bnt["dy"]["bnC"] == Co + KC.WIDE
        assert coef["dy"]["bn"] == "coef" and coef["dy"]["bnC"] == Co + KC.WIDE and "coef_bwd" in coef["dy"]
        assert wn1["N"] == 1
        assert not base["kp"].flags.writeable and not base["delta"].flags.writeable


@pytest.mark.parametrize("rid", RIDS)
def test_keypoint_kinds(rid):
    """The keypoints the issue lists, as far as the row's part slots go."""
    row, kp = KC.ROW[rid], KC.keypoints(rid)
    assert kp.shape == (3, row.parts, 3)
    assert not any(KC.drawn(q) for q in kp[1]), "image 1 draws nothing"
    assert not KC.row_maps(rid)[1].any()
    assert any(KC.drawn(q) for q in kp[0]) and any(KC.drawn(q) for q in kp[2])
    assert kp[1, 0, 2] == 0.0  # a part that is not visible
    if row.parts >= 2:
        assert tuple(kp[0, 1, :2]) == KC.corner(row) and KC.drawn(kp[0, 1])
        assert np.isnan(kp[1, 1, 0]) and kp[1, 1, 2] > 0
        wins = [w for n, _, w, _ in KC.windows(row, kp) if n in (0, 2)]
        assert any(w[1] <= w[0] or w[3] <= w[2] for w in wins), "a window wholly outside"
    if row.parts >= 3:
        assert kp[1, 2, 1] == -1e300 and kp[1, 2, 2] > 0
    if row.parts >= 5:
        assert np.isinf(kp[1, 3, 0]) and kp[1, 4, 0] == 1e300
    x0, x1, y0, y1 = KC.window(row, kp[2, 0])
    assert (x0, y0) == (0, 0) and 1 <= x1 <= 2 and 1 <= y1 <= 2  # about (-r + 1.5, -r + 1.5)


@pytest.mark.parametrize("rid", RIDS)
def test_threshold_ties(rid):
    """The threshold is a 0.01-high step: no window pixel's e is within 1e-9 of it, so a
    last-bit difference between two exp implementations cannot flip a pixel."""
    d = KC.tie_distance(KC.ROW[rid], KC.keypoints(rid))
    assert d > KC.TIE_MARGIN, d
    # and the oracle keeps exactly the pixels above it
    m = KC.row_maps(rid)
    assert m.max() <= 1.0 and (m[m > 0] > KC.THRESHOLD).all()


@pytest.mark.parametrize("rid", RIDS)
def test_coverage(rid):
    row, kp = KC.ROW[rid], KC.keypoints(rid)
    hits = KC.tile_hits(row, kp)
    assert (hits == 0).any(), "a tile no window reaches"
    if rid != "k1s3":  # (two tiles, and both the origin and the one-row window are in image 2)
        assert any((hits[n] == 0).any() for n in range(3) if hits[n].any()), "... in an image that has windows"
    if row.parts >= 2:  # (k3 has one part: ROWS note)
        assert (hits >= 2).any(), "a tile two windows reach"
    else:
        assert rid == "k3"
    assert row.OH % KC.TILE or row.OW % KC.TILE, "a partial tile"
    wins = KC.windows(row, kp)
    assert any((int(kp[n, j, 0] + row.r + 1) > row.W - 1 or int(kp[n, j, 1] + row.r + 1) > row.H - 1)
               and w[1] > w[0] and w[3] > w[2] for n, j, w, _ in wins), "a window clipped by W-1 or H-1"
    assert any((raw[0] < 0 and w[0] == 0) or (raw[1] < 0 and w[2] == 0) for _, _, w, raw in wins), \
        "a window that starts at 0 after a negative int(k - r)"
    # the mag == 0 pixels are exactly the pixels no window's value reaches: some exist
    c = KC.make_case(rid, "fwd-base")
    assert (c["mag"] == 0).any() and (c["mag"][0] > 0).any()
    # (k3's one part of image 2 is the origin keypoint: a 2 x 2 window of values below the threshold)
    assert (c["mag"][2] > 0).any() or row.parts == 1
    assert not c["mag"][1].any()
    assert c["P"] >= 1
    if rid == "k1s3":
        dead = [w for _, _, w, _ in wins if w[1] > w[0] and w[3] > w[2]
                and (KC.out_range(row, w)[1] < KC.out_range(row, w)[0] or KC.out_range(row, w)[3] < KC.out_range(row, w)[2])]
        assert dead, "a non-empty window that reaches no output pixel"
    if rid == "chunks":
        assert any(rows > max(1, KC.WG_PIX // ncol) for _, _, _, rows, ncol in KC.wg_blocks(row, kp)), \
            "a (window, band) of two or more chunks"
    if rid == "p32":
        assert KC.row_maps(rid)[:, 31].any(), "part 31 (the ballot's last bit) draws"


def test_replica_sets():
    """The weight gradient's replica choice: every row's workgroups land in several replicas, some
    of them surely outside replica 0, and every part leaves some replica alone, which is what
    shows a kernel that chose another."""
    for rid in RIDS:
        case = KC.make_case(rid, "wgrad-plain")
        may, must = KC.replicas_of(case, L.WREP)
        assert not (must & ~may).any() and must[1:].any()
        assert (~may).any(0).all()
        drawn = case["maps"].any((0, 2, 3))
        assert (must.any(0) == (np.abs(case["mag_w"]).sum((0, 2, 3)) > 0)).all() and (must.any(0) <= drawn).all()
        may1, must1 = KC.replicas_of(case, 1)
        assert (must1[0] == must.any(0)).all()


# ---- the documented refusals return on the host ---------------------------------------------
P = 64  # a non-NULL address no refused call may read


@pytest.mark.parametrize("what,entries,over,code", KC.REFUSED, ids=[r[0].replace(" ", "_") for r in KC.REFUSED])
def test_refused_before_any_launch(what, entries, over, code):
    lib = L.lib()
    before = lib.isg_last_launch()
    ptrs = dict.fromkeys(("kp", "w", "y", "stats", "dw", "out", "p"), P)
    fn = {"fwd": lib.isg_kp_stem_fwd, "wgrad": lib.isg_kp_stem_wgrad, "pool": lib.isg_kp_pool}
    for e in entries:
        a = struct(L.KpStem, KC.refusal_spec(over, ptrs, L.WREP))
        rc = fn[e](ctypes.byref(a), None)
        assert rc == code, (what, e, rc, lib.isg_last_error())
        assert lib.isg_last_error()
    assert lib.isg_last_launch() == before, "a refused call reached a launch"


def test_refusal_list_is_the_issues():
    names = {r[0] for r in KC.REFUSED}
    assert len(names) == len(KC.REFUSED) == 30
    assert sum(r[3] == KC.INVALID for r in KC.REFUSED) == 19
    # the base descriptor itself passes every geometry check a refusal overrides one of
    g = KC.REF_GEOM
    assert KC.REF_CKP0 + KC.REF_PARTS == g["Ci"] and g["H"] % 4 == 0 and g["W"] % 4 == 0
