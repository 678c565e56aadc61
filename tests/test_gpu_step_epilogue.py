"""Kernel-level tests of the step-epilogue kernels (csrc/eltwise.hip): isg_bn_finalize,
isg_grad_finalize, isg_bn_update_running, isg_sum_replicas and their fused form
isg_step_tail, called straight through the C ABI on synthetic statistics and compared
with the fp64 oracle (oracle/epilogue_oracle.py, pinned to torch by
tests/test_epilogue_oracle_cpu.py).

Bars (derived, not measured). The kernels evaluate in fp64 and round once to fp32, so a
value that is one rounding of an fp64 expression is held to one fp32 ulp of the oracle's
unrounded value, |got - ref| <= 2^-23 |ref| (floor 1e-37 where that is below fp32's
smallest normal). The oracle's own fp64 evaluation differs from the kernel's by a few
2^-53 (times <= 1e4 where the variance cancels: ordinary channels have var >= 1e-4 mean^2),
far inside the ulp. Other bars are stated where they are used. Every test prints the worst
observed ratio to its bar.

Inputs: statistics spread over all ISG_STAT_REP replicas with different values in each;
channel counts 1, 3, 64, 65 (bn_finalize1_kernel's 64/128-thread switch), 130 (the strided
channel loop of a 128-thread block), 512 (ISG_MAX_CH); 1, 2 and 33 items (the single-item
kernel; a second launch past ISG_LIST_CHUNK = 32); counts M = 30720 (2x96x160), 105 and
4096; per layer one channel whose sumsq/M - mean^2 is negative by 1e-9 mean^2 and one
constant channel with var == 0 exactly — both must clamp to rstd = 1/sqrt(eps).

All device memory of a case lives in one buffer with guard bytes between the arrays
(Arena); after each call every byte outside the declared outputs must be unchanged.
"""
import ctypes

import numpy as np
import pytest
import torch

from instancesegmentation_amd import _lib as L
from oracle import epilogue_oracle as E
from tests.isg_helpers import stream, struct

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS32 = float(np.float32(1e-5))       # isg_bn.eps is a float
ULP = 2.0 ** -23
ERR_INVALID, ERR_UNSUPPORTED = -1, -2  # isg.h ISG_ERR_*
CHANNELS = (1, 3, 64, 65, 130, 512)
COUNTS = (30720, 105, 4096)
SENTINEL = np.float32(-777.25)


# ---- device memory with guards ----------------------------------------------------------
class Arena:
    """Host arrays laid out in one byte buffer, 64-B aligned, 64 guard bytes (0xA5) apart."""
    GUARD = 64

    def __init__(self):
        self.items = []
        self.size = self.GUARD

    def add(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes > 0
        self.items.append((self.size, arr))
        self.size += (arr.nbytes + 63) // 64 * 64 + self.GUARD
        return len(self.items) - 1

    def host(self):
        buf = np.full(self.size, 0xA5, np.uint8)
        for off, arr in self.items:
            buf[off:off + arr.nbytes] = arr.reshape(-1).view(np.uint8)
        return buf

    def upload(self):
        return Inst(self, torch.from_numpy(self.host()).to(DEV))


class Inst:
    """One device copy of an Arena."""

    def __init__(self, arena, dev):
        self.a, self.dev = arena, dev

    def ptr(self, h, elem=0):
        off, arr = self.a.items[h]
        assert 0 <= elem <= arr.size
        return self.dev.data_ptr() + off + elem * arr.itemsize

    def read(self, h):
        off, arr = self.a.items[h]
        return self.dev[off:off + arr.nbytes].cpu().numpy().view(arr.dtype).reshape(arr.shape)

    def bytes(self):
        return self.dev.cpu().numpy()

    def span(self, h, lo=0, hi=None):
        off, arr = self.a.items[h]
        hi = arr.size if hi is None else hi
        return off + lo * arr.itemsize, off + hi * arr.itemsize

    def assert_untouched(self, outputs=()):
        """Every byte outside the (handle, lo, hi) element ranges equals the uploaded one."""
        keep = np.ones(self.a.size, bool)
        for h, lo, hi in outputs:
            b0, b1 = self.span(h, lo, hi)
            keep[b0:b1] = False
        changed = np.nonzero((self.bytes() != self.a.host()) & keep)[0]
        assert changed.size == 0, f"{changed.size} bytes outside the outputs changed, first at {changed[0]}"


def run(name, *args):
    """The call's status (no exception), after the stream has drained."""
    rc = getattr(L.lib(), name)(*args)
    torch.cuda.synchronize()
    return rc


def ratio(got, ref, bar=None):
    """Worst |got - ref| / bar; the default bar is one fp32 ulp of ref (floor 1e-37)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if bar is None:
        bar = np.maximum(ULP * np.abs(ref), 1e-37)
    return float((np.abs(got - ref) / bar).max())


def report(what, worst):
    print(f"{what}: worst |err| / bar = " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, (what, bad)


def upd(worst, key, r):
    worst[key] = max(worst.get(key, 0.0), r)


# ---- synthetic layers ---------------------------------------------------------------------
def dyadic(nrep):
    w = [2.0 ** -(r + 1) for r in range(nrep - 1)]
    return np.array(w + [1.0 - sum(w)])


def spread(vals, nrep, rng, exact=()):
    """[nrep, n] with different values in each replica that sum to ~vals; the entries in
    `exact` are split by dyadic weights, so their fp64 replica sum is vals exactly."""
    vals = np.asarray(vals, np.float64)
    w = rng.uniform(0.2, 1.0, (nrep, vals.size))
    w /= w.sum(0)
    for i in exact:
        w[:, i] = dyadic(nrep)
    return w * vals[None, :]


class Layer:
    """One BatchNorm layer's replicated statistics block and fp32 parameters, with the
    oracle's view of them (replica sums in replica order)."""

    def __init__(self, rng, C, M, specials=True):
        self.C, self.M = C, M
        mean = rng.uniform(0.1, 3.0, C) * rng.choice([-1.0, 1.0], C)
        var = rng.uniform(0.05, 4.0, C)  # >= 1e-4 mean^2 (mean^2 <= 9)
        s, sq = M * mean, M * (var + mean * mean)
        exact = []
        self.clamped = []
        if specials and C >= 3:
            sq[1] = (1.0 - 1e-9) * M * mean[1] ** 2     # variance negative beyond rounding
            s[C - 1], sq[C - 1] = M * 2.0, M * 4.0      # constant channel: var == 0 exactly
            exact = [C - 1, 2 * C - 1]
            self.clamped = [1, C - 1]
        gs = rng.normal(0.0, 1.0, C) * np.sqrt(M)
        gxs = rng.normal(0.0, 1.0, C) * np.sqrt(M)
        self.rep = spread(np.concatenate([s, sq, gs, gxs]), L.STAT_REP, rng, exact)
        self.gamma = (rng.uniform(0.5, 1.5, C) * rng.choice([-1.0, 1.0], C)).astype(np.float32)
        self.beta = rng.normal(0.0, 1.0, C).astype(np.float32)
        self.rm = rng.normal(0.0, 1.0, C).astype(np.float32)
        self.rv = rng.uniform(0.5, 2.0, C).astype(np.float32)
        self.nbt = np.array([int(rng.integers(0, 1000))], np.int64)
        self._totals()

    def _totals(self):
        C, M = self.C, self.M
        tot = E.replica_sum(self.rep)
        self.s, self.sq, self.gs, self.gxs = (tot[i * C:(i + 1) * C] for i in range(4))
        self.mean, self.var = E.batch_mean_var(self.s, self.sq, M)
        assert (self.var[self.clamped] == 0.0).all()
        self.rstd = E.rstd_of(self.var, EPS32)
        self.rstd_eval = E.rstd_of(self.rv, EPS32)

    def train_dconv_bias(self):
        return E.dconv_bias_train(self.gamma, self.rstd, self.s, self.gs, self.gxs, self.M)

    def want_residues(self, rng, at_least):
        """Redraw gsum of the channels whose train-mode dconv_bias expression evaluates to
        exactly 0 in plain fp64 (M*(gs/M) often rounds back to gs) until `at_least` channels
        leave a non-zero residue: a comparison of that gradient must not be one of zeros."""
        C = self.C
        for _ in range(1000):
            zero = np.nonzero(self.train_dconv_bias()[0] == 0.0)[0]
            if C - zero.size >= at_least:
                return
            new = rng.normal(0.0, 1.0, zero.size) * np.sqrt(self.M)
            self.rep[:, 2 * C + zero] = spread(new, L.STAT_REP, rng)
            self._totals()
        raise AssertionError("no statistics with non-zero dconv_bias residues found")

    def add_to(self, A):
        self.h = {k: A.add(getattr(self, k)) for k in ("rep", "gamma", "beta", "rm", "rv", "nbt")}


def cycle(seq, i):
    return seq[i % len(seq)]


# ---- isg_bn_finalize --------------------------------------------------------------------
BN_FINAL_CASES = [(f"single_C{C}", [C]) for C in CHANNELS] + \
                 [("two", [65, 3]), ("chunked33", [cycle(CHANNELS, i + 2) for i in range(33)])]


@pytest.mark.parametrize("bwd", [0, 1], ids=["fwd", "bwd"])
@pytest.mark.parametrize("name,Cs", BN_FINAL_CASES, ids=[c[0] for c in BN_FINAL_CASES])
def test_bn_finalize_matches_oracle(name, Cs, bwd):
    rng = np.random.default_rng(100 + len(Cs) + Cs[0])
    A = Arena()
    layers = [Layer(rng, C, cycle(COUNTS, i)) for i, C in enumerate(Cs)]
    coefs = []
    for ly in layers:
        ly.add_to(A)
        coefs.append(A.add(np.full(8 * ly.C, SENTINEL, np.float32)))
    I = A.upload()
    items = (L.Bn * len(layers))(*[
        struct(L.Bn, {"gamma": I.ptr(ly.h["gamma"]), "beta": I.ptr(ly.h["beta"]),
                      "stats": I.ptr(ly.h["rep"]), "C": ly.C, "train": 1, "count": float(ly.M),
                      "eps": 1e-5, "coef": I.ptr(hc)}) for ly, hc in zip(layers, coefs)])
    assert run("isg_bn_finalize", items, len(layers), bwd, stream()) == 0
    worst = {}
    outs = []
    for ly, hc in zip(layers, coefs):
        C = ly.C
        got = I.read(hc).reshape(2 * C, 4)[bwd * C:(bwd + 1) * C]
        outs.append((hc, bwd * 4 * C, (bwd + 1) * 4 * C))  # the other half: untouched
        if not bwd:
            ref = E.bn_fwd_coef(ly.mean, ly.rstd, ly.gamma, ly.beta)
            assert (got[:, 3] == 0).all() and not np.signbit(got[:, 3]).any()
            assert (got[:, 2] == ly.beta).all()
            names = ("mean", "gamma*rstd", "beta", "zero")
        else:
            ref = E.bn_bwd_coef(ly.mean, ly.rstd, ly.gamma, ly.gs, ly.gxs, ly.M)
            names = ("A", "B", "mean", "C")
        for j, nm in enumerate(names):
            upd(worst, nm, ratio(got[:, j], ref[:, j]))
        if ly.clamped:  # rstd = 1/sqrt(eps): lane 1 (fwd) / lane 0 (bwd) is gamma*rstd
            cl = ly.clamped
            upd(worst, "clamped gamma/sqrt(eps)",
                ratio(got[cl, 0 if bwd else 1], ly.gamma[cl].astype(np.float64) / np.sqrt(EPS32)))
    I.assert_untouched(outs)
    report(f"bn_finalize {name} bwd={bwd}", worst)


def test_bn_finalize_rejects_bad_items():
    rng = np.random.default_rng(7)
    A = Arena()
    ly = Layer(rng, 8, 105)
    ly.add_to(A)
    hc = A.add(np.full(8 * ly.C + 4, SENTINEL, np.float32))
    I = A.upload()
    spec = {"gamma": I.ptr(ly.h["gamma"]), "beta": I.ptr(ly.h["beta"]),
            "stats": I.ptr(ly.h["rep"]), "C": ly.C, "train": 1, "count": float(ly.M),
            "eps": 1e-5, "coef": I.ptr(hc)}
    good = struct(L.Bn, spec)
    no_stats = struct(L.Bn, dict(spec, stats=None))
    misaligned = struct(L.Bn, dict(spec, coef=I.ptr(hc, 1)))
    for bwd in (0, 1):
        for bad in (no_stats, misaligned):
            assert run("isg_bn_finalize", (L.Bn * 1)(bad), 1, bwd, stream()) == ERR_INVALID
            # a bad item anywhere in the list: nothing is launched, the good one not either
            assert run("isg_bn_finalize", (L.Bn * 2)(good, bad), 2, bwd, stream()) == ERR_INVALID
    I.assert_untouched()


# ---- isg_grad_finalize ------------------------------------------------------------------
FORMS = ("train_dcb", "train_no_dcb", "eval", "slope_C", "train_no_dgamma", "slope_4C",
         "train_no_dbeta")
GF_CASES = [(f"single_{f}", [f]) for f in FORMS] + \
           [("two", ["train_dcb", "eval"]), ("chunked33", [cycle(FORMS, i) for i in range(33)])]


class GfItem:
    """One isg_grad_final item of a given form over its own Layer and output arrays."""

    def __init__(self, rng, form, C, M, A):
        self.form, self.C = form, C
        self.ly = Layer(rng, C, M)
        self.ly.add_to(A)
        self.out = {}
        if form.startswith("slope"):
            self.out["dslope"] = A.add(np.full(C, SENTINEL, np.float32))
            if form == "slope_C":
                self.acc = spread(rng.normal(0, 1, C) * 2.0 ** rng.uniform(-10, 10, C),
                                  L.STAT_REP, rng)
                self.hacc = A.add(self.acc)
                self.ref = E.replica_sum(self.acc)
            else:  # the sum half of a stats block: replica stride 4*C
                self.hacc = self.ly.h["rep"]
                self.ref = self.ly.s
            return
        for k in ("dgamma", "dbeta", "dconv_bias"):
            if form != "train_no_" + {"dgamma": "dgamma", "dbeta": "dbeta", "dconv_bias": "dcb"}[k]:
                self.out[k] = A.add(np.full(C, SENTINEL, np.float32))

    def spec(self, I):
        ly, C = self.ly, self.C
        o = {k: I.ptr(h) for k, h in self.out.items()}
        if self.form.startswith("slope"):
            return dict(o, slope_acc=I.ptr(self.hacc), C=C,
                        slope_stride=C if self.form == "slope_C" else 4 * C)
        return dict(o, stats=I.ptr(ly.h["rep"]), gamma=I.ptr(ly.h["gamma"]),
                    running_mean=I.ptr(ly.h["rm"]), running_var=I.ptr(ly.h["rv"]), C=C,
                    train=0 if self.form == "eval" else 1, count=float(ly.M), eps=1e-5)

    def check(self, I, worst):
        ly = self.ly
        got = {k: I.read(h) for k, h in self.out.items()}
        if self.form.startswith("slope"):
            upd(worst, "dslope", ratio(got["dslope"], self.ref))
            return
        train = self.form != "eval"
        rstd = ly.rstd if train else ly.rstd_eval
        dgamma, dbeta = E.dgamma_dbeta(rstd, ly.gs, ly.gxs)
        if "dgamma" in got:
            upd(worst, "dgamma" if train else "eval dgamma", ratio(got["dgamma"], dgamma))
        if "dbeta" in got:
            upd(worst, "dbeta", ratio(got["dbeta"], dbeta))
        if "dconv_bias" in got:
            if train:  # mathematically zero: only the rounding residue of the expression
                _, bound = E.dconv_bias_train(ly.gamma, ly.rstd, ly.s, ly.gs, ly.gxs, ly.M)
                upd(worst, "train dconv_bias residue", ratio(got["dconv_bias"], 0.0, bound))
            else:
                upd(worst, "eval dconv_bias",
                    ratio(got["dconv_bias"], E.dconv_bias_eval(ly.gamma, rstd, ly.gs)))


@pytest.mark.parametrize("name,forms", GF_CASES, ids=[c[0] for c in GF_CASES])
def test_grad_finalize_matches_oracle(name, forms):
    rng = np.random.default_rng(200 + len(forms) + FORMS.index(forms[0]))
    A = Arena()
    shift = FORMS.index(forms[0])
    its = [GfItem(rng, f, cycle(CHANNELS, i + shift + 1), cycle(COUNTS, i + shift), A)
           for i, f in enumerate(forms)]
    I = A.upload()
    arr = (L.GradFinal * len(its))(*[struct(L.GradFinal, it.spec(I)) for it in its])
    assert run("isg_grad_finalize", arr, len(its), stream()) == 0
    worst = {}
    for it in its:
        it.check(I, worst)
    # outputs whose pointer was NULL do not exist; everything else (the guards next to
    # every output included) keeps its bytes
    I.assert_untouched([(h, 0, None) for it in its for h in it.out.values()])
    report(f"grad_finalize {name}", worst)


# ---- isg_bn_update_running --------------------------------------------------------------
def running_ref(ly, M, mom):
    """Oracle running statistics and their bar 4 * 2^-24 * (|(1-m) old| + |m new|): the
    kernel's fp32 expression has three roundings per term pair (1-m or the cast, the
    product, the sum), one product possibly contracted into the sum."""
    m = float(np.float32(mom))  # isg_bn_update.momentum is a float
    mean, var = E.batch_mean_var(ly.s, ly.sq, M)
    rm, rv, nbt = E.running_update(ly.rm, ly.rv, ly.nbt[0], mean, var, M, m)
    unb = var * M / (M - 1.0) if M > 1 else var
    bar_m = 4 * 2.0 ** -24 * (np.abs((1 - m) * ly.rm.astype(np.float64)) + np.abs(m * mean))
    bar_v = 4 * 2.0 ** -24 * (np.abs((1 - m) * ly.rv.astype(np.float64)) + np.abs(m * unb))
    return rm, rv, nbt, bar_m, bar_v


@pytest.mark.parametrize("nitems", [1, 2, 33])
def test_bn_update_running_matches_oracle(nitems):
    rng = np.random.default_rng(300 + nitems)
    A = Arena()
    counts = (30720, 1, 105, 4096)  # M = 1: the M > 1 guard (variance left unscaled)
    cfg = [(cycle(CHANNELS, i + nitems), cycle(counts, i + nitems // 2), cycle((0.1, 0.25), i),
            i % 3 != 1) for i in range(nitems)]
    assert nitems < 33 or {1, 30720} <= {c[1] for c in cfg}
    layers = []
    for C, M, mom, has_nbt in cfg:
        ly = Layer(rng, C, M)
        ly.add_to(A)
        layers.append(ly)
    I = A.upload()
    arr = (L.BnUpdate * nitems)(*[
        struct(L.BnUpdate, {"stats": I.ptr(ly.h["rep"]), "running_mean": I.ptr(ly.h["rm"]),
                            "running_var": I.ptr(ly.h["rv"]),
                            "num_batches_tracked": I.ptr(ly.h["nbt"]) if has_nbt else None,
                            "C": C, "count": float(M), "momentum": mom})
        for ly, (C, M, mom, has_nbt) in zip(layers, cfg)])
    assert run("isg_bn_update_running", arr, nitems, stream()) == 0
    worst = {}
    outs = []
    for ly, (C, M, mom, has_nbt) in zip(layers, cfg):
        rm, rv, nbt, bar_m, bar_v = running_ref(ly, M, mom)
        got_m, got_v, got_n = I.read(ly.h["rm"]), I.read(ly.h["rv"]), I.read(ly.h["nbt"])
        assert np.isfinite(got_m).all() and np.isfinite(got_v).all()
        upd(worst, "running_mean", ratio(got_m, rm, bar_m))
        upd(worst, "running_var" if M > 1 else "running_var (M=1)", ratio(got_v, rv, bar_v))
        assert got_n.dtype == np.int64 and int(got_n[0]) == (nbt if has_nbt else int(ly.nbt[0]))
        outs += [(ly.h["rm"], 0, None), (ly.h["rv"], 0, None)]
        if has_nbt:
            outs.append((ly.h["nbt"], 0, None))
    I.assert_untouched(outs)
    report(f"bn_update_running x{nitems}", worst)


# ---- isg_sum_replicas -------------------------------------------------------------------
def _sum_rep_case(rng, n, nrep, stride, dst_off):
    A = Arena()
    src = rng.normal(0, 1, nrep * stride) * 2.0 ** rng.integers(0, 21, nrep * stride)
    hs = A.add(src)
    hd = A.add(np.full(n + dst_off + 3, SENTINEL, np.float32))
    I = A.upload()
    rc = run("isg_sum_replicas", I.ptr(hd, dst_off), I.ptr(hs), n, nrep, stride, stream())
    assert rc == 0
    ref = E.replica_sum(np.stack([src[r * stride:r * stride + n] for r in range(nrep)]))
    got = I.read(hd)[dst_off:dst_off + n]
    # fp64 adds in a fixed order are deterministic: the fp32 result is determined bit for bit
    diff = int((got.view(np.uint32) != ref.astype(np.float32).view(np.uint32)).sum())
    assert diff == 0, (n, nrep, stride, dst_off, diff)
    I.assert_untouched([(hd, dst_off, dst_off + n)])


@pytest.mark.parametrize("nrep", [1, 2, 3, 5])
def test_sum_replicas_runtime_count_is_bitwise_the_ordered_fp64_sum(nrep):
    """The runtime-count kernel: 16-B path, its n % 4 tail, and the scalar fallback (dst
    one float past 16-B alignment, or a replica stride that is no multiple of 4)."""
    rng = np.random.default_rng(400 + nrep)
    cases = 0
    for n in (1, 5, 1023, 1024):
        pad4 = (n + 3) // 4 * 4 + 4
        odd = n + 1 if (n + 1) % 4 else n + 2
        for stride, dst_off in ((pad4, 0), (pad4, 1), (odd, 0), (n, 0)):
            _sum_rep_case(rng, n, nrep, stride, dst_off)
            cases += 1
    print(f"sum_replicas nrep={nrep}: {cases} layouts bit-identical to float(ordered fp64 sum)")


@pytest.mark.parametrize("nrep", [4, 8, 16])
def test_sum_replicas_compile_time_count_is_bitwise_the_ordered_fp64_sum(nrep):
    rng = np.random.default_rng(450 + nrep)
    for stride, dst_off in ((1000, 0), (1003, 1)):
        _sum_rep_case(rng, 1000, nrep, stride, dst_off)
    print(f"sum_replicas nrep={nrep}: n=1000 bit-identical to float(ordered fp64 sum)")


def test_sum_replicas_rejects_bad_arguments():
    A = Arena()
    hs = A.add(np.ones(64, np.float64))
    hd = A.add(np.full(16, SENTINEL, np.float32))
    I = A.upload()
    assert run("isg_sum_replicas", I.ptr(hd), I.ptr(hs), 8, 0, 8, stream()) == ERR_INVALID
    assert run("isg_sum_replicas", I.ptr(hd), I.ptr(hs), 8, 2, 7, stream()) == ERR_INVALID
    I.assert_untouched()


# ---- isg_step_tail ----------------------------------------------------------------------
HYPER = (1e-3, 0.9, 0.999, 1e-8, 0.01)  # lr, beta1, beta2, eps, weight_decay (non-zero)
# the flat layout (float offsets), as the Trainer lays a model out: a BatchNorm's gamma at
# `param + off` has its gradient at `grad + off`
T_C, E_C, S_C = 24, 20, 16
T_GAMMA, T_BETA, T_CB = 0, 24, 48
E_GAMMA, E_BETA, E_CB = 72, 92, 112
S_OFF = 132
ORPHANS = (148, 149)  # owner bit 1 set but no grad_final item writes them: owner 2 and 3
FOLD0 = 150


class TailCase:
    def __init__(self, n, nrep, step0, seed):
        rng = np.random.default_rng(seed)
        self.n, self.nrep, self.step0 = n, nrep, step0
        A = self.A = Arena()
        self.T = Layer(rng, T_C, 30720)   # train item, M = 2*96*160, with dconv_bias
        self.T.want_residues(rng, T_C // 2)
        self.Ev = Layer(rng, E_C, 105)    # eval item with dconv_bias (running stats constant)
        self.U2 = Layer(rng, 7, 105)      # second BN-update layer (the first is T)
        for ly in (self.T, self.Ev, self.U2):
            ly.add_to(A)
        self.slope = spread(rng.normal(0, 1, S_C), L.STAT_REP, rng)
        self.h_slope = A.add(self.slope)
        owner = (rng.uniform(size=n) < 0.8).astype(np.uint8)
        owner[FOLD0:FOLD0 + 4] = (0, 1, 0, 1)
        owner[:S_OFF + S_C] = 3
        owner[S_OFF + 12:S_OFF + S_C] = 2   # gradient written, parameter not updated
        owner[E_BETA + 3] = 2
        owner[ORPHANS[0]], owner[ORPHANS[1]] = 2, 3
        assert set(owner.tolist()) == {0, 1, 2, 3}
        self.owner = owner
        param = rng.normal(0, 1, n).astype(np.float32)
        param[T_GAMMA:T_GAMMA + T_C] = self.T.gamma
        param[E_GAMMA:E_GAMMA + E_C] = self.Ev.gamma
        self.param = param
        if step0:
            self.m0 = rng.normal(0, 1e-2, n).astype(np.float32)
            self.v0 = rng.uniform(0, 1e-4, n).astype(np.float32)
        else:
            self.m0, self.v0 = np.zeros(n, np.float32), np.zeros(n, np.float32)
        self.rep = rng.normal(0, 1, (nrep, n)) * 2.0 ** rng.integers(-10, 1, (nrep, n))
        self.h = {"grad": A.add(np.full(n, 123.0, np.float32)), "rep": A.add(self.rep),
                  "param": A.add(param), "m": A.add(self.m0), "v": A.add(self.v0),
                  "owner": A.add(owner), "step": A.add(np.array([step0], np.int32)),
                  "hyper": A.add(np.array(HYPER, np.float64)),
                  "live": A.add(owner & 1)}

    def gf_specs(self, I):
        g, p = self.h["grad"], self.h["param"]
        T, Ev = self.T, self.Ev
        return [
            {"stats": I.ptr(T.h["rep"]), "gamma": I.ptr(p, T_GAMMA), "running_mean": I.ptr(T.h["rm"]),
             "running_var": I.ptr(T.h["rv"]), "dgamma": I.ptr(g, T_GAMMA), "dbeta": I.ptr(g, T_BETA),
             "dconv_bias": I.ptr(g, T_CB), "C": T_C, "train": 1, "count": float(T.M), "eps": 1e-5},
            {"stats": I.ptr(Ev.h["rep"]), "gamma": I.ptr(p, E_GAMMA), "running_mean": I.ptr(Ev.h["rm"]),
             "running_var": I.ptr(Ev.h["rv"]), "dgamma": I.ptr(g, E_GAMMA), "dbeta": I.ptr(g, E_BETA),
             "dconv_bias": I.ptr(g, E_CB), "C": E_C, "train": 0, "count": float(Ev.M), "eps": 1e-5},
            {"slope_acc": I.ptr(self.h_slope), "dslope": I.ptr(g, S_OFF), "C": S_C,
             "slope_stride": S_C}]

    def bnu_specs(self, I):
        return [{"stats": I.ptr(ly.h["rep"]), "running_mean": I.ptr(ly.h["rm"]),
                 "running_var": I.ptr(ly.h["rv"]), "num_batches_tracked": nbt, "C": ly.C,
                 "count": float(ly.M), "momentum": mom}
                for ly, mom, nbt in ((self.T, 0.1, I.ptr(self.T.h["nbt"])), (self.U2, 0.25, None))]

    def tail_args(self, I, gf_dev, bnu_dev, **over):
        h = self.h
        spec = {"grad": I.ptr(h["grad"]), "rep": I.ptr(h["rep"]), "n": self.n, "nrep": self.nrep,
                "ngf": 3, "param": I.ptr(h["param"]), "exp_avg": I.ptr(h["m"]),
                "exp_avg_sq": I.ptr(h["v"]), "owner": I.ptr(h["owner"]), "step": I.ptr(h["step"]),
                "hyper": I.ptr(h["hyper"]), "gf": gf_dev.data_ptr(), "bnu": bnu_dev.data_ptr(),
                "nbnu": 2}
        spec.update(over)
        return struct(L.StepTail, spec)

    def device_items(self, I):
        gf = (L.GradFinal * 3)(*[struct(L.GradFinal, s) for s in self.gf_specs(I)])
        bnu = (L.BnUpdate * 2)(*[struct(L.BnUpdate, s) for s in self.bnu_specs(I)])
        up = [torch.frombuffer(bytearray(bytes(a)), dtype=torch.uint8).to(DEV) for a in (gf, bnu)]
        return gf, bnu, up[0], up[1]

    def run_separate(self):
        I = self.A.upload()
        h = self.h
        gf, bnu, _, _ = self.device_items(I)
        st = stream()
        assert run("isg_sum_replicas", I.ptr(h["grad"]), I.ptr(h["rep"]), self.n, self.nrep,
                   self.n, st) == 0
        assert run("isg_grad_finalize", gf, 3, st) == 0
        assert run("isg_adam_dev", I.ptr(h["param"]), I.ptr(h["grad"]), I.ptr(h["m"]),
                   I.ptr(h["v"]), I.ptr(h["live"]), self.n, I.ptr(h["step"]), *HYPER, st) == 0
        assert run("isg_bn_update_running", bnu, 2, st) == 0
        return I

    def run_fused(self):
        I = self.A.upload()
        _, _, gf_dev, bnu_dev = self.device_items(I)
        assert run("isg_step_inc", I.ptr(self.h["step"]), stream()) == 0
        assert run("isg_step_tail", ctypes.byref(self.tail_args(I, gf_dev, bnu_dev)), stream()) == 0
        return I

    def oracle(self):
        """(grad, param, exp_avg, exp_avg_sq) in fp64; the train-mode dconv_bias is 0."""
        T, Ev = self.T, self.Ev
        g = E.replica_sum(self.rep)
        g[T_GAMMA:T_GAMMA + T_C], g[T_BETA:T_BETA + T_C] = E.dgamma_dbeta(T.rstd, T.gs, T.gxs)
        g[T_CB:T_CB + T_C] = 0.0
        g[E_GAMMA:E_GAMMA + E_C], g[E_BETA:E_BETA + E_C] = E.dgamma_dbeta(Ev.rstd_eval, Ev.gs, Ev.gxs)
        g[E_CB:E_CB + E_C] = E.dconv_bias_eval(Ev.gamma, Ev.rstd_eval, Ev.gs)
        g[S_OFF:S_OFF + S_C] = E.replica_sum(self.slope)
        p, m, v = E.adam_step(self.param, g, self.m0, self.v0, self.step0 + 1, *HYPER)
        return g, p, m, v


TAIL_CASES = [(n, nrep, step0) for n in (256, 1000) for nrep in (4, 8, 16) for step0 in (0, 6)]


@pytest.mark.parametrize("n,nrep,step0", TAIL_CASES)
def test_step_tail_matches_separate_calls_and_oracle(n, nrep, step0):
    """(a) bit for bit the separate calls (fold, grad_finalize, adam_dev, bn_update_running)
    on an identical copy of the buffers; (b) the oracle's gradients and its Adam step.
    Before grad_final_item read gamma ahead of its first store, (a) failed on grad and
    exp_avg of the conv-bias elements and (b) on the eval item's dconv_bias (a relative error
    of lr/|gamma|): the fused form read the gamma its own dgamma store had just updated."""
    tc = TailCase(n, nrep, step0, 500 + n + nrep + step0)
    T = tc.T
    db64, bound = T.train_dconv_bias()
    # vacuity guard, checked on the CPU first: these statistics leave rounding residues
    assert np.count_nonzero(db64) >= T_C // 2, "inputs give no non-zero train-mode dconv_bias"
    sep, fus = tc.run_separate(), tc.run_fused()
    live = (tc.owner & 1).astype(bool)
    orphan = np.zeros(n, bool)
    orphan[list(ORPHANS)] = True

    # ---- (a) bitwise against the separate calls
    sep_cb = sep.read(tc.h["grad"])[T_CB:T_CB + T_C]
    assert np.count_nonzero(sep_cb) > 0, "no non-zero train-mode dconv_bias: (a) would be vacuous"
    diff = {}
    for k in ("grad", "param", "m", "v"):
        a, b = fus.read(tc.h[k]).view(np.uint32), sep.read(tc.h[k]).view(np.uint32)
        diff[k] = int(((a != b) & ~orphan).sum())
    for name, ly in (("T", tc.T), ("U2", tc.U2), ("Ev", tc.Ev)):
        for k in ("rm", "rv", "nbt"):
            diff[f"{name}.{k}"] = int((fus.read(ly.h[k]) != sep.read(ly.h[k])).sum())
    diff["step"] = int((fus.read(tc.h["step"]) != sep.read(tc.h["step"])).sum())
    print(f"step_tail n={n} nrep={nrep} step {step0 + 1}: elements differing fused vs separate {diff}")
    assert not any(diff.values()), diff
    assert int(fus.read(tc.h["step"])[0]) == step0 + 1
    # beyond the named buffers: every other byte (guards, inputs) agrees too
    fb, sb = fus.bytes(), sep.bytes()
    skip = np.zeros(tc.A.size, bool)
    for k in ("grad", "param", "m", "v"):
        for o in ORPHANS:
            b0, b1 = fus.span(tc.h[k], o, o + 1)
            skip[b0:b1] = True
    assert ((fb == sb) | skip).all()

    # ---- untouched elements
    got = {k: fus.read(tc.h[k]) for k in ("grad", "param", "m", "v")}
    for k, orig in (("param", tc.param), ("m", tc.m0), ("v", tc.v0)):
        same = got[k].view(np.uint32) == orig.view(np.uint32)
        assert same[~live].all(), f"{k}: an element with owner bit 0 clear changed"
        assert same[orphan].all(), f"{k}: an element no kernel owns changed"
    assert (got["grad"][orphan] == np.float32(123.0)).all(), "the fold wrote an owner-bit-1 element"
    outs = [(tc.h[k], 0, None) for k in ("grad", "param", "m", "v", "step")]
    outs += [(ly.h[k], 0, None) for ly in (tc.T, tc.U2) for k in ("rm", "rv")]
    outs.append((tc.T.h["nbt"], 0, None))
    fus.assert_untouched(outs)  # U2's nbt (NULL pointer) and Ev's running statistics included

    # ---- (b) against the oracle
    g, p, m, v = tc.oracle()
    worst = {}
    ulp_mask = ~orphan
    ulp_mask[T_CB:T_CB + T_C] = False
    upd(worst, "grad (1 ulp)", ratio(got["grad"][ulp_mask], g[ulp_mask]))
    upd(worst, "eval dconv_bias (1 ulp)", ratio(got["grad"][E_CB:E_CB + E_C], g[E_CB:E_CB + E_C]))
    upd(worst, "train dconv_bias residue", ratio(got["grad"][T_CB:T_CB + T_C], 0.0, bound))
    upd_mask = live & ~orphan
    # the project's Adam bar (tests/test_gpu_trainer.py): rtol 2e-6, atol 1e-9
    upd(worst, "param (Adam bar)", ratio(got["param"][upd_mask], p[upd_mask],
                                         2e-6 * np.abs(p[upd_mask]) + 1e-9))
    for ly, mom in ((tc.T, 0.1), (tc.U2, 0.25)):
        rm, rv, nbt, bar_m, bar_v = running_ref(ly, ly.M, mom)
        upd(worst, "running_mean", ratio(fus.read(ly.h["rm"]), rm, bar_m))
        upd(worst, "running_var", ratio(fus.read(ly.h["rv"]), rv, bar_v))
    assert int(fus.read(tc.T.h["nbt"])[0]) == int(tc.T.nbt[0]) + 1
    report(f"step_tail n={n} nrep={nrep} step {step0 + 1} vs oracle", worst)


def test_step_tail_rejects_bad_arguments():
    tc = TailCase(256, 4, 0, 9)
    I = tc.A.upload()
    _, _, gf_dev, bnu_dev = tc.device_items(I)
    bad_nrep = tc.tail_args(I, gf_dev, bnu_dev, nrep=5)
    no_owner = tc.tail_args(I, gf_dev, bnu_dev, owner=None)
    no_owner.owner = None
    assert run("isg_step_tail", ctypes.byref(bad_nrep), stream()) == ERR_UNSUPPORTED
    assert run("isg_step_tail", ctypes.byref(no_owner), stream()) == ERR_INVALID
    I.assert_untouched()
