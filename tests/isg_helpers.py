"""Direct C-ABI call helpers for kernel-level GPU tests (real pointers in the structs)."""
import ctypes

import numpy as np
import torch

from instancesegmentation_amd import _lib as L
from instancesegmentation_amd.engine import _fill


def struct(cls, spec):
    obj = cls()
    fix = []
    _fill(obj, spec, 0, fix)
    assert not fix
    return obj


def ptr(t):
    return t.data_ptr() if t is not None else None


def rep_zeros(n, device="cuda"):
    """An accumulator of n doubles in its ISG_STAT_REP replicas (isg.h)."""
    return torch.zeros(L.STAT_REP * n, dtype=torch.float64, device=device)


def rep_from(vals, device="cuda"):
    """Replicated accumulator holding `vals` (replica 0) — precomputed stats input."""
    out = rep_zeros(vals.numel(), device)
    out[:vals.numel()] = vals.to(device=device, dtype=torch.float64)
    return out


def rep_fold(t, n):
    """Sum of the replicas of an accumulator of n values."""
    return t.view(L.STAT_REP, n).sum(0)


def bn_spec_eval(gamma, beta, rm, rv, eps=1e-5):
    return {"gamma": ptr(gamma), "beta": ptr(beta), "running_mean": ptr(rm),
            "running_var": ptr(rv), "C": gamma.numel(), "train": 0, "count": 1.0, "eps": eps}


def bn_spec_train(gamma, beta, stats, count, eps=1e-5):
    return {"gamma": ptr(gamma), "beta": ptr(beta), "stats": ptr(stats), "C": gamma.numel(),
            "train": 1, "count": float(count), "eps": eps}


def vt(segs, N, H, W):
    return struct(L.VTensor, {"s": segs, "nseg": len(segs), "N": N, "H": H, "W": W})


def sinks(lst):
    return struct(L.Sinks, {"s": lst, "nsink": len(lst)})


def geom(**kw):
    return struct(L.Geom, kw)


def stream():
    return L.stream_ptr()


def call(name, *args):
    fn = getattr(L.lib(), name)
    conv = []
    for a in args:
        if isinstance(a, ctypes.Structure):
            conv.append(ctypes.byref(a))
        else:
            conv.append(a)
    L.check(fn(*conv), name)
    torch.cuda.synchronize()


# ---- operands as the network presents them: channel slices, replicas, canaries --------------
NAN = float("nan")
POISON = 1e30  # around the slice of an input: a misplaced read shows


def dev(a, device="cuda"):
    return torch.from_numpy(np.array(a, order="C")).to(device)  # a copy: the cases are read-only


def bits(t):
    """The raw words of a float tensor as numpy (NaN compares as its bits)."""
    t = t.detach().contiguous().cpu()
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32).numpy()


def same_bits(got, want, what):
    bad = int((bits(got) != bits(want)).sum())
    assert bad == 0, f"{what}: {bad} elements differ bitwise"


class Slab:
    """A [N, C, H, W] channel slice at channel c0 of a wider [N, C + pad, H, W] buffer, which
    starts `off` floats into its allocation and leaves `tail` unused floats after every image
    (n_stride = (C + pad)*H*W + tail). `data` fills the slice, `fill` everything else."""

    def __init__(self, C, H, W, data=None, fill=NAN, pad=3, c0=2, off=0, N=2, tail=0, device="cuda"):
        self.C, self.c0 = C, c0
        self.n_stride = (C + pad) * H * W + tail
        self.flat = torch.full((off + N * self.n_stride,), fill, dtype=torch.float32, device=device)
        self.buf = self.flat[off:].as_strided((N, C + pad, H, W), (self.n_stride, H * W, W, 1))
        if data is not None:
            self.buf[:, c0:c0 + C] = dev(np.asarray(data, np.float32), device)
        self.ptr = self.buf[0, c0].data_ptr()
        inside = torch.zeros(N, self.n_stride, dtype=torch.bool)
        inside[:, c0 * H * W:(c0 + C) * H * W] = True
        self.inside = torch.cat([torch.zeros(off, dtype=torch.bool), inside.reshape(-1)])
        self.before = self.flat.clone()

    def get(self):
        return self.buf[:, self.c0:self.c0 + self.C]

    def outside_untouched(self, what, whole=False):
        changed = torch.from_numpy(bits(self.flat) != bits(self.before))
        if not whole:
            changed &= ~self.inside
        assert not changed.any(), f"{what}: {int(changed.sum())} words around the slice changed"


def rep_spread(vals):
    """A replicated accumulator whose replicas sum to `vals` (dyadic shares: to within an fp64
    rounding), so a consumer that read replica 0 alone would be off by half."""
    vals = np.asarray(vals, np.float64)
    w = [2.0 ** -(r + 1) for r in range(L.STAT_REP - 1)]
    w.append(1.0 - sum(w))
    return dev(np.concatenate([wi * vals for wi in w]))
