"""Graph values: arena buffers, the BatchNorm / PReLU references a virtual value carries,
channel segments (Val), concatenations of them (Value) and the keypoint input."""
from .records import S_STATS, Ptr


class Buf:
    """An NCHW fp32 region of an arena (act or grad) or an external slot."""
    # offset (doubles, statistics arena) of the per-channel sum of this buffer's gradient
    # that the consumers' sinks accumulate (Graph.conv_transpose sets it; GradState.sink_for,
    # TailOp.bwd and the plan's finalisation read it)
    need_sum = None

    def __init__(self, slot, N, C, H, W, name, off=0):
        self.slot, self.N, self.C, self.H, self.W, self.name = slot, N, C, H, W, name
        self.off = off  # elements

    @property
    def n_stride(self):
        return self.C * self.H * self.W

    @property
    def numel(self):
        return self.N * self.C * self.H * self.W

    def ptr(self, c0=0):
        return Ptr(self.slot, (self.off + c0 * self.H * self.W) * 4)


def _buf_range(buf):
    """(slot, lo, hi): the byte range of a whole arena buffer. A pool writes a channel slice
    of its output buffer, but a later record's pointer into that buffer names only where
    its own access STARTS (e.g. channel 0 of a concat it reads whole): any pointer into the
    buffer counts as touching the slice, so the join can never be placed after a reader
    whose start lies below the slice."""
    o = buf.ptr(0)
    return (o.slot, o.off, o.off + buf.numel * 4)


MAX_TENSOR_ELEMS = 2 ** 31 - 1


def check_elems(b):
    """The kernels address a tensor's elements (image stride x image + pixel) with 32-bit
    offsets; a tensor at or above 2^31 elements is refused here, at plan time."""
    if b.numel > MAX_TENSOR_ELEMS:
        raise RuntimeError(f"{b.name}: {b.N}x{b.C}x{b.H}x{b.W} = {b.numel} elements exceeds "
                           f"the kernels' 32-bit element offsets ({MAX_TENSOR_ELEMS}); "
                           "split the batch")


class BNRef:
    def __init__(self, mod, C, count, stats_off, names, fin, coef_off, coef_end):
        self.mod, self.C, self.count, self.stats_off = mod, C, count, stats_off
        self.names = names  # dict: gamma, beta, rm, rv, nbt -> tensor slot
        # finalised once per layer by an OP_BN_FINAL launch, or by every consumer
        self.fin = fin
        # finalised coefficients (isg_bn.coef): 8*C floats = 4*C doubles, 64-B aligned
        self.coef_off, self.coef_end = coef_off, coef_end


class SlopeRef:
    def __init__(self, mod, C, acc_off, slot):
        self.mod, self.C, self.acc_off, self.slot = mod, C, acc_off, slot
        self.used_in_bwd = False

    def put(self, spec):
        """The slope pointer of a spec that applies the activation."""
        spec["slope"] = Ptr(self.slot)

    def put_grad(self, spec):
        """The slope-gradient accumulator of a backward spec; the plan then finalises it."""
        spec["slope_grad"] = Ptr(S_STATS, self.acc_off * 8)
        self.used_in_bwd = True


class Val:
    """One channel segment: act(BN(buf[c0:c0+C])) (identity when bn is None, act none)."""

    def __init__(self, buf, c0, C, bn=None, act="none", slope=None, grad=True):
        self.buf, self.c0, self.C = buf, c0, C
        self.bn, self.act, self.slope = bn, act, slope
        self.grad = grad

    @property
    def virtual(self):
        return self.bn is not None or self.act != "none"


class Value:
    def __init__(self, segs):
        self.segs = list(segs)
        assert len({(s.buf.H, s.buf.W) for s in self.segs}) == 1
        self.H, self.W = self.segs[0].buf.H, self.segs[0].buf.W
        self.C = sum(s.C for s in self.segs)

    @property
    def grad(self):
        return any(s.grad for s in self.segs)


def cat(*vals):
    segs = []
    for v in vals:
        segs += v.segs
    return Value(segs)


class Keypoints:
    """Keypoint input [N, nparts, 3] float64 = (x, y, visible > 0) of slot `slot`, standing
    for `nparts` heatmap channels (train_instance.py:33-68) that are never materialised:
    the stem synthesises them on the fly (isg_kp_stem)."""

    def __init__(self, slot, N, nparts, sigma=10.0, threshold=0.01):
        self.slot, self.N, self.nparts = slot, N, nparts
        self.sigma, self.threshold = sigma, threshold
        self.C = nparts
        self.grad = False

    def spec(self):
        return {"kp": Ptr(self.slot), "nparts": self.nparts, "sigma": float(self.sigma),
                "threshold": float(self.threshold)}
