"""Record specs of the structures every op shares (isg_bn, isg_vseg, isg_vtensor, isg_sinks)
and GradState, the backward's bookkeeping, which hands out the gradient sinks."""
from .. import _lib as L
from .records import ALIGN, S_GRAD, S_STATS, Ptr, Record
from .values import Buf, check_elems


def sinks_spec(sinks):
    """isg_sinks spec from sink specs."""
    return {"s": sinks, "nsink": len(sinks)}


def bn_spec(bnr, train, coef=True):
    if bnr is None:
        return {"train": 1}
    n = bnr.names
    s = {"gamma": n["gamma"], "beta": n["beta"], "running_mean": n["rm"],
         "running_var": n["rv"], "stats": Ptr(S_STATS, bnr.stats_off * 8), "C": bnr.C,
         "train": 1 if train else 0, "count": float(bnr.count), "eps": float(bnr.mod.eps)}
    if train and coef and bnr.fin:
        # consumers read the coefficients OP_BN_FINAL wrote (forward half after the
        # producing conv, backward half after the op that completes gsum/gxsum)
        s["coef"] = Ptr(S_STATS, bnr.coef_off * 8)
    return s


def bn_final_record(bnrs, bwd):
    items = [bn_spec(b, True) for b in bnrs]
    return Record(L.OP_BN_FINAL, L.ListRec, {"n": len(items), "pad_": 1 if bwd else 0}, L.Bn,
                  items, label=("bn_final_bwd " if bwd else "bn_final ") +
                  ",".join(str(b.C) for b in bnrs))


def fwd_seg(val, train):
    s = {"p": val.buf.ptr(val.c0), "n_stride": val.buf.n_stride, "C": val.C,
         "xform": L.XF_BN_FWD if val.virtual else L.XF_PLAIN, "act": L.ACT[val.act]}
    if val.virtual:
        s["bn"] = bn_spec(val.bn, train)
        if val.slope is not None:
            val.slope.put(s)
    return s


def vtensor(segs, N, H, W):
    return {"s": segs, "nseg": len(segs), "N": N, "H": H, "W": W}


def value_vtensor(g, x):
    """The forward vtensor of a Value: what an op reads as its input."""
    return vtensor([fwd_seg(v, g.train) for v in x.segs], g.N, x.H, x.W)


class GradState:
    """Backward bookkeeping: gradient buffers in the grad arena."""

    def __init__(self, g):
        self.g = g
        self.size = 0
        self.D = {}       # id(buf) -> grad Buf (materialised values / plain raws)
        self.G = {}       # id(raw buf) -> g Buf (dL/d BN-output of a virtual value)
        self.inited = {}  # id(buf) -> set of (c0, C)
        self.external = {}  # id(buf) -> Buf (e.g. dlogits slot)
        self.pending_final = []  # BNs whose gsum/gxsum the last op completed
        # what the ops leave for the plan's finalisation items (plan._final_items):
        self.bias_sums = []     # (convT, its output buf, dy): bias = the sinks' channel sums
        self.bias_from_bn = []  # (conv, bnr): conv bias before a BatchNorm

    def alloc(self, like, name):
        b = Buf(S_GRAD, like.N, like.C, like.H, like.W, name, off=self.size)
        check_elems(b)
        self.size += (b.numel + ALIGN - 1) // ALIGN * ALIGN
        return b

    def dbuf(self, buf):
        if id(buf) in self.external:
            return self.external[id(buf)]
        if id(buf) not in self.D:
            self.D[id(buf)] = self.alloc(buf, "d_" + buf.name)
        return self.D[id(buf)]

    def has_grad(self, buf, c0, C):
        return id(buf) in self.external or (c0, C) in self.inited.get(id(buf), set())

    def mark(self, buf, c0, C):
        first = (c0, C) not in self.inited.setdefault(id(buf), set())
        self.inited[id(buf)].add((c0, C))
        return first

    def sink_for(self, val, c0_glob, train):
        """Sink that receives dL/d(val) for channels [c0_glob, c0_glob+val.C) of a kernel's
        output rows."""
        if not val.grad:
            return {"c0": c0_glob, "C": val.C, "mode": L.SINK_NONE}
        if val.virtual:
            assert id(val.buf) not in self.G, f"virtual value {val.buf.name} consumed twice"
            gb = self.alloc(val.buf, "g_" + val.buf.name)
            self.G[id(val.buf)] = gb
            s = {"p": gb.ptr(val.c0), "n_stride": gb.n_stride, "c0": c0_glob, "C": val.C,
                 "mode": L.SINK_ACTBWD, "act": L.ACT[val.act],
                 "y": val.buf.ptr(val.c0), "y_n_stride": val.buf.n_stride,
                 "bn": bn_spec(val.bn, train)}
            if val.slope is not None:
                val.slope.put(s)
                val.slope.put_grad(s)
            if val.bn is not None and val.bn.fin:
                self.pending_final.append(val.bn)
            return s
        d = self.dbuf(val.buf)
        first = self.mark(val.buf, val.c0, val.C)
        s = {"p": d.ptr(val.c0), "n_stride": d.n_stride, "c0": c0_glob, "C": val.C,
             "mode": L.SINK_STORE if first else L.SINK_ACCUM}
        if val.buf.need_sum is not None:
            assert val.c0 == 0 and val.C == val.buf.C
            s["stats"] = Ptr(S_STATS, val.buf.need_sum * 8)
        return s

    def sinks(self, x):
        """The sinks that receive dL/d(x), one per segment of the Value x, in channel
        order."""
        out, c = [], 0
        for v in x.segs:
            out.append(self.sink_for(v, c, self.g.train))
            c += v.C
        return out

    def dy_seg(self, buf, bnr, train):
        """The gradient w.r.t. a conv's raw output `buf`, as a virtual segment, or None
        when nothing downstream produced one (the output does not reach the loss)."""
        if bnr is not None:
            if id(buf) not in self.G:
                return None
            gb = self.G[id(buf)]
            return {"p": gb.ptr(), "y": buf.ptr(), "n_stride": gb.n_stride,
                    "y_n_stride": buf.n_stride, "C": buf.C, "xform": L.XF_BN_BWD,
                    "bn": bn_spec(bnr, train)}
        if not self.has_grad(buf, 0, buf.C):
            return None
        d = self.dbuf(buf)
        return {"p": d.ptr(), "n_stride": d.n_stride, "C": buf.C, "xform": L.XF_PLAIN}
