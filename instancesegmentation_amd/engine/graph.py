"""The tracer: a module's `emit` calls Graph methods, which allocate activation buffers and
statistics and append ops; param_layout is the flat parameter order a Trainer gives it."""
import contextlib

import torch.nn as nn

from .. import _lib as L
from . import knobs
from .ops import ConvOp, ConvPairOp, HeadOp, KpPoolOp, PoolOp, TailOp
from .records import ALIGN, S_ACT, S_IN, S_PGRAD, S_TENSOR0, S_WREP, Ptr
from .values import BNRef, Buf, Keypoints, SlopeRef, Val, Value, check_elems


def param_layout(owner):
    """The flat parameter order of a Trainer (train.flatten_module): the module's
    parameter order, except that the weight of the second conv of each sibling pair — two
    1x1 Convs reading the same input, declared by a module's `siblings()` (BottleneckDim_Res
    convs.0 + resconv, segment.py:198-202; BottleneckUp_Res convs.0 + conv2, :326-331) —
    follows the first one's weight directly, so the pair's weights [W1; W2] (and their
    gradients) are ONE contiguous [C1 + C2][Ci] matrix and the pair runs as one GEMM
    (Graph.conv_pair)."""
    names = {id(m): pre for pre, m in owner.named_modules()}
    order = [k for k, _ in owner.named_parameters()]
    for m in owner.modules():
        sib = getattr(m, "siblings", None)
        if not callable(sib):
            continue
        a, b = sib()
        ka, kb = f"{names[id(a)]}.conv.weight", f"{names[id(b)]}.conv.weight"
        if ka in order and kb in order:
            order.remove(kb)
            order.insert(order.index(ka) + 1, kb)
    return order


class Graph:
    """Forward trace of an engine module at one input shape."""

    def __init__(self, owner, N, train, need_grad, layout=None):
        self.owner = owner
        self.N = N
        self.train = train
        self.need_grad = need_grad
        self.ops = []
        self.act_bufs = []
        self.act_size = 0
        self.stats_size = 0
        self.bns = []
        self.slopes = {}
        self.bn_by_mod = {}
        names = {}
        for pre, m in owner.named_modules():
            names[id(m)] = pre
        self.mod_names = names
        self.tensor_names = [k for k, _ in owner.named_parameters()] + \
                            [k for k, _ in owner.named_buffers()]
        self.tslot = {k: S_TENSOR0 + i for i, k in enumerate(self.tensor_names)}
        self.params = dict(owner.named_parameters())
        named = list(self.params)
        # the flat gradient's order: the parameter order, or a Trainer's layout (param_layout)
        self.param_names = list(layout) if layout is not None else named
        if sorted(self.param_names) != sorted(named):
            raise ValueError("parameter layout is not a permutation of the module's parameters")
        self.layout_pos = {k: i for i, k in enumerate(self.param_names)}
        self.param_shapes = {k: tuple(p.shape) for k, p in owner.named_parameters()}
        off = 0
        self.pgrad_off = {}
        for k in self.param_names:
            self.pgrad_off[k] = off
            off += self.params[k].numel()  # packed: the flat grad buffer in layout order
        self.pgrad_size = off
        self.used_params = set()
        # (tensor index of a's weight, of b's weight, a's weight bytes) of every sibling pair
        # emitted as ONE stacked GEMM: the plan reads b's rows through a's pointer, so it is
        # valid only while the two weights stay adjacent (Plan.stacking_holds)
        self.stacked = []

    # -- naming ------------------------------------------------------------------------
    def pname(self, mod, attr):
        pre = self.mod_names[id(mod)]
        return f"{pre}.{attr}" if pre else attr

    def tptr(self, mod, attr):
        return Ptr(self.tslot[self.pname(mod, attr)])

    def gptr(self, mod, attr):
        k = self.pname(mod, attr)
        self.used_params.add(k)
        return Ptr(S_PGRAD, self.pgrad_off[k] * 4)

    def wrep_ptr(self, mod, attr):
        """Replica 0 of a parameter's gradient in the S_WREP arena (L.WREP fp64 replicas of
        the flat gradient, stride pgrad_size doubles); folded into S_PGRAD by OP_SUM_REP."""
        k = self.pname(mod, attr)
        self.used_params.add(k)
        return Ptr(S_WREP, self.pgrad_off[k] * 8)

    # -- allocation ----------------------------------------------------------------------
    def act_buf(self, C, H, W, name):
        b = Buf(S_ACT, self.N, C, H, W, name, off=self.act_size)
        check_elems(b)
        self.act_size += (b.numel + ALIGN - 1) // ALIGN * ALIGN
        self.act_bufs.append(b)
        return b

    def stats_alloc(self, ndouble):
        """An accumulator of `ndouble` values, replicated L.STAT_REP times (isg.h)."""
        off = self.stats_size
        self.stats_size += (ndouble * L.STAT_REP + 7) // 8 * 8
        return off

    def bn_ref(self, bn, count):
        if id(bn) in self.bn_by_mod:
            raise ValueError("a BatchNorm module used twice in one trace is not supported")
        if not isinstance(bn, nn.BatchNorm2d) or bn.momentum is None or not bn.affine \
                or not bn.track_running_stats:
            raise NotImplementedError("BatchNorm2d(affine, momentum, tracked stats) only")
        C = bn.num_features
        stats_off = self.stats_alloc(4 * C)
        coef_off = self.stats_size
        self.stats_size += (4 * C + 7) // 8 * 8
        ref = BNRef(bn, C, count, stats_off, {
            "gamma": self.tptr(bn, "weight"), "beta": self.tptr(bn, "bias"),
            "rm": self.tptr(bn, "running_mean"), "rv": self.tptr(bn, "running_var"),
            "nbt": self.tptr(bn, "num_batches_tracked")},
            fin=knobs.BN_FINAL or count >= knobs.BN_FINAL_COUNT,
            coef_off=coef_off, coef_end=self.stats_size)
        self.bns.append(ref)
        self.bn_by_mod[id(bn)] = ref
        return ref

    def slope_ref(self, prelu):
        if id(prelu) not in self.slopes:
            C = prelu.weight.numel()
            self.slopes[id(prelu)] = SlopeRef(prelu, C, self.stats_alloc(C),
                                              self.tslot[self.pname(prelu, "weight")])
        return self.slopes[id(prelu)]

    def act_of(self, act_mod):
        """(kind, SlopeRef|None) for an activation module of the reference."""
        if act_mod is None or isinstance(act_mod, nn.Identity):
            return "none", None
        if isinstance(act_mod, nn.ReLU):
            return "relu", None
        if isinstance(act_mod, nn.PReLU):
            return "prelu", self.slope_ref(act_mod)
        raise NotImplementedError(f"activation {type(act_mod).__name__} is not on the hot path")

    # -- ops -----------------------------------------------------------------------------
    def input(self, idx, C, H, W, grad):
        b = Buf(S_IN[idx], self.N, C, H, W, f"in{idx}")
        check_elems(b)
        return Value([Val(b, 0, C, grad=grad)])

    def keypoints(self, idx, N, nparts):
        return Keypoints(S_IN[idx], N, nparts)

    def kp_pool(self, kp, k, H, W, out, c0=0):
        """max_pool(k) of the keypoint heatmaps of an H x W image into out[:, c0:c0+parts]."""
        if H % k or W % k:
            raise RuntimeError(f"max_pool{k}: {H}x{W} not divisible")
        self.ops.append(KpPoolOp(self, kp, k, H, W, out, c0))
        return Value([Val(out, c0, kp.nparts, grad=False)])

    def conv(self, conv, x, bn=None, act="none", slope=None, name="", kp=None):
        """nn.Conv2d (dense or depthwise) on value x, optionally followed by BN/act
        applied lazily by the consumer. kp (Keypoints): the conv's input is cat(x, the
        keypoint heatmaps); x feeds the dense conv, the heatmap channels the keypoint
        stem kernels (isg_kp_stem)."""
        k, s, p, d = conv.kernel_size, conv.stride, conv.padding, conv.dilation
        if isinstance(p, str):
            raise NotImplementedError("string padding")
        H, W = x.H, x.W
        OH = (H + 2 * p[0] - d[0] * (k[0] - 1) - 1) // s[0] + 1
        OW = (W + 2 * p[1] - d[1] * (k[1] - 1) - 1) // s[1] + 1
        ckp = kp.nparts if kp is not None else 0
        if x.C + ckp != conv.in_channels:
            raise RuntimeError(f"{name}: expected {conv.in_channels} input channels, got {x.C + ckp}")
        if kp is not None and (conv.groups != 1 or x.grad):
            raise NotImplementedError("keypoint stem: dense conv of an input without gradient only")
        if conv.groups not in (1, conv.in_channels) or (conv.groups > 1 and
                                                         conv.in_channels != conv.out_channels):
            raise NotImplementedError("grouped conv other than depthwise")
        geom = dict(N=self.N, Ci=x.C, H=H, W=W, Co=conv.out_channels, OH=OH, OW=OW,
                    KH=k[0], KW=k[1], SH=s[0], SW=s[1], PH=p[0], PW=p[1], DH=d[0], DW=d[1],
                    groups=conv.groups)
        if kp is not None:
            geom["w_ci"] = conv.in_channels
        out = self.act_buf(conv.out_channels, OH, OW, name)
        bnr = self.bn_ref(bn, self.N * OH * OW) if bn is not None else None
        op = ConvOp(self, "conv", conv, geom, x, out, bnr)
        op.kp = kp
        self.ops.append(op)
        return Value([Val(out, 0, conv.out_channels, bnr, act, slope, grad=self.need_grad)])

    def conv_pair(self, ca, cb, x):
        """Two sibling Conv modules (1x1 conv + BatchNorm + act, segment.py:34-45) on the same
        input x as ONE stacked GEMM: weights [Wa; Wb] (contiguous in a Trainer's parameter
        layout, param_layout), output channels [0, Ca) to a's buffer and [Ca, Ca + Cb) to
        b's through two sinks (own bias and BatchNorm statistics); the backward is one
        K-stacked input gradient (Wa^T ga + Wb^T gb, no ACCUM pass) and one weight gradient
        over the stacked rows. Returns (value_a, value_b), or None when the pair does not
        qualify (then the caller emits two convs): not 1x1 / stride 1 / dense, no BN, or the
        weights not adjacent in the layout AND in memory (a module's own parameters are
        separate tensors)."""
        a, b = ca.conv, cb.conv
        for c in (a, b):
            if not (c.kernel_size == (1, 1) and c.stride == (1, 1) and c.padding == (0, 0)
                    and c.dilation == (1, 1) and c.groups == 1 and c.bias is not None):
                return None
        if a.in_channels != b.in_channels or a.in_channels != x.C:
            return None
        bna, bnb = getattr(ca, "bn", None), getattr(cb, "bn", None)
        if bna is None or bnb is None:
            return None
        ka, kb = self.pname(a, "weight"), self.pname(b, "weight")
        if self.layout_pos[kb] != self.layout_pos[ka] + 1:
            return None
        wa, wb = a.weight, b.weight
        if (wa.device != wb.device or not wa.is_contiguous() or not wb.is_contiguous()
                or wb.data_ptr() != wa.data_ptr() + wa.numel() * wa.element_size()):
            return None
        self.stacked.append((self.tensor_names.index(ka), self.tensor_names.index(kb),
                             wa.numel() * wa.element_size()))
        H, W = x.H, x.W
        geom = dict(N=self.N, Ci=x.C, H=H, W=W, Co=a.out_channels + b.out_channels, OH=H, OW=W,
                    KH=1, KW=1, SH=1, SW=1, PH=0, PW=0, DH=1, DW=1, groups=1)
        outs, vals = [], []
        for cm, c in ((ca, a), (cb, b)):
            out = self.act_buf(c.out_channels, H, W, self.mod_names.get(id(cm), "conv"))
            bnr = self.bn_ref(cm.bn, self.N * H * W)
            kind, slope = self.act_of(cm.act)
            outs.append((c, out, bnr))
            vals.append(Value([Val(out, 0, c.out_channels, bnr, kind, slope, grad=self.need_grad)]))
        self.ops.append(ConvPairOp(self, geom, x, outs))
        return vals[0], vals[1]

    def conv_transpose(self, ct, x, bn=None, act="none", slope=None, name=""):
        k, s, p = ct.kernel_size, ct.stride, ct.padding
        if ct.groups != 1 or ct.dilation != (1, 1) or any(ct.output_padding):
            raise NotImplementedError("convT: groups/dilation/output_padding")
        H, W = x.H, x.W
        OH = (H - 1) * s[0] - 2 * p[0] + k[0]
        OW = (W - 1) * s[1] - 2 * p[1] + k[1]
        geom = dict(N=self.N, Ci=ct.in_channels, H=H, W=W, Co=ct.out_channels, OH=OH, OW=OW,
                    KH=k[0], KW=k[1], SH=s[0], SW=s[1], PH=p[0], PW=p[1], DH=1, DW=1, groups=1)
        out = self.act_buf(ct.out_channels, OH, OW, name)
        if bn is None and ct.bias is not None:
            # the wgrad of a convT runs with swapped roles and cannot sum dY per output
            # channel: consumers' gradient sinks accumulate it here instead
            # (a BN-layout block: sinks add into its sum half, replica stride 4*C)
            out.need_sum = self.stats_alloc(4 * ct.out_channels)
        bnr = self.bn_ref(bn, self.N * OH * OW) if bn is not None else None
        op = ConvOp(self, "convT", ct, geom, x, out, bnr)
        self.ops.append(op)
        return Value([Val(out, 0, ct.out_channels, bnr, act, slope, grad=self.need_grad)])

    def head(self, ct, conv, x, name=""):
        """The mask head (segment.py:435-438, 504-505): ConvTranspose2d(16 -> 4, k8, s4, p2)
        then Conv2d(4 -> 1, 3x3, p1) as ONE fused op (isg_mask_head_*: the 4-channel
        intermediate never reaches HBM), or None when the modules / input do not have
        that exact shape (the caller then emits the two convolutions)."""
        if not (ct.in_channels == 16 and ct.out_channels == 4 and ct.kernel_size == (8, 8)
                and ct.stride == (4, 4) and ct.padding == (2, 2) and ct.groups == 1
                and ct.dilation == (1, 1) and not any(ct.output_padding)
                and conv.in_channels == 4 and conv.out_channels == 1
                and conv.kernel_size == (3, 3) and conv.stride == (1, 1)
                and conv.padding == (1, 1) and conv.dilation == (1, 1) and conv.groups == 1
                and x.C == 16 and all(not s.virtual for s in x.segs)):
            return None
        out = self.act_buf(1, 4 * x.H, 4 * x.W, name)
        # the un-cropped intermediate on the ring outside the image, written by the forward
        # for the backward's 3x3 weight-gradient border term (isg.h isg_mask_head)
        ring = self.act_buf(1, 1, L.head_ring_floats(x.H, x.W), name + ".ring") \
            if self.need_grad else None
        op = HeadOp(self, ct, conv, x, out, ring)
        self.ops.append(op)
        return Value([Val(out, 0, 1, grad=self.need_grad)])

    def maxpool(self, x, k, out=None, c0=0, name=""):
        if x.H % k or x.W % k:
            raise RuntimeError(f"max_pool{k}: {x.H}x{x.W} not divisible (reference needs "
                               "H, W multiples of 16, SURVEY.md §0.5)")
        if out is None:
            out = self.act_buf(x.C, x.H // k, x.W // k, name)
        op = PoolOp(self, x, k, out, c0)
        self.ops.append(op)
        return Value([Val(out, c0, x.C, grad=x.grad)])

    @contextlib.contextmanager
    def side_branch(self):
        """Convolutions (and max-pools) emitted inside run on the executor's side stream in the forward
        pass (an independent residual branch: it reads only values produced before it
        and nothing reads its output until the block's tail), see _fork_branches."""
        n0 = len(self.ops)
        yield
        for op in self.ops[n0:]:
            if not isinstance(op, (ConvOp, PoolOp)):
                raise NotImplementedError("side branch: convolutions and max-pools only")
            op.side = True

    def tail(self, terms, act="none", slope=None, out=None, c0=0, name=""):
        """out = act(sum(terms)); terms = [(Value single-seg, up)]; BN'd terms must have
        act none (the activation of a Conv(act=None), segment.py:42)."""
        C = terms[0][0].C
        H, W = terms[0][0].H * (2 if terms[0][1] else 1), terms[0][0].W * (2 if terms[0][1] else 1)
        for v, up in terms:
            assert len(v.segs) == 1 and v.C == C
            assert v.H * (2 if up else 1) == H and v.W * (2 if up else 1) == W, (v.H, v.W, H, W)
            assert v.segs[0].act == "none"
        if out is None:
            out = self.act_buf(C, H, W, name)
        op = TailOp(self, [(v.segs[0], up) for v, up in terms], act, slope, out, c0)
        self.ops.append(op)
        return Value([Val(out, c0, C, grad=any(v.grad for v, _ in terms))])

    def materialize(self, v, out=None, c0=0, name=""):
        s = v.segs[0]
        assert len(v.segs) == 1
        term = Value([Val(s.buf, s.c0, s.C, s.bn, "none", None, s.grad)])
        return self.tail([(term, False)], s.act, s.slope, out, c0, name)
