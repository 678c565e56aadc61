"""The traced ops. Each writes its forward record(s) with fwd(oplist) and, visited in reverse
order, its backward record(s) with bwd(oplist, GradState)."""
from .. import _lib as L
from . import knobs
from .records import S_GRAD, S_STATS, Ptr, Record
from .specs import bn_spec, fwd_seg, sinks_spec, value_vtensor, vtensor
from .values import Buf, Val, _buf_range


class Op:
    """What the plan and the scheduling passes read off any op."""
    side = False  # Graph.side_branch: the forward runs on the side stream (_fork_branches)
    bnr = None    # BNRef of the BatchNorm behind the op's output

    @property
    def bnrs(self):
        return [self.bnr]

    def x_vtensor(self):
        return value_vtensor(self.g, self.x)


class _ResFold(Op):
    """A residual tail folded into a 1x1 conv (ConvOp) or stacked sibling pair (ConvPairOp):
    read on the input load (res_in; res_mat: this op writes the tail's buffer), run in the
    input gradient's sink (res_tail). _fold_tails sets them."""
    res_in, res_mat, res_tail = None, False, None

    def _fwd_input(self):
        """(input vtensor, factor on the cost's x bytes)."""
        if self.res_in is None:
            return self.x_vtensor(), 1
        # BN'd y and the residual read (+ the output written)
        return self._res_input(), 3 if self.res_mat else 2

    def _dx_sinks(self, gs):
        """The input gradient's sinks: the folded tail's residual sink, or one per segment."""
        rs = self._res_sink(gs) if self.res_tail is not None else None
        return [rs] if rs is not None else gs.sinks(self.x)

    def _res_input(self):
        """The forward input of a folded tail act(BN(y) + x): one BN_FWD segment of y with
        the residual x and the tail's activation, and the tail's buffer as `mat`."""
        g, t = self.g, self.res_in
        (y, _), (r, _) = t.terms
        seg = fwd_seg(Val(y.buf, y.c0, y.C, y.bn, t.act, t.slope), g.train)
        seg["y"] = r.buf.ptr(r.c0)
        seg["y_n_stride"] = r.buf.n_stride
        vt = vtensor([seg], g.N, self.geom["H"], self.geom["W"])
        if self.res_mat:
            vt["mat"] = t.out.ptr()
            vt["mat_n_stride"] = t.out.n_stride
        if r.bn is not None:  # a BatchNorm'd residual: act(BN(y) + BN2(r))
            vt["rbn"] = bn_spec(r.bn, g.train)
        return vt

    def _res_sink(self, gs):
        """The input-gradient sink that also runs the folded tail's backward (isg.h ACTBWD
        residual form), or None when the gradient bookkeeping does not allow it (then the
        tail runs its own backward): dL/d out must be this conv's input gradient plus at
        most what later consumers accumulated over the whole buffer (`old`); the residual
        term's gradient goes out as the second output (p2: STORE when it is the first
        contribution, else ACCUM)."""
        g, t = self.g, self.res_tail
        (y, _), (r, _) = t.terms
        C = t.out.C
        ini = gs.inited.get(id(t.out), set())
        if id(t.out) in gs.external or ini - {(0, C)} or id(y.buf) in gs.G:
            return None
        if r.bn is not None and id(r.buf) in gs.G:
            return None
        gb = gs.alloc(y.buf, "g_" + y.buf.name)
        gs.G[id(y.buf)] = gb
        s = {"p": gb.ptr(), "n_stride": gb.n_stride, "c0": 0, "C": C, "mode": L.SINK_ACTBWD,
             "act": L.ACT[t.act], "y": y.buf.ptr(), "y_n_stride": y.buf.n_stride,
             "bn": bn_spec(y.bn, g.train), "r": r.buf.ptr(r.c0), "r_n_stride": r.buf.n_stride}
        if t.slope is not None:
            t.slope.put(s)
            t.slope.put_grad(s)
        if (0, C) in ini:
            d = gs.dbuf(t.out)
            s["old"] = d.ptr()
            s["old_n_stride"] = d.n_stride
        if r.bn is not None:
            # a BatchNorm'd residual: its BN-output gradient is the same g (the tail's
            # backward gives both BN terms one buffer), its backward sums go to its own stats
            gs.G[id(r.buf)] = gb
            s["rbn"] = bn_spec(r.bn, g.train)
            if r.bn.fin:
                gs.pending_final.append(r.bn)
        elif r.grad:
            db = gs.dbuf(r.buf)
            first = gs.mark(r.buf, r.c0, r.C)
            s["p2"] = db.ptr(r.c0)
            s["p2_n_stride"] = db.n_stride
            s["p2_accum"] = 0 if first else 1
        if y.bn.fin:
            gs.pending_final.append(y.bn)
        t.bwd_folded = True
        return s


class ConvOp(_ResFold):
    def __init__(self, g, kind, mod, geom, x, out, bnr):
        self.g, self.kind, self.mod, self.geom, self.x, self.out, self.bnr = g, kind, mod, geom, x, out, bnr
        self.kp = None

    def _kp_spec(self):
        """isg_kp_stem fields shared by the forward and weight-gradient records."""
        ge = dict(self.geom)
        ge["Ci"] = ge.pop("w_ci")
        return dict(self.kp.spec(), c_kp0=self.x.C, g=ge)

    def _cost(self):
        """(flops, bytes of x, bytes of y, bytes of w) — algorithmic, fp32, each read once."""
        ge = self.geom
        N = ge["N"]
        if self.kind == "convT":
            macs = N * ge["H"] * ge["W"] * ge["Ci"] * ge["Co"] * ge["KH"] * ge["KW"]
        elif ge["groups"] > 1:
            macs = N * ge["OH"] * ge["OW"] * ge["Co"] * ge["KH"] * ge["KW"]
        else:
            macs = N * ge["OH"] * ge["OW"] * ge["Co"] * ge["Ci"] * ge["KH"] * ge["KW"]
        xb = 4 * N * ge["Ci"] * ge["H"] * ge["W"]
        yb = 4 * N * ge["Co"] * ge["OH"] * ge["OW"]
        wb = 4 * self.mod.weight.numel()
        return 2 * macs, xb, yb, wb

    def fwd(self, ops):
        g = self.g
        sink = {"p": self.out.ptr(), "n_stride": self.out.n_stride, "c0": 0, "C": self.out.C,
                "mode": L.SINK_STORE}
        if self.mod.bias is not None:
            sink["bias"] = g.tptr(self.mod, "bias")
        if self.bnr is not None and g.train:
            sink["stats"] = Ptr(S_STATS, self.bnr.stats_off * 8)
        a, xfactor = self._fwd_input()
        rec = {"g": self.geom, "a": a, "w": g.tptr(self.mod, "weight"), "out": sinks_spec([sink])}
        kind = L.OP_CONVT_FWD if self.kind == "convT" else L.OP_CONV_FWD
        fl, xb, yb, wb = self._cost()
        ops.add(Record(kind, L.ConvRec, rec, label=self.out.name, flops=fl,
                       nbytes=xb * xfactor + yb + wb))
        if self.kp is not None:
            ks = dict(self._kp_spec(), w=g.tptr(self.mod, "weight"), y=self.out.ptr(),
                      y_n_stride=self.out.n_stride)
            if self.bnr is not None and g.train:
                ks["stats"] = Ptr(S_STATS, self.bnr.stats_off * 8)
            ops.add(Record(L.OP_KP_STEM_FWD, L.KpStem, ks, label="kp_" + self.out.name,
                           nbytes=2 * yb))

    def bwd(self, ops, gs):
        g = self.g
        ge = self.geom
        dy = gs.dy_seg(self.out, self.bnr, g.train)
        if dy is None:
            return
        fl, xb, yb, wb = self._cost()
        dyb = yb * (2 if dy["xform"] == L.XF_BN_BWD else 1)  # g and y for BN backward
        dyv = vtensor([dy], g.N, ge["OH"], ge["OW"])
        w = g.tptr(self.mod, "weight")
        dw = g.wrep_ptr(self.mod, "weight")
        rep = {"rep_stride": g.pgrad_size, "nrep": L.WREP}
        has_bias = self.mod.bias is not None
        if has_bias and self.bnr is not None:
            gs.bias_from_bn.append((self.mod, self.bnr))
        if (self.kind == "conv" and ge["groups"] > 1 and self.x.grad and self.kp is None
                and len(self.x.segs) == 1 and not knobs.no_dw_fuse()):
            # a depthwise layer's input and weight gradients as ONE op on the main stream
            # (isg_depthwise_bwd: the dy tile staged once; the weight gradient is no
            # side-stream node of its own)
            rec = {"g": ge, "dy": dyv, "w": w, "dx": sinks_spec(gs.sinks(self.x)),
                   "x": self.x_vtensor(), "dw": dw, **rep}
            if has_bias and self.bnr is None:
                rec["dbias"] = g.wrep_ptr(self.mod, "bias")
            ops.add(Record(L.OP_DW_BWD, L.DwBwdRec, rec, label="dx_" + self.out.name,
                           flops=2 * fl, nbytes=2 * dyb + 2 * xb + wb))
            return
        tg = None
        if self.kind == "convT":
            # dx_T = conv(dy_T, W) with the forward conv's stride/pad/kernel
            tg = dict(N=g.N, Ci=ge["Co"], H=ge["OH"], W=ge["OW"], Co=ge["Ci"], OH=ge["H"],
                      OW=ge["W"], KH=ge["KH"], KW=ge["KW"], SH=ge["SH"], SW=ge["SW"],
                      PH=ge["PH"], PW=ge["PW"], DH=1, DW=1, groups=1)
        # ---- input gradient
        if self.x.grad:
            rkind, geo = (L.OP_CONV_FWD, tg) if tg else (L.OP_CONV_DGRAD, ge)
            ops.add(Record(rkind, L.ConvRec,
                           {"g": geo, "a": dyv, "w": w, "out": sinks_spec(self._dx_sinks(gs))},
                           label="dx_" + self.out.name, flops=fl, nbytes=dyb + xb + wb))
        # ---- weight / bias gradient
        if tg:
            rec = {"g": tg, "dy": self.x_vtensor(), "x": dyv, "dw": dw, **rep}
            if has_bias and self.bnr is None:
                gs.bias_sums.append((self.mod, self.out, dy))
        else:
            rec = {"g": ge, "dy": dyv, "x": self.x_vtensor(), "dw": dw, **rep}
            if has_bias and self.bnr is None:
                rec["dbias"] = g.wrep_ptr(self.mod, "bias")
        ops.add(Record(L.OP_CONV_WGRAD, L.WgradRec, rec, label="dw_" + self.out.name, flops=fl,
                       nbytes=dyb + xb + wb))
        if self.kp is not None:
            ops.add(Record(L.OP_KP_STEM_WGRAD, L.KpStem,
                           dict(self._kp_spec(), dy=dyv, dw=dw, **rep),
                           label="dwkp_" + self.out.name))


class ConvPairOp(_ResFold):
    """Two sibling 1x1 convs on one input as one stacked GEMM (Graph.conv_pair)."""

    def __init__(self, g, geom, x, outs):
        self.g, self.geom, self.x, self.outs = g, geom, x, outs  # outs: [(conv, buf, bnr)] x2
        self.label = "+".join(buf.name for _, buf, _ in outs)

    @property
    def bnrs(self):
        return [bnr for _, _, bnr in self.outs]

    def _cost(self, co):
        ge = self.geom
        P = ge["N"] * ge["H"] * ge["W"]
        return 2 * P * co * ge["Ci"], 4 * P * ge["Ci"], 4 * P * co, 4 * co * ge["Ci"]

    def fwd(self, ops):
        g = self.g
        sinks, c0 = [], 0
        for c, buf, bnr in self.outs:
            sk = {"p": buf.ptr(), "n_stride": buf.n_stride, "c0": c0, "C": buf.C,
                  "mode": L.SINK_STORE, "bias": g.tptr(c, "bias")}
            if g.train:
                sk["stats"] = Ptr(S_STATS, bnr.stats_off * 8)
            sinks.append(sk)
            c0 += buf.C
        ge = self.geom
        fl, xb, yb, wb = self._cost(ge["Co"])
        a, xfactor = self._fwd_input()
        ops.add(Record(L.OP_CONV_FWD, L.ConvRec,
                       {"g": ge, "a": a,
                        "w": g.tptr(self.outs[0][0], "weight"), "out": sinks_spec(sinks)},
                       label=self.label, flops=fl, nbytes=xb * xfactor + yb + wb))

    def bwd(self, ops, gs):
        g = self.g
        ge = self.geom
        parts = [(c, buf, bnr, gs.dy_seg(buf, bnr, g.train)) for c, buf, bnr in self.outs]
        live = [p for p in parts if p[3] is not None]
        if not live:
            return
        for c, buf, bnr, _ in live:
            gs.bias_from_bn.append((c, bnr))
        if len(live) == 1:  # one branch reaches the loss: its own conv's weight rows
            c, buf, bnr, dy = live[0]
            segs, w, dwp = [dy], g.tptr(c, "weight"), g.wrep_ptr(c, "weight")
            co = buf.C
        else:
            segs = [p[3] for p in parts]
            w = g.tptr(self.outs[0][0], "weight")
            dwp = g.wrep_ptr(self.outs[0][0], "weight")
            g.wrep_ptr(self.outs[1][0], "weight")  # its rows follow (param_layout)
            co = ge["Co"]
        sg = dict(ge, Co=co)
        fl, xb, yb, wb = self._cost(co)
        dyb = 2 * yb  # g and the saved y of the BatchNorm backward
        dyv = vtensor(segs, g.N, ge["H"], ge["W"])
        label = "+".join(p[1].name for p in live)
        if self.x.grad:
            ops.add(Record(L.OP_CONV_DGRAD, L.ConvRec,
                           {"g": sg, "a": dyv, "w": w, "out": sinks_spec(self._dx_sinks(gs))},
                           label="dx_" + label, flops=fl, nbytes=dyb + xb + wb))
        ops.add(Record(L.OP_CONV_WGRAD, L.WgradRec,
                       {"g": sg, "dy": dyv, "x": self.x_vtensor(),
                        "dw": dwp, "rep_stride": g.pgrad_size, "nrep": L.WREP},
                       label="dw_" + label, flops=fl, nbytes=dyb + xb + wb))


class HeadOp(Op):
    """Fused mask head (Graph.head): one forward and one backward record."""

    def __init__(self, g, ct, conv, x, out, ring=None):
        self.g, self.ct, self.conv, self.x, self.out, self.ring = g, ct, conv, x, out, ring

    def _spec(self):
        g = self.g
        s = {"x": self.x_vtensor(), "w1": g.tptr(self.ct, "weight"),
             "w2": g.tptr(self.conv, "weight"), "N": g.N, "Hi": self.x.H, "Wi": self.x.W}
        if self.ring is not None:
            s["ring"] = self.ring.ptr()
        if self.ct.bias is not None:
            s["b1"] = g.tptr(self.ct, "bias")
        if self.conv.bias is not None:
            s["b2"] = g.tptr(self.conv, "bias")
        return s

    def _cost(self):
        """(flops, bytes) of the forward: convT 2*16*4*64 MAC per input pixel, the 3x3
        2*36 per output pixel; input read once, logits written once."""
        g = self.g
        q = g.N * self.x.H * self.x.W
        p = 16 * q
        return 2 * (16 * 4 * 64 * q + 36 * p), 4 * (16 * q + p)

    def fwd(self, ops):
        s = dict(self._spec(), out=self.out.ptr(), out_n_stride=self.out.n_stride)
        fl, nb = self._cost()
        ops.add(Record(L.OP_HEAD_FWD, L.MaskHead, s, label=self.out.name, flops=fl, nbytes=nb))

    def bwd(self, ops, gs):
        g = self.g
        dy = gs.dy_seg(self.out, None, g.train)
        if dy is None:
            return
        s = dict(self._spec(), dout=dy["p"], dout_n_stride=dy["n_stride"],
                 rep_stride=g.pgrad_size, nrep=L.WREP)
        s["dx"] = sinks_spec(gs.sinks(self.x)) if self.x.grad else {"nsink": 0}
        s["dw1"] = g.wrep_ptr(self.ct, "weight")
        s["dw2"] = g.wrep_ptr(self.conv, "weight")
        if self.ct.bias is not None:
            s["db1"] = g.wrep_ptr(self.ct, "bias")
        if self.conv.bias is not None:
            s["db2"] = g.wrep_ptr(self.conv, "bias")
        # the convT weight gradient's per-workgroup partials go to a slab folded into the
        # replicas by a side-stream op (isg.h isg_mask_head.dw1_part): the kernel's tail was
        # its 4096 fp64 atomics per workgroup
        nslab = L.head_part_floats(g.N, self.x.H, self.x.W)
        if nslab > 0:
            part = gs.alloc(Buf(S_GRAD, 1, 1, 1, nslab, "head_dw1_part"), "head_dw1_part")
            s["dw1_part"] = part.ptr()
        fl, nb = self._cost()
        # algorithmic: input gradient + both weight gradients = 2x the forward (SURVEY
        # §8d). The kernel does not recompute the 4-channel intermediate: the 3x3's weight
        # gradient comes from W1·Z' plus the forward's border ring (isg.h ISG_HEAD_RING).
        ops.add(Record(L.OP_HEAD_BWD, L.MaskHead, s, label="d_" + self.out.name,
                       flops=2 * fl, nbytes=nb + 4 * 16 * g.N * self.x.H * self.x.W))
        if "dw1_part" in s:
            ops.add(Record(L.OP_HEAD_FOLD, L.MaskHead, s, label="fold_" + self.out.name))


class KpPoolOp(Op):
    """max_pool(k) of the keypoint heatmaps (segment.py:31 on the heatmap channels)."""

    def __init__(self, g, kp, k, H, W, out, c0):
        self.g, self.kp, self.k, self.H, self.W, self.out, self.c0 = g, kp, k, H, W, out, c0

    def fwd(self, ops):
        g = self.g
        r = Record(L.OP_KP_POOL, L.KpStem,
                   dict(self.kp.spec(), g={"N": g.N, "H": self.H, "W": self.W}, k=self.k,
                        out=self.out.ptr(self.c0), out_n_stride=self.out.n_stride),
                   label="kp_pool_" + self.out.name,
                   nbytes=4 * g.N * self.kp.nparts * self.out.H * self.out.W)
        r.out_range = _buf_range(self.out)  # for _fork_pools
        ops.add(r)

    def bwd(self, ops, gs):
        return  # keypoints carry no gradient


class PoolOp(Op):
    def __init__(self, g, x, k, out, c0):
        self.g, self.x, self.k, self.out, self.c0 = g, x, k, out, c0

    def fwd(self, ops):
        g = self.g
        r = Record(L.OP_MAXPOOL_FWD, L.PoolRec,
                   {"x": self.x_vtensor(), "k": self.k,
                    "out": self.out.ptr(self.c0), "out_ns": self.out.n_stride},
                   label=self.out.name,
                   nbytes=4 * g.N * self.x.C * (self.x.H * self.x.W + self.out.H * self.out.W))
        r.out_range = _buf_range(self.out)  # for _fork_pools
        ops.add(r)

    def bwd(self, ops, gs):
        g = self.g
        if not self.x.grad or not gs.has_grad(self.out, self.c0, self.x.C):
            return
        d = gs.dbuf(self.out)
        if any(v.virtual for v in self.x.segs):
            raise NotImplementedError("max-pool of a virtual value needs materialisation")
        ops.add(Record(L.OP_MAXPOOL_BWD, L.PoolRec,
                       {"x": self.x_vtensor(), "k": self.k,
                        "dout": d.ptr(self.c0), "dout_ns": d.n_stride,
                        "dx": sinks_spec(gs.sinks(self.x))}, label="dx_" + self.out.name,
                       nbytes=4 * g.N * self.x.C * (2 * self.x.H * self.x.W + self.out.H * self.out.W)))


class TailOp(Op):
    # set by _fold_tails / _ResFold._res_sink: the reader of the output runs this tail's
    # forward on its input load / its backward in its input-gradient sink
    fwd_folded = bwd_folded = False

    def __init__(self, g, terms, act, slope, out, c0):
        self.g, self.terms, self.act, self.slope, self.out, self.c0 = g, terms, act, slope, out, c0

    def spec(self):
        g = self.g
        C = self.terms[0][0].C
        t = {"term": [fwd_seg(v, g.train) for v, _ in self.terms],
             "up": [1 if up else 0 for _, up in self.terms], "nterm": len(self.terms),
             "act": L.ACT[self.act], "out": self.out.ptr(self.c0),
             "out_n_stride": self.out.n_stride, "N": g.N, "C": C, "H": self.out.H,
             "W": self.out.W}
        if self.slope is not None:
            self.slope.put(t)
        return t

    def fwd(self, ops):
        if self.fwd_folded:
            return  # the next 1x1 conv computes and writes the output (_fold_tails)
        ops.add(Record(L.OP_TAIL_FWD, L.Tail, self.spec(), label=self.out.name))

    def bwd(self, ops, gs):
        g = self.g
        C = self.terms[0][0].C
        if self.bwd_folded:
            return  # done in the consumer's input-gradient sink (ConvOp._res_sink)
        if not gs.has_grad(self.out, self.c0, C):
            return
        d = gs.dbuf(self.out)
        rec = {"f": self.spec(), "dout": d.ptr(self.c0), "dout_n_stride": d.n_stride}
        if self.slope is not None:
            self.slope.put_grad(rec)
        if any(v.bn is not None for v, _ in self.terms):
            gb = gs.alloc(Buf(S_GRAD, g.N, C, self.out.H, self.out.W, "gt"), "gt_" + self.out.name)
            rec["g"] = gb.ptr()
            rec["g_n_stride"] = gb.n_stride
            for v, _ in self.terms:
                if v.bn is not None:
                    assert v.c0 == 0 and v.C == v.buf.C
                    assert id(v.buf) not in gs.G
                    gs.G[id(v.buf)] = gb
                    if v.bn.fin:
                        gs.pending_final.append(v.bn)
        dterm, dns, dacc = [None] * 3, [0] * 3, [0] * 3
        for i, (v, up) in enumerate(self.terms):
            if v.bn is None and v.grad:
                if v.buf.need_sum is not None:
                    raise NotImplementedError("tail term that needs a bias-gradient sum")
                db = gs.dbuf(v.buf)
                first = gs.mark(v.buf, v.c0, v.C)
                dterm[i] = db.ptr(v.c0)
                dns[i] = db.n_stride
                dacc[i] = 0 if first else 1
        rec["dterm"] = dterm
        rec["dterm_n_stride"] = dns
        rec["dterm_accum"] = dacc
        ops.add(Record(L.OP_TAIL_BWD, L.TailGrad, rec, label="d_" + self.out.name))
