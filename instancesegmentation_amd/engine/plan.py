"""Plan: one module at one input shape, traced, scheduled and compiled into the forward and
backward op lists the runtime replays."""
import ctypes
import struct

from .. import _lib as L
from . import knobs
from .graph import Graph
from .ops import HeadOp
from .records import (S_DIN, S_DOUT, S_EXPAVG, S_EXPAVGSQ, S_HYPER, S_OUT, S_OWNER, S_PARAM,
                      S_PGRAD, S_STATS, S_STEP, S_TAILBNU, S_TAILGF, S_WREP, OpList, Ptr, Record)
from .schedule import _fold_tails, _fork_late_wgrads, _trailing_on_main, schedule_forward
from .specs import GradState, bn_final_record
from .values import Buf, Val, Value, _buf_range


def _final_items(g, gs):
    """Finalisation of BN / PReLU / conv-bias-before-BN gradients: [(module, item)]."""
    conv_before = {id(bnr): mod for mod, bnr in gs.bias_from_bn}
    items = []
    # bias of a convT with no BN after it (segment.py:435-436): the per-channel sum
    # of its output gradient, accumulated by the consumers' gradient sinks
    for mod, out, dy in gs.bias_sums:
        items.append((mod, {"slope_acc": Ptr(S_STATS, out.need_sum * 8),
                            "dslope": g.gptr(mod, "bias"), "C": out.C,
                            "slope_stride": 4 * out.C}))
    for b in g.bns:
        it = {"stats": Ptr(S_STATS, b.stats_off * 8), "gamma": b.names["gamma"],
              "running_mean": b.names["rm"], "running_var": b.names["rv"],
              "dgamma": g.gptr(b.mod, "weight"), "dbeta": g.gptr(b.mod, "bias"),
              "C": b.C, "train": 1 if g.train else 0, "count": float(b.count),
              "eps": float(b.mod.eps)}
        if id(b) in conv_before:
            it["dconv_bias"] = g.gptr(conv_before[id(b)], "bias")
        items.append((b.mod, it))
    for sl in g.slopes.values():
        if sl.used_in_bwd:
            items.append((sl.mod, {"slope_acc": Ptr(S_STATS, sl.acc_off * 8),
                                   "dslope": g.gptr(sl.mod, "weight"), "C": sl.C,
                                   "slope_stride": sl.C}))
    return items


class Plan:
    """Compiled forward (+ optional backward) op lists of one module at one shape."""

    def __init__(self, owner, in_shapes, train, need_grad, in_grad, buckets=2, layout=None,
                 fused_tail=False):
        """buckets: gradient buckets of the backward (2: the stem's parameters finalised in a
        second part after the others, for a data-parallel exchange that overlaps the stem
        backward; 1: one part, every finalisation at the end — at world size 1 nothing
        needs bucket 1 early, and the part boundary's side-stream join made the stem's
        input-gradient chain wait ~0.6 ms for the queued weight gradients).
        fused_tail (a training plan with one bucket: the Trainer at world size 1): the
        backward ends in ONE OP_STEP_TAIL record — replica fold, gradient finalisation,
        Adam and the BatchNorm running-stat updates (isg.h isg_step_tail) — instead of the
        fold, the finalisation lists and the forward's BN-update lists; the Adam step
        counter advances in an OP_STEP_INC record forked at the backward's head. Its
        pointers come from slots S_PARAM..S_TAILBNU; the item tables to resolve and upload
        are tail_gf / tail_bnu (Records), the owned gradient ranges tail_owned."""
        self.n_buckets = buckets
        self.fused_tail = bool(fused_tail and train and need_grad and buckets == 1)
        self.tail_gf, self.tail_bnu, self.tail_owned = None, None, []
        g, ins = self._trace(owner, in_shapes, train, need_grad, in_grad, layout)
        _fold_tails(g)
        # a training step's loss accumulator (one double): in the statistics arena, so the
        # forward's memset zeroes it (no separate fill launch before the loss kernel)
        self.loss_off = None
        if train and need_grad:
            self.loss_off = g.stats_size
            g.stats_size += 8
        fw, side_recs = self._build_forward(g)
        schedule_forward(fw, side_recs)
        self.fwd = fw.compile()
        self.act_size = g.act_size
        self.stats_size = max(g.stats_size, 8)
        self.bwd = None
        if need_grad:
            self._build_backward(g, ins)

    def _trace(self, owner, in_shapes, train, need_grad, in_grad, layout):
        """Trace owner.emit into a Graph and route each output into its slot: (g, inputs)."""
        N = in_shapes[0][0]
        g = Graph(owner, N, train, need_grad, layout)
        ins = [g.input(i, s[1], s[2], s[3], in_grad[i]) if len(s) == 4 else
               g.keypoints(i, s[0], s[1]) for i, s in enumerate(in_shapes)]
        outs = owner.emit(g, *ins)
        if isinstance(outs, Value):
            outs = (outs,)
        self.graph = g
        # outputs: materialise each into its output slot
        self.out_bufs = []
        for i, o in enumerate(outs):
            ob = Buf(S_OUT[i], N, o.C, o.H, o.W, f"out{i}")
            head = next((op for op in g.ops if isinstance(op, HeadOp) and len(o.segs) == 1
                         and op.out is o.segs[0].buf and not o.segs[0].virtual), None)
            if head is not None:
                head.out = ob  # the fused head writes the output slot itself (no copy)
            else:
                self._emit_output(g, o, ob)
            self.out_bufs.append(ob)
        self.out_shapes = [(N, b.C, b.H, b.W) for b in self.out_bufs]
        return g, ins

    def _build_forward(self, g):
        """The forward list in trace order, unscheduled, and [(record, byte ranges it
        writes)] of the side-branch ops' records for _fork_branches."""
        train = g.train
        fw = OpList()
        if g.stats_size:
            fw.add(Record(L.OP_MEMSET, L.MemsetRec, {"p": Ptr(S_STATS), "bytes": g.stats_size * 8}))
        if g.need_grad:
            # the weight-gradient replicas (L.WREP fp64 copies of the flat gradient, 34 MB for
            # Segment(20)) are zeroed on the side stream under the forward instead of at the
            # head of the backward's critical path; the forward's final join covers it
            r = Record(L.OP_MEMSET, L.MemsetRec, {"p": Ptr(S_WREP),
                                                  "bytes": L.WREP * g.pgrad_size * 8},
                       label="zero_wgrad_replicas")
            r.flags |= Record.OPF_SIDE | Record.OPF_FORK_NOW
            fw.add(r)
        side_recs = []
        for op in g.ops:
            i0 = len(fw.recs)
            op.fwd(fw)
            for b in op.bnrs:
                if train and b is not None and b.fin:
                    fw.add(bn_final_record([b], False))
            if op.side:
                rng = [_buf_range(op.out)]
                if op.bnr is not None:
                    rng.append((S_STATS, op.bnr.stats_off * 8, op.bnr.coef_end * 8))
                side_recs += [(r, rng) for r in fw.recs[i0:]]
        if train and g.bns:
            items = []
            for b in g.bns:
                items.append({"stats": Ptr(S_STATS, b.stats_off * 8),
                              "running_mean": b.names["rm"], "running_var": b.names["rv"],
                              "num_batches_tracked": b.names["nbt"], "C": b.C,
                              "count": float(b.count), "momentum": float(b.mod.momentum)})
            if self.fused_tail:  # updated by the step tail (the statistics stay intact)
                self.tail_bnu = Record(L.OP_BN_UPDATE, L.ListRec, {"n": len(items)}, L.BnUpdate,
                                       items)
                self.tail_bnu_n = len(items)
                items = []
            # (measured: forked as one side batch at the head of the backward instead, the
            # step was 0.1 ms slower, profiles/r07v_ab_bn_update.txt)
            for i in range(0, len(items), L.LIST_CHUNK):
                chunk = items[i:i + L.LIST_CHUNK]
                fw.add(Record(L.OP_BN_UPDATE, L.ListRec, {"n": len(chunk)}, L.BnUpdate, chunk))
        return fw, side_recs

    def stacking_holds(self, tensors):
        """True while every stacked sibling pair's weights (Graph.stacked) are still adjacent
        in memory in `tensors` (the module's parameters + buffers in named order). Parameters
        rebound after the plan was built (load_state_dict(assign=True), `p.data = ...`, a
        re-flatten) can break that; the caller then rebuilds the plan."""
        for ia, ib, nb in self.graph.stacked:
            wa, wb = tensors[ia], tensors[ib]
            if (wa.device != wb.device or not wa.is_contiguous() or not wb.is_contiguous()
                    or wb.data_ptr() != wa.data_ptr() + nb):
                return False
        return True

    def tail_tables(self, table):
        """The fused tail's item tables with every pointer resolved against `table` (the
        pointer-table array the Trainer runs the plan with): (grad_final items bytes,
        BatchNorm-update items bytes), to upload into the buffers of slots S_TAILGF /
        S_TAILBNU. The Trainer's arenas never move, so this is done once."""
        def resolve(rec):
            if rec is None:
                return b""
            body = bytearray(rec.body)
            for loc, slot, off in rec.fix:
                base = table[slot]
                struct.pack_into("<Q", body, loc, (base + off) if base else 0)
            return bytes(body[ctypes.sizeof(L.ListRec):])
        return resolve(self.tail_gf), resolve(self.tail_bnu)

    def _step_tail(self, g, ol, gf_items):
        """The fused end of the step (fused_tail): the Adam step counter advanced on the side
        stream from the backward's head (the tail's join waits for it), then one
        OP_STEP_TAIL record joining every forked weight gradient."""
        inc = Record(L.OP_STEP_INC, L.StepIncRec, {"step": Ptr(S_STEP)}, label="step_inc")
        inc.flags |= Record.OPF_SIDE | Record.OPF_FORK_NOW
        ol.recs.insert(0, inc)
        self.tail_gf = Record(L.OP_GRAD_FINAL, L.ListRec, {"n": len(gf_items)}, L.GradFinal,
                              gf_items)
        # gradient elements a grad_final item writes (the fold skips them): (offset, count)
        self.tail_owned = []
        for it in gf_items:
            for k in ("dgamma", "dbeta", "dconv_bias", "dslope"):
                v = it.get(k)
                if isinstance(v, Ptr):
                    assert v.slot == S_PGRAD and v.off % 4 == 0
                    self.tail_owned.append((v.off // 4, it["C"]))
        nbnu = self.tail_bnu_n if self.tail_bnu else 0
        r = Record(L.OP_STEP_TAIL, L.StepTail,
                   {"grad": Ptr(S_PGRAD), "rep": Ptr(S_WREP), "n": g.pgrad_size, "nrep": L.WREP,
                    "ngf": len(gf_items), "param": Ptr(S_PARAM), "exp_avg": Ptr(S_EXPAVG),
                    "exp_avg_sq": Ptr(S_EXPAVGSQ), "owner": Ptr(S_OWNER), "step": Ptr(S_STEP),
                    "hyper": Ptr(S_HYPER), "gf": Ptr(S_TAILGF),
                    "bnu": Ptr(S_TAILBNU) if nbnu else None, "nbnu": nbnu},
                   label="step_tail")
        r.flags |= Record.OPF_JOIN  # every forked weight gradient (and the counter) is done
        ol.add(r)

    @staticmethod
    def _late_prefix(g):
        """Module-name prefix of the late gradient bucket: the owner's first child module
        (Segment: `init_conv.`, whose parameters lead the parameter order and whose
        backward runs last), or None when the owner has no children with parameters."""
        for name, child in g.owner.named_children():
            if any(True for _ in child.parameters()):
                return name + "."
            return None
        return None

    def _bucket_split(self, g, gs, recs, late):
        """(cut, split): bucket 2 = the parameters under the late prefix, a leading range
        [0, cut) of the flat gradient; split = the first backward op after which no op
        touches (by any pointer) bucket 1's gradient replicas or the statistics its
        finalisation reads. Returns (0, len(recs)) when no such split exists."""
        if late is None or not g.train or self.n_buckets < 2:
            return 0, len(recs)
        cut = 0
        for k in g.param_names:
            if not k.startswith(late):
                break
            n = 1
            for s in g.param_shapes[k]:
                n *= s
            cut += n
        if any(k.startswith(late) for k in g.param_names[len([1 for k in g.param_names
                                                               if k.startswith(late)]):]):
            return 0, len(recs)  # late parameters are not a leading range
        # statistics ranges (bytes in S_STATS) of bucket-1 modules
        early_stats = []
        for b in g.bns:
            if not g.mod_names[id(b.mod)].startswith(late):
                n = (4 * b.C * L.STAT_REP + 7) // 8 * 8
                early_stats.append((b.stats_off * 8, (b.stats_off + n) * 8))
                early_stats.append((b.coef_off * 8, b.coef_end * 8))
        for sl in g.slopes.values():
            if not g.mod_names[id(sl.mod)].startswith(late):
                early_stats.append((sl.acc_off * 8, (sl.acc_off + sl.C * L.STAT_REP) * 8))
        for mod, out, _ in gs.bias_sums:
            if not g.mod_names[id(mod)].startswith(late):
                early_stats.append((out.need_sum * 8, (out.need_sum + 4 * out.C * L.STAT_REP) * 8))

        def touches_early(r):
            for _, slot, off in r.fix:
                if (slot == S_PGRAD and off >= cut * 4) or (slot == S_WREP and off >= cut * 8):
                    return True
                if slot == S_STATS and any(lo <= off < hi for lo, hi in early_stats):
                    return True
            return False

        split = 0
        for i, r in enumerate(recs):
            if touches_early(r):
                split = i + 1
        return cut, split

    def _emit_output(self, g, o, ob):
        # route the value into the output slot with a tail (copy / BN+act)
        c = 0
        for s in o.segs:
            term = Value([Val(s.buf, s.c0, s.C, s.bn, "none", None, s.grad)])
            g.tail([(term, False)], s.act, s.slope, out=ob, c0=c, name=ob.name)
            c += s.C

    def _backward_body(self, g, gs):
        """Every op's backward in reverse trace order, the weight gradients on the side
        stream."""
        # weight gradients accumulate (fp64 atomics of fp32 workgroup partials: exact, so
        # order-independent, isg.h ISG_WREP) into L.WREP replicas — zeroed by the forward
        # (its side-stream memset) — folded into S_PGRAD by OP_SUM_REP before the BN/PReLU
        # finalisation overwrites its own entries
        body = OpList()
        for op in reversed(g.ops):
            op.bwd(body, gs)
            if g.train and gs.pending_final:
                body.add(bn_final_record(gs.pending_final, True))
                gs.pending_final = []
        for r in body.recs:
            if r.kind in (L.OP_CONV_WGRAD, L.OP_KP_STEM_WGRAD, L.OP_HEAD_FOLD):
                r.flags |= Record.OPF_SIDE  # nothing later in the list reads a weight gradient
        return body

    @staticmethod
    def _close(g, ol, lo, hi, its, side=False):
        """Fold the weight-gradient replicas of parameter range [lo, hi) (floats) and
        finalise the statistics-derived gradients of that range. side: on the side
        stream behind the forked weight gradients (in order after them), forked from
        the main stream here (every statistic is complete), so the stem backward that
        follows overlaps it; the list's final join covers it."""
        recs = []
        if hi > lo:
            recs.append(Record(L.OP_SUM_REP, L.SumRepRec,
                               {"dst": Ptr(S_PGRAD, lo * 4), "src": Ptr(S_WREP, lo * 8),
                                "n": hi - lo, "stride": g.pgrad_size, "nrep": L.WREP},
                               label="sum_wgrad_replicas"))
            if not side:  # every forked weight gradient is in the replicas
                recs[-1].flags |= Record.OPF_JOIN
        for i in range(0, len(its), L.LIST_CHUNK):
            chunk = its[i:i + L.LIST_CHUNK]
            recs.append(Record(L.OP_GRAD_FINAL, L.ListRec, {"n": len(chunk)}, L.GradFinal,
                               chunk))
        for r in recs:
            if side or r.kind == L.OP_GRAD_FINAL:
                # the finalisation lists are independent of each other: forked behind
                # the fold, dealt over both side streams (csrc/exec.cpp), joined at the end
                # of the list (5 launches of ~5 us each ran back to back on the main
                # stream at the very end of the step)
                r.flags |= Record.OPF_SIDE | Record.OPF_FORK_NOW
            ol.add(r)

    def _build_backward(self, g, ins):
        gs = GradState(g)
        for i, ob in enumerate(self.out_bufs):
            gs.external[id(ob)] = Buf(S_DOUT[i], ob.N, ob.C, ob.H, ob.W, f"dout{i}")
        for i, v in enumerate(ins):
            if isinstance(v, Value) and v.grad:
                b = v.segs[0].buf
                gs.external[id(b)] = Buf(S_DIN[i], b.N, b.C, b.H, b.W, f"din{i}")
        body = self._backward_body(g, gs)
        late = self._late_prefix(g)
        _fork_late_wgrads(body.recs, late)
        _trailing_on_main(body.recs)
        self.din_written = [isinstance(v, Value) and v.grad and
                            bool(gs.inited.get(id(v.segs[0].buf))) for v in ins]
        items = _final_items(g, gs)
        cut, split = self._bucket_split(g, gs, body.recs, late)

        def is_late(mod):
            return late is not None and g.mod_names[id(mod)].startswith(late)

        # Two gradient buckets for data parallelism: bucket 1 = parameters
        # [cut, n), final once body[:split] has run; bucket 2 = [0, cut) (the stem, whose
        # backward runs last). The Trainer all-reduces bucket 1 on RCCL's stream while the
        # stem backward (body[split:]) runs. split == len(body): one bucket at the end.
        part1, part2 = OpList(), OpList()
        for r in body.recs[:split]:
            part1.add(r)
        if split < len(body.recs):
            self._close(g, part1, cut, g.pgrad_size, [it for m, it in items if not is_late(m)],
                        side=knobs.side_close())  # opt-in: measured
            # 377.9 -> 376.7 images/s on the side stream (r02h, 3 interleaved pairs)
            for r in body.recs[split:]:
                part2.add(r)
            self._close(g, part2, 0, cut, [it for m, it in items if is_late(m)])
        elif self.fused_tail:
            cut = 0
            self._step_tail(g, part1, [it for _, it in items])
        else:
            cut = 0
            self._close(g, part1, 0, g.pgrad_size, [it for _, it in items])
        bw = OpList()
        for r in part1.recs + part2.recs:
            bw.add(r)
        self.bucket_cut = cut
        self.bwd_parts = [part1.compile()] + ([part2.compile()] if part2.recs else [])
        self.stats_size = max(g.stats_size, 8)
        self.bwd = bw.compile()
        self.grad_size = gs.size
        self.grad_bufs = list(gs.D.values()) + list(gs.G.values())  # for debugging tools
        self.used_params = set(g.used_params)
