"""Passes over a traced graph or a finished record list: residual tails folded into their
readers (_fold_tails, before any record exists), forward forks and joins
(schedule_forward), the backward's late forks (_fork_late_wgrads, _trailing_on_main).
A fork is a Record flag; what a join waits for is Record.join_deps."""
from .. import _lib as L
from . import knobs
from .ops import ConvOp, ConvPairOp, TailOp
from .records import S_ACT, Record


def _fork_pools(ol):
    """Max-pool forwards (and the keypoint heatmaps' pool) depend only on their input and
    nothing writes what they read or produce until their first consumer: fork each onto
    the executor's side stream and join right before the first later op that touches its
    output buffer (out_range = the whole buffer, _buf_range)."""
    recs = ol.recs
    pool = lambda r: r.kind in (L.OP_MAXPOOL_FWD, L.OP_KP_POOL) and r.out_range is not None
    for i, r in enumerate(recs):
        if not pool(r):
            continue
        slot, lo, hi = r.out_range
        for j in range(i + 1, len(recs)):
            # a pool right behind it into the same buffer (the stem's RGB max-pool and the
            # heatmaps' pool write disjoint channel slices of init_down) follows it on the
            # side stream: not a reader to join before
            if j == i + 1 and pool(recs[j]) and recs[j].out_range == r.out_range:
                continue
            if any(fs == slot and lo <= off < hi for _, fs, off in recs[j].fix):
                if j > i + 1:  # something to overlap with
                    r.flags |= Record.OPF_SIDE | Record.OPF_FORK_NOW
                    recs[j].flags |= Record.OPF_JOIN
                    _join_dep(recs[j], r)
                break


def _fork_branches(ol, side_recs):
    """Forward records of side-branch convolutions (Graph.side_branch) run on the
    executor's side stream, each forked at its place in the list (OPF_FORK_NOW: the side
    stream waits for everything issued on the main stream so far, i.e. the branch
    input). The first later main-stream record that reads any byte the branch writes —
    its output or its BN statistics/coefficients — joins the side stream. Forward only:
    backward sinks accumulate into shared gradient buffers."""
    if not side_recs:
        return
    recs = ol.recs
    pos = {id(r): i for i, r in enumerate(recs)}
    for r, ranges in side_recs:
        r.flags |= Record.OPF_SIDE | Record.OPF_FORK_NOW
    side_ids = {id(r) for r, _ in side_recs}
    for r, ranges in side_recs:
        for j in range(pos[id(r)] + 1, len(recs)):
            if id(recs[j]) in side_ids:
                continue
            if any(fs == slot and lo <= off < hi for _, fs, off in recs[j].fix
                   for slot, lo, hi in ranges):
                recs[j].flags |= Record.OPF_JOIN
                _join_dep(recs[j], r)
                break


def _join_dep(rec, side_rec):
    """Remember which forked record a join waits for (_join_exclusions)."""
    if rec.join_deps is None:
        rec.join_deps = set()
    rec.join_deps.add(id(side_rec))


def _join_exclusions(recs):
    """Narrow every join to the side work it depends on: a join made by _fork_pools /
    _fork_branches waits only for the side records up to the LAST one it reads (in list
    order), not for side records forked after that one — the executor's join would
    otherwise cover the side stream's whole tail, e.g. bottle1_1's 2x2 conv waiting for its
    own forked residual branch (pool + convm) when it only reads the stem's pools. The
    count of excluded (later) side records goes into the header flags' upper bits
    (csrc/exec.cpp ISG_OPF_JOIN, SideSched::join_upto); joins without recorded dependencies wait for everything."""
    order = []
    for r in recs:
        if r.flags & Record.OPF_JOIN:
            r.flags &= (1 << Record.EXCL_SHIFT) - 1
            deps = r.join_deps
            pos = {i: k for k, i in enumerate(order)}
            if deps and all(d in pos for d in deps):
                excl = len(order) - 1 - max(pos[d] for d in deps)
                r.flags |= min(excl, Record.EXCL_MAX) << Record.EXCL_SHIFT
        if r.flags & Record.OPF_SIDE:
            order.append(id(r))


def _delay_forks(ol):
    """Capture a forward fork group behind the main-stream record that follows it (unless
    that record joins it). The graph runtime dispatches nodes in capture order and a node
    that waits on another queue waits for everything already dispatched there: with the
    side work captured first, the main stream's next node (at the step's start: the stem's
    first conv behind the replica memset and both stem pools) waited for the whole group
    (kernel trace: 40 us of the stem chain's start). Delaying a group only adds one main-
    stream dependency to it; nothing a main record between fork and join reads is written
    by the group (the join sits at its first reader, _fork_pools / _fork_branches)."""
    if knobs.FORK_DELAY == "0":
        return
    recs, out, i, done = ol.recs, [], 0, False
    while i < len(recs):
        r = recs[i]
        if not r.flags & Record.OPF_SIDE or (done and knobs.FORK_DELAY == "1"):
            out.append(r)
            i += 1
            continue
        j = i
        while j < len(recs) and recs[j].flags & Record.OPF_SIDE:
            j += 1
        done = True
        if j < len(recs) and not recs[j].flags & Record.OPF_JOIN:
            out.append(recs[j])
            out += recs[i:j]
            i = j + 1
        else:
            out += recs[i:j]
            i = j
    recs[:] = out


def schedule_forward(ol, side_recs):
    """Every forward pass, in the order they depend on each other: fork the pools and the
    side branches (side_recs: [(record, byte ranges it writes)]), move fork groups behind
    the next main record, then count each join's exclusions over the final order."""
    _fork_pools(ol)
    _fork_branches(ol, side_recs)
    _delay_forks(ol)
    _join_exclusions(ol.recs)


def _fork_late_wgrads(recs, late):
    """The executor defers side-stream weight gradients in batches until a join; at the end
    of the backward that parks the last batch (and the stem's own weight gradients, whose
    dy is ready before the stem's input-gradient chain runs) behind the whole stem chain.
    Fork the pending batch where the stem's backward begins, and each stem weight gradient
    at its place (OPF_FORK_NOW), so they overlap the stem's input-gradient kernels."""
    if not late:
        return
    tag = late.rstrip(".")
    first_late = next((i for i, r in enumerate(recs) if tag in r.label), None)
    if first_late is None:
        return
    prev = [r for r in recs[:first_late] if r.flags & Record.OPF_SIDE]
    if prev:
        prev[-1].flags |= Record.OPF_FORK_NOW
    for r in recs[first_late:]:
        if r.flags & Record.OPF_SIDE:
            r.flags |= Record.OPF_FORK_NOW
    # a stem weight gradient right behind its own input gradient moves in front of it: its
    # operands (dy, the forward input) are ready, so it forks before that kernel instead of
    # behind it (a weight gradient reads nothing the input gradient writes)
    for i in range(first_late, len(recs) - 1):
        a, b = recs[i], recs[i + 1]
        if (a.kind == L.OP_CONV_DGRAD and b.kind == L.OP_CONV_WGRAD and a.label.startswith("dx_")
                and b.label == "dw_" + a.label[3:]):
            recs[i], recs[i + 1] = b, a


def _trailing_on_main(recs):
    """Side records after the backward's last main-stream record (the stem's layer-1 weight
    gradients, behind the last input gradient) overlap nothing on the main stream, which then
    only waits at the final join, while on the side stream they queue behind every weight
    gradient forked before them: run them on the main stream instead (round 6 kernel trace:
    the main stream idled 161 us before the step tail)."""
    i = len(recs)
    while i > 0 and recs[i - 1].flags & Record.OPF_SIDE:
        i -= 1
    for r in recs[i:]:
        r.flags &= ~(Record.OPF_SIDE | Record.OPF_FORK_NOW)


def _fold_tails(g):
    """Residual tails folded into their first consumer: a tail
    out = act(BN(y) + x) (segment.py:75-77, 107-109, 259: BatchNorm'd raw conv output plus a
    materialised value, no upsampling) whose output is read FIRST by the very next op, a
    1x1 stride-1 conv on exactly that value, stops being a launch of its own:
      forward  — the conv reads act(BN(y) + x) on load (isg_vseg residual form) and its
                 first row block writes the materialised output on the way (vtensor.mat),
                 which every later reader (the next tail's residual term, skips, the
                 weight gradient) still finds in the tail's buffer;
      backward — the conv's input gradient, the last contribution to dL/d out, carries the
                 tail's backward in its sink (ACTBWD residual form: + the gradient already
                 accumulated for out, act' at BN(y) + x, BatchNorm-backward sums of y, the
                 PReLU slope gradient, and the residual term's gradient as a second
                 output), decided in ConvOp.bwd (falls back to the tail's own launch when
                 the gradient bookkeeping does not allow it).
    Train mode, and forward-only eval plans (infer: the BN-folded network's tails add a
    plain conv output, read as an identity-BN segment with the tail's activation);
    ISG_NO_TAIL_FOLD=1 off."""
    if knobs.no_tail_fold() or (not g.train and g.need_grad):
        return
    ops = g.ops
    for i, t in enumerate(ops):
        if not isinstance(t, TailOp) or len(t.terms) != 2:
            continue
        (y, upy), (r, upr) = t.terms
        C = t.out.C
        # the residual: a materialised value, or a second BatchNorm'd conv output (the
        # BottleneckDown2 / BottleneckDim_Res tails, segment.py:147-148, 202-207)
        r_ok = not r.virtual or (g.train and r.bn is not None and r.act == "none" and r.c0 == 0
                                 and r.C == r.buf.C and r.buf is not y.buf)
        # y: a BatchNorm'd raw conv output, or (BN folded into the conv) a plain one under
        # the tail's activation (the residual form is a BN_FWD segment either way)
        y_ok = y.act == "none" and (y.bn is not None or (not y.virtual and t.act != "none"))
        if upy or upr or not y_ok or not r_ok or t.c0 != 0:
            continue
        if t.out.slot != S_ACT or y.C != C or r.C != C or y.c0 != 0 or y.buf.C != C:
            continue
        if (t.out.H * t.out.W) % 4 or C % 4 or C > 128:
            continue
        # the side-branch ops forked right after the tail (BottleneckUp_Res's conv2,
        # segment.py:230-236, reads the block input beside the main chain): each one either
        # does not read the tail's output or is a 1x1 conv folding the tail on its own load
        # (no materialised output); then the main-stream 1x1 that writes it
        side = []
        j = i + 1
        while j < len(ops) and ops[j].side:
            if any(v.buf is t.out for v in ops[j].x.segs):
                side.append(ops[j])
            j += 1
        if j >= len(ops) or not all(_fold_reader_ok(o, t) for o in side + [ops[j]]):
            continue
        if r.virtual and isinstance(ops[j], ConvPairOp):
            continue  # the residual's own BatchNorm needs one sink (pw_gemm.hip host check)
        c = ops[j]
        t.fwd_folded = True
        for o in side:
            o.res_in, o.res_mat = t, False
        c.res_in, c.res_mat = t, True
        # the backward: the first reader's input gradient is the last contribution
        (side[0] if side else c).res_tail = t


def _fold_reader_ok(c, t):
    """A reader of a residual tail's output that can take the tail's forward on its input
    load (and, as the last gradient contributor, its backward in the input-gradient sink):
    a dense 1x1 stride-1 conv, or a stacked sibling pair of them (Graph.conv_pair), on exactly
    that value (pw_gemm.hip: 16-B rows, K, M <= 128)."""
    if not isinstance(c, (ConvOp, ConvPairOp)):
        return False
    ge = c.geom
    if isinstance(c, ConvOp) and not (c.kind == "conv" and c.kp is None):
        return False
    if not (ge["KH"] == 1 and ge["KW"] == 1 and ge["SH"] == 1 and ge["SW"] == 1
            and ge["PH"] == 0 and ge["PW"] == 0 and ge["DH"] == 1 and ge["DW"] == 1
            and ge["groups"] == 1 and "w_ci" not in ge):
        return False
    if len(c.x.segs) != 1:
        return False
    xv = c.x.segs[0]
    if xv.buf is not t.out or xv.c0 != 0 or xv.C != t.out.C or xv.virtual:
        return False
    return ge["Co"] <= 128 and ge["Co"] % 4 == 0
