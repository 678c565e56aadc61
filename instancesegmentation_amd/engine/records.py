"""The record and blob format the native executor reads (include/isg.h, csrc/exec.cpp):
pointer-table slots, symbolic pointers, one Record per launch, an OpList per pass."""
import copy
import ctypes
import struct

from .. import _lib as L

# fixed pointer-table slots
S_ACT, S_GRAD, S_STATS, S_PGRAD, S_LOSS, S_TARGET = 0, 1, 2, 3, 4, 5
S_IN = (6, 7)
S_OUT = (8, 9)
S_DOUT = (10, 11)
S_DIN = (12, 13)
S_WREP = 14  # L.WREP fp64 replicas of the flat parameter gradient (wgrad atomics, isg.h)
S_STAMP = 15  # timestamp buffer of OP_STAMP records (isg_stamp: uint32 counter, then slots)
# the fused step tail (Plan fused_tail, isg.h isg_step_tail): the Trainer's flat parameters,
# Adam moments, per-element owner mask, device step counter, hyperparameters (5 doubles) and
# the device tables of its grad_final / BatchNorm-update items
S_PARAM, S_EXPAVG, S_EXPAVGSQ, S_OWNER, S_STEP, S_HYPER, S_TAILGF, S_TAILBNU = range(16, 24)
S_TENSOR0 = 24

ALIGN = 64  # elements (256 B) between arena buffers


class Ptr:
    __slots__ = ("slot", "off")

    def __init__(self, slot, off=0):
        self.slot = slot
        self.off = off

    def plus(self, nbytes):
        return Ptr(self.slot, self.off + nbytes)


# ---------------------------------------------------------------------------------
# record building
def _fill(obj, spec, base, fix):
    for k, v in spec.items():
        fld = getattr(type(obj), k)
        off = base + fld.offset
        if v is None:
            continue
        if isinstance(v, Ptr):
            fix.append((off, v.slot, v.off))
        elif isinstance(v, dict):
            _fill(getattr(obj, k), v, off, fix)
        elif isinstance(v, (list, tuple)):
            arr = getattr(obj, k)
            esz = ctypes.sizeof(arr._type_)
            for i, e in enumerate(v):
                if e is None:
                    continue
                if isinstance(e, dict):
                    _fill(arr[i], e, off + i * esz, fix)
                elif isinstance(e, Ptr):
                    fix.append((off + i * esz, e.slot, e.off))
                else:
                    arr[i] = e
        else:
            setattr(obj, k, v)


class Record:
    OPF_SIDE, OPF_JOIN, OPF_FORK_NOW = 1, 2, 4  # executor header flags (csrc/exec.cpp)
    # a join's count of the most recent side records it does NOT wait for (_join_exclusions)
    EXCL_SHIFT, EXCL_MAX = 8, (1 << 20) - 1

    def __init__(self, kind, cls, spec, items_cls=None, items=None, label="", flops=0, nbytes=0):
        self.kind = kind
        self.flags = 0
        self.label = label
        self.flops = flops    # algorithmic FLOPs of this launch (2*MAC)
        self.nbytes = nbytes  # algorithmic HBM bytes (each operand read/written once)
        # a pool's (slot, lo, hi) bytes of its whole output buffer (PoolOp / KpPoolOp.fwd set
        # it, schedule._fork_pools joins before the first record that points into it)
        self.out_range = None
        # ids of the forked records a join waits for (schedule._join_dep sets, _join_exclusions
        # and OpList.stamped read); None: the join waits for everything
        self.join_deps = None
        rec = cls()
        fix = []
        _fill(rec, spec, 0, fix)
        body = bytes(rec)
        if items_cls is not None:
            parts = [body]
            isz = ctypes.sizeof(items_cls)
            for i, it in enumerate(items):
                o = items_cls()
                _fill(o, it, len(body) + i * isz, fix)
                parts.append(bytes(o))
            body = b"".join(parts)
        self.body = body
        self.fix = fix

    def pack(self):
        n = len(self.body)
        pad = (-n) % 8
        out = [struct.pack("<iiii", self.kind, n, len(self.fix), self.flags), self.body,
               b"\0" * pad]
        out += [struct.pack("<iiq", loc, slot, off) for loc, slot, off in self.fix]
        return b"".join(out)


class OpList:
    def __init__(self):
        self.recs = []

    def add(self, rec):
        self.recs.append(rec)

    def compile(self):
        self.blob = b"".join(r.pack() for r in self.recs)
        self._buf = ctypes.create_string_buffer(self.blob, len(self.blob))
        return self

    def run(self, table, stream, side=None, side2=None):
        if side is None:
            L.check(L.lib().isg_exec(ctypes.addressof(self._buf), len(self.recs), table, stream),
                    "exec")
        else:
            L.check(L.lib().isg_exec_ms2(ctypes.addressof(self._buf), len(self.recs), table,
                                         stream, side, side2), "exec")

    def slice(self, i, j):
        """A compiled sub-list recs[i:j] (to bracket one op with events)."""
        o = OpList()
        o.recs = self.recs[i:j]
        return o.compile()

    def stamped(self, idx):
        """A compiled copy with OP_STAMP records (isg_stamp into slot S_STAMP) on the main
        stream: a calibration pair first (two stamps back to back, slot 1: what a bracket
        costs without an op), then one right before and one right after record `idx` (slot
        0) — the op timed where it runs in the step, side streams and all, without cutting
        the list."""
        from .schedule import _join_exclusions  # schedule imports this module

        def stamp(slot, sign):
            return Record(L.OP_STAMP, L.StampRec, {"buf": Ptr(S_STAMP), "slot": slot,
                                                   "sign": sign}, label="stamp")
        op = copy.copy(self.recs[idx])
        before = stamp(0, -1)
        # a join the op carries happens before its first stamp; a side-stream op (a weight
        # gradient) is timed on the main stream
        # (with its exclusion count: the stamp adds no side record)
        before.flags = op.flags & (Record.OPF_JOIN | (Record.EXCL_MAX << Record.EXCL_SHIFT))
        was_side = op.flags & Record.OPF_SIDE
        op.flags = 0
        o = OpList()
        o.recs = [stamp(1, -1), stamp(1, 1)] + self.recs[:idx] + [before, op, stamp(0, 1)] + \
            self.recs[idx + 1:]
        if was_side:  # one side record fewer: recount (a join on the moved op waits for all)
            new = {id(r): copy.copy(r) for r in o.recs}
            for r in new.values():
                if r.join_deps:
                    r.join_deps = {id(new[d]) for d in r.join_deps if d in new}
            o.recs = [new[id(r)] for r in o.recs]
            _join_exclusions(o.recs)
        return o.compile()
