"""Fingerprint of everything the engine hands the executor, over a matrix of small plans
(CPU only): per compiled list the record count, the sha256 of its blob and a sha256 over the
records' (kind, flags, label, flops, nbytes); then the plan's sizes. Two trees whose output
is identical, line for line, build the same plans.

    python tools/plan_fingerprint.py > fingerprint.txt
"""
import argparse
import hashlib
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from instancesegmentation_amd import _lib as L  # noqa: E402
from instancesegmentation_amd.engine import Plan, param_layout  # noqa: E402
from instancesegmentation_amd.model.segment import (BottleneckDim_Res, BottleneckDown2,  # noqa: E402
                                                    Segment)
from instancesegmentation_amd.runtime import EngineModule  # noqa: E402
from instancesegmentation_amd.train import flatten_module  # noqa: E402

KP = [(2, 3, 128, 128), (2, 17, 3)]
# the flattened buckets=2 plan under each switch, one fresh process each (three are read at
# import)
SWITCHES = ("ISG_NO_TAIL_FOLD=1", "ISG_NO_DW_FUSE=1", "ISG_SIDE_CLOSE=1", "ISG_FORK_DELAY=0",
            "ISG_FORK_DELAY=2", "ISG_BN_FINAL=1", "ISG_BN_FINAL_COUNT=32768")


class _Down2ThenDimRes(EngineModule):
    """tests/test_host_cpu.py: a two-BatchNorm tail read by a stacked sibling pair."""

    def __init__(self):
        super().__init__()
        self.down = BottleneckDown2(16, 8, 32)
        self.dimres = BottleneckDim_Res(32, 8, 48, True)

    def emit(self, g, x):
        y, _ = self.down.emit(g, x)
        return self.dimres.emit(g, y)


def sha(b):
    return hashlib.sha256(b).hexdigest()


def list_line(tag, name, ol):
    cost = repr([(r.kind, r.flags, r.label, r.flops, r.nbytes) for r in ol.recs]).encode()
    print(f"{tag} {name} n={len(ol.recs)} blob={sha(ol.blob)} cost={sha(cost)}")


def fingerprint(tag, p):
    list_line(tag, "fwd", p.fwd)
    if p.bwd is not None:
        list_line(tag, "bwd", p.bwd)
        for i, part in enumerate(p.bwd_parts):
            list_line(tag, f"bwd_parts[{i}]", part)
    for k in ("act_size", "stats_size", "grad_size", "loss_off", "bucket_cut", "out_shapes",
              "din_written"):
        print(f"{tag} {k}={getattr(p, k, None)!r}")  # a forward-only plan has no grad_size
    print(f"{tag} used_params={sha(repr(sorted(getattr(p, 'used_params', ()))).encode())} "
          f"n={len(getattr(p, 'used_params', ()))}")
    print(f"{tag} stacked={p.graph.stacked!r}")
    if p.fused_tail:
        for k in ("tail_gf", "tail_bnu"):
            r = getattr(p, k)
            print(f"{tag} {k} body={sha(r.body)} fix={sha(repr(r.fix).encode())}")
        print(f"{tag} tail_owned={sha(repr(p.tail_owned).encode())} n={len(p.tail_owned)}")


def flat(m):
    lay = param_layout(m)
    flatten_module(m, "cpu", order=lay)
    return lay


def flat_plan(**kw):
    m = Segment(20)
    return Plan(m, KP, True, True, (False, False), layout=flat(m), **kw)


def matrix():
    for b in (2, 1):
        fingerprint(f"seg20_kp128_b{b}", Plan(Segment(20), KP, True, True, (False, False),
                                              buckets=b))
    for b in (2, 1):
        fingerprint(f"seg20_kp128_flat_b{b}", flat_plan(buckets=b))
    ft = flat_plan(buckets=1, fused_tail=True)
    fingerprint("seg20_kp128_flat_b1_fused", ft)
    fingerprint("seg20_kp64_n1", Plan(Segment(20), [(1, 3, 64, 64), (1, 17, 3)], True, True,
                                      (False, False)))
    dense = [(2, 3, 64, 64), (2, 17, 64, 64)]
    for ig in ((False, False), (True, False)):
        fingerprint(f"seg20_dense64_din{int(ig[0])}", Plan(Segment(20), dense, True, True, ig))
    fingerprint("seg3_128", Plan(Segment(3), [(2, 3, 128, 128)], True, True, (False,)))
    fingerprint("seg20_kp128_infer", Plan(Segment(20), KP, False, False, (False, False)))
    fingerprint("seg20_kp128_eval_grad", Plan(Segment(20), KP, False, True, (False, False)))
    m = _Down2ThenDimRes()
    fingerprint("down2_dimres_flat", Plan(m, [(2, 16, 32, 32)], True, True, (False,),
                                          layout=flat(m)))
    fingerprint("down2_dimres", Plan(_Down2ThenDimRes(), [(2, 16, 32, 32)], True, True,
                                     (False,)))
    # the stamped copies (a main-stream record; a side-stream one: the recount) and a slice
    main = next(i for i, r in enumerate(ft.bwd.recs) if r.kind == L.OP_CONV_DGRAD
                and not r.flags & 1)
    side = next(i for i, r in enumerate(ft.bwd.recs) if r.kind == L.OP_CONV_WGRAD
                and r.flags & 1)
    list_line("fused", f"bwd.stamped({main})", ft.bwd.stamped(main))
    list_line("fused", f"bwd.stamped({side})", ft.bwd.stamped(side))
    list_line("fused", "bwd.slice(10,20)", ft.bwd.slice(10, 20))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--switch", help="(internal) print the flattened buckets=2 plan under this tag")
    a = ap.parse_args()
    if a.switch:
        fingerprint(a.switch, flat_plan(buckets=2))
        return
    matrix()
    sys.stdout.flush()
    for sw in SWITCHES:
        k, v = sw.split("=")
        env = {e: x for e, x in os.environ.items() if e not in {s.split("=")[0] for s in SWITCHES}}
        subprocess.run([sys.executable, os.path.abspath(__file__), "--switch", sw],
                       env=dict(env, **{k: v}), check=True)


if __name__ == "__main__":
    main()
