"""The engine's environment switches, each read at the moment it always was: the first three
once at import (tests patch the module attribute, so read them as knobs.NAME, never
`from .knobs import NAME`), the last three every time a plan is built.

  ISG_BN_FINAL=1        one OP_BN_FINAL launch per BatchNorm point (below)
  ISG_BN_FINAL_COUNT=n  ... only at points normalising >= n values (below)
  ISG_FORK_DELAY=0|1|2  schedule._delay_forks: 0 off, 1 the first fork group, 2 all
  ISG_NO_TAIL_FOLD=1    schedule._fold_tails off: every residual tail is its own launch
  ISG_NO_DW_FUSE=1      ConvOp.bwd: a depthwise layer's input and weight gradients as two ops
  ISG_SIDE_CLOSE=1      Plan._build_backward: bucket 1 closed on the side stream
"""
import os

# BatchNorm coefficients. Default: every consumer evaluates them from the replicated fp64
# statistics itself (isg_bn.coef NULL; ISG_STAT_REP = 4 replicas, i.e. 8-16 loads per
# channel per workgroup), so no launch sits between a producer and its consumers.
# Measured on the bench step (profiles/r03h_bn_ab.txt, 2 x 200 steps each): 5.16 ms with
# one OP_BN_FINAL launch per BN point (140 per step, 16 replicas), 4.71 ms without them at
# 4 replicas (2 replicas 4.92: atomic contention in the producers; 8 replicas 4.82: more
# consumer reads; 16 replicas +0.8 ms, round 2). ISG_BN_FINAL=1 restores the launches.
BN_FINAL = os.environ.get("ISG_BN_FINAL", "0") == "1"
# ISG_BN_FINAL_COUNT=n keeps one OP_BN_FINAL launch at BN points normalising >= n values
# (N*H*W). Default: none. (131072 — the stem and the 256^2 decoder — paid while thin_pw ran
# one-wave workgroups whose statistics atomics and reads piled on the same lines; after its
# four-wave form all-consumer-side measured 4.39 vs 4.41 ms/step, profiles/r03u_ab.txt.)
BN_FINAL_COUNT = int(os.environ.get("ISG_BN_FINAL_COUNT", str(1 << 62)))

FORK_DELAY = os.environ.get("ISG_FORK_DELAY", "1")  # 0 off, 1 the first fork group, 2 all


def no_tail_fold():
    return os.environ.get("ISG_NO_TAIL_FOLD", "0") == "1"


def no_dw_fuse():
    return os.environ.get("ISG_NO_DW_FUSE", "0") == "1"


def side_close():
    return os.environ.get("ISG_SIDE_CLOSE", "0") == "1"
