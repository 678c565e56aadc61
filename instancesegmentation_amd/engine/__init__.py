"""Static-schedule engine: turns a module's `emit` description into two recorded op
lists (forward, backward) for the native executor `isg_exec` (include/isg.h).

Why: the reference runs ~300 forward and ~600 backward eager kernels per step, each
launched from Python (segment.py:44-45 is conv -> bn -> act as three kernels). Here
a module is traced once per input shape into a list of fused-op records whose
pointers are symbolic (slot, byte offset); a call replays the list with one ctypes
call and a fresh pointer table, and the same list can be captured into a HIP graph.

Values flowing between ops are *virtual tensors*: a raw conv output plus the
BatchNorm/activation its consumer applies on load (Conv.forward, segment.py:44-45),
possibly several channel segments (torch.cat, segment.py:31, 331, 485, 494).
Residual-block tails (`out = act(sum terms)`) are the only materialisation points.

Backward is derived op by op in reverse order:
  * a consumer of a virtual value writes g = dL/d(BN output) through an ACTBWD sink
    and accumulates the BN-backward statistics; the producer conv then rebuilds
    dL/dy on load (BN_BWD segment) for its dgrad and wgrad;
  * a consumer of a materialised value accumulates dL/dvalue (STORE first, then ACCUM);
  * BN gamma/beta, conv-bias-before-BN and PReLU gradients are finalised from the
    double-precision statistics in one pass at the end.

Modules, in import order (DESIGN.md §2 has the map of who hands what to whom):
  knobs     the ISG_* environment switches (patch knobs.NAME: they are not re-exported)
  records   slots, Ptr, Record, OpList: the blob format
  values    Buf, BNRef, SlopeRef, Val, Value, Keypoints
  specs     the shared record specs and GradState
  ops       ConvOp, ConvPairOp, HeadOp, KpPoolOp, PoolOp, TailOp
  graph     param_layout and Graph, the tracer
  schedule  the fold, fork and join passes
  plan      Plan
"""
from .graph import Graph, param_layout  # noqa: F401
from .ops import ConvOp, ConvPairOp, HeadOp, KpPoolOp, PoolOp, TailOp  # noqa: F401
from .plan import Plan  # noqa: F401
from .records import (ALIGN, S_ACT, S_DIN, S_DOUT, S_EXPAVG, S_EXPAVGSQ, S_GRAD,  # noqa: F401
                      S_HYPER, S_IN, S_LOSS, S_OUT, S_OWNER, S_PARAM, S_PGRAD, S_STAMP, S_STATS,
                      S_STEP, S_TAILBNU, S_TAILGF, S_TARGET, S_TENSOR0, S_WREP, OpList, Ptr,
                      Record, _fill)
from .schedule import (_delay_forks, _fold_reader_ok, _fold_tails, _fork_branches,  # noqa: F401
                       _fork_late_wgrads, _fork_pools, _join_dep, _join_exclusions,
                       _trailing_on_main)
from .specs import GradState  # noqa: F401
from .values import (MAX_TENSOR_ELEMS, BNRef, Buf, Keypoints, SlopeRef, Val, Value,  # noqa: F401
                     cat, check_elems)
