// The plan executor of libisg.so (include/isg.h isg_exec*): the op-list records and their
// dispatch (run_op), then isg_exec_ms2 in three pieces — the decoder, the grouping of a
// batch's 1x1 weight gradients, and the side-stream scheduler (SideSched), which owns the
// step's ordering contract: the stream of every record, the fork a side batch waits for,
// what a join waits for. tools/asan/exec_order_check.cpp checks that contract without a
// device. Below itself the executor calls only the public launchers, the isg_pwg_* hooks,
// the error plumbing and five HIP calls (hipGetDevice, hipEventCreateWithFlags,
// hipEventRecord, hipStreamWaitEvent, hipMemsetAsync).
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/isg.h"
#include "launch.h"

static bool geom_ok(const isg_conv_geom* g) { return check_geom(g) == ISG_OK; }

extern "C" {

// ---- plan executor ----------------------------------------------------------------
// Blob layout, per op (all 8-byte aligned):
//   int32 kind, int32 desc_bytes, int32 nfix, int32 pad
//   desc_bytes of the op's argument record (one of the structs below)
//   nfix x { int32 loc, int32 slot, int64 offset }: *(void**)(desc+loc) = table[slot]+offset
enum {
    OP_CONV_FWD = 1,
    OP_CONV_DGRAD = 2,
    OP_CONV_WGRAD = 3,
    OP_CONVT_FWD = 4,
    OP_MAXPOOL_FWD = 5,
    OP_MAXPOOL_BWD = 6,
    OP_TAIL_FWD = 7,
    OP_TAIL_BWD = 8,
    OP_BN_UPDATE = 9,
    OP_GRAD_FINAL = 10,
    OP_BCE = 11,
    OP_MEMSET = 12,
    OP_SUM_REP = 13,
    OP_BN_FINAL = 14,
    OP_KP_STEM_FWD = 15,
    OP_KP_STEM_WGRAD = 16,
    OP_KP_POOL = 17,
    OP_HEAD_FWD = 18,
    OP_HEAD_BWD = 19,
    OP_STAMP = 20,
    OP_DW_BWD = 21,
    OP_STEP_TAIL = 24,
    OP_STEP_INC = 25,
    OP_HEAD_FOLD = 22,
};

struct ConvRec {
    isg_conv_geom g;
    isg_vtensor a;
    const float* w;
    isg_sinks out;
};
struct WgradRec {
    isg_conv_geom g;
    isg_vtensor dy;
    isg_vtensor x;
    double* dw;
    double* dbias;
    int64_t rep_stride;
    int32_t nrep;
    int32_t pad_;
};
struct SumRepRec {
    float* dst;
    const double* src;
    int64_t n;
    int64_t stride;
    int32_t nrep;
    int32_t pad_;
};
struct PoolRec {
    isg_vtensor x;
    int32_t k;
    int32_t pad_;
    float* out;
    int64_t out_ns;
    const float* dout;
    int64_t dout_ns;
    isg_sinks dx;
};
struct ListRec {  // followed in the record by n items (host memory)
    int32_t n;
    int32_t pad_;  // OP_BN_FINAL: 0 forward / 1 backward coefficients
};
struct BceRec {
    const float* logits;
    const float* target;
    int64_t n;
    double* loss;
    float* dlogits;
    float grad_scale;
    int32_t pad_;
};
struct MemsetRec {
    void* p;
    int64_t bytes;
};
struct StepIncRec {  // OP_STEP_INC: isg_step_inc
    int32_t* step;
};
struct DwBwdRec {  // OP_DW_BWD: isg_depthwise_bwd
    isg_conv_geom g;
    isg_vtensor dy;
    const float* w;
    isg_sinks dx;
    isg_vtensor x;
    double* dw;
    double* dbias;
    int64_t rep_stride;
    int32_t nrep, pad_;
};
struct StampRec {  // OP_STAMP: isg_stamp(buf, slot, sign)
    uint64_t* buf;
    int32_t slot;
    int32_t sign;
};

struct OpHdr {
    int32_t kind, desc_bytes, nfix, flags;  // flags: ISG_OPF_SIDE | ISG_OPF_JOIN
};
enum { ISG_OPF_SIDE = 1, ISG_OPF_JOIN = 2, ISG_OPF_FORK_NOW = 4 };  // FORK_NOW: forked at the next main-stream op
// flags >> 8 of a JOIN: how many of the most recent side records (in list order) the op does
// NOT depend on — it waits only for the side work up to the one before them (engine/schedule.py
// _join_exclusions); 0 = wait for all side work
constexpr int kJoinExclShift = 8;

// fork / join events of the executor's side streams, per device (created on first use,
// never destroyed; timing disabled): the joins of side stream 0 and 1, the fork pool, the
// batch-completion pool (two per batch, one per side stream)
constexpr int kForkPool = 16;  // fork events of side-stream batches, used round robin
constexpr int kDonePool = 64;  // batch-completion events (partial joins), round robin
static int32_t side_events(hipEvent_t* join, hipEvent_t* join2, hipEvent_t** forks, hipEvent_t** done) {
    static hipEvent_t ev[64][2 + kForkPool + 2 * kDonePool];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64)
        return isg_set_error(ISG_ERR_HIP, "exec: no device for the side stream");
    if (!ev[dev][0]) {
        for (int i = 0; i < 2 + kForkPool + 2 * kDonePool; ++i)
            if (hipEventCreateWithFlags(&ev[dev][i], hipEventDisableTiming) != hipSuccess)
                return isg_check_launch("exec: side-stream events");
    }
    *join = ev[dev][0];
    *join2 = ev[dev][1];
    *forks = &ev[dev][2];
    *done = &ev[dev][2 + kForkPool];
    return ISG_OK;
}
struct Fix {
    int32_t loc, slot;
    int64_t offset;
};

static int32_t run_op(int32_t kind, char* buf, isg_stream_t st) {
    int32_t rc = 0;
    switch (kind) {
        case OP_CONV_FWD: {
            auto* r = (ConvRec*)buf;
            rc = isg_conv_fwd(&r->g, &r->a, r->w, &r->out, st);
            break;
        }
        case OP_CONV_DGRAD: {
            auto* r = (ConvRec*)buf;
            rc = isg_conv_dgrad(&r->g, &r->a, r->w, &r->out, st);
            break;
        }
        case OP_CONV_WGRAD: {
            auto* r = (WgradRec*)buf;
            rc = isg_conv_wgrad_rep(&r->g, &r->dy, &r->x, r->dw, r->dbias, r->rep_stride,
                                    r->nrep < 1 ? 1 : r->nrep, st);
            break;
        }
        case OP_CONVT_FWD: {
            auto* r = (ConvRec*)buf;
            rc = isg_convT_fwd(&r->g, &r->a, r->w, &r->out, st);
            break;
        }
        case OP_MAXPOOL_FWD: {
            auto* r = (PoolRec*)buf;
            rc = isg_maxpool_fwd(&r->x, r->k, r->out, r->out_ns, st);
            break;
        }
        case OP_MAXPOOL_BWD: {
            auto* r = (PoolRec*)buf;
            rc = isg_maxpool_bwd(&r->x, r->k, r->dout, r->dout_ns, &r->dx, st);
            break;
        }
        case OP_TAIL_FWD:
            rc = isg_tail_fwd((const isg_tail*)buf, st);
            break;
        case OP_TAIL_BWD:
            rc = isg_tail_bwd((const isg_tail_grad*)buf, st);
            break;
        case OP_BN_UPDATE: {
            auto* r = (ListRec*)buf;
            rc = isg_bn_update_running((const isg_bn_update*)(buf + sizeof(ListRec)), r->n, st);
            break;
        }
        case OP_BN_FINAL: {
            auto* r = (ListRec*)buf;
            rc = isg_bn_finalize((const isg_bn*)(buf + sizeof(ListRec)), r->n, r->pad_, st);
            break;
        }
        case OP_GRAD_FINAL: {
            auto* r = (ListRec*)buf;
            rc = isg_grad_finalize((const isg_grad_final*)(buf + sizeof(ListRec)), r->n, st);
            break;
        }
        case OP_BCE: {
            auto* r = (BceRec*)buf;
            rc = isg_bce_sigmoid(r->logits, r->target, r->n, r->loss, r->dlogits, r->grad_scale, st);
            break;
        }
        case OP_SUM_REP: {
            auto* r = (SumRepRec*)buf;
            rc = isg_sum_replicas(r->dst, r->src, r->n, r->nrep, r->stride, st);
            break;
        }
        case OP_KP_STEM_FWD:
            rc = isg_kp_stem_fwd((const isg_kp_stem*)buf, st);
            break;
        case OP_KP_STEM_WGRAD:
            rc = isg_kp_stem_wgrad((const isg_kp_stem*)buf, st);
            break;
        case OP_KP_POOL:
            rc = isg_kp_pool((const isg_kp_stem*)buf, st);
            break;
        case OP_HEAD_FWD:
            rc = isg_mask_head_fwd((const isg_mask_head*)buf, st);
            break;
        case OP_HEAD_BWD:
            rc = isg_mask_head_bwd((const isg_mask_head*)buf, st);
            break;
        case OP_HEAD_FOLD:
            rc = isg_mask_head_fold((const isg_mask_head*)buf, st);
            break;
        case OP_DW_BWD: {
            auto* r = (DwBwdRec*)buf;
            rc = isg_depthwise_bwd(&r->g, &r->dy, r->w, &r->dx, &r->x, r->dw, r->dbias, r->rep_stride,
                                   r->nrep, st);
            break;
        }
        case OP_STAMP: {
            auto* r = (StampRec*)buf;
            rc = isg_stamp(r->buf, r->slot, r->sign, st);
            break;
        }
        case OP_STEP_TAIL:
            rc = isg_step_tail((const isg_step_tail_args*)buf, st);
            break;
        case OP_STEP_INC: {
            auto* r = (StepIncRec*)buf;
            rc = isg_step_inc(r->step, st);
            break;
        }
        case OP_MEMSET: {
            auto* r = (MemsetRec*)buf;
            if (hipMemsetAsync(r->p, 0, (size_t)r->bytes, st) != hipSuccess)
                rc = isg_check_launch("memset");
            break;
        }
        default:
            return isg_set_error(ISG_ERR_INVALID, "exec: unknown op kind %d", kind);
    }
    return rc;
}

// ---- the decoder: the list's next record, no scheduling state ------------------------------
struct Decoder {
    const char* p;
    void* const* table;
    OpHdr h;
    alignas(16) char buf[8192];  // the record's payload, pointer fix-ups applied

    int32_t next(int i) {
        std::memcpy(&h, p, sizeof(h));
        p += sizeof(h);
        if (h.desc_bytes < 0 || h.desc_bytes > (int)sizeof(buf))
            return isg_set_error(ISG_ERR_INVALID, "exec: op %d bad desc size %d", i, h.desc_bytes);
        std::memcpy(buf, p, h.desc_bytes);
        p += (h.desc_bytes + 7) & ~7;
        for (int f = 0; f < h.nfix; ++f) {
            Fix fx;
            std::memcpy(&fx, p, sizeof(fx));
            p += sizeof(fx);
            char* base = fx.slot >= 0 ? (char*)table[fx.slot] : nullptr;
            void* v = base ? base + fx.offset : nullptr;
            std::memcpy(buf + fx.loc, &v, sizeof(v));
        }
        return ISG_OK;
    }
};

// ---- a batch of side records and the stream each of its launches goes to ------------------
struct SideOp {
    int32_t kind;
    std::string body;
};
// consecutive one-op batches (the stem's weight gradients, forked one by one behind its
// input-gradient chain) land on different side streams and overlap: `deal` is the
// scheduler's, so the alternation continues across batches
struct StreamPick {
    isg_stream_t side, side2;
    bool spread;
    int& deal;
    isg_stream_t operator()() { return spread && (deal++ & 1) ? side2 : side; }
};

static bool wgrad_kind(int32_t k) { return k == OP_CONV_WGRAD || k == OP_KP_STEM_WGRAD || k == OP_HEAD_FOLD; }

static int32_t run_copy(const SideOp& op, isg_stream_t st) {  // (run_op may write into its record)
    alignas(16) char pb[8192];
    std::memcpy(pb, op.body.data(), op.body.size());
    return run_op(op.kind, pb, st);
}

// a batch of weight gradients only (independent accumulations): the 1x1 ones that would run
// on pwg_kernel go out grouped, up to isg_pwg_group_max() per launch of one instantiation
// (wgrad.hip pwg_group_kernel; DESIGN §3.5: 4.04 -> 3.96 ms/step, 2 interleaved 200-step
// pairs); each group at its first member
static int32_t run_grouped(const std::vector<SideOp>& ops, StreamPick& pick) {
    const size_t n = ops.size();
    const int gmax = isg_pwg_group_max();
    std::vector<std::vector<char>> plans(n);
    std::vector<int> key(n, 0);
    for (size_t i = 0; i < n; ++i) {
        if (ops[i].kind != OP_CONV_WGRAD) continue;
        alignas(16) char pb[8192];
        std::memcpy(pb, ops[i].body.data(), ops[i].body.size());
        auto* r = (WgradRec*)pb;
        if (!geom_ok(&r->g)) continue;
        plans[i].resize((size_t)isg_pwg_plan_bytes());
        key[i] = isg_pwg_plan(&r->g, &r->dy, &r->x, r->dw, r->dbias, r->rep_stride,
                              r->nrep < 1 ? 1 : r->nrep, plans[i].data());
    }
    std::vector<char> done(n, 0);
    for (size_t i = 0; i < n; ++i) {
        if (done[i]) continue;
        if (key[i] <= 0) {
            if (int32_t e = run_copy(ops[i], pick())) return e;
            continue;
        }
        const void* grp[8];
        int m = 0;
        for (size_t j = i; j < n && m < gmax && m < 8; ++j)
            if (!done[j] && key[j] == key[i]) {
                grp[m++] = plans[j].data();
                done[j] = 1;
            }
        if (int32_t e = isg_pwg_run(grp, m, pick())) return e;
    }
    return ISG_OK;
}

// ---- the scheduler: which stream a side record runs on, what it and the joins wait for ----
struct SideSched {
    // weight gradients deferred per fork. Round 6 (eager issue, fused step tail,
    // profiles/r08e_ab_side_batch.txt): 16 -> 3.385 ms/step, 8: 3.377, 24: 3.407, 48: 3.67 —
    // a batch of 48 held the first weight gradients until deep into the backward and then
    // flooded the chain's kernels (round 3 had measured 48 best: 4.365 vs 4.415 at 24)
    static constexpr int batch = 16;
    struct Done {  // an issued batch: the side-record count after it and the events recorded
        int upto;  // behind it on the side stream(s) with outstanding work (partial joins)
        hipEvent_t e1, e2;
    };

    isg_stream_t main_st, side, side2;
    hipEvent_t ev_join = nullptr, ev_join2 = nullptr, *ev_forks = nullptr, *ev_done = nullptr;
    bool forked = false, forked2 = false;  // side-stream work outstanding since the last join
    std::vector<SideOp> pending;           // the open batch
    // a FORK_NOW record's batch is issued when the next main-stream record (or a join, or
    // the end) comes: consecutive forked records share one fork event on the main stream
    // (each event record there cost the main queue ~6 us of idle, round-6 kernel trace;
    // interleaved A/B 3.212-3.221 vs 3.231-3.245 ms/step)
    bool fork_due = false;
    int pool_next = 0, done_next = 0;  // the round-robin places in ev_forks / ev_done
    std::vector<Done> done_list;
    int nside = 0;   // side records seen so far (list order)
    int issued = 0;  // side records issued so far
    int deal = 0;    // weight gradients alternate between the side streams across batches too
    bool side_serial = false;  // a side-only batch ran on `side` since side 2 last waited for it

    // the events, created once per device: at the first side record
    int32_t events() { return ev_join ? ISG_OK : side_events(&ev_join, &ev_join2, &ev_forks, &ev_done); }

    // deferred: launched in batches behind one fork (a later fork only adds dependencies, so
    // batching is always safe)
    int32_t on_side_record(const Decoder& d) {
        ++nside;
        pending.push_back({d.h.kind, std::string(d.buf, d.buf + d.h.desc_bytes)});
        if ((int)pending.size() < batch) {
            fork_due = fork_due || (d.h.flags & ISG_OPF_FORK_NOW);
            return ISG_OK;
        }
        fork_due = false;
        return close_batch();
    }

    int32_t launch_batch(const std::vector<SideOp>& ops, hipEvent_t fork) {
        // a batch of weight gradients only (independent accumulations into the replica
        // buffers) is dealt over both side streams: their grids (128-512 workgroups) leave
        // most of the chip idle one at a time; anything else keeps its order on stream 0
        // (the step counter too: it touches nothing else — as a non-spread batch at the head
        // of the backward it had kept every later batch off side 2, round 6).
        // A batch behind a side-only one (the gradient finalisation lists behind the replica
        // fold at ISG_SIDE_CLOSE=1) may read what that one writes: it stays on `side`, in order
        bool spread = side2 != nullptr && !side_serial, all_wgrad = true;
        for (const SideOp& op : ops) {
            all_wgrad = all_wgrad && wgrad_kind(op.kind);
            spread = spread && (wgrad_kind(op.kind) || op.kind == OP_GRAD_FINAL ||
                                op.kind == OP_BN_UPDATE || op.kind == OP_STEP_INC);
        }
        if (hipStreamWaitEvent(side, fork, 0) != hipSuccess ||
            (spread && hipStreamWaitEvent(side2, fork, 0) != hipSuccess))
            return isg_check_launch("exec: fork side stream");
        if (!spread && forked2) {
            // a non-weight-gradient batch (e.g. the replica fold / gradient finalisation at
            // ISG_SIDE_CLOSE=1) runs on `side` only: order it after side2's outstanding
            // weight-gradient accumulations, which it may read
            forked2 = false;
            if (hipEventRecord(ev_join2, side2) != hipSuccess || hipStreamWaitEvent(side, ev_join2, 0) != hipSuccess)
                return isg_check_launch("exec: order side stream after side stream 2");
        }
        side_serial = side_serial || (!spread && side2 != nullptr);
        forked = true;
        forked2 = forked2 || spread;
        StreamPick pick{side, side2, spread, deal};
        if (all_wgrad) return run_grouped(ops, pick);
        for (const SideOp& op : ops)
            if (int32_t e = run_copy(op, pick())) return e;
        return ISG_OK;
    }

    int32_t close_batch() {  // the pending batch forks here and is issued
        if (pending.empty()) return ISG_OK;
        std::vector<SideOp> ops;
        ops.swap(pending);
        const hipEvent_t fork = ev_forks[pool_next++ % kForkPool];
        if (hipEventRecord(fork, main_st) != hipSuccess) return isg_check_launch("exec: fork point");
        if (int32_t e = launch_batch(ops, fork)) return e;
        issued += (int)ops.size();
        // its completion on the side stream(s) holding outstanding work, for a later partial
        // join (side 2 behind this batch covers it too when the batch did not use side 2)
        Done d{issued, ev_done[2 * (done_next % kDonePool)], nullptr};
        if (hipEventRecord(d.e1, side) != hipSuccess) return isg_check_launch("exec: batch done");
        if (forked2) {
            d.e2 = ev_done[2 * (done_next % kDonePool) + 1];
            if (hipEventRecord(d.e2, side2) != hipSuccess) return isg_check_launch("exec: batch done 2");
        }
        ++done_next;
        done_list.push_back(d);
        return ISG_OK;
    }

    // wait for the side work up to side record `upto` (exclusive count) only
    int32_t join_upto(int upto) {
        if (upto > issued)
            if (int32_t e = close_batch()) return e;
        for (const Done& d : done_list) {
            if (d.upto < upto) continue;
            if (hipStreamWaitEvent(main_st, d.e1, 0) != hipSuccess ||
                (d.e2 && hipStreamWaitEvent(main_st, d.e2, 0) != hipSuccess))
                return isg_check_launch("exec: partial join");
            return ISG_OK;
        }
        return ISG_OK;  // (nothing issued up to there: no side work to wait for)
    }

    int32_t join() {
        if (int32_t e = close_batch()) return e;
        side_serial = false;  // later forks start from the main stream, which waits for both
        if (forked) {
            forked = false;
            if (hipEventRecord(ev_join, side) != hipSuccess || hipStreamWaitEvent(main_st, ev_join, 0) != hipSuccess)
                return isg_check_launch("exec: join side stream");
        }
        if (forked2) {
            forked2 = false;
            if (hipEventRecord(ev_join2, side2) != hipSuccess || hipStreamWaitEvent(main_st, ev_join2, 0) != hipSuccess)
                return isg_check_launch("exec: join side stream 2");
        }
        return ISG_OK;
    }
};

// decode -> fork due? -> join? -> side or main. Without a side stream the SIDE and JOIN
// flags are ignored: every record runs on the main stream, no event call is made.
int32_t isg_exec_ms2(const void* ops, int32_t nops, void* const* table, isg_stream_t main_st,
                     isg_stream_t side, isg_stream_t side2) {
    Decoder d{(const char*)ops, table};
    SideSched s{main_st, side, side2};
    for (int i = 0; i < nops; ++i) {
        if (int32_t e = d.next(i)) return e;
        const bool on_side = side && (d.h.flags & ISG_OPF_SIDE);
        if (s.fork_due && !on_side) {
            s.fork_due = false;
            if (int32_t e = s.close_batch()) return e;
        }
        if (side && (d.h.flags & ISG_OPF_JOIN)) {
            // flags >> 8: the most recent side records the op does not wait for (0: none)
            const int excl = d.h.flags >> kJoinExclShift;
            if (int32_t e = excl > 0 && excl <= s.nside ? s.join_upto(s.nside - excl) : s.join()) return e;
        }
        if (on_side)  // (the op depends on everything issued so far on the main stream)
            if (int32_t e = s.events()) return e;
        if (int32_t rc = on_side ? s.on_side_record(d) : run_op(d.h.kind, d.buf, main_st)) {
            std::string m = isg_last_error();
            return isg_set_error(rc, "exec op %d (kind %d): %s", i, d.h.kind, m.c_str());
        }
    }
    return s.join();
}

int32_t isg_exec_ms(const void* ops, int32_t nops, void* const* table, isg_stream_t main_st,
                    isg_stream_t side) {
    return isg_exec_ms2(ops, nops, table, main_st, side, nullptr);
}

int32_t isg_exec(const void* ops, int32_t nops, void* const* table, isg_stream_t st) {
    return isg_exec_ms2(ops, nops, table, st, nullptr, nullptr);
}

// sizes of the executor records, so the Python planner can verify its ctypes mirrors
int32_t isg_record_size(int32_t which) {
    switch (which) {
        case 0: return (int32_t)sizeof(isg_vtensor);
        case 1: return (int32_t)sizeof(isg_sinks);
        case 2: return (int32_t)sizeof(ConvRec);
        case 3: return (int32_t)sizeof(WgradRec);
        case 4: return (int32_t)sizeof(PoolRec);
        case 5: return (int32_t)sizeof(isg_tail);
        case 6: return (int32_t)sizeof(isg_tail_grad);
        case 7: return (int32_t)sizeof(isg_bn_update);
        case 8: return (int32_t)sizeof(isg_grad_final);
        case 9: return (int32_t)sizeof(BceRec);
        case 10: return (int32_t)sizeof(isg_conv_geom);
        case 11: return (int32_t)sizeof(isg_bn);
        case 12: return (int32_t)sizeof(isg_vseg);
        case 13: return (int32_t)sizeof(isg_sink);
        case 14: return (int32_t)sizeof(SumRepRec);
        case 15: return (int32_t)sizeof(isg_kp_stem);
        case 16: return (int32_t)sizeof(isg_mask_head);
        case 17: return (int32_t)sizeof(StampRec);
        case 18: return (int32_t)sizeof(DwBwdRec);
        case 19: return (int32_t)sizeof(isg_step_tail_args);
        case 20: return (int32_t)sizeof(isg_train_sample);
        case 21: return (int32_t)sizeof(isg_train_aug);
        default: return -1;
    }
}

}  // extern "C"
