// Link-time stand-ins for everything the executor (csrc/exec.cpp) calls below itself: the
// five HIP calls it makes, the two error.cpp makes, every public launcher run_op dispatches
// to and the grouped weight gradient's hooks. Nothing runs; each call appends one entry to
// g_trace (exec_trace.h). Streams and events are small integers in pointer clothing.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstring>

#include "../../include/isg.h"
#include "../../instancesegmentation_amd/csrc/launch.h"
#include "exec_trace.h"

std::vector<TraceEntry> g_trace;
int g_fail_at = 0;
int g_group_max = 4;
static int g_events = 0;

static int sid(const void* st) { return (int)(uintptr_t)st; }
static int eid(hipEvent_t e) { return (int)(uintptr_t)e - 1; }

void trace_print(const TraceEntry& e) {
    switch (e.type) {
        case TraceEntry::GETDEVICE: std::printf("getdevice\n"); return;
        case TraceEntry::CREATE: std::printf("create e%d\n", e.event); return;
        case TraceEntry::RECORD: std::printf("record e%d s%d\n", e.event, e.stream); return;
        case TraceEntry::WAIT: std::printf("wait s%d e%d\n", e.stream, e.event); return;
        default: break;
    }
    if (e.type == TraceEntry::LAUNCH) std::printf("launch s%d kind %d", e.stream, e.kind);
    else std::printf("launch s%d group %zu", e.stream, e.members.size());
    for (const TraceMember& m : e.members) std::printf(" %016llx:%d", (unsigned long long)m.id, m.key);
    std::printf(e.failed ? " FAILED\n" : "\n");
}

// ---- payload identity: FNV-1a over the argument bytes and values ------------------------
struct Hash {
    uint64_t h = 1469598103934665603ull;
    Hash& bytes(const void* p, size_t n) {
        for (size_t i = 0; i < n; ++i) h = (h ^ ((const unsigned char*)p)[i]) * 1099511628211ull;
        return *this;
    }
    template <class T>
    Hash& val(T v) { return bytes(&v, sizeof(v)); }
    // the record's bytes from the start of `a` to the end of `b`, which lies behind it
    template <class A, class B>
    Hash& span(const A* a, const B* b) { return bytes(a, (size_t)((const char*)(b + 1) - (const char*)a)); }
};

static int32_t launch(int kind, isg_stream_t st, const Hash& id, int key = 0) {
    TraceEntry e{TraceEntry::LAUNCH, sid(st), -1, kind, g_fail_at == 1, {{id.h, key}}};
    g_trace.push_back(e);
    if (g_fail_at > 0 && --g_fail_at == 0) return isg_set_error(ISG_ERR_HIP, "stub: the launch fails");
    return ISG_OK;
}

// the key isg_pwg_plan reports: a 1x1 conv's output channels (steered by the payload)
static int pwg_key(const isg_conv_geom* g) { return g->KH == 1 && g->KW == 1 ? g->Co : 0; }
static Hash wgrad_id(const isg_conv_geom* g, const isg_vtensor* x, double* dw, double* dbias,
                     int64_t rep_stride, int32_t nrep) {
    return Hash().span(g, x).val(dw).val(dbias).val(rep_stride).val(nrep);
}
struct PwgPlan {
    uint64_t id;
    int key;
};

extern "C" {

// ---- HIP ---------------------------------------------------------------------------------
hipError_t hipGetDevice(int* dev) {
    g_trace.push_back({TraceEntry::GETDEVICE, 0, -1, 0, false, {}});
    *dev = 0;
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t* ev, unsigned) {
    g_trace.push_back({TraceEntry::CREATE, 0, g_events, 0, false, {}});
    *ev = (hipEvent_t)(uintptr_t)(++g_events);
    return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t ev, hipStream_t st) {
    g_trace.push_back({TraceEntry::RECORD, sid(st), eid(ev), 0, false, {}});
    return hipSuccess;
}
hipError_t hipStreamWaitEvent(hipStream_t st, hipEvent_t ev, unsigned) {
    g_trace.push_back({TraceEntry::WAIT, sid(st), eid(ev), 0, false, {}});
    return hipSuccess;
}
hipError_t hipMemsetAsync(void* p, int, size_t bytes, hipStream_t st) {
    return launch(12, st, Hash().val(p).val(bytes)) ? hipErrorUnknown : hipSuccess;
}
hipError_t hipGetLastError(void) { return hipErrorUnknown; }  // (asked only after a failure)
const char* hipGetErrorString(hipError_t) { return "stub: the launch fails"; }

// ---- the launchers run_op dispatches to, by record kind ----------------------------------
int32_t isg_conv_fwd(const isg_conv_geom* g, const isg_vtensor*, const float*, const isg_sinks* out,
                     isg_stream_t st) {
    return launch(1, st, Hash().span(g, out));
}
int32_t isg_conv_dgrad(const isg_conv_geom* g, const isg_vtensor*, const float*, const isg_sinks* dx,
                       isg_stream_t st) {
    return launch(2, st, Hash().span(g, dx));
}
int32_t isg_conv_wgrad_rep(const isg_conv_geom* g, const isg_vtensor*, const isg_vtensor* x, double* dw,
                           double* dbias, int64_t rep_stride, int32_t nrep, isg_stream_t st) {
    return launch(3, st, wgrad_id(g, x, dw, dbias, rep_stride, nrep), pwg_key(g));
}
int32_t isg_convT_fwd(const isg_conv_geom* g, const isg_vtensor*, const float*, const isg_sinks* out,
                      isg_stream_t st) {
    return launch(4, st, Hash().span(g, out));
}
int32_t isg_maxpool_fwd(const isg_vtensor* x, int32_t k, float* out, int64_t ns, isg_stream_t st) {
    return launch(5, st, Hash().span(x, x).val(k).val(out).val(ns));
}
int32_t isg_maxpool_bwd(const isg_vtensor* x, int32_t, const float*, int64_t, const isg_sinks* dx,
                        isg_stream_t st) {
    return launch(6, st, Hash().span(x, dx));
}
int32_t isg_tail_fwd(const isg_tail* t, isg_stream_t st) { return launch(7, st, Hash().span(t, t)); }
int32_t isg_tail_bwd(const isg_tail_grad* t, isg_stream_t st) { return launch(8, st, Hash().span(t, t)); }
int32_t isg_bn_update_running(const isg_bn_update* it, int32_t n, isg_stream_t st) {
    return launch(9, st, Hash().val(n).bytes(it, n > 0 ? sizeof(*it) * (size_t)n : 0));
}
int32_t isg_grad_finalize(const isg_grad_final* it, int32_t n, isg_stream_t st) {
    return launch(10, st, Hash().val(n).bytes(it, n > 0 ? sizeof(*it) * (size_t)n : 0));
}
int32_t isg_bce_sigmoid(const float* logits, const float* target, int64_t n, double* loss,
                        float* dlogits, float scale, isg_stream_t st) {
    return launch(11, st, Hash().val(logits).val(target).val(n).val(loss).val(dlogits).val(scale));
}
int32_t isg_sum_replicas(float* dst, const double* src, int64_t n, int32_t nrep, int64_t stride,
                         isg_stream_t st) {
    return launch(13, st, Hash().val(dst).val(src).val(n).val(nrep).val(stride));
}
int32_t isg_bn_finalize(const isg_bn* it, int32_t n, int32_t bwd, isg_stream_t st) {
    return launch(14, st, Hash().val(n).val(bwd).bytes(it, n > 0 ? sizeof(*it) * (size_t)n : 0));
}
int32_t isg_kp_stem_fwd(const isg_kp_stem* a, isg_stream_t st) { return launch(15, st, Hash().span(a, a)); }
int32_t isg_kp_stem_wgrad(const isg_kp_stem* a, isg_stream_t st) { return launch(16, st, Hash().span(a, a)); }
int32_t isg_kp_pool(const isg_kp_stem* a, isg_stream_t st) { return launch(17, st, Hash().span(a, a)); }
int32_t isg_mask_head_fwd(const isg_mask_head* a, isg_stream_t st) { return launch(18, st, Hash().span(a, a)); }
int32_t isg_mask_head_bwd(const isg_mask_head* a, isg_stream_t st) { return launch(19, st, Hash().span(a, a)); }
int32_t isg_stamp(uint64_t* buf, int32_t slot, int32_t sign, isg_stream_t st) {
    return launch(20, st, Hash().val(buf).val(slot).val(sign));
}
int32_t isg_depthwise_bwd(const isg_conv_geom* g, const isg_vtensor*, const float*, const isg_sinks*,
                          const isg_vtensor* x, double* dw, double* dbias, int64_t rep_stride,
                          int32_t nrep, isg_stream_t st) {
    return launch(21, st, wgrad_id(g, x, dw, dbias, rep_stride, nrep));
}
int32_t isg_mask_head_fold(const isg_mask_head* a, isg_stream_t st) { return launch(22, st, Hash().span(a, a)); }
int32_t isg_step_tail(const isg_step_tail_args* a, isg_stream_t st) { return launch(24, st, Hash().span(a, a)); }
int32_t isg_step_inc(int32_t* step, isg_stream_t st) { return launch(25, st, Hash().val(step)); }

// ---- the grouped 1x1 weight gradient (launch.h) -----------------------------------------
int32_t isg_pwg_plan_bytes() { return (int32_t)sizeof(PwgPlan); }
int32_t isg_pwg_group_max() { return g_group_max; }
int32_t isg_pwg_plan(const isg_conv_geom* g, const isg_vtensor*, const isg_vtensor* x, double* dw,
                     double* dbias, int64_t rep_stride, int32_t nrep, void* plan) {
    const PwgPlan p{wgrad_id(g, x, dw, dbias, rep_stride, nrep).h, pwg_key(g)};
    std::memcpy(plan, &p, sizeof(p));
    return p.key;
}
int32_t isg_pwg_run(const void* const* plans, int32_t n, hipStream_t st) {
    TraceEntry e{TraceEntry::GROUP, sid(st), -1, 3, g_fail_at == 1, {}};
    for (int i = 0; i < n; ++i) {
        PwgPlan p;
        std::memcpy(&p, plans[i], sizeof(p));
        e.members.push_back({p.id, p.key});
    }
    g_trace.push_back(e);
    if (g_fail_at > 0 && --g_fail_at == 0) return isg_set_error(ISG_ERR_HIP, "stub: the launch fails");
    return ISG_OK;
}

}  // extern "C"
