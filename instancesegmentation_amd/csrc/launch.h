// Host side of the conv launchers, stated once: the internal launchers' prototypes, the
// operand and geometry predicates that pick a kernel and its template flags, and the launch
// idioms. Included by api.cpp, exec.cpp and (through common.h) by every .hip file, the defining ones
// too, so a signature that drifts from its callers' fails to compile or link.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/isg.h"

// ---- error plumbing (error.cpp) ------------------------------------------------------
int32_t isg_set_error(int32_t code, const char* fmt, ...);
int32_t isg_check_launch(const char* what);  // ISG_OK / error

// ---- conv geometry: consistent, dense or depthwise (every public conv entry of api.cpp,
// the executor's grouping): ISG_OK / error ----------------------------------------------------
inline int32_t check_geom(const isg_conv_geom* g) {
    if (!g) return isg_set_error(ISG_ERR_INVALID, "conv: NULL geometry");
    if (g->N < 1 || g->Ci < 1 || g->Co < 1 || g->H < 1 || g->W < 1 || g->KH < 1 || g->KW < 1 ||
        g->SH < 1 || g->SW < 1 || g->DH < 1 || g->DW < 1 || g->PH < 0 || g->PW < 0)
        return isg_set_error(ISG_ERR_INVALID, "conv: invalid geometry");
    const int oh = (g->H + 2 * g->PH - g->DH * (g->KH - 1) - 1) / g->SH + 1;
    const int ow = (g->W + 2 * g->PW - g->DW * (g->KW - 1) - 1) / g->SW + 1;
    if (oh != g->OH || ow != g->OW)
        return isg_set_error(ISG_ERR_INVALID, "conv: output %dx%d but geometry gives %dx%d", g->OH,
                             g->OW, oh, ow);
    if (g->groups != 1 && !(g->groups == g->Ci && g->Ci == g->Co))
        return isg_set_error(ISG_ERR_UNSUPPORTED, "conv: groups=%d (dense or depthwise only)",
                             g->groups);
    if (g->w_ci < 0 || (g->w_ci > 0 && (g->w_ci < g->Ci || g->groups != 1)))
        return isg_set_error(ISG_ERR_INVALID, "conv: weight input channels %d < Ci %d", g->w_ci,
                             g->Ci);
    return ISG_OK;
}

// ---- internal launchers ----------------------------------------------------------------
// "tries": 1 launched, 0 not for this kernel (the caller goes on to the next), < 0 error
int32_t isg_thin_conv(const isg_conv_geom* g, const isg_vtensor* src, const float* w,
                      const isg_sinks* out, bool dgrad, hipStream_t st);     // thin_conv.hip
int32_t isg_tap_conv(const isg_conv_geom* g, const isg_vtensor* src, const float* w,
                     const isg_sinks* out, bool dgrad, hipStream_t st);      // tap_conv.hip
int32_t isg_halo_conv_fwd(const isg_conv_geom* g, const isg_vtensor* x, const float* w,
                          const isg_sinks* out, hipStream_t st);             // halo_conv.hip
int32_t isg_down_conv_fwd(const isg_conv_geom* g, const isg_vtensor* src, const float* w,
                          const isg_sinks* out, hipStream_t st);             // down_conv.hip
int32_t isg_s2k5_fwd(const isg_conv_geom* g, const isg_vtensor* x, const float* w,
                     const isg_sinks* out, hipStream_t st);                  // down_conv.hip
int32_t isg_sub2_dgrad(const isg_conv_geom* g, const isg_vtensor* dy, const float* w,
                       const isg_sinks* dx, hipStream_t st);                 // down_conv.hip
int32_t isg_thin_wgrad(const isg_conv_geom* g, const isg_vtensor* dy, const isg_vtensor* x, double* dw,
                       double* dbias, int64_t rep_stride, int32_t nrep, hipStream_t st);  // thin_conv.hip
int32_t isg_down_conv_wgrad(const isg_conv_geom* g, const isg_vtensor* dy, const isg_vtensor* x, double* dw,
                            double* dbias, int64_t rep_stride, int32_t nrep, hipStream_t st);  // down_conv.hip
int32_t isg_s2k5_wgrad(const isg_conv_geom* g, const isg_vtensor* dy, const isg_vtensor* x, double* dw,
                       double* dbias, int64_t rep_stride, int32_t nrep, hipStream_t st);  // down_conv.hip
int32_t isg_tap_wgrad(const isg_conv_geom* g, const isg_vtensor* dy, const isg_vtensor* x, double* dw,
                      double* dbias, int64_t rep_stride, int32_t nrep, hipStream_t st);  // tap_wgrad.hip
// the ends of a chain: ISG_OK / error
int32_t isg_pw_gemm(const isg_conv_geom* g, const isg_vtensor* src, const float* w,
                    const isg_sinks* out, bool dgrad, hipStream_t st);       // pw_gemm.hip
int32_t isg_dense_conv_fwd(const isg_conv_geom* g, const isg_vtensor* x, const float* w,
                           const isg_sinks* out, hipStream_t st);            // conv_mfma.hip
int32_t isg_dense_conv_dgrad(const isg_conv_geom* g, const isg_vtensor* dy, const float* w,
                             const isg_sinks* dx, hipStream_t st);           // conv_mfma.hip
int32_t isg_dense_conv_wgrad(const isg_conv_geom* g, const isg_vtensor* dy, const isg_vtensor* x, double* dw,
                             double* dbias, int64_t rep_stride, int32_t nrep, hipStream_t st);  // wgrad.hip
int32_t isg_depthwise_fwd(const isg_conv_geom* g, const isg_vtensor* x, const float* w,
                          const isg_sinks* out, hipStream_t st);             // dw_convt.hip
int32_t isg_depthwise_dgrad(const isg_conv_geom* g, const isg_vtensor* dy, const float* w,
                            const isg_sinks* dx, hipStream_t st);            // dw_convt.hip
int32_t isg_depthwise_wgrad(const isg_conv_geom* g, const isg_vtensor* dy, const isg_vtensor* x, double* dw,
                            double* dbias, int64_t rep_stride, int32_t nrep, hipStream_t st);  // dw_convt.hip
// wgrad.hip, the executor's grouped 1x1 weight gradients. isg_pwg_plan: > 0 (the
// instantiation key, the plan written into isg_pwg_plan_bytes() bytes) when
// isg_conv_wgrad_rep would run the op on pwg_kernel, else 0. isg_pwg_run: n <=
// isg_pwg_group_max() plans of one key as one launch, ISG_OK / error
extern "C" {
int32_t isg_pwg_plan_bytes();
int32_t isg_pwg_group_max();
int32_t isg_pwg_plan(const isg_conv_geom* g, const isg_vtensor* dy, const isg_vtensor* x, double* dw,
                     double* dbias, int64_t rep_stride, int32_t nrep, void* plan);
int32_t isg_pwg_run(const void* const* plans, int32_t n, hipStream_t st);
}

// ---- the residual forms ------------------------------------------------------------------
// (isg.h: a BN_FWD segment with y, vtensor.mat, the ACTBWD sink's r / old / p2): only the
// 1x1 stride-1 GEMM (pw_gemm.hip) implements them, every other entry point refuses them
// instead of silently dropping the residual.
inline bool isg_seg_res(const isg_vseg& s) { return s.xform == ISG_XF_BN_FWD && s.y; }
inline bool isg_vt_res(const isg_vtensor* v) {
    if (!v) return false;
    bool r = v->mat != nullptr || v->rbn.stats != nullptr || v->rbn.coef != nullptr;
    for (int i = 0; i < v->nseg && i < ISG_MAX_SEGS; ++i) r |= isg_seg_res(v->s[i]);
    return r;
}
// a BN_BWD segment without y (isg.h isg_vseg: y = p, at p's image stride), resolved at
// every public entry point that takes a vtensor, so no kernel has to know the convention
inline isg_vtensor isg_resolve_y(const isg_vtensor* v) {
    isg_vtensor r{};
    if (!v) return r;  // nseg 0: refused by the kernels' channel checks
    r = *v;
    for (int i = 0; i < r.nseg && i < ISG_MAX_SEGS; ++i)
        if (r.s[i].xform == ISG_XF_BN_BWD && !r.s[i].y) {
            r.s[i].y = r.s[i].p;
            r.s[i].y_n_stride = r.s[i].n_stride;
        }
    return r;
}
inline bool isg_sinks_res(const isg_sinks* k) {
    if (!k) return false;
    bool r = false;
    for (int i = 0; i < k->nsink && i < ISG_MAX_SEGS; ++i)
        r |= k->s[i].r || k->s[i].old || k->s[i].p2 || k->s[i].rbn.stats || k->s[i].rbn.coef;
    return r;
}

// ---- operand predicates ------------------------------------------------------------------
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline bool bn_xform(const isg_vseg& s) { return s.xform == ISG_XF_BN_FWD || s.xform == ISG_XF_BN_BWD; }

// every channel row of the vtensor starts 16-B aligned when its plane size is a multiple of
// 4 floats (HW % 4, W % 4 or OW % 4: the caller's term, it differs per kernel): each
// operand's base and image stride. A NULL y (the input itself) has nothing of its own.
inline bool vt_rows16(const isg_vtensor& v) {
    for (int i = 0; i < v.nseg; ++i) {
        const isg_vseg& s = v.s[i];
        if (!aligned16(s.p) || s.n_stride % 4) return false;
        if (bn_xform(s) && s.y && (!aligned16(s.y) || s.y_n_stride % 4)) return false;
    }
    return !(v.mat && (!aligned16(v.mat) || v.mat_n_stride % 4));
}
inline bool sinks_rows16(const isg_sinks& sk) {
    for (int s = 0; s < sk.nsink; ++s) {
        const isg_sink& k = sk.s[s];
        if (k.mode == ISG_SINK_NONE) continue;
        if (!aligned16(k.p) || k.n_stride % 4) return false;
        if (k.mode == ISG_SINK_ACTBWD && (!aligned16(k.y) || k.y_n_stride % 4)) return false;
    }
    return true;
}
inline int vt_channels(const isg_vtensor* v) {
    int c = 0;
    for (int i = 0; i < v->nseg; ++i) c += v->s[i].C;
    return c;
}
// some channel (sink row) evaluates its BatchNorm statistics in the kernel: no finalised
// coefficients, but statistics
inline bool vt_stat_on(const isg_vtensor& v) {
    for (int i = 0; i < v.nseg; ++i)
        if (bn_xform(v.s[i]) && !v.s[i].bn.coef && v.s[i].bn.stats) return true;
    return false;
}
inline bool sinks_stat_on(const isg_sinks& sk) {
    for (int s = 0; s < sk.nsink; ++s)
        if (sk.s[s].mode == ISG_SINK_ACTBWD && !sk.s[s].bn.coef && sk.s[s].bn.stats) return true;
    return false;
}
// some sink reads an operand (ACTBWD: the saved forward output, ACCUM: the old value)
inline bool sinks_read_operand(const isg_sinks& sk) {
    for (int s = 0; s < sk.nsink; ++s)
        if (sk.s[s].mode == ISG_SINK_ACTBWD || sk.s[s].mode == ISG_SINK_ACCUM) return true;
    return false;
}
// ("fast": stage.h vt_fast / sinks_fast, the kernels' own definitions, callable from the host)

// ---- geometry predicates: the common part only, a site's further terms stay at the site ---
inline bool geom_1x1_s1(const isg_conv_geom* g) {
    return g->KH == 1 && g->KW == 1 && g->SH == 1 && g->SW == 1 && g->PH == 0 && g->PW == 0;
}
// 5x5 stride 2 pad 2 over an even plane (the keypoint stem's convs)
inline bool geom_s2k5(const isg_conv_geom* g) {
    return g->groups == 1 && g->SH == 2 && g->SW == 2 && g->KH == 5 && g->KW == 5 && g->PH == 2 &&
           g->PW == 2 && g->DH == 1 && g->DW == 1 && g->H == 2 * g->OH && g->W == 2 * g->OW;
}

// ---- launch idioms -----------------------------------------------------------------------
// a try's result after its launch: the launch error, else 1
inline int32_t launched(int32_t e) { return e ? e : 1; }
inline int32_t launched(const char* what) { return launched(isg_check_launch(what)); }
// one step of a chain of tries: a nonzero result ends the chain (launched: ISG_OK)
#define ISG_TRY(call)                                   \
    do {                                                \
        const int32_t t_ = (call);                      \
        if (t_ != 0) return t_ < 0 ? t_ : ISG_OK;       \
    } while (0)

// compute units of the current device (256 when the query fails), cached per ordinal
inline int isg_cu_count() {
    static int cus[64] = {};
    int dev = 0, n = 0;
    (void)hipGetDevice(&dev);
    const bool slot = dev >= 0 && dev < 64;
    if (slot && cus[dev]) return cus[dev];
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) n = 256;
    if (slot) cus[dev] = n;
    return n;
}

// a weight gradient's replicas as the kernels index them: no stride for one replica, nrep >= 1
inline void norm_replicas(int64_t& rep_stride, int32_t& nrep) {
    if (nrep <= 1) rep_stride = 0;
    if (nrep < 1) nrep = 1;
}

// f(std::integral_constant<int, T>) with T the instantiated tiles-per-wave count covering
// tpw: 1, 2, 3, 4, 5-6 -> 6, else 8 (surplus tiles compute on unused rows, never stored)
template <class F>
auto with_tpw(int tpw, F f) {
    switch (tpw) {
        case 1: return f(std::integral_constant<int, 1>());
        case 2: return f(std::integral_constant<int, 2>());
        case 3: return f(std::integral_constant<int, 3>());
        case 4: return f(std::integral_constant<int, 4>());
        case 5: case 6: return f(std::integral_constant<int, 6>());
        default: return f(std::integral_constant<int, 8>());
    }
}
