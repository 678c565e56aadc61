// C-ABI front of libisg.so: the public conv entries and their dispatch (dense MFMA vs
// depthwise VALU) (include/isg.h). The error plumbing is error.cpp, the geometry check
// launch.h's check_geom, the plan executor exec.cpp.
#include <hip/hip_runtime.h>

#include "../../include/isg.h"
#include "launch.h"

// the residual forms (isg.h) exist for the 1x1 stride-1 dense conv only
static bool pointwise(const isg_conv_geom* g) {
    return geom_1x1_s1(g) && g->DH == 1 && g->DW == 1 && g->groups == 1 && g->w_ci == 0;
}
// segments covering `cin` channels in (forward: one), consecutive sinks covering all `cout`
// rows out (input gradient: one)
static bool res_shape_ok(const isg_vtensor* v, int cin, const isg_sinks* k, int cout, bool dgrad) {
    if (v->nseg < 1 || v->nseg > ISG_MAX_SEGS || k->nsink < 1 || k->nsink > ISG_MAX_SEGS) return false;
    if (dgrad ? k->nsink != 1 : v->nseg != 1) return false;
    int c = 0;
    for (int i = 0; i < v->nseg; ++i) c += v->s[i].C;
    if (c != cin) return false;
    c = 0;
    for (int i = 0; i < k->nsink; ++i) {
        if (k->s[i].c0 != c) return false;
        c += k->s[i].C;
    }
    return c == cout;
}

// a conv over the first Ci of the weight's w_ci input channels (the keypoint stem's RGB
// part): only tap_conv / tap_wgrad index the weight with a separate channel count
static bool partial_w(const isg_conv_geom* g) { return g->w_ci > 0 && g->w_ci != g->Ci; }

extern "C" {

int32_t isg_abi_version(void) { return 14; }  // 14: isg_train_crop_aug (train_crop.hip)
int32_t isg_stat_replicas(void) { return ISG_STAT_REP; }

int32_t isg_conv_fwd(const isg_conv_geom* g, const isg_vtensor* x_, const float* w,
                     const isg_sinks* out, isg_stream_t st) {
    if (int32_t e = check_geom(g)) return e;
    if (!x_ || !out) return isg_set_error(ISG_ERR_INVALID, "conv fwd: NULL tensor");
    if (isg_sinks_res(out)) return isg_set_error(ISG_ERR_UNSUPPORTED, "conv fwd: residual sink form");
    if (isg_vt_res(x_)) {  // a folded residual tail: the slab 1x1 GEMM or nothing
        if (!pointwise(g) || !res_shape_ok(x_, g->Ci, out, g->Co, false))
            return isg_set_error(ISG_ERR_UNSUPPORTED, "conv fwd: residual input needs a 1x1 conv and one segment");
        return isg_pw_gemm(g, x_, w, out, false, st);
    }
    const isg_vtensor xr = isg_resolve_y(x_);
    const isg_vtensor* x = &xr;
    if (partial_w(g)) {
        // the stem's RGB layer 1 (5x5 s2, weight over w_ci = 20 channels): s2k5_fwd_kernel
        ISG_TRY(isg_s2k5_fwd(g, x, w, out, st));
        ISG_TRY(isg_tap_conv(g, x, w, out, false, st));
        return isg_set_error(ISG_ERR_UNSUPPORTED, "conv fwd: w_ci %d != Ci %d off tap_conv", g->w_ci, g->Ci);
    }
    if (g->groups == 1) return isg_dense_conv_fwd(g, x, w, out, st);
    return isg_depthwise_fwd(g, x, w, out, st);
}

int32_t isg_conv_dgrad(const isg_conv_geom* g, const isg_vtensor* dy_, const float* w,
                       const isg_sinks* dx, isg_stream_t st) {
    if (int32_t e = check_geom(g)) return e;
    if (!dy_ || !dx) return isg_set_error(ISG_ERR_INVALID, "conv dgrad: NULL tensor");
    if (isg_vt_res(dy_)) return isg_set_error(ISG_ERR_UNSUPPORTED, "conv dgrad: residual input form");
    const isg_vtensor dyr = isg_resolve_y(dy_);
    const isg_vtensor* dy = &dyr;
    if (isg_sinks_res(dx)) {  // a folded residual tail's backward: the slab 1x1 GEMM or nothing
        if (!pointwise(g) || !res_shape_ok(dy, g->Co, dx, g->Ci, true))
            return isg_set_error(ISG_ERR_UNSUPPORTED, "conv dgrad: residual sink needs a 1x1 conv and one sink");
        return isg_pw_gemm(g, dy, w, dx, true, st);
    }
    if (partial_w(g)) return isg_set_error(ISG_ERR_UNSUPPORTED, "conv dgrad with w_ci != Ci");
    if (g->groups == 1) return isg_dense_conv_dgrad(g, dy, w, dx, st);
    return isg_depthwise_dgrad(g, dy, w, dx, st);
}

int32_t isg_conv_wgrad_rep(const isg_conv_geom* g, const isg_vtensor* dy_, const isg_vtensor* x_,
                           double* dw, double* dbias, int64_t rep_stride, int32_t nrep,
                           isg_stream_t st) {
    if (int32_t e = check_geom(g)) return e;
    if (isg_vt_res(dy_) || isg_vt_res(x_))
        return isg_set_error(ISG_ERR_UNSUPPORTED, "conv wgrad: residual input form");
    const isg_vtensor dyr = isg_resolve_y(dy_), xr = isg_resolve_y(x_);
    const isg_vtensor *dy = &dyr, *x = &xr;
    if (nrep < 1 || (nrep > 1 && rep_stride <= 0))
        return isg_set_error(ISG_ERR_INVALID, "conv wgrad: bad replicas %d / stride %lld", nrep,
                             (long long)rep_stride);
    if (!dy_ || !x_) return isg_set_error(ISG_ERR_INVALID, "conv wgrad: NULL tensor");
    if (partial_w(g)) {
        // the stem's RGB layer 1 (weight over w_ci = 20 channels): s2k5_wgrad_kernel
        ISG_TRY(isg_s2k5_wgrad(g, dy, x, dw, dbias, rep_stride, nrep, st));
        ISG_TRY(isg_tap_wgrad(g, dy, x, dw, dbias, rep_stride, nrep, st));
        return isg_set_error(ISG_ERR_UNSUPPORTED, "conv wgrad: w_ci %d != Ci %d off tap_wgrad", g->w_ci, g->Ci);
    }
    if (g->groups == 1) return isg_dense_conv_wgrad(g, dy, x, dw, dbias, rep_stride, nrep, st);
    return isg_depthwise_wgrad(g, dy, x, dw, dbias, rep_stride, nrep, st);
}

int32_t isg_conv_wgrad(const isg_conv_geom* g, const isg_vtensor* dy, const isg_vtensor* x,
                       double* dw, double* dbias, isg_stream_t st) {
    return isg_conv_wgrad_rep(g, dy, x, dw, dbias, 0, 1, st);
}

}  // extern "C"
