/*
 * isg.h — C-ABI of libisg.so, the MI355X (gfx950) kernels behind the
 * instance-segmentation hot path.
 *
 * The reference (YanMiaoW/instanceSegmentation) is pure Python with no FFI; every
 * entry point below replaces the torch eager kernels that one reference call site
 * runs (file:line into /root/reference). The Python host
 * (instancesegmentation_amd/_lib.py, ctypes) binds exactly these symbols; see
 * INTEGRATION.md for the binding a maintainer adds on the reference side.
 *
 * Conventions:
 *   - all tensors are fp32 NCHW device pointers owned by the caller (torch's caching
 *     allocator); the library never allocates, frees or synchronises;
 *   - "virtual" inputs (isg_vtensor) are raw conv outputs plus a per-channel
 *     transform applied on load (BatchNorm fwd + activation, or BatchNorm bwd);
 *     channel segments let a consumer read a concat without materialising it;
 *   - every call enqueues on the caller's hipStream_t and returns 0, or a negative
 *     status with a thread-local message in isg_last_error();
 *   - functions are stateless and re-entrant (backward runs on torch's autograd
 *     worker thread).
 */
#ifndef ISG_H
#define ISG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* isg_stream_t; /* == hipStream_t */

#define ISG_OK 0
#define ISG_ERR_INVALID -1
#define ISG_ERR_UNSUPPORTED -2
#define ISG_ERR_HIP -3

#define ISG_MAX_SEGS 3
#define ISG_MAX_CH 512
#define ISG_LIST_CHUNK 32
/* Every cross-workgroup accumulator (BN statistics, PReLU slope and bias sums) is kept
 * in ISG_STAT_REP replicas, each workgroup adding into one chosen by its block index,
 * so at most (workgroups / ISG_STAT_REP) atomics contend on an address; readers sum the
 * replicas. An accumulator "of n values" therefore occupies ISG_STAT_REP*n doubles,
 * replica r at offset r*n. (Overridable at build time for experiments; the Python side
 * reads the count back through isg_stat_replicas.) */
#ifndef ISG_STAT_REP
#define ISG_STAT_REP 4
#endif

enum { ISG_ACT_NONE = 0, ISG_ACT_RELU = 1, ISG_ACT_PRELU = 2 };
enum { ISG_XF_PLAIN = 0, ISG_XF_BN_FWD = 1, ISG_XF_BN_BWD = 2 };
enum { ISG_SINK_STORE = 0, ISG_SINK_ACCUM = 1, ISG_SINK_ACTBWD = 2, ISG_SINK_NONE = 3 };

/* One BatchNorm2d layer (segment.py:41 `nn.BatchNorm2d(c2)`; eps 1e-5, momentum 0.1).
 * stats layout: [sum(C) | sumsq(C) | gsum(C) | gxsum(C)] in double; sum/sumsq are of
 * the raw (pre-BN, bias included) conv output over N*H*W, gsum of the gradient g
 * w.r.t. the BN output and gxsum of g*(y - mean), accumulated centred so the BN
 * backward never cancels against mean*gsum. train=0 uses the running statistics.
 * The 4*C block is replicated ISG_STAT_REP times (4*C*ISG_STAT_REP doubles). */
typedef struct {
    const float* gamma;
    const float* beta;
    const float* running_mean;
    const float* running_var;
    double* stats;
    int32_t C;
    int32_t train;
    float count; /* N*H*W */
    float eps;
    /* Finalised per-channel coefficients (8*C floats), or NULL: forward [C][4] =
     * (mean, gamma*rstd, beta, 0) then backward [C][4] = (A, B, mean, C) of
     * dy = A*g + B*(y - mean) + C. Written by isg_bn_finalize once per layer and step
     * so consumers read 16 bytes per channel instead of reducing the fp64 replicas;
     * NULL makes every consumer derive them from `stats` (or the running stats). */
    float* coef;
} isg_bn;

/* A channel segment of a virtual tensor.
 *   PLAIN : v = p
 *   BN_FWD: v = act((p - mean) * gamma*rstd + beta)            (Conv.forward, segment.py:44-45)
 *           with y non-NULL (a residual block's tail read by its consumer):
 *           v = act((p - mean) * gamma*rstd + beta + y)        (segment.py:75-77: out += residual;
 *           prelu) — accepted only by the 1x1 stride-1 conv forward, one segment (any
 *           sinks: a stacked sibling pair's two)
 *   BN_BWD: v = dL/d(conv output) rebuilt from g (= dL/d BN-output) and the forward
 *           raw y: A*g + B*(y - mean) + C                       (BatchNorm2d backward) */
typedef struct {
    const float* p;
    const float* y;        /* BN_BWD: saved raw output (NULL: y = p, with p's n_stride);
                              BN_FWD: residual term or NULL */
    int64_t n_stride;      /* elements between images of p */
    int64_t y_n_stride;
    int32_t C;
    int32_t xform;
    int32_t act;           /* BN_FWD only */
    int32_t pad_;
    const float* slope;    /* PReLU weight [C] (segment.py:24 nn.PReLU(planes)) */
    isg_bn bn;
} isg_vseg;

typedef struct {
    isg_vseg s[ISG_MAX_SEGS];
    int32_t nseg;
    int32_t N, H, W;       /* C = sum of segment channels */
    /* non-NULL: the consumer also writes the transformed values v here ([N][C][H][W] at
     * mat_n_stride per image) — the materialised block output a residual tail would have
     * written; 1x1 stride-1 conv forward with one segment only */
    float* mat;
    int64_t mat_n_stride;
    /* the residual term's own BatchNorm (a tail of two BatchNorm'd conv outputs,
     * segment.py:147-148, 202-207): when rbn.stats or rbn.coef is set the residual form
     * reads act(BN(p) + BN2(y)) */
    isg_bn rbn;
} isg_vtensor;

/* Where a kernel writes channels [c0, c0+C) of its result.
 *   STORE : p = v + bias; optional BN sum/sumsq into stats   (forward conv outputs)
 *   ACCUM : p += v                                            (gradient of a consumed tensor)
 *   ACTBWD: v is dL/dz for z = act(BN(y)); writes g = v*act'(BN(y)) into p and
 *           accumulates bn.stats gsum/gxsum and the PReLU slope gradient.
 *           Residual form (r non-NULL; a block tail's backward folded into the input
 *           gradient of the next block's first 1x1, segment.py:75-77): v' = v + old,
 *           z = BN(y) + r, g = v'*act'(z) into p and, when p2 is non-NULL, also into p2
 *           (the residual term's gradient; STORE, or ACCUM with p2_accum); statistics as
 *           ACTBWD with v'. Accepted only by the 1x1 stride-1 input gradient with one
 *           sink (any gradient segments: a stacked sibling pair's two). */
typedef struct {
    float* p;
    int64_t n_stride;
    int32_t c0, C;
    int32_t mode;
    int32_t act;
    const float* bias;
    double* stats;         /* STORE/ACCUM: a BN-layout block (4*C per replica) whose
                              sum/sumsq halves receive the output sums, or NULL */
    const float* y;        /* ACTBWD */
    int64_t y_n_stride;
    const float* slope;    /* ACTBWD + PRELU */
    double* slope_grad;    /* ACTBWD + PRELU, C doubles per replica */
    isg_bn bn;             /* ACTBWD; bn.stats==NULL means "no BN" (identity). bn.C must equal C
                              (the sink covers its whole layer): the kernels lay gsum / gxsum
                              out by the sink's C. Only a vseg may read the first channels of
                              a wider layer (its bn.C > C) */
    const float* r;        /* ACTBWD residual form: the tail's residual term, or NULL */
    int64_t r_n_stride;
    const float* old;      /* ACTBWD residual form: gradient already accumulated for v, or NULL */
    int64_t old_n_stride;
    float* p2;             /* ACTBWD residual form: second output of g, or NULL */
    int64_t p2_n_stride;
    int32_t p2_accum;      /* p2 += g instead of p2 = g */
    int32_t pad2_;
    isg_bn rbn;            /* ACTBWD residual form: the residual's own BatchNorm (stats or coef
                              set): z = BN(y) + BN2(r); rbn.stats receives Σg and Σg(r - mean2) */
} isg_sink;

typedef struct {
    isg_sink s[ISG_MAX_SEGS];
    int32_t nsink;
    int32_t pad_;
} isg_sinks;

typedef struct {
    int32_t N, Ci, H, W;         /* conv input  */
    int32_t Co, OH, OW;          /* conv output */
    int32_t KH, KW, SH, SW, PH, PW, DH, DW;
    int32_t groups;              /* 1 (dense) or Ci == Co (depthwise) */
    /* input channels of the weight tensor when the conv reads only its first Ci (0 = Ci):
     * the keypoint stem runs the dense conv over the RGB channels of a weight
     * [Co][w_ci][KH][KW] (isg_kp_stem below); tap_conv forward / tap_wgrad only */
    int32_t w_ci;
    int32_t pad_;
} isg_conv_geom;

/* Residual-block tail: out = act(sum_i term_i), term_i = vtensor channel-aligned
 * with the output, optionally nearest-upsampled x2 (segment.py:76-77, 107-109,
 * 147-148, 202-207, 255-259, 331-333). */
typedef struct {
    isg_vseg term[3];
    int32_t up[3];
    int32_t nterm;
    int32_t act;
    const float* slope;
    float* out;
    int64_t out_n_stride;
    int32_t N, C, H, W;
} isg_tail;

typedef struct {
    isg_tail f;
    const float* dout;        /* dL/d out */
    int64_t dout_n_stride;
    float* g;                 /* dL/d(sum) written here when non-NULL */
    int64_t g_n_stride;
    float* dterm[3];          /* PLAIN terms: gradient destination (ACCUM or store) */
    int64_t dterm_n_stride[3];
    int32_t dterm_accum[3];
    double* slope_grad;
} isg_tail_grad;

/* ---- forward / backward building blocks -------------------------------- */

/* Dense or depthwise conv forward: y = conv(x) (+bias, BN stats) into `out` sinks.
 * Replaces nn.Conv2d.forward inside Conv (segment.py:39-45) and the bare convs at
 * segment.py:91-92, 323, 343, 437. Dense convs run as implicit GEMM on
 * v_mfma_f32_16x16x4_f32; depthwise on VALU. */
int32_t isg_conv_fwd(const isg_conv_geom* g, const isg_vtensor* x, const float* w,
                     const isg_sinks* out, isg_stream_t stream);

/* Input gradient of a conv: dx = conv^T(dy, w) into per-segment sinks. */
int32_t isg_conv_dgrad(const isg_conv_geom* g, const isg_vtensor* dy, const float* w,
                       const isg_sinks* dx, isg_stream_t stream);

/* Weight/bias gradient: dw += sum dy (x) im2col(x); dbias += sum dy (either may be
 * NULL), into fp64 accumulators that the caller zeroes before the first contribution and
 * folds to fp32 with isg_sum_replicas (nrep 1). */
int32_t isg_conv_wgrad(const isg_conv_geom* g, const isg_vtensor* dy, const isg_vtensor* x,
                       double* dw, double* dbias, isg_stream_t stream);

/* Weight-gradient replicas. A dW element receives one atomic add from every workgroup
 * along the pixel dimension (hundreds); same-address atomics serialise at the memory
 * side (~40 ns each), so the wgrad kernels add into one of `nrep` replicas of dw/dbias
 * (replica r at dw + r*rep_stride elements), chosen per workgroup, and one
 * isg_sum_replicas pass folds them at the end of the backward.
 *
 * The replicas are fp64 and every addend is a workgroup's fp32 partial (reduced in a fixed
 * order inside the workgroup): an fp64 sum of fp32 values is EXACT — so the same whatever
 * order the atomics land in — as long as the running sum stays within 2^29 of the smallest
 * addend's magnitude (53 - 24 significand bits), and otherwise off by at most 2^-53 of
 * the running sum, 2^-29 of the fp32 result's rounding step. The fold sums the replicas in
 * fixed order and rounds once to fp32. With the BatchNorm statistics (fp64 sums of fp32
 * workgroup partials, the same argument) the backward is reproducible bit for bit across
 * runs WHILE every element's partials span less than 2^29 in magnitude; outside that range
 * an fp64 sum can differ in its last bit with the atomic order, which can flip the fp32
 * rounding: then within 1 fp32 ulp, not bitwise. The fixtures and the bench batch stay
 * inside the range (tests/test_gpu_trainer.py::test_backward_is_bitwise_reproducible
 * asserts exact equality of logits and gradients there). The summed
 * LOSS is not covered: isg_bce_sigmoid adds fp64 workgroup partials (not fp32 ones), so its
 * last bits depend on the atomic order. With fp32 replicas nothing was reproducible
 * (VERDICT r04). */
#define ISG_WREP 16
int32_t isg_conv_wgrad_rep(const isg_conv_geom* g, const isg_vtensor* dy, const isg_vtensor* x,
                           double* dw, double* dbias, int64_t rep_stride, int32_t nrep,
                           isg_stream_t stream);
/* Both backward halves of one depthwise layer (segment.py:63-64 groups=planes, the
 * Bottleneck blocks' 3x3 / 5x1 / 1x5): dx through the one sink `dx` (as isg_conv_dgrad;
 * NULL or nsink 0 skips it) and dw / dbias accumulated into replicas (as
 * isg_conv_wgrad_rep; dw NULL skips it), in ONE launch when both tile kernels apply
 * (same-size layer, W % 4 == 0, 16-B aligned sink rows): the dy tile is staged once. Same
 * partials and reduction order as the two calls, so the results are bitwise theirs. */
int32_t isg_depthwise_bwd(const isg_conv_geom* g, const isg_vtensor* dy, const float* w,
                          const isg_sinks* dx, const isg_vtensor* x, double* dw, double* dbias,
                          int64_t rep_stride, int32_t nrep, isg_stream_t stream);
/* dst[i] = (float) sum_{r<nrep} src[r*stride + i] for i < n (fp64, fixed order). */
int32_t isg_sum_replicas(float* dst, const double* src, int64_t n, int32_t nrep, int64_t stride,
                         isg_stream_t stream);

/* ConvTranspose2d forward (segment.py:305-306, 435-436) with kernel = 2*stride,
 * weight [Ci][Co][K][K], as a sub-pixel direct kernel. geom describes the transposed
 * conv: input (N,Ci,H,W) -> output (N,Co,OH,OW), KH=KW=K, SH=SW=s, PH=PW=p. */
int32_t isg_convT_fwd(const isg_conv_geom* g, const isg_vtensor* x, const float* w,
                      const isg_sinks* out, isg_stream_t stream);

/* Max-pool k x k stride k (segment.py:29, 145) of a virtual tensor into a slice: channels
 * [0, C) of `out` at out_n_stride per image. torch CPU max_pool2d semantics: the first
 * maximum of a window wins, a NaN wins over everything before it.
 * ISG_ERR_UNSUPPORTED before any launch: H or W not a multiple of k, a residual input
 * form, nseg outside 1..ISG_MAX_SEGS, a segment without channels, more than ISG_MAX_CH
 * channels in all. With k = 2 / 4 each window row is read as one 8-B / 16-B load when
 * every segment's p is aligned to that and its n_stride a multiple of k; otherwise pixel
 * by pixel, in the same order with the same result. */
int32_t isg_maxpool_fwd(const isg_vtensor* x, int32_t k, float* out, int64_t out_n_stride,
                        isg_stream_t stream);
/* Route dL/d out to the arg-max of each window (same rule). A STORE sink receives zeros
 * off the arg-max, an ACCUM sink is touched at the arg-max only, a NONE sink not at all.
 * Refused as the forward, and with ISG_ERR_UNSUPPORTED too: an ACTBWD sink, nsink outside
 * 1..ISG_MAX_SEGS, sinks that do not cover [0, C) in order (s[0].c0 = 0,
 * s[i].c0 = s[i-1].c0 + s[i-1].C, the last ending at C). Sinks need not split where the
 * segments do. */
int32_t isg_maxpool_bwd(const isg_vtensor* x, int32_t k, const float* dout,
                        int64_t dout_n_stride, const isg_sinks* dx, isg_stream_t stream);

/* Residual tail (isg_tail above) and its backward: g = dL/d(sum) = dout * act'(sum) into
 * `g`, into every PLAIN term's dterm (an x2-upsampled term receives its 2x2 block's sum)
 * and, for every BN_FWD term with statistics, gsum / gxsum (centred on that term's own
 * mean) into its bn.stats; the PReLU slope gradient into slope_grad. g, a PLAIN term's
 * dterm and slope_grad may each be NULL: nothing is written for it.
 * ISG_ERR_UNSUPPORTED before any launch: odd H or W, nterm outside 1..3, a residual term
 * form, a BN_BWD term (the kernels load no saved output y), and in the backward a BN_FWD
 * term whose own act is not ISG_ACT_NONE (the forward applies it; the backward passes g
 * to the term unchanged, which is the gradient only without it). ISG_ERR_INVALID: two
 * terms sharing a gradient destination of which one accumulates. */
int32_t isg_tail_fwd(const isg_tail* t, isg_stream_t stream);
int32_t isg_tail_bwd(const isg_tail_grad* t, isg_stream_t stream);

/* BatchNorm running-stat update for `nitems` layers; `items` is a HOST array (copied
 * into kernel arguments in chunks of ISG_LIST_CHUNK) (torch BatchNorm2d train semantics):
 * rm = (1-m) rm + m mean; rv = (1-m) rv + m var*M/(M-1); nbt += 1. */
typedef struct {
    const double* stats;
    float* running_mean;
    float* running_var;
    int64_t* num_batches_tracked;
    int32_t C;
    float count;
    float momentum;
    int32_t pad_;
} isg_bn_update;
int32_t isg_bn_update_running(const isg_bn_update* items, int32_t nitems, isg_stream_t stream);

/* Coefficient finalisation for `nitems` BatchNorm layers (HOST array, chunked like
 * isg_bn_update_running): from the replicated fp64 statistics write items[i].coef's
 * forward half (bwd == 0, after the forward statistics are complete) or backward half
 * (bwd == 1, after the gsum/gxsum statistics are complete). Same fp64 formulas the
 * consumers would evaluate (BatchNorm2d train: biased variance, eps). */
int32_t isg_bn_finalize(const isg_bn* items, int32_t nitems, int32_t bwd, isg_stream_t stream);

/* Parameter-gradient finalisation (HOST item array, like isg_bn_update_running):
 *   dgamma = rstd*gxsum, dbeta = gsum,
 *   dbias(conv before BN) = sum of rebuilt dy, dslope = double accumulator -> float. */
typedef struct {
    const double* stats;       /* BN stats (4*C per replica) or NULL */
    const float* gamma;
    const float* running_mean; /* eval-mode backward */
    const float* running_var;
    float* dgamma;
    float* dbeta;
    float* dconv_bias;         /* may be NULL */
    const double* slope_acc;   /* may be NULL (then stats describe a BN) */
    float* dslope;
    int32_t C;
    int32_t train;
    float count;
    float eps;
    int32_t slope_stride;      /* replica stride of slope_acc in doubles: C for a PReLU
                                  slope, 4*C for the sum half of a sink's stats block */
    int32_t pad_;
} isg_grad_final;
int32_t isg_grad_finalize(const isg_grad_final* items, int32_t nitems, isg_stream_t stream);

/* The end of a world-size-1 training step as ONE launch (train_instance.py:379-380:
 * the gradient complete, then optimizer.step()): fold the weight-gradient replicas
 * (isg_sum_replicas) into `grad` and apply Adam (isg_adam_dev's arithmetic, step already
 * advanced by isg_step_inc) to every folded element; finalise the statistics-derived
 * gradients of the `ngf` items (isg_grad_finalize) into `grad` and apply Adam to those; update
 * the running statistics of the `nbnu` BatchNorm layers (isg_bn_update_running). `gf` and
 * `bnu` are DEVICE arrays. owner[i]: bit 0 = Adam updates element i (a used parameter),
 * bit 1 = a grad_final item writes grad[i] (the fold skips it). Bitwise the result of those
 * separate calls for every item form (a grad_final item may read a gamma that its own
 * dgamma element's Adam updates: it reads before it writes); an eval-mode (train 0) item
 * must not read the running statistics of a layer in `bnu`.
 * hyper = (lr, beta1, beta2, eps, weight_decay), device doubles. */
typedef struct {
    float* grad;
    const double* rep;         /* nrep replicas, replica stride n */
    int64_t n;
    int32_t nrep;
    int32_t ngf;
    float* param;
    float* exp_avg;
    float* exp_avg_sq;
    const uint8_t* owner;
    const int32_t* step;
    const double* hyper;
    const isg_grad_final* gf;
    const isg_bn_update* bnu;
    int32_t nbnu;
    int32_t pad_;
} isg_step_tail_args;
int32_t isg_step_tail(const isg_step_tail_args* args, isg_stream_t stream);
/* step += 1 on the device (the 1-based Adam step of isg_step_tail / isg_adam_dev). */
int32_t isg_step_inc(int32_t* step, isg_stream_t stream);

/* sigmoid + nn.BCELoss(mean) forward and backward in one pass (segment.py:534,
 * train_instance.py:299,378-379), torch clamp semantics: log clamped at -100,
 * dL/dp = (p-y)/max(p(1-p),1e-12)/n, dL/dlogit = dL/dp * p(1-p).
 * loss_acc: one double (sum); dlogits may be NULL. */
int32_t isg_bce_sigmoid(const float* logits, const float* target, int64_t n, double* loss_acc,
                        float* dlogits, float grad_scale, isg_stream_t stream);
int32_t isg_sigmoid_fwd(const float* x, float* y, int64_t n, isg_stream_t stream);
int32_t isg_sigmoid_bwd(const float* y, const float* dy, float* dx, int64_t n,
                        isg_stream_t stream);

/* torch.optim.Adam (defaults lr 1e-3, betas (0.9,0.999), eps 1e-8; train_instance.py:297)
 * over a flat fp32 buffer. `live` (uint8 per element, may be NULL) masks parameters
 * whose grad is None (they are skipped, as torch does). step is 1-based. The
 * hyperparameters are doubles, as torch's python floats: 1-beta and the bias corrections
 * are rounded from them the way torch does, so a torch optimizer state continues here
 * bit-for-bit in the update formula. */
int32_t isg_adam(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                 const uint8_t* live, int64_t n, int32_t step, double lr, double beta1,
                 double beta2, double eps, double weight_decay, isg_stream_t stream);

/* Same update with the step counter in device memory: *step is incremented on the
 * stream first, then used — the launch sequence can be captured in a HIP graph and
 * replayed (the host-side form bakes `step` into the kernel arguments). */
int32_t isg_adam_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                     const uint8_t* live, int64_t n, int32_t* step, double lr, double beta1,
                     double beta2, double eps, double weight_decay, isg_stream_t stream);

int32_t isg_fill_f64(double* p, int64_t n, double v, isg_stream_t stream);

/* Timestamp t of the chip-global 100 MHz counter (s_memrealtime) when this launch runs on
 * the stream, accumulated into buf (uint64, two's complement): buf[slot] += sign < 0 ? -t : t
 * (slot 0 or 1), buf[2] = max(buf[2], t), buf[3] = min(buf[3], t). A (-, +) pair around one
 * op of the executor's list (the OP_STAMP record) sums that op's time where it runs in the
 * step, over every replay of one HIP graph (bench.py's roofline; ROCm rejects timing events
 * recorded under graph capture). */
int32_t isg_stamp(uint64_t* buf, int32_t slot, int32_t sign, isg_stream_t stream);

/* ---- infer post-process (build-defined; infer.py:32-36 is a stub) -------- */

/* A13: paste K crop probability maps [K,S,S] back onto an HxW canvas through their
 * crop windows boxes[K][4] = (x0,y0,x1,y1), bilinear, uint8 by truncation of p*255
 * (train_instance.py:398-399). Contract: oracle/maskops_oracle.py (bit-exact). */
int32_t isg_mask_paste(const float* prob, int32_t K, int32_t S, const int32_t* boxes,
                       int32_t H, int32_t W, uint8_t* out, isg_stream_t stream);

/* A14: per-mask count/sum/score and greedy mask-NMS (K <= 256). keep[K] receives the
 * kept indices in keep order, *nkeep their number (both device memory).
 * work: isg_mask_nms_workspace(K,H,W) bytes, caller-owned. */
int64_t isg_mask_nms_workspace(int32_t K, int32_t H, int32_t W);
int32_t isg_mask_nms(const uint8_t* masks, int32_t K, int32_t H, int32_t W, float iou_thr,
                     void* work, float* scores_out, int32_t* keep, int32_t* nkeep,
                     isg_stream_t stream);

/* A13 + A14 in one pass (the infer product path): isg_mask_paste's canvases written and
 * bit-packed for the NMS in the same kernel (no memset, no re-read of the canvases),
 * then isg_mask_nms's intersections and greedy suppression. Same outputs, bit-exact to
 * isg_mask_paste followed by isg_mask_nms; work: isg_mask_nms_workspace(K,H,W) bytes. */
int32_t isg_mask_paste_nms(const float* prob, int32_t K, int32_t S, const int32_t* boxes,
                           int32_t H, int32_t W, float iou_thr, uint8_t* masks, void* work,
                           float* scores_out, int32_t* keep, int32_t* nkeep, isg_stream_t stream);

/* COCO run-length encoding of selected canvases (csrc/mask_rle.hip; the contract is stated
 * on the CPU by instancesegmentation_amd/rle.py `encode`). A pixel is set when mask >= 128;
 * the H x W mask is flattened column-major (pixel (x, y) at position x*H + y) and counts
 * are the lengths of the alternating runs, the first of zeros (so counts[0] == 0 when pixel
 * 0 is set): between 1 and H*W + 1 uint32 values per mask, H*W < 2^31.
 * masks: [K,H,W]. sel / nsel: device memory (isg_mask_nms's keep / nkeep plug in); slot
 * j < min(*nsel, max_sel) encodes mask sel[j] into runs[offsets[j] .. offsets[j+1]), slots
 * packed in slot order; offsets[j] of every j past the last slot is the total. sel == NULL:
 * slots 0..K-1 in order (max_sel <= K), nsel may then be NULL too (all max_sel slots). A
 * sel[j] outside [0,K) encodes as the all-zero mask [H*W] and reads nothing. max_sel <= K
 * (the workspace is sized by K): more is ISG_ERR_UNSUPPORTED.
 * Overflow: offsets[max_sel + 1] always holds the true values; runs[i] is written only for
 * i < runs_cap (runs may be NULL when runs_cap == 0); the caller checks
 * offsets[last] > runs_cap. Nothing is raised on the device.
 * Capturable: the launch geometry depends on (K, H, W, max_sel) only, nothing is allocated
 * or synchronised, and the result does not depend on what work, runs or offsets held.
 * work: isg_mask_rle_workspace(K,H,W) bytes, caller-owned. */
int64_t isg_mask_rle_workspace(int32_t K, int32_t H, int32_t W);
int32_t isg_mask_rle(const uint8_t* masks, int32_t K, int32_t H, int32_t W, const int32_t* sel,
                     const int32_t* nsel, int32_t max_sel, uint32_t* runs, int64_t runs_cap,
                     int64_t* offsets /* [max_sel+1] */, void* work, isg_stream_t stream);

/* COCO run-length decoding onto canvases (csrc/mask_rle_decode.hip; the contract is stated on
 * the CPU by instancesegmentation_amd/rle.py `decode_canvas`): the inverse of isg_mask_rle,
 * whose runs / offsets plug in unchanged. Slot j < n decodes the counts
 * runs[offsets[j] .. offsets[j+1]) into masks[j] (row-major [H,W], every byte written, 0 or
 * 255) and totals[j] = their unclipped sum; the caller compares totals with H*W, nothing is
 * raised on the device. With ends = cumsum(counts), column-major position p = x*H + y
 * belongs to run i = #{ends <= p} (zero-length runs are stepped over) and is 255 when i is
 * odd and i < the number of counts: positions at or past the sum are background, runs past
 * H*W are ignored. A slot whose range is empty or reversed, starts below 0 or reaches past
 * runs_cap is the all-zero canvas with total 0; runs at index >= runs_cap are never read.
 * Slots may overlap or repeat. offsets: device memory. masks: any byte address (dword stores
 * where W % 4 == 0 and masks is 4-B aligned, byte stores otherwise).
 * Refused with ISG_ERR_INVALID before any HIP call: n < 0, H <= 0, W <= 0, H*W >= 2^31,
 * runs_cap < 0, a NULL pointer that would be used (runs and work may be NULL when
 * runs_cap == 0), offsets / totals / work not 8-B aligned, runs not 4-B aligned.
 * runs_cap >= 2^31 is ISG_ERR_UNSUPPORTED. n == 0 does nothing.
 * Capturable: the launch geometry depends on (n, H, W, runs_cap) only, nothing is allocated
 * or synchronised, and the result does not depend on what masks, totals or work held.
 * work: isg_mask_rle_decode_workspace(n,H,W,runs_cap) bytes (-1 for sizes the call
 * refuses), caller-owned. */
int64_t isg_mask_rle_decode_workspace(int32_t n, int32_t H, int32_t W, int64_t runs_cap);
int32_t isg_mask_rle_decode(const uint32_t* runs, int64_t runs_cap,
                            const int64_t* offsets /* [n+1], device */, int32_t n,
                            int32_t H, int32_t W, uint8_t* masks /* [n,H,W] */,
                            int64_t* totals /* [n] */, void* work, isg_stream_t stream);

/* The COCO `counts` string of every slot, with its box and area (csrc/mask_rle_string.hip;
 * the contract is stated on the CPU by instancesegmentation_amd/rle.py `compress` and
 * `summarize`). isg_mask_rle's runs / offsets / runs_cap plug in unchanged. Slot j < n turns
 * the counts c = runs[offsets[j] .. offsets[j+1]) into the bytes
 * chars[char_offsets[j] .. char_offsets[j+1]), slots packed in slot order from 0: count i is
 * written as v = c_i (i <= 2) or c_i - c_{i-2} (signed, 64 bits) in the fewest n of 1..7
 * groups with -2^(5n-1) <= v < 2^(5n-1), group k = (((v >> 5k) & 31) | (k < n-1 ? 32 : 0))
 * + 48. boxes[j] = [x, y, w, h], the tight box of the canvas isg_mask_rle_decode gives for
 * the slot (runs clipped at H*W, zero-length runs stepped over, a set run across a column
 * seam spans y = 0..H-1, [0,0,0,0] without a set pixel), areas[j] its set pixels.
 * A slot whose range is empty or reversed, starts below 0 or reaches past runs_cap is void:
 * no characters, box [0,0,0,0], area 0; runs at index >= runs_cap are never read. Slots may
 * overlap or repeat. offsets: device memory.
 * Overflow: all n + 1 char_offsets always hold the true values; chars[i] is written only for
 * i < chars_cap (chars may be NULL when chars_cap == 0, at any byte address otherwise); boxes
 * and areas do not depend on it. Nothing is raised on the device.
 * Refused with ISG_ERR_INVALID before any HIP call: n < 0, a capacity < 0, H <= 0, W <= 0,
 * H*W >= 2^31, a NULL pointer that would be used (runs may be NULL when runs_cap == 0),
 * offsets / char_offsets / areas / work not 8-B aligned, runs / boxes not 4-B aligned. A
 * capacity >= 2^31 is ISG_ERR_UNSUPPORTED. n == 0 does nothing.
 * Capturable: the launch geometry depends on n only (one workgroup per slot, which walks its
 * slot in chunks of isg_rle_string_chunk() counts), nothing is allocated or synchronised, and
 * no result depends on what chars, char_offsets, boxes, areas or work held.
 * work: isg_rle_compress_workspace(n, runs_cap) bytes (-1 for sizes the call refuses). */
int32_t isg_rle_string_chunk(void);
int64_t isg_rle_compress_workspace(int32_t n, int64_t runs_cap);
int32_t isg_rle_compress(const uint32_t* runs, int64_t runs_cap,
                         const int64_t* offsets /* [n+1], device */, int32_t n, int32_t H,
                         int32_t W, uint8_t* chars, int64_t chars_cap,
                         int64_t* char_offsets /* [n+1] */, int32_t* boxes /* [n][4] */,
                         int64_t* areas /* [n] */, void* work, isg_stream_t stream);

/* `counts` strings back to counts (csrc/mask_rle_string.hip; the contract is stated on the
 * CPU by instancesegmentation_amd/rle.py `parse_total`): the inverse of isg_rle_compress,
 * whose chars / char_offsets plug in unchanged, and the feeder of isg_mask_rle_decode, which
 * takes runs / offsets / runs_cap as they come out. Slot j < n reads the bytes
 * chars[char_offsets[j] .. char_offsets[j+1]) as g = (byte - 48) & 63; a byte with
 * g & 32 == 0 ends a count, so the slot has as many counts as terminators, written to
 * runs[offsets[j] .. offsets[j+1]), slots packed in slot order from 0. A count of k groups is
 * worth its last min(k, 7): the sum of (g & 31) << 5m, lowest first, sign-extended from bit
 * 5 min(k, 7) when the terminator has g & 16; count i >= 3 adds count i - 2 (64 bits,
 * wrapping); the low 32 bits are stored. status[j] is the OR of 1 TRUNCATED (the last byte
 * continues; its groups yield no count), 2 BAD_CHAR (a byte outside 48..111), 4 TOO_LONG (a
 * count of more than 7 groups), 8 RANGE (a count outside [0, 2^32)); the caller judges,
 * nothing is raised on the device.
 * A slot whose range is empty or reversed, starts below 0 or reaches past chars_cap is void:
 * no counts, status 0; chars at index >= chars_cap are never read. Slots may overlap.
 * Overflow: all n + 1 offsets always hold the true values; runs[i] is written only for
 * i < runs_cap (runs may be NULL when runs_cap == 0); status does not depend on it.
 * Refusals, n == 0 and capturability as isg_rle_compress (8-B: char_offsets, offsets, work;
 * 4-B: runs, status; chars at any byte).
 * work: isg_rle_parse_workspace(n, chars_cap) bytes (-1 for sizes the call refuses). */
int64_t isg_rle_parse_workspace(int32_t n, int64_t chars_cap);
int32_t isg_rle_parse(const uint8_t* chars, int64_t chars_cap,
                      const int64_t* char_offsets /* [n+1], device */, int32_t n,
                      uint32_t* runs, int64_t runs_cap, int64_t* offsets /* [n+1] */,
                      int32_t* status /* [n] */, void* work, isg_stream_t stream);

/* ---- scoring (csrc/mask_eval.hip) ------------------------ */

/* Crop-space validation IoU counts (the contract is stated on the CPU by
 * instancesegmentation_amd/evaluate.py `crop_iou_counts_cpu`; it is
 * train_loop.tensors_mean_iou's tensor2mask followed by >= 128). pred, target: [B][hw]
 * fp32, any 4-B aligned address. Per sample b, counts[b] = (|P and T|, |P or T|) with
 *   T = fp32(target * 255) >= 128,   P = fp32(p * 255) >= 128,
 *   p = pred, or with from_logits != 0 the sigmoid of isg_sigmoid_fwd, 1/(1 + expf(-pred))
 * (the same device function, so counting the logits equals counting their stored
 * probabilities bit for bit). One fp32 multiply, no contraction; NaN is background. The
 * counts are exact integers and are OVERWRITTEN, not accumulated: a caller that validates
 * several batches passes counts + 2 * offset and reads one table back at the end.
 * Refused with ISG_ERR_INVALID before any HIP call: B < 0, hw <= 0, and with B > 0 a NULL
 * pointer, pred / target not 4-B aligned or counts not 8-B aligned. B == 0 does nothing.
 * Capturable: nothing is allocated or synchronised. */
int32_t isg_mask_iou_crops(const float* pred, const float* target, int32_t B, int64_t hw,
                           int32_t from_logits, int64_t* counts /* [B][2] */,
                           isg_stream_t stream);

/* Detections x ground truth on image canvases (evaluate.py `iou_matrix_cpu`): det [K,H,W]
 * and gt [G,H,W] uint8 at any byte address, foreground >= 128 (the NMS contract's
 * threshold). inter[i][j] = |det_i and gt_j|, area_det[i] = |det_i|, area_gt[j] = |gt_j|,
 * exact integers (H*W < 2^31, else ISG_ERR_INVALID). Both stacks are bit-packed as the
 * NMS packs its masks (csrc/mask_bits.h), the areas taken in the same pass, then one
 * workgroup per pair runs AND-popcount over the words.
 * K == 0 or G == 0 is valid: only the non-empty outputs are written (inter needs both).
 * K + G <= 65535, more is ISG_ERR_UNSUPPORTED. The result does not depend on what work,
 * inter or the areas held. Refused before any HIP call: K < 0, G < 0, H <= 0, W <= 0, a
 * NULL pointer that would be used, work not 8-B aligned.
 * work: isg_mask_iou_matrix_workspace(K,G,H,W) bytes (-1 for sizes the call refuses),
 * caller-owned. */
int64_t isg_mask_iou_matrix_workspace(int32_t K, int32_t G, int32_t H, int32_t W);
int32_t isg_mask_iou_matrix(const uint8_t* det, int32_t K, const uint8_t* gt, int32_t G,
                            int32_t H, int32_t W, void* work, int32_t* inter /* [K][G] */,
                            int32_t* area_det /* [K] */, int32_t* area_gt /* [G] */,
                            isg_stream_t stream);

/* ---- infer pre-process ----------------------------- */

/* Per-instance crop: window k = (x0,y0,x1,y1) of an HxWx3 uint8 RGB image (instance box
 * +/- 16 px, may reach outside the image) resampled to SxS, rounded to uint8 and
 * normalised to [-1,1] into out[K][3][S][S]; pixels outside valid[k] = (x0,y0,x1,y1)
 * (the image minus what the centring translation moved out of the frame) read as the
 * fill value 0. Replaces the reference's translate + CropAndPad + Resize +
 * ToTensor/Normalize test branch (train_instance.py:139-196, :80-85; imgaug/cv2 absent:
 * contract frozen in oracle/infer_oracle.py, bit-exact). */
int32_t isg_instance_crop(const uint8_t* image, int32_t H, int32_t W, const int32_t* windows,
                          const int32_t* valid, int32_t K, int32_t S, float* out,
                          isg_stream_t stream);

/* keypoint2heatmaps (train_instance.py:33-68) for K instances: keypoints[K][nparts][3] =
 * (x, y, visible) in double, out[K][nparts][H][W] float32 (zeroed, then each visible
 * keypoint's window written with the float32 of the double-precision Gaussian). */
int32_t isg_keypoint_heatmaps(const double* keypoints, int32_t K, int32_t nparts, int32_t H,
                              int32_t W, double sigma, double threshold, float* out,
                              isg_stream_t stream);

/* ---- training batches (csrc/train_crop.hip) -------------------------------- */

/* One sample of a training batch inside the packed uint8 arena: its image (H x W x 3, HWC)
 * at byte img_off, its instance mask (H x W) at byte mask_off, and valid = (x0,y0,x1,y1),
 * the rectangle the reference's centring translation keeps in the frame (data.py
 * centring_valid). Offsets need no alignment: the kernels read bytes, and dwords only at
 * addresses they have aligned themselves. */
typedef struct {
    int64_t img_off, mask_off;
    int32_t H, W;
    int32_t valid[4];
} isg_train_sample;

#define ISG_TRAIN_PARTS 17 /* keypoints per sample (data.py ORDER_PART_NAMES) */
#define ISG_TRAIN_PAD 16   /* the window is the mask box +/- this (train_instance.py:166) */

/* The loader's crop on the GPU for the first n of B samples (the CPU statement is
 * data.py InstanceCommonDataset.__getitem__ / instance_window, bit for bit):
 *   stage A  the exclusive-max box of the non-zero mask pixels, over the whole mask and over
 *            the mask inside valid, reduced in the wave and the workgroup, one slot of work
 *            per workgroup, the slots reduced by stage B (a second tiny pass: no atomics);
 *            the window is the clipped box if there is one, else the whole-mask box, else
 *            (0,0,W,H), then +/- ISG_TRAIN_PAD. It never leaves the device.
 *   stage B  that window of the image resampled to x[b][3][S][S] = (q/255 - 0.5)/0.5 and of
 *            the mask to mask[b][1][S][S] = q/255 by isg_instance_crop's arithmetic (q the
 *            uint8 rounded half up; coordinates clamped into the window; 0 outside valid);
 *            kp_out[b][j] = ((x - wx0) * S / (wx1 - wx0), same in y, visible > 0 ? 1 : 0) in
 *            double for every part; windows[b] = (x0,y0,x1,y1).
 * samples is HOST memory (n entries, passed to the kernels by value, ISG_LIST_CHUNK/2 a
 * launch); arena, keypoints [B][17][3], work and the outputs are device memory. Rows
 * n .. B-1 of every output are not written. 16-byte stores are used when S % 4 == 0 and x
 * and mask are 16-byte aligned, 4-byte stores otherwise. Every word of work that is read was
 * written earlier in the same call (nothing depends on an earlier call, nothing needs
 * clearing); isg_train_crop_workspace(B) bytes (2 KiB a sample), caller-owned.
 * Refused with ISG_ERR_INVALID before any HIP call: a NULL pointer, S <= 0, n < 0 or n > B,
 * a sample with H or W <= 0, with 3*H*W >= 2^31, or reaching outside [0, arena_bytes).
 * n == 0: nothing is launched, returns 0. */
int64_t isg_train_crop_workspace(int32_t B);
int32_t isg_train_crop(const uint8_t* arena, int64_t arena_bytes, const isg_train_sample* samples,
                       const double* keypoints, int32_t n, int32_t B, int32_t S, void* work,
                       float* x, float* mask, double* kp_out, int32_t* windows,
                       isg_stream_t stream);

/* The augmentation of one sample, drawn by the host (augment.py draw_augment): the kernel takes
 * parameters, never probabilities. All zero but rot_cos = contrast = mult[] = 1 is the identity. */
typedef struct {
    double rot_cos, rot_sin; /* rotation of the output grid about the crop's centre; (1, 0) = none */
    int32_t jitter[4];       /* each in [-1024, 1024]: side i of the padded window (x0, y0, x1, y1)
                              * moves by floor(jitter[i] * (box extent / 5) / 1024) pixels */
    int32_t flip;            /* 0 / 1: mirror the columns, exchange the left and right keypoints */
    int32_t noise_per_channel; /* 0: one noise value a pixel for the three planes; 1: one each */
    float contrast;          /* q -> (q - 127) * contrast + 127 */
    float noise;             /* q -> q + (s - 510) * noise, s the sum of four Philox bytes; 0 = none */
    float mult[3];           /* q -> q * mult[c] */
    int32_t pad_;
} isg_train_aug;

#define ISG_TRAIN_AUG_MAX 65536.0f /* upper bound of contrast, noise and mult[] */

/* isg_train_crop with random geometry and colour in stage B (the CPU statement is augment.py
 * augment_sample, bit for bit; stage A is isg_train_crop's):
 *   window   the box before the pad is isg_train_crop's (bx0,by0,bx1,by1); ax = (bx1-bx0)/5,
 *            ay = (by1-by0)/5; x0 = bx0 - 16 + floor(jitter[0]*ax/1024), x1 = bx1 + 16 +
 *            floor(jitter[2]*ax/1024), y0 and y1 alike with jitter[1], jitter[3] and ay.
 *   geometry rot = (1, 0): isg_train_crop's resampling of that window; flip writes column u
 *            from column S-1-u. Otherwise output (u, v), u un-flipped, samples the crop at
 *            p = R (u + 0.5 - S/2, v + 0.5 - S/2) + S/2, R = [[cos, -sin], [sin, cos]] in float,
 *            mapped into the image like an output centre ((p * scale) - 0.5) + lo; bilinear
 *            taps at floor and floor + 1 without clamping, 0 outside valid and the image.
 *   colour   on the quantised image planes, each step rounded half up and clamped to 0..255:
 *            contrast, noise, mult (see the record); then (q/255 - 0.5)/0.5. The noise of output
 *            pixel i = v*S + u of sample b is Philox4x32-10 with key (seed lo, seed hi) and
 *            counter (i lo, i hi, o lo, o hi), o = ordinal0 + b; plane c sums the four bytes of
 *            output word c (noise_per_channel) or word 0.
 *   keypoints  projected as by isg_train_crop, then (if rotated) R^T applied about (S/2, S/2),
 *            then (if flipped) x -> S - x and the left/right rows exchanged with visibility.
 * aug is HOST memory, n records, passed by value with the sample descriptors. Everything
 * isg_train_crop refuses is refused, and also: aug == NULL, a jitter outside +/-1024,
 * |cos^2 + sin^2 - 1| > 1e-6, flip or noise_per_channel not 0 / 1, a contrast, noise or mult
 * that is negative, not finite or above ISG_TRAIN_AUG_MAX. With identity records the outputs
 * are isg_train_crop's. */
int32_t isg_train_crop_aug(const uint8_t* arena, int64_t arena_bytes, const isg_train_sample* samples,
                           const isg_train_aug* aug, uint64_t seed, uint64_t ordinal0,
                           const double* keypoints, int32_t n, int32_t B, int32_t S, void* work,
                           float* x, float* mask, double* kp_out, int32_t* windows,
                           isg_stream_t stream);

/* ---- keypoint stem ------------------------------------ */

/* The stem of Segment(20) (init_head_s4, segment.py:19-31, on cat(image, heatmaps),
 * segment.py:531-532) with the 17 heatmaps (train_instance.py:33-68) never written to
 * HBM: map j of image n is exp(-((x-kx)^2+(y-ky)^2)/sigma^2) (double, stored float) inside
 * keypoint j's window [max(0,int(kx-r)), min(W-1,int(kx+r+1))) x (same in y), where it
 * exceeds the threshold, and 0 elsewhere; keypoints[n][j] = (kx, ky, visible > 0).
 *   fwd  : y[n][co] += sum_{j,tap} w[co][c_kp0+j][tap] * map_j   over the output pixels a
 *          window reaches (y holds the dense conv of the first c_kp0 channels + bias);
 *          stats (BN sum / sum^2 replicas, 4*Co doubles each) get the change of sum and
 *          sum^2 of every changed pixel
 *   wgrad: dw[co][c_kp0+j][tap] += sum_p dy[co][p] * map_j(tap(p)), dy a vtensor
 *   pool : out[n][c0+j] = max_pool(map_j, k) (k x k windows, stride k)
 * geom: the conv (Ci = the weight's input channels, Co <= 16, groups 1).
 * A keypoint with visible <= 0, or a NaN or infinite coordinate, draws nothing; finite
 * coordinates of any size are safe (a window wholly outside the image is empty).
 * Refused before any launch, nothing written. With r = sqrt(-log(threshold)) * sigma:
 *   all three, ISG_ERR_INVALID: a NULL descriptor or kp, nparts outside 1..32, sigma <= 0 or
 *     NaN, threshold outside (0, 1) or NaN, g.N, g.H or g.W < 1;
 *   all three, ISG_ERR_UNSUPPORTED: r > 120;
 *   fwd and wgrad, ISG_ERR_UNSUPPORTED: groups != 1, Co outside 1..16, KH*KW > 49, a stride
 *     or dilation < 1, c_kp0 < 0, c_kp0 + nparts != Ci, or a 16 x 16 output tile's footprint
 *     S*15 + D*(K-1) + 1 above 64 on either axis;
 *   fwd: NULL w or y (ISG_ERR_INVALID); 16 * nparts * KH*KW > 8192 (ISG_ERR_UNSUPPORTED);
 *   wgrad, in this order: a residual-form dy (ISG_ERR_UNSUPPORTED); NULL dw, dy.nseg != 1 or
 *     dy.s[0].C != Co (ISG_ERR_INVALID); nrep < 1, or nrep > 1 with rep_stride <= 0
 *     (ISG_ERR_INVALID); Co * KH*KW > 512 (ISG_ERR_UNSUPPORTED); a widest window, int(2r) + 2
 *     pixels, that reaches more than 256 output columns, (int(2r) + 1 + DW*(KW-1))/SW + 1, or
 *     whose staged footprint exceeds 4096 floats at any column count nc up to that:
 *     ((nr-1)*SH + DH*(KH-1) + 1) * ((nc-1)*SW + DW*(KW-1) + 1) with nr = min(max(1, 256/nc),
 *     ceil(nrow/4)), nrow the row count alike (ISG_ERR_UNSUPPORTED);
 *   pool: NULL out, k < 1, or k not dividing g.H and g.W (ISG_ERR_INVALID). */
typedef struct {
    const double* kp;            /* [N][nparts][3] */
    int32_t nparts, c_kp0;
    double sigma, threshold;
    isg_conv_geom g;
    const float* w;              /* fwd */
    float* y;                    /* fwd: raw conv output [N][Co][OH][OW] */
    int64_t y_n_stride;
    double* stats;               /* fwd: NULL or the output's BN statistics block */
    isg_vtensor dy;              /* wgrad */
    double* dw;                  /* wgrad: [Co][Ci][KH][KW] fp64 (+ replicas) */
    int64_t rep_stride;
    int32_t nrep;
    int32_t k;                   /* pool: window */
    float* out;                  /* pool */
    int64_t out_n_stride;
} isg_kp_stem;

int32_t isg_kp_stem_fwd(const isg_kp_stem* a, isg_stream_t stream);
int32_t isg_kp_stem_wgrad(const isg_kp_stem* a, isg_stream_t stream);
int32_t isg_kp_pool(const isg_kp_stem* a, isg_stream_t stream);

/* ---- fused mask head (segment.py:435-438, 504-505) ------------------------ */

/* bottle6_1 = ConvTranspose2d(16 -> 4, k8, s4, p2) followed by bottle6_2 = Conv2d(4 -> 1,
 * 3x3, p1) (no nonlinearity between them), with the 4-channel full-resolution
 * intermediate kept on chip (never recomputed in the backward).
 *   fwd: out = logits [N,1,4Hi,4Wi]; when `ring` is non-NULL also the UN-cropped
 *        intermediate (bias included) on the one-pixel ring just outside the 4Hi x 4Wi
 *        image, per image [4 channels][ISG_HEAD_RING(Hi, Wi)]: row -1 (columns -1 .. 4Wi),
 *        row 4Hi (same), column -1 (rows 0 .. 4Hi-1), column 4Wi (same). The backward
 *        needs it (the 3x3's weight gradient border term).
 *   bwd: dx (sinks: STORE / ACCUM without statistics) = dL/dx; dw1/db1/dw2/db2 += the
 *        parameter gradients, added into replica (workgroup % nrep) of each (replica r at
 *        + r*rep_stride elements; NULL skips one); `ring` as written by the forward
 *        (required). Replaces the unfused isg_convT_fwd + isg_conv_fwd (+ their dgrad /
 *        wgrad) pair, which round-trips the intermediate through HBM.
 * Refused before any launch. ISG_ERR_INVALID: NULL w1 / w2, N, Hi or Wi < 1, NULL out (fwd),
 * NULL dout or ring (bwd), nrep < 1, or nrep > 1 without a rep_stride. ISG_ERR_UNSUPPORTED: a
 * residual input or sink form, nseg outside 1..ISG_MAX_SEGS, a segment with C <= 0, segments
 * that do not add up to 16 channels, x.N / x.H / x.W other than N / Hi / Wi, N*16*Hi*Wi >=
 * 2^31; in the backward also nsink outside 0..ISG_MAX_SEGS (0: no input gradient), with
 * nsink > 0 sinks that do not cover [0, 16) in order (s[0].c0 = 0, s[i].c0 = s[i-1].c0 +
 * s[i-1].C, the last ending at 16; sinks need not split where the segments do), an ACTBWD
 * sink, a STORE / ACCUM sink with statistics or without a buffer, and a sink with `bias` (the
 * kernel would not apply it).
 * isg_last_launch after the backward names the instantiation: "head_bwd_kernel<vec>" (16-B
 * staging and dx stores: Wi % 4 == 0 and dout, every segment's p and every written sink's p
 * 16-B aligned with image strides that are multiples of 4) or "head_bwd_kernel<scalar>". */
#define ISG_HEAD_RING(Hi, Wi) (2 * (4 * (int64_t)(Wi) + 2) + 2 * 4 * (int64_t)(Hi))
typedef struct {
    isg_vtensor x;               /* [N,16,Hi,Wi] */
    const float* w1;             /* ConvTranspose2d weight [16][4][8][8] */
    const float* b1;             /* [4] or NULL */
    const float* w2;             /* Conv2d weight [1][4][3][3] */
    const float* b2;             /* [1] or NULL */
    float* out;                  /* fwd */
    int64_t out_n_stride;
    const float* dout;           /* bwd: dL/dlogits */
    int64_t dout_n_stride;
    isg_sinks dx;                /* bwd */
    double* dw1;                 /* bwd: fp64 accumulators (+ replicas, isg_conv_wgrad_rep) */
    double* db1;
    double* dw2;
    double* db2;
    int64_t rep_stride;
    int32_t nrep;
    int32_t N, Hi, Wi;
    int32_t pad_;
    float* ring;                 /* [N][4][ISG_HEAD_RING(Hi, Wi)] (fwd: written if non-NULL; bwd: read) */
    /* bwd: non-NULL = each workgroup STORES its fp32 dW1 partial here ([blocks][4096],
     * isg_mask_head_part_floats) instead of adding it into dw1, and isg_mask_head_fold
     * adds the partials into dw1's replicas later (off the critical path: the end-of-
     * workgroup fp64 atomics of the 4096 dW1 values were the kernel's tail) */
    float* dw1_part;
} isg_mask_head;

int32_t isg_mask_head_fwd(const isg_mask_head* a, isg_stream_t stream);
int32_t isg_mask_head_bwd(const isg_mask_head* a, isg_stream_t stream);
/* floats of the backward's dW1 partial slab for an N x 16 x Hi x Wi input */
int64_t isg_mask_head_part_floats(int32_t N, int32_t Hi, int32_t Wi);
/* dw1 replicas += the partial slab (fp64 sums of the fp32 partials: exact, so the result
 * is the one of the in-kernel atomics, bit for bit) */
int32_t isg_mask_head_fold(const isg_mask_head* a, isg_stream_t stream);

/* ---- plan executor ------------------------------------------------------ */

/* A recorded op list (built once per input shape by the Python planner) replayed
 * with a table of base pointers: pointer = table[slot] + byte offset. */
typedef struct {
    int32_t slot;
    int32_t pad_;
    int64_t offset;
} isg_ref;

int32_t isg_exec(const void* ops, int32_t nops, void* const* table, isg_stream_t stream);

/* Same, with a side stream: ops flagged "side" in their record header (the weight
 * gradients, which nothing later in the list reads) are forked onto `side` after every
 * op issued before them on `stream`; ops flagged "join" (and the end of the list) wait
 * for all forked work. side == NULL runs everything on `stream`. Under HIP-graph
 * capture the fork/join become graph edges, so the weight gradients overlap the
 * input-gradient chain. Header flags (csrc/exec.cpp OpHdr.flags): bit 0 side, bit 1 join,
 * bit 2 fork-now (the side op depends on everything issued on `stream` so far; consecutive
 * fork-now ops share one fork), bits 8+ of a join: how many of the most recent side ops it
 * does NOT wait for (0: all). Side ops are otherwise issued in batches of 16 behind one
 * fork each. */
int32_t isg_exec_ms(const void* ops, int32_t nops, void* const* table, isg_stream_t stream,
                    isg_stream_t side);

/* Same with a second side stream: a forked batch made only of weight gradients (independent
 * atomic accumulations) is dealt alternately over `side` and `side2`, so two of their small
 * grids run at once; every other side op stays in order on `side`. side2 == NULL is
 * isg_exec_ms. */
int32_t isg_exec_ms2(const void* ops, int32_t nops, void* const* table, isg_stream_t stream,
                     isg_stream_t side, isg_stream_t side2);

/* sizeof() of the ABI structs and executor records (0 vtensor, 1 sinks, 2 conv record,
 * 3 wgrad record, 4 pool record, 5 tail, 6 tail_grad, 7 bn_update, 8 grad_final,
 * 9 bce record, 10 conv_geom, 11 bn, 12 vseg, 13 sink, 14 sum_rep record, 15 kp_stem,
 * 16 mask_head, 17 stamp record, 18 depthwise-backward record, 19 step tail,
 * 20 train sample) so bindings can verify layouts. */
int32_t isg_record_size(int32_t which);

const char* isg_last_error(void);
/* The kernel name given to this thread's latest launch check (e.g. "tap_conv_kernel"; an error
 * return before the launch appends ": dynamic LDS"), "" before any: a static string, for tests
 * that assert which kernel a dispatch chain chose. Costs one thread-local pointer store. */
const char* isg_last_launch(void);
int32_t isg_abi_version(void);
/* ISG_STAT_REP the library was built with (accumulator replica count). */
int32_t isg_stat_replicas(void);

#ifdef __cplusplus
}
#endif
#endif
