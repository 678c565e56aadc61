// Scoring on the GPU: the two integer count kernels under the mask IoU
// metric. Their contracts are stated on the CPU by instancesegmentation_amd/evaluate.py
// (crop_iou_counts_cpu, iou_matrix_cpu) and the kernels are bit-exact to them: the only
// float op is one fp32 multiply per value (contraction off), everything after is integer.
//
//   isg_mask_iou_crops  : per training / validation crop, (|P and T|, |P or T|) of the
//                         thresholded prediction and target (train_loop.tensors_mean_iou);
//   isg_mask_iou_matrix : detections x ground truth intersections and areas on image
//                         canvases (mask >= 128, the NMS contract's threshold).
#include <algorithm>

#include "common.h"
#include "mask_bits.h"

namespace {

constexpr int kThreads = 256;

// tensor2mask followed by >= 128 (train_loop.py): uint8(v * 255) >= 128 is v * 255 >= 128
// for every v the truncation is defined for; NaN compares false (background).
ISG_DEV bool crop_fg(float v) {
#pragma clang fp contract(off)
    return v * 255.f >= 128.f;
}

template <bool kLogits>
ISG_DEV void crop_count(float p, float t, int& inter, int& uni) {
    const bool P = crop_fg(kLogits ? sigmoid_f(p) : p);
    const bool T = crop_fg(t);
    inter += (P && T) ? 1 : 0;
    uni += (P || T) ? 1 : 0;
}

// kCropQ 16-B quads of each operand per thread, all loads in flight before the first use
// (as bce4_kernel). Workgroup blockIdx.x % bps of sample blockIdx.x / bps owns quads
// [bx * kThreads * kCropQ, ...) of the sample's 16-B aligned middle; the <= 3 floats before
// it and after it are read one by one. When the two operands of a sample sit at different
// offsets from a 16-B boundary there is no common middle: the whole sample is read one
// float at a time (nq = 0). One 64-bit atomic per count per workgroup: 29 workgroups per
// 480^2 sample, so 29 adds per address.
constexpr int kCropQ = 8;

template <bool kLogits>
__global__ __launch_bounds__(kThreads) void iou_crops_kernel(const float* __restrict__ pred,
                                                              const float* __restrict__ target,
                                                              int64_t hw, int bps,
                                                              unsigned long long* __restrict__ counts) {
    __shared__ int sh[2][4];
    const int b = (int)(blockIdx.x / (unsigned)bps), bx = (int)(blockIdx.x % (unsigned)bps);
    const float* p = pred + (int64_t)b * hw;
    const float* t = target + (int64_t)b * hw;
    const unsigned ap = (unsigned)((uintptr_t)p & 15u), at = (unsigned)((uintptr_t)t & 15u);
    int64_t head = 0, nq = 0;
    if (ap == at) {
        head = (int64_t)(((16u - ap) & 15u) >> 2);
        head = head < hw ? head : hw;
        nq = (hw - head) >> 2;
    }
    int inter = 0, uni = 0;
    const int64_t q0 = (int64_t)bx * kThreads * kCropQ;
    if (q0 < nq) {  // uniform over the workgroup; nq >= 1, so quad 0 is readable
        f32x4 x[kCropQ], y[kCropQ];
#pragma unroll
        for (int u = 0; u < kCropQ; ++u) {
            const int64_t q = q0 + (int64_t)u * kThreads + threadIdx.x;
            x[u] = gld4(p, head + 4 * (q < nq ? q : 0));
            y[u] = gld4(t, head + 4 * (q < nq ? q : 0));
        }
#pragma unroll
        for (int u = 0; u < kCropQ; ++u) {
            const int64_t q = q0 + (int64_t)u * kThreads + threadIdx.x;
            if (q < nq) {
#pragma unroll
                for (int e = 0; e < 4; ++e) crop_count<kLogits>(x[u][e], y[u][e], inter, uni);
            }
        }
    }
    // the floats outside the quads: [0, head) and [head + 4 nq, hw), dealt over the sample's
    // workgroups (6 at the most unless the operands are misaligned to each other)
    const int64_t ns = hw - 4 * nq;
    for (int64_t e = (int64_t)bx * kThreads + threadIdx.x; e < ns; e += (int64_t)bps * kThreads) {
        const int64_t i = e < head ? e : e + 4 * nq;
        crop_count<kLogits>(gld(p, i), gld(t, i), inter, uni);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        inter += __shfl_xor(inter, o, 64);
        uni += __shfl_xor(uni, o, 64);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        sh[0][wave] = inter;
        sh[1][wave] = uni;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int* s = sh[threadIdx.x];
        const int v = s[0] + s[1] + s[2] + s[3];
        if (v) atomicAdd(&counts[2 * (int64_t)b + threadIdx.x], (unsigned long long)v);
    }
}

// Both stacks bit-packed in one launch (blockIdx.y < K: detection, else ground truth), the
// area of each mask from the same pass. The stacks may start at any byte.
__global__ __launch_bounds__(kThreads) void eval_pack_kernel(const uint8_t* __restrict__ det, int K,
                                                              const uint8_t* __restrict__ gt,
                                                              int64_t hw, int64_t words,
                                                              unsigned long long* __restrict__ bits,
                                                              int32_t* __restrict__ area_det,
                                                              int32_t* __restrict__ area_gt) {
    __shared__ unsigned long long sc[4];
    const int k = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint8_t* src = k < K ? det + (int64_t)k * hw : gt + (int64_t)(k - K) * hw;
    const bool dword = ((uintptr_t)src & 3u) == 0;
    unsigned long long* row = bits + (int64_t)k * words;
    const int64_t groups = words / 4;
    unsigned long long cnt = 0, sum = 0;
    for (int64_t g = (int64_t)blockIdx.x * 4 + wave; g < groups; g += (int64_t)gridDim.x * 4) {
        const uint32_t v4 = mask_load_px4(src, g * 256 + 4 * lane, hw, dword);
        mask_ballot_px4(v4, lane, row + 4 * g, cnt, sum);
    }
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if (lane == 0) sc[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int v = (int)(sc[0] + sc[1] + sc[2] + sc[3]);
        if (v) atomicAdd(k < K ? &area_det[k] : &area_gt[k - K], v);
    }
}

// One workgroup per (detection i, ground truth j): AND-popcount over the packed words, four
// loads of each row in flight per thread.
constexpr int kInterU = 4;

__global__ __launch_bounds__(kThreads) void eval_inter_kernel(int K, int G, int64_t words,
                                                               const unsigned long long* __restrict__ bits,
                                                               int32_t* __restrict__ inter) {
    __shared__ int sh[4];
    const int i = blockIdx.x, j = blockIdx.y;
    const unsigned long long* a = bits + (int64_t)i * words;
    const unsigned long long* b = bits + (int64_t)(K + j) * words;
    int c = 0;
    for (int64_t t0 = threadIdx.x; t0 < words; t0 += kInterU * kThreads) {
        unsigned long long va[kInterU], vb[kInterU];
#pragma unroll
        for (int u = 0; u < kInterU; ++u) {
            const int64_t t = t0 + (int64_t)u * kThreads;
            va[u] = a[t < words ? t : t0];
            vb[u] = b[t < words ? t : t0];
        }
#pragma unroll
        for (int u = 0; u < kInterU; ++u)
            if (t0 + (int64_t)u * kThreads < words) c += __popcll(va[u] & vb[u]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) sh[wave] = c;
    __syncthreads();
    if (threadIdx.x == 0) inter[(int64_t)i * G + j] = sh[0] + sh[1] + sh[2] + sh[3];
}

constexpr int kMaxGridY = 65535;

// NULL / range checks of isg_mask_iou_matrix: host code, nothing is dereferenced
int32_t check_matrix(int32_t K, int32_t G, int32_t H, int32_t W) {
    if (K < 0 || G < 0 || H <= 0 || W <= 0)
        return isg_set_error(ISG_ERR_INVALID, "mask_iou_matrix: bad sizes K=%d G=%d H=%d W=%d", K, G,
                             H, W);
    if ((int64_t)H * W >= ((int64_t)1 << 31))
        return isg_set_error(ISG_ERR_INVALID, "mask_iou_matrix: H*W = %lld needs < 2^31",
                             (long long)((int64_t)H * W));
    if ((int64_t)K + G > kMaxGridY)
        return isg_set_error(ISG_ERR_UNSUPPORTED, "mask_iou_matrix: K + G = %lld (max %d)",
                             (long long)((int64_t)K + G), kMaxGridY);
    return ISG_OK;
}

}  // namespace

extern "C" {

int32_t isg_mask_iou_crops(const float* pred, const float* target, int32_t B, int64_t hw,
                           int32_t from_logits, int64_t* counts, isg_stream_t st) {
    if (B < 0 || hw <= 0)
        return isg_set_error(ISG_ERR_INVALID, "mask_iou_crops: bad sizes B=%d hw=%lld", B,
                             (long long)hw);
    if (B == 0) return ISG_OK;
    if (!pred || !target || !counts)
        return isg_set_error(ISG_ERR_INVALID, "mask_iou_crops: NULL pointer");
    if (((uintptr_t)pred & 3u) || ((uintptr_t)target & 3u) || ((uintptr_t)counts & 7u))
        return isg_set_error(ISG_ERR_INVALID, "mask_iou_crops: pred / target need 4-B alignment, "
                             "counts 8-B");
    const int64_t quads = (hw + 3) / 4;
    const int64_t bps = std::max<int64_t>(1, (quads + kThreads * kCropQ - 1) / (kThreads * kCropQ));
    if (bps * B >= ((int64_t)1 << 31))
        return isg_set_error(ISG_ERR_UNSUPPORTED, "mask_iou_crops: %lld workgroups",
                             (long long)(bps * B));
    if (hipMemsetAsync(counts, 0, (size_t)B * 2 * sizeof(int64_t), st) != hipSuccess)
        return isg_check_launch("mask_iou_crops memset");
    const dim3 grid((unsigned)(bps * B));
    if (from_logits)
        hipLaunchKernelGGL(iou_crops_kernel<true>, grid, dim3(kThreads), 0, st, pred, target, hw,
                           (int)bps, (unsigned long long*)counts);
    else
        hipLaunchKernelGGL(iou_crops_kernel<false>, grid, dim3(kThreads), 0, st, pred, target, hw,
                           (int)bps, (unsigned long long*)counts);
    return isg_check_launch("iou_crops_kernel");
}

int64_t isg_mask_iou_matrix_workspace(int32_t K, int32_t G, int32_t H, int32_t W) {
    if (K < 0 || G < 0 || H <= 0 || W <= 0) return -1;
    return ((int64_t)K + G) * mask_bit_words((int64_t)H * W) * 8;
}

int32_t isg_mask_iou_matrix(const uint8_t* det, int32_t K, const uint8_t* gt, int32_t G, int32_t H,
                            int32_t W, void* work, int32_t* inter, int32_t* area_det,
                            int32_t* area_gt, isg_stream_t st) {
    const int32_t rc = check_matrix(K, G, H, W);
    if (rc != ISG_OK) return rc;
    if (K + G == 0) return ISG_OK;
    if (!work || (K > 0 && (!det || !area_det)) || (G > 0 && (!gt || !area_gt)) ||
        (K > 0 && G > 0 && !inter))
        return isg_set_error(ISG_ERR_INVALID, "mask_iou_matrix: NULL pointer");
    if (((uintptr_t)work & 7u) || ((uintptr_t)inter & 3u) || ((uintptr_t)area_det & 3u) ||
        ((uintptr_t)area_gt & 3u))
        return isg_set_error(ISG_ERR_INVALID, "mask_iou_matrix: work needs 8-B alignment, the "
                             "outputs 4-B");
    const int64_t hw = (int64_t)H * W;
    const int64_t words = mask_bit_words(hw);
    if (K > 0) (void)hipMemsetAsync(area_det, 0, (size_t)K * sizeof(int32_t), st);
    if (G > 0) (void)hipMemsetAsync(area_gt, 0, (size_t)G * sizeof(int32_t), st);
    const int64_t gblocks = std::min<int64_t>((words / 4 + 3) / 4, 256);
    hipLaunchKernelGGL(eval_pack_kernel, dim3((unsigned)gblocks, (unsigned)(K + G)), dim3(kThreads), 0,
                       st, det, K, gt, hw, words, (unsigned long long*)work, area_det, area_gt);
    if (K > 0 && G > 0)
        hipLaunchKernelGGL(eval_inter_kernel, dim3((unsigned)K, (unsigned)G), dim3(kThreads), 0, st,
                           K, G, words, (const unsigned long long*)work, inter);
    return isg_check_launch("mask_iou_matrix kernels");
}

}  // extern "C"
