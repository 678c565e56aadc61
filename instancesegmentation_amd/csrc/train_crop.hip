// Training batches prepared on the GPU (isg_train_crop, isg.h): what the loader's
// InstanceCommonDataset.__getitem__ (data.py) does per sample after decoding, for B samples
// that each come from an image of their own size, packed with their masks into one uint8
// arena.
//
//   train_box_kernel   stage A. Per sample the box of the non-zero mask pixels, twice in one
//                      pass: over the whole mask and over the mask inside `valid` (the
//                      centring translation's frame). The mask is read as dwords at
//                      addresses aligned here (its offset in the arena is arbitrary), the
//                      first and last partial dword as bytes, four loads in flight per
//                      thread. Each bound is kept in a form that only grows (W - min x,
//                      H - min y, max x + 1, max y + 1; 0 = nothing seen), so every
//                      reduction is a max: in the lane, across the wave by shuffles, across
//                      the workgroup through LDS. Every workgroup then stores its eight
//                      numbers in its own slot of the workspace and stage B takes the max
//                      over a sample's slots: no atomics (a first version sent one integer
//                      atomic max per wave and bound to a sample's single 32-byte record
//                      and spent 82 us there for eight 640 x 480 masks) and nothing to clear,
//                      since every slot that is read was written by the same call.
//   train_crop_body    stage B, one body for both entries. Derives the window from those
//                      numbers (data.py instance_box: the clipped box, else the whole-mask
//                      box, else the image; then +/- 16) and resamples it to S x S with
//                      crop_core.h's arithmetic (shared with crop_kernel, infer_ops.hip), the
//                      coordinates and weights computed once per output pixel for the three
//                      image planes and the mask plane. V consecutive u per lane, one 16-byte
//                      store per plane when V == 4. Workgroup 0 of a sample also writes its
//                      window and projects its 17 keypoints through it in double.
//                      With AUG one isg_train_aug record per sample applies (augment.py
//                      augment_sample is its CPU statement): the window's sides are jittered;
//                      the output grid is mirrored and/or rotated about the crop's centre;
//                      contrast, noise and a multiplier act on the quantised image planes.
//                      blockIdx.y is the sample, so every choice (separable or rotated taps,
//                      which colour steps, noise at all) is uniform in the workgroup. The
//                      noise is one Philox4x32-10 call per output pixel, its counter the
//                      pixel and the sample's ordinal. Without AUG every one of those
//                      operands and branches is compiled out (`if constexpr`), not switched
//                      at run time: the plain kernel takes no record and pays for none.
//   train_crop_kernel<V>      isg_train_crop's stage B: the body without AUG.
//   train_crop_aug_kernel<V>  isg_train_crop_aug's stage B: the body with AUG.
//
// Sample descriptors are host memory and reach the kernels by value, kChunk to a launch.
#include "common.h"
#include "crop_core.h"

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = ISG_LIST_CHUNK / 2;  // 16 samples x 40 B of kernel arguments
constexpr int kWaves = kThreads / 64;
constexpr int kBoxBlocksMax = 64;           // workgroups (and workspace slots) per sample of stage A
constexpr int kBoxU = 4;                    // dword loads of a thread in flight together
constexpr int kBoxGroups = 2 * kBoxU;       // dwords per thread that size stage A's grid

struct TrainChunk {
    isg_train_sample s[kChunk];
};

struct AugChunk {
    isg_train_aug a[kChunk];
};

typedef const uint32_t __attribute__((address_space(1)))* gcu32_p;

// ---- stage A -----------------------------------------------------------------------
// dword g of the mask's aligned image: pixels p0 .. p0+3, p0 = 4*g - head; bytes outside the
// mask (and every g >= ngroups) read as 0 and are never loaded
ISG_DEV uint32_t box_load(const uint8_t* m, int hw, int head, int g, int ngroups) {
    if (g >= ngroups) return 0u;
    const int p0 = 4 * g - head;
    if (p0 >= 0 && p0 + 4 <= hw) return *(gcu32_p)(m + p0);  // 4-byte aligned, inside the mask
    uint32_t v = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b)
        if (p0 + b >= 0 && p0 + b < hw) v |= (uint32_t)m[p0 + b] << (8 * b);
    return v;
}

__global__ __launch_bounds__(kThreads) void train_box_kernel(const uint8_t* __restrict__ arena,
                                                              TrainChunk ch, int base,
                                                              int32_t* __restrict__ work) {
    __shared__ int s_a[kWaves][8];
    const int k = blockIdx.y;
    const int H = ch.s[k].H, W = ch.s[k].W;
    const int vx0 = max(ch.s[k].valid[0], 0), vy0 = max(ch.s[k].valid[1], 0);
    const int vx1 = min(ch.s[k].valid[2], W), vy1 = min(ch.s[k].valid[3], H);
    const uint8_t* m = arena + ch.s[k].mask_off;
    const int hw = H * W;                          // 3*H*W < 2^31 (checked by the caller)
    const int head = (int)((uintptr_t)m & 3);      // bytes of the first dword before the mask
    const int ngroups = (hw + head + 3) >> 2;
    const int stride = gridDim.x * kThreads;
    int a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int g0 = blockIdx.x * kThreads + threadIdx.x; g0 < ngroups; g0 += kBoxU * stride) {
        uint32_t v[kBoxU];
#pragma unroll
        for (int u = 0; u < kBoxU; ++u) v[u] = box_load(m, hw, head, g0 + u * stride, ngroups);
#pragma unroll
        for (int u = 0; u < kBoxU; ++u) {
            if (v[u] == 0) continue;
            const int p0 = 4 * (g0 + u * stride) - head;  // pixel of the dword's byte 0
            const int pb = max(p0, 0);
            int y = pb / W, x = pb - y * W;        // the first byte that belongs to the mask
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                if (p0 + b < pb) continue;
                if ((v[u] >> (8 * b)) & 0xffu) {   // non-zero is the rule (data.py mask_box)
                    a[0] = max(a[0], W - x); a[1] = max(a[1], H - y);
                    a[2] = max(a[2], x + 1); a[3] = max(a[3], y + 1);
                    if (x >= vx0 && x < vx1 && y >= vy0 && y < vy1) {
                        a[4] = max(a[4], W - x); a[5] = max(a[5], H - y);
                        a[6] = max(a[6], x + 1); a[7] = max(a[7], y + 1);
                    }
                }
                if (++x == W) { x = 0; ++y; }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a[i] = max(a[i], __shfl_xor(a[i], o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) s_a[threadIdx.x >> 6][i] = a[i];
    }
    __syncthreads();
    if (threadIdx.x < 8) {  // this workgroup's slot, written whether or not it saw a pixel
        int r = 0;
#pragma unroll
        for (int wv = 0; wv < kWaves; ++wv) r = max(r, s_a[wv][threadIdx.x]);
        work[((int64_t)(base + k) * kBoxBlocksMax + blockIdx.x) * 8 + threadIdx.x] = r;
    }
}

// ---- stage B -----------------------------------------------------------------------
// the pre-pad box of sample b: the max over the nbox slots stage A wrote for it (nbox <= 64:
// two a thread), then data.py instance_box's three-way choice
ISG_DEV void sample_box(const int32_t* __restrict__ work, int b, int nbox, int H, int W,
                        int (*s_w)[8], int& x0, int& y0, int& x1, int& y1) {
    {
        const int i = threadIdx.x & 7, j = threadIdx.x >> 3;
        const int32_t* slot = work + (int64_t)b * kBoxBlocksMax * 8 + i;
        int r = max(j < nbox ? slot[j * 8] : 0, j + 32 < nbox ? slot[(j + 32) * 8] : 0);
#pragma unroll
        for (int o = 32; o >= 8; o >>= 1) r = max(r, __shfl_xor(r, o, 64));
        if ((threadIdx.x & 63) < 8) s_w[threadIdx.x >> 6][i] = r;
    }
    __syncthreads();
    int w[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        w[i] = 0;
#pragma unroll
        for (int wv = 0; wv < kWaves; ++wv) w[i] = max(w[i], s_w[wv][i]);
    }
    x0 = 0; y0 = 0; x1 = W; y1 = H;  // no mask pixel at all (train_instance.py:163-164)
    if (w[6] > 0) {
        x0 = W - w[4]; y0 = H - w[5]; x1 = w[6]; y1 = w[7];
    } else if (w[2] > 0) {  // every mask pixel was pushed out of the frame
        x0 = W - w[0]; y0 = H - w[1]; x1 = w[2]; y1 = w[3];
    }
}

// Philox4x32-10 (Salmon et al., SC'11), the Random123 constants
ISG_DEV void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                           uint32_t k1, uint32_t out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1;
        c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

ISG_DEV int byte_sum(uint32_t w) {
    return (int)((w & 255u) + ((w >> 8) & 255u) + ((w >> 16) & 255u) + (w >> 24));
}

// row of ORDER_PART_NAMES (data.py) that holds the other side's part; the nose is its own
__constant__ const int kMirrorPart[ISG_TRAIN_PARTS] = {3, 4, 5, 0, 1, 2, 9, 10, 11, 6, 7, 8,
                                                       13, 12, 14, 16, 15};

// sample b of the call: its descriptor sm and, with AUG, its record au (without AUG au, seed
// and ordinal0 are never read)
template <int V, bool AUG>
ISG_DEV void train_crop_body(const uint8_t* __restrict__ arena, const isg_train_sample& sm,
                             const isg_train_aug* au, int b, const int32_t* __restrict__ work,
                             int nbox, const double* __restrict__ kp, int S, uint64_t seed,
                             uint64_t ordinal0, float* __restrict__ xo, float* __restrict__ mo,
                             double* __restrict__ kpo, int32_t* __restrict__ wino) {
#pragma clang fp contract(off)
    __shared__ int s_w[kWaves][8];
    const int H = sm.H, W = sm.W;
    int x0, y0, x1, y1;
    sample_box(work, b, nbox, H, W, s_w, x0, y0, x1, y1);
    bool flip = false, rot = false;  // constants without AUG: what they guard is compiled out
    if constexpr (AUG) {
        // each side moves by floor(j * a / 1024), |j| <= 1024, a = a fifth of the box: never empty
        const int64_t ax = (x1 - x0) / 5, ay = (y1 - y0) / 5;
        x0 += (int)((au->jitter[0] * ax) >> 10);
        y0 += (int)((au->jitter[1] * ay) >> 10);
        x1 += (int)((au->jitter[2] * ax) >> 10);
        y1 += (int)((au->jitter[3] * ay) >> 10);
        flip = au->flip != 0;
        rot = !(au->rot_cos == 1.0 && au->rot_sin == 0.0);
    }
    x0 -= ISG_TRAIN_PAD; y0 -= ISG_TRAIN_PAD; x1 += ISG_TRAIN_PAD; y1 += ISG_TRAIN_PAD;
    if (blockIdx.x == 0) {
        if (threadIdx.x < 4)
            wino[4 * b + threadIdx.x] = threadIdx.x == 0 ? x0 : threadIdx.x == 1 ? y0
                                        : threadIdx.x == 2 ? x1 : y1;
        if (threadIdx.x < ISG_TRAIN_PARTS) {  // numpy's float64 arithmetic, one op at a time
            int part = (int)threadIdx.x;
            if constexpr (AUG) part = flip ? kMirrorPart[threadIdx.x] : part;
            const int64_t i = ((int64_t)b * ISG_TRAIN_PARTS + part) * 3;
            const int64_t j = ((int64_t)b * ISG_TRAIN_PARTS + threadIdx.x) * 3;
            double kx = ((kp[i] - (double)x0) * (double)S) / (double)(x1 - x0);
            double ky = ((kp[i + 1] - (double)y0) * (double)S) / (double)(y1 - y0);
            if constexpr (AUG) {
                if (rot) {  // the inverse of the pixels' map: a keypoint stays on the pixel it marked
                    const double h = (double)S * 0.5, dx = kx - h, dy = ky - h;
                    kx = ((au->rot_cos * dx) + (au->rot_sin * dy)) + h;
                    ky = ((au->rot_cos * dy) - (au->rot_sin * dx)) + h;
                }
                if (flip) kx = (double)S - kx;
            }
            kpo[j] = kx;
            kpo[j + 1] = ky;
            kpo[j + 2] = kp[i + 2] > 0.0 ? 1.0 : 0.0;
        }
    }
    const int64_t ss = (int64_t)S * S;
    const int64_t o = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * V;
    if (o >= ss) return;
    const int v = (int)(o / S), u0 = (int)(o - (int64_t)v * S);  // V == 4: S % 4 == 0, one row
    const int vx0 = max(sm.valid[0], 0), vy0 = max(sm.valid[1], 0);
    const int vx1 = min(sm.valid[2], W), vy1 = min(sm.valid[3], H);
    const uint8_t* img = arena + sm.img_off;
    const uint8_t* msk = arena + sm.mask_off;
    const float sx = (float)(x1 - x0) / (float)S;
    const float sy = (float)(y1 - y0) / (float)S;
    Tap ty = make_tap(v, sy, y0, y1, vy0, vy1);  // the separable path's row
    float r[4][V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        int uu = u0 + j;
        Tap tx;
        uint32_t noise[4] = {0u, 0u, 0u, 0u};
        if constexpr (AUG) {
            if (flip) uu = S - 1 - uu;
            if (rot) {  // uniform in the workgroup
                // |f| < 2^31: the window is within 1.2 W + 32 of the image (W < 2^31 / 3)
                const float rc = (float)au->rot_cos, rs = (float)au->rot_sin, half = (float)S * 0.5f;
                const float du = ((float)uu + 0.5f) - half, dv = ((float)v + 0.5f) - half;
                const float px = ((rc * du) - (rs * dv)) + half;
                const float py = ((rs * du) + (rc * dv)) + half;
                tx = free_tap(((px * sx) - 0.5f) + (float)x0, vx0, vx1);
                ty = free_tap(((py * sy) - 0.5f) + (float)y0, vy0, vy1);
            }
            if (au->noise != 0.f) {
                const uint64_t pix = (uint64_t)(o + j), ordinal = ordinal0 + (uint64_t)b;
                philox4x32_10((uint32_t)pix, (uint32_t)(pix >> 32), (uint32_t)ordinal,
                              (uint32_t)(ordinal >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), noise);
            }
        }
        if (!rot) tx = make_tap(uu, sx, x0, x1, vx0, vx1);
        const Taps<int> taps(tx, ty, W);  // 3*H*W < 2^31 (checked by the caller)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            int q = c < 3 ? crop_sample(taps, img + c, 3) : crop_sample(taps, msk, 1);
            if constexpr (AUG) {
                if (c < 3) {  // each step is the identity on an integer q when its parameter is neutral
                    if (au->contrast != 1.f) q = round_u8(((float)(q - 127) * au->contrast) + 127.f);
                    if (au->noise != 0.f) {
                        const int s = byte_sum(noise[au->noise_per_channel != 0 ? c : 0]);
                        q = round_u8((float)q + ((float)(s - 510) * au->noise));
                    }
                    if (au->mult[c] != 1.f) q = round_u8((float)q * au->mult[c]);
                }
            }
            r[c][j] = c < 3 ? normalise_u8(q) : (float)q / 255.f;
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float* dst = c < 3 ? xo + ((int64_t)b * 3 + c) * ss : mo + (int64_t)b * ss;
        if (V == 4) {
            gst4(dst, o, f32x4{r[c][0], r[c][1], r[c][2], r[c][3]});
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) gst(dst, o + j, r[c][j]);
        }
    }
}

template <int V>
__global__ __launch_bounds__(kThreads) void train_crop_kernel(
    const uint8_t* __restrict__ arena, TrainChunk ch, int base, const int32_t* __restrict__ work,
    int nbox, const double* __restrict__ kp, int S, float* __restrict__ xo, float* __restrict__ mo,
    double* __restrict__ kpo, int32_t* __restrict__ wino) {
    const int k = blockIdx.y;
    train_crop_body<V, false>(arena, ch.s[k], nullptr, base + k, work, nbox, kp, S, 0, 0, xo, mo, kpo,
                              wino);
}

template <int V>
__global__ __launch_bounds__(kThreads) void train_crop_aug_kernel(
    const uint8_t* __restrict__ arena, TrainChunk ch, AugChunk ag, int base,
    const int32_t* __restrict__ work, int nbox, const double* __restrict__ kp, int S, uint64_t seed,
    uint64_t ordinal0, float* __restrict__ xo, float* __restrict__ mo, double* __restrict__ kpo,
    int32_t* __restrict__ wino) {
    const int k = blockIdx.y;
    train_crop_body<V, true>(arena, ch.s[k], &ag.a[k], base + k, work, nbox, kp, S, seed, ordinal0, xo,
                             mo, kpo, wino);
}

// ---- host ----------------------------------------------------------------------------
// the checks of both entries, before any HIP call; max_hw: the largest mask of the first n
int32_t check_train_args(const char* who, const void* arena, int64_t arena_bytes,
                         const isg_train_sample* samples, const void* keypoints, int32_t n,
                         int32_t B, int32_t S, const void* work, const void* x, const void* mask,
                         const void* kp_out, const void* windows, int64_t* max_hw) {
    if (!arena || !samples || !keypoints || !work || !x || !mask || !kp_out || !windows)
        return isg_set_error(ISG_ERR_INVALID, "%s: NULL pointer", who);
    if (S <= 0 || n < 0 || n > B)
        return isg_set_error(ISG_ERR_INVALID, "%s: bad sizes S=%d n=%d B=%d", who, S, n, B);
    *max_hw = 0;
    for (int i = 0; i < n; ++i) {
        const isg_train_sample& s = samples[i];
        if (s.H <= 0 || s.W <= 0)
            return isg_set_error(ISG_ERR_INVALID, "%s: sample %d is %d x %d", who, i, s.H, s.W);
        const int64_t hw = (int64_t)s.H * s.W;
        if (3 * hw >= ((int64_t)1 << 31))
            return isg_set_error(ISG_ERR_INVALID, "%s: sample %d: 3*H*W = %lld needs < 2^31", who,
                                 i, (long long)(3 * hw));
        if (s.img_off < 0 || s.mask_off < 0 || s.img_off > arena_bytes - 3 * hw ||
            s.mask_off > arena_bytes - hw)
            return isg_set_error(ISG_ERR_INVALID,
                                 "%s: sample %d (image at %lld, mask at %lld, %d x %d) "
                                 "reaches outside the arena of %lld bytes", who, i,
                                 (long long)s.img_off, (long long)s.mask_off, s.H, s.W,
                                 (long long)arena_bytes);
        *max_hw = hw > *max_hw ? hw : *max_hw;
    }
    return ISG_OK;
}

bool aug_value_ok(float v) { return v >= 0.f && v <= ISG_TRAIN_AUG_MAX; }  // false for a NaN

// Both entries after their checks: kChunk samples to a launch of stage A and of stage B, the
// 16-byte-store stage B where S % 4 == 0 and x and mask are 16-byte aligned. aug NULL: the
// plain kernels (seed and ordinal0 are then unused).
int32_t launch_train_crop(const uint8_t* arena, const isg_train_sample* samples,
                          const isg_train_aug* aug, uint64_t seed, uint64_t ordinal0,
                          const double* keypoints, int32_t n, int32_t S, int64_t max_hw, void* work,
                          float* x, float* mask, double* kp_out, int32_t* windows, isg_stream_t st) {
    if (n == 0) return ISG_OK;
    const bool wide = S % 4 == 0 && (((uintptr_t)x | (uintptr_t)mask) & 15) == 0;
    const int64_t per_crop = (int64_t)kThreads * (wide ? 4 : 1);  // outputs per workgroup of stage B
    const int64_t crop_blocks = ((int64_t)S * S + per_crop - 1) / per_crop;
    if (crop_blocks > 0x7fffffff)
        return isg_set_error(ISG_ERR_UNSUPPORTED, "%s: %lld workgroups",
                             aug ? "train_crop_aug" : "train_crop", (long long)crop_blocks);
    const int64_t per_box = (int64_t)kThreads * kBoxGroups * 4;  // mask bytes per workgroup of stage A
    const int64_t bb = (max_hw + per_box - 1) / per_box;
    const int box_blocks = bb < 1 ? 1 : (bb > kBoxBlocksMax ? kBoxBlocksMax : (int)bb);
    const auto plain_kernel = wide ? train_crop_kernel<4> : train_crop_kernel<1>;
    const auto aug_kernel = wide ? train_crop_aug_kernel<4> : train_crop_aug_kernel<1>;
    for (int base = 0; base < n; base += kChunk) {
        const int cnt = n - base < kChunk ? n - base : kChunk;
        TrainChunk ch;
        AugChunk ag;
        for (int i = 0; i < kChunk; ++i) {
            ch.s[i] = samples[base + (i < cnt ? i : 0)];
            if (aug) ag.a[i] = aug[base + (i < cnt ? i : 0)];
        }
        hipLaunchKernelGGL(train_box_kernel, dim3((unsigned)box_blocks, (unsigned)cnt),
                           dim3(kThreads), 0, st, arena, ch, base, (int32_t*)work);
        const dim3 grid((unsigned)crop_blocks, (unsigned)cnt);
        if (aug)
            hipLaunchKernelGGL(aug_kernel, grid, dim3(kThreads), 0, st, arena, ch, ag, base,
                               (const int32_t*)work, box_blocks, keypoints, S, seed, ordinal0, x, mask,
                               kp_out, windows);
        else
            hipLaunchKernelGGL(plain_kernel, grid, dim3(kThreads), 0, st, arena, ch, base,
                               (const int32_t*)work, box_blocks, keypoints, S, x, mask, kp_out, windows);
    }
    return isg_check_launch(aug ? "train_crop_aug kernels" : "train_crop kernels");
}

}  // namespace

extern "C" {

int64_t isg_train_crop_workspace(int32_t B) {
    return B > 0 ? (int64_t)B * kBoxBlocksMax * 8 * (int64_t)sizeof(int32_t) : 0;
}

int32_t isg_train_crop(const uint8_t* arena, int64_t arena_bytes, const isg_train_sample* samples,
                       const double* keypoints, int32_t n, int32_t B, int32_t S, void* work,
                       float* x, float* mask, double* kp_out, int32_t* windows, isg_stream_t st) {
    int64_t max_hw = 0;
    const int32_t rc = check_train_args("train_crop", arena, arena_bytes, samples, keypoints, n, B,
                                        S, work, x, mask, kp_out, windows, &max_hw);
    if (rc != ISG_OK) return rc;
    return launch_train_crop(arena, samples, nullptr, 0, 0, keypoints, n, S, max_hw, work, x, mask,
                             kp_out, windows, st);
}

int32_t isg_train_crop_aug(const uint8_t* arena, int64_t arena_bytes, const isg_train_sample* samples,
                           const isg_train_aug* aug, uint64_t seed, uint64_t ordinal0,
                           const double* keypoints, int32_t n, int32_t B, int32_t S, void* work,
                           float* x, float* mask, double* kp_out, int32_t* windows, isg_stream_t st) {
    int64_t max_hw = 0;
    const int32_t rc = check_train_args("train_crop_aug", arena, arena_bytes, samples, keypoints, n,
                                        B, S, work, x, mask, kp_out, windows, &max_hw);
    if (rc != ISG_OK) return rc;
    if (!aug) return isg_set_error(ISG_ERR_INVALID, "train_crop_aug: NULL pointer");
    for (int i = 0; i < n; ++i) {
        const isg_train_aug& a = aug[i];
        for (int s = 0; s < 4; ++s)
            if (a.jitter[s] < -1024 || a.jitter[s] > 1024)
                return isg_set_error(ISG_ERR_INVALID, "train_crop_aug: record %d: jitter[%d] = %d "
                                     "outside +/-1024", i, s, a.jitter[s]);
        const double norm = a.rot_cos * a.rot_cos + a.rot_sin * a.rot_sin - 1.0;
        if (!(norm >= -1e-6 && norm <= 1e-6))  // also a NaN
            return isg_set_error(ISG_ERR_INVALID, "train_crop_aug: record %d: (cos, sin) = (%g, %g) "
                                 "is not a rotation", i, a.rot_cos, a.rot_sin);
        if ((a.flip != 0 && a.flip != 1) || (a.noise_per_channel != 0 && a.noise_per_channel != 1))
            return isg_set_error(ISG_ERR_INVALID, "train_crop_aug: record %d: flip = %d, "
                                 "noise_per_channel = %d (0 or 1)", i, a.flip, a.noise_per_channel);
        if (!aug_value_ok(a.contrast) || !aug_value_ok(a.noise) || !aug_value_ok(a.mult[0]) ||
            !aug_value_ok(a.mult[1]) || !aug_value_ok(a.mult[2]))
            return isg_set_error(ISG_ERR_INVALID, "train_crop_aug: record %d: contrast %g, noise %g, "
                                 "mult (%g, %g, %g) need to be finite, >= 0 and <= %g", i, a.contrast,
                                 a.noise, a.mult[0], a.mult[1], a.mult[2], (double)ISG_TRAIN_AUG_MAX);
    }
    return launch_train_crop(arena, samples, aug, seed, ordinal0, keypoints, n, S, max_hw, work, x,
                             mask, kp_out, windows, st);
}

}  // extern "C"
