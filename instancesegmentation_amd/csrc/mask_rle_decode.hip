// COCO run-length decoding onto image canvases on the GPU (isg_mask_rle_decode, isg.h): the
// inverse of mask_rle.hip, shaped so that what the encoder writes (runs, offsets) plugs in.
//
// Contract (instancesegmentation_amd/rle.py `decode_canvas` is its CPU statement): slot j
// holds counts c_0 .. c_{L-1} = runs[offsets[j] .. offsets[j+1]); with ends e_i = c_0 + ... +
// c_i, column-major position p = x*H + y belongs to run i = #{e <= p} (zero-length runs are
// stepped over), and the pixel is 255 when i is odd and i < L, else 0. Positions at or past
// the sum are background, runs past H*W are ignored, totals[j] is the unclipped sum. A slot
// whose range is empty, reversed, starts below 0 or reaches past runs_cap is the all-zero
// canvas with total 0.
//
// Ends. The slots are arbitrary ranges of one runs buffer (they may even overlap), so the
// prefix sum is not segmented: P[i] = runs[0] + ... + runs[i-1] over the whole buffer in 64
// bits (P[0] = 0), and the ends of slot [a, b) are P[i+1] - P[a], its total P[b] - P[a].
// Only the prefix below the largest valid offsets[j+1] is scanned, so a buffer far larger
// than its content costs nothing. The scan crosses workgroups in two levels:
//   dec_sum_kernel   per chunk of kChunk runs: their sum;
//   dec_scan_kernel  per chunk: the sum of the chunks before it, then the scan inside it.
//
// Fill. The canvas is row-major, the scan order column-major, so the tile is the encoder's:
// lanes run along x (dword path: 32 lanes x 4 columns, one 128-byte line per row), a
// workgroup is kCL lanes times kNSeg row segments, and every lane walks down its own columns.
// A (column, segment) finds the run of its first pixel by one upper-bound search in the
// slot's ends and advances the run index as it walks; every row of the tile leaves as one
// contiguous line. Each canvas byte is written exactly once; the ends come from L2.
//
// The launch geometry depends on (n, H, W, runs_cap) only, nothing is allocated or
// synchronised, and nothing reads what an earlier call left in masks / totals / work.
#include <algorithm>

#include "common.h"

namespace {

constexpr int kCL = 32;                // lanes across x of one workgroup
constexpr int kNSeg = 32;              // row segments of one column
constexpr int kThreads = kCL * kNSeg;  // 1024
constexpr int kScanThreads = 256;
constexpr int kScanU = 8;              // consecutive runs of one thread
constexpr int kChunk = kScanThreads * kScanU;
constexpr int64_t kMaxRuns = ((int64_t)1 << 31) - 1;  // run indices relative to a slot fit 32 bits

int64_t dec_chunks(int64_t runs_cap) { return (runs_cap + kChunk - 1) / kChunk; }

struct DecWork {
    uint64_t* P;     // [runs_cap + 1] prefix sums of the runs buffer
    uint64_t* csum;  // [chunks] per-chunk sums
};

DecWork carve(void* work, int64_t runs_cap) {
    uint64_t* p = (uint64_t*)work;
    return DecWork{p, p + runs_cap + 1};
}

ISG_DEV bool slot_ok(int64_t a, int64_t b, int64_t cap) { return a >= 0 && a < b && b <= cap; }

ISG_DEV uint64_t block_sum(uint64_t v, uint64_t* sh) {  // kScanThreads threads, all of them
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();  // sh of an earlier reduction is read
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    v = 0;
    for (int i = 0; i < kScanThreads / 64; ++i) v += sh[i];
    return v;
}

// the largest offsets[j+1] of a valid slot (0: none): runs at and past it are nobody's
ISG_DEV int64_t used_end(const int64_t* __restrict__ offsets, int n, int64_t cap, int64_t* sh) {
    int64_t m = 0;
    for (int j = threadIdx.x; j < n; j += kScanThreads) {
        const int64_t a = offsets[j], b = offsets[j + 1];
        if (slot_ok(a, b, cap)) m = max(m, b);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (int64_t)__shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
    __syncthreads();
    m = 0;
    for (int i = 0; i < kScanThreads / 64; ++i) m = max(m, sh[i]);
    return m;
}

__global__ __launch_bounds__(kScanThreads) void dec_sum_kernel(const uint32_t* __restrict__ runs,
                                                                int64_t cap,
                                                                const int64_t* __restrict__ offsets,
                                                                int n, DecWork w) {
    __shared__ int64_t s_m[kScanThreads / 64];
    __shared__ uint64_t s_s[kScanThreads / 64];
    const int64_t limit = used_end(offsets, n, cap, s_m);
    const int64_t i0 = (int64_t)blockIdx.x * kChunk;
    if (i0 >= limit) return;  // uniform over the workgroup
    uint32_t v[kScanU];
#pragma unroll
    for (int u = 0; u < kScanU; ++u) {  // clamped, not predicated: all loads in flight
        const int64_t i = i0 + u * kScanThreads + threadIdx.x;
        v[u] = runs[min(i, limit - 1)];
    }
    uint64_t s = 0;
#pragma unroll
    for (int u = 0; u < kScanU; ++u)
        if (i0 + u * kScanThreads + threadIdx.x < limit) s += v[u];
    s = block_sum(s, s_s);
    if (threadIdx.x == 0) w.csum[blockIdx.x] = s;
}

__global__ __launch_bounds__(kScanThreads) void dec_scan_kernel(const uint32_t* __restrict__ runs,
                                                                 int64_t cap,
                                                                 const int64_t* __restrict__ offsets,
                                                                 int n, DecWork w) {
    constexpr int NW = kScanThreads / 64;
    __shared__ int64_t s_m[NW];
    __shared__ uint64_t s_s[NW], s_w[NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t limit = used_end(offsets, n, cap, s_m);
    const int64_t i0 = (int64_t)blockIdx.x * kChunk;
    if (i0 >= limit) return;
    uint64_t base = 0;  // the chunks before this one
    for (int64_t c = tid; c < (int64_t)blockIdx.x; c += kScanThreads) base += w.csum[c];
    base = block_sum(base, s_s);
    const int64_t t0 = i0 + (int64_t)tid * kScanU;  // this thread's kScanU consecutive runs
    uint32_t v[kScanU];
#pragma unroll
    for (int u = 0; u < kScanU; ++u) v[u] = runs[min(t0 + u, limit - 1)];
    uint64_t inc[kScanU], ts = 0;
#pragma unroll
    for (int u = 0; u < kScanU; ++u) {
        ts += t0 + u < limit ? v[u] : 0u;
        inc[u] = ts;
    }
    uint64_t is = ts;  // inclusive over the wave, then the waves before
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t p = __shfl_up(is, o, 64);
        if (lane >= o) is += p;
    }
    if (lane == 63) s_w[wave] = is;
    __syncthreads();
    uint64_t ex = base + is - ts;
    for (int k = 0; k < wave; ++k) ex += s_w[k];
#pragma unroll
    for (int u = 0; u < kScanU; ++u)
        if (t0 + u < limit) w.P[t0 + u + 1] = ex + inc[u];
    if (blockIdx.x == 0 && tid == 0) w.P[0] = 0;
}

// end of run i of a slot whose ends are e[0 .. len), clipped to hw; hw past the last run
ISG_DEV uint32_t end_of(const uint64_t* __restrict__ e, uint64_t pa, uint32_t i, uint32_t len,
                        uint32_t hw) {
    const uint64_t v = e[min(i, len - 1)] - pa;  // clamped: len >= 1 wherever this is called
    return i < len ? (uint32_t)min(v, (uint64_t)hw) : hw;
}

template <int C>
__global__ __launch_bounds__(kThreads) void dec_fill_kernel(const int64_t* __restrict__ offsets,
                                                            int64_t cap, int H, int W, int G,
                                                            DecWork w, uint8_t* __restrict__ masks,
                                                            int64_t* __restrict__ totals) {
    const int j = blockIdx.x / G, g = blockIdx.x - j * G;
    const int64_t a = offsets[j], b = offsets[j + 1];
    const bool ok = slot_ok(a, b, cap);
    const uint32_t hw = (uint32_t)H * (uint32_t)W;
    const uint32_t len = ok ? (uint32_t)(b - a) : 0u;
    const uint64_t pa = ok ? w.P[a] : 0u;
    const uint64_t* e = w.P + (ok ? a + 1 : 0);  // e[i] - pa: the end of run i
    if (g == 0 && threadIdx.x == 0) totals[j] = ok ? (int64_t)(w.P[b] - pa) : 0;
    const int cl = threadIdx.x & (kCL - 1), seg = threadIdx.x / kCL;
    const int rows = (H + kNSeg - 1) / kNSeg;
    const int x0 = (g * kCL + cl) * C;
    const int r0 = (int)min((int64_t)seg * rows, (int64_t)H);
    const int r1 = (int)min((int64_t)r0 + rows, (int64_t)H);
    if (x0 >= W || r0 >= r1) return;
    uint32_t pos[C], ri[C], ne[C];  // position, its run, that run's end
#pragma unroll
    for (int c = 0; c < C; ++c) {
        pos[c] = (uint32_t)(x0 + c) * (uint32_t)H + (uint32_t)r0;
        ri[c] = 0;
        ne[c] = hw;
    }
    if (ok) {
        // upper bound: the number of ends <= pos, the C searches of a thread side by side
        uint32_t lo[C], hi[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            lo[c] = 0;
            hi[c] = len;
        }
        for (uint32_t s = len; s > 0; s >>= 1) {  // an interval of s halves to floor(s / 2)
            uint64_t v[C];
            uint32_t mid[C];
#pragma unroll
            for (int c = 0; c < C; ++c) {
                mid[c] = min((lo[c] + hi[c]) >> 1, len - 1);
                v[c] = e[mid[c]];
            }
#pragma unroll
            for (int c = 0; c < C; ++c) {
                if (lo[c] < hi[c]) {
                    if (v[c] - pa <= (uint64_t)pos[c]) lo[c] = mid[c] + 1;
                    else hi[c] = mid[c];
                }
            }
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
            ri[c] = lo[c];
            ne[c] = end_of(e, pa, ri[c], len, hw);
        }
    }
    uint8_t* m = masks + (int64_t)j * H * W + x0;
    for (int r = r0; r < r1; ++r) {
        uint32_t word = 0;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            while (pos[c] >= ne[c]) {  // ne == hw > pos past the last run: it ends
                ++ri[c];
                ne[c] = end_of(e, pa, ri[c], len, hw);
            }
            if ((ri[c] & 1u) && ri[c] < len) word |= 0xffu << (8 * c);
            ++pos[c];
        }
        if (C == 4) *(uint32_t*)(m + (int64_t)r * W) = word;
        else m[(int64_t)r * W] = (uint8_t)word;
    }
}

// size checks of isg_mask_rle_decode and its workspace: host code, nothing is dereferenced
int32_t check_decode(int32_t n, int32_t H, int32_t W, int64_t runs_cap) {
    if (n < 0 || H <= 0 || W <= 0 || runs_cap < 0)
        return isg_set_error(ISG_ERR_INVALID, "mask_rle_decode: bad sizes n=%d H=%d W=%d "
                             "runs_cap=%lld", n, H, W, (long long)runs_cap);
    if ((int64_t)H * W >= ((int64_t)1 << 31))
        return isg_set_error(ISG_ERR_INVALID, "mask_rle_decode: H*W = %lld needs < 2^31",
                             (long long)((int64_t)H * W));
    if (runs_cap > kMaxRuns)
        return isg_set_error(ISG_ERR_UNSUPPORTED, "mask_rle_decode: runs_cap=%lld (max %lld)",
                             (long long)runs_cap, (long long)kMaxRuns);
    return ISG_OK;
}

}  // namespace

extern "C" {

int64_t isg_mask_rle_decode_workspace(int32_t n, int32_t H, int32_t W, int64_t runs_cap) {
    if (check_decode(n, H, W, runs_cap) != ISG_OK) return -1;
    return (runs_cap + 1 + dec_chunks(runs_cap)) * (int64_t)sizeof(uint64_t);
}

int32_t isg_mask_rle_decode(const uint32_t* runs, int64_t runs_cap, const int64_t* offsets,
                            int32_t n, int32_t H, int32_t W, uint8_t* masks, int64_t* totals,
                            void* work, isg_stream_t st) {
    const int32_t rc = check_decode(n, H, W, runs_cap);
    if (rc != ISG_OK) return rc;
    if (n == 0) return ISG_OK;
    if (!offsets || !masks || !totals || (runs_cap > 0 && (!runs || !work)))
        return isg_set_error(ISG_ERR_INVALID, "mask_rle_decode: NULL runs, offsets, masks, totals "
                             "or work");
    if (((uintptr_t)offsets & 7u) || ((uintptr_t)totals & 7u) || ((uintptr_t)work & 7u) ||
        ((uintptr_t)runs & 3u))
        return isg_set_error(ISG_ERR_INVALID, "mask_rle_decode: offsets, totals and work need 8-B "
                             "alignment, runs 4-B");
    // dword stores, 4 columns per lane, where every row of every canvas is 4-byte aligned
    const bool dword = W % 4 == 0 && ((uintptr_t)masks & 3) == 0;
    const int C = dword ? 4 : 1;
    const int G = (int)((W + (int64_t)kCL * C - 1) / ((int64_t)kCL * C));
    const int64_t blocks = (int64_t)n * G;
    if (blocks > 0x7fffffff)
        return isg_set_error(ISG_ERR_UNSUPPORTED, "mask_rle_decode: %lld workgroups",
                             (long long)blocks);
    const DecWork w = carve(work, runs_cap);
    const int64_t chunks = dec_chunks(runs_cap);
    if (chunks > 0) {
        hipLaunchKernelGGL(dec_sum_kernel, dim3((unsigned)chunks), dim3(kScanThreads), 0, st, runs,
                           runs_cap, offsets, n, w);
        hipLaunchKernelGGL(dec_scan_kernel, dim3((unsigned)chunks), dim3(kScanThreads), 0, st, runs,
                           runs_cap, offsets, n, w);
    }
    if (dword)
        hipLaunchKernelGGL(dec_fill_kernel<4>, dim3((unsigned)blocks), dim3(kThreads), 0, st, offsets,
                           runs_cap, H, W, G, w, masks, totals);
    else
        hipLaunchKernelGGL(dec_fill_kernel<1>, dim3((unsigned)blocks), dim3(kThreads), 0, st, offsets,
                           runs_cap, H, W, G, w, masks, totals);
    return isg_check_launch("mask_rle_decode kernels");
}

}  // extern "C"
