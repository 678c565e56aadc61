// COCO run-length encoding of the kept instance masks on the GPU (isg_mask_rle, isg.h).
//
// Contract (instancesegmentation_amd/rle.py `encode` is its CPU statement): a pixel is set
// when mask >= 128; the H x W mask is flattened column-major (pixel (x, y) at position
// p = x*H + y); with a virtual zero before position 0, t_0 < t_1 < ... are the positions
// whose bit differs from the predecessor's, and counts = diff([0, t..., H*W]). A mask with
// T transitions has T + 1 counts.
//
// The canvas is row-major, the scan order column-major. Lanes run along x, so one row of a
// workgroup's tile is one contiguous 128-byte line (dword path: 32 lanes x 4 columns) and
// every lane walks down its own columns. A workgroup is kCL lanes across x times kNSeg row
// segments (H cut into kNSeg pieces of ceil(H/kNSeg) rows); the predecessor of a segment's
// first pixel is the pixel above it, for row 0 the last row of the column to the left, for
// position 0 the virtual zero.
//
// Chunk order. A chunk is one (slot, column, segment); in scan order chunks sort by slot,
// then column, then segment. A workgroup owns all kNSeg segments of kCL*C adjacent columns,
// which is one contiguous range of that order, so the prefix sum has three levels:
//   rle_count_kernel  per workgroup: the number of transitions in its tile and the position
//                     of the last one (a sum and a max: no order needed);
//   rle_scan_kernel   per slot: exclusive scan of those pairs over the slot's workgroups,
//                     the slot's offset (sum over earlier slots), its final count;
//   rle_emit_kernel   per workgroup: the walk again, an ordered scan of the per-chunk
//                     (count, last position) pairs through LDS, then every transition
//                     writes runs[offset + index] = position - previous transition.
// Output order is by position (compaction by prefix sum, no atomics), the launch geometry
// depends on (K, H, W, max_sel) only, and nothing reads what an earlier call left in
// work / runs / offsets.
#include <algorithm>

#include "common.h"

namespace {

constexpr int kCL = 32;                  // lanes across x of one workgroup
constexpr int kNSeg = 32;                // row segments of one column
constexpr int kThreads = kCL * kNSeg;    // 1024
constexpr int kWaves = kThreads / 64;
constexpr int kU = 8;                    // rows whose loads are in flight together
constexpr int kScanThreads = 256;

// per (slot, workgroup) pairs; each array holds K * ceil(W / kCL) entries
struct RleWork {
    uint32_t* tot_cnt;    // transitions in the workgroup's tile
    uint32_t* tot_last;   // position of the last of them (0: none)
    uint32_t* base_cnt;   // transitions of the slot before the tile
    uint32_t* prev_last;  // position of the last transition before the tile (0: none)
};

int64_t rle_groups_max(int64_t W) { return (W + kCL - 1) / kCL; }

RleWork carve(void* work, int64_t K, int64_t W) {
    const int64_t n = K * rle_groups_max(W);
    uint32_t* p = (uint32_t*)work;
    return RleWork{p, p + n, p + 2 * n, p + 3 * n};
}

ISG_DEV int rle_nsel(const int32_t* nsel, int max_sel) {
    const int n = nsel ? *nsel : max_sel;
    return min(max(n, 0), max_sel);
}

template <int C>
ISG_DEV uint32_t load_px(const uint8_t* p);
typedef const uint32_t __attribute__((address_space(1)))* gcu32_p;
typedef const uint8_t __attribute__((address_space(1)))* gcu8_p;
template <>
ISG_DEV uint32_t load_px<4>(const uint8_t* p) { return *(gcu32_p)p; }
template <>
ISG_DEV uint32_t load_px<1>(const uint8_t* p) { return *(gcu8_p)p; }

// Walk rows [r0, r1) of columns x0 .. x0+C-1 of mask m. Every transition bumps cnt[c] and
// sets last[c] to its position; with EMIT it first writes its count (position - last[c]) at
// out[cnt[c]] when that index is below cap. The count pass starts cnt and last at 0, the emit pass at
// the chunk's exclusive prefix and the last transition before the chunk.
template <int C, bool EMIT>
ISG_DEV void walk(const uint8_t* __restrict__ m, int H, int W, int x0, int r0, int r1,
                  uint32_t (&cnt)[C], uint32_t (&last)[C], uint32_t* __restrict__ out, int64_t cap) {
    uint32_t prev[C];
    if (r0 > 0) {
        const uint32_t v = load_px<C>(m + (int64_t)(r0 - 1) * W + x0);
#pragma unroll
        for (int c = 0; c < C; ++c) prev[c] = (v >> (8 * c + 7)) & 1u;
    } else {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int x = x0 + c;  // row 0: the last row of the column to the left
            prev[c] = x > 0 ? load_px<1>(m + (int64_t)(H - 1) * W + x - 1) >> 7 : 0u;
        }
    }
    for (int r = r0; r < r1; r += kU) {
        uint32_t v[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u)  // clamped, not predicated: no branch around a load
            v[u] = load_px<C>(m + (int64_t)min(r + u, r1 - 1) * W + x0);
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            if (r + u < r1) {
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const uint32_t bit = (v[u] >> (8 * c + 7)) & 1u;
                    if (bit != prev[c]) {
                        const uint32_t pos = (uint32_t)(x0 + c) * (uint32_t)H + (uint32_t)(r + u);
                        if (EMIT) {
                            if ((int64_t)cnt[c] < cap) out[cnt[c]] = pos - last[c];
                        }
                        ++cnt[c];
                        last[c] = pos;
                    }
                    prev[c] = bit;
                }
            }
        }
    }
}

// tile of the calling thread: first column and row range (empty: x0 >= W or r0 >= r1)
template <int C>
ISG_DEV void my_tile(int g, int H, int& x0, int& r0, int& r1) {
    const int cl = threadIdx.x & (kCL - 1), seg = threadIdx.x / kCL;
    const int rows = (H + kNSeg - 1) / kNSeg;
    x0 = (g * kCL + cl) * C;
    r0 = min((int64_t)seg * rows, (int64_t)H);
    r1 = min((int64_t)r0 + rows, (int64_t)H);
}

template <int C>
__global__ __launch_bounds__(kThreads) void rle_count_kernel(
    const uint8_t* __restrict__ masks, int K, int H, int W, const int32_t* __restrict__ sel,
    const int32_t* __restrict__ nsel, int max_sel, int G, RleWork w) {
    __shared__ uint32_t s_c[kWaves], s_l[kWaves];
    const int j = blockIdx.x / G, g = blockIdx.x - j * G;
    if (j >= rle_nsel(nsel, max_sel)) return;  // surplus workgroup
    const int src = sel ? sel[j] : j;
    uint32_t cs = 0, lm = 0;
    if (src >= 0 && src < K) {  // out of range: the all-zero mask, nothing read
        int x0, r0, r1;
        my_tile<C>(g, H, x0, r0, r1);
        if (x0 < W && r0 < r1) {
            uint32_t cnt[C], last[C];
#pragma unroll
            for (int c = 0; c < C; ++c) cnt[c] = last[c] = 0;
            walk<C, false>(masks + (int64_t)src * H * W, H, W, x0, r0, r1, cnt, last, nullptr, 0);
#pragma unroll
            for (int c = 0; c < C; ++c) {
                cs += cnt[c];
                lm = max(lm, last[c]);
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        cs += __shfl_xor(cs, o, 64);
        lm = max(lm, (uint32_t)__shfl_xor(lm, o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        s_c[threadIdx.x >> 6] = cs;
        s_l[threadIdx.x >> 6] = lm;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        cs = 0;
        lm = 0;
        for (int i = 0; i < kWaves; ++i) {
            cs += s_c[i];
            lm = max(lm, s_l[i]);
        }
        w.tot_cnt[blockIdx.x] = cs;
        w.tot_last[blockIdx.x] = lm;
    }
}

// inclusive scan of (sum, max) over the 64 lanes of a wave
ISG_DEV void wave_scan(uint32_t& c, uint32_t& l) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t pc = __shfl_up(c, o, 64), pl = __shfl_up(l, o, 64);
        if (lane >= o) {
            c += pc;
            l = max(l, pl);
        }
    }
}

// One workgroup per slot j in [0, max_sel]: offsets[j] (the sum over earlier slots of
// transitions + 1; slots at and past the last one get the total); for a live slot the
// exclusive scan of its workgroups' pairs and its final count.
__global__ __launch_bounds__(kScanThreads) void rle_scan_kernel(
    int64_t hw, const int32_t* __restrict__ nsel, int max_sel, int G, RleWork w,
    uint32_t* __restrict__ runs, int64_t cap, int64_t* __restrict__ offsets) {
    constexpr int NW = kScanThreads / 64;
    __shared__ int64_t s_sum[NW];
    __shared__ uint32_t s_c[NW], s_l[NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = blockIdx.x;
    const int ns = rle_nsel(nsel, max_sel);
    const int jj = min(j, ns);
    int64_t s = 0;
    for (int64_t i = tid; i < (int64_t)jj * G; i += kScanThreads) s += w.tot_cnt[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) s_sum[wave] = s;
    __syncthreads();
    int64_t off = jj;  // one more count than transitions per earlier slot
    for (int i = 0; i < NW; ++i) off += s_sum[i];
    if (tid == 0) offsets[j] = off;
    if (j >= ns) return;
    uint32_t carry_c = 0, carry_l = 0;
    for (int base = 0; base < G; base += kScanThreads) {
        const int i = base + tid;
        const uint32_t c = i < G ? w.tot_cnt[(int64_t)j * G + i] : 0u;
        const uint32_t l = i < G ? w.tot_last[(int64_t)j * G + i] : 0u;
        uint32_t ic = c, il = l;
        wave_scan(ic, il);
        uint32_t el = __shfl_up(il, 1, 64);
        if (lane == 0) el = 0;
        __syncthreads();  // s_c / s_l of the previous round are read
        if (lane == 63) {
            s_c[wave] = ic;
            s_l[wave] = il;
        }
        __syncthreads();
        uint32_t wc = carry_c, wl = carry_l;
        for (int k = 0; k < wave; ++k) {
            wc += s_c[k];
            wl = max(wl, s_l[k]);
        }
        if (i < G) {
            w.base_cnt[(int64_t)j * G + i] = wc + (ic - c);
            w.prev_last[(int64_t)j * G + i] = max(wl, el);
        }
        for (int k = 0; k < NW; ++k) {
            carry_c += s_c[k];
            carry_l = max(carry_l, s_l[k]);
        }
    }
    if (tid == 0) {
        const int64_t idx = off + carry_c;
        if (idx < cap) runs[idx] = (uint32_t)hw - carry_l;
    }
}

// LDS image of the per-chunk pairs in scan order, one pad word per 32 (the writers of one
// segment are 32 lanes whose entries lie kNSeg apart)
ISG_DEV int pad(int e) { return e + (e >> 5); }

template <int C>
__global__ __launch_bounds__(kThreads) void rle_emit_kernel(
    const uint8_t* __restrict__ masks, int K, int H, int W, const int32_t* __restrict__ sel,
    const int32_t* __restrict__ nsel, int max_sel, int G, RleWork w, uint32_t* __restrict__ runs,
    int64_t cap, const int64_t* __restrict__ offsets) {
    constexpr int E = kThreads * C;
    __shared__ uint32_t s_c[E + E / 32], s_l[E + E / 32];
    __shared__ uint32_t s_wc[kWaves], s_wl[kWaves];
    const int j = blockIdx.x / G, g = blockIdx.x - j * G;
    if (j >= rle_nsel(nsel, max_sel)) return;
    const int src = sel ? sel[j] : j;
    if (src < 0 || src >= K) return;  // its single count is the scan kernel's
    const uint8_t* m = masks + (int64_t)src * H * W;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cl = tid & (kCL - 1), seg = tid / kCL;
    int x0, r0, r1;
    my_tile<C>(g, H, x0, r0, r1);
    const bool live = x0 < W && r0 < r1;
    uint32_t cnt[C], last[C];
#pragma unroll
    for (int c = 0; c < C; ++c) cnt[c] = last[c] = 0;
    if (live) walk<C, false>(m, H, W, x0, r0, r1, cnt, last, nullptr, 0);
    // scan order inside the tile: column, then segment
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int e = pad((cl * C + c) * kNSeg + seg);
        s_c[e] = cnt[c];
        s_l[e] = last[c];
    }
    __syncthreads();
    uint32_t a[C], b[C], ts = 0, tm = 0;
#pragma unroll
    for (int i = 0; i < C; ++i) {  // this thread's C consecutive entries: local exclusive
        const int e = pad(tid * C + i);
        a[i] = ts;
        b[i] = tm;
        ts += s_c[e];
        tm = max(tm, s_l[e]);
    }
    uint32_t ic = ts, il = tm;
    wave_scan(ic, il);
    uint32_t el = __shfl_up(il, 1, 64);
    if (lane == 0) el = 0;
    if (lane == 63) {
        s_wc[wave] = ic;
        s_wl[wave] = il;
    }
    __syncthreads();
    uint32_t bc = ic - ts, bl = el;
    for (int k = 0; k < wave; ++k) {
        bc += s_wc[k];
        bl = max(bl, s_wl[k]);
    }
#pragma unroll
    for (int i = 0; i < C; ++i) {
        const int e = pad(tid * C + i);
        s_c[e] = bc + a[i];
        s_l[e] = max(bl, b[i]);
    }
    __syncthreads();
    if (!live) return;
    const uint32_t gc = w.base_cnt[blockIdx.x], gl = w.prev_last[blockIdx.x];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int e = pad((cl * C + c) * kNSeg + seg);
        cnt[c] = gc + s_c[e];
        last[c] = max(gl, s_l[e]);
    }
    const int64_t off = offsets[j];
    // runs + off may lie past the buffer; walk() dereferences it only below the capacity left
    walk<C, true>(m, H, W, x0, r0, r1, cnt, last, runs + off, cap - off);
}

}  // namespace

extern "C" {

int64_t isg_mask_rle_workspace(int32_t K, int32_t H, int32_t W) {
    if (K <= 0 || H <= 0 || W <= 0) return 0;
    return 4 * (int64_t)K * rle_groups_max(W) * (int64_t)sizeof(uint32_t);
}

int32_t isg_mask_rle(const uint8_t* masks, int32_t K, int32_t H, int32_t W, const int32_t* sel,
                     const int32_t* nsel, int32_t max_sel, uint32_t* runs, int64_t runs_cap,
                     int64_t* offsets, void* work, isg_stream_t st) {
    if (K <= 0 || H <= 0 || W <= 0)
        return isg_set_error(ISG_ERR_INVALID, "mask_rle: bad sizes K=%d H=%d W=%d", K, H, W);
    const int64_t hw = (int64_t)H * W;
    if (hw >= ((int64_t)1 << 31))
        return isg_set_error(ISG_ERR_INVALID, "mask_rle: H*W = %lld needs < 2^31", (long long)hw);
    if (max_sel < 0 || (!sel && max_sel > K))
        return isg_set_error(ISG_ERR_INVALID, "mask_rle: max_sel=%d (K=%d, sel %s)", max_sel, K,
                             sel ? "given" : "NULL");
    if (runs_cap < 0 || (!runs && runs_cap > 0))
        return isg_set_error(ISG_ERR_INVALID, "mask_rle: runs_cap=%lld with runs %s",
                             (long long)runs_cap, runs ? "given" : "NULL");
    if (!masks || !offsets || !work)
        return isg_set_error(ISG_ERR_INVALID, "mask_rle: NULL masks, offsets or work");
    if (max_sel > K)  // the workspace is sized by K
        return isg_set_error(ISG_ERR_UNSUPPORTED, "mask_rle: max_sel=%d > K=%d", max_sel, K);
    // dword loads, 4 columns per lane, where every row of every mask is 4-byte aligned
    const bool dword = W % 4 == 0 && ((uintptr_t)masks & 3) == 0;
    const int C = dword ? 4 : 1;
    const int G = (int)((W + (int64_t)kCL * C - 1) / ((int64_t)kCL * C));
    const int64_t blocks = (int64_t)max_sel * G;
    if (blocks > 0x7fffffff)
        return isg_set_error(ISG_ERR_UNSUPPORTED, "mask_rle: %lld workgroups", (long long)blocks);
    const RleWork w = carve(work, K, W);
    if (blocks > 0) {
        if (dword)
            hipLaunchKernelGGL(rle_count_kernel<4>, dim3((unsigned)blocks), dim3(kThreads), 0, st,
                               masks, K, H, W, sel, nsel, max_sel, G, w);
        else
            hipLaunchKernelGGL(rle_count_kernel<1>, dim3((unsigned)blocks), dim3(kThreads), 0, st,
                               masks, K, H, W, sel, nsel, max_sel, G, w);
    }
    hipLaunchKernelGGL(rle_scan_kernel, dim3((unsigned)max_sel + 1), dim3(kScanThreads), 0, st, hw,
                       nsel, max_sel, G, w, runs, runs_cap, offsets);
    if (blocks > 0) {
        if (dword)
            hipLaunchKernelGGL(rle_emit_kernel<4>, dim3((unsigned)blocks), dim3(kThreads), 0, st,
                               masks, K, H, W, sel, nsel, max_sel, G, w, runs, runs_cap, offsets);
        else
            hipLaunchKernelGGL(rle_emit_kernel<1>, dim3((unsigned)blocks), dim3(kThreads), 0, st,
                               masks, K, H, W, sel, nsel, max_sel, G, w, runs, runs_cap, offsets);
    }
    return isg_check_launch("mask_rle kernels");
}

}  // extern "C"
