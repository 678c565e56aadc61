// The COCO `counts` string codec on the GPU, with boxes and areas (isg_rle_compress,
// isg_rle_parse, isg.h): what stands between isg_mask_rle / isg_mask_rle_decode and a
// results file. Their runs / offsets / runs_cap plug in unchanged in both directions.
//
// Contracts (instancesegmentation_amd/rle.py holds their CPU statements):
//   compress   slot j's counts c_0 .. c_{L-1} = runs[offsets[j] .. offsets[j+1]) become the
//              bytes of `compress`: v_i = c_i for i <= 2, c_i - c_{i-2} (signed, 64 bits)
//              from i = 3; n_i the fewest groups in 1..7 with -2^(5n-1) <= v < 2^(5n-1);
//              group k = ((v >> 5k) & 31) | (k < n-1 ? 32 : 0), plus 48. boxes[j], areas[j]
//              are `summarize`: with ends clipped at H*W the set runs are the odd ones, the
//              box is tight around them ([0,0,0,0] without one), a run across a column seam
//              makes y span 0..H-1.
//   parse      slot j's bytes chars[char_offsets[j] .. char_offsets[j+1]) become the counts
//              and status of `parse_total`: g = (byte - 48) & 63, a byte without 0x20 ends
//              a count, a count is worth its last min(k, 7) groups, the stride-2 delta is
//              undone in wrapping 64-bit arithmetic, the low 32 bits are stored.
// A slot whose input range is empty, reversed, starts below 0 or reaches past the input
// capacity is void (the decoder's rule): no characters, box [0,0,0,0], area 0; no counts,
// status 0. The output offsets always hold the true values and nothing is written at or past
// the output capacity (the encoder's rule).
//
// Shape. Both directions are two launches of one workgroup per slot, so slots may overlap or
// repeat and the geometry depends on n alone:
//   *_measure_kernel  walks the slot in chunks of kChunk with a carry and leaves the slot's
//                     output length in work (compress: the box and the area as well, from
//                     the 64-bit scan of the counts);
//   *_emit_kernel     sums the lengths of the slots before its own (the output offset), walks
//                     the slot again and writes every count's characters (every terminator's
//                     count) at its prefix-sum position.
// A real image is 16 slots of about 900 counts: one chunk per workgroup, two dependent
// launches. A slot of any length is walked serially by its workgroup (a noise mask of
// 10^6 counts: some 500 rounds); nothing is sized by a slot, and LDS holds one chunk.
// Bytes cross the LDS on their way in and out, placed so that their LDS and global addresses
// agree mod 4: the body of a chunk moves as dwords, its ragged ends as bytes, and neither a
// load nor a store touches a byte outside the slot's range or past a capacity.
// Nothing is allocated or synchronised, no atomics, and nothing reads what an earlier call
// left in an output or in work.
#include <algorithm>

#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWavesN = kThreads / 64;
constexpr int kU = 8;                  // consecutive counts (bytes) of one thread
constexpr int kChunk = kThreads * kU;  // counts (bytes) of one round of a workgroup
constexpr int kBack = 7;               // bytes before a chunk that parse looks at
constexpr int64_t kMaxCap = ((int64_t)1 << 31) - 1;

ISG_DEV bool slot_ok(int64_t a, int64_t b, int64_t cap) { return a >= 0 && a < b && b <= cap; }

// exclusive prefix of v over the workgroup's threads, `total` its sum; sh: [kWavesN]
template <class T>
ISG_DEV T block_excl(T v, T* sh, T& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T p = __shfl_up(inc, o, 64);
        if (lane >= o) inc += p;
    }
    __syncthreads();  // sh of an earlier scan is read
    if (lane == 63) sh[wave] = inc;
    __syncthreads();
    T ex = inc - v;
    total = 0;
#pragma unroll
    for (int k = 0; k < kWavesN; ++k) {
        if (k < wave) ex += sh[k];
        total += sh[k];
    }
    return ex;
}

struct OpMin { ISG_DEV uint32_t operator()(uint32_t a, uint32_t b) const { return min(a, b); } };
struct OpMax { ISG_DEV uint32_t operator()(uint32_t a, uint32_t b) const { return max(a, b); } };
struct OpOr { ISG_DEV uint32_t operator()(uint32_t a, uint32_t b) const { return a | b; } };
struct OpAdd { ISG_DEV uint32_t operator()(uint32_t a, uint32_t b) const { return a + b; } };

template <class Op>
ISG_DEV uint32_t block_red(uint32_t v, uint32_t* sh, Op op) {  // sh: [kWavesN]
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, (uint32_t)__shfl_xor(v, o, 64));
    __syncthreads();  // sh of an earlier reduction is read
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    v = sh[0];
#pragma unroll
    for (int k = 1; k < kWavesN; ++k) v = op(v, sh[k]);
    return v;
}

// sum over k < j of len[k]: the output offset of slot j; sh: [kWavesN]
ISG_DEV int64_t sum_before(const int64_t* __restrict__ len, int j, int64_t* sh) {
    int64_t s = 0;
    for (int k = threadIdx.x; k < j; k += kThreads) s += len[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    s = 0;
#pragma unroll
    for (int k = 0; k < kWavesN; ++k) s += sh[k];
    return s;
}

// ---- compress -------------------------------------------------------------------------

// groups of the signed value v: x = v for v >= 0 and -v - 1 below, so x < 2^(5n-1) is
// the range test and x needs 65 - clz(x) bits with its sign (x == 0: one group)
ISG_DEV int groups_of(int64_t v) {
    const uint64_t x = (uint64_t)(v ^ (v >> 63));
    const int bits = x ? 65 - __clzll((long long)x) : 1;
    return (bits + 4) / 5;  // <= 7: |v| < 2^32
}

// this thread's kU counts of the chunk at c0 and the two before them: v[u + 2] is the
// count at r0 + u, clamped into the slot (not predicated: all loads in flight)
ISG_DEV void load_counts(const uint32_t* __restrict__ c, int64_t r0, int64_t len,
                         uint32_t (&v)[kU + 2]) {
#pragma unroll
    for (int u = 0; u < kU + 2; ++u) v[u] = c[min(max(r0 + u - 2, (int64_t)0), len - 1)];
}

// the value count r is written as: itself up to r == 2, then its difference to count r - 2
ISG_DEV int64_t delta_of(const uint32_t (&v)[kU + 2], int u, int64_t r) {
    return r < 3 ? (int64_t)v[u + 2] : (int64_t)v[u + 2] - (int64_t)v[u];
}

__global__ __launch_bounds__(kThreads) void rs_measure_kernel(
    const uint32_t* __restrict__ runs, int64_t cap, const int64_t* __restrict__ offsets, int H,
    int W, int64_t* __restrict__ len_out, int32_t* __restrict__ boxes,
    int64_t* __restrict__ areas) {
    __shared__ uint64_t s_64[kWavesN];
    __shared__ uint32_t s_32[kWavesN];
    const int j = blockIdx.x, tid = threadIdx.x;
    const int64_t a = offsets[j], b = offsets[j + 1];
    const bool ok = slot_ok(a, b, cap);
    const int64_t len = ok ? b - a : 0;
    const uint32_t* c = runs + (ok ? a : 0);
    const uint32_t hw = (uint32_t)H * (uint32_t)W, h = (uint32_t)H;
    uint64_t carry = 0;  // the sum of the counts before the chunk
    uint64_t nchars = 0;  // this thread's characters
    uint32_t area = 0, smin = hw, emax = 0, ymin = h, ymax = 0, cross = 0;
    for (int64_t c0 = 0; c0 < len; c0 += kChunk) {  // uniform over the workgroup
        const int64_t r0 = c0 + (int64_t)tid * kU;
        uint32_t v[kU + 2];
        load_counts(c, r0, len, v);
        uint64_t inc[kU], ts = 0;
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const bool in = r0 + u < len;
            if (in) nchars += groups_of(delta_of(v, u, r0 + u));
            ts += in ? v[u + 2] : 0u;
            inc[u] = ts;
        }
        uint64_t tot;
        const uint64_t ex = carry + block_excl<uint64_t>(ts, s_64, tot);
#pragma unroll
        for (int u = 1; u < kU; u += 2) {  // r0 is even: the odd counts are the set runs
            if (r0 + u < len) {
                const uint64_t e1 = ex + inc[u], e0 = e1 - v[u + 2];
                const uint32_t s = (uint32_t)min(e0, (uint64_t)hw);
                const uint32_t e = (uint32_t)min(e1, (uint64_t)hw);
                if (e > s) {  // positions s .. e - 1
                    const uint32_t xs = s / h, xe = (e - 1) / h;
                    area += e - s;
                    smin = min(smin, s);
                    emax = max(emax, e);
                    cross |= xs != xe;
                    ymin = min(ymin, s - xs * h);
                    ymax = max(ymax, e - 1 - xe * h);
                }
            }
        }
        carry += tot;
    }
    uint64_t wide;  // the slot's characters: up to 7 * 2^31
    block_excl<uint64_t>(nchars, s_64, wide);
    area = block_red(area, s_32, OpAdd());
    smin = block_red(smin, s_32, OpMin());
    emax = block_red(emax, s_32, OpMax());
    ymin = block_red(ymin, s_32, OpMin());
    ymax = block_red(ymax, s_32, OpMax());
    cross = block_red(cross, s_32, OpOr());
    if (tid == 0) {
        len_out[j] = (int64_t)wide;
        areas[j] = area;
        int32_t* bx = boxes + (int64_t)j * 4;
        if (emax == 0) {
            bx[0] = bx[1] = bx[2] = bx[3] = 0;
        } else {
            const uint32_t x0 = smin / h, x1 = (emax - 1) / h;
            const uint32_t y0 = cross ? 0u : ymin, y1 = cross ? h - 1 : ymax;
            bx[0] = (int32_t)x0;
            bx[1] = (int32_t)y0;
            bx[2] = (int32_t)(x1 - x0 + 1);
            bx[3] = (int32_t)(y1 - y0 + 1);
        }
    }
}

// Copy `nbytes` staged bytes to dst[0 .. nbytes). The stage holds them from byte `shift` =
// dst & 3 on, so stage word w and the dword at dst - shift + 4w are the same four bytes:
// words that lie inside the range go as dwords, the ragged ends byte by byte.
ISG_DEV void store_staged(uint8_t* dst, const uint32_t* stage, uint32_t shift, uint32_t nbytes) {
    const uint8_t* stage8 = (const uint8_t*)stage;
    uint8_t* base = dst - shift;  // 4-byte aligned; nothing below dst is touched
    const uint32_t end = shift + nbytes, words = (end + 3) / 4;
    for (uint32_t w = threadIdx.x; w < words; w += kThreads) {
        const uint32_t q0 = 4 * w;
        if (q0 >= shift && q0 + 4 <= end) {
            *(uint32_t*)(base + q0) = stage[w];
        } else {
            for (uint32_t q = max(q0, shift); q < min(q0 + 4, end); ++q) base[q] = stage8[q];
        }
    }
}

// The mirror: stage[shift ..) = src[0 .. nbytes), shift = src & 3; no byte outside the range
// is read.
ISG_DEV void load_staged(const uint8_t* src, uint32_t* stage, uint32_t shift, uint32_t nbytes) {
    uint8_t* stage8 = (uint8_t*)stage;
    const uint8_t* base = src - shift;
    const uint32_t end = shift + nbytes, words = (end + 3) / 4;
    for (uint32_t w = threadIdx.x; w < words; w += kThreads) {
        const uint32_t q0 = 4 * w;
        if (q0 >= shift && q0 + 4 <= end) {
            stage[w] = *(const uint32_t*)(base + q0);
        } else {
            for (uint32_t q = max(q0, shift); q < min(q0 + 4, end); ++q) stage8[q] = base[q];
        }
    }
}

__global__ __launch_bounds__(kThreads) void rs_emit_kernel(
    const uint32_t* __restrict__ runs, int64_t cap, const int64_t* __restrict__ offsets, int n,
    const int64_t* __restrict__ len_in, uint8_t* __restrict__ chars, int64_t chars_cap,
    int64_t* __restrict__ char_offsets) {
    __shared__ int64_t s_b[kWavesN];
    __shared__ uint32_t s_32[kWavesN];
    __shared__ uint32_t s_stage[(4 + 7 * kChunk + 3) / 4];
    const int j = blockIdx.x, tid = threadIdx.x;
    const int64_t base = sum_before(len_in, j, s_b);
    if (tid == 0) {
        char_offsets[j] = base;
        if (j == n - 1) char_offsets[n] = base + len_in[j];
    }
    const int64_t a = offsets[j], b = offsets[j + 1];
    if (!slot_ok(a, b, cap)) return;  // uniform
    const int64_t len = b - a;
    const uint32_t* c = runs + a;
    uint8_t* stage8 = (uint8_t*)s_stage;
    int64_t pos = base;  // where the chunk's first character goes
    for (int64_t c0 = 0; c0 < len; c0 += kChunk) {
        const int64_t r0 = c0 + (int64_t)tid * kU;
        uint32_t v[kU + 2];
        load_counts(c, r0, len, v);
        int64_t d[kU];
        int ng[kU];
        uint32_t ls = 0;
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            d[u] = delta_of(v, u, r0 + u);
            ng[u] = r0 + u < len ? groups_of(d[u]) : 0;
            ls += ng[u];
        }
        uint32_t tot;
        uint32_t at = block_excl<uint32_t>(ls, s_32, tot);  // its barriers also end the
        const uint32_t shift = (uint32_t)(((uintptr_t)chars + (uint64_t)pos) & 3u);  // last copy
        at += shift;
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            for (int k = 0; k < ng[u]; ++k)
                stage8[at + k] = (uint8_t)((((uint32_t)(d[u] >> (5 * k)) & 31u) |
                                            (k < ng[u] - 1 ? 32u : 0u)) + 48u);
            at += ng[u];
        }
        __syncthreads();
        const int64_t room = chars_cap - pos;  // nothing at or past the capacity
        const uint32_t nbytes = (uint32_t)min((int64_t)tot, max(room, (int64_t)0));
        if (nbytes) store_staged(chars + pos, s_stage, shift, nbytes);
        pos += tot;
    }
}

// ---- parse ------------------------------------------------------------------------------

ISG_DEV bool is_term(uint32_t byte) { return (((byte - 48u) & 0x20u) == 0u); }

__global__ __launch_bounds__(kThreads) void rp_measure_kernel(
    const uint8_t* __restrict__ chars, int64_t cap, const int64_t* __restrict__ char_offsets,
    int64_t* __restrict__ cnt_out) {
    __shared__ uint32_t s_stage[(4 + kChunk + 3) / 4];
    __shared__ uint32_t s_32[kWavesN];
    const int j = blockIdx.x, tid = threadIdx.x;
    const int64_t a = char_offsets[j], b = char_offsets[j + 1];
    const bool ok = slot_ok(a, b, cap);
    const int64_t len = ok ? b - a : 0;
    const uint8_t* stage8 = (const uint8_t*)s_stage;
    int64_t cnt = 0;
    for (int64_t c0 = 0; c0 < len; c0 += kChunk) {
        const uint32_t nb = (uint32_t)min((int64_t)kChunk, len - c0);
        const uint8_t* src = chars + a + c0;
        const uint32_t shift = (uint32_t)((uintptr_t)src & 3u);
        __syncthreads();  // the stage of the round before is read
        load_staged(src, s_stage, shift, nb);
        __syncthreads();
        uint32_t t = 0;
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const uint32_t q = (uint32_t)tid * kU + u;
            if (q < nb) t += is_term(stage8[shift + q]);
        }
        cnt += block_red(t, s_32, OpAdd());
    }
    if (tid == 0) cnt_out[j] = cnt;
}

__global__ __launch_bounds__(kThreads) void rp_emit_kernel(
    const uint8_t* __restrict__ chars, int64_t cap, const int64_t* __restrict__ char_offsets,
    int n, const int64_t* __restrict__ cnt_in, uint32_t* __restrict__ runs, int64_t runs_cap,
    int64_t* __restrict__ offsets, int32_t* __restrict__ status) {
    __shared__ int64_t s_b[kWavesN];
    __shared__ uint32_t s_32[kWavesN];
    __shared__ uint64_t s_e[kWavesN], s_o[kWavesN];
    __shared__ uint32_t s_stage[(4 + kBack + kChunk + 3) / 4];
    const int j = blockIdx.x, tid = threadIdx.x;
    const int64_t base = sum_before(cnt_in, j, s_b);
    if (tid == 0) {
        offsets[j] = base;
        if (j == n - 1) offsets[n] = base + cnt_in[j];
    }
    const int64_t a = char_offsets[j], b = char_offsets[j + 1];
    if (!slot_ok(a, b, cap)) {  // uniform
        if (tid == 0) status[j] = 0;
        return;
    }
    const int64_t len = b - a;
    const uint8_t* stage8 = (const uint8_t*)s_stage;
    int64_t index = 0;         // counts before the chunk
    uint64_t ce = 0, co = 0;   // the even chain (from count 2) and the odd chain before it
    uint32_t flags = 0;
    for (int64_t c0 = 0; c0 < len; c0 += kChunk) {
        const int64_t lo = max(c0 - kBack, (int64_t)0), hi = min(c0 + kChunk, len);
        const uint8_t* src = chars + a + lo;
        const uint32_t shift = (uint32_t)((uintptr_t)src & 3u);
        __syncthreads();  // the stage of the round before is read
        load_staged(src, s_stage, shift, (uint32_t)(hi - lo));
        __syncthreads();
        // the groups since the last terminator, seen from kBack bytes before this thread's
        // own: acc their last min(k, 7) values, lowest first. A count that began before the
        // window reaches an own terminator with k >= 8, as it must
        const int64_t t0 = c0 + (int64_t)tid * kU;
        uint64_t acc = 0;
        int k = 0;
        int64_t val[kU];
        uint32_t has = 0;
#pragma unroll
        for (int q = 0; q < kBack + kU; ++q) {
            const int64_t p = t0 - kBack + q;
            if (p < 0 || p >= len) continue;
            const uint32_t byte = stage8[shift + (uint32_t)(p - lo)];
            const uint32_t g = (byte - 48u) & 0x3fu;
            if (k >= 7) acc = (acc >> 5) | ((uint64_t)(g & 31u) << 30);
            else acc |= (uint64_t)(g & 31u) << (5 * k);
            ++k;
            if (q >= kBack) {
                if (byte < 48u || byte > 111u) flags |= 2u;             // BAD_CHAR
                if (p == len - 1 && (g & 0x20u)) flags |= 1u;            // TRUNCATED
            }
            if (!(g & 0x20u)) {
                if (q >= kBack) {
                    const int nn = min(k, 7);
                    if (k > 7) flags |= 4u;                              // TOO_LONG
                    if (g & 0x10u) acc |= ~(uint64_t)0 << (5 * nn);      // sign-extend
                    val[q - kBack] = (int64_t)acc;
                    has |= 1u << (q - kBack);
                }
                acc = 0;
                k = 0;
            }
        }
        // this thread's terminators: their number, and their values summed per chain. The
        // parity of a count's index needs the exclusive number first, so the number is
        // scanned, then the two chain sums
        uint32_t tot;
        const uint32_t before = block_excl<uint32_t>((uint32_t)__popc(has), s_32, tot);
        const int64_t i0 = index + before;  // index of this thread's first count
        uint64_t se = 0, so = 0;
        {
            int64_t i = i0;
#pragma unroll
            for (int u = 0; u < kU; ++u) {
                if (has & (1u << u)) {
                    if (i & 1) so += (uint64_t)val[u];
                    else if (i) se += (uint64_t)val[u];
                    ++i;
                }
            }
        }
        uint64_t te, to;
        uint64_t pe = ce + block_excl<uint64_t>(se, s_e, te);
        uint64_t po = co + block_excl<uint64_t>(so, s_o, to);
        {
            int64_t i = i0;
#pragma unroll
            for (int u = 0; u < kU; ++u) {
                if (has & (1u << u)) {
                    int64_t cv;
                    if (i & 1) cv = (int64_t)(po += (uint64_t)val[u]);
                    else if (i) cv = (int64_t)(pe += (uint64_t)val[u]);
                    else cv = val[u];
                    if (cv < 0 || cv > (int64_t)0xffffffffLL) flags |= 8u;  // RANGE
                    if (base + i < runs_cap) runs[base + i] = (uint32_t)cv;
                    ++i;
                }
            }
        }
        index += tot;
        ce += te;
        co += to;
    }
    flags = block_red(flags, s_32, OpOr());
    if (tid == 0) status[j] = (int32_t)flags;
}

// size checks shared by an entry and its workspace function: host code, nothing dereferenced
int32_t check_sizes(const char* what, int32_t n, int64_t in_cap, int64_t out_cap) {
    if (n < 0 || in_cap < 0 || out_cap < 0)
        return isg_set_error(ISG_ERR_INVALID, "%s: bad sizes n=%d capacities %lld, %lld", what, n,
                             (long long)in_cap, (long long)out_cap);
    if (in_cap > kMaxCap || out_cap > kMaxCap)
        return isg_set_error(ISG_ERR_UNSUPPORTED, "%s: capacities %lld, %lld (max %lld)", what,
                             (long long)in_cap, (long long)out_cap, (long long)kMaxCap);
    return ISG_OK;
}

int32_t check_hw(const char* what, int32_t H, int32_t W) {
    if (H <= 0 || W <= 0)
        return isg_set_error(ISG_ERR_INVALID, "%s: bad sizes H=%d W=%d", what, H, W);
    if ((int64_t)H * W >= ((int64_t)1 << 31))
        return isg_set_error(ISG_ERR_INVALID, "%s: H*W = %lld needs < 2^31", what,
                             (long long)((int64_t)H * W));
    return ISG_OK;
}

int64_t work_bytes(int32_t n) { return std::max<int64_t>(n, 1) * (int64_t)sizeof(int64_t); }

}  // namespace

extern "C" {

int32_t isg_rle_string_chunk(void) { return kChunk; }

int64_t isg_rle_compress_workspace(int32_t n, int64_t runs_cap) {
    if (check_sizes("rle_compress", n, runs_cap, 0) != ISG_OK) return -1;
    return work_bytes(n);
}

int32_t isg_rle_compress(const uint32_t* runs, int64_t runs_cap, const int64_t* offsets, int32_t n,
                         int32_t H, int32_t W, uint8_t* chars, int64_t chars_cap,
                         int64_t* char_offsets, int32_t* boxes, int64_t* areas, void* work,
                         isg_stream_t st) {
    int32_t rc = check_sizes("rle_compress", n, runs_cap, chars_cap);
    if (rc == ISG_OK) rc = check_hw("rle_compress", H, W);
    if (rc != ISG_OK) return rc;
    if (n == 0) return ISG_OK;
    if (!offsets || !char_offsets || !boxes || !areas || !work || (runs_cap > 0 && !runs) ||
        (chars_cap > 0 && !chars))
        return isg_set_error(ISG_ERR_INVALID, "rle_compress: NULL runs, offsets, chars, "
                             "char_offsets, boxes, areas or work");
    if (((uintptr_t)offsets & 7u) || ((uintptr_t)char_offsets & 7u) || ((uintptr_t)areas & 7u) ||
        ((uintptr_t)work & 7u) || ((uintptr_t)runs & 3u) || ((uintptr_t)boxes & 3u))
        return isg_set_error(ISG_ERR_INVALID, "rle_compress: offsets, char_offsets, areas and "
                             "work need 8-B alignment, runs and boxes 4-B");
    int64_t* len = (int64_t*)work;
    hipLaunchKernelGGL(rs_measure_kernel, dim3((unsigned)n), dim3(kThreads), 0, st, runs, runs_cap,
                       offsets, H, W, len, boxes, areas);
    hipLaunchKernelGGL(rs_emit_kernel, dim3((unsigned)n), dim3(kThreads), 0, st, runs, runs_cap,
                       offsets, n, len, chars, chars_cap, char_offsets);
    return isg_check_launch("rle_compress kernels");
}

int64_t isg_rle_parse_workspace(int32_t n, int64_t chars_cap) {
    if (check_sizes("rle_parse", n, chars_cap, 0) != ISG_OK) return -1;
    return work_bytes(n);
}

int32_t isg_rle_parse(const uint8_t* chars, int64_t chars_cap, const int64_t* char_offsets,
                      int32_t n, uint32_t* runs, int64_t runs_cap, int64_t* offsets,
                      int32_t* status, void* work, isg_stream_t st) {
    const int32_t rc = check_sizes("rle_parse", n, chars_cap, runs_cap);
    if (rc != ISG_OK) return rc;
    if (n == 0) return ISG_OK;
    if (!char_offsets || !offsets || !status || !work || (chars_cap > 0 && !chars) ||
        (runs_cap > 0 && !runs))
        return isg_set_error(ISG_ERR_INVALID, "rle_parse: NULL chars, char_offsets, runs, "
                             "offsets, status or work");
    if (((uintptr_t)char_offsets & 7u) || ((uintptr_t)offsets & 7u) || ((uintptr_t)work & 7u) ||
        ((uintptr_t)runs & 3u) || ((uintptr_t)status & 3u))
        return isg_set_error(ISG_ERR_INVALID, "rle_parse: char_offsets, offsets and work need "
                             "8-B alignment, runs and status 4-B");
    int64_t* cnt = (int64_t*)work;
    hipLaunchKernelGGL(rp_measure_kernel, dim3((unsigned)n), dim3(kThreads), 0, st, chars,
                       chars_cap, char_offsets, cnt);
    hipLaunchKernelGGL(rp_emit_kernel, dim3((unsigned)n), dim3(kThreads), 0, st, chars, chars_cap,
                       char_offsets, n, cnt, runs, runs_cap, offsets, status);
    return isg_check_launch("rle_parse kernels");
}

}  // extern "C"
