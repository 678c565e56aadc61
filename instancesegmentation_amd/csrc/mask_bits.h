// Bit-packing of uint8 masks (foreground: byte >= 128) shared by the mask-NMS
// (maskops.hip) and the scoring IoU matrix (mask_eval.hip).
//
// Layout: a wave owns 256-pixel groups of one mask, lane l the 4 pixels 256g + 4l .. + 3;
// word 4g + j holds byte j of every lane of group g (one ballot). The bit order is internal
// to a workspace: every mask packed here uses the same one, so AND-popcount intersections
// do not depend on it.
#pragma once
#include "common.h"

// packed 64-bit words per mask: 4 per 256-pixel group
static inline int64_t mask_bit_words(int64_t hw) { return (hw + 255) / 256 * 4; }

// The 4 bytes src[base .. base + 3] of one lane, 0 past hw; `dword`: src + base is 4-B
// aligned, so a group that lies inside the mask is one 4-B load.
ISG_DEV uint32_t mask_load_px4(const uint8_t* __restrict__ src, int64_t base, int64_t hw,
                               bool dword) {
    uint32_t v4 = 0;
    if (dword && base + 3 < hw) {
        v4 = *reinterpret_cast<const uint32_t*>(src + base);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (base + j < hw) v4 |= (uint32_t)src[base + j] << (8 * j);
    }
    return v4;
}

// Ballot the 4 bytes of every lane into words4[0..3] (the group's words, written by lane 0);
// cnt / sum accumulate this lane's foreground pixels and their byte values (exact integers).
ISG_DEV void mask_ballot_px4(uint32_t v4, int lane, unsigned long long* __restrict__ words4,
                             unsigned long long& cnt, unsigned long long& sum) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned v = (v4 >> (8 * j)) & 0xffu;
        const bool on = v >= 128u;
        const unsigned long long b = __ballot(on);
        if (lane == 0) words4[j] = b;
        if (on) {
            cnt += 1;
            sum += v;
        }
    }
}
