// The crop contract's resampling, stated once for crop_kernel (infer_ops.hip) and stage B of
// the training crop (train_crop.hip). The oracle is oracle/infer_oracle.py; the numpy form is
// data.py crop_resample (augment.py rot_resample on a rotated grid).
//
// A window [lo, hi) of a uint8 plane is resampled with half-pixel-centre bilinear weights, the
// taps clamped into the window; a tap outside `valid` (already clamped to the image) counts as
// the fill value 0; the blend is rounded half up to a byte. Every float op is one IEEE op in
// the oracle's order (contraction off). A tap is loaded only through an index that was made
// valid first (index 0 where the tap is not read), so no address outside the plane is ever
// formed into a load.
#pragma once
#include "common.h"

struct Tap {        // one output coordinate along one axis
    float a, b;     // weights of the far and the near tap (a = frac, b = 1 - a)
    int c0, c1;     // tap coordinates
    bool o0, o1;    // tap inside valid (and therefore inside the image)
};

// output coordinate i of a window [lo, hi) resampled at `scale` source pixels per output pixel
ISG_DEV Tap make_tap(int i, float scale, int lo, int hi, int vlo, int vhi) {
#pragma clang fp contract(off)
    Tap t;
    const float f = (((float)i + 0.5f) * scale - 0.5f) + (float)lo;
    const float fl = floorf(f);
    t.a = f - fl;
    t.b = 1.f - t.a;
    const int ii = (int)fl;
    t.c0 = min(max(ii, lo), hi - 1);
    t.c1 = min(max(ii + 1, lo), hi - 1);
    t.o0 = t.c0 >= vlo && t.c0 < vhi;
    t.o1 = t.c1 >= vlo && t.c1 < vhi;
    return t;
}

// a tap pair at the source coordinate f (the rotated grid): floor and floor + 1, not clamped
// into the window (it has no meaning there); a tap counts where it lies inside valid
ISG_DEV Tap free_tap(float f, int vlo, int vhi) {
#pragma clang fp contract(off)
    Tap t;
    const float fl = floorf(f);
    t.a = f - fl;
    t.b = 1.f - t.a;
    t.c0 = (int)fl;  // the caller keeps |f| < 2^31
    t.c1 = t.c0 + 1;
    t.o0 = t.c0 >= vlo && t.c0 < vhi;
    t.o1 = t.c1 >= vlo && t.c1 < vhi;
    return t;
}

ISG_DEV int round_u8(float val) {
#pragma clang fp contract(off)
    const int q = (int)(val + 0.5f);
    return q < 0 ? 0 : (q > 255 ? 255 : q);
}

ISG_DEV int quantise(float by, float top, float ay, float bot) {
#pragma clang fp contract(off)
    const float val = (by * top) + (ay * bot);
    return round_u8(val);
}

// The four taps of one output pixel in an image W pixels a row: which are read, and the pixel
// index of each (0, always inside the plane, where the tap is not read). I is the type of the
// index arithmetic: int where the caller has checked the plane's size against 2^31, int64_t
// where it has not. Made once per output pixel and used for every plane of it.
template <typename I>
struct Taps {
    Tap x, y;
    bool k00, k01, k10, k11;
    I i00, i01, i10, i11;
    ISG_DEV Taps(const Tap& tx, const Tap& ty, I W)
        : x(tx), y(ty),
          k00(ty.o0 && tx.o0), k01(ty.o0 && tx.o1), k10(ty.o1 && tx.o0), k11(ty.o1 && tx.o1),
          i00(k00 ? ty.c0 * W + tx.c0 : 0), i01(k01 ? ty.c0 * W + tx.c1 : 0),
          i10(k10 ? ty.c1 * W + tx.c0 : 0), i11(k11 ? ty.c1 * W + tx.c1 : 0) {}
};

// the quantised byte of that output pixel in the plane p, `stride` bytes a pixel
template <typename I>
ISG_DEV int crop_sample(const Taps<I>& t, const uint8_t* __restrict__ p, int stride) {
#pragma clang fp contract(off)
    const uint8_t q00 = p[t.i00 * stride], q01 = p[t.i01 * stride];
    const uint8_t q10 = p[t.i10 * stride], q11 = p[t.i11 * stride];
    const float s00 = t.k00 ? (float)q00 : 0.f, s01 = t.k01 ? (float)q01 : 0.f;
    const float s10 = t.k10 ? (float)q10 : 0.f, s11 = t.k11 ? (float)q11 : 0.f;
    const float top = (t.x.b * s00) + (t.x.a * s01);
    const float bot = (t.x.b * s10) + (t.x.a * s11);
    return quantise(t.y.b, top, t.y.a, bot);
}

// ToTensor + Normalize(0.5, 0.5) of a quantised byte (train_instance.py:80-85)
ISG_DEV float normalise_u8(int q) {
#pragma clang fp contract(off)
    return ((float)q / 255.f - 0.5f) / 0.5f;
}
