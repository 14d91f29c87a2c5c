// svc_jump.h — the line walk behind the jump statistics of the focus stability (get_points_on_line and the mean of
// sc_check_for_extra_cuts, smartVidCrop.py:1337-1455), stated once.  No HIP dependency: svc_host_focus_stability (svc_host.cpp) and
// k_focus_jumps (svc_tail.hip) evaluate the same inline expressions, so host and device agree to the bit by construction.
//
// The walk: the integer-stepped samples strictly after p1 up to p2 along the dominant axis, kept where they fall inside the image.
// The reference builds them in a float32 buffer with a float32 slope; the conversions below are its own, in its order.
//   jump_setup(p1, p2, min_d)  -> false = "no statistic" (a move below min_d; a NumPy arange whose length neither matches the buffer
//                                 nor broadcasts -- NumPy raises there), else the line: sample count m = ceil(max(|dX|, |dY|)), mode,
//                                 slope, start and step of the leading axis, and whether the arange has one element (broadcast)
//   jump_sample(line, i)       -> (bx, by) of sample i as float32
//   jump_inside / jump_index   -> the buffer's filter and the map index floor(by) * w + floor(bx)
//
// Why every expression rounds the same in a host and in a device compilation (the library is built with -ffp-contract=off; the
// statements below hold even where a compiler contracts):
//   * float64 add, subtract, fabs, ceil, comparisons and the float64 <-> float32 / integer conversions are IEEE operations with one
//     result on either side (gfx950 keeps float32 and float64 denormals: HIP's default).
//   * The divisions of arange_len are by the step, +1 or -1: exact.
//   * The one float32 division, the slope, is a plain `/`: hipcc emits the correctly rounded sequence for it (its default; the
//     library passes no fast-math flag and uses no __fdividef), which is what the host's divss gives.
//   * No multiply feeds an add.  slope * (lead - fp1) is converted to an integer before p1 is added, and a product that passes
//     through an integer conversion cannot be fused with the addition behind it.
//   * i * step in lead0 + i * step is exact (step is +1 or -1 and i < 2^53), so the sum rounds once whether or not the pair is
//     fused into an fma.
//   * floorf and the (long) conversions are exact.
//
// Domain.  The arithmetic is defined -- every (long) conversion in range -- when the four coordinates are finite and lie within
// SVC_FOCUS_MAX_COORD = 65 536 of zero: then m <= 131 072, |slope| <= 1 and |slope * (lead - fp1)| < 2^18.  jump_in_domain tests
// that; the device entry refuses a move outside it (include/svc.h: svc_focus_jumps_u8) and reads nothing for it.  The host entry
// takes its centres from svc_host_fill_empty_centres, which leaves no NaN, and does not test.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
// (__forceinline__ spelled out: svc_host.cpp is compiled as HIP too, without the runtime header that defines the word)
#define SVC_JUMP_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define SVC_JUMP_FN static inline
#endif

#define SVC_JUMP_MAX_COORD 65536.0      // include/svc.h: SVC_FOCUS_MAX_COORD

struct JumpLine {
    long m;                 // samples on the line, >= 1
    int mode;               // 0: x fixed, 1: y fixed, 2: y leads, 3: x leads
    int bcast;              // the leading arange has ONE element, which NumPy broadcasts over the m rows
    float slope;            // modes 2, 3: d(other) / d(lead) in float32
    float fp1x, fp1y;       // p1 as the float32 buffer holds it
    double p1x, p1y;
    double lead0, step;     // leading axis: sample i = lead0 + i * step, step = +1 or -1
};

SVC_JUMP_FN bool jump_in_domain(double p1x, double p1y, double p2x, double p2y) {
    return fabs(p1x) <= SVC_JUMP_MAX_COORD && fabs(p1y) <= SVC_JUMP_MAX_COORD && fabs(p2x) <= SVC_JUMP_MAX_COORD &&
           fabs(p2y) <= SVC_JUMP_MAX_COORD;                   // (a NaN fails every comparison, an infinity the one it is in)
}

// numpy.arange(start, stop, step) for float arguments: ceil((stop - start) / step) elements, element i = start + i * step
SVC_JUMP_FN long jump_arange_len(double start, double stop, double step) {
    const double v = ceil((stop - start) / step);
    return v > 0 ? (long)v : 0;
}

SVC_JUMP_FN bool jump_setup(double p1x, double p1y, double p2x, double p2y, double min_d, JumpLine *L) {
    const double dX = p2x - p1x, dY = p2y - p1y, dXa = fabs(dX), dYa = fabs(dY);
    if (dXa < min_d && dYa < min_d) return false;
    const long m = (long)ceil(dYa > dXa ? dYa : dXa);
    if (m < 1) return false;
    const bool negY = p1y > p2y, negX = p1x > p2x;
    const double sy0 = negY ? p1y - 1 : p1y + 1, sys = negY ? -1.0 : 1.0;
    const double sx0 = negX ? p1x - 1 : p1x + 1, sxs = negX ? -1.0 : 1.0;
    const long ny = jump_arange_len(sy0, negY ? (p1y - dYa) - 1 : (p1y + dYa) + 1, sys);
    const long nx = jump_arange_len(sx0, negX ? (p1x - dXa) - 1 : (p1x + dXa) + 1, sxs);
    int mode;
    if (p1x == p2x) mode = 0;
    else if (p1y == p2y) mode = 1;
    else if (dYa > dXa) mode = 2;
    else mode = 3;
    const bool y_leads = mode == 0 || mode == 2;
    const long len = y_leads ? ny : nx;
    if (!(len == m || len == 1)) return false;               // an array assigned to a column of the buffer must have its length, or 1
    L->m = m;
    L->mode = mode;
    L->bcast = len == 1;
    L->slope = mode == 2 ? (float)dX / (float)dY : (mode == 3 ? (float)dY / (float)dX : 0.f);
    L->fp1x = (float)p1x;
    L->fp1y = (float)p1y;
    L->p1x = p1x;
    L->p1y = p1y;
    L->lead0 = y_leads ? sy0 : sx0;
    L->step = y_leads ? sys : sxs;
    return true;
}

SVC_JUMP_FN void jump_sample(const JumpLine &L, long i, float *bx, float *by) {
    const float lead = (float)(L.lead0 + (double)(L.bcast ? 0 : i) * L.step);
    if (L.mode == 0 || L.mode == 2) {
        *by = lead;
        *bx = L.mode == 0 ? L.fp1x : (float)((double)(long)(L.slope * (lead - L.fp1y)) + L.p1x);
    } else {
        *bx = lead;
        *by = L.mode == 1 ? L.fp1y : (float)((double)(long)(L.slope * (lead - L.fp1x)) + L.p1y);
    }
}

SVC_JUMP_FN bool jump_inside(float bx, float by, int w, int h) { return bx >= 0.f && by >= 0.f && bx < (float)w && by < (float)h; }

// index of an inside sample in a row-major h x w map: 0 <= floor(by) < h and 0 <= floor(bx) < w there, so it lies in [0, h w)
SVC_JUMP_FN long jump_index(float bx, float by, int w) { return (long)floorf(by) * w + (long)floorf(bx); }
