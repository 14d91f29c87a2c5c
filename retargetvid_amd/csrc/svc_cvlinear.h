// svc_cvlinear.h — OpenCV INTER_LINEAR on u8 (cv2.resize; 11-bit fixed-point weights), stated once for every kernel that
// resamples bytes: the frames (svc_frames.hip) and the maps of resize_factor != 1 (svc_tail.hip).
// tab layout (int32): xofs[ow] | xa[ow][2] | yofs[oh] | ya[oh][2] | xmax
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

// one axis of the table; scale = source samples per destination sample
static inline void cv_linear_axis(int src, int dst, double scale, bool horizontal, int *ofs, int *a, int *xmax_out) {
    int xmax = dst;
    for (int d = 0; d < dst; ++d) {
        float f = (float)((d + 0.5) * scale - 0.5);
        int s = (int)floorf(f);
        f -= (float)s;
        if (horizontal) {
            if (s < 0) { f = 0.f; s = 0; }
            if (s + 1 >= src) {
                xmax = std::min(xmax, d);
                if (s >= src - 1) { f = 0.f; s = src - 1; }
            }
        }
        ofs[d] = s;
        long w0 = lrintf((1.f - f) * 2048.f), w1 = lrintf(f * 2048.f);
        a[2 * d] = (int)std::min(std::max(w0, -32768L), 32767L);
        a[2 * d + 1] = (int)std::min(std::max(w1, -32768L), 32767L);
    }
    if (xmax_out) *xmax_out = xmax;
}

// the table of (h, w) -> (oh, ow) with the scales sy, sx (cv2.resize to a size: (double)h / oh, (double)w / ow)
static inline std::vector<int> cv_linear_tab(int h, int w, int oh, int ow, double sy, double sx) {
    std::vector<int> tab(3 * ow + 3 * oh + 1);
    int xmax = ow;
    cv_linear_axis(w, ow, sx, true, tab.data(), tab.data() + ow, &xmax);
    cv_linear_axis(h, oh, sy, false, tab.data() + 3 * ow, tab.data() + 3 * ow + oh, nullptr);
    tab[3 * ow + 3 * oh] = xmax;
    return tab;
}

// the table as a kernel reads it
struct CvLinear {
    const int *xofs, *xa, *yofs, *ya;
    int xmax;
    __device__ __forceinline__ CvLinear(const int *__restrict__ tab, int oh, int ow)
        : xofs(tab), xa(tab + ow), yofs(tab + 3 * ow), ya(tab + 3 * ow + oh), xmax(tab[3 * ow + 3 * oh]) {}
    // output row oy of a picture of h rows: its two source rows and their weights
    __device__ __forceinline__ void row(int oy, int h, int &y0, int &y1, int &b0, int &b1) const {
        const int sy = yofs[oy];
        y0 = min(max(sy, 0), h - 1);
        y1 = min(max(sy + 1, 0), h - 1);
        b0 = ya[2 * oy];
        b1 = ya[2 * oy + 1];
    }
    // output column ox of a picture of w columns: its two source columns (both inside the picture) and their weights;
    // !inner: only x0 counts
    __device__ __forceinline__ void col(int ox, int w, int &x0, int &x1, int &a0, int &a1, bool &inner) const {
        x0 = xofs[ox];
        x1 = min(x0 + 1, w - 1);
        a0 = xa[2 * ox];
        a1 = xa[2 * ox + 1];
        inner = ox < xmax;
    }
    // one channel of one output pixel from its four taps t<row><column>
    __device__ __forceinline__ static uint8_t blend(int t00, int t01, int t10, int t11, int a0, int a1, int b0, int b1, bool inner) {
        const int h0 = inner ? t00 * a0 + t01 * a1 : t00 * 2048;
        const int h1 = inner ? t10 * a0 + t11 * a1 : t10 * 2048;
        const int v = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2;
        return (uint8_t)min(max(v, 0), 255);
    }
};
