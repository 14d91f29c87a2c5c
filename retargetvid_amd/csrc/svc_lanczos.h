// svc_lanczos.h -- Pillow's LANCZOS coefficient tables (host code, no HIP): shared by the network's input resampling
// (svc_net.hip: k_lanczos_norm, k_front) and the renderer's Lanczos path (svc_frames.hip: k_render_lanczos), and compiled on
// its own by tests/native/lanczos_tab_harness.cpp.
#pragma once
#include <math.h>

#include <algorithm>
#include <vector>

#define LZ_PREC 22      // fractional bits of a coefficient (Pillow: PRECISION_BITS = 32 - 8 - 2)

static double lz_sinc(double x) {
    if (x == 0.0) return 1.0;
    x *= M_PI;
    return sin(x) / x;
}
static double lz_filter(double x) { return (-3.0 <= x && x < 3.0) ? lz_sinc(x) * lz_sinc(x / 3.0) : 0.0; }

// Pillow's precompute_coeffs + normalize_coeffs_8bpc.  Identity table when sizes match
// (Pillow skips that pass).
static void lanczos_tab(int in_size, int out_size, std::vector<int> &bounds, std::vector<int> &coef, int &ksize) {
    bounds.assign(2 * out_size, 0);
    if (in_size == out_size) {
        ksize = 1;
        coef.assign(out_size, 1 << LZ_PREC);
        for (int i = 0; i < out_size; ++i) { bounds[2 * i] = i; bounds[2 * i + 1] = 1; }
        return;
    }
    double scale = (double)in_size / out_size, filterscale = std::max(scale, 1.0);
    double support = 3.0 * filterscale, ss = 1.0 / filterscale;
    ksize = (int)ceil(support) * 2 + 1;
    coef.assign((size_t)out_size * ksize, 0);
    std::vector<double> k(ksize);
    for (int xx = 0; xx < out_size; ++xx) {
        double center = (xx + 0.5) * scale, ww = 0.0;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        for (int x = 0; x < xmax; ++x) {
            k[x] = lz_filter((x + xmin - center + 0.5) * ss);
            ww += k[x];
        }
        for (int x = 0; x < xmax; ++x) {
            double v = (ww != 0.0) ? k[x] / ww : k[x];
            coef[(size_t)xx * ksize + x] = v < 0 ? (int)(-0.5 + v * (1 << LZ_PREC)) : (int)(0.5 + v * (1 << LZ_PREC));
        }
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
}
