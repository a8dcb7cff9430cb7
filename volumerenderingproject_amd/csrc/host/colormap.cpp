// colormap.cpp -- the colour map of VR_MODE_CDVR on the host (colormap.h) and vr_colormap_eval.
// Compiled without FP contraction (Makefile FPFLAGS): the device march (vr_cmap.hip) evaluates the
// same expressions from the same x / inv / rgba tables, so the two agree bit for bit.
#include "colormap.h"

#include <cmath>

#pragma clang fp contract(off)

namespace vr {

bool colormap_build(const vr_cmap_point* points, int32_t n, Colormap* out) {
    if (n < 1 || n > VR_CMAP_MAX_POINTS) return false;
    out->n = n;
    out->x.assign((size_t)n, 0.0f);
    out->inv.assign((size_t)n, 0.0f);
    out->rgba.assign((size_t)n * 4, 0.0f);
    for (int i = 0; i < n; ++i) {
        const vr_cmap_point& p = points[i];
        if (!std::isfinite(p.x)) return false;
        for (int k = 0; k < 4; ++k)
            if (!std::isfinite(p.rgba[k])) return false;
        if (!(p.rgba[3] >= 0.0f && p.rgba[3] <= 1.0f)) return false;
        if (i > 0 && !(points[i - 1].x < p.x)) return false;
        out->x[(size_t)i] = p.x;
        for (int k = 0; k < 4; ++k) out->rgba[(size_t)i * 4 + k] = p.rgba[k];
    }
    for (int i = 0; i + 1 < n; ++i) {
        const float w = out->x[(size_t)i + 1] - out->x[(size_t)i];
        const float inv = 1.0f / w;
        if (!std::isfinite(inv)) return false;   // (a span so narrow that 1 / w overflows)
        out->inv[(size_t)i] = inv;
    }
    return true;
}

void colormap_eval(const Colormap& m, float v, float out[4]) {
    int j = 0;   // the number of points x_i <= v (a NaN: none)
    for (int i = 0; i < m.n; ++i) j += (m.x[(size_t)i] <= v) ? 1 : 0;
    if (j == 0 || j == m.n) {
        const float* c = &m.rgba[(size_t)(j == 0 ? 0 : m.n - 1) * 4];
        for (int k = 0; k < 4; ++k) out[k] = c[k];
        return;
    }
    const float* a = &m.rgba[(size_t)(j - 1) * 4];
    const float* b = &m.rgba[(size_t)j * 4];
    const float u = std::fmin((v - m.x[(size_t)j - 1]) * m.inv[(size_t)j - 1], 1.0f);
    const float u1 = 1.0f - u;
    for (int k = 0; k < 4; ++k) out[k] = a[k] * u1 + b[k] * u;
}

}  // namespace vr

extern "C" int vr_colormap_eval(const vr_cmap_point* points, int32_t n, const float* v, int64_t count,
                                float* rgba_out) {
    if (!points || !v || !rgba_out || count < 0) return VR_EINVAL;
    vr::Colormap m;
    if (!vr::colormap_build(points, n, &m)) return VR_EINVAL;
    for (int64_t i = 0; i < count; ++i) vr::colormap_eval(m, v[i], rgba_out + 4 * i);
    return VR_OK;
}
