// colormap.cpp -- the colour map of VR_MODE_CDVR and the gradient-opacity map of VR_MODE_SCDVR on the
// host (colormap.h), vr_colormap_eval and vr_gradient_opacity_eval.
// Compiled without FP contraction (Makefile FPFLAGS): the device march (vr_cmap.hip, with and without SHADE)
// evaluates the same expressions from the same x / inv / value tables, so the two agree bit for bit.
#include "colormap.h"

#include <cmath>
#include <limits>

#pragma clang fp contract(off)

namespace vr {

namespace {

// The two maps' common law.  inv[i] = 1.0f / (x[i + 1] - x[i]) for the n - 1 spans; false when one is
// not finite (a span so narrow that 1 / w overflows).
bool spans_inv(const float* x, int n, float* inv) {
    for (int i = 0; i + 1 < n; ++i) {
        const float w = x[i + 1] - x[i];
        const float v = 1.0f / w;
        if (!std::isfinite(v)) return false;
        inv[i] = v;
    }
    return true;
}

// j = the number of points x_i <= v (a NaN: none); for 0 < j < n also u = min((v - x_{j-1}) * inv_{j-1}, 1)
int span_of(const float* x, const float* inv, int n, float v, float* u) {
    int j = 0;
    for (int i = 0; i < n; ++i) j += (x[i] <= v) ? 1 : 0;
    if (j != 0 && j != n) *u = std::fmin((v - x[j - 1]) * inv[j - 1], 1.0f);
    return j;
}

}  // namespace

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
    return spans_inv(out->x.data(), n, out->inv.data());
}

void colormap_eval(const Colormap& m, float v, float out[4]) {
    float u = 0.0f;
    const int j = span_of(m.x.data(), m.inv.data(), m.n, v, &u);
    if (j == 0 || j == m.n) {
        const float* c = &m.rgba[(size_t)(j == 0 ? 0 : m.n - 1) * 4];
        for (int k = 0; k < 4; ++k) out[k] = c[k];
        return;
    }
    const float* a = &m.rgba[(size_t)(j - 1) * 4];
    const float* b = &m.rgba[(size_t)j * 4];
    const float u1 = 1.0f - u;
    for (int k = 0; k < 4; ++k) out[k] = a[k] * u1 + b[k] * u;
}

bool gopa_build(const vr_gopa_point* points, int32_t n, Gopa* out) {
    if (n < 1 || n > VR_GOPA_MAX_POINTS) return false;
    out->n = n;
    for (int i = 0; i < VR_GOPA_MAX_POINTS; ++i) {
        out->m[i] = std::numeric_limits<float>::quiet_NaN();
        out->inv[i] = 0.0f;
    }
    for (int i = 0; i < n; ++i) {
        const vr_gopa_point& p = points[i];
        if (!std::isfinite(p.m) || !std::isfinite(p.w)) return false;
        if (!(p.w >= 0.0f && p.w <= 1.0f)) return false;
        if (i > 0 && !(points[i - 1].m < p.m)) return false;
        out->m[i] = p.m;
        out->w[i] = p.w;
    }
    for (int i = n; i < VR_GOPA_MAX_POINTS; ++i) out->w[i] = out->w[n - 1];
    return spans_inv(out->m, n, out->inv);
}

float gopa_eval(const Gopa& g, float mag) {
    float u = 0.0f;
    const int j = span_of(g.m, g.inv, g.n, mag, &u);
    if (j == 0 || j == g.n) return g.w[j == 0 ? 0 : g.n - 1];
    const float u1 = 1.0f - u;
    return g.w[j - 1] * u1 + g.w[j] * u;
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

extern "C" int vr_gradient_opacity_eval(const vr_gopa_point* points, int32_t n, const float* mag, int64_t count,
                                        float* w_out) {
    if (!points || !mag || !w_out || count < 0) return VR_EINVAL;
    vr::Gopa g;
    if (!vr::gopa_build(points, n, &g)) return VR_EINVAL;
    for (int64_t i = 0; i < count; ++i) w_out[i] = vr::gopa_eval(g, mag[i]);
    return VR_OK;
}
