// colormap.h -- VR_MODE_CDVR's classification law on the host: the piecewise-linear RGBA colour map
// C(v) of include/vr_api.h.  One validation and one table (the points' x, the spans' inv, the
// colours) for vr_set_colormap, vr_colormap_eval, the march's device tables and the cells' rule.
// Beside it VR_MODE_SCDVR's gradient-opacity map G(mag): the same law with one channel and at most
// VR_GOPA_MAX_POINTS points, for vr_set_gradient_opacity, vr_gradient_opacity_eval and the march's
// per-launch arguments.
#pragma once
#include <cstdint>
#include <vector>

#include "../../../include/vr_api.h"

namespace vr {

struct Colormap {
    int n = 0;
    std::vector<float> x;      // n, strictly ascending
    std::vector<float> inv;    // n: inv[i] = 1.0f / (x[i + 1] - x[i]), the last one 0 (never read)
    std::vector<float> rgba;   // 4 n
};

// Rule 6's checks (n in range, finite x and colours, alpha in [0, 1], x strictly ascending, finite
// inv); false leaves *out unspecified.  points must not be null.
bool colormap_build(const vr_cmap_point* points, int32_t n, Colormap* out);

// Rule 2: float32, every operation rounded on its own.
void colormap_eval(const Colormap& m, float v, float out[4]);

// G as the law and the march read it: fixed arrays that go into the kernel arguments as they are.
struct Gopa {
    int n = 0;
    float m[VR_GOPA_MAX_POINTS];     // m[0 .. n) strictly ascending, the rest NaN (no magnitude is >= NaN)
    float inv[VR_GOPA_MAX_POINTS];   // inv[i] = 1.0f / (m[i + 1] - m[i]), 0 from n - 1 on (never read)
    float w[VR_GOPA_MAX_POINTS];     // w[0 .. n), the rest w[n - 1]
};

// The checks of vr_set_gradient_opacity (n in range, finite m and w, w in [0, 1], m strictly ascending,
// finite inv); false leaves *out unspecified.  points must not be null.
bool gopa_build(const vr_gopa_point* points, int32_t n, Gopa* out);

// VR_MODE_SCDVR's rule 4: float32, every operation rounded on its own.
float gopa_eval(const Gopa& g, float mag);

}  // namespace vr
