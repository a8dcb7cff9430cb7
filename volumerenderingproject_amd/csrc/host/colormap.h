// colormap.h -- VR_MODE_CDVR's classification law on the host: the piecewise-linear RGBA colour map
// C(v) of include/vr_api.h.  One validation and one table (the points' x, the spans' inv, the
// colours) for vr_set_colormap, vr_colormap_eval, the march's device tables and the cells' rule.
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

}  // namespace vr
