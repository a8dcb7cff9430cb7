// vr_device.h -- shared host/device structures of the HIP ray marcher (internal, not the ABI).
#pragma once
#include <stdint.h>

namespace vr {

// Workgroup = 256 lanes = 16 x 16 rays; each wave64 covers an 8 x 8 ray block.
constexpr int kWgRaysX = 16;
constexpr int kWgRaysY = 16;
constexpr int kWgThreads = 256;
// march geometry variants; kGeomAxis1Run = kGeomAxis1 with the run-word class gathers (VrcFrame.zrun),
// kGeomAxis1Z = kGeomAxis1 along z with the split {byte, bit} view table (VrcFrame.tsplit)
constexpr int kGeomOrtho = 0, kGeomAxis1 = 1, kGeomConic = 2, kGeomAxis1Run = 3, kGeomAxis1Z = 4;
constexpr int kMaxTf = 256;
constexpr int kLeafColsMax = 2048;   // leaf-column masks (AXIS1 ESS) up to this many leaves per axis
constexpr int kBgGroup = 8;         // culled whole-frame work tiles stored per background-only workgroup
// the column path's expand pass (axis_expand_kernel): work tiles of the visible rectangle per workgroup,
// culled work tiles per background-only workgroup, and its lane -> pixel mapping inside a tile
// (0: ray_of_thread's 8 y per row, 1: 16).  -D knobs of the experiment builds only (tools/build_ab.sh)
#ifndef VR_EXPAND_GROUP
#define VR_EXPAND_GROUP 3
#endif
#ifndef VR_EXPAND_BG_GROUP
#define VR_EXPAND_BG_GROUP 8
#endif
#ifndef VR_EXPAND_ROW16
#define VR_EXPAND_ROW16 0
#endif
constexpr int kExpandGroup = VR_EXPAND_GROUP, kExpandBgGroup = VR_EXPAND_BG_GROUP, kExpandRow16 = VR_EXPAND_ROW16;
static_assert(kExpandGroup >= 1 && kExpandGroup <= 8 && kExpandBgGroup >= 1 && kExpandBgGroup <= 16,
              "the expand keeps a group's tiles and columns in registers");
constexpr int kCellDistCap = 16;  // cap of the ESS Chebyshev cell-distance field (relaxation steps)
constexpr int kMaxTabSamples = 8192;   // AXIS1 per-frame sample table (LDS) up to this many samples per ray
constexpr int kMaxTestTab = 4096;      // TEST general views: per-frame B table (16 B per entry, <= 64 KB LDS)
constexpr int kMaxHull = 8;         // edges of the projected dataset box's hull (workgroup cull)
// general views: a leaf outside the dataset is -2^29 in the staged leaf maps, so for class volumes
// under 2^29 units the sum of the three contributions is negative -- an out-of-range buffer offset --
// whenever one of them is outside
constexpr int32_t kMapOut = -(1 << 29);
// general 32-bit views: the leaf maps in global memory carry kMapPadMax kMapOut entries either side
// of each axis (pmaps_pad), so a frame's LDS maps with pad <= kMapPadMax are one contiguous copy
constexpr int kMapPadMax = 64;
// zero bytes after the TEST class volume: the corner-row dword gathers may read up to 3 bytes past
// the last voxel (class 0 there IS the reference's idx < total guard); the buffer bound is total +
// kClsPad / 4, so even an in-range dword at the bound stays inside the allocation
constexpr int kClsPad = 64;

// One workgroup's work tile: rays [x0, x0+16) x [y0, y0+16).  In tile-output mode `slot` is the
// compact user-tile slot and (tox, toy) the work tile's offset inside that user tile.
struct WorkTile {
    int32_t x0, y0, slot, tofs;   // tofs = (tox << 16) | toy
};

// worklist_kernel's occupancy cull of an axis-parallel orthographic whole frame (vr_api.cpp
// frame_list): a work tile all of whose rays' cell columns along the view axis are empty is exactly
// the background.  sat = the column table of that axis (occupied columns in [0, u) x [0, v), side x
// side), nullptr = no cull; the two fixed axes' top-left / right / up components in double.
struct WlCull {
    const int32_t* sat;
    int32_t side, cb_shift, nleaf, W, H;
    double tl[2], right[2], up[2];
    double rsw, rsh;
};

// The fused column march (vrc_march_kernel, FUSE): a workgroup owns a tile of P x Q pixels (multiples of
// 16), marches the leaf columns under it and stores its pixels.  The frame is ntx x nty such tiles, of
// which [rx0, rx0 + nrx) x [ry0, ry0 + nry) touch the visible rectangle of 16 x 16 work tiles [vtx0,
// vtx1) x [vty0, vty1) -- the rectangle whose work tiles have slot >= 0 in the two-kernel path's list,
// up to its occupancy cull -- and come first in block order; every other tile is the background.
struct FuseTiles {
    int32_t P, Q, ntx, nty, rx0, ry0, nrx, nry, vtx0, vtx1, vty0, vty1;
};
constexpr int kFuseCols = 256;      // leaf columns a tile may march: one per lane

// Per-frame constants of the VRC march, passed by value (kernarg segment -> SGPRs).
struct VrcFrame {
    // screen / camera (AppData fields, utils.h:36-74; camera after processInput)
    int32_t W, H, S, flags;
    float rsw, rsh, sd, fc;
    float tlc[3], right[3], up[3], front[3];
    float bg[4];
    float ert_eps;
    // volume (leaf grid of the implicit octree, Octree.cu:35-49)
    int64_t d2d3, d3;
    int32_t depth;          // D
    float leaves;           // 2^D
    int32_t cb_shift;       // macro cell = 2^cb_shift leaves per axis
    int32_t ncell;          // macro cells per axis
    float cell_q;           // macro cell edge in q units (2^cb_shift / 2^D)
    float shrink_q;         // ESS safety shrink, q units
    float step[3];          // q advance per sample = sd * front (per frame: rays are parallel)
    float inv_step[3];      // 1 / step (0 where step == 0)
    int32_t occ_words;      // 32-bit words of the occupancy bitmask
    int32_t occ_lds;        // bitmask staged in LDS
    int32_t axis1;          // index of the only non-zero component of front (axis-aligned view), else -1
    float box_lo[3], box_hi[3];   // dataset box in q space (+margin), for clipping
    int edge_guard;               // marched samples may leave the unit cube (ESS must not jump there)
    int conic;                    // VR_FLAG_CONIC: rays from campos through the screen point
    float campos[3];
    int32_t zero_transparent;     // TF(0).a == 0
    int32_t cls0;                 // class of TF(0 / (float)(int)cal_max): outside cube / dataset
    int32_t nleaf;                // 2^D (leaf-map length per axis)
    // output
    int32_t out_tiles;            // 0: frame [x*H+y]; 1: compact tiles
    int32_t out_rgb;              // compact tiles of 3 floats per pixel (VR_OUT_RGB)
    int32_t tile_w, tile_h;
    int32_t n_work;               // entries in the work list
    int32_t n_slots;              // entries in the block order (>= grid size)
    int32_t persist_wgs;          // > 0: persistent launch with this many workgroups per CU
    int32_t cls_bytes;            // class volume bytes when < 2^31 (buffer-resource bound of the gathers)
    // class addressing (32-bit volumes): offsets are bits when cbits < 8 -- the class is the cbits-wide
    // field at bit (o & omask) of byte o >> osh -- and bytes at 8 bits (osh = omask = 0)
    int32_t cbits, osh, omask;
    int32_t mapout_ok;            // offsets stay below 2^29 units: a kMapOut term makes any sum negative
    // AXIS1 run words (views along z): a batch's classes come from the two aligned 8-byte words that
    // hold its first and last samples; qsh = log2(units per word) (6 bits, 3 bytes), bsh = log2(bits
    // per unit) (0, 3).  0: one class load per sample
    int32_t zrun, qsh, bsh;
    int32_t zspan2;               // zrun: every batch spans at most two z-bricks (host bound on the step)
    int32_t tsplit;               // AXIS1 along z, 32-bit volume: view-table entries {byte offset, bit}
    int32_t c0_noop;              // TF class 0 has alpha 0: its premultiplied entry (0, 0, 0, 1) is a no-op
    int32_t bg_first;             // whole frames: first culled entry of the work list (n_work: none)
    int32_t bg_group;             // culled entries per background-only workgroup (blocks >= bg_first)
    int32_t pad;                  // general views: kMapOut entries either side of each LDS leaf map (0: none)
    int32_t leafcols;             // AXIS1 + ESS: occcol holds leaf-column masks (3 nleaf^2), else cell-column masks
    // whole frames, general views: the projected dataset box's hull, edge e keeping the pixels with
    // hull[e][0] x + hull[e][1] y <= hull[e][2] (vr_api.cpp hull_edges); 0 edges = no claim
    int32_t n_hull;
    union {
        float hull[kMaxHull][3];
        FuseTiles fuse;           // the fused column march's frames (axis views: n_hull = 0, no hull)
    };
    // shading (VR_FLAG_SHADE)
    float ka, kd, ks, shininess;
    int32_t d1i, d2i, d3i;        // dims as int for gradient clamping
    // AXIS1 column path (vr_api.cpp axis_columns_plan): the leaf-column rectangle [col_i0, col_i0 +
    // col_n0) x [col_i1, col_i1 + col_n1) of the two fixed axes (ascending).  The column march runs
    // over it as a col_n0 x col_n1 "frame" (W = col_n0, H = col_n1: one lane per leaf column) into the
    // column buffer, which axis_expand_kernel then copies to the pixels
    int32_t col_i0, col_i1, col_n0, col_n1;
    int64_t col_ofs;              // column marches: the frame's first float4 in the launch's column buffer
};

// The frames whose column marches share one launch (vrc_march_kernel, COLS: grid y = frame), passed by
// value: with the march's other arguments it stays under the 4 KB a kernel's arguments may take
constexpr int kColBatch = 6;
struct ColBatch {
    VrcFrame f[kColBatch];
};
static_assert(sizeof(ColBatch) + 256 <= 4096, "ColBatch must fit the kernel argument segment");
// The frames of one launch when the march reads them from an array in device memory (vrc_march_kernel,
// DEVF): nothing but the grid's y extent bounds it; a call beyond it takes one more launch
constexpr int kColFrames = 32;

// Per-frame constants of the TEST march (kernel.cu:72-187).
struct TestFrame {
    int32_t W, H, S, flags;
    float mc[16], iv[16], tv[16];   // modelCam, inverse(lookAt), toVolume; column-major
    float bg[4];
    float ert_eps;
    float rS;                       // VR_FLAG_PERSP: 1.0f / (float)S, t(s) = fs * rS (in the padding ahead of d1:
                                    // no other field's offset moves); 0 otherwise
    int64_t d1, d2, d3, total;
    float fd1, fd2, fd3;
    int32_t zero_transparent;
    int32_t cls0;                   // class of TF(0 / cal_max)
    int32_t out_tiles, tile_w, tile_h, n_work;
    int32_t out_rgb;                // compact tiles of 3 floats per pixel (VR_OUT_RGB)
    int32_t idx64;                  // 64-bit corner indices (total + d2*d3 + d3 >= 2^31)
    int32_t tcb, tnc[3];            // ESS macro cells: 2^tcb voxels per axis, cells per axis
    int32_t occ_words, occ_lds;
    int32_t sep;                    // mc and tv are axis-separable (scale + translate): see test_march_kernel;
                                    // the field marches' position law (vr_march.h kLawGeneral / kLawSep / kLawPersp):
                                    // 2 under VR_FLAG_PERSP, whatever the matrices hold
    int32_t sep_tab;                // sep + the per-frame B table fits its LDS budget (S + 8 <= kMaxTestTab)
    int32_t axt;                    // -1, or the volume axis a along which the rays march with the other two
                                    // coordinates of p fixed (test_axis_kernel; make_test's conditions)
    int32_t axt_up;                 // p_a grows with s (tv_aa * iv_{8+a} * mc10 > 0)
    int32_t ax_sb, ax_se;           // axis views: the clip range [ax_sb, ax_se) of every ray whose (p_b, p_c)
                                    // lies in the volume -- p_a(s) is the same for every ray (make_test)
    // axis views: per corner line (the two other coordinates, each in [0, d + 2)) a 64-bit mask over
    // cells of tca[a] voxels along a (tnca[a] <= 64 cells): bit c = a byte of the line's flat
    // indices at a in [c tca, c tca + tca + 1] (the corners a sample whose (int)p_a lies in cell c
    // reads) has alpha > 0 (test_columns_kernel); line (u, v) at tcol_base[a] + u tcol_pitch[a] + v
    int32_t tca[3], tnca[3], tcol_pitch[3];
    int64_t tcol_base[3];
    int32_t cv;                     // the general march's corner volume (test_corner_kernel): 0 none; CB = 2 / 4 / 8
                                    // bits per corner class in 4^3-voxel bricks, 16 + CB x-major
    int32_t cv_bytes;               // its bytes (< 2^31: the gathers' buffer bound)
    int32_t mul24;                  // d1 and d2 d3 < 2^24: x-major corner offsets in 24-bit multiplies
    float wthr[3];                  // 1 - ulp(d_a + 1): a fraction below it has (int)(p + 1) == (int)p + 1
    int32_t lin;                    // every voxel on the volume's six faces is class 0: the general march's
                                    // trilinear colour is continuous across the faces (test_faces_kernel)
    int32_t bg_first;               // whole frames: first background-only workgroup (INT32_MAX: none)
    int32_t bg_group;               // culled work tiles per background-only workgroup
    int32_t n_hull;                 // general views: the projected dataset box's hull (VrcFrame.hull)
    float hull[kMaxHull][3];
};

// The DVR march (vr_dvr.hip) takes its positions, clip, work list, cull and output from a TestFrame
// (tcb / tnc / occ_words / occ_lds describing its own min/max cells) and adds the classification:
// the TF as segments of the ordered floats (vr_tf_segments), segment j = [start[j], start[j + 1]).
constexpr int kDvrSeg8 = 8;                  // up to 1 + 8 segments: the starts past -inf in SGPRs
constexpr int kMaxDvrSeg = 2 * kMaxTf + 1;   // segments of a TF of kMaxTf intervals
constexpr int kDvrPad = 64;                  // zero bytes after the byte copy of the volume (dword gathers)
constexpr int kDvrLdsMax = 64 * 1024;        // LDS budget of a DVR workgroup (tables staged only within it)
struct DvrFrame {
    int32_t nseg;               // segments
    int32_t seg0;               // the segment of the value 0: a sample outside the volume
    int32_t vol_bytes;          // bytes of the array the corner gathers read (their buffer bound)
    int32_t reserved;
    float start[kDvrSeg8];      // nseg <= 9: start[1 .. nseg), the rest NaN (no value is >= NaN)
};

// The MIP march (vr_mip.hip) takes the same from a TestFrame (zero_transparent = 1: a sample outside
// the volume takes no part whatever the TF is; tcb / tnc describing the min/max cells) and adds:
struct MipFrame {
    double cal_max;             // the pixel is (float)((double)max / cal_max), clamped to [0, 1]
    float vol_bound;            // the largest cell bound: no sample exceeds it (the ERT stop)
    int32_t vol_bytes;          // bytes of the array the corner gathers read (their buffer bound)
    int32_t bound_bytes;        // bytes of the cells' upper bounds (one float per cell)
    int32_t reserved;
};

// The ISO march (vr_iso.hip) takes the same from a TestFrame as the MIP march, reads MIP's cell bounds
// against a fixed threshold, and adds -- by value per launch, so vr_set_isosurface between queued
// frames needs no synchronisation:
constexpr int kIsoRefine = 6;   // bisection rounds (VR_ISO_REFINE)
struct IsoFrame {
    float iso;                  // the isovalue, in voxel units
    float rgb[3];               // the surface colour
    float ka, kd, ks, shininess;   // vr_params.shade_*
    int32_t vol_bytes;          // bytes of the array the corner gathers read (their buffer bound)
    int32_t bound_bytes;        // bytes of the cells' upper bounds (one float per cell)
};

// The SDVR march (dvr_march_kernel's SHADE variants, vr_dvr.hip) takes DVR's TestFrame and DvrFrame
// unchanged and adds the Phong coefficients, by value per launch like IsoFrame's:
struct SdvrFrame {
    float ka, kd, ks, shininess;   // vr_params.shade_*
};

// The CDVR march (vr_cmap.hip) takes DVR's TestFrame (zero_transparent = C(0.0f).a == 0, the cells
// those of its own bitmask) and adds the colour map: n points, their (x, inv) and colours in device
// tables (host/colormap.h), C(0.0f) by value, and for a small map the x as wave-uniform arguments.
constexpr int kCmapSmall = 8;                // up to 8 points: the span index is a sum of compares
constexpr int kMaxCmap = 256;                // VR_CMAP_MAX_POINTS (one point per lane of a workgroup)
struct CmapFrame {
    int32_t n;                  // points
    int32_t vol_bytes;          // bytes of the array the corner gathers read (their buffer bound)
    float c0[4];                // C(0.0f): a sample outside the volume
    float x[kCmapSmall];        // n <= kCmapSmall: x[0 .. n), the rest NaN (no value is >= NaN)
};

// The SCDVR march (cmap_march_kernel's SHADE variants, vr_cmap.hip) takes CDVR's TestFrame, CmapFrame and
// device tables unchanged and adds, by value per launch like IsoFrame's (so vr_set_gradient_opacity between queued frames needs no
// synchronisation): the Phong coefficients and the gradient-opacity map G (host/colormap.h).  The
// march counts the m_i <= mag against the wave-uniform m and reads point max(j - 1, 0) from a
// 16-entry LDS table {m_i, inv_i, w_i, w_{min(i + 1, n - 1)}} staged from these arguments.
constexpr int kMaxGopa = 16;                 // VR_GOPA_MAX_POINTS
constexpr int kGopaLds = kMaxGopa * 16;      // bytes of that table, ahead of CDVR's carve-up
struct ScdvrFrame {
    float ka, kd, ks, shininess;   // vr_params.shade_*
    int32_t n;                  // points of G
    float m[kMaxGopa];          // m[0 .. n), the rest NaN (no magnitude is >= NaN)
    float inv[kMaxGopa];        // inv[i] = 1.0f / (m[i + 1] - m[i]), 0 from n - 1 on (never used)
    float w[kMaxGopa];          // w[0 .. n), the rest w[n - 1]
};

// The crop box of the six field marches (vr_set_crop_box; their CROP instantiations read it, the others
// ignore it), by value per launch like IsoFrame's values -- its own kernel argument, the last one, so
// TestFrame and every argument offset of the CROP = false instantiations stay as they were.  The
// effective box E = [max(lo, 0), min(hi, d)) per axis: "in the volume and in the box" is then
// lo <= p < hi alone.  hi > 0 on every axis, or -- E empty on some axis -- lo = hi = +0 on all three,
// which no position satisfies (the upper test is the unsigned compare of the bits, the lower p >= lo).
struct CropBox {
    float lo[3], hi[3];
};

// TransferFunction::getMaterial (TransferFunction.cu:46-55): last closed interval containing v, else 0
__device__ __forceinline__ int tf_class(const float* lo, const float* hi, int n, float v) {
    int r = 0;
    for (int i = 0; i < n; ++i)
        if (v >= lo[i] && v <= hi[i]) r = i;
    return r;
}

}  // namespace vr
