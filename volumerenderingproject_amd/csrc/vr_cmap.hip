// vr_cmap.hip -- VR_MODE_CDVR for gfx950: VR_MODE_DVR's trilinear sample of the scalar field
// classified by a piecewise-linear RGBA colour map (include/vr_api.h, host/colormap.h) instead of
// the interval transfer function, and the empty-cell bits that follow that map; VR_MODE_SCDVR is the
// same march with every non-transparent in-volume sample lit and its alpha scaled by the
// gradient-opacity map G (the kernel's SHADE flag).  Its own translation unit and its own kernel (the
// classification differs from DVR's and neither contains the other); the ray set-up, the inside test,
// the trilinear sample, the gradient and the headlight are vr_march.h's, shared with DVR, MIP and ISO.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "vr_device.h"
#include "vr_march.h"

#pragma clang fp contract(off)

namespace vr {

// ------------------------------------------------------------------------------------------------
// CDVR march, one launch per frame, the shape of dvr_march_kernel: 16 x 16 rays per workgroup, work
// list / background workgroups / hull cull (test_background), TEST's position chain with its
// per-frame B table in LDS, its linear-model clip and its macro-cell jumps, batches of K = 4 samples
// whose positions and gathers are all issued before any is used; the byte path (four unaligned
// dword gathers) and the float path (eight gathers, a non-finite voxel reads as 0).
//
// Per sample, after the value v: j = the number of points x_i <= v; the two colours a = rgba[ja],
// b = rgba[jb] with ja = max(j - 1, 0), jb = min(j, n - 1), and (x, inv) of point ja, all from the
// per-workgroup LDS tables; u = min((v - x) * inv, 1) and the four unfused lerps a (1 - u) + b u.
// Below the first point and from the last one on ja == jb, and the colour is a itself: a select on
// the lerps' results, no branch (the u of such a sample is never used).
//
// SMALL: at most kCmapSmall points: the x are wave-uniform kernel arguments (SGPRs) and j is the sum
// of kCmapSmall compares (unused x are NaN: never <= v).  Otherwise a branch-free binary search
// over the x staged in LDS (kMaxCmap = 256 = 2^8: 9 steps).
//
// ESS: cells of 2^tcb voxels per axis whose bit in gocc is clear hold no sample with alpha != 0
// (cmap_cells_kernel); skipping them leaves either blend unchanged bit for bit.
//
// SHADE (VR_MODE_SCDVR; h is read by these instantiations only): dvr_march_kernel's SHADE -- the
// headlight per ray, and per sample, once its colour C(v) is known, six more single samples of the
// field (field_gradient) around the position of a sample in the volume with alpha != 0, the tap loop
// rolled -- and from the central differences len2, mag = sqrtf(len2), the weight G(mag) that scales
// the sample's alpha and, with len2 > 0 and a light, the normal that goes through shade_normal.  A
// wave none of whose lanes lights the sample skips all of it.
//
// G(mag): j = the number of m_i <= mag, a sum of kMaxGopa compares against the wave-uniform m (the
// unused ones NaN: never <= mag; a NaN mag: 0); the point max(j - 1, 0) as {m, inv, w, w of the next
// point} in one 16-byte LDS read from the table at the head of LDS (kGopaLds bytes, ahead of the
// carve-up above) that the workgroup's first lane stages from the kernel arguments; flat tails
// (j == 0, j == n) give that point's w itself, otherwise the unfused lerp at
// u = min((mag - m) * inv, 1) -- the law of the colour map with one channel.
//
// An alpha-0 sample is neither lit nor scaled: it stays the exact no-op of both blends that the
// empty-cell skip (ESS, over CDVR's own cell bits) and the blank-batch skip rely on.  (No
// amdgpu_waves_per_eu cap: profiles/scdvr/resource_usage.txt -- every instantiation fits without
// scratch left to itself.)
//
// CROP (vr_set_crop_box; bx is read by these instantiations only): dvr_march_kernel's CROP -- the
// effective box in the volume's place in in[k] and in the ESS first-sample test (field_inside), crop_clip
// for the ray range; a sample not in the box is C(0.0f), neither lit nor scaled.
// ------------------------------------------------------------------------------------------------
constexpr int kCmapK = 4;

template <bool F2B, bool ESS, bool U8, bool SMALL, int LAW, bool SHADE, bool CROP>
__global__ __launch_bounds__(256) void cmap_march_kernel(TestFrame f, CmapFrame g, ScdvrFrame h,
                                                         const WorkTile* __restrict__ work,
                                                         const void* __restrict__ vol,
                                                         const float2* __restrict__ gxi,
                                                         const float4* __restrict__ gcol,
                                                         const uint32_t* __restrict__ gocc,
                                                         float4* __restrict__ out, CropBox bx) {
    constexpr int K = kCmapK;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_all[];
    // LDS: G's points (SHADE) | the points' colours | their (x, inv) | the cell bits (ESS) | the B
    // table (SEP, PERSP)
    float4* s_G = reinterpret_cast<float4*>(smem_all);
    unsigned char* smem = smem_all + (SHADE ? kGopaLds : 0);
    float4* s_col = reinterpret_cast<float4*>(smem);
    float2* s_xi = reinterpret_cast<float2*>(smem + (size_t)g.n * sizeof(float4));
    const bool occ_st = ESS && f.occ_lds;
    const size_t o_occ = (size_t)g.n * sizeof(float4) + ((size_t)g.n * sizeof(float2) + 15) / 16 * 16;
    uint32_t* s_occ = reinterpret_cast<uint32_t*>(smem + o_occ);
    float4* s_B = reinterpret_cast<float4*>(smem + o_occ + ((occ_st ? (size_t)f.occ_words * 4 : 0) + 15) / 16 * 16);
    // first round of loads, unconditional (index clamped, value selected): one point (n <= kMaxCmap =
    // kWgThreads) and 4 cell words per lane and the work tile; a culled work tile (or a
    // background-only workgroup) stores the background and leaves before any staging
    const int ip = (int)threadIdx.x < g.n ? (int)threadIdx.x : 0;
    const float4 cv = gcol[ip];
    const float2 xv = gxi[ip];
    asm volatile("" ::"s"(f.out_tiles), "s"(f.bg_first), "s"(f.n_work), "s"(f.n_hull), "s"(f.W), "s"(f.H));
    uint32_t ov[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int i = (int)threadIdx.x + u * kWgThreads;
        const bool io = occ_st && i < f.occ_words;
        ov[u] = 0u;
        if (ESS) { const uint32_t w = gocc[io ? i : 0]; ov[u] = io ? w : 0u; }
    }
    const int b = (int)blockIdx.x;
    const WorkTile wt = work[b < f.n_work ? b : 0];
    if (b >= f.n_work) return;
    if (test_background(f, work, wt, out)) return;
    if ((int)threadIdx.x < g.n) {
        s_col[threadIdx.x] = cv;
        s_xi[threadIdx.x] = xv;
    }
    // G's table from the kernel arguments: constant indices only (a lane-indexed read of a by-value
    // struct would go through scratch), so one lane stores the 16 entries
    if (SHADE && threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < kMaxGopa; ++i)
            s_G[i] = make_float4(h.m[i], h.inv[i], h.w[i], h.w[i + 1 < kMaxGopa ? i + 1 : i]);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int i = (int)threadIdx.x + u * kWgThreads;
        if (occ_st && i < f.occ_words) s_occ[i] = ov[u];
    }
    if (occ_st)
        for (int i = threadIdx.x + 4 * kWgThreads; i < f.occ_words; i += kWgThreads) s_occ[i] = gocc[i];
    if (LAW != kLawGeneral && f.sep_tab) test_stage_B<LAW>(f, s_B, K);
    __syncthreads();
    const __amdgpu_buffer_rsrc_t ors = uniform_rsrc(gocc, ESS ? f.occ_words * 4 : 0);
    auto occ_word = [&](int wi) -> uint32_t {
        if (f.occ_lds) return s_occ[wi];
        return __builtin_amdgcn_raw_buffer_load_b32(ors, wi * 4, 0, 0);
    };
    // the ERT threshold pinned in a VGPR (test_march_kernel)
    float ert_eps = f.ert_eps;
    asm volatile("" : "+v"(ert_eps));
    int x, y;
    ray_of_thread(wt, x, y);
    if (x >= f.W || y >= f.H) return;

    // the ray: TEST's position chain, clip and linear model; SHADE: the headlight from its two end points
    FieldRay<LAW> R;
    int s_begin, s_end;
    float L[3] = {0.0f, 0.0f, 0.0f};
    bool lit = false;   // SHADE: the ray has a light direction
    {
        float pb[3];
        field_ray_init<LAW, CROP>(f, bx, x, y, s_B, K, R, pb, s_begin, s_end);
        if (SHADE) lit = headlight(R.pa, pb, L);
    }

    const float4 c0 = make_float4(g.c0[0], g.c0[1], g.c0[2], g.c0[3]);
    const int nl = g.n - 1;
    const FieldGrid fv = field_grid(f, vol, g.vol_bytes);
    float r, gr, bl, T = 1.0f;
    if (F2B) { r = 0.0f; gr = 0.0f; bl = 0.0f; }
    else { r = f.bg[0]; gr = f.bg[1]; bl = f.bg[2]; }

    int s = F2B ? s_begin : s_end - 1;
    bool done = F2B ? (s >= s_end) : (s < s_begin);
    float pfirst[3];   // ESS: the position of the batch's first sample, from the empty-cell test
    while (!done) {
        if (ESS) {
            R.position(f, s, pfirst);
            const bool inside = field_inside<CROP>(f, bx, pfirst[0], pfirst[1], pfirst[2]);
            int cc[3];
            const int cell = field_cell(f, inside, pfirst, cc);
            if (inside && !((occ_word(cell >> 5) >> (cell & 31)) & 1u)) {
                test_cell_jump<F2B>(f, cc, R.pa, R.dp, R.idp, s_begin, s_end, s, done);
                continue;
            }
        }
        // the batch: every position and every gather issued before any is used
        FieldCorners cs[K];
        FieldRawA<U8> raw[K];
        bool in[K];
        bool any_in = false;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int sk = F2B ? s + k : s - k;
            const bool valid = F2B ? (sk < s_end) : (sk >= s_begin);
            float p[3];
            if (ESS && k == 0) {   // (s did not move since the empty-cell test: the same position)
                p[0] = pfirst[0]; p[1] = pfirst[1]; p[2] = pfirst[2];
            } else {
                R.position(f, sk, p);
            }
            in[k] = field_inside<CROP>(f, bx, p[0], p[1], p[2], valid);
            any_in |= in[k];
            // (field_corners' statements with the three conversions ahead of the fractions, not the call: through
            // the call <F2B, ESS, float, SMALL, general law, no SHADE, no CROP> takes 97 VGPRs for 96 and goes from
            // 5 waves per SIMD to 4)
            const int i0[3] = {(int)p[0], (int)p[1], (int)p[2]};
#pragma unroll
            for (int a = 0; a < 3; ++a) cs[k].w[a] = __builtin_amdgcn_fractf(p[a]);
            const int base = i0[0] * fv.d23 + i0[1] * fv.d3 + i0[2];
            const int ox = i0[0] >= fv.xl ? 0 : fv.d23, oy = i0[1] >= fv.yl ? 0 : fv.d3;
            cs[k].off[0] = base;
            cs[k].off[1] = base + oy;
            cs[k].off[2] = base + ox;
            cs[k].off[3] = base + ox + oy;
            cs[k].lastz = i0[2] >= fv.zl;
        }
#pragma unroll
        for (int k = 0; k < K; ++k) raw[k] = field_gather<U8, FieldRawA<U8>>(fv, in[k], cs[k]);
        // a batch with every lane's samples outside the volume composites C(0) only: with C(0)
        // transparent an exact no-op of either blend (f * (1 - 0) + c * 0 = f, T * (1 - 0) = T)
        const bool blank = f.zero_transparent && !__any(any_in);
        if (!blank) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const float v = field_value<U8>(raw[k], cs[k]);
                int j = 0;   // the points x_i <= v (a NaN: none)
                if (SMALL) {
#pragma unroll
                    for (int i = 0; i < kCmapSmall; ++i) j += (int)(v >= g.x[i]);
                } else {
#pragma unroll
                    for (int step = kMaxCmap; step >= 1; step >>= 1) {
                        const int np = j + step;
                        const float xs = s_xi[min(np, g.n) - 1].x;
                        j = (np <= g.n && v >= xs) ? np : j;
                    }
                }
                const int ja = max(j - 1, 0), jb = min(j, nl);
                const float2 xi = s_xi[ja];
                const float4 ca = s_col[ja], cb = s_col[jb];
                const float u = fminf((v - xi.x) * xi.y, 1.0f);
                const float u1 = 1.0f - u;
                const bool flat = ja == jb;   // below x_0, or from x_{n-1} on: the end colour itself
                float4 cs;
                cs.x = flat ? ca.x : ca.x * u1 + cb.x * u;
                cs.y = flat ? ca.y : ca.y * u1 + cb.y * u;
                cs.z = flat ? ca.z : ca.z * u1 + cb.z * u;
                cs.w = flat ? ca.w : ca.w * u1 + cb.w * u;
                float4 cf = in[k] ? cs : c0;
                const int sk = F2B ? s + k : s - k;
                // SHADE: the lit samples: in the volume (in[k] holds the range test too) with alpha != 0
                const bool sh = SHADE && in[k] && cf.w != 0.0f;
                if (SHADE && __any(sh)) {
                    float ps[3];
                    R.position(f, sk, ps);   // (the batch kept the sample's fractions only: the same position again)
                    // the gradient of the trilinear field at p (six taps, all in the volume for a lane that lights)
                    float gx, gy, gz;
                    field_gradient<U8>(sh, ps[0], ps[1], ps[2], fv, gx, gy, gz);
                    const float len2 = (gx * gx + gy * gy) + gz * gz;
                    const float mag = sqrtf(len2);
                    // gradient opacity G(mag), with or without a normal
                    // (CROP without SEP: the three matrices, G and the box together passed the scalar registers
                    // by enough to leave two instantiations a stack slot; there the m_i are read from the LDS
                    // table -- the same floats -- and the 16 SGPRs go to the rest)
                    int jg = 0;   // the points m_i <= mag (a NaN: none)
#pragma unroll
                    for (int i = 0; i < kMaxGopa; ++i) jg += (int)(mag >= ((CROP && LAW == kLawGeneral) ? s_G[i].x : h.m[i]));
                    const float4 ge = s_G[max(jg - 1, 0)];
                    const float ug = fminf((mag - ge.x) * ge.y, 1.0f);
                    const float ug1 = 1.0f - ug;
                    const float gw = (jg == 0 || jg == h.n) ? ge.z : ge.z * ug1 + ge.w * ug;
                    float4 nv = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    if (lit && len2 > 0.0f) {   // (without a light direction: d = 1, spec = 0, as without a normal)
                        const float inv = 1.0f / mag;
                        nv = make_float4(-gx * inv, -gy * inv, -gz * inv, 1.0f);
                        // two-sided: a normal facing away from the light is negated (exact), so the law's own
                        // dot product is -ndl
                        const float ndl = (nv.x * L[0] + nv.y * L[1]) + nv.z * L[2];
                        if (ndl < 0.0f) { nv.x = -nv.x; nv.y = -nv.y; nv.z = -nv.z; }
                    }
                    float cr = cf.x, cg = cf.y, cb_ = cf.z;
                    shade_normal(nv, L, h.ka, h.kd, h.ks, h.shininess, cr, cg, cb_);
                    cf.x = sh ? cr : cf.x;
                    cf.y = sh ? cg : cf.y;
                    cf.z = sh ? cb_ : cf.z;
                    cf.w = sh ? cf.w * gw : cf.w;
                }
                const float a = (F2B ? (sk < s_end) : (sk >= s_begin)) ? cf.w : 0.0f;
                if (F2B) {
                    const float wt_ = T * a;
                    r = fmaf(wt_, cf.x, r); gr = fmaf(wt_, cf.y, gr); bl = fmaf(wt_, cf.z, bl);
                    T = T * (1.0f - a);
                } else {
                    r = r * (1 - a) + cf.x * a;
                    gr = gr * (1 - a) + cf.y * a;
                    bl = bl * (1 - a) + cf.z * a;
                }
            }
        }
        if (F2B && T < ert_eps) done = true;
        s = F2B ? s + K : s - K;
        if (F2B ? (s >= s_end) : (s < s_begin)) done = true;
    }
    if (F2B) { r = r + T * f.bg[0]; gr = gr + T * f.bg[1]; bl = bl + T * f.bg[2]; }
    store_pixel(out, out_index(f.out_tiles, wt, x, y, f.H, f.tile_w, f.tile_h), f.out_rgb, r, gr, bl);
}

// ------------------------------------------------------------------------------------------------
// Cell bits of the colour map, over dvr_minmax_kernel's cells (rebuilt on every vr_set_colormap): a
// cell is empty (bit clear) iff every piece of the map meeting [min - m, max + m] is transparent,
// m = 2^-20 max(|min|, |max|) (the margin derived at dvr_cells_kernel: the unfused three-level lerp
// of values in [min, max] ends within 6 ulps of that range).  The pieces: the lower tail
// (-inf, x_0) with alpha_0, the spans [x_i, x_{i+1}) with both end alphas, the upper tail
// [x_{n-1}, +inf) with alpha_{n-1}.  A value in a span with both end alphas 0 has alpha
// 0 (1 - u) + 0 u = 0 exactly, whatever u in [0, 1] is.  A widened range that is not finite keeps
// the cell.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cmap_cells_kernel(const float2* __restrict__ mm, int64_t ncells,
                                                         const float2* __restrict__ xi,
                                                         const float4* __restrict__ col, int n,
                                                         unsigned long long* __restrict__ occ) {
    const int64_t cell = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool occupied = false;
    if (cell < ncells) {
        const float2 r = mm[cell];
        const float m = fmaxf(fabsf(r.x), fabsf(r.y)) * 9.5367431640625e-07f;   // 2^-20
        const float lo = r.x - m, hi = r.y + m;
        const bool finite = (__float_as_uint(lo) & 0x7f800000u) != 0x7f800000u &&
                            (__float_as_uint(hi) & 0x7f800000u) != 0x7f800000u;
        occupied = !finite;
        occupied = occupied || (lo < xi[0].x && col[0].w != 0.0f);
        occupied = occupied || (hi >= xi[n - 1].x && col[n - 1].w != 0.0f);
        for (int i = 0; i + 1 < n; ++i) {
            const bool meets = xi[i].x <= hi && xi[i + 1].x > lo;
            occupied = occupied || (meets && (col[i].w != 0.0f || col[i + 1].w != 0.0f));
        }
    }
    const unsigned long long mask = __ballot(occupied);
    if ((threadIdx.x & 63) == 0 && cell < ncells) occ[cell >> 6] = mask;
}

// ------------------------------------------------------------------------------------------------
// Launch wrappers (called from vr_api.cpp)
// ------------------------------------------------------------------------------------------------

// LDS bytes of a CDVR workgroup, or with shade an SCDVR one (host: DVR's budget logic -- the B table
// is dropped, then the cell bits, when the sum would pass kDvrLdsMax)
size_t cmap_lds_bytes(const TestFrame& f, const CmapFrame& g, bool ess, bool shade) {
    return (shade ? (size_t)kGopaLds : 0) + (size_t)g.n * sizeof(float4) +
           ((size_t)g.n * sizeof(float2) + 15) / 16 * 16 +
           (((ess && f.occ_lds) ? (size_t)f.occ_words * 4 : 0) + 15) / 16 * 16 +
           ((f.sep && f.sep_tab) ? (size_t)(f.S + 2 * kCmapK) * sizeof(float4) : 0);
}

// shade: the coefficients and G of an SCDVR frame, or null for a CDVR frame (whose kernels read none);
// crop: the effective crop box, or null with the box off (the CROP = false instantiations)
hipError_t launch_cmap_march(const TestFrame& f, const CmapFrame& g, const ScdvrFrame* shade, const WorkTile* work,
                             int n_blocks, const void* vol, bool u8, const float2* xi, const float4* col,
                             const uint32_t* occ, float4* out, hipStream_t st, const CropBox* crop) {
    const bool f2b = (f.flags & 2) != 0, ess = (f.flags & 1) != 0 && f.zero_transparent && occ != nullptr;
    const bool small = g.n <= kCmapSmall;
    const size_t lds = cmap_lds_bytes(f, g, ess, shade != nullptr);
    const ScdvrFrame h = shade ? *shade : ScdvrFrame{};
    const CropBox cb = crop ? *crop : CropBox{};
    with_flag(f2b, [&](auto F2B) { with_flag(ess, [&](auto ESS) { with_flag(small, [&](auto SMALL) {
        with_flag(shade != nullptr, [&](auto SHADE) {
            field_variant(u8, f.sep, crop != nullptr, [&](auto U8, auto LAW, auto CROP) {
                hipLaunchKernelGGL((cmap_march_kernel<decltype(F2B)::value, decltype(ESS)::value, decltype(U8)::value,
                                                      decltype(SMALL)::value, decltype(LAW)::value,
                                                      decltype(SHADE)::value, decltype(CROP)::value>),
                                   dim3(n_blocks), dim3(kWgThreads), lds, st, f, g, h, work, vol, xi, col, occ, out, cb);
            });
        });
    }); }); });
    return hipGetLastError();
}

hipError_t launch_cmap_cells(const float2* mm, int64_t ncells, const float2* xi, const float4* col, int n,
                             unsigned long long* occ, hipStream_t st) {
    hipLaunchKernelGGL(cmap_cells_kernel, dim3((unsigned)((ncells + 255) / 256)), dim3(256), 0, st, mm, ncells, xi, col,
                       n, occ);
    return hipGetLastError();
}

}  // namespace vr
